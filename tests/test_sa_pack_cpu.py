"""The host side of the split set-abstraction kernels: pointnet2/fused.py packs a conv weight as three bf16 planes in
MFMA-fragment order and folds the eval-mode BatchNorm into an fp32 affine.  The layout is restated here index by index
(csrc/split_mma.h: PACK) and the planes are compared with a bf16 residual chain computed on the bit patterns.
"""
import numpy as np
import pytest
import torch

from msr3d_amd.pointnet2 import fused

N, K = 32, 64


def _layer(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(k, n, 1, bias=True)
    bn = torch.nn.BatchNorm2d(n).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        conv.bias.copy_(torch.randn(n, generator=g))
        bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(n, generator=g))
        bn.running_mean.copy_(torch.randn(n, generator=g))
        bn.running_var.copy_(torch.rand(n, generator=g) + 0.25)
    return conv, bn


def _rne_bf16(x):
    """float32 array -> the nearest bf16 (ties to even) as a float32 array, on the bit patterns."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _residual_chain(w):
    w0 = _rne_bf16(w)
    r1 = w - w0                     # exact in fp32: the residual of a 24-bit significand after its top 8 bits
    w1 = _rne_bf16(r1)
    w2 = _rne_bf16(r1 - w1)
    return w0, w1, w2


def _read_planes(packed, n, kp, kperm):
    """(3, n, kp) fp32 from the packed bf16 tensor: [kp/32 slabs][n/16 tiles][3 planes][64 lanes = 16 g + i][8]; position
    (g, e) of slab s holds column 32 s + 8 g + e of row 16 t + i, or, kperm, column 32 s + 16 (e >> 2) + 4 g + (e & 3)."""
    assert packed.dtype == torch.bfloat16 and packed.numel() == 3 * n * kp
    flat = packed.float().numpy()
    out = np.full((3, n, kp), np.nan, dtype=np.float32)
    nt = n // 16
    for s in range(kp // 32):
        for t in range(nt):
            for p in range(3):
                for g in range(4):
                    for i in range(16):
                        for e in range(8):
                            col = 32 * s + 16 * (e >> 2) + 4 * g + (e & 3) if kperm else 32 * s + 8 * g + e
                            out[p, 16 * t + i, col] = flat[((((s * nt + t) * 3 + p) * 64 + 16 * g + i) * 8) + e]
    assert not np.isnan(out).any()          # every element was written: the numbering is a permutation
    return out


def _check_planes(planes, w):
    """planes (3, n, kp) against the fp32 weight w (n, kp) they should split."""
    w0, w1, w2 = _residual_chain(w)
    assert np.array_equal(planes[0], w0) and np.array_equal(planes[1], w1) and np.array_equal(planes[2], w2)
    # three 8-bit significands cover the 24 bits of an fp32 significand: what is left is below 2^-24 |w|
    total = planes[0].astype(np.float64) + planes[1].astype(np.float64) + planes[2].astype(np.float64)
    assert (np.abs(total - w.astype(np.float64)) <= 2.0 ** -24 * np.abs(w.astype(np.float64))).all()


def _folded(conv, bn):
    """(scale, shift, |terms of shift|) of the eval-mode BN after the conv bias, in float64."""
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.double() - bn.running_mean.double() * scale + conv.bias.double() * scale
    mag = bn.bias.double().abs() + (bn.running_mean.double() * scale).abs() + (conv.bias.double() * scale).abs()
    return scale.detach().numpy(), shift.detach().numpy(), mag.detach().numpy()


def _check_affine(scale, shift, conv, bn):
    # fp32 evaluation: var + eps, rsqrt, one product for the scale (at most 4 roundings of 2^-24 relative); the shift
    # adds two products and two sums of terms that each carry the scale's error (8 roundings of the terms' magnitudes)
    s64, h64, mag = _folded(conv, bn)
    assert (np.abs(scale.astype(np.float64) - s64) <= 4 * 2.0 ** -24 * np.abs(s64)).all()
    assert (np.abs(shift.astype(np.float64) - h64) <= 8 * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("feat_first,kperm", [(False, False), (False, True), (True, False)])
def test_pack_layer_split(feat_first, kperm):
    conv, bn = _layer(N, K, seed=1)
    packed, affine = fused._pack_layer_split(conv, bn, K, feat_first=feat_first, kperm=kperm)
    w = conv.weight.detach().reshape(N, K).numpy()
    if feat_first:                  # the kernels' K order [features, xyz]; the module's is [xyz, features]
        w = np.concatenate([w[:, 3:], w[:, :3]], axis=1)
    _check_planes(_read_planes(packed, N, K, kperm), w)
    assert affine.dtype == torch.float32 and affine.numel() == 2 * N
    _check_affine(affine[:N].numpy(), affine[N:].numpy(), conv, bn)


def test_pack_layer_split_pads_k():
    conv, bn = _layer(N, 35, seed=2)
    packed, _ = fused._pack_layer_split(conv, bn, K, feat_first=False)
    w = np.zeros((N, K), dtype=np.float32)
    w[:, :35] = conv.weight.detach().reshape(N, 35).numpy()
    _check_planes(_read_planes(packed, N, K, False), w)


def test_pack_level2_first():
    conv, bn = _layer(N, 35, seed=3)        # [xyz (3), features (32)]
    packed, affine = fused._pack_level2_first(conv, bn)
    w = conv.weight.detach().reshape(N, 35).numpy()
    _check_planes(_read_planes(packed, N, 32, False), np.ascontiguousarray(w[:, 3:]))
    assert affine.dtype == torch.float32 and affine.numel() == 2 * N + 4 * N
    _check_affine(affine[:N].numpy(), affine[N:2 * N].numpy(), conv, bn)
    wxyz = affine[2 * N:].numpy().reshape(N, 4)          # the coordinate columns as fp32 rows (x, y, z, 0)
    assert np.array_equal(wxyz[:, :3], w[:, :3]) and (wxyz[:, 3] == 0).all()
