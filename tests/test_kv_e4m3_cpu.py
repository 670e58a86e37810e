"""The kv="e4m3" cache format as msr3d_amd/llm/kv_cache.py states it in torch (torch_kv_quantize / torch_kv_dequantize):
per (slot, head) one power-of-two scale 2^e, e the smallest integer with amax 2^-e <= 448, stored as the byte e + 127,
and OCP e4m3 codes of x 2^-e.  CPU only: the statement is what the kernels are tested against on the GPU.

The error bound per element: a normal e4m3 number has 3 mantissa bits, so RNE is within 2^-4 relative; below the
smallest normal (2^-6) the codes are multiples of 2^-9, so RNE is within 2^-10 absolute -- times the scale 2^e."""
import pytest
import torch

from msr3d_amd.llm.kv_cache import torch_kv_dequantize, torch_kv_quantize


def _check(x):
    """x (..., H, D) bf16 -> codes, exps after every property of the statement has been asserted."""
    codes, exps = torch_kv_quantize(x)
    assert codes.dtype == torch.uint8 and exps.dtype == torch.uint8
    assert codes.shape == x.shape and exps.shape == x.shape[:-1]
    e = exps.to(torch.int32) - 127
    xf = x.float()
    amax = xf.abs().amax(-1)
    # e is THE smallest exponent that fits: amax 2^-e <= 448 < amax 2^-(e - 1), i.e. the scaled amax lies in (224, 448];
    # its CODE lies in [224, 448]: e4m3 has no number between 224 and 256, so a scaled amax of up to 240 rounds to 224
    vals = codes.view(torch.float8_e4m3fn).float()
    top = vals.abs().amax(-1)
    nz = amax > 0
    assert bool(((top[nz] >= 224) & (top[nz] <= 448)).all())
    assert bool((e[~nz] == 0).all()) and bool((codes[~nz] & 0x7f == 0).all())     # (+-0 keeps its sign)
    assert bool((torch.ldexp(amax, -e)[nz] <= 448).all()) and bool((torch.ldexp(amax, 1 - e)[nz] > 448).all())
    # one rounding of the exactly scaled value
    want = torch.ldexp(xf, -e[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes, want)
    # every dequantised value is a bf16 number, and the format is a fixed point of itself
    d = torch_kv_dequantize(codes, exps)
    assert d.dtype == torch.bfloat16
    exact = torch.ldexp(vals, e[..., None])
    assert torch.equal(d.float(), exact) and torch.equal(exact.bfloat16().float(), exact)
    # ... in VALUE always: rounding a rounded head changes nothing.  In codes and exponents too, except where the head's
    # largest code is 224 (a scaled amax in (224, 240] rounded down): 224 2^e = 448 2^(e - 1), so the second pass takes
    # the exponent below and every code moves up one binade, exactly
    c2, e2 = torch_kv_quantize(d)
    assert torch.equal(torch_kv_dequantize(c2, e2), d)
    moved = nz & (top == 224)
    assert torch.equal(c2[~moved], codes[~moved]) and torch.equal(e2[~moved], exps[~moved])
    assert torch.equal(e2[moved], exps[moved] - 1)
    # the error of one e4m3 rounding
    bound = torch.maximum(xf.abs() * 2.0 ** -4, torch.ldexp(torch.full_like(xf, 2.0 ** -10), e[..., None]))
    assert bool(((d.float() - xf).abs() <= bound).all())
    return codes, exps


@pytest.mark.parametrize("shape", [(5, 8, 64), (37, 4, 128)])
def test_random_heads_of_very_different_magnitudes(shape):
    gen = torch.Generator().manual_seed(shape[0])
    mag = torch.exp(2.0 * torch.randn(shape[:2], generator=gen))
    x = (mag[..., None] * torch.randn(shape, generator=gen)).bfloat16()
    _check(x)


def test_the_exponent_rule_at_its_edges():
    above_448 = torch.tensor(448.0).bfloat16().view(torch.int16) + 1          # the next bf16: 450
    above_448 = float(above_448.view(torch.bfloat16))
    assert above_448 == 450.0
    cases = [(448.0, 0), (above_448, 1), (224.0, -1), (1.0, -8), (2.0 ** -20, -28), (0.0, 0),
             (448.0 * 2.0 ** 7, 7), (above_448 * 2.0 ** -12, -11)]
    D = 64
    x = torch.zeros((len(cases), 1, D))
    gen = torch.Generator().manual_seed(7)
    for i, (amax, _) in enumerate(cases):
        x[i, 0] = amax * (torch.rand(D, generator=gen) * 1.9 - 0.95)
        x[i, 0, i % D] = -amax if i % 2 else amax                               # the amax itself, either sign
    x = x.bfloat16()
    assert torch.equal(x.float().abs().amax(-1)[:, 0], torch.tensor([c[0] for c in cases]))
    codes, exps = _check(x)
    assert (exps[:, 0].to(torch.int32) - 127).tolist() == [c[1] for c in cases]
    assert int((codes[5] & 0x7f).max()) == 0


def test_other_input_dtypes_and_leading_shapes_give_the_same_bytes():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((2, 3, 4, 64), generator=gen).bfloat16()
    c, e = torch_kv_quantize(x)
    c32, e32 = torch_kv_quantize(x.float())
    assert torch.equal(c, c32) and torch.equal(e, e32)
    c1, e1 = torch_kv_quantize(x[1, 2])
    assert torch.equal(c1, c[1, 2]) and torch.equal(e1, e[1, 2])


def test_the_exponent_is_clamped_so_that_both_scales_are_normal_floats():
    x = torch.zeros((1, 2, 64))
    x[0, 0, 3], x[0, 0, 9] = -(2.0 ** -120), 2.0 ** -123
    x[0, 1, 0] = 2.0 ** -130                                                    # a bf16 subnormal
    codes, exps = torch_kv_quantize(x.bfloat16())
    assert exps.tolist() == [[1, 1]]
    want = torch.ldexp(x, torch.tensor(126)).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes, want) and float(codes.view(torch.float8_e4m3fn).float()[0, 0, 3]) == -64.0
    assert torch.equal(torch_kv_dequantize(codes, exps).float()[0, 0], x[0, 0])
