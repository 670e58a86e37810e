"""msr3d_attn_decode_shared (csrc/llm_decode.hip) alone: decode attention for B prompts of G rows whose prompt keys are
stored once per prompt and whose generated tails are stored per row.

1. BIT equality with msr3d_attn_decode on the materialised (B G, T + Ttail, H, D) cache and key padding, with the same
   number of splits: the two kernels state their arithmetic through the same device functions in the same order.
2. Independently of the old kernel, the same cases against a float64 statement of the attention at 4e-3 rel-L2, the
   bound tests/test_llm_decode_gpu.py puts on msr3d_attn_decode; rows without a visible key are exact zeros.
3. Invalid arguments are refused with -22 and no launch.

H = 8.  T puts the prompt / tail boundary off every multiple of a wave step (4 keys at D = 128, 8 at D = 64) and on
one (64); (B, G) covers one row, the five beams, a full workgroup of 8 rows and 9 rows (a second, partly idle, chunk).
The float64 reference of a (D, B, G, T) case is computed once per tail length and shared by both split settings."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
H, TTAIL = 8, 72
TAILS = (0, 1, 5, 70)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _L():
    from msr3d_amd import _lib as L
    return L


def _st():
    return _L().current_stream_ptr(torch.device("cuda"))


def _bf(*shape, gen):
    return torch.randn(*shape, generator=gen, device="cuda").to(torch.bfloat16)


def _case(B, G, T, D, gen, dead_prompt=None):
    """q (B G, H D); prompt planes (B, T, H, D) and keep (B, T); tail planes (B G, TTAIL, H, D), every row's different."""
    N = B * G
    q = _bf(N, H * D, gen=gen)
    kp, vp = _bf(B, T, H, D, gen=gen), _bf(B, T, H, D, gen=gen)
    kt, vt = _bf(N, TTAIL, H, D, gen=gen), _bf(N, TTAIL, H, D, gen=gen)
    keep = (torch.rand(B, T, generator=gen, device="cuda") >= 0.2).to(torch.uint8)
    keep[:, T - 1] = 1
    if dead_prompt is not None:
        keep[dead_prompt] = 0
    return q, kp, vp, keep, kt, vt


def _materialise(G, kp, vp, keep, kt, vt):
    """The rows layout of the same cache: (B G, T + TTAIL, H, D) planes, keep (B G, T + TTAIL) with the tail visible."""
    kc = torch.cat([kp.repeat_interleave(G, 0), kt], 1).contiguous()
    vc = torch.cat([vp.repeat_interleave(G, 0), vt], 1).contiguous()
    kk = torch.cat([keep.repeat_interleave(G, 0), torch.ones((kt.shape[0], TTAIL), dtype=torch.uint8, device="cuda")], 1)
    return kc, vc, kk.contiguous()


def _workspace(N, D, split):
    S = _L().load().msr3d_attn_decode_splits(N, H) if split else 1
    return torch.empty(N * H * S * (D + 2), dtype=torch.float32, device="cuda") if S > 1 else None


def _run_shared(B, G, T, D, q, kp, vp, keep, kt, vt, tail_len, len_add=0, split=True):
    N = B * G
    out = torch.full((N, H * D), 7.0, dtype=torch.bfloat16, device="cuda")
    ws = _workspace(N, D, split)                      # (splits 0 without a workspace is one split, as in msr3d_attn_decode)
    L = _L()
    L.check(L.load().msr3d_attn_decode_shared(B, G, T, TTAIL, H, D, _p(q), H * D, _p(kp), _p(vp), _p(keep), _p(kt), _p(vt),
                                               _p(tail_len), len_add, ctypes.c_float(1.0 / math.sqrt(D)), _p(out), H * D,
                                               _p(ws), ws.numel() if ws is not None else 0, 0 if split else 1, _st()),
            "msr3d_attn_decode_shared")
    torch.cuda.synchronize()
    return out


def _run_rows(N, D, q, kc, vc, kk, ln, len_add=0, split=True):
    out = torch.full((N, H * D), 7.0, dtype=torch.bfloat16, device="cuda")
    ws = _workspace(N, D, split)
    L = _L()
    L.check(L.load().msr3d_attn_decode(N, kc.shape[1], H, D, _p(q), H * D, _p(kc), _p(vc), _p(ln), len_add, _p(kk),
                                        ctypes.c_float(1.0 / math.sqrt(D)), _p(out), H * D, _p(ws),
                                        ws.numel() if ws is not None else 0, _st()), "msr3d_attn_decode")
    torch.cuda.synchronize()
    return out


def _ref64(q, kc, vc, kk, ln, D):
    """float64: softmax(q K^T / sqrt(D) + padding) V over the first ln[n] keys of the materialised cache."""
    N, Tm = kc.shape[:2]
    qd = q.double().view(N, H, 1, D)
    kd, vd = kc.double().permute(0, 2, 1, 3), vc.double().permute(0, 2, 1, 3)
    s = (qd @ kd.transpose(-1, -2)) / math.sqrt(D)
    vis = (torch.arange(Tm, device="cuda")[None] < ln[:, None]) & kk.bool()
    p = torch.softmax(s.masked_fill(~vis[:, None, None], float("-inf")), -1).nan_to_num(0.0)
    return (p @ vd).reshape(N, H * D)


@pytest.mark.parametrize("T", [1, 7, 64, 65, 333])
@pytest.mark.parametrize("B,G", [(1, 1), (3, 5), (2, 8), (2, 9)])
@pytest.mark.parametrize("D", [64, 128])
def test_bits_of_attn_decode_on_the_materialised_cache_and_float64(D, B, G, T):
    gen = torch.Generator(device="cuda").manual_seed(1000 * D + 100 * B + 10 * G + T)
    N = B * G
    dead = 1 if B > 1 else None                       # one prompt with every key masked
    q, kp, vp, keep, kt, vt = _case(B, G, T, D, gen, dead_prompt=dead)
    kc, vc, kk = _materialise(G, kp, vp, keep, kt, vt)
    worst = 0.0
    for tail in TAILS:
        tl = torch.full((B,), tail, dtype=torch.int32, device="cuda")
        ln = torch.full((N,), T + tail, dtype=torch.int32, device="cuda")
        ref = _ref64(q, kc, vc, kk, ln.long(), D)
        for split in (True, False):
            got = _run_shared(B, G, T, D, q, kp, vp, keep, kt, vt, tl, split=split)
            want = _run_rows(N, D, q, kc, vc, kk, ln, split=split)
            assert torch.equal(got, want), (tail, split, float((got.float() - want.float()).abs().max()))
            err = rel(got, ref)
            worst = max(worst, err)
            assert err < 4e-3, (tail, split, err)
            if dead is not None and tail == 0:        # a fully masked prompt with an empty tail: exact zeros
                assert float(got[dead * G:(dead + 1) * G].float().abs().max()) == 0.0
    print("shared vs float64: D %d B %d G %d T %d worst rel-L2 %.5f" % (D, B, G, T, worst))


@pytest.mark.parametrize("D", [64, 128])
def test_len_add_a_length_beyond_the_tail_and_no_key_padding(D):
    gen = torch.Generator(device="cuda").manual_seed(77 + D)
    B, G, T = 3, 5, 65
    N = B * G
    q, kp, vp, keep, kt, vt = _case(B, G, T, D, gen)
    kc, vc, kk = _materialise(G, kp, vp, keep, kt, vt)
    # a different tail length per prompt, one more key through len_add (what a decode step passes)
    tl = torch.tensor([0, 4, 69], dtype=torch.int32, device="cuda")
    ln = (T + tl).repeat_interleave(G).contiguous()
    for split in (True, False):
        got = _run_shared(B, G, T, D, q, kp, vp, keep, kt, vt, tl, len_add=1, split=split)
        assert torch.equal(got, _run_rows(N, D, q, kc, vc, kk, ln, len_add=1, split=split))
        assert rel(got, _ref64(q, kc, vc, kk, ln.long() + 1, D)) < 4e-3
    # a tail length beyond Ttail is clamped to it, not followed
    far = torch.full((B,), 100000, dtype=torch.int32, device="cuda")
    full = torch.full((N,), T + TTAIL, dtype=torch.int32, device="cuda")
    got = _run_shared(B, G, T, D, q, kp, vp, keep, kt, vt, far)
    assert torch.equal(got, _run_rows(N, D, q, kc, vc, kk, full))
    assert rel(got, _ref64(q, kc, vc, kk, full.long(), D)) < 4e-3
    # prompt_keep NULL: every prompt slot visible
    got = _run_shared(B, G, T, D, q, kp, vp, None, kt, vt, tl)
    assert torch.equal(got, _run_rows(N, D, q, kc, vc, None, ln))
    assert rel(got, _ref64(q, kc, vc, torch.ones_like(kk), ln.long(), D)) < 4e-3


def test_invalid_arguments_are_refused_without_a_launch():
    h = _L().load()
    one = ctypes.c_void_p(torch.zeros(64, device="cuda").data_ptr())
    null, f1 = ctypes.c_void_p(0), ctypes.c_float(1.0)

    def go(B=1, G=5, T=8, Tt=4, Hh=2, D=64, q=one, ldq=128, kp=one, vp=one, kt=one, vt=one, tl=one, ldo=128, ws=null, wsn=0,
           splits=0):
        return h.msr3d_attn_decode_shared(B, G, T, Tt, Hh, D, q, ldq, kp, vp, null, kt, vt, tl, 0, f1, one, ldo, ws, wsn,
                                          splits, null)

    assert go(D=96, ldq=192, ldo=192) == -22                       # D
    assert go(ldq=64) == -22                                       # ldq < H D
    assert go(kp=null) == -22 and go(vp=null) == -22               # a null prompt plane
    assert go(kt=null) == -22 and go(tl=null) == -22               # a null tail plane with Ttail > 0; no lengths
    assert go(ws=one, wsn=4) == -22 and go(ws=one, wsn=4, splits=2) == -22     # a workspace that is too small
    assert go(splits=2) == -22                                     # more than one split without a workspace
    assert go(T=0) == -22 and go(G=0) == -22 and go(splits=9) == -22
    assert go(B=0, q=null, kp=null, vp=null, kt=null, vt=null, tl=null) == 0
