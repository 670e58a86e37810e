"""The four kernels of the e4m3 key / value cache (csrc/llm_decode.hip) alone, against the format's statement in torch
(msr3d_amd/llm/kv_cache.py: torch_kv_quantize / torch_kv_dequantize) and against their bf16 twins:

1. msr3d_kv_quantize_e4m3 writes the statement's codes and exponents, bit for bit.
2. msr3d_rope_kv_append_e4m3: q's bits are msr3d_rope_kv_append's, the written slot is the statement applied to the slot
   the bf16 entry writes, and no other byte of the planes changes; a full cache is not written.
3. msr3d_attn_decode_e4m3 gives the BITS of msr3d_attn_decode on the dequantised cache (and is within the bf16 output
   rounding, 4e-3 rel-L2, of float64 on it) at every length where the walk changes: KPW = 64 / (D / 8) keys a wave step,
   4 KPW U keys a round of the workgroup with U = 8 steps in flight.
4. msr3d_attn_decode_shared_e4m3 gives the bits of msr3d_attn_decode_e4m3 on the materialised cache.
5. Invalid arguments are refused with -22 and no launch.

Every slot that must not reach a product (beyond the length, or masked) holds NaN codes (0x7f) and exponent byte 0xff;
the exponent planes are padded to 16 bytes a slot (lde = 16 at H = 8) and the padding holds a sentinel."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
H = 8
LDE = 16


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _L():
    from msr3d_amd import _lib as L
    return L


def _call(name, *args):
    L = _L()
    L.check(getattr(L.load(), name)(*args), name)


def _st():
    return _L().current_stream_ptr(torch.device("cuda"))


def _fmt():
    from msr3d_amd.llm import kv_cache
    return kv_cache.torch_kv_quantize, kv_cache.torch_kv_dequantize


def _heads(*shape, gen):
    """(..., H, D) bf16 with per-head magnitudes exp(2 randn)."""
    mag = torch.exp(2.0 * torch.randn(shape[:-1], generator=gen, device="cuda"))
    return (mag[..., None] * torch.randn(shape, generator=gen, device="cuda")).to(torch.bfloat16)


def _pad_exps(e, lde=LDE, fill=0x5A):
    """exps (..., H) -> (..., lde) with the sentinel in the padding."""
    out = torch.full((*e.shape[:-1], lde), fill, dtype=torch.uint8, device=e.device)
    out[..., :e.shape[-1]] = e
    return out.contiguous()


# ----------------------------------------------------------------------------------------------------------- quantise
@pytest.mark.parametrize("rows,Hh,D", [(5, 8, 64), (37, 4, 128), (3, 32, 128)])
def test_quantize_kernel_writes_the_statements_codes_and_exponents(rows, Hh, D):
    quant, _ = _fmt()
    gen = torch.Generator(device="cuda").manual_seed(rows * D)
    ldx = Hh * D + 64                                           # rows are a column block of a wider buffer
    buf = torch.zeros((rows, ldx), dtype=torch.bfloat16, device="cuda")
    x = _heads(rows, Hh, D, gen=gen)
    x[0, 0] = 0.0                                               # a zero head, with a negative zero in it
    x[0, 0, 5] = -0.0
    above = float((torch.tensor(448.0).bfloat16().view(torch.int16) + 1).view(torch.bfloat16))
    for i, (amax, k) in enumerate([(448.0, 0), (above, 0), (448.0, -9), (above, -9), (448.0, 6), (above, 6)]):
        r, h = 1 + i // Hh, i % Hh                              # heads whose amax is 448 2^k and the next bf16 above it
        v = torch.rand(D, generator=gen, device="cuda") * 1.8 - 0.9
        v[(7 * i) % D] = -1.0 if i % 2 else 1.0                 # ... carried by a negative element every other time
        x[r, h] = (v * amax * 2.0 ** k).to(torch.bfloat16)
    buf[:, :Hh * D] = x.view(rows, Hh * D)
    lde = -(-Hh // 16) * 16
    codes = torch.full((rows, Hh, D), 0xA5, dtype=torch.uint8, device="cuda")
    exps = torch.full((rows, lde), 0x5A, dtype=torch.uint8, device="cuda")
    _call("msr3d_kv_quantize_e4m3", rows, Hh, D, _p(buf), ldx, _p(codes), _p(exps), lde, _st())
    torch.cuda.synchronize()
    want_c, want_e = quant(x)
    assert torch.equal(exps[:, :Hh], want_e)
    assert torch.equal(codes, want_c)
    assert bool((exps[:, Hh:] == 0x5A).all())
    assert int(want_e[0, 0]) == 127 and int(want_c[0, 0, 5]) == 0x80
    assert torch.equal(torch.cat([quant(x.cpu())[0].view(-1), quant(x.cpu())[1].view(-1)]),
                       torch.cat([want_c.view(-1), want_e.view(-1)]).cpu())        # the statement is device-agnostic


# ------------------------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("D", [64, 128])
def test_append_writes_the_statement_of_the_bf16_entrys_slot_and_nothing_else(D):
    from msr3d_amd.llm.decoder import rope_tables
    quant, _ = _fmt()
    gen = torch.Generator(device="cuda").manual_seed(D + 1)
    N, Tmax = 5, 40
    HD = H * D
    cs, sn = rope_tables(Tmax, D, 10000.0, torch.device("cuda"))
    qkv = _heads(N, 3 * H, D, gen=gen).view(N, 3 * HD).contiguous()          # q | k | v column blocks (ld = 3 H D)
    qkv[1, 2 * HD:2 * HD + D] = 0.0                                           # a zero head of v
    qkv2 = qkv.clone()
    pos = torch.tensor([0, 3, 17, 39, 8], dtype=torch.int32, device="cuda")
    ln = torch.tensor([5, 0, 39, 12, 40], dtype=torch.int32, device="cuda")  # the last row's cache is full
    kb = torch.zeros((N, Tmax, H, D), dtype=torch.bfloat16, device="cuda")
    vb = torch.zeros_like(kb)

    def args(b):
        return (_p(b), ctypes.c_void_p(b.data_ptr() + 2 * HD), ctypes.c_void_p(b.data_ptr() + 4 * HD), 3 * HD, _p(pos), _p(ln),
                _p(cs), _p(sn), Tmax)

    _call("msr3d_rope_kv_append", N, H, D, Tmax, *args(qkv), _p(kb), _p(vb), _st())
    kc = torch.full((N, Tmax, H, D), 0xA5, dtype=torch.uint8, device="cuda")
    vc = torch.full_like(kc, 0xA6)
    ke = torch.full((N, Tmax, LDE), 0x5A, dtype=torch.uint8, device="cuda")
    ve = torch.full_like(ke, 0x5B)
    want = [t.clone() for t in (kc, vc, ke, ve)]
    _call("msr3d_rope_kv_append_e4m3", N, H, D, Tmax, *args(qkv2), _p(kc), _p(vc), _p(ke), _p(ve), LDE, _st())
    torch.cuda.synchronize()
    assert torch.equal(qkv2, qkv)                               # q rotated to the same bits; k and v only read
    for n in range(N):
        slot = int(ln[n])
        if slot < Tmax:
            for plane, ex, src in ((want[0], want[2], kb), (want[1], want[3], vb)):
                c, e = quant(src[n, slot])
                plane[n, slot], ex[n, slot, :H] = c, e
    for got, w in zip((kc, vc, ke, ve), want):
        assert torch.equal(got, w)
    assert int(ve[1, 0, 0]) == 127                              # (the zero head)


# ---------------------------------------------------------------------------------------------------------- attention
def _quantized_cache(N, Tmax, D, gen):
    quant, dequant = _fmt()
    kc, ke = quant(_heads(N, Tmax, H, D, gen=gen))
    vc, ve = quant(_heads(N, Tmax, H, D, gen=gen))
    return kc, vc, _pad_exps(ke), _pad_exps(ve)


def _poison(planes, dead):
    """dead (N, T) bool: slots that must not reach a product get NaN codes and exponent byte 0xff."""
    kc, vc, ke, ve = planes
    kc[dead], vc[dead] = 0x7F, 0x7F
    ke[dead], ve[dead] = 0xFF, 0xFF


def _ws(N, D, split):
    S = _L().load().msr3d_attn_decode_splits(N, H) if split else 1
    return S, (torch.empty(N * H * S * (D + 2), dtype=torch.float32, device="cuda") if S > 1 else None)


def _run_e4m3(q, planes, keep, ln, D, len_add, split=True):
    kc, vc, ke, ve = planes
    N, Tmax = kc.shape[:2]
    out = torch.full((N, H * D), 7.0, dtype=torch.bfloat16, device="cuda")
    _, ws = _ws(N, D, split)
    _call("msr3d_attn_decode_e4m3", N, Tmax, H, D, _p(q), H * D, _p(kc), _p(vc), _p(ke), _p(ve), LDE, _p(ln), len_add,
          _p(keep), ctypes.c_float(1.0 / math.sqrt(D)), _p(out), H * D, _p(ws), ws.numel() if ws is not None else 0, _st())
    torch.cuda.synchronize()
    return out


def _run_bf16(q, kd, vd, keep, ln, D, len_add, split=True):
    N, Tmax = kd.shape[:2]
    out = torch.full((N, H * D), 7.0, dtype=torch.bfloat16, device="cuda")
    _, ws = _ws(N, D, split)
    _call("msr3d_attn_decode", N, Tmax, H, D, _p(q), H * D, _p(kd), _p(vd), _p(ln), len_add, _p(keep),
          ctypes.c_float(1.0 / math.sqrt(D)), _p(out), H * D, _p(ws), ws.numel() if ws is not None else 0, _st())
    torch.cuda.synchronize()
    return out


def _ref64(q, kd, vd, keep, ln, D):
    """float64 softmax(q K^T / sqrt(D) + padding) V over the first ln[n] keys (unread slots, NaN, count as 0)."""
    N, Tm = kd.shape[:2]
    qd = q.double().view(N, H, 1, D)
    k64, v64 = kd.double().nan_to_num(0.0).permute(0, 2, 1, 3), vd.double().nan_to_num(0.0).permute(0, 2, 1, 3)
    s = (qd @ k64.transpose(-1, -2)) / math.sqrt(D)
    vis = (torch.arange(Tm, device="cuda")[None] < ln[:, None]) & keep.bool()
    p = torch.softmax(s.masked_fill(~vis[:, None, None], float("-inf")), -1).nan_to_num(0.0)
    return (p @ v64).reshape(N, H * D)


@pytest.mark.parametrize("len_add", [0, 1])
@pytest.mark.parametrize("N", [1, 40])                          # 1 x 8: eight splits and the merge launch; 40 x 8: one split
@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_e4m3_gives_the_bits_of_the_bf16_twin_on_the_dequantised_cache(D, N, len_add):
    _, dequant = _fmt()
    gen = torch.Generator(device="cuda").manual_seed(1000 * D + 10 * N + len_add)
    KPW, Tmax = 64 // (D // 8), 340
    rnd = 4 * KPW * 8
    lengths = [0, 1, KPW - 1, KPW, rnd - 1, rnd, rnd + 1, 333]
    assert msr_splits(N) == (8 if N == 1 else 1)
    q = _heads(N, H, D, gen=gen).view(N, H * D).contiguous()
    clean = _quantized_cache(N, Tmax, D, gen)
    keep = (torch.rand(N, Tmax, generator=gen, device="cuda") >= 0.2).to(torch.uint8)      # key-padding holes
    keep[:, 0] = 1
    worst = 0.0
    for shift in range(len(lengths) if N == 1 else 2):
        ln = torch.tensor([lengths[(n + shift) % len(lengths)] for n in range(N)], dtype=torch.int32, device="cuda")
        planes = [t.clone() for t in clean]
        live = torch.arange(Tmax, device="cuda")[None] < (ln + len_add)[:, None]
        _poison(planes, ~(live & keep.bool()))
        kd, vd = dequant(planes[0], planes[2][..., :H]), dequant(planes[1], planes[3][..., :H])
        got = _run_e4m3(q, planes, keep, ln, D, len_add)
        assert torch.equal(got, _run_bf16(q, kd, vd, keep, ln, D, len_add)), (ln.tolist(), "bits of the bf16 twin")
        assert torch.equal(got, _run_e4m3(q, planes, keep, ln, D, len_add)), "the same bits twice"
        assert not bool(got.float().isnan().any())
        err = rel(got, _ref64(q, kd, vd, keep, (ln + len_add).long(), D))
        worst = max(worst, err)
        assert err < 4e-3, (ln.tolist(), err)
        empty = (ln + len_add) == 0
        if bool(empty.any()):
            assert float(got[empty].float().abs().max()) == 0.0                            # no visible key: 0
    print("attn_decode_e4m3 vs float64 on the dequantised cache: D %d N %d len_add %d worst rel-L2 %.5f"
          % (D, N, len_add, worst))


def msr_splits(N):
    return _L().load().msr3d_attn_decode_splits(N, H)


TTAIL = 72
TAILS = (0, 1, 5, 70)


@pytest.mark.parametrize("T", [1, 7, 64, 65, 333])
@pytest.mark.parametrize("B,G", [(1, 1), (3, 5), (2, 8), (2, 9)])
@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_shared_e4m3_gives_the_bits_of_the_rows_kernel_on_the_materialised_cache(D, B, G, T):
    _, dequant = _fmt()
    gen = torch.Generator(device="cuda").manual_seed(1000 * D + 100 * B + 10 * G + T)
    N = B * G
    q = _heads(N, H, D, gen=gen).view(N, H * D).contiguous()
    prompt = _quantized_cache(B, T, D, gen)
    tails = _quantized_cache(N, TTAIL, D, gen)
    keep = (torch.rand(B, T, generator=gen, device="cuda") >= 0.2).to(torch.uint8)
    keep[:, T - 1] = 1
    if B > 1:
        keep[1] = 0                                             # one prompt with every key masked
    _poison(prompt, ~keep.bool())
    visible = torch.ones((N, TTAIL), dtype=torch.uint8, device="cuda")
    rows_keep = torch.cat([keep.repeat_interleave(G, 0), visible], 1).contiguous()
    for tail in TAILS:
        tp = [t.clone() for t in tails]
        _poison(tp, (torch.arange(TTAIL, device="cuda") >= tail)[None].expand(N, TTAIL))
        rows = [torch.cat([p.repeat_interleave(G, 0), t], 1).contiguous() for p, t in zip(prompt, tp)]
        tl = torch.full((B,), tail, dtype=torch.int32, device="cuda")
        ln = torch.full((N,), T + tail, dtype=torch.int32, device="cuda")
        for split in (True, False):
            out = torch.full((N, H * D), 7.0, dtype=torch.bfloat16, device="cuda")
            _, ws = _ws(N, D, split)
            _call("msr3d_attn_decode_shared_e4m3", B, G, T, TTAIL, H, D, _p(q), H * D, _p(prompt[0]), _p(prompt[1]),
                  _p(prompt[2]), _p(prompt[3]), _p(keep), _p(tp[0]), _p(tp[1]), _p(tp[2]), _p(tp[3]), LDE, _p(tl), 0,
                  ctypes.c_float(1.0 / math.sqrt(D)), _p(out), H * D, _p(ws), ws.numel() if ws is not None else 0,
                  0 if split else 1, _st())
            torch.cuda.synchronize()
            want = _run_e4m3(q, rows, rows_keep, ln, D, 0, split=split)
            assert torch.equal(out, want), (tail, split, float((out.float() - want.float()).abs().max()))
            assert not bool(out.float().isnan().any())
        if tail == 5:                                           # and, through the rows kernel, the bf16 twin and float64
            kd, vd = dequant(rows[0], rows[2][..., :H]), dequant(rows[1], rows[3][..., :H])
            assert torch.equal(out, _run_bf16(q, kd, vd, rows_keep, ln, D, 0, split=False))
            assert rel(out, _ref64(q, kd, vd, rows_keep, ln.long(), D)) < 4e-3


# ------------------------------------------------------------------------------------------------------ invalid arguments
def test_invalid_arguments_are_refused_without_a_launch():
    h = _L().load()
    buf = torch.zeros(4096, device="cuda")
    one = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 8)                   # not 16-byte aligned
    null, f1 = ctypes.c_void_p(0), ctypes.c_float(1.0)

    def quant(rows=2, Hh=2, D=64, x=one, ldx=128, c=one, e=one, lde=16):
        return h.msr3d_kv_quantize_e4m3(rows, Hh, D, x, ldx, c, e, lde, null)

    assert quant(D=96, ldx=192) == -22 and quant(ldx=64) == -22 and quant(lde=1) == -22
    assert quant(x=odd) == -22 and quant(c=odd) == -22 and quant(e=null) == -22 and quant(c=null) == -22
    assert quant(rows=0, x=null, c=null, e=null) == 0

    def append(N=2, Hh=2, D=64, Tmax=4, q=one, ld=128, kc=one, vc=one, ke=one, ve=one, lde=16):
        return h.msr3d_rope_kv_append_e4m3(N, Hh, D, Tmax, q, one, one, ld, one, one, one, one, 8, kc, vc, ke, ve, lde, null)

    assert append(D=96, ld=192) == -22 and append(D=32) == -22 and append(ld=64) == -22 and append(lde=1) == -22
    assert append(kc=odd) == -22 and append(vc=odd) == -22 and append(ke=null) == -22 and append(ve=null) == -22
    assert append(N=0, q=null) == 0

    def rows(N=2, Tmax=4, Hh=2, D=64, q=one, ldq=128, kc=one, vc=one, ke=one, ve=one, lde=16, ws=null, wsn=0):
        return h.msr3d_attn_decode_e4m3(N, Tmax, Hh, D, q, ldq, kc, vc, ke, ve, lde, one, 0, null, f1, one, 128, ws, wsn, null)

    assert rows(D=96, ldq=192) == -22 and rows(ldq=64) == -22 and rows(lde=1) == -22
    assert rows(kc=odd) == -22 and rows(vc=odd) == -22 and rows(ke=null) == -22 and rows(ve=null) == -22
    assert rows(ws=one, wsn=4) == -22
    assert rows(N=0, q=null, kc=null, vc=null, ke=null, ve=null) == 0

    def shared(B=1, G=5, T=8, Tt=4, Hh=2, D=64, ldq=128, kp=one, vp=one, kep=one, vep=one, kt=one, vt=one, ket=one, vet=one,
               lde=16, ws=null, wsn=0, splits=0):
        return h.msr3d_attn_decode_shared_e4m3(B, G, T, Tt, Hh, D, one, ldq, kp, vp, kep, vep, null, kt, vt, ket, vet, lde, one,
                                               0, f1, one, 128, ws, wsn, splits, null)

    assert shared(D=96, ldq=192) == -22 and shared(ldq=64) == -22 and shared(lde=1) == -22
    assert shared(kp=odd) == -22 and shared(vp=odd) == -22 and shared(kt=odd) == -22 and shared(vt=odd) == -22
    assert shared(kep=null) == -22 and shared(vep=null) == -22 and shared(ket=null) == -22 and shared(vet=null) == -22
    assert shared(splits=2) == -22 and shared(ws=one, wsn=4, splits=2) == -22 and shared(T=0) == -22
    assert shared(B=0) == 0
