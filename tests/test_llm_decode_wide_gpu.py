"""msr3d_bf16_skinny_lowrank_wide (csrc/llm_decode.hip): the weight-stream product at 33 .. 64 activation rows -- three
and four 16-row MFMA tiles per workgroup -- against a float64 torch statement on bf16-rounded inputs and against the
wide-tile GEMM (lora._gemm), as tests/test_llm_decode_gpu.py does for the entry that stops at 32 rows.  Tolerances are
the ones the project states for a bf16 product against float64: rel-L2 4e-3, and 2 x 4e-3 for the SwiGLU product (two
bf16-rounded factors).  Operands and the float64 reference of a shape are made once for 64 rows; a case with M rows
reads the first M of them.

M: 33 a third tile with one row, 48 a full third tile, 49 a fourth tile with one row, 64 a full fourth tile, 40 in
between.  (K, N): (128, 16) one chunk, so three of the four waves have an empty K range, and one tile; (384, 48) three
chunks over four waves (an uneven split) and an odd tile count, so one tile a workgroup; (512, 1024) the common case;
(4096, 11008) a real layer shape (a weight of 90 MB: byte offsets pass 2^31 bits only if mis-typed) on two tiles a
workgroup (344 workgroups as pairs: the entry takes the pair from 256); (512, 32000) the >= 16384-row dispatch of the
narrow entry, two tiles here as well."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 4e-3
MS = [33, 40, 48, 49, 64]
SHAPES = [(128, 16), (384, 48), (512, 1024), (4096, 11008), (512, 32000)]
SENTINEL = 9.0


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _lib():
    from msr3d_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    rc = getattr(L.load(), name)(*args)
    L.check(rc, name)


def _st():
    return _lib().current_stream_ptr(torch.device("cuda"))


def _bf(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen, device="cuda") * scale).to(torch.bfloat16)


def _wide(M, K, R, P, P2, jobs, swiglu=0):
    L = _lib()
    arr = (L.SkinnyJob * len(jobs))(*[L.SkinnyJob(W.data_ptr(), K, B2.data_ptr() if B2 is not None else 0, R,
                                                  C.data_ptr() if C is not None else 0, W.shape[0], W.shape[0])
                                      for W, B2, C in jobs])
    _call("msr3d_bf16_skinny_lowrank_wide", M, K, R, _p(P), K, _p(P2), R, len(jobs), arr, swiglu, _st())
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(K, N):
    """Operands for 64 rows and the two float64 products (without / with the low-rank term), made once per shape."""
    gen = torch.Generator(device="cuda").manual_seed(K + N)
    P, W = _bf(64, K, gen=gen, scale=0.5), _bf(N, K, gen=gen, scale=0.5 / K ** 0.5)
    P2, B2 = _bf(64, 64, gen=gen, scale=0.5), _bf(N, 64, gen=gen, scale=0.5)
    base = P.double() @ W.double().t()
    return P, W, P2, B2, base, base + P2.double() @ B2.double().t()


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,N", SHAPES)
def test_wide_matches_float64_and_gemm_lowrank_and_leaves_rows_beyond_m_alone(M, K, N):
    from msr3d_amd.llm import lora
    P, W, P2, B2, base, full = _case(K, N)
    for R in (64, 0):
        C = torch.full((80, N), SENTINEL, dtype=torch.bfloat16, device="cuda")           # taller than any M
        _wide(M, K, R, P, P2 if R else None, [(W, B2 if R else None, C)])
        want = (full if R else base)[:M]
        err = rel(C[:M], want)
        G = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        lora._gemm(M, N, K, R, P, K, W, K, P2 if R else None, R, B2 if R else None, R, G, N, False, 1.0, P.device)
        torch.cuda.synchronize()
        err_g = rel(C[:M], G.float())
        print("wide M %d K %d N %d R %d: rel-L2 vs float64 %.2e, vs gemm_lowrank %.2e" % (M, K, N, R, err, err_g))
        assert err < TOL
        assert err_g < TOL
        assert bool((C[M:] == SENTINEL).all())                                           # rows >= M are never stored


@pytest.mark.parametrize("M", [33, 64])
@pytest.mark.parametrize("ns", [(512, 512, 1024), (4096, 2048, 2048)])           # one tile of W a workgroup; two
def test_wide_three_jobs_in_one_launch_and_the_swiglu_epilogue(M, ns):
    gen = torch.Generator(device="cuda").manual_seed(M)
    K, N = 512, 1024
    P, P2 = _bf(M, K, gen=gen, scale=0.5), _bf(M, 64, gen=gen, scale=0.5)
    Ws = [_bf(n, K, gen=gen, scale=1.0 / K ** 0.5) for n in ns]
    Bs = [_bf(n, 64, gen=gen, scale=0.3) for n in ns]
    Cs = [torch.empty((M, w.shape[0]), dtype=torch.bfloat16, device="cuda") for w in Ws]
    _wide(M, K, 64, P, P2, list(zip(Ws, Bs, Cs)))
    for W, B2, C in zip(Ws, Bs, Cs):
        one = torch.empty_like(C)
        _wide(M, K, 64, P, P2, [(W, B2, one)])
        assert torch.equal(C, one)                                   # a job's result does not depend on its neighbours
        assert rel(C, P.double() @ W.double().t() + P2.double() @ B2.double().t()) < TOL
    Wg, Wu = _bf(N, K, gen=gen, scale=1.0 / K ** 0.5), _bf(N, K, gen=gen, scale=1.0 / K ** 0.5)
    Bg, Bu = _bf(N, 64, gen=gen, scale=0.3), _bf(N, 64, gen=gen, scale=0.3)
    act = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    _wide(M, K, 64, P, P2, [(Wg, Bg, act), (Wu, Bu, None)], swiglu=1)
    gate, up = torch.empty_like(act), torch.empty_like(act)
    _wide(M, K, 64, P, P2, [(Wg, Bg, gate), (Wu, Bu, up)])
    want = torch.empty_like(act)
    _call("msr3d_swiglu_fwd", act.numel(), _p(gate), _p(up), _p(want), _st())
    torch.cuda.synchronize()
    assert torch.equal(act, want)                                    # the same roundings as the two-launch path
    gd = P.double() @ Wg.double().t() + P2.double() @ Bg.double().t()
    ud = P.double() @ Wu.double().t() + P2.double() @ Bu.double().t()
    assert rel(act, torch.nn.functional.silu(gd) * ud) < 2 * TOL     # (a product of two bf16-rounded factors)


@pytest.mark.parametrize("K,N", [(384, 48), (512, 32000)])           # one tile of W a workgroup; two
def test_wide_a_row_of_c_depends_on_that_row_of_p_alone_and_launches_repeat(K, N):
    M = 64
    P, W, P2, B2, _, _ = _case(K, N)
    clean = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    _wide(M, K, 64, P, P2, [(W, B2, clean)])
    again = torch.empty_like(clean)
    _wide(M, K, 64, P, P2, [(W, B2, again)])
    assert torch.equal(clean, again)                                 # two launches: the same bits
    assert bool(torch.isfinite(clean.float()).all())
    for bad in (17, 63):
        Pn, P2n = P.clone(), P2.clone()
        Pn[bad], P2n[bad] = float("nan"), float("nan")
        C = torch.empty_like(clean)
        _wide(M, K, 64, Pn, P2n, [(W, B2, C)])
        others = [r for r in range(M) if r != bad]
        assert torch.equal(C[others].view(torch.int16), clean[others].view(torch.int16))
        assert bool(torch.isnan(C[bad].float()).all())               # ... and the poisoned row did reach its own output


def test_wide_below_33_rows_is_the_narrow_entry_bit_for_bit():
    """Up to 32 rows the wide entry launches what msr3d_bf16_skinny_lowrank launches."""
    K, N = 512, 1024
    P, W, P2, B2, _, _ = _case(K, N)
    L = _lib()
    for M in (5, 32):
        a = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        b = torch.empty_like(a)
        _wide(M, K, 64, P, P2, [(W, B2, a)])
        job = (L.SkinnyJob * 1)(L.SkinnyJob(W.data_ptr(), K, B2.data_ptr(), 64, b.data_ptr(), N, N))
        _call("msr3d_bf16_skinny_lowrank", M, K, 64, _p(P), K, _p(P2), 64, 1, job, 0, _st())
        torch.cuda.synchronize()
        assert torch.equal(a, b)


def test_wide_invalid_arguments_are_refused_without_a_launch():
    L = _lib()
    h = L.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    job = (L.SkinnyJob * 1)(L.SkinnyJob(16, 128, 0, 0, 16, 16, 16))
    wide = h.msr3d_bf16_skinny_lowrank_wide
    assert wide(65, 128, 0, one, 128, null, 0, 1, job, 0, null) == -22          # M > 64
    assert wide(0, 128, 0, one, 128, null, 0, 1, job, 0, null) == 0             # no rows: a no-op
    assert wide(40, 96, 0, one, 96, null, 0, 1, job, 0, null) == -22            # K % 128
    assert wide(40, 128, 0, one, 128, null, 0, 1, job, 1, null) == -22          # swiglu needs two jobs
    assert wide(40, 128, 64, one, 128, null, 64, 1, job, 0, null) == -22        # R without P2
    assert wide(40, 128, 0, one, 128, null, 0, 4, job, 0, null) == -22          # njobs
    assert h.msr3d_bf16_skinny_lowrank(33, 128, 0, one, 128, null, 0, 1, job, 0, null) == -22     # the narrow entry: as before
