"""msr3d_fp8_skinny_lowrank (csrc/llm_decode_fp8.hip) alone: the decode step's weight-stream product on e4m3 weights,

    C_j (M, N_j) bf16 = diag(sp) (Pq Wq_j^T) diag(sw_j) + P2 B2_j^T.

M in {1, 5, 16, 17, 32, 33, 48, 49, 64} (every activation-tile count, full and ragged), K in {128, 384, 640, 1024} (one
step; a wave without a step; an uneven split; two steps a wave), N in {128, 384}, R in {0, 64}.

A. against a float64 product of the DEQUANTISED operands plus the float64 low-rank term: rel-L2 < 4e-3, the bound
   tests/test_lora_fp8_gpu.py puts on the wide e4m3 product (bf16 output rounding 2^-9 plus fp32 accumulation; e4m3 x
   e4m3 products are exact in fp32).  Rows >= M of C keep a sentinel.
B. row m of C has the same bits in a call of m + 1 rows and in one of 64; a NaN in another row's P2 or sp does not reach
   it; two launches give equal bits.
C. three jobs in one launch == three one-job launches, bit for bit.
D. the SwiGLU launch == two plain launches + msr3d_swiglu_fwd, bit for bit.
E. invalid arguments return -22 without a launch, empty problems 0.

Measured on an MI355X (printed by the tests), worst rel-L2 over all M and N:
   K  128: R 0 0.001832, R 64 0.001758     K  384: R 0 0.001700, R 64 0.001882
   K  640: R 0 0.001842, R 64 0.001861     K 1024: R 0 0.001730, R 64 0.001780
(a bf16 rounding is up to 2^-9 = 0.00195 of a value and 2^-9 / sqrt 3 = 0.0011 in the mean); B to E hold bit for bit."""
import ctypes
import functools

import pytest
import torch

from tests.test_lora_fp8_gpu import e4m3_decode, rel

pytestmark = pytest.mark.gpu
M_ALL = (1, 5, 16, 17, 32, 33, 48, 49, 64)
K_ALL = (128, 384, 640, 1024)
N_ALL = (128, 384)
NMAX, MMAX, PAD_R = 384, 64, 64
SENTINEL = 768.0          # (a bf16 value)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


@functools.lru_cache(maxsize=None)
def _case(K):
    """The operands of every test at this K, made once: 64 activation rows of very different scale, 384 weight rows, a
    low-rank pair of rank 48 in its 64 zero-padded columns, and the float64 statement of both terms."""
    from msr3d_amd.llm.lora import quant_rows_fp8
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(MMAX, K, generator=g) * torch.exp(torch.randn(MMAX, 1, generator=g))).bfloat16().cuda()
    w = (torch.randn(NMAX, K, generator=g) / K ** 0.5).bfloat16().cuda()
    xq, sx = quant_rows_fp8(x)
    wq, sw = quant_rows_fp8(w)
    u = torch.zeros(MMAX, PAD_R).bfloat16()
    b2 = torch.zeros(NMAX, PAD_R).bfloat16()
    u[:, :48] = (torch.randn(MMAX, 48, generator=g) * 0.3).bfloat16()
    b2[:, :48] = (torch.randn(NMAX, 48, generator=g) * 0.3).bfloat16()
    torch.cuda.synchronize()
    xd = torch.from_numpy(e4m3_decode(xq.cpu().numpy())) * sx.double().cpu()[:, None]
    wd = torch.from_numpy(e4m3_decode(wq.cpu().numpy())) * sw.double().cpu()[:, None]
    return dict(K=K, xq=xq, sx=sx, wq=wq, sw=sw, u=u.cuda(), b2=b2.cuda(), main=xd @ wd.T, low=u.double() @ b2.double().T)


def _launch(c, M, R, spans, swiglu=False, sx=None, u=None, expect=0):
    """One launch with one job per (n0, n1) span of the case's weight rows -> the jobs' outputs (64, n1 - n0) bf16, every
    element preset to the sentinel."""
    from msr3d_amd import _lib
    K = c["K"]
    sx = c["sx"] if sx is None else sx
    u = c["u"] if u is None else u
    outs = [torch.full((MMAX, n1 - n0), SENTINEL, dtype=torch.bfloat16, device="cuda") for n0, n1 in spans]
    jobs = (_lib.Fp8SkinnyJob * max(1, len(spans)))()
    for j, (n0, n1) in enumerate(spans):
        jobs[j] = _lib.Fp8SkinnyJob(c["wq"][n0:n1].data_ptr(), K, c["sw"][n0:n1].data_ptr(),
                                    c["b2"][n0:n1].data_ptr() if R else 0, PAD_R,
                                    0 if (swiglu and j == 1) else outs[j].data_ptr(), n1 - n0, n1 - n0)
    rc = _lib.load().msr3d_fp8_skinny_lowrank(M, K, R, _p(c["xq"]), K, _p(sx), _p(u if R else None), PAD_R, len(spans), jobs,
                                              int(swiglu), _lib.current_stream_ptr(torch.device("cuda")))
    assert rc == expect, rc
    torch.cuda.synchronize()
    return outs


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("R", [0, 64])
@pytest.mark.parametrize("K", K_ALL)
def test_product_against_float64_on_the_dequantised_operands(K, R):
    c = _case(K)
    want = c["main"] + (c["low"] if R else 0)
    worst = 0.0
    for N in N_ALL:
        whole, = _launch(c, MMAX, R, [(0, N)])
        for M in M_ALL:
            got, = _launch(c, M, R, [(0, N)])
            e = rel(got[:M], want[:M, :N])
            worst = max(worst, e)
            assert e < 4e-3, (M, N, e)
            assert bool((got[M:].float() == SENTINEL).all()), "a row >= M was written"
            # row m in a call of m + 1 rows and in one of 64 (and every row below it): the same bits
            assert torch.equal(_bits(got[:M]), _bits(whole[:M])), (M, N)
            again, = _launch(c, M, R, [(0, N)])
            assert torch.equal(_bits(again), _bits(got)), "two launches, two results"
    print("A: K %d R %d: worst rel-L2 over M, N %.6f" % (K, R, worst))


@pytest.mark.parametrize("K", K_ALL)
def test_a_nan_in_another_rows_scale_or_low_rank_activation_stays_there(K):
    c = _case(K)
    clean, = _launch(c, MMAX, PAD_R, [(0, NMAX)])
    for m in (0, 17, 40, 63):
        sx, u = c["sx"].clone(), c["u"].clone()
        others = torch.arange(MMAX, device="cuda") != m
        sx[others] = float("nan")
        u[others] = float("nan")
        got, = _launch(c, MMAX, PAD_R, [(0, NMAX)], sx=sx, u=u)
        assert torch.equal(_bits(got[m]), _bits(clean[m])), m
        assert bool(torch.isnan(got[others].float()).all())           # (and the poisoned rows do show it)
        if m + 1 < MMAX:                                               # the clamped reads of rows >= M as well
            short, = _launch(c, m + 1, PAD_R, [(0, NMAX)], sx=sx, u=u)
            assert torch.equal(_bits(short[m]), _bits(clean[m])), m


@pytest.mark.parametrize("R", [0, 64])
@pytest.mark.parametrize("K", K_ALL)
def test_jobs_of_one_launch_equal_one_job_launches_and_swiglu_equals_its_parts(K, R):
    from msr3d_amd import _lib
    c = _case(K)
    spans = [(0, 128), (128, 256), (256, 384)]
    for M in (1, 17, 33, 64):
        three = _launch(c, M, R, spans)
        ones = [_launch(c, M, R, [s])[0] for s in spans]
        for a, b in zip(three, ones):
            assert torch.equal(_bits(a), _bits(b)), M
        # gate = rows 0 .. 127, up = rows 128 .. 255
        act = _launch(c, M, R, spans[:2], swiglu=True)[0]
        want = torch.full_like(ones[0], SENTINEL)
        gate, up = ones[0][:M].contiguous(), ones[1][:M].contiguous()
        part = torch.empty_like(gate)
        _lib.call("msr3d_swiglu_fwd", gate.numel(), _p(gate), _p(up), _p(part), _lib.current_stream_ptr(torch.device("cuda")))
        torch.cuda.synchronize()
        want[:M] = part
        assert torch.equal(_bits(act), _bits(want)), M


def test_invalid_arguments_are_refused_and_empty_problems_succeed():
    from msr3d_amd import _lib
    h, st = _lib.load(), _lib.current_stream_ptr(torch.device("cuda"))
    c = _case(128)
    K = 128
    out = torch.full((MMAX, 128), SENTINEL, dtype=torch.bfloat16, device="cuda")

    def job(**o):
        return _lib.Fp8SkinnyJob(o.get("Wq", c["wq"].data_ptr()), o.get("ldw", K), o.get("sw", c["sw"].data_ptr()),
                                 o.get("B2", c["b2"].data_ptr()), o.get("ldb2", PAD_R), o.get("C", out.data_ptr()),
                                 o.get("ldc", 128), o.get("N", 128))

    def run(jobs=None, **o):
        jobs = [job()] if jobs is None else jobs
        arr = (_lib.Fp8SkinnyJob * max(1, len(jobs)))(*jobs)
        return h.msr3d_fp8_skinny_lowrank(o.get("M", 5), o.get("K", K), o.get("R", PAD_R), o.get("Pq", _p(c["xq"])),
                                          o.get("ldp", K), o.get("sp", _p(c["sx"])), o.get("P2", _p(c["u"])),
                                          o.get("ldp2", PAD_R), o.get("njobs", len(jobs)), o.get("jobs", arr),
                                          o.get("swiglu", 0), st)
    null = ctypes.c_void_p(0)
    assert run() == 0
    # null pointers
    assert run(Pq=null) == -22 and run(sp=null) == -22 and run(P2=null) == -22
    assert h.msr3d_fp8_skinny_lowrank(5, K, 0, _p(c["xq"]), K, _p(c["sx"]), null, 0, 1, None, 0, st) == -22
    assert run([job(Wq=0)]) == -22 and run([job(sw=0)]) == -22 and run([job(C=0)]) == -22
    assert run([job(B2=0)]) == 0                                       # (a job without a low-rank term is allowed)
    # K % 128, N % 16, leading dimensions, alignment
    assert run(K=64) == -22 and run(K=0) == -22 and run(R=16) == -22
    assert run([job(N=120)]) == -22 and run([job(N=0)]) == -22
    assert run(ldp=K - 16) == -22 and run(ldp=K + 8) == -22 and run([job(ldw=K - 16)]) == -22 and run([job(ldw=K + 8)]) == -22
    assert run(ldp2=32) == -22 and run(ldp2=PAD_R + 4) == -22 and run([job(ldb2=32)]) == -22 and run([job(ldc=64)]) == -22
    assert run(Pq=ctypes.c_void_p(c["xq"].data_ptr() + 8)) == -22 and run([job(Wq=c["wq"].data_ptr() + 8)]) == -22
    assert run(P2=ctypes.c_void_p(c["u"].data_ptr() + 2)) == -22 and run(sp=ctypes.c_void_p(c["sx"].data_ptr() + 2)) == -22
    # M and njobs
    assert run(M=65) == -22 and run(M=-1) == -22
    assert run([job()] * 4) == -22 and run(njobs=-1) == -22
    # swiglu: exactly two jobs of equal N
    assert run(swiglu=1) == -22 and run([job()] * 3, swiglu=1) == -22 and run([job(), job(N=64)], swiglu=1) == -22
    assert run([job(), job(C=0)], swiglu=1) == 0
    # empty problems
    assert run(M=0) == 0 and run(njobs=0) == 0
    torch.cuda.synchronize()
    assert bool((out[5:].float() == SENTINEL).all())
