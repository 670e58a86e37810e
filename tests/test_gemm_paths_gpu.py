"""GPU: every kernel the bf16 and e4m3 projection GEMMs can launch (csrc/lora_linear.hip: bf16_gemm_kernel<128 | 192>,
bf16_gemm_glds_kernel<192>, bf16_gemm_wide_kernel<8 | 9 | 10>; csrc/lora_fp8.hip: fp8_gemm_wide_kernel<8 | 9 | 10>), each
at shapes that take it -- asserted with the library's own path query before the launch -- and held to the BITS of the
float64 product.

Exact cases: operands are integers in {-3 .. 3} (exact in bf16 and in e4m3), scales are 1 or 1/2 (e4m3: per-row powers of
two in 2^-3 .. 2^1), K + R <= 4160, so every product, every partial sum in any order and the scaled total is a multiple of
2^-7 below 2^17 in magnitude: 24 bits, exact in fp32.  The kernel's only rounding is the final one to the output type, and
the reference is the float64 product rounded once the same way (round to nearest even) -- any differing bit is a bug, not
noise.  This is derived, not measured.  Ten launches per case, each into a freshly sentinel-filled buffer with ldc > N,
pad columns on both sides of C and guard rows below it, which must come back untouched; P, Q and the low-rank pair are
column blocks of wider matrices (ld > K) whose other columns hold other integers.

The shapes and the kernel each one pins are listed in tests/gemm_path_cases.py (tests/test_gemm_paths_cpu.py holds them
against the rule without a device)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import gemm_path_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = 10
BITS = {torch.float32: (torch.int32, 0x7fc5a5a5), torch.bfloat16: (torch.int16, 0x7fa5)}      # (integer view, sentinel)


def _env():
    from msr3d_amd import _lib
    return _lib, _lib.load(), _lib.current_stream_ptr(torch.device("cuda"))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum(int(k) * 7919 ** i for i, k in enumerate(key)) % (2 ** 31))


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, device="cuda", generator=g)


def _block(full, cols, off):
    """Columns off .. off + cols of a wider matrix: (the view the kernel reads, its leading dimension)."""
    return full[:, off:off + cols], full.stride(0)


def _same_bits(got, want, what):
    it = BITS[want.dtype][0]
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = got.contiguous().view(it) != want.contiguous().view(it)
    if bool(bad.any()):
        where = bad.nonzero()
        first = [(tuple(int(v) for v in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in where[:6]]
        rows = sorted({int(ix[-2]) for ix in where[:4096]})[:12]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 product; first "
                             f"(index, got, want): {first}; rows {rows} ...")


class _Out:
    """An output buffer of `dtype` filled with a sentinel bit pattern; `blocks` are the views a launch may write."""

    def __init__(self, shape, dtype):
        self.it, self.sent = BITS[dtype]
        self.buf = torch.empty(shape, dtype=dtype, device="cuda")
        self.bits = self.buf.view(self.it)
        self.blocks = []

    def reset(self):
        self.bits.fill_(self.sent)

    def untouched_outside_blocks(self):
        b = self.bits.clone()
        for sl in self.blocks:
            b[sl] = self.sent
        return bool((b == self.sent).all())


def _out2d(M, N, dtype):
    """C (M, N) at columns 8 .. 8 + N of a (M + 3, ldc) buffer: ldc > N, pad columns on both sides, three guard rows."""
    out = _Out((M + 3, (N + 3) // 4 * 4 + 16), dtype)
    out.blocks = [(slice(0, M), slice(8, 8 + N))]
    return out, out.buf[:M, 8:8 + N], out.buf.stride(0)


def _expect_path(lib, stated, M, N, R, batch, ldp, ldq, ldp2, ldq2):
    """The kernel this launch takes, from the library's query; it must be what the rule says under this process's
    MSR3D_BF16_GEMM, and under the default the kernel the case is listed for."""
    mode = G.mode_from_env()
    got = lib.msr3d_bf16_gemm_path(M, N, R, batch, ldp, ldq, ldp2, ldq2)
    assert got == G.rule(M, N, R, batch, mode, ldp, ldq, ldp2, ldq2), (G.PATH_NAMES.get(got, got), mode)
    if mode == "wide":
        assert got == stated, f"{M} x {N}, R = {R}, batch {batch}: takes {G.PATH_NAMES.get(got, got)}, listed for {G.PATH_NAMES[stated]}"
    return got


def _bf16_operands(g, M, N, K, R, make):
    """P (M, K), Q (N, K), P2 (M, R), Q2 (N, R) bf16 as column blocks of wider matrices (a q | k | v buffer's form)."""
    P, ldp = _block(make(g, M, K + 72), K, 8)
    Q, ldq = _block(make(g, N, K + 136), K, 16)
    if not R:
        return P, ldp, Q, ldq, None, 0, None, 0
    P2, ldp2 = _block(make(g, M, R + 24), R, 8)
    Q2, ldq2 = _block(make(g, N, R + 8), R, 8)
    return P, ldp, Q, ldq, P2, ldp2, Q2, ldq2


def _int_bf16(g, *shape):
    return _ints(g, *shape).to(torch.bfloat16)


def _product(P, Q, P2, Q2):
    want = P.double() @ Q.double().t()
    return want + P2.double() @ Q2.double().t() if P2 is not None else want


def _ids(cases):
    return ["-".join(str(v) for v in c[:-1]) + "-" + (G.PATH_NAMES[c[-1]] if c[-1] in G.PATH_NAMES else f"h{c[-1]}") for c in cases]


# ---------------------------------------------------------------------------------------------- msr3d_bf16_gemm_lowrank
@pytest.mark.parametrize("M,N,K,R,path", G.LOWRANK, ids=_ids(G.LOWRANK))
def test_bf16_lowrank_exact(M, N, K, R, path):
    _lib, lib, st = _env()
    P, ldp, Q, ldq, P2, ldp2, Q2, ldq2 = _bf16_operands(_gen(M, N, K, R), M, N, K, R, _int_bf16)
    _expect_path(lib, path, M, N, R, 1, ldp, ldq, ldp2, ldq2)
    prod = _product(P, Q, P2, Q2)
    flip = (M + K // 64 + R // 8) % 2                       # which output type meets which scale
    for dtype, scale in ((torch.float32, (1.0, 0.5)[flip]), (torch.bfloat16, (0.5, 1.0)[flip])):
        want = (prod * scale).to(dtype)
        out, C, ldc = _out2d(M, N, dtype)
        for launch in range(LAUNCHES):
            out.reset()
            rc = lib.msr3d_bf16_gemm_lowrank(M, N, K, R, _p(P), ldp, _p(Q), ldq, _p(P2), ldp2, _p(Q2), ldq2, _p(C), ldc,
                                             int(dtype == torch.float32), ctypes.c_float(scale), st)
            _lib.check(rc, "msr3d_bf16_gemm_lowrank")
            _same_bits(C, want, f"{dtype}, scale {scale}, launch {launch}")
            assert out.untouched_outside_blocks(), f"{dtype}, launch {launch}: wrote outside C"


@pytest.mark.parametrize("M,N,K,R,path", G.RANDOM, ids=_ids(G.RANDOM))
def test_bf16_random_operands_against_float64(M, N, K, R, path):
    _lib, lib, st = _env()
    make = lambda g, r, c: (torch.randn(r, c, device="cuda", generator=g) * 0.5).to(torch.bfloat16)      # noqa: E731
    P, ldp, Q, ldq, P2, ldp2, Q2, ldq2 = _bf16_operands(_gen(M, N, K, R, 1), M, N, K, R, make)
    _expect_path(lib, path, M, N, R, 1, ldp, ldq, ldp2, ldq2)
    out, C, ldc = _out2d(M, N, torch.bfloat16)
    out.reset()
    rc = lib.msr3d_bf16_gemm_lowrank(M, N, K, R, _p(P), ldp, _p(Q), ldq, _p(P2), ldp2, _p(Q2), ldq2, _p(C), ldc, 0,
                                     ctypes.c_float(1.0), st)
    _lib.check(rc, "msr3d_bf16_gemm_lowrank")
    want = _product(P, Q, P2, Q2)
    err = float((C.double() - want).norm() / want.norm())
    print(f"rel-L2 {err:.3e}")
    assert err < 4e-3                  # bf16 output rounding + fp32 accumulation: tests/test_lora_gpu.py's bound for this result
    assert out.untouched_outside_blocks()


# ------------------------------------------------------------------------------------------ msr3d_bf16_gemm_lowrank_acc
@pytest.mark.parametrize("M,N,K,R,height", G.ACC, ids=_ids(G.ACC))
def test_acc_exact(M, N, K, R, height):
    _lib, lib, st = _env()
    g = _gen(M, N, K, R, 2)
    P, ldp, Q, ldq, P2, ldp2, Q2, ldq2 = _bf16_operands(g, M, N, K, R, _int_bf16)
    assert lib.msr3d_bf16_gemm_acc_tile(M, N) == height
    C0 = _int_bf16(g, M, N)
    scale = (1.0, 0.5)[(M + K // 64) % 2]
    want = (_product(P, Q, P2, Q2) * scale + C0.double()).to(torch.bfloat16)
    out, C, ldc = _out2d(M, N, torch.bfloat16)
    for launch in range(LAUNCHES):
        out.reset()
        C.copy_(C0)
        rc = lib.msr3d_bf16_gemm_lowrank_acc(M, N, K, R, _p(P), ldp, _p(Q), ldq, _p(P2), ldp2, _p(Q2), ldq2, _p(C), ldc,
                                             ctypes.c_float(scale), st)
        _lib.check(rc, "msr3d_bf16_gemm_lowrank_acc")
        _same_bits(C, want, f"scale {scale}, launch {launch}")
        assert out.untouched_outside_blocks(), f"launch {launch}: wrote outside C"
    # outside the wide kernel's domain the entry refuses, and leaves C alone
    out.reset()
    for m, n in ((64, N), (M, 192), (M, N - 2)):
        assert lib.msr3d_bf16_gemm_lowrank_acc(m, n, K, R, _p(P), ldp, _p(Q), ldq, _p(P2), ldp2, _p(Q2), ldq2, _p(C), ldc,
                                               ctypes.c_float(scale), st) == -22
    torch.cuda.synchronize()
    assert bool((out.bits == out.sent).all())


@pytest.mark.parametrize("M,N,K,R,height", G.RANDOM_ACC, ids=_ids(G.RANDOM_ACC))
def test_acc_random_operands_against_float64(M, N, K, R, height):
    _lib, lib, st = _env()
    g = _gen(M, N, K, R, 3)
    make = lambda g, r, c: (torch.randn(r, c, device="cuda", generator=g) * 0.5).to(torch.bfloat16)      # noqa: E731
    P, ldp, Q, ldq, P2, ldp2, Q2, ldq2 = _bf16_operands(g, M, N, K, R, make)
    assert lib.msr3d_bf16_gemm_acc_tile(M, N) == height
    C0 = make(g, M, N) * 8
    out, C, ldc = _out2d(M, N, torch.bfloat16)
    out.reset()
    C.copy_(C0)
    rc = lib.msr3d_bf16_gemm_lowrank_acc(M, N, K, R, _p(P), ldp, _p(Q), ldq, _p(P2), ldp2, _p(Q2), ldq2, _p(C), ldc,
                                         ctypes.c_float(1.0), st)
    _lib.check(rc, "msr3d_bf16_gemm_lowrank_acc")
    want = _product(P, Q, P2, Q2) + C0.double()
    err = float((C.double() - want).norm() / want.norm())
    print(f"rel-L2 {err:.3e}")
    assert err < 4e-3
    assert out.untouched_outside_blocks()


# ---------------------------------------------------------------------------------------------- msr3d_bf16_gemm_batched
def _batched(name, P, Q, spec, strides, out, c_strides, want_of, dtypes):
    """P / Q: the full operand tensors; strides = (ldp, p_outer, p_inner, ldq, q_outer, q_inner); out: an _Out whose blocks
    are the batch elements' C in (outer, inner) order; want_of(dtype, scale) -> the list of their expected values."""
    _lib, lib, st = _env()
    outer, inner, M, N, K, path = spec
    ldp, po, pi, ldq, qo, qi = strides
    ldc, co, ci = c_strides
    _expect_path(lib, path, M, N, 0, outer * inner, ldp, ldq, 0, 0)
    for dtype, scale in dtypes:
        o = out(dtype)
        want = want_of(dtype, scale)
        for launch in range(LAUNCHES):
            o.reset()
            rc = lib.msr3d_bf16_gemm_batched(outer, inner, M, N, K, _p(P), ldp, po, pi, _p(Q), ldq, qo, qi, _p(o.buf), ldc, co, ci,
                                             int(dtype == torch.float32), ctypes.c_float(scale), st)
            _lib.check(rc, "msr3d_bf16_gemm_batched")
            for e, (sl, w) in enumerate(zip(o.blocks, want)):
                _same_bits(o.buf[sl], w, f"{name}: element {e} of {outer} x {inner}, {dtype}, launch {launch}")
            assert o.untouched_outside_blocks(), f"{name}, {dtype}, launch {launch}: wrote outside the elements' C"


def test_bf16_batched_head_backward_form():
    """FrozenLinear's split-reduction dx (llm/stack.py): dy (M, S K') against W^T (N, S K') as S products over the column
    chunks, fp32 partials stacked at c_outer = M N -- the wide kernel under blockIdx.z with spo / sqo / sco strides."""
    spec = S, _, M, N, K, _ = G.BATCHED["head_backward"]
    g = _gen(S, M, N, K)
    dy, wt = _int_bf16(g, M, S * K), _int_bf16(g, N, S * K)
    prod = torch.einsum("msk,nsk->smn", dy.double().view(M, S, K), wt.double().view(N, S, K))

    def out(dtype):
        o = _Out((S * M + 3, N), dtype)                      # the partials are contiguous: three guard rows after the last
        o.blocks = [(slice(s * M, (s + 1) * M), slice(0, N)) for s in range(S)]
        return o

    _batched("head backward", dy, wt, spec, (S * K, K, 0, S * K, K, 0), out, (N, M * N, 0),
             lambda dtype, scale: [(prod[s] * scale).to(dtype) for s in range(S)],
             [(torch.float32, 1.0), (torch.bfloat16, 0.5)])


@pytest.mark.parametrize("name", ["attention", "small"])
def test_bf16_batched_sequence_head_form(name):
    """Attention's per-(sequence, head) products: q, k as (B, T, H, D) token-major, scores (B, H, T, T') -- here with pad
    columns after every row and two guard rows after every element."""
    spec = B, H, M, N, K, _ = G.BATCHED[name]
    g = _gen(B, H, M, N, K)
    q, k = _int_bf16(g, B, M, H, K), _int_bf16(g, B, N, H, K)
    prod = torch.einsum("bmhk,bnhk->bhmn", q.double(), k.double())
    ldc = (N + 3) // 4 * 4 + 8

    def out(dtype):
        o = _Out((B, H, M + 2, ldc), dtype)
        o.blocks = [(b, h, slice(0, M), slice(0, N)) for b in range(B) for h in range(H)]
        return o

    _batched(name, q, k, spec, (H * K, M * H * K, K, H * K, N * H * K, K), out, (ldc, H * (M + 2) * ldc, (M + 2) * ldc),
             lambda dtype, scale: [(prod[b, h] * scale).to(dtype) for b in range(B) for h in range(H)],
             [(torch.float32, 0.5), (torch.bfloat16, 1.0)])


# -------------------------------------------------------------------------------------- msr3d_fp8_gemm_lowrank (and _acc)
def _e4m3_table():
    """The 256 OCP e4m3fn codes as float64 (0x7f / 0xff, the NaNs, as 0: never produced here)."""
    c = torch.arange(256)
    s, e, m = c >> 7, (c >> 3) & 15, (c & 7).double()
    v = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e.double() - 7))
    v = torch.where((c & 0x7f) == 0x7f, torch.zeros_like(v), v)
    return torch.where(s == 1, -v, v).cuda()


_E4M3_OF_INT = [0xc4, 0xc0, 0xb8, 0x00, 0x38, 0x40, 0x44]                 # -3 .. 3: sign | exponent (bias 7) | mantissa


def _fp8_block(g, rows, K):
    """(integers (rows, K) in -3 .. 3, their e4m3 codes as bytes 16 .. 16 + K of (K + 32)-byte rows, ld)."""
    lut = torch.tensor(_E4M3_OF_INT, dtype=torch.uint8, device="cuda")
    full = _ints(g, rows, K + 32)
    codes = lut[full + 3]
    assert torch.equal(_e4m3_table()[codes.long()], full.double())       # the hand-written codes are those integers
    return full[:, 16:16 + K].double(), codes[:, 16:16 + K], codes.stride(0)


def _fp8_launch(lib, st, accumulate, M, N, K, Pq, ldp, sp, Qq, ldq, sq, P2, ldp2, Q2, ldq2, C, ldc):
    fn = "msr3d_fp8_gemm_lowrank_acc" if accumulate else "msr3d_fp8_gemm_lowrank"
    return fn, getattr(lib, fn)(M, N, K, _p(Pq), ldp, _p(sp), _p(Qq), ldq, _p(sq), _p(P2), ldp2, _p(Q2), ldq2, _p(C), ldc, st)


@pytest.mark.parametrize("M,N,K,height", G.FP8, ids=_ids(G.FP8))
def test_fp8_exact(M, N, K, height):
    """diag(sp) (Pq Qq^T) diag(sq) + P2 Q2^T (+ C) with power-of-two row scales: the kernel's parking of the LoRA term as
    lora / (sp sq) under the e4m3 sums and its epilogue acc sp sq only move exponents, so the bits are the float64
    statement's here too."""
    _lib, lib, st = _env()
    g = _gen(M, N, K, 4)
    assert lib.msr3d_fp8_gemm_tile(M, N) == height
    Pi, Pq, ldp = _fp8_block(g, M, K)
    Qi, Qq, ldq = _fp8_block(g, N, K)
    sp = (2.0 ** torch.randint(-3, 2, (M,), device="cuda", generator=g).double()).float()
    sq = (2.0 ** torch.randint(-3, 2, (N,), device="cuda", generator=g).double()).float()
    P2, ldp2 = _block(_int_bf16(g, M, 72), 64, 8)
    Q2, ldq2 = _block(_int_bf16(g, N, 80), 64, 16)
    C0 = _int_bf16(g, M, N)
    main = (Pi * sp.double()[:, None]) @ (Qi * sq.double()[:, None]).t()
    low = P2.double() @ Q2.double().t()
    out, C, ldc = _out2d(M, N, torch.bfloat16)
    for lora in (False, True):
        for accumulate in (False, True):
            want = (main + (low if lora else 0) + (C0.double() if accumulate else 0)).to(torch.bfloat16)
            for launch in range(LAUNCHES):
                out.reset()
                if accumulate:
                    C.copy_(C0)
                fn, rc = _fp8_launch(lib, st, accumulate, M, N, K, Pq, ldp, sp, Qq, ldq, sq, P2 if lora else None, ldp2,
                                     Q2 if lora else None, ldq2, C, ldc)
                _lib.check(rc, fn)
                _same_bits(C, want, f"lora {lora}, accumulate {accumulate}, launch {launch}")
                assert out.untouched_outside_blocks(), f"lora {lora}, accumulate {accumulate}, launch {launch}: wrote outside C"


@pytest.mark.parametrize("M,N,K,height", G.RANDOM_FP8, ids=_ids(G.RANDOM_FP8))
def test_fp8_random_operands_against_float64_on_the_dequantised_operands(M, N, K, height):
    from msr3d_amd.llm.lora import quant_rows_fp8
    _lib, lib, st = _env()
    g = _gen(M, N, K, 5)
    assert lib.msr3d_fp8_gemm_tile(M, N) == height
    x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
    (xq, sx), (wq, sw) = quant_rows_fp8(x), quant_rows_fp8(w)
    u, b2 = torch.zeros(M, 64, device="cuda", dtype=torch.bfloat16), torch.zeros(N, 64, device="cuda", dtype=torch.bfloat16)
    u[:, :16] = (torch.randn(M, 16, device="cuda", generator=g) * 0.3).to(torch.bfloat16)
    b2[:, :16] = (torch.randn(N, 16, device="cuda", generator=g) * 0.3).to(torch.bfloat16)
    table = _e4m3_table()
    want = (table[xq.long()] * sx.double()[:, None]) @ (table[wq.long()] * sw.double()[:, None]).t() + u.double() @ b2.double().t()
    C0 = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    out, C, ldc = _out2d(M, N, torch.bfloat16)
    for accumulate in (False, True):
        out.reset()
        if accumulate:
            C.copy_(C0)
        fn, rc = _fp8_launch(lib, st, accumulate, M, N, K, xq, K, sx, wq, K, sw, u, 64, b2, 64, C, ldc)
        _lib.check(rc, fn)
        ref = want + C0.double() if accumulate else want
        err = float((C.double() - ref).norm() / ref.norm())
        print(f"accumulate {accumulate}: rel-L2 {err:.3e}")
        assert err < 4e-3              # tests/test_lora_fp8_gpu.py's bound for this result
        assert out.untouched_outside_blocks()


# ------------------------------------------------------------------------------- MSR3D_BF16_GEMM = reg, glds (per process)
def test_the_switches_reg_and_glds_in_child_processes():
    """MSR3D_BF16_GEMM is read once per process: the bf16 cases of this file again in a child pytest under `reg`, then under
    `glds`.  Every case takes its expectation from the path query and the restated rule, so it checks the kernel the switch
    sends it to (the accumulate and e4m3 entries never consult the switch and are left out, as is this test)."""
    me = os.path.join("tests", os.path.basename(__file__))
    for value in ("reg", "glds"):
        env = dict(os.environ, MSR3D_GPU_INPROC="1", MSR3D_BF16_GEMM=value)
        env.pop("MSR3D_GPU_CHILD", None)                    # (the child reports to this test, not to the suite's runner)
        out = subprocess.run([sys.executable, "-m", "pytest", me, "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                              "-k", "test_bf16_ and not child_processes"], env=env, cwd=ROOT, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0 and " passed" in out.stdout, f"MSR3D_BF16_GEMM={value}\n" + out.stdout[-3000:] + out.stderr[-1000:]
