"""msr3d_lora_merge (csrc/lora_merge.hip) against its float64 statement.

    out[n][k] = bf16_rne( W[n][k] + s * sum_r B[n][r] A[r][k] ),  the sum in fp32, in any order

The yardstick: ref = W + s (B @ A) in float64; the window e = (r + 2) 2^-24 (|W| + s (|B| @ |A|)) bounds an r-term fp32
dot product plus the final add in any order (r products or fused steps, r - 1 adds, the scale / final add: at most r + 2
roundings on any term); lo = bf16_rne(ref - e), hi = bf16_rne(ref + e), both rounded from float64 DIRECTLY (no detour
through fp32: `bf16_rne_f64`); an element passes if its bits equal lo or hi.  A condition on the INPUTS, asserted: at most
1 % of a job's elements may have lo != hi (a window astride a rounding boundary decides nothing there).
Where W and the update cancel to nearly nothing the window is wider than one bf16 step of the tiny result (a handful
of elements per million with random signs) and lo and hi are not neighbours: there every bf16 value from lo to hi is the
rounding of a point of the window -- bf16_rne(ref) itself is neither lo nor hi -- so the test reads "equals lo or hi" as
lo <= value <= hi in bf16 order, which is the same statement wherever lo and hi are equal or adjacent.

Cases: the smallest at which tiling (128-column x 128-row wave tiles, 16-row steps), the job table and both ranks can go
wrong -- one tile; several column blocks; several row and column blocks; one launch of five jobs of mixed shapes (rows no
multiple of 16, columns no multiple of 128, both ranks, both scales, padded `out` rows); B = 0; an update four times the
weight; two runs; the rejections.  The CPU test holds the yardstick itself against torch's fp32 arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

CAP = 0.01


def bf16_rne_f64(x):
    """float64 ndarray -> the bits (uint16) of the nearest bf16, ties to even, rounded from the float64 directly."""
    x = np.asarray(x, dtype=np.float64)
    mag = np.abs(x)
    t = (mag.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).astype(np.int64)      # near |x|, a bf16 pattern
    best, best_d = None, None
    for step in (-1, 0, 1):                      # the fp32 detour can land one bf16 away from the bracket: three candidates
        c = np.clip(t + step * 0x10000, 0, 0x7F800000)
        d = np.abs(c.astype(np.uint32).view(np.float32).astype(np.float64) - mag)
        if best is None:
            best, best_d = c, d
        else:
            even = ((c >> 16) & 1) == 0
            take = (d < best_d) | ((d == best_d) & even & (c != best))
            best, best_d = np.where(take, c, best), np.where(take, d, best_d)
    return ((best >> 16) | np.where(np.signbit(x), 0x8000, 0)).astype(np.uint16)


def ordered(bits):
    """uint16 bf16 bits -> int32 keys in the order of the values they encode (-0 and +0 both 0)."""
    b = bits.astype(np.int32)
    return np.where(b >= 0x8000, 0x8000 - b, b)


def bits_of(t):
    """bf16 tensor -> uint16 ndarray of its bits."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def window(W, A, B, s):
    """-> (lo, hi) uint16 bits for W (N, K) bf16 tensor, A (r, K), B (N, r) fp32 tensors."""
    Wd, Ad, Bd = W.double().numpy(), A.double().numpy(), B.double().numpy()
    ref = Wd + s * (Bd @ Ad)
    e = (A.shape[0] + 2) * 2.0 ** -24 * (np.abs(Wd) + s * (np.abs(Bd) @ np.abs(Ad)))
    return bf16_rne_f64(ref - e), bf16_rne_f64(ref + e)


def job(seed, N, K, r, scale, ratio=0.5, pad=0):
    """Seeded inputs: W ~ 0.02 N(0, 1) as bf16; A uniform in +-1 / sqrt(K) (peft's init); B normal, scaled so that the
    mean |s B A| is `ratio` x the mean |W| (0: B = 0)."""
    g = torch.Generator().manual_seed(seed)
    W = (0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    A = ((torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5).float()
    B = torch.randn(N, r, generator=g).float()
    if ratio == 0:
        B.zero_()
    else:
        B *= ratio * float(W.float().abs().mean()) / (scale * float((B @ A).abs().mean()))
    return dict(W=W, A=A, B=B, scale=float(scale), r=r, ldo=K + pad)


CASES = {
    "one_tile": [job(1, 64, 128, 16, 1.0)],
    "column_blocks_r32": [job(2, 192, 1024, 32, 2.0)],
    "row_and_column_blocks": [job(3, 1024, 512, 16, 1.0)],
    "five_mixed": [job(4, 64, 128, 16, 1.0, pad=8), job(5, 80, 72, 32, 2.0, pad=24), job(6, 192, 1024, 32, 1.0, pad=8),
                   job(7, 273, 392, 16, 2.0, pad=16), job(8, 1024, 512, 16, 1.0, pad=8)],
    "update_4x_weight": [job(9, 64, 128, 16, 1.0, ratio=4.0), job(10, 192, 1024, 16, 2.0, ratio=4.0)],
}
_windows = {}


def windows(name):
    if name not in _windows:
        _windows[name] = [window(j["W"], j["A"], j["B"], j["scale"]) for j in CASES[name]]
    return _windows[name]


def check(name, outs):
    """outs: per job the (N, K) uint16 bits -> asserts the cap on the inputs and lo / hi membership of every element."""
    for n, (j, (lo, hi), got) in enumerate(zip(CASES[name], windows(name), outs)):
        open_share = float((lo != hi).mean())
        bad = (ordered(got) < ordered(lo)) | (ordered(got) > ordered(hi))
        far = int((ordered(hi) - ordered(lo) > 1).sum())
        print("%s job %d (%d x %d, r %d, s %g): lo != hi on %.3f %% of the elements (%d of them not neighbours); outside "
              "the window: %d" % (name, n, *j["W"].shape, j["r"], j["scale"], 100 * open_share, far, int(bad.sum())))
        assert open_share <= CAP, "the inputs leave too many elements undecided"
        assert not bad.any(), (name, n, np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_yardstick_accepts_torch_fp32_arithmetic(name):
    """The window itself, on the CPU: torch's (W.float() + s B @ A).bfloat16() lies inside it on every case, and the
    direct float64 -> bf16 rounding agrees with torch where no double rounding can occur (bf16 -> bf16, fp32 -> bf16)."""
    outs = [bits_of((j["W"].float() + j["scale"] * (j["B"] @ j["A"])).to(torch.bfloat16)) for j in CASES[name]]
    check(name, outs)
    j = CASES[name][0]
    assert np.array_equal(bf16_rne_f64(j["W"].double().numpy()), bits_of(j["W"]))
    assert np.array_equal(bf16_rne_f64(j["A"].double().numpy()), bits_of(j["A"].to(torch.bfloat16)))


def test_update_case_really_exceeds_the_weight():
    for j in CASES["update_4x_weight"]:
        ratio = float((j["scale"] * (j["B"] @ j["A"])).abs().mean() / j["W"].float().abs().mean())
        assert 3.9 < ratio < 4.1, ratio


# ------------------------------------------------------------------------------------------------------------- GPU
SENTINEL = 0x7FC1           # a NaN pattern no merge produces: what `out` holds before the launch


def _table(entries):
    from msr3d_amd import _lib
    arr = (_lib.LoraMergeJob * len(entries))(*[_lib.LoraMergeJob(*e) for e in entries])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def run_merge(jobs):
    """One launch over `jobs` -> per job the whole (N, ldo) uint16 buffer."""
    from msr3d_amd import _lib
    dev, keep, entries, outs = torch.device("cuda"), [], [], []
    for j in jobs:
        W, A, B = j["W"].cuda().contiguous(), j["A"].cuda().contiguous(), j["B"].cuda().contiguous()
        N, K = W.shape
        out = torch.full((N, j["ldo"]), SENTINEL, dtype=torch.int32).to(torch.int16).cuda()
        keep += [W, A, B]
        outs.append(out)
        entries.append((W.data_ptr(), A.data_ptr(), B.data_ptr(), out.data_ptr(), j["ldo"], j["r"], N, K, j["scale"], 0))
    tab = _table(entries)
    rc = _lib.load().msr3d_lora_merge(len(entries), ctypes.c_void_p(tab.data_ptr()), _lib.current_stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint16) for o in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_merge_kernel_inside_the_float64_window(name):
    full = run_merge(CASES[name])
    check(name, [o[:, :j["W"].shape[1]] for o, j in zip(full, CASES[name])])
    for o, j in zip(full, CASES[name]):                           # the padding columns of `out` stay untouched
        assert (o[:, j["W"].shape[1]:] == SENTINEL).all()


@pytest.mark.gpu
def test_zero_B_returns_the_weight_and_two_runs_give_the_same_bits():
    j = job(11, 192, 1024, 32, 2.0, ratio=0)
    assert np.array_equal(run_merge([j])[0], bits_of(j["W"]))
    a, b = run_merge(CASES["five_mixed"]), run_merge(CASES["five_mixed"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_bad_jobs_are_rejected_before_anything_is_written():
    from msr3d_amd import _lib
    h, st = _lib.load(), _lib.current_stream_ptr(torch.device("cuda"))
    W = torch.zeros((64, 128), dtype=torch.bfloat16, device="cuda")
    A, B = torch.zeros((32, 128), device="cuda"), torch.zeros((64, 32), device="cuda")
    out = torch.full((64, 128), SENTINEL, dtype=torch.int32).to(torch.int16).cuda()
    good = (W.data_ptr(), A.data_ptr(), B.data_ptr(), out.data_ptr(), 128, 16, 64, 128, 1.0, 0)

    def rc(*entries):
        tab = _table(entries)
        return h.msr3d_lora_merge(len(entries), ctypes.c_void_p(tab.data_ptr()), st)

    def edit(**kw):
        names = ("W", "A", "B", "out", "ldo", "r", "N", "K", "scale", "pad_")
        return tuple(kw.get(n, v) for n, v in zip(names, good))

    assert rc(edit(r=8)) == -22
    assert rc(edit(K=124, ldo=128)) == -22                                    # K % 8 != 0
    assert rc(edit(out=W.data_ptr())) == -22                                  # out aliases W
    assert rc(edit(out=W.data_ptr() + 2 * 128 * 16, N=32)) == -22             # ... or overlaps its tail
    assert rc(good, edit(r=8)) == -22                                         # one bad job refuses the launch
    assert h.msr3d_lora_merge(1, ctypes.c_void_p(0), st) == -22               # NULL table with njobs > 0
    assert h.msr3d_lora_merge(-1, ctypes.c_void_p(0), st) == -22
    assert h.msr3d_lora_merge(0, ctypes.c_void_p(0), st) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == out.view(torch.int16)[0, 0]).all()), "a refused call wrote through a job"
    assert rc(good) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.bfloat16) == 0).all())
