"""CPU: which kernel the bf16 and e4m3 projection GEMMs launch for a shape (msr3d_bf16_gemm_path,
msr3d_bf16_gemm_acc_tile, msr3d_fp8_gemm_tile: the host-only functions the launch code itself calls).  Every shape
tests/test_gemm_paths_gpu.py launches maps to the kernel it is listed under in tests/gemm_path_cases.py, the listed shapes
reach all six bf16 kernels and all three wide-tile heights of the accumulate and e4m3 entries, and the library's answer is
the rule as tests/gemm_path_cases.py restates it, under each value of MSR3D_BF16_GEMM (read once per process: the other
two values are asked of a child interpreter, no device involved)."""
import json
import os
import subprocess
import sys

from tests import gemm_path_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from msr3d_amd import _lib
    return _lib.load()


def _bf16_queries():
    """(M, N, R, batch, ldp, ldq, ldp2, ldq2, stated path) of every bf16 product the listed cases launch."""
    out = []
    for M, N, K, R, p in G.LOWRANK + G.RANDOM:
        out.append((M, N, R, 1, K + 72, K + 136, R + 24, R + 8, p))
    for outer, inner, M, N, K, p in G.BATCHED.values():
        out.append((M, N, 0, outer * inner, outer * inner * K, outer * inner * K, 0, 0, p))
    for M, N, R, p in G.SUITE_RACE_SCREEN + G.SUITE_LORA_LINEAR:
        out.append((M, N, R, 1, 4096, 4096, 64, 64, p))
    return out


def test_every_listed_shape_takes_the_kernel_it_is_listed_under():
    lib = _lib()
    mode = G.mode_from_env()
    for M, N, R, batch, ldp, ldq, ldp2, ldq2, stated in _bf16_queries():
        got = lib.msr3d_bf16_gemm_path(M, N, R, batch, ldp, ldq, ldp2, ldq2)
        assert got == G.rule(M, N, R, batch, mode, ldp, ldq, ldp2, ldq2), (M, N, R, batch, got)
        if mode == "wide":
            assert got == stated, (M, N, R, batch, G.PATH_NAMES.get(got, got), G.PATH_NAMES[stated])
    for M, N, _, _, h in G.ACC + G.RANDOM_ACC:
        assert lib.msr3d_bf16_gemm_acc_tile(M, N) == h == G.wide_height(M, N), (M, N)
    for M, N, h in G.SUITE_ACC:
        assert lib.msr3d_bf16_gemm_acc_tile(M, N) == h == G.wide_height(M, N), (M, N)
    for M, N, _, h in G.FP8 + G.RANDOM_FP8:
        assert lib.msr3d_fp8_gemm_tile(M, N) == h == G.wide_height(M, N), (M, N)
    for M, N, h in G.SUITE_FP8:
        assert lib.msr3d_fp8_gemm_tile(M, N) == h == G.wide_height(M, N), (M, N)


def test_the_listed_shapes_reach_every_kernel_and_every_height():
    assert {p for *_, p in G.LOWRANK} == G.ALL_PATHS              # exact cases
    assert {p for *_, p in G.RANDOM} == G.ALL_PATHS               # random-operand cases
    assert {h for *_, h in G.ACC} == {h for *_, h in G.RANDOM_ACC} == G.HEIGHTS
    assert {h for *_, h in G.FP8} == {h for *_, h in G.RANDOM_FP8} == G.HEIGHTS
    # every wide height meets every (K, R) of the prologue / steady-loop set
    for p in (G.WIDE128, G.WIDE144, G.WIDE160):
        assert {(K, R) for _, _, K, R, q in G.LOWRANK if q == p} >= set(G.WIDE_KR)
    # the batched forms: the wide kernel under blockIdx.z, and the small tile
    assert {p for *_, p in G.BATCHED.values()} == {G.WIDE128, G.REG128}
    # the patch numbering's remainders: a tile count that is no multiple of 8, column tiles no multiple of 4
    assert any(p >= 8 and (-(-M // (16 * p)) * -(-N // 256)) % 8 and -(-N // 256) % 4 for M, N, _, _, p in G.LOWRANK)


def test_a_step_of_four_640_token_sequences_takes_height_160():
    lib = _lib()
    for N in (4096, 11008):
        if G.mode_from_env() == "wide":
            assert lib.msr3d_bf16_gemm_path(2560, N, 64, 1, 11008, 11008, 64, 64) == G.WIDE160
        assert lib.msr3d_bf16_gemm_acc_tile(2560, N) == 160
        assert lib.msr3d_fp8_gemm_tile(2560, N) == 160
    # before the two M = 2560 cases, the module-level tests reached every kernel but that height and reg192
    assert {p for *_, p in G.SUITE_LORA_LINEAR[:-2]} == {G.WIDE144, G.WIDE128, G.GLDS192, G.REG128}
    assert {p for *_, p in G.SUITE_RACE_SCREEN} == {G.WIDE144, G.WIDE128, G.GLDS192, G.REG128}
    assert {h for *_, h in G.SUITE_ACC} == {h for *_, h in G.SUITE_FP8[:-1]} == {144, 128}


def test_rule_edges_and_refusals():
    lib = _lib()
    q = lambda M, N, R=0, batch=1, ld=4096: lib.msr3d_bf16_gemm_path(M, N, R, batch, ld, ld, 64, 64)   # noqa: E731
    mode = G.mode_from_env()
    for M, N, R, batch in [(1000, 4096, 0, 1),           # 128 tiles: the fewest the wide kernel takes
                           (896, 4096, 0, 1),            # 112: below it
                           (127, 8192, 0, 8), (128, 8192, 0, 8), (1024, 255, 0, 64), (191, 300, 64, 1), (192, 300, 64, 1),
                           (192, 300, 16, 1), (256, 130, 16, 1), (257, 130, 16, 1), (385, 130, 8, 1), (576, 576, 0, 32)]:
        assert q(M, N, R, batch) == G.rule(M, N, R, batch, mode, 4096, 4096, 64, 64), (M, N, R, batch)
    if mode == "wide":
        assert q(1000, 4096) == G.WIDE128 and q(896, 4096) == G.GLDS192
        # operands past the wide kernel's 32-bit element offsets go to the kernels with 64-bit ones
        assert lib.msr3d_bf16_gemm_path(200000, 4096, 0, 1, 11008, 4096, 0, 0) == G.GLDS192
    for bad in [(0, 256, 0, 1), (256, 0, 0, 1), (256, 256, -8, 1), (256, 256, 0, 0)]:
        assert q(*bad) == -22
    assert lib.msr3d_bf16_gemm_acc_tile(0, 256) == -22 and lib.msr3d_fp8_gemm_tile(256, 0) == -22


_CHILD = """
import json, sys
sys.path.insert(0, %r)
from msr3d_amd import _lib
lib = _lib.load()
print(json.dumps([lib.msr3d_bf16_gemm_path(*q) for q in json.loads(sys.argv[1])]))
"""


def test_the_per_process_switch_moves_the_query_as_the_rule_says():
    queries = [q[:8] for q in _bf16_queries()]
    for value in ("reg", "glds", "wide"):
        out = subprocess.run([sys.executable, "-c", _CHILD % ROOT, json.dumps(queries)], cwd=ROOT, capture_output=True, text=True,
                             env=dict(os.environ, MSR3D_BF16_GEMM=value), timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        got = json.loads(out.stdout.strip().splitlines()[-1])
        assert got == [G.rule(M, N, R, b, value, lp, lq, lp2, lq2) for M, N, R, b, lp, lq, lp2, lq2 in queries], value
        assert (value != "reg") or set(got) <= {G.REG128, G.REG192}
        assert (value != "glds") or set(got) <= {G.REG128, G.REG192, G.GLDS192}
