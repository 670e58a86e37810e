"""The shapes tests/test_gemm_paths_gpu.py launches, each with the kernel it is there to pin, and a restatement of the
selection rule of csrc/lora_linear.hip (gemm_path) / csrc/lora_fp8.hip in plain Python.  tests/test_gemm_paths_cpu.py
holds the library's answer (msr3d_bf16_gemm_path, msr3d_bf16_gemm_acc_tile, msr3d_fp8_gemm_tile) against both, so an
edit to the rule cannot silently move a case to another kernel.

Paths: 0 = bf16_gemm_kernel<128>, 1 = bf16_gemm_kernel<192>, 2 = bf16_gemm_glds_kernel<192>, 8 / 9 / 10 = the wide-tile
kernel at tile height 128 / 144 / 160."""
import os

REG128, REG192, GLDS192, WIDE128, WIDE144, WIDE160 = 0, 1, 2, 8, 9, 10
PATH_NAMES = {0: "reg128", 1: "reg192", 2: "glds192", 8: "wide128", 9: "wide144", 10: "wide160"}
ALL_PATHS = set(PATH_NAMES)
HEIGHTS = {128, 144, 160}


def mode_from_env():
    """MSR3D_BF16_GEMM as the library reads it: first letter r -> reg, g -> glds, anything else -> wide."""
    e = os.environ.get("MSR3D_BF16_GEMM", "")
    return "reg" if e[:1] == "r" else "glds" if e[:1] == "g" else "wide"


def wide_height(M, N, batch=1):
    """The tile height with the least (rounds of 256 CUs) x height; the taller one on a tie."""
    tn = -(-N // 256)
    cost = {h: -(-(-(-M // h) * tn * batch) // 256) * h for h in (160, 144, 128)}
    return min((160, 144, 128), key=lambda h: (cost[h], -h))


def rule(M, N, R, batch=1, mode="wide", ldp=0, ldq=0, ldp2=0, ldq2=0):
    if (mode == "wide" and M >= 128 and N >= 256 and R % 64 == 0 and M * ldp < 2 ** 31 and N * ldq < 2 ** 31
            and (R == 0 or (M * ldp2 < 2 ** 31 and N * ldq2 < 2 ** 31))):
        h = wide_height(M, N, batch)
        if -(-M // h) * -(-N // 256) * batch >= 128:
            return h // 16
    if mode in ("wide", "glds") and M >= 192 and R % 64 == 0:
        return GLDS192
    w128, w192 = -(-M // 128) * 128, -(-M // 192) * 192
    return REG192 if (M >= 192 and w192 <= w128) else REG128


# ---- msr3d_bf16_gemm_lowrank: (M, N, K, R, path under the default mode) ------------------------------------------------
# the (K, R) set every wide height meets: nk = 1, 2, 2 (second stage the low-rank pair), 3, 4, the steady loop, and two
# low-rank stages
WIDE_KR = [(64, 0), (128, 0), (64, 64), (128, 64), (192, 64), (1024, 64), (64, 128)]
# one (M, N) per height for that cross: the ragged ones (1273 = 7 x 160 + 153, N % 4 == 2: the scalar column tail)
WIDE_CROSS = {WIDE160: (1273, 8186), WIDE144: (1145, 8190), WIDE128: (1000, 4096)}
LOWRANK = [(M, N, K, R, p) for p, (M, N) in WIDE_CROSS.items() for K, R in WIDE_KR]
LOWRANK += [
    (1280, 8192, 1024, 64, WIDE160),          # 8 x 32 = 256 tiles: one round
    (800, 11008, 1024, 64, WIDE160),          # 43 column tiles, 215 tiles: both remainders of the patch numbering
    (800, 11008, 64, 0, WIDE160),
    (2560, 4096, 4096, 64, WIDE160),          # 4 sequences x 640 tokens against a 4096 x 4096 projection
    (1152, 8192, 1024, 64, WIDE144),
    (1152, 8192, 128, 0, WIDE144),
    (1024, 8192, 1024, 64, WIDE128),
    (1024, 8192, 128, 64, WIDE128),
]
LOWRANK += [(200, N, K, R, GLDS192) for N in (300, 298) for R in (0, 64) for K in (64, 128, 192)]
LOWRANK += [(257, 130, 64, 16, REG192), (257, 130, 192, 16, REG192), (384, 136, 128, 32, REG192),
            (130, 72, 64, 16, REG128), (130, 72, 128, 8, REG128), (100, 520, 192, 64, REG128), (100, 520, 64, 64, REG128)]

# ---- msr3d_bf16_gemm_lowrank_acc: (M, N, K, R, height) ---------------------------------------------------------------------
ACC = [(M, N, K, R, h) for M, N, h in [(1280, 8192, 160), (1273, 8188, 160), (1152, 8192, 144), (1145, 8188, 144),
                                       (1024, 8192, 128), (1000, 4096, 128)]
       for K, R in ([(1024, 64), (64, 0)] if M % 16 == 0 else [(128, 64), (192, 0), (64, 64)])]

# ---- msr3d_bf16_gemm_batched: name -> (outer, inner, M, N, K, path) ----------------------------------------------------------
BATCHED = {
    "head_backward": (5, 1, 260, 4096, 128, WIDE128),      # FrozenLinear's split-reduction dx: 5 chunks of the reduction
    "attention": (4, 8, 576, 576, 128, WIDE128),            # (B, T, H, D) operands, one product per sequence and head
    "small": (2, 3, 100, 200, 64, REG128),
}

# ---- msr3d_fp8_gemm_lowrank(_acc): (M, N, K, height); each with the LoRA pair on / off and accumulate on / off --------------
FP8_SHAPES = [(1280, 8192, 160), (1273, 8188, 160), (1152, 8192, 144), (1145, 8188, 144), (1024, 8192, 128), (300, 512, 128)]
FP8 = [(M, N, K, h) for M, N, h in FP8_SHAPES for K in (128, 256, 384, 1024)]

# ---- one random-operand case per path: (M, N, K, R, path) ------------------------------------------------------------------
RANDOM = [(1273, 8186, 1024, 64, WIDE160), (1145, 8190, 1024, 64, WIDE144), (1000, 4096, 1024, 64, WIDE128),
          (200, 298, 192, 64, GLDS192), (257, 130, 192, 16, REG192), (130, 72, 128, 16, REG128)]
RANDOM_ACC = [(1273, 8188, 1024, 64, 160), (1145, 8188, 1024, 64, 144), (1000, 4096, 1024, 64, 128)]
RANDOM_FP8 = [(1273, 8188, 1024, 160), (1145, 8188, 1024, 144), (300, 512, 1024, 128)]

# ---- what the rest of the suite launches (tests/test_lora_gpu.py, test_lora_fp8_gpu.py), as (M, N, R, path) -----------------
# test_wide_gemm_exact_on_integer_operands_run_after_run
SUITE_RACE_SCREEN = [(2304, 4096, 64, WIDE144), (2304, 1024, 0, GLDS192), (1000, 4096, 0, WIDE128), (4600, 512, 64, GLDS192),
                     (144, 256, 0, REG128)]
# test_lora_linear_matches_the_float64_formulation: forward (M, N, 64) and dx (M, K, 64) of each (M, K, N)
SUITE_LORA_LINEAR = [(2304, 4096, 64, WIDE144), (300, 11008, 64, WIDE128), (300, 4096, 64, GLDS192), (129, 4096, 64, REG128),
                     (129, 11008, 64, REG128), (64, 192, 64, REG128), (64, 256, 64, REG128), (4000, 256, 64, GLDS192),
                     (4000, 512, 64, GLDS192),
                     (2560, 4096, 64, WIDE160), (2560, 11008, 64, WIDE160)]      # the two M = 2560 cases
SUITE_ACC = [(2304, 4096, 144), (300, 512, 128)]
SUITE_FP8 = [(2304, 4096, 144), (300, 512, 128), (144, 256, 128), (2304, 11008, 144), (11520, 4096, 144), (6000, 4096, 128),
             (5000, 11008, 144), (2560, 4096, 160)]
