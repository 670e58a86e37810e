// lora_linear.hip -- a LoRA-augmented linear layer of the frozen bf16 language model
// (/root/reference/model/msr3d/msr3d.py:103-112: peft LoraConfig r = 16, alpha = 16, dropout 0 on
// q/k/v/o/gate/up/down_proj; the LLM runs under bf16 autocast, msr3d.py:409-415):
//
//     y = x W^T + s (x A^T) B^T                     W (N,K) frozen bf16, A (r,K), B (N,r) trainable
//     dx = dy W + s (dy B) A        dA = s (dy B)^T x        dB = s dy^T (x A^T)         (no dW)
//
// One bf16 MFMA kernel (v_mfma_f32_16x16x32_bf16, fp32 accumulate) serves forward and dx:
//
//     C (M,N) = P Q^T + P2 Q2^T        P (M,K), Q (N,K), P2 (M,R), Q2 (N,R): all k-contiguous bf16
//
// i.e. the low-rank term rides as ONE extra K step of the same product (P2 = s x A^T computed by a
// first call of the same kernel against the zero-padded A; R = 32).  The frozen weight is kept in
// BOTH orientations (W for the forward, W^T for dx): 13 GB extra for a 7B model, which is what a
// 288 GB part is for -- no transposing load path, both products read k-contiguous rows.
// 192 x 128 (or 128 x 128) tile, BK = 64, one LDS stage + register prefetch, 4 waves of 96 x 64 (6 x 4 MFMA
// tiles); msr3d_bf16_gemm_batched: the same kernel over a batch (attention's per-head products).  The weight gradients' token reduction (M = a few thousand, output r x K / N x r) is a
// column-per-thread VALU kernel: it is bound by reading x / dy once.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "../../include/msr3d_hip.h"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int BN = 128, BK = 64;
constexpr int LD = BK + 8;                 // bf16 units: row stride 144 B (conflict-free 16-byte fragment reads)

__device__ __forceinline__ unsigned short f2bf(float f) {        // round to nearest even
  unsigned u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

struct GemmArgs {
  int M, N, K, R;
  const unsigned short *P; int ldp;
  const unsigned short *Q; int ldq;
  const unsigned short *P2; int ldp2;
  const unsigned short *Q2; int ldq2;
  void *C; int ldc; int c_f32;
  int accumulate;                          // wide kernel, bf16 C only: C += the product
  float scale;                             // applied to the whole result (the forward's u = s x A^T)
  int inner;                               // blockIdx.z = outer * inner + inner index (e.g. sequence, head)
  long long spo, spi, sqo, sqi, sco, sci;   // batch strides (elements) of P, Q, C, outer and inner
};

// ROWS x 64 k of a row-major bf16 matrix -> registers: 16 B per thread and pass (row = t/8 + 32 j, k8 = t%8)
template <int ROWS>
__device__ __forceinline__ void tile_load(uint4 (&r)[ROWS / 32], const unsigned short *__restrict__ S, int ld, int row0,
                                          int rows, int k0, int kmax) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < ROWS / 32; ++j) {
    const int row = min(row0 + (t >> 3) + 32 * j, rows - 1), k = k0 + (t & 7) * 8;
    r[j] = k < kmax ? *reinterpret_cast<const uint4 *>(S + (size_t)row * ld + k) : make_uint4(0, 0, 0, 0);
  }
}
template <int ROWS>
__device__ __forceinline__ void tile_store(unsigned short *L, const uint4 (&r)[ROWS / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < ROWS / 32; ++j)
    *reinterpret_cast<uint4 *>(L + ((t >> 3) + 32 * j) * LD + (t & 7) * 8) = r[j];
}

// BM x 128 tile, 4 waves as 2 x 2, each (BM / 2) x 64 = MT x 4 MFMA tiles.  BM = 192 is the shape for the
// language model's token counts (4 x 576 = 2304 = 12 x 192): 6 x 4 tiles per wave read 10 fragments per 24
// MFMAs -- the 64 x 64 sub-tile of the 128 x 128 variant reads 8 per 16, which with two workgroups per CU is
// exactly the LDS's 128 B/clk (round 2: 275 TFLOP/s, the 576 tiles of 2304 x 4096 also being 1.125 rounds of
// the chip's 512 slots).  The accumulators are transposed (D = Q P^T: a lane holds FOUR CONSECUTIVE output
// columns of one row), so the epilogue is one 8-byte (bf16) or 16-byte (fp32) store per tile instead of four
// scattered 2-byte ones.  Single LDS stage + register prefetch: next tile's loads fly under this tile's MFMAs.
template <int BM>
__global__ __launch_bounds__(256, 2) void bf16_gemm_kernel(const GemmArgs a) {
  constexpr int MT = BM / 32;                    // 16-row tiles per wave
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  unsigned short *As = lds, *Bs = lds + BM * LD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int bo = blockIdx.z / a.inner, bi = blockIdx.z - bo * a.inner;
  const unsigned short *P = a.P + bo * a.spo + bi * a.spi, *Q = a.Q + bo * a.sqo + bi * a.sqi;

  f32x4 acc[MT][4];
#pragma unroll
  for (int x = 0; x < MT; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the K walk: main operands, then (if R > 0) the low-rank pair as extra stages
  const int nk_main = a.K / BK, nk = nk_main + (a.R + BK - 1) / BK;
  uint4 ra[BM / 32], rb[BN / 32];
  auto fetch = [&](int kt) {
    if (kt < nk_main) {
      tile_load<BM>(ra, P, a.ldp, m0, a.M, kt * BK, a.K);
      tile_load<BN>(rb, Q, a.ldq, n0, a.N, kt * BK, a.K);
    } else {
      const int k0 = (kt - nk_main) * BK;
      tile_load<BM>(ra, a.P2, a.ldp2, m0, a.M, k0, a.R);
      tile_load<BN>(rb, a.Q2, a.ldq2, n0, a.N, k0, a.R);
    }
  };
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    tile_store<BM>(As, ra);
    tile_store<BN>(Bs, rb);
    __syncthreads();
    if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 fa[MT], fb[4];
#pragma unroll
      for (int y = 0; y < 4; ++y)
        fb[y] = *reinterpret_cast<const bf16x8 *>(Bs + (wn * 64 + y * 16 + i) * LD + ks * 32 + g * 8);
#pragma unroll
      for (int x = 0; x < MT; ++x)
        fa[x] = *reinterpret_cast<const bf16x8 *>(As + (wm * (BM / 2) + x * 16 + i) * LD + ks * 32 + g * 8);
#pragma unroll
      for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
          acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[y], fa[x], acc[x][y], 0, 0, 0);
    }
    __syncthreads();
  }
  // epilogue: D = Q P^T -- lane (i, g) holds columns n = 4 g + r of row m = i
#pragma unroll
  for (int x = 0; x < MT; ++x) {
    const int row = m0 + wm * (BM / 2) + x * 16 + i;
    if (row >= a.M) continue;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int col = n0 + wn * 64 + y * 16 + 4 * g;
      if (col >= a.N) continue;
      const float v0 = acc[x][y][0] * a.scale, v1 = acc[x][y][1] * a.scale, v2 = acc[x][y][2] * a.scale,
                  v3 = acc[x][y][3] * a.scale;
      const size_t o = (size_t)(bo * a.sco + bi * a.sci) + (size_t)row * a.ldc + col;
      if (col + 3 < a.N) {
        if (a.c_f32) *reinterpret_cast<float4 *>(reinterpret_cast<float *>(a.C) + o) = make_float4(v0, v1, v2, v3);
        else *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(a.C) + o) =
            make_uint2(f2bf(v0) | ((unsigned)f2bf(v1) << 16), f2bf(v2) | ((unsigned)f2bf(v3) << 16));
      } else {
        const float vv[4] = {v0, v1, v2, v3};
        for (int r = 0; r < 4 && col + r < a.N; ++r) {
          if (a.c_f32) reinterpret_cast<float *>(a.C)[o + r] = vv[r];
          else reinterpret_cast<unsigned short *>(a.C)[o + r] = f2bf(vv[r]);
        }
      }
    }
  }
}

// The same product with the operands staged by LDS-DMA (global_load_lds, 16 bytes per lane) into THREE LDS
// stages, two K steps in flight: the register-staged kernel above has one K step (768 cycles of MFMA) to
// cover a ~2k-cycle load, and its prefetch registers (40 per stage) leave no room for a second one.  The DMA
// writes wave-uniform base + lane x 16, so the LDS image is unpadded ([rows][64] bf16 = 8 chunks of 16 B per
// row) and the bank-conflict fix is on the SOURCE side: chunk c of row r is stored at position c ^ (r & 7), and
// the fragment read of lane (i, g) takes position (4 ks + g) ^ (i & 7) -- every ds_read_b128 lane group then
// covers sixteen distinct 16-byte slots of the 256-byte bank row.  One raw s_barrier per K step; the loads are
// retired by a counted vmcnt (this stage's 10 done, the next stage's 10 still flying), never by a full drain.
template <int BM>
__global__ __launch_bounds__(256, 1) void bf16_gemm_glds_kernel(const GemmArgs a) {
  constexpr int MT = BM / 32;
  constexpr int STAGE = (BM + BN) * BK;          // bf16 elements per stage
  constexpr int NA = BM * 8 / 256, NB = BN * 8 / 256;     // 16-byte chunks per thread and stage: 6 + 4
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int bo = blockIdx.z / a.inner, bi = blockIdx.z - bo * a.inner;
  const unsigned short *P = a.P + bo * a.spo + bi * a.spi, *Q = a.Q + bo * a.sqo + bi * a.sqi;

  f32x4 acc[MT][4];
#pragma unroll
  for (int x = 0; x < MT; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk_main = a.K / BK, nk = nk_main + (a.R + BK - 1) / BK;
  // per-thread source rows / chunks of the stage image (fixed over the K walk)
  const unsigned short *srcA[NA], *srcA2[NA], *srcB[NB], *srcB2[NB];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int q = tid + 256 * j, row = q >> 3, c = (q & 7) ^ (row & 7);
    const size_t r = (size_t)min(m0 + row, a.M - 1);
    srcA[j] = P + r * a.ldp + c * 8;
    srcA2[j] = a.R ? a.P2 + r * a.ldp2 + c * 8 : nullptr;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int q = tid + 256 * j, row = q >> 3, c = (q & 7) ^ (row & 7);
    const size_t r = (size_t)min(n0 + row, a.N - 1);
    srcB[j] = Q + r * a.ldq + c * 8;
    srcB2[j] = a.R ? a.Q2 + r * a.ldq2 + c * 8 : nullptr;
  }
  auto issue = [&](int kt) {                     // stage kt -> LDS buffer kt % 3
    unsigned short *buf = lds + (kt % 3) * STAGE;
    const bool main = kt < nk_main;
    const int k0 = main ? kt * BK : (kt - nk_main) * BK;
#pragma unroll
    for (int j = 0; j < NA; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((main ? srcA[j] : srcA2[j]) + k0),
                                       (__attribute__((address_space(3))) void *)(buf + (256 * j + 64 * wave) * 8), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < NB; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((main ? srcB[j] : srcB2[j]) + k0),
                                       (__attribute__((address_space(3))) void *)(buf + BM * BK + (256 * j + 64 * wave) * 8), 16, 0, 0);
  };
  issue(0);
  if (nk > 1) issue(1);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");      // stage kt landed; kt + 1 may still fly
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();               // ... for every wave; and every wave is done reading stage kt - 1
    if (kt + 2 < nk) issue(kt + 2);             // (into the buffer stage kt - 1 occupied)
    const unsigned short *As = lds + (kt % 3) * STAGE, *Bs = As + BM * BK;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int pos = ((4 * ks + g) ^ (i & 7)) * 8;
      bf16x8 fa[MT], fb[4];
#pragma unroll
      for (int y = 0; y < 4; ++y) fb[y] = *reinterpret_cast<const bf16x8 *>(Bs + (wn * 64 + y * 16 + i) * BK + pos);
#pragma unroll
      for (int x = 0; x < MT; ++x) fa[x] = *reinterpret_cast<const bf16x8 *>(As + (wm * (BM / 2) + x * 16 + i) * BK + pos);
#pragma unroll
      for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
          acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[y], fa[x], acc[x][y], 0, 0, 0);
    }
  }
  // epilogue: D = Q P^T -- lane (i, g) holds columns n = 4 g + r of row m = i
#pragma unroll
  for (int x = 0; x < MT; ++x) {
    const int row = m0 + wm * (BM / 2) + x * 16 + i;
    if (row >= a.M) continue;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int col = n0 + wn * 64 + y * 16 + 4 * g;
      if (col >= a.N) continue;
      const float v0 = acc[x][y][0] * a.scale, v1 = acc[x][y][1] * a.scale, v2 = acc[x][y][2] * a.scale,
                  v3 = acc[x][y][3] * a.scale;
      const size_t o = (size_t)(bo * a.sco + bi * a.sci) + (size_t)row * a.ldc + col;
      if (col + 3 < a.N) {
        if (a.c_f32) *reinterpret_cast<float4 *>(reinterpret_cast<float *>(a.C) + o) = make_float4(v0, v1, v2, v3);
        else *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(a.C) + o) =
            make_uint2(f2bf(v0) | ((unsigned)f2bf(v1) << 16), f2bf(v2) | ((unsigned)f2bf(v3) << 16));
      } else {
        const float vv[4] = {v0, v1, v2, v3};
        for (int r = 0; r < 4 && col + r < a.N; ++r) {
          if (a.c_f32) reinterpret_cast<float *>(a.C)[o + r] = vv[r];
          else reinterpret_cast<unsigned short *>(a.C)[o + r] = f2bf(vv[r]);
        }
      }
    }
  }
}

// ---- the wide-tile kernel: (16 MTB) x 256 tile, 8 waves side by side along N ----------------------------------
// The 4-wave kernels above keep one wave per SIMD in lockstep: every LDS-DMA piece a wave issues (~60-180 cycles
// of issue each, 10 per K step) and every wait at the K step's barrier is time its SIMD's matrix pipe idles.  Here
// a workgroup is 8 waves = two per SIMD, each owning ALL the tile's rows (MTB MFMA tiles) x 32 columns, so one
// wave's staging runs under the other's MFMAs, and the tile height is chosen per problem from {128, 144, 160} so
// that the tile count lands on whole rounds of the 256 CUs: the language model's M = 2304 tokens x N = 4096 is
// 16 x 16 = 256 tiles of 144 x 256 -- one per CU, one round (192 x 128: 384 tiles, 1.5).
// Three LDS stages of (BM + 256) x 64 bf16 filled by LDS-DMA (source-side XOR swizzle as above), two K steps in
// flight, one raw s_barrier per K step, counted vmcnt; the pieces of the next-but-one stage are issued between
// the MFMAs.  Tiles are numbered so that each XCD (blockIdx % 8) owns a compact 8 (M) x 4 (N) patch of them.
//
// Measured on 2304 x 4096 x 4096 (tools/bench_bf16_gemm.py, ablation builds of this file): 85 us = 900 TFLOP/s;
// alone, the fragment reads take 30 us (the LDS delivers ~156 B/clk to 8 waves reading 22 KB each per K step),
// the MFMAs 27 us (= the matrix pipe's rate), the staging 25 us, over a 20 us floor (launch, 64 barriers, 19 MB
// of C) -- and the three overlap little: all waves read, then all multiply.  A finer pipeline (ring of six
// 32-deep units, next unit's fragments read under this unit's MFMAs) was built and measured SLOWER (104 us):
// 64-byte rows double the DMA's cache-line requests (staging alone 61 -> 85 us) and twice the barriers eat what
// the read/MFMA overlap gives.
constexpr int WBN = 256;

template <int MTB>
__global__ __launch_bounds__(512, 1) void bf16_gemm_wide_kernel(const GemmArgs a, int tiles_m, int tiles_n) {
  constexpr int BM = 16 * MTB;
  constexpr int STAGE = (BM + WBN) * BK;                 // bf16 elements per stage
  constexpr int PIECES = (BM + WBN) / 8;                 // 1 KB wave-pieces per stage (8 rows x 128 B)
  constexpr int NP = (PIECES + 7) / 8;                   // per wave, at most
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;

  // tile of this workgroup: XCD x = id % 8 takes a contiguous run of the patch order (4-tile-wide panels, M-major)
  int tm, tn;
  {
    const int T = tiles_m * tiles_n, id = blockIdx.x;
    const int q = T / 8, r = T % 8, x = id % 8;
    const int t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + id / 8;
    const int per_panel = tiles_m * 4, p = t / per_panel, rem = t - p * per_panel;
    const int w = min(4, tiles_n - 4 * p);
    tm = rem / w;
    tn = 4 * p + rem - tm * w;
  }
  const int m0 = tm * BM, n0 = tn * WBN;
  const int bo = blockIdx.z / a.inner, bi = blockIdx.z - bo * a.inner;
  const unsigned short *P = a.P + bo * a.spo + bi * a.spi, *Q = a.Q + bo * a.sqo + bi * a.sqi;

  f32x4 acc[MTB][2];
#pragma unroll
  for (int x = 0; x < MTB; ++x) acc[x][0] = acc[x][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk_main = a.K / BK, nk = nk_main + (a.R + BK - 1) / BK;
  // this wave's pieces: piece = wave + 8 j; rows 8 piece .. + 7 of the stage image (first BM rows: P, then Q)
  const int np = (PIECES - wave + 7) / 8;                // wave-uniform
  unsigned off1[NP], off2[NP];                           // element offsets of this lane's 16 bytes, main / low-rank pass
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int piece = min(wave + 8 * j, PIECES - 1), row = 8 * piece + (lane >> 3), c = (lane & 7) ^ (row & 7);
    const bool isA = row < BM;
    const int r = isA ? min(m0 + row, a.M - 1) : min(n0 + row - BM, a.N - 1);
    off1[j] = (unsigned)r * (unsigned)(isA ? a.ldp : a.ldq) + c * 8;
    off2[j] = (unsigned)r * (unsigned)(isA ? a.ldp2 : a.ldq2) + c * 8;
  }
  auto issue_piece = [&](int kt, int j) {                // piece j of stage kt -> LDS buffer kt % 3
    const bool main = kt < nk_main;
    const int k0 = main ? kt * BK : (kt - nk_main) * BK;
    const bool isA = wave + 8 * j < BM / 8;              // (wave-uniform)
    const unsigned short *base = isA ? (main ? P : a.P2) : (main ? Q : a.Q2);
    const unsigned short *src = base + (main ? off1[j] : off2[j]) + k0;
    unsigned short *dst = lds + (kt % 3) * STAGE + (wave + 8 * j) * 512;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
  };
  auto issue = [&](int kt) {
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (j < np) issue_piece(kt, j);
  };
  // Two wave groups half a K step apart (waves 0-3 = group A, 4-7 = group B: one of each per SIMD).  Every wave
  // runs the same stream  read(kt) -> multiply(kt);  group A meets the step's barrier BEFORE its reads, group B
  // BETWEEN its reads and its multiplies (its barrier kt + 1: it reads stage kt while A multiplies it, and multiplies
  // it while A reads stage kt + 1).  So A's reads share the CU with B's MFMAs and the other way round -- with all
  // eight waves in step, read time and multiply time simply added up (85 us for 27 us of MFMA).  Both groups pass
  // the barrier nk times; a wave issues its pieces of stage kt + 2 (A) / kt + 3 (B) among its multiplies of stage
  // kt, i.e. after the barrier that certifies everyone is done with the buffer they go into.
  const int grp_b = wave >= 4 ? 1 : 0;           // (wave-uniform)
  auto wait_stage = [&](bool last) {              // this wave's pieces of the stage about to be certified have landed
    if (!last) {                                  // (the stage after it may still fly)
      if (np == NP) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP - 1) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  };
  issue(0);
  if (nk > 1) issue(1);
  if (grp_b) {                                    // barrier 0 (stage 0 landed); B runs one stage further ahead
    if (nk > 2) issue(2);
    if (nk > 2) {
      if (np == NP) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NP - 1)) : "memory");
    } else {
      wait_stage(nk == 1);
    }
    __builtin_amdgcn_s_barrier();
  }
  for (int kt = 0; kt < nk; ++kt) {
    if (!grp_b) {                                 // A: barrier kt
      wait_stage(kt + 1 >= nk);
      __builtin_amdgcn_s_barrier();
    }
    const unsigned short *As = lds + (kt % 3) * STAGE, *Bs = As + BM * BK;
    bf16x8 fa[2][MTB], fb[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int pos = ((4 * ks + g) ^ (i & 7)) * 8;
#pragma unroll
      for (int y = 0; y < 2; ++y) fb[ks][y] = *reinterpret_cast<const bf16x8 *>(Bs + (wave * 32 + y * 16 + i) * BK + pos);
#pragma unroll
      for (int x = 0; x < MTB; ++x) fa[ks][x] = *reinterpret_cast<const bf16x8 *>(As + (x * 16 + i) * BK + pos);
    }
    if (grp_b && kt + 1 < nk) {                   // B: barrier kt + 1 -- its reads of stage kt are in registers
      wait_stage(kt + 2 >= nk);
      __builtin_amdgcn_s_waitcnt(0xc07f);         // lgkmcnt(0), as a builtin: the compiler's scoreboard must see it
      __builtin_amdgcn_s_barrier();
    }
    const int st = kt + 2 + grp_b;                // the stage whose buffer the last barrier has freed
    const bool more = st < nk;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int x = 0; x < MTB; ++x) {
        acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[ks][0], fa[ks][x], acc[x][0], 0, 0, 0);
        acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[ks][1], fa[ks][x], acc[x][1], 0, 0, 0);
        const int slot = ks * MTB + x;            // 0 .. 2 MTB - 1: one piece every other slot
        if (more && (slot & 1) == 0 && slot / 2 < NP && slot / 2 < np) issue_piece(st, slot / 2);
      }
    }
  }
  // epilogue: D = Q P^T -- lane (i, g) holds columns n = 4 g + r of row m = i
#pragma unroll
  for (int x = 0; x < MTB; ++x) {
    const int row = m0 + x * 16 + i;
    if (row >= a.M) continue;
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int col = n0 + wave * 32 + y * 16 + 4 * g;
      if (col >= a.N) continue;
      float v0 = acc[x][y][0] * a.scale, v1 = acc[x][y][1] * a.scale, v2 = acc[x][y][2] * a.scale,
            v3 = acc[x][y][3] * a.scale;
      const size_t o = (size_t)(bo * a.sco + bi * a.sci) + (size_t)row * a.ldc + col;
      if (a.accumulate) {                  // (bf16 C, N % 4 == 0: checked by the caller)
        const uint2 old = *reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned short *>(a.C) + o);
        v0 += bf_lo(old.x); v1 += bf_hi(old.x); v2 += bf_lo(old.y); v3 += bf_hi(old.y);
      }
      if (col + 3 < a.N) {
        if (a.c_f32) *reinterpret_cast<float4 *>(reinterpret_cast<float *>(a.C) + o) = make_float4(v0, v1, v2, v3);
        else *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(a.C) + o) =
            make_uint2(f2bf(v0) | ((unsigned)f2bf(v1) << 16), f2bf(v2) | ((unsigned)f2bf(v3) << 16));
      } else {
        const float vv[4] = {v0, v1, v2, v3};
        for (int r = 0; r < 4 && col + r < a.N; ++r) {
          if (a.c_f32) reinterpret_cast<float *>(a.C)[o + r] = vv[r];
          else reinterpret_cast<unsigned short *>(a.C)[o + r] = f2bf(vv[r]);
        }
      }
    }
  }
}

// dA and dB of ONE LoRA pair in ONE launch, no partial sums at all (round 4 cut the rows into 64 chunks for
// parallelism, wrote the chunks' partials to a workspace and added them up in a second launch: four launches per pair,
// 896 a step for a 32-layer stack, 8.5 ms of an 83 ms step; a first one-launch version -- tickets + agent-scope fences, the
// last workgroup of a column block adding the partials -- measured 80-150 us per pair against 37-41: an L2 write-back per
// wave).  Here a workgroup OWNS 64 output columns over ALL rows: 64 + 172 = 236 workgroups for a 4096 / 11008 pair, one
// per CU; the sum over the tokens never leaves the accumulators, so the result is bit-reproducible by construction.  One
// CU's share of the bandwidth needs ~64 KB in flight: a register ring of kGD passes (64 rows x 128 bytes each), refilled
// as it drains; the pass's rows go row-major into LDS (double-buffered: one barrier per pass) and each wave gathers the
// fragments of its 16 columns with the LDS transpose read (an MFMA fragment here is 8 consecutive TOKENS of one column:
// ds_read_b64_tr_b16 hands a 16-lane group's [4 tokens][16 columns] block out column-wise).  (Measured and dropped: 32
// columns per workgroup where 64-column blocks number fewer than the CUs -- 4096 + 4096 columns are 128 -- with 128-row
// passes and the two token halves met in LDS: 15.2 us against 14.1.)
struct GradJob {
  int C;
  const unsigned short *P; int ldp;          // (M, R)
  const unsigned short *Q; int ldq;          // (M, C)
  float *out; int transpose_out;
  int blocks;                                // 64-column blocks of this job
};
struct GradPair { GradJob j[2]; };
using v4s = __attribute__((ext_vector_type(4))) short;
__device__ __forceinline__ v4s tr_read(const unsigned short *p) {          // ds_read_b64_tr_b16
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3))) *)p);
}
constexpr int kGD = 8;                       // passes in flight per workgroup
constexpr int kGC = 64 + 8;                  // LDS pitch of a staged Q row, bf16 units (144 B)

template <int R>
__global__ __launch_bounds__(256) void lora_grad_cols_kernel(int M, const GradPair pr, float scale, int accumulate) {
  constexpr int RT = R / 16;
  constexpr int GP = R + 4;                  // LDS pitch of a staged P row (40 / 72 B: 8-byte aligned for the transpose reads)
  constexpr int PCH = R / 8;                 // 16-byte chunks per P row
  const int z = (int)blockIdx.x >= pr.j[0].blocks ? 1 : 0;
  const GradJob &jb = pr.j[z];
  const int C = jb.C;
  const int cb = 64 * ((int)blockIdx.x - (z ? pr.j[0].blocks : 0));
  __shared__ __attribute__((aligned(16))) unsigned short qs[2][64 * kGC];
  __shared__ __attribute__((aligned(16))) unsigned short ps[2][64 * GP];
  const unsigned short *__restrict__ P = jb.P;
  const unsigned short *__restrict__ Q = jb.Q;
  const int ldp = jb.ldp, ldq = jb.ldq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  f32x4 acc[RT];
#pragma unroll
  for (int u = 0; u < RT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging roles: Q -- thread t covers 16 bytes (8 columns) of rows t / 8 and 32 + t / 8; P -- threads 0 .. 64 PCH - 1
  const int qrow = tid >> 3, qc = (tid & 7) * 8;
  const bool qlive = cb + qc < C;            // (C % 8 == 0: a 16-byte piece is inside or outside)
  const int prow = tid / PCH, pc = (tid % PCH) * 8;
  const int np = (M + 63) >> 6;
  uint4 qv[kGD][2], pv[kGD];
  auto fetch = [&](int d, int pass) {
    const int m0 = pass * 64;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = m0 + qrow + 32 * h;
      qv[d][h] = (qlive && m < M) ? *reinterpret_cast<const uint4 *>(Q + (size_t)m * ldq + cb + qc) : make_uint4(0, 0, 0, 0);
    }
    const int m = m0 + prow;
    pv[d] = (prow < 64 && m < M) ? *reinterpret_cast<const uint4 *>(P + (size_t)m * ldp + pc) : make_uint4(0, 0, 0, 0);
  };
#pragma unroll
  for (int d = 0; d < kGD; ++d) fetch(d, d);                // (passes beyond the last read nothing: zeros)
  for (int base = 0; base < np; base += kGD) {
#pragma unroll
    for (int d = 0; d < kGD; ++d) {
      const int pass = base + d;
      if (pass < np) {                                      // (uniform)
        unsigned short *q_ = qs[d & 1], *p_ = ps[d & 1];    // (kGD is even: pass parity == d parity)
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<uint4 *>(q_ + (qrow + 32 * h) * kGC + qc) = qv[d][h];
        if (prow < 64) {
          uint2 *dst = reinterpret_cast<uint2 *>(p_ + prow * GP + pc);
          dst[0] = make_uint2(pv[d].x, pv[d].y); dst[1] = make_uint2(pv[d].z, pv[d].w);
        }
        fetch(d, pass + kGD);                               // refill the ring slot just drained
        __syncthreads();                                    // (the other buffer's readers finished before the last barrier)
        // fragments by the LDS transpose read: a 16-lane group hands in the addresses of a [4 tokens][16 columns] block
        // (lane i': token i' >> 2, columns 4 (i' & 3) ..) and lane i receives column i of it -- four consecutive tokens
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          const int tr = 32 * sl + 8 * g + (i >> 2), tc = 4 * (i & 3);
          union { v4s h[2]; bf16x8 v; } wq;
#pragma unroll
          for (int h = 0; h < 2; ++h) wq.h[h] = tr_read(q_ + (tr + 4 * h) * kGC + wave * 16 + tc);
#pragma unroll
          for (int u = 0; u < RT; ++u) {
            union { v4s h[2]; bf16x8 v; } wp;
#pragma unroll
            for (int h = 0; h < 2; ++h) wp.h[h] = tr_read(p_ + (tr + 4 * h) * GP + 16 * u + tc);
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq.v, wp.v, acc[u], 0, 0, 0);
          }
        }
      }
    }
  }
  // D[c][r]: lane (i, g) holds columns c = cb + 16 wave + 4 g + q (q = 0..3) of r = 16 u + i
  const int c = cb + wave * 16 + 4 * g;
  if (c >= C) return;                                       // (C % 4 == 0)
  float *out = jb.out;
#pragma unroll
  for (int u = 0; u < RT; ++u) {
    const int r = 16 * u + i;
    if (jb.transpose_out) {
      float *o = out + (size_t)c * R + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q * R] = (accumulate ? o[q * R] : 0.f) + acc[u][q] * scale;
    } else {
      float4 *o = reinterpret_cast<float4 *>(out + (size_t)r * C + c);
      float4 t = accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
      t.x += acc[u][0] * scale; t.y += acc[u][1] * scale; t.z += acc[u][2] * scale; t.w += acc[u][3] * scale;
      *o = t;
    }
  }
}

// The bf16 images of EVERY LoRA pair of a stack in the four orientations its products read, in one launch (once per
// optimiser step; round 4 issued four conversion launches per pair: 896 a step):
//   a_pad (r, K) = bf16(A)         bt_pad (r, N) = bf16(B^T)
//   at2   (K, 64)[:, :r] = bf16(A^T)    b2 (N, 64)[:, :r] = bf16(B)     (columns r..63 are zero and are not touched)
// blockIdx.y = pair; a thread owns one column k of A (then one row n of B).
template <int R>
__device__ __forceinline__ void shadow_pair(const msr3d_lora_shadow_job_t &jb) {
  const int K = jb.K, N = jb.N;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < K + N; t += gridDim.x * 256) {
    if (t < K) {
      const int k = t;
      unsigned w[R / 2];
#pragma unroll
      for (int r = 0; r < R; r += 2) {
        const unsigned lo = f2bf(jb.A[(size_t)r * K + k]), hi = f2bf(jb.A[(size_t)(r + 1) * K + k]);
        jb.a_pad[(size_t)r * K + k] = (unsigned short)lo;
        jb.a_pad[(size_t)(r + 1) * K + k] = (unsigned short)hi;
        w[r / 2] = lo | (hi << 16);
      }
      uint4 *d = reinterpret_cast<uint4 *>(jb.at2 + (size_t)k * 64);
#pragma unroll
      for (int q = 0; q < R / 8; ++q) d[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    } else {
      const int n = t - K;
      const float4 *src = reinterpret_cast<const float4 *>(jb.B + (size_t)n * R);
      unsigned w[R / 2];
#pragma unroll
      for (int q = 0; q < R / 4; ++q) {
        const float4 v = src[q];
        const unsigned b0 = f2bf(v.x), b1 = f2bf(v.y), b2 = f2bf(v.z), b3 = f2bf(v.w);
        w[2 * q] = b0 | (b1 << 16);
        w[2 * q + 1] = b2 | (b3 << 16);
        jb.bt_pad[(size_t)(4 * q) * N + n] = (unsigned short)b0;
        jb.bt_pad[(size_t)(4 * q + 1) * N + n] = (unsigned short)b1;
        jb.bt_pad[(size_t)(4 * q + 2) * N + n] = (unsigned short)b2;
        jb.bt_pad[(size_t)(4 * q + 3) * N + n] = (unsigned short)b3;
      }
      uint4 *d = reinterpret_cast<uint4 *>(jb.b2 + (size_t)n * 64);
#pragma unroll
      for (int q = 0; q < R / 8; ++q) d[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
  }
}
__global__ __launch_bounds__(256) void lora_shadows_kernel(const msr3d_lora_shadow_job_t *__restrict__ jobs) {
  const msr3d_lora_shadow_job_t jb = jobs[blockIdx.y];
  if (jb.r == 16) shadow_pair<16>(jb);
  else shadow_pair<32>(jb);
}

// C (M, N <= 64) = scale * P Q^T for a Q of a few rows (the LoRA down-projections x A^T and dy B: N = 16 of
// 64 padded columns), and C[:, N:zero_to] = 0.  A tile of the big kernels would put this on 18 CUs; here a
// workgroup owns 16 rows of P, its four waves each a quarter of K, fragments loaded straight from global memory
// (P is read once; the 16 x K operand Q stays in L2), and the four partial tiles meet in LDS.
// waves per workgroup, each a share of K: sixteen (four per SIMD) while their partial tiles fit 32 KB of LDS (N <= 32), eight
// otherwise (round 3: four).  2304 tokens are only 144 workgroups: what a CU has in flight is what its own waves issue.
template <int NT> constexpr int kSkinnyWaves = NT <= 2 ? 16 : 8;
// (Measured and dropped: 8 rows per workgroup, half of the MFMA tile empty, so that 2304 tokens are 288 workgroups
// instead of 144 on 256 CUs -- 19 us against 13 per call.)
// QUANT: the same pass also leaves the e4m3 image of P with one scale per row (= msr3d_quant_rows_fp8, bit for bit) --
// the frozen-weight product that follows reads exactly this tensor, and its own quantisation launch read it a second
// time: the rows' absolute maxima are taken from the fragments as they go by (integer maxima of the bf16 bit patterns),
// met across the waves in LDS, and a second walk over the wave's K slice (L2 hits) converts and stores 8 bytes per lane.
template <int NT, bool QUANT = false>
__global__ __launch_bounds__(64 * kSkinnyWaves<NT>) void bf16_gemm_skinny_kernel(int M, int N, int K, const unsigned short *__restrict__ P,
                                                               int ldp, const unsigned short *__restrict__ Q, int ldq,
                                                               unsigned short *__restrict__ C, int ldc, int zero_to,
                                                               float scale, unsigned char *__restrict__ q8 = nullptr,
                                                               int ldq8 = 0, float *__restrict__ row_scale = nullptr) {
  constexpr int NW = kSkinnyWaves<NT>;
  __shared__ __attribute__((aligned(16))) float red[NW][NT][64][4];
  __shared__ unsigned rmax[NW][16];
  unsigned amax = 0;                                   // two 15-bit maxima of |bf16| bit patterns, packed
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * 16;
  const int nks = K / 32, ks0 = wave * nks / NW, ks1 = (wave + 1) * nks / NW;
  const unsigned short *p = P + (size_t)min(m0 + i, M - 1) * ldp + 8 * g;
  const unsigned short *q[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) q[t] = Q + (size_t)min(16 * t + i, N - 1) * ldq + 8 * g;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // batches of U K steps, the NEXT batch's loads issued before this batch's MFMAs (round 3 loaded a batch, waited a full
  // memory latency, multiplied, and started over: 8 latencies per 16 rows x 4096 -- 15 us for 19 MB on 144 workgroups)
  constexpr int U = 4;
  struct Batch { bf16x8 fp[U], fq[U][NT]; };
  auto fetch = [&](Batch &b_, int ks) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      b_.fp[u] = *reinterpret_cast<const bf16x8 *>(p + (ks + u) * 32);
#pragma unroll
      for (int t = 0; t < NT; ++t) b_.fq[u][t] = *reinterpret_cast<const bf16x8 *>(q[t] + (ks + u) * 32);
    }
  };
  auto track = [&](const bf16x8 &f) {                  // |x| as integers: for non-negative floats the orders agree
    if constexpr (QUANT) {
      union { bf16x8 v; unsigned w[4]; } x;
      x.v = f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned a = x.w[e] & 0x7fff7fffu;
        amax = (max(amax >> 16, a >> 16) << 16) | max(amax & 0xffffu, a & 0xffffu);
      }
    }
  };
  auto mma = [&](const Batch &b_) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      track(b_.fp[u]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b_.fq[u][t], b_.fp[u], acc[t], 0, 0, 0);
    }
  };
  const int nb = (ks1 - ks0) / U;
  int ks = ks0;
  if (nb > 0) {
    Batch ba, bb;
    fetch(ba, ks0);
    for (int b2 = 0; b2 < nb; b2 += 2) {
      if (b2 + 1 < nb) fetch(bb, ks0 + (b2 + 1) * U);
      mma(ba);
      if (b2 + 2 < nb) fetch(ba, ks0 + (b2 + 2) * U);
      if (b2 + 1 < nb) mma(bb);
    }
    ks = ks0 + nb * U;
  }
  for (; ks < ks1; ++ks) {
    const bf16x8 fp = *reinterpret_cast<const bf16x8 *>(p + ks * 32);
    track(fp);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8 *>(q[t] + ks * 32), fp, acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4 *>(&red[wave][t][lane][0]) = acc[t];
  constexpr int QU = 8;                                // 16-byte pieces per thread and round of the second walk
  constexpr int TPR = 4 * NW, QS = 8 * TPR;            // threads per row of the second walk; elements per row and step
  const int qr = threadIdx.x / TPR, qc = (threadIdx.x % TPR) * 8;
  const unsigned short *src = P + (size_t)min(m0 + qr, M - 1) * ldp + qc;
  uint4 xv[QUANT ? QU : 1];
  if constexpr (QUANT) {
    unsigned m = max(amax >> 16, amax & 0xffffu);
    m = max(m, (unsigned)__shfl_xor((int)m, 16));
    m = max(m, (unsigned)__shfl_xor((int)m, 32));
    if (g == 0) rmax[wave][i] = m;
    // the second walk's first round of loads leaves BEFORE the barrier (it needs the scale only to convert)
#pragma unroll
    for (int u = 0; u < QU; ++u) xv[u] = QS * u + qc < K ? *reinterpret_cast<const uint4 *>(src + QS * u) : make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
  if constexpr (QUANT) {
    unsigned m = rmax[0][i];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = max(m, rmax[w][i]);
    const float mx = __uint_as_float(m << 16);
    const float sc = mx > 0.f ? mx * (1.0f / 448.0f) : 1.0f;
    if (m0 + i < M && wave == 0 && g == 0) row_scale[m0 + i] = sc;
    // second walk, ROW-major over the workgroup's 16 x K block (L2 hits): 32 threads per row, 16 bytes each -- 512
    // contiguous bytes read and 256 written per row and step (the fragment order of pass 1 would store 32-byte pieces)
    unsigned mr = rmax[0][qr];
#pragma unroll
    for (int w = 1; w < NW; ++w) mr = max(mr, rmax[w][qr]);
    const float mxr = __uint_as_float(mr << 16);
    const float inv = 1.0f / (mxr > 0.f ? mxr * (1.0f / 448.0f) : 1.0f);
    const bool live = m0 + qr < M;
    unsigned char *dst = q8 + (size_t)(m0 + qr) * ldq8 + qc;
    for (int c0 = 0; c0 < K; c0 += QS * QU) {
      if (c0 > 0) {
#pragma unroll
        for (int u = 0; u < QU; ++u)
          xv[u] = c0 + QS * u + qc < K ? *reinterpret_cast<const uint4 *>(src + c0 + QS * u) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < QU; ++u) {
        const int c = c0 + QS * u + qc;
        const unsigned w4[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(w4[0] << 16) * inv, __uint_as_float(w4[0] & 0xffff0000u) * inv, lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(w4[1] << 16) * inv, __uint_as_float(w4[1] & 0xffff0000u) * inv, lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(w4[2] << 16) * inv, __uint_as_float(w4[2] & 0xffff0000u) * inv, hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(w4[3] << 16) * inv, __uint_as_float(w4[3] & 0xffff0000u) * inv, hi, true);
        if (live && c < K) *reinterpret_cast<uint2 *>(dst + c0 + QS * u) = make_uint2((unsigned)lo, (unsigned)hi);
      }
    }
  }
  // D = Q P^T: lane (i, g) of tile t holds columns n = 16 t + 4 g + r of row m = i; wave w finishes tiles w, w + 4 ..
  const int row = m0 + i;
  for (int t = wave; t < NT; t += NW) {
    f32x4 v = *reinterpret_cast<const f32x4 *>(&red[0][t][lane][0]);
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const f32x4 o = *reinterpret_cast<const f32x4 *>(&red[w][t][lane][0]);
      v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
    }
    const int col = 16 * t + 4 * g;
    if (row < M && col < N)              // (N is a multiple of 4)
      *reinterpret_cast<uint2 *>(C + (size_t)row * ldc + col) =
          make_uint2(f2bf(v[0] * scale) | ((unsigned)f2bf(v[1] * scale) << 16),
                     f2bf(v[2] * scale) | ((unsigned)f2bf(v[3] * scale) << 16));
  }
  // the padding columns the next product reads as part of its K step
  for (int e = threadIdx.x; e < 16 * ((zero_to - N) / 4); e += 64 * NW) {
    const int r = e / ((zero_to - N) / 4), c = N + 4 * (e - r * ((zero_to - N) / 4));
    if (m0 + r < M) *reinterpret_cast<uint2 *>(C + (size_t)(m0 + r) * ldc + c) = make_uint2(0u, 0u);
  }
}

inline bool al16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

template <int BM>
int launch_gemm(const GemmArgs &a, int batch, hipStream_t st) {
  constexpr size_t lds = sizeof(unsigned short) * (BM + BN) * LD;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&bf16_gemm_kernel<BM>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) return (int)attr;
  dim3 grid((a.N + BN - 1) / BN, (a.M + BM - 1) / BM, batch);
  bf16_gemm_kernel<BM><<<grid, 256, lds, st>>>(a);
  return (int)hipGetLastError();
}

template <int BM>
int launch_gemm_glds(const GemmArgs &a, int batch, hipStream_t st) {
  constexpr size_t lds = sizeof(unsigned short) * 3 * (BM + BN) * BK;         // 192: 122,880 B
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&bf16_gemm_glds_kernel<BM>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) return (int)attr;
  dim3 grid((a.N + BN - 1) / BN, (a.M + BM - 1) / BM, batch);
  bf16_gemm_glds_kernel<BM><<<grid, 256, lds, st>>>(a);
  return (int)hipGetLastError();
}

template <int MTB>
int launch_gemm_wide(const GemmArgs &a, int batch, hipStream_t st) {
  constexpr int BM = 16 * MTB;
  constexpr size_t lds = sizeof(unsigned short) * 3 * (BM + WBN) * BK;        // 144: 153,600 B
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&bf16_gemm_wide_kernel<MTB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (attr != hipSuccess) return (int)attr;
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + WBN - 1) / WBN;
  bf16_gemm_wide_kernel<MTB><<<dim3(tiles_m * tiles_n, 1, batch), 512, lds, st>>>(a, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

std::atomic<int> g_gemm_path{-1};                // -1: read MSR3D_BF16_GEMM (wide | glds | reg) on first use

// wide tiles: tile height = the one with the least (rounds of 256 CUs) x height
int wide_tile_height(int M, int N, int batch) {
  const int tn = (N + WBN - 1) / WBN;
  long long best = -1;
  int bm = 0;
  for (int h : {160, 144, 128}) {
    const long long tiles = (long long)((M + h - 1) / h) * tn * batch, cost = (tiles + 255) / 256 * h;
    if (best < 0 || cost < best) best = cost, bm = h;
  }
  return bm;
}

// the kernel a product takes, from its shape alone: 0 = bf16_gemm_kernel<128>, 1 = bf16_gemm_kernel<192>,
// 2 = bf16_gemm_glds_kernel<192>, 8 / 9 / 10 = bf16_gemm_wide_kernel<MTB> (msr3d_bf16_gemm_path reports it)
int gemm_path(int M, int N, int R, int batch, int ldp, int ldq, int ldp2, int ldq2) {
  int path = g_gemm_path.load(std::memory_order_relaxed);
  if (path < 0) {
    const char *e = getenv("MSR3D_BF16_GEMM");
    path = (e && e[0] == 'r') ? 0 : (e && e[0] == 'g') ? 1 : 2;
    g_gemm_path.store(path, std::memory_order_relaxed);
  }
  // wide tiles: big products whose offsets fit the kernel's 32-bit element offsets
  if (path == 2 && M >= 128 && N >= 256 && (R % BK) == 0 &&
      (long long)M * ldp < (1ll << 31) && (long long)N * ldq < (1ll << 31) &&
      (R == 0 || ((long long)M * ldp2 < (1ll << 31) && (long long)N * ldq2 < (1ll << 31)))) {
    const int bm = wide_tile_height(M, N, batch);
    // (fewer tiles than half the chip: the 128-wide tiles of the 4-wave kernels spread the product further)
    if ((long long)((M + bm - 1) / bm) * ((N + WBN - 1) / WBN) * batch >= 128) return bm / 16;
  }
  // LDS-DMA path: rows >= 16 bytes-aligned sources (checked by the callers) and R a multiple of 64 (a stage
  // reads 64 columns of the low-rank pair)
  if (path >= 1 && M >= 192 && (R % BK) == 0) return 2;
  // tile height: the one that wastes fewer padded rows; 192 on a tie at >= 192 rows (fewer LDS reads per MFMA)
  const long long w128 = (long long)((M + 127) / 128) * 128, w192 = (long long)((M + 191) / 192) * 192;
  return (M >= 192 && w192 <= w128) ? 1 : 0;
}

int launch_wide(int mtb, const GemmArgs &a, int batch, hipStream_t st) {
  return mtb == 10 ? launch_gemm_wide<10>(a, batch, st) : mtb == 9 ? launch_gemm_wide<9>(a, batch, st)
                                                                   : launch_gemm_wide<8>(a, batch, st);
}

int gemm_dispatch(GemmArgs &a, int batch, hipStream_t st) {
  const int path = gemm_path(a.M, a.N, a.R, batch, a.ldp, a.ldq, a.ldp2, a.ldq2);
  if (path >= 8) return launch_wide(path, a, batch, st);
  return path == 2 ? launch_gemm_glds<192>(a, batch, st) : path == 1 ? launch_gemm<192>(a, batch, st)
                                                                     : launch_gemm<128>(a, batch, st);
}

}  // namespace

extern "C" {

int msr3d_bf16_gemm_lowrank(int M, int N, int K, int R, const void *P, int ldp, const void *Q, int ldq,
                            const void *P2, int ldp2, const void *Q2, int ldq2, void *C, int ldc,
                            int c_f32, float scale, msr3d_stream_t stream) {
  if (M < 0 || N < 0 || K < 0 || R < 0 || (K % BK) != 0 || (R % 8) != 0) return MSR3D_EINVAL;
  if (M == 0 || N == 0) return 0;
  if (!P || !Q || !C || ldp < K || ldq < K || ldc < N || (ldp % 8) || (ldq % 8) || !al16(P) || !al16(Q))
    return MSR3D_EINVAL;
  if ((ldc % 4) || (reinterpret_cast<uintptr_t>(C) & 15u)) return MSR3D_EINVAL;
  if (R > 0 && (!P2 || !Q2 || ldp2 < R || ldq2 < R || (ldp2 % 8) || (ldq2 % 8) || !al16(P2) || !al16(Q2)))
    return MSR3D_EINVAL;
  GemmArgs a;
  a.M = M; a.N = N; a.K = K; a.R = R;
  a.P = (const unsigned short *)P; a.ldp = ldp; a.Q = (const unsigned short *)Q; a.ldq = ldq;
  a.P2 = (const unsigned short *)P2; a.ldp2 = ldp2; a.Q2 = (const unsigned short *)Q2; a.ldq2 = ldq2;
  a.C = C; a.ldc = ldc; a.c_f32 = c_f32; a.scale = scale;
  a.accumulate = 0;
  a.inner = 1;
  a.spo = a.spi = a.sqo = a.sqi = a.sco = a.sci = 0;
  return gemm_dispatch(a, 1, (hipStream_t)stream);
}

int msr3d_bf16_gemm_lowrank_acc(int M, int N, int K, int R, const void *P, int ldp, const void *Q, int ldq,
                                const void *P2, int ldp2, const void *Q2, int ldq2, void *C, int ldc, float scale,
                                msr3d_stream_t stream) {
  if (M < 0 || N < 0 || K < 0 || R < 0 || (K % BK) != 0 || (R % BK) != 0 || (N % 4) != 0) return MSR3D_EINVAL;
  if (M == 0 || N == 0) return 0;
  if (!P || !Q || !C || ldp < K || ldq < K || ldc < N || (ldp % 8) || (ldq % 8) || !al16(P) || !al16(Q))
    return MSR3D_EINVAL;
  if ((ldc % 4) || (reinterpret_cast<uintptr_t>(C) & 15u)) return MSR3D_EINVAL;
  if (R > 0 && (!P2 || !Q2 || ldp2 < R || ldq2 < R || (ldp2 % 8) || (ldq2 % 8) || !al16(P2) || !al16(Q2)))
    return MSR3D_EINVAL;
  // the wide-tile kernel only (the language model's products): its domain, as gemm_dispatch states it
  if (M < 128 || N < 256 || (long long)M * ldp >= (1ll << 31) || (long long)N * ldq >= (1ll << 31) ||
      (R > 0 && ((long long)M * ldp2 >= (1ll << 31) || (long long)N * ldq2 >= (1ll << 31))))
    return MSR3D_EINVAL;
  GemmArgs a;
  a.M = M; a.N = N; a.K = K; a.R = R;
  a.P = (const unsigned short *)P; a.ldp = ldp; a.Q = (const unsigned short *)Q; a.ldq = ldq;
  a.P2 = (const unsigned short *)P2; a.ldp2 = ldp2; a.Q2 = (const unsigned short *)Q2; a.ldq2 = ldq2;
  a.C = C; a.ldc = ldc; a.c_f32 = 0; a.scale = scale;
  a.accumulate = 1;
  a.inner = 1;
  a.spo = a.spi = a.sqo = a.sqi = a.sco = a.sci = 0;
  return launch_wide(msr3d_bf16_gemm_acc_tile(M, N) / 16, a, 1, (hipStream_t)stream);
}

int msr3d_bf16_gemm_path(int M, int N, int R, int batch, int ldp, int ldq, int ldp2, int ldq2) {
  if (M <= 0 || N <= 0 || R < 0 || batch <= 0) return MSR3D_EINVAL;
  return gemm_path(M, N, R, batch, ldp, ldq, ldp2, ldq2);
}

int msr3d_bf16_gemm_acc_tile(int M, int N) {
  if (M <= 0 || N <= 0) return MSR3D_EINVAL;
  return wide_tile_height(M, N, 1);
}

int msr3d_bf16_gemm_batched(int outer, int inner, int M, int N, int K, const void *P, int ldp, long long p_outer,
                            long long p_inner, const void *Q, int ldq, long long q_outer, long long q_inner, void *C,
                            int ldc, long long c_outer, long long c_inner, int c_f32, float scale,
                            msr3d_stream_t stream) {
  if (outer < 0 || inner <= 0 || M < 0 || N < 0 || K < 0 || (K % BK) != 0) return MSR3D_EINVAL;
  if (outer == 0 || M == 0 || N == 0) return 0;
  if ((long long)outer * inner > 65535 || !P || !Q || !C || ldp < K || ldq < K || ldc < N || (ldp % 8) || (ldq % 8) ||
      !al16(P) || !al16(Q))
    return MSR3D_EINVAL;
  if ((p_outer % 8) || (p_inner % 8) || (q_outer % 8) || (q_inner % 8) || (c_outer % 4) || (c_inner % 4) || (ldc % 4) ||
      (reinterpret_cast<uintptr_t>(C) & 15u))
    return MSR3D_EINVAL;
  GemmArgs a;
  a.M = M; a.N = N; a.K = K; a.R = 0;
  a.P = (const unsigned short *)P; a.ldp = ldp; a.Q = (const unsigned short *)Q; a.ldq = ldq;
  a.P2 = nullptr; a.ldp2 = 0; a.Q2 = nullptr; a.ldq2 = 0;
  a.C = C; a.ldc = ldc; a.c_f32 = c_f32; a.scale = scale;
  a.accumulate = 0;
  a.inner = inner;
  a.spo = p_outer; a.spi = p_inner; a.sqo = q_outer; a.sqi = q_inner; a.sco = c_outer; a.sci = c_inner;
  return gemm_dispatch(a, outer * inner, (hipStream_t)stream);
}

int msr3d_lora_grad_pair(int M, int R, int njobs, const msr3d_lora_grad_job_t *jobs, float scale, int accumulate,
                         msr3d_stream_t stream) {
  if (M < 0 || (R != 16 && R != 32) || njobs < 1 || njobs > 2 || !jobs) return MSR3D_EINVAL;
  if (M == 0) return 0;
  GradPair pr{};
  int total = 0;
  for (int z = 0; z < njobs; ++z) {
    const msr3d_lora_grad_job_t &j = jobs[z];
    if (j.C <= 0 || (j.C % 8) || !j.P || !j.Q || !j.out || j.ldp < R || j.ldq < j.C || (j.ldp % 8) || (j.ldq % 8) ||
        !al16(j.P) || !al16(j.Q) || (reinterpret_cast<uintptr_t>(j.out) & 15u))
      return MSR3D_EINVAL;
    GradJob &g = pr.j[z];
    g.C = j.C; g.P = (const unsigned short *)j.P; g.ldp = j.ldp; g.Q = (const unsigned short *)j.Q; g.ldq = j.ldq;
    g.out = j.out; g.transpose_out = j.transpose_out;
    g.blocks = (j.C + 63) / 64;
    total += g.blocks;
  }
  hipStream_t st = (hipStream_t)stream;
  if (R == 16) lora_grad_cols_kernel<16><<<total, 256, 0, st>>>(M, pr, scale, accumulate);
  else lora_grad_cols_kernel<32><<<total, 256, 0, st>>>(M, pr, scale, accumulate);
  return (int)hipGetLastError();
}

int msr3d_lora_shadows(int njobs, const msr3d_lora_shadow_job_t *jobs_device, msr3d_stream_t stream) {
  if (njobs < 0) return MSR3D_EINVAL;
  if (njobs == 0) return 0;
  if (!jobs_device) return MSR3D_EINVAL;
  lora_shadows_kernel<<<dim3(16, njobs), 256, 0, (hipStream_t)stream>>>(jobs_device);
  return (int)hipGetLastError();
}

static int skinny_launch(int M, int N, int K, const void *P, int ldp, const void *Q, int ldq, void *C, int ldc, int zero_to,
                         float scale, void *q8, int ldq8, float *row_scale, msr3d_stream_t stream) {
  if (M < 0 || N <= 0 || N > 64 || (N % 16) || K <= 0 || (K % 32) || zero_to < N || (zero_to % 4) || zero_to > ldc)
    return MSR3D_EINVAL;
  if (M == 0) return 0;
  if (!P || !Q || !C || ldp < K || ldq < K || ldc < N || (ldp % 8) || (ldq % 8) || (ldc % 4) || !al16(P) || !al16(Q) ||
      (reinterpret_cast<uintptr_t>(C) & 7u))
    return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const unsigned short *p = (const unsigned short *)P, *q = (const unsigned short *)Q;
  unsigned short *c = (unsigned short *)C;
  const int grid = (M + 15) / 16;
  if (q8) {
    unsigned char *q8p = (unsigned char *)q8;
    switch (N / 16) {
      case 1: bf16_gemm_skinny_kernel<1, true><<<grid, 64 * kSkinnyWaves<1>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale, q8p, ldq8, row_scale); break;
      case 2: bf16_gemm_skinny_kernel<2, true><<<grid, 64 * kSkinnyWaves<2>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale, q8p, ldq8, row_scale); break;
      case 3: bf16_gemm_skinny_kernel<3, true><<<grid, 64 * kSkinnyWaves<3>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale, q8p, ldq8, row_scale); break;
      default: bf16_gemm_skinny_kernel<4, true><<<grid, 64 * kSkinnyWaves<4>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale, q8p, ldq8, row_scale); break;
    }
    return (int)hipGetLastError();
  }
  switch (N / 16) {
    case 1: bf16_gemm_skinny_kernel<1><<<grid, 64 * kSkinnyWaves<1>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale); break;
    case 2: bf16_gemm_skinny_kernel<2><<<grid, 64 * kSkinnyWaves<2>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale); break;
    case 3: bf16_gemm_skinny_kernel<3><<<grid, 64 * kSkinnyWaves<3>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale); break;
    default: bf16_gemm_skinny_kernel<4><<<grid, 64 * kSkinnyWaves<4>, 0, st>>>(M, N, K, p, ldp, q, ldq, c, ldc, zero_to, scale); break;
  }
  return (int)hipGetLastError();
}

int msr3d_bf16_gemm_skinny(int M, int N, int K, const void *P, int ldp, const void *Q, int ldq, void *C, int ldc,
                           int zero_to, float scale, msr3d_stream_t stream) {
  return skinny_launch(M, N, K, P, ldp, Q, ldq, C, ldc, zero_to, scale, nullptr, 0, nullptr, stream);
}

int msr3d_bf16_gemm_skinny_quant(int M, int N, int K, const void *P, int ldp, const void *Q, int ldq, void *C, int ldc,
                                 int zero_to, float scale, void *q8, int ldq8, float *row_scale, msr3d_stream_t stream) {
  if (!q8 || !row_scale || ldq8 < K || (ldq8 % 8) || (reinterpret_cast<uintptr_t>(q8) & 7u)) return MSR3D_EINVAL;
  return skinny_launch(M, N, K, P, ldp, Q, ldq, C, ldc, zero_to, scale, q8, ldq8, row_scale, stream);
}

}  // extern "C"
