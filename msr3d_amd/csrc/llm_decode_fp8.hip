// llm_decode_fp8.hip -- the skinny weight-stream product of a decoding step (llm_decode.hip: skinny_kernel) on OCP e4m3
// weights: what `CachedDecoder(weights="e4m3")` launches for every LoRA projection of a base="fp8" stack.
//
//     msr3d_fp8_skinny_lowrank    C_j (M <= 64, N_j) = diag(sp) (Pq Wq_j^T) diag(sw_j) + P2 B2_j^T,  j < njobs <= 3
//
// Pq (M, K) e4m3 codes with row scales sp (what msr3d_bf16_gemm_skinny_quant writes), Wq_j (N_j, K) e4m3 codes with
// per-output-channel scales sw_j (LoRALinear.weight_q / weight_scale), the low-rank pair bf16.  A weight byte is read
// once per call: half the stream of the bf16 kernel.
//
// v_mfma_scale_f32_16x16x128_f8f6f4 (both formats e4m3, block scales 2^0) with the ACTIVATIONS as the 16-row side: lane l
// supplies 32 contiguous bytes at k0 + 32 (l >> 4) of row l & 15 of both operands -- for W two 16-byte non-temporal
// loads of a k-contiguous weight row straight into the operand registers (no LDS: nothing of W is shared between
// waves).  A workgroup of four waves owns 16 TN rows of W; the waves split K in 128-wide steps (one instruction per
// tile and step), keep the loads of the NEXT TWO steps in flight while the matrix pipe works on this one -- a step is
// 32 bytes a lane and tile, half the bf16 kernel's chunk, so two steps ahead are the bytes that kernel has in flight --
// and add their partial sums through LDS in wave order.  e4m3 x e4m3 products are exact in fp32.
// The low-rank pair goes on the bf16 instruction into a SECOND accumulator set (wave 3, a fifth LDS slot): the output is
// bf16(fma(sum of the e4m3 partial sums, sp[m] sw[n], low-rank sum)).  No division trick: at these tile sizes the
// registers are there (MT = 4, TN = 2: 8 accumulator tiles twice).
// Row m of an accumulator tile comes from row m of the activation operand alone, and sp[m] is read for row m alone, so
// a row of C never sees another row of Pq, sp or P2 (NaN included), whatever MT; the tile count TN and the job a tile
// belongs to change which workgroup computes an output, not how.  Nothing atomic: every output has one owner.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/msr3d_hip.h"

namespace {

using u8 = unsigned char;
using u16 = unsigned short;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int kOne = 0x7f7f7f7f;         // four E8M0 block scales of 2^0

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}
inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// a lane's 32 bytes of one row and K step: the MX operand as it is
struct Frag {
  u32x4 lo, hi;
};
// a weight: read once per call and never again -- non-temporal, so the stream does not push the activations and the
// K / V cache out of L2
__device__ __forceinline__ Frag load_stream(const u8 *p) {
  return Frag{__builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)),
              __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p + 16))};
}
__device__ __forceinline__ Frag load_keep(const u8 *p) {
  return Frag{*reinterpret_cast<const u32x4 *>(p), *reinterpret_cast<const u32x4 *>(p + 16)};
}
__device__ __forceinline__ u32x4 load_keep16(const u16 *p) { return *reinterpret_cast<const u32x4 *>(p); }
__device__ __forceinline__ i32x8 operand(const Frag &f) {
  return i32x8{(int)f.lo[0], (int)f.lo[1], (int)f.lo[2], (int)f.lo[3], (int)f.hi[0], (int)f.hi[1], (int)f.hi[2], (int)f.hi[3]};
}
__device__ __forceinline__ f32x4 mfma_e4m3(const Frag &a, const Frag &b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(operand(a), operand(b), c, 0, 0, 0, kOne, 0, kOne);
}
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// the wide rule of llm_decode.hip: two tiles of W a workgroup only where that still gives every CU a workgroup
constexpr long long kSkinnyWideMinWg = 256;
struct Fp8SkinnyJobs {
  const u8 *W[3];
  const float *sw[3];
  const u16 *B2[3];
  u16 *C[3];
  int N[3];
  int ldw[3], ldb2[3], ldc[3];
  int tiles[3];      // exclusive prefix sums of the jobs' tile counts are formed in the kernel (njobs <= 3)
  int njobs;
};

// Steps in flight ahead of the one being multiplied.  A step is 32 bytes a lane and tile, so two are the 64 bytes the
// bf16 kernel keeps in flight.  Measured at Vicuna-7B projection shapes, 1 / 5 / 20 / 64 rows, the entry alone on cold
// weights: 4, 6 and 8 steps ahead (3 and 4 for the three- and four-tile forms) moved no launch by more than its
// run-to-run spread in either direction (q | k | v 15.1 / 15.1 / 15.3 / 14.8 us at one row, down 33.3 / 32.9 / 34.6 /
// 33.0 at 64), at up to 256 registers instead of 175 -- the launch is not waiting on this queue.
constexpr int kDepth = 2;

template <int MT, int TN, bool SWIGLU>
__global__ __launch_bounds__(256) void fp8_skinny_kernel(int M, int K, int R, const u8 *__restrict__ P, int ldp,
                                                         const float *__restrict__ sp, const u16 *__restrict__ P2, int ldp2,
                                                         Fp8SkinnyJobs jobs) {
  // slots 0 .. 3: the waves' e4m3 partial sums; slot 4: the low-rank sum (written only when R > 0)
  __shared__ float red[5][MT * TN][64][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  int tile = blockIdx.x, job = 0;
  if (!SWIGLU) {
    while (job + 1 < jobs.njobs && tile >= jobs.tiles[job]) { tile -= jobs.tiles[job]; ++job; }
  }
  // SWIGLU: job 0 = gate, job 1 = up, the workgroup takes the SAME 16 rows of both (TN == 2 is the job index)
  const u8 *wrow[TN];
  const u16 *brow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int j = SWIGLU ? t : job;
    const int n = SWIGLU ? tile * 16 + r16 : (tile * TN + t) * 16 + r16;       // < N_j: tiles[j] = N_j / (16 TN)
    wrow[t] = jobs.W[j] + (size_t)n * jobs.ldw[j] + 32 * g;
    brow[t] = jobs.B2[j] ? jobs.B2[j] + (size_t)n * jobs.ldb2[j] + 8 * g : nullptr;
  }
  const u8 *prow[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = min(m * 16 + r16, M - 1);       // rows >= M: a valid row is read and its result not stored
    prow[m] = P + (size_t)row * ldp + 32 * g;
  }
  f32x4 acc[MT][TN];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // steps [c0, c1) of this wave; K = 128, 384: some waves get none (c0 == c1) and contribute zeros
  const int steps = K >> 7;
  const int c0 = (steps * wave) >> 2, c1 = (steps * (wave + 1)) >> 2;
  // a ring of DEPTH + 1 register stages: stage s holds step c + s while the loads of the DEPTH steps after the one being
  // multiplied are in flight; the loop is unrolled by the ring so that every stage index is a constant.  The steps are
  // accumulated in the order c0 .. c1 - 1 whatever DEPTH is.
  constexpr int DEPTH = kDepth, RING = DEPTH + 1;
  Frag w[RING][TN], a[RING][MT];
  auto fetch = [&](int c, Frag (&ws)[TN], Frag (&as)[MT]) {     // (c < c1 <= K / 128: every byte inside the row)
#pragma unroll
    for (int t = 0; t < TN; ++t) ws[t] = load_stream(wrow[t] + (size_t)c * 128);
#pragma unroll
    for (int m = 0; m < MT; ++m) as[m] = load_keep(prow[m] + (size_t)c * 128);
  };
#pragma unroll
  for (int s = 0; s < DEPTH; ++s)
    if (c0 + s < c1) fetch(c0 + s, w[s], a[s]);
  for (int c = c0; c < c1; c += RING) {
#pragma unroll
    for (int s = 0; s < RING; ++s) {
      if (c + s < c1) {                              // (wave-uniform)
        // step c + s + DEPTH goes into the stage multiplied last (s - 1), before this step's MFMAs
        if (c + s + DEPTH < c1) fetch(c + s + DEPTH, w[(s + DEPTH) % RING], a[(s + DEPTH) % RING]);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int t = 0; t < TN; ++t) acc[m][t] = mfma_e4m3(a[s][m], w[s][t], acc[m][t]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave][m * TN + t][lane][i] = acc[m][t][i];
  if (wave == 3 && R > 0) {
    // the low-rank pair, R / 32 bf16 k steps into accumulators of its own: P2 (M, R) = s P A^T, B2 (N, R) = B, zero-padded
    f32x4 low[MT][TN];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < TN; ++t) low[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < R; k += 32) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int row = min(m * 16 + r16, M - 1);
        const u32x4 pa = load_keep16(P2 + (size_t)row * ldp2 + 8 * g + k);
#pragma unroll
        for (int t = 0; t < TN; ++t)
          if (brow[t]) low[m][t] = mfma_bf16(pa, load_keep16(brow[t] + k), low[m][t]);
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[4][m * TN + t][lane][i] = low[m][t][i];
  }
  __syncthreads();
  // accumulator element i of lane l is C[row 4 (l >> 4) + i][column l & 15]; the four waves' partial sums in wave order,
  // then ONE fma: the scales and the low-rank sum (explicit, so that every instantiation rounds alike)
  auto value = [&](int mt, int l, int i, float scale) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) s += red[wv][mt][l][i];
    return fmaf(s, scale, R > 0 ? red[4][mt][l][i] : 0.f);
  };
  if (SWIGLU) {
    for (int e = threadIdx.x; e < MT * 256; e += 256) {
      const int m = e >> 8, l = (e >> 2) & 63, i = e & 3;
      const int row = m * 16 + 4 * (l >> 4) + i, col = tile * 16 + (l & 15);
      if (row >= M) continue;
      const float sr = sp[row];
      const float gsum = value(m * TN + 0, l, i, sr * jobs.sw[0][col]);
      const float usum = value(m * TN + (TN - 1), l, i, sr * jobs.sw[TN - 1][col]);
      // the same roundings as the training graph: gate and up are bf16 tensors, silu a bf16 op of its own
      const float gb = bf2f(f2bf(gsum)), ub = bf2f(f2bf(usum));
      const float sg = bf2f(f2bf(gb / (1.0f + expf(-gb))));
      jobs.C[0][(size_t)row * jobs.ldc[0] + col] = f2bf(sg * ub);
    }
  } else {
    for (int e = threadIdx.x; e < MT * TN * 256; e += 256) {
      const int mt = e >> 8, l = (e >> 2) & 63, i = e & 3;
      const int m = mt / TN, t = mt % TN;
      const int row = m * 16 + 4 * (l >> 4) + i, col = (tile * TN + t) * 16 + (l & 15);
      if (row >= M) continue;
      jobs.C[job][(size_t)row * jobs.ldc[job] + col] = f2bf(value(mt, l, i, sp[row] * jobs.sw[job][col]));
    }
  }
}

}  // namespace

extern "C" {

int msr3d_fp8_skinny_lowrank(int M, int K, int R, const void *Pq, int ldp, const float *sp, const void *P2, int ldp2,
                             int njobs, const msr3d_fp8_skinny_job_t *jobs, int swiglu, msr3d_stream_t stream) {
  if (M < 0 || M > MSR3D_SKINNY_WIDE_MAX_M || K <= 0 || (K % 128) || R < 0 || (R % 32) || njobs < 0 || njobs > 3)
    return MSR3D_EINVAL;
  if (njobs == 0) return 0;
  if (!jobs) return MSR3D_EINVAL;
  if (!Pq || !sp || ldp < K || (ldp % 16) || !al16(Pq) || !al4(sp)) return MSR3D_EINVAL;
  if (R > 0 && (!P2 || ldp2 < R || (ldp2 % 8) || !al16(P2))) return MSR3D_EINVAL;
  if (swiglu && (njobs != 2 || jobs[0].N != jobs[1].N || !jobs[0].C)) return MSR3D_EINVAL;
  long long rows = 0;
  bool pairs = true;                                  // every job's N a multiple of 32: two tiles a workgroup possible
  for (int j = 0; j < njobs; ++j) {
    const msr3d_fp8_skinny_job_t &jb = jobs[j];
    if (jb.N <= 0 || (jb.N % 16) || !jb.Wq || jb.ldw < K || (jb.ldw % 16) || !al16(jb.Wq) || !jb.sw || !al4(jb.sw))
      return MSR3D_EINVAL;
    if (R > 0 && jb.B2 && (jb.ldb2 < R || (jb.ldb2 % 8) || !al16(jb.B2))) return MSR3D_EINVAL;
    if (!(swiglu && j == 1) && (!jb.C || jb.ldc < jb.N)) return MSR3D_EINVAL;
    rows += jb.N;
    if (jb.N % 32) pairs = false;
  }
  if (M == 0) return 0;
  const int mt = (M + 15) / 16;
  // the tile rule of the bf16 kernel (llm_decode.hip: skinny_launch): the activations a workgroup reads out of L2 and the
  // rows of W it streams are both half the bytes here, so the ratio that rule weighs is the same.  Which rule applies
  // changes the workgroup an output is computed in, never its bits.
  const int tn = swiglu ? 2 : (mt <= 2 ? (rows >= 16384 && pairs) : (pairs && rows / 32 >= kSkinnyWideMinWg)) ? 2 : 1;
  Fp8SkinnyJobs sj{};
  sj.njobs = njobs;
  long long grid = 0;
  for (int j = 0; j < njobs; ++j) {
    sj.W[j] = (const u8 *)jobs[j].Wq; sj.sw[j] = jobs[j].sw; sj.B2[j] = R > 0 ? (const u16 *)jobs[j].B2 : nullptr;
    sj.C[j] = (u16 *)jobs[j].C;
    sj.N[j] = jobs[j].N; sj.ldw[j] = jobs[j].ldw; sj.ldb2[j] = jobs[j].ldb2; sj.ldc[j] = jobs[j].ldc;
    sj.tiles[j] = swiglu ? jobs[j].N / 16 : jobs[j].N / (16 * tn);
    grid += sj.tiles[j];
  }
  if (swiglu) grid = sj.tiles[0];
  hipStream_t st = (hipStream_t)stream;
  const u8 *p = (const u8 *)Pq;
  const u16 *p2 = (const u16 *)P2;
#define MSR3D_FSK(MT, TN, SW) fp8_skinny_kernel<MT, TN, SW><<<(unsigned)grid, 256, 0, st>>>(M, K, R, p, ldp, sp, p2, ldp2, sj)
#define MSR3D_FSK_MT(TN, SW)                                                                                           \
  switch (mt) {                                                                                                        \
    case 1: MSR3D_FSK(1, TN, SW); break;                                                                               \
    case 2: MSR3D_FSK(2, TN, SW); break;                                                                               \
    case 3: MSR3D_FSK(3, TN, SW); break;                                                                               \
    default: MSR3D_FSK(4, TN, SW); break;                                                                              \
  }
  if (swiglu) { MSR3D_FSK_MT(2, true) }
  else if (tn == 2) { MSR3D_FSK_MT(2, false) }
  else { MSR3D_FSK_MT(1, false) }
#undef MSR3D_FSK_MT
#undef MSR3D_FSK
  return (int)hipGetLastError();
}

}  // extern "C"
