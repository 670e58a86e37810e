// llm_decode.hip -- the kernels of one KV-cached decoding step of the LoRA-Llama stack (msr3d_amd/llm/generate.py):
// what transformers' `generate` runs per new token, for N <= 64 live rows (batch x beams); `search` walks a larger batch
// in groups of whole prompts.
//
//     msr3d_bf16_skinny_lowrank   C (M <= 32, N) = P W^T + P2 B2^T      every projection and the head: a weight stream
//     msr3d_bf16_skinny_lowrank_wide   the same for M <= 64: three and four activation tiles a workgroup
//     msr3d_bf16_skinny_fused     the same product (R = 0) with the step's norm as a prologue, its residual addition or its
//                                 rotation + cache append as an epilogue: the bits of the launches it replaces
//     msr3d_fp8_skinny_lowrank    the same product on e4m3 weights and row-quantised activations, M <= 64, half the
//                                 stream (llm_decode_fp8.hip: this file's skinny_kernel on the MX fp8 instruction)
//     msr3d_rope_kv_append        rotate q, k by the row's own position, write k, v into cache slot len[n]
//     msr3d_rope_positions        the prefill twin: (B, T, H, D) rotated by pos (B, T)
//     msr3d_attn_decode           one query row per (row, head) against the row's cache: a stream over K and V
//     msr3d_attn_decode_shared    the same bits with the prompt's keys stored once per prompt: up to 8 rows a workgroup
//     msr3d_kv_reorder            beam search's cache gather, every layer in one launch
//     msr3d_kv_quantize_e4m3, msr3d_rope_kv_append_e4m3, msr3d_attn_decode_e4m3, msr3d_attn_decode_shared_e4m3
//                                 the cache as e4m3 codes with one power-of-two scale per (slot, head): the prefill's
//                                 write, the step's append, and the two attentions as instantiations of the bf16
//                                 kernels on 8-byte pieces -- the bits of the bf16 kernels on the dequantised cache
//     msr3d_decode_select         logits processors + log-softmax + the row's top-k candidates
//
// bf16 storage, fp32 accumulation.  Nothing here uses atomics: every output has one owner and partial results are
// merged in a fixed order, so a step is bit-reproducible.  Lengths and positions are read from device memory (a step
// has no host synchronisation) and every index read from memory is range-checked before it forms an address.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/msr3d_hip.h"
#include "llm_rowmath.h"

namespace {

using namespace msr3d::llm;          // u16, bf2f, f2bf, unpack8, pack8, the RMSNorm row arithmetic, rope_pair
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// a 16-byte piece of a weight: read once per call and never again -- non-temporal, so the stream does not push the
// activations and the K / V cache out of L2
__device__ __forceinline__ u32x4 load_stream(const u16 *p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
}
__device__ __forceinline__ u32x4 load_keep(const u16 *p) { return *reinterpret_cast<const u32x4 *>(p); }
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- skinny product -------------------------------------------------------------------------------------------
// v_mfma_f32_16x16x32_bf16 with the ACTIVATIONS as the 16-row side: lane l supplies P[row l & 15][k0 + 8 (l >> 4) + j] and
// W[n0 + (l & 15)][k0 + 8 (l >> 4) + j], j < 8 -- for W that is 16 contiguous bytes of a k-contiguous weight row, loaded
// straight from memory into the operand registers (no LDS: nothing of W is shared between waves).  A workgroup of four
// waves owns 16 TN rows of W; the waves split K in 128-wide chunks, keep the loads of the next chunk in flight while the
// matrix pipe works on this one, and add their partial sums through LDS in wave order.  The activations (M rows, a few
// hundred KB at most) are read from L2 by every workgroup -- 32 x 11008 bf16 do not fit the 160 KB of LDS, and staging
// K in slices would put a barrier into the weight stream.
// MT = 3, 4 (33 .. 64 rows, the wide entry): a[MT][4] and its prefetch copy are 32 MT registers; MT = 4, TN = 2 compiles to
// 222 VGPRs + 32 AGPRs, no scratch, two waves a SIMD, 32 KB of LDS.  Row m of an accumulator tile comes from row m of the
// activation operand alone, so a row of C never sees another row of P (NaN included), whatever MT.

// the wide entry takes two tiles of W a workgroup only where that still gives every CU of the part a workgroup
constexpr long long kSkinnyWideMinWg = 256;
struct SkinnyJobs {
  const u16 *W[3];
  const u16 *B2[3];
  u16 *C[3];
  int N[3];
  int ldw[3], ldb2[3], ldc[3];
  int tiles[3];      // exclusive prefix sums of the jobs' tile counts are formed in the kernel (njobs <= 3)
  int njobs;
};

// What msr3d_bf16_skinny_fused adds to the product (step="fused", generate.CachedDecoder): the launches around it in a
// decode step, restated as a prologue on its activation operand and as epilogues on its finished sums -- each through the
// device functions of the launch it replaces (llm_rowmath.h), so the bits of the split chain.  Nothing changes the sums:
// every output element is still the four waves' K quarters added in wave order.
//   NORM  (q | k | v, gate | up, the head)  the operand is RMSNorm(P) nw: rmsnorm_fwd_kernel's rstd per row, computed by
//         every workgroup for its M rows before the K loop (one wave a row, waves taking rows w, w + 4, ...), and its two
//         roundings applied to each 16-byte piece as it enters the matrix pipe.  K = hidden: K % 512 == 0, K <= 8192.
//   RES   (o, down)  C = bf16(res + bf16(sum)): the addition rmsnorm_fwd_kernel does in front of the next norm.
//   ROPE  (q | k | v on a bf16 cache)  rope_kv_append_kernel: a 16-row tile of W is eight columns [i0, i0 + 8) of ONE head
//         and their eight partners [i0 + D / 2, ...), so both halves of each rotary pair meet in one workgroup under the
//         plain entry's own tile rule (pairing the 16-column tiles c and c + D / 2 instead forces two tiles a workgroup:
//         384 workgroups for Vicuna's q | k | v where the plain launch has 768, 1.5 a CU, and the launch measured 10 us
//         slower for it); q rotated -> C[0], k rotated and v -> slot len[n] of the planes (the same guard: a slot outside
//         0 .. Tmax - 1 writes nothing to the cache, q is still rotated).
struct SkinnyFused {
  const u16 *nw;                 // NORM: the norm weight (K), eps, 1 / K as a float
  float eps, inv_k;
  const u16 *res;                // RES: the residual operand (M, N), row stride ldres
  int ldres;
  int H, D, table_rows, Tmax;    // ROPE: heads x head size = every job's N; cos / sin (table_rows, D); planes (M, Tmax, H, D)
  const int *pos, *len;
  const float *cs, *sn;
  u16 *kc, *vc;
};

// one 16-byte piece of the activations as the matrix pipe reads it under NORM: rmsnorm_fwd_kernel's y for these elements
__device__ __forceinline__ u32x4 norm_operand(u32x4 x, u32x4 nw, float rstd) {
  float s[8], gf[8];
  unpack8(__builtin_bit_cast(uint4, x), s);
  unpack8(__builtin_bit_cast(uint4, nw), gf);
  return __builtin_bit_cast(u32x4, rms_scale8(s, gf, rstd));
}

// THE product: skinny_kernel (the plain entries) and skinny_fused_kernel are this body
template <int MT, int TN, bool SWIGLU, bool NORM, bool RES, bool ROPE>
__device__ __forceinline__ void skinny_body(int M, int K, int R, const u16 *__restrict__ P, int ldp,
                                            const u16 *__restrict__ P2, int ldp2, const SkinnyJobs &jobs,
                                            const SkinnyFused &fz) {
  static_assert(!(ROPE && (SWIGLU || RES)) && !(SWIGLU && RES), "epilogues exclude each other");
  __shared__ float red[4][MT * TN][64][4];
  __shared__ float rstd_s[NORM ? MT * 16 : 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  int tile = blockIdx.x, job = 0;
  if (!SWIGLU) {
    while (job + 1 < jobs.njobs && tile >= jobs.tiles[job]) { tile -= jobs.tiles[job]; ++job; }
  }
  // SWIGLU: job 0 = gate, job 1 = up, the workgroup takes the SAME 16 rows of both (TN == 2 is the job index)
  // ROPE: tile tt = (head, c), c < D / 16: the rows [8 c, 8 c + 8) of the head's two halves
  const int rope_tiles = ROPE ? fz.D >> 4 : 1, half = ROPE ? fz.D >> 1 : 0;
  const u16 *wrow[TN];
  const u16 *brow[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int j = SWIGLU ? t : job;
    const int tt = tile * TN + t;
    const int n = SWIGLU ? tile * 16 + r16
                         : (ROPE ? (tt / rope_tiles) * fz.D + (tt % rope_tiles) * 8 + (r16 & 7) + (r16 >> 3) * half
                                 : tt * 16 + r16);
    wrow[t] = jobs.W[j] + (size_t)n * jobs.ldw[j] + 8 * g;
    brow[t] = jobs.B2[j] ? jobs.B2[j] + (size_t)n * jobs.ldb2[j] + 8 * g : nullptr;
  }
  const u16 *prow[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = min(m * 16 + r16, M - 1);       // rows >= M: a valid row is read and its result not stored
    prow[m] = P + (size_t)row * ldp + 8 * g;
  }
  f32x4 acc[MT][TN];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int chunks = K >> 7;
  const int c0 = (chunks * wave) >> 2, c1 = (chunks * (wave + 1)) >> 2;
  u32x4 w[TN][4], a[MT][4], nw[NORM ? 4 : 1];
  const u16 *nrow = NORM ? fz.nw + 8 * g : nullptr;   // the norm weight's pieces travel with the activations'
  if (c0 < c1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int t = 0; t < TN; ++t) w[t][i] = load_stream(wrow[t] + (size_t)c0 * 128 + 32 * i);
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m][i] = load_keep(prow[m] + (size_t)c0 * 128 + 32 * i);
      if (NORM) nw[i] = load_keep(nrow + (size_t)c0 * 128 + 32 * i);
    }
  }
  float rstd[MT];
  if (NORM) {
    // rmsnorm_fwd_kernel's row walk, under the first chunk's weight loads: lane l owns the 16-byte vectors v 64 + l, the
    // sum of squares grows in (v, e) order (eight vectors of loads in flight change when a vector arrives, not the order)
    const int V = K >> 9;
    for (int row = wave; row < M; row += 4) {         // (wave-uniform)
      const u16 *xr = P + (size_t)row * ldp + 8 * lane;
      float ss = 0.f;
      for (int v0 = 0; v0 < V; v0 += 8) {
        uint4 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (v0 + u < V) x[u] = *reinterpret_cast<const uint4 *>(xr + (size_t)(v0 + u) * 512);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (v0 + u < V) {
            float s[8];
            unpack8(x[u], s);
            ss = rms_sumsq8(s, ss);
          }
      }
      const float r = rms_rstd(ss, fz.inv_k, fz.eps);
      if (lane == 0) rstd_s[row] = r;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) rstd[m] = rstd_s[min(m * 16 + r16, M - 1)];
  }
  for (int c = c0; c < c1; ++c) {
    u32x4 wn[TN][4], an[MT][4], nwn[NORM ? 4 : 1];
    if (c + 1 < c1) {                               // (wave-uniform: the next chunk's loads go out before this one's MFMAs)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int t = 0; t < TN; ++t) wn[t][i] = load_stream(wrow[t] + (size_t)(c + 1) * 128 + 32 * i);
#pragma unroll
        for (int m = 0; m < MT; ++m) an[m][i] = load_keep(prow[m] + (size_t)(c + 1) * 128 + 32 * i);
        if (NORM) nwn[i] = load_keep(nrow + (size_t)(c + 1) * 128 + 32 * i);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const u32x4 am = NORM ? norm_operand(a[m][i], nw[i], rstd[m]) : a[m][i];
#pragma unroll
        for (int t = 0; t < TN; ++t) acc[m][t] = mfma(am, w[t][i], acc[m][t]);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int t = 0; t < TN; ++t) w[t][i] = wn[t][i];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m][i] = an[m][i];
      if (NORM) nw[i] = nwn[i];
    }
  }
  if (wave == 3 && R > 0) {
    // the low-rank pair rides as R / 32 extra k steps: P2 (M, R) = s P A^T, B2 (N, R) = B, zero-padded
    for (int k = 0; k < R; k += 32) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int row = min(m * 16 + r16, M - 1);
        const u32x4 pa = load_keep(P2 + (size_t)row * ldp2 + 8 * g + k);
#pragma unroll
        for (int t = 0; t < TN; ++t)
          if (brow[t]) acc[m][t] = mfma(pa, load_keep(brow[t] + k), acc[m][t]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave][m * TN + t][lane][i] = acc[m][t][i];
  __syncthreads();
  // accumulator element i of lane l is C[row 4 (l >> 4) + i][column l & 15]; the four waves' partial sums in wave order
  if (SWIGLU) {
    for (int e = threadIdx.x; e < MT * 256; e += 256) {
      const int m = e >> 8, l = (e >> 2) & 63, i = e & 3;
      const int row = m * 16 + 4 * (l >> 4) + i, col = l & 15;
      if (row >= M) continue;
      float gsum = 0.f, usum = 0.f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) { gsum += red[wv][m * TN + 0][l][i]; usum += red[wv][m * TN + (TN - 1)][l][i]; }
      // the same roundings as the training graph: gate and up are bf16 tensors, silu a bf16 op of its own
      const float gb = bf2f(f2bf(gsum)), ub = bf2f(f2bf(usum));
      const float sg = bf2f(f2bf(gb / (1.0f + expf(-gb))));
      jobs.C[0][(size_t)row * jobs.ldc[0] + tile * 16 + col] = f2bf(sg * ub);
    }
  } else if (ROPE) {
    // rope_kv_append_kernel on the sums rounded to bf16 (what it reads from the projections' output): a thread takes the
    // pair (x[d], x[d + D / 2]) of head `hd` -- columns p and p + 8 of the tile, lanes l and l + 8 of the accumulator
    for (int e = threadIdx.x; e < MT * TN * 128; e += 256) {
      const int mt = e >> 7, r = (e >> 3) & 15, p = e & 7;
      const int m = mt / TN, tt = tile * TN + mt % TN;
      const int row = m * 16 + r, l = (r >> 2) * 16 + p, i = r & 3;
      const int hd = tt / rope_tiles, d = (tt % rope_tiles) * 8 + p;
      if (row >= M) continue;
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) { sa += red[wv][mt][l][i]; sb += red[wv][mt][l + 8][i]; }
      float ya = bf2f(f2bf(sa)), yb = bf2f(f2bf(sb));
      if (job < 2) {
        const int t = min(max(fz.pos[row], 0), fz.table_rows - 1);
        const float *cr = fz.cs + (size_t)t * fz.D + d, *sr = fz.sn + (size_t)t * fz.D + d;
        rope_pair(ya, yb, cr[0], cr[half], sr[0], sr[half], ya, yb);
      }
      u16 *dst;
      if (job == 0) {
        dst = jobs.C[0] + (size_t)row * jobs.ldc[0] + (size_t)hd * fz.D + d;
      } else {
        const int slot = fz.len[row];
        if (slot < 0 || slot >= fz.Tmax) continue;   // a full cache: nothing is written outside it
        dst = (job == 1 ? fz.kc : fz.vc) + (((size_t)row * fz.Tmax + slot) * fz.H + hd) * fz.D + d;
      }
      dst[0] = f2bf(ya);
      dst[half] = f2bf(yb);
    }
  } else {
    for (int e = threadIdx.x; e < MT * TN * 256; e += 256) {
      const int mt = e >> 8, l = (e >> 2) & 63, i = e & 3;
      const int m = mt / TN, t = mt % TN;
      const int row = m * 16 + 4 * (l >> 4) + i, col = l & 15;
      if (row >= M) continue;
      float s = 0.f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) s += red[wv][mt][l][i];
      const size_t n = (size_t)(tile * TN + t) * 16 + col;
      if (RES) s = residual_add(bf2f(fz.res[(size_t)row * fz.ldres + n]), bf2f(f2bf(s)));
      jobs.C[job][(size_t)row * jobs.ldc[job] + n] = f2bf(s);
    }
  }
}

template <int MT, int TN, bool SWIGLU>
__global__ __launch_bounds__(256) void skinny_kernel(int M, int K, int R, const u16 *__restrict__ P, int ldp,
                                                     const u16 *__restrict__ P2, int ldp2, SkinnyJobs jobs) {
  skinny_body<MT, TN, SWIGLU, false, false, false>(M, K, R, P, ldp, P2, ldp2, jobs, SkinnyFused{});
}

// (R = 0: the merged planes and the head have no low-rank pair, and the r-row product of the other sources reads the
// normed activations as a tensor)
template <int MT, int TN, bool SWIGLU, bool NORM, bool RES, bool ROPE>
__global__ __launch_bounds__(256) void skinny_fused_kernel(int M, int K, const u16 *__restrict__ P, int ldp, SkinnyJobs jobs,
                                                           SkinnyFused fz) {
  skinny_body<MT, TN, SWIGLU, NORM, RES, ROPE>(M, K, 0, P, ldp, nullptr, 0, jobs, fz);
}

// ---- rotary embedding by explicit positions ------------------------------------------------------------------
// The arithmetic of rope_vec_kernel (llm_layer.hip), operation for operation: where pos is arange the results are
// the same bits (tests/test_llm_decode_gpu.py holds the two together).  A thread owns eight adjacent pairs of one head.
struct RopeCoef {
  float c1[8], c2[8], s1[8], s2[8];
};
__device__ __forceinline__ RopeCoef rope_coef(const float *__restrict__ cs, const float *__restrict__ sn, int t, int D, int i0) {
  RopeCoef r;
  const int half = D >> 1;
  const float *cr = cs + (size_t)t * D + i0, *sr = sn + (size_t)t * D + i0;
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const float4 a = *reinterpret_cast<const float4 *>(cr + 4 * v), b = *reinterpret_cast<const float4 *>(cr + half + 4 * v);
    const float4 e = *reinterpret_cast<const float4 *>(sr + 4 * v), f = *reinterpret_cast<const float4 *>(sr + half + 4 * v);
    r.c1[4 * v] = a.x; r.c1[4 * v + 1] = a.y; r.c1[4 * v + 2] = a.z; r.c1[4 * v + 3] = a.w;
    r.c2[4 * v] = b.x; r.c2[4 * v + 1] = b.y; r.c2[4 * v + 2] = b.z; r.c2[4 * v + 3] = b.w;
    r.s1[4 * v] = e.x; r.s1[4 * v + 1] = e.y; r.s1[4 * v + 2] = e.z; r.s1[4 * v + 3] = e.w;
    r.s2[4 * v] = f.x; r.s2[4 * v + 1] = f.y; r.s2[4 * v + 2] = f.z; r.s2[4 * v + 3] = f.w;
  }
  return r;
}
__device__ __forceinline__ void rope_rotate(const RopeCoef &r, uint4 va, uint4 vb, uint4 &oa, uint4 &ob) {
  float a[8], b[8], ya[8], yb[8];
  unpack8(va, a);
  unpack8(vb, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) rope_pair(a[e], b[e], r.c1[e], r.c2[e], r.s1[e], r.s2[e], ya[e], yb[e]);
  oa = pack8(ya);
  ob = pack8(yb);
}

__global__ __launch_bounds__(256) void rope_positions_kernel(long long n_items, int H, int D, u16 *__restrict__ x0,
                                                             u16 *__restrict__ x1, const int *__restrict__ pos, int table_rows,
                                                             const float *__restrict__ cs, const float *__restrict__ sn) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;     // one (b t, h, 16-dim piece) per thread
  if (id >= n_items) return;
  const int half = D >> 1, npc = D >> 4;
  const int c = (int)(id % npc);
  const int h = (int)((id / npc) % H);
  const long long bt = id / ((long long)npc * H);
  const int t = min(max(pos[bt], 0), table_rows - 1);
  const RopeCoef r = rope_coef(cs, sn, t, D, 8 * c);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    u16 *x = which ? x1 : x0;
    if (!x) continue;
    u16 *row = x + (bt * H + h) * D + 8 * c;
    uint4 oa, ob;
    rope_rotate(r, *reinterpret_cast<const uint4 *>(row), *reinterpret_cast<const uint4 *>(row + half), oa, ob);
    *reinterpret_cast<uint4 *>(row) = oa;
    *reinterpret_cast<uint4 *>(row + half) = ob;
  }
}

__global__ __launch_bounds__(256) void rope_kv_append_kernel(int n_items, int H, int D, int Tmax, u16 *__restrict__ q,
                                                             const u16 *__restrict__ k, const u16 *__restrict__ v, int ld,
                                                             const int *__restrict__ pos, const int *__restrict__ len,
                                                             int table_rows, const float *__restrict__ cs,
                                                             const float *__restrict__ sn, u16 *__restrict__ kc,
                                                             u16 *__restrict__ vc) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= n_items) return;
  const int half = D >> 1, npc = D >> 4;
  const int c = id % npc, h = (id / npc) % H, n = id / (npc * H);
  const int t = min(max(pos[n], 0), table_rows - 1);
  const int slot = len[n];
  const RopeCoef r = rope_coef(cs, sn, t, D, 8 * c);
  const size_t src = (size_t)n * ld + (size_t)h * D + 8 * c;
  uint4 oa, ob;
  rope_rotate(r, *reinterpret_cast<const uint4 *>(q + src), *reinterpret_cast<const uint4 *>(q + src + half), oa, ob);
  *reinterpret_cast<uint4 *>(q + src) = oa;
  *reinterpret_cast<uint4 *>(q + src + half) = ob;
  if (slot < 0 || slot >= Tmax) return;             // a full cache: nothing is written outside it
  rope_rotate(r, *reinterpret_cast<const uint4 *>(k + src), *reinterpret_cast<const uint4 *>(k + src + half), oa, ob);
  const size_t dst = (((size_t)n * Tmax + slot) * H + h) * D + 8 * c;
  *reinterpret_cast<uint4 *>(kc + dst) = oa;
  *reinterpret_cast<uint4 *>(kc + dst + half) = ob;
  *reinterpret_cast<uint4 *>(vc + dst) = *reinterpret_cast<const uint4 *>(v + src);
  *reinterpret_cast<uint4 *>(vc + dst + half) = *reinterpret_cast<const uint4 *>(v + src + half);
}

// ---- the e4m3 cache's quantiser -----------------------------------------------------------------------------------
// kv_cache.torch_kv_quantize is the statement: per (slot, head) e = the smallest integer with amax 2^-e <= 448, from
// amax's own exponent and mantissa fields (448 = 1.75 2^8: a mantissa above 1.75 takes the next exponent), clamped at
// -126, stored biased by 127; codes = RNE_e4m3(x 2^-e), an exact scaling and one rounding.
// `a` = amax's bf16 bits, sign cleared (for finite values the integer order is the order of the magnitudes).
__device__ __forceinline__ int kv_biased_exponent(unsigned a) {
  if (a == 0) return 127;
  const int E = (int)(a >> 7), M = (int)(a & 0x7fu);
  if (E == 0) return 1;                             // a bf16 subnormal: the clamp
  const int e = max(E - 126 - (M <= 0x60 ? 9 : 8), -126);
  return e + 127;
}
__device__ __forceinline__ unsigned amax_bits8(uint4 v) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned a = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) a = max(a, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
  return a;
}
// eight bf16 values times 2^(127 - b) -> eight e4m3 codes
__device__ __forceinline__ uint2 kv_encode8(uint4 v, int b) {
  const float inv = __uint_as_float((unsigned)(254 - b) << 23);
  float f[8];
  unpack8(v, f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, hi, true);
  return make_uint2((unsigned)lo, (unsigned)hi);
}

// one (row, head) per D / 8 adjacent lanes, eight values a lane; amax over those lanes by shuffles (a group lies inside
// one wave and is live or idle as a whole: n_items is a multiple of D / 8)
template <int D>
__global__ __launch_bounds__(256) void kv_quantize_kernel(long long n_items, int H, const u16 *__restrict__ x, int ldx,
                                                          unsigned char *__restrict__ codes,
                                                          unsigned char *__restrict__ exps, int lde) {
  constexpr int LPH = D / 8;
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n_items) return;
  const int piece = (int)(id % LPH), h = (int)((id / LPH) % H);
  const long long row = id / ((long long)LPH * H);
  const uint4 v = *reinterpret_cast<const uint4 *>(x + (size_t)row * ldx + (size_t)h * D + 8 * piece);
  unsigned a = amax_bits8(v);
#pragma unroll
  for (int s = 1; s < LPH; s <<= 1) a = max(a, (unsigned)__shfl_xor((int)a, s));
  const int b = kv_biased_exponent(a);
  *reinterpret_cast<uint2 *>(codes + ((size_t)row * H + h) * D + 8 * piece) = kv_encode8(v, b);
  if (piece == 0) exps[(size_t)row * lde + h] = (unsigned char)b;
}

// rope_kv_append_kernel with the quantiser behind it: the same thread layout (a thread owns elements [8 c, 8 c + 8) of
// both halves of a head, D / 16 lanes a head), q rotated with the same operations, k rotated and rounded to bf16 as
// there and then quantised, v quantised
template <int D>
__global__ __launch_bounds__(256) void rope_kv_append_e4m3_kernel(int n_items, int H, int Tmax, u16 *__restrict__ q,
                                                                  const u16 *__restrict__ k, const u16 *__restrict__ v,
                                                                  int ld, const int *__restrict__ pos,
                                                                  const int *__restrict__ len, int table_rows,
                                                                  const float *__restrict__ cs, const float *__restrict__ sn,
                                                                  unsigned char *__restrict__ kc,
                                                                  unsigned char *__restrict__ vc,
                                                                  unsigned char *__restrict__ ke,
                                                                  unsigned char *__restrict__ ve, int lde) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= n_items) return;
  constexpr int half = D >> 1, npc = D >> 4;
  const int c = id % npc, h = (id / npc) % H, n = id / (npc * H);
  const int t = min(max(pos[n], 0), table_rows - 1);
  const int slot = len[n];
  const RopeCoef r = rope_coef(cs, sn, t, D, 8 * c);
  const size_t src = (size_t)n * ld + (size_t)h * D + 8 * c;
  uint4 oa, ob;
  rope_rotate(r, *reinterpret_cast<const uint4 *>(q + src), *reinterpret_cast<const uint4 *>(q + src + half), oa, ob);
  *reinterpret_cast<uint4 *>(q + src) = oa;
  *reinterpret_cast<uint4 *>(q + src + half) = ob;
  if (slot < 0 || slot >= Tmax) return;             // a full cache: nothing is written outside it (the whole head's lanes)
  rope_rotate(r, *reinterpret_cast<const uint4 *>(k + src), *reinterpret_cast<const uint4 *>(k + src + half), oa, ob);
  const uint4 va = *reinterpret_cast<const uint4 *>(v + src), vb = *reinterpret_cast<const uint4 *>(v + src + half);
  unsigned ak = max(amax_bits8(oa), amax_bits8(ob)), av = max(amax_bits8(va), amax_bits8(vb));
#pragma unroll
  for (int s = 1; s < npc; s <<= 1) {
    ak = max(ak, (unsigned)__shfl_xor((int)ak, s));
    av = max(av, (unsigned)__shfl_xor((int)av, s));
  }
  const int bk = kv_biased_exponent(ak), bv = kv_biased_exponent(av);
  const size_t sl = (size_t)n * Tmax + slot, dst = (sl * H + h) * D + 8 * c;
  *reinterpret_cast<uint2 *>(kc + dst) = kv_encode8(oa, bk);
  *reinterpret_cast<uint2 *>(kc + dst + half) = kv_encode8(ob, bk);
  *reinterpret_cast<uint2 *>(vc + dst) = kv_encode8(va, bv);
  *reinterpret_cast<uint2 *>(vc + dst + half) = kv_encode8(vb, bv);
  if (c == 0) { ke[sl * lde + h] = (unsigned char)bk; ve[sl * lde + h] = (unsigned char)bv; }
}

// ---- decode attention -------------------------------------------------------------------------------------------
// grid (H, N, S): split s of (row n, head h) takes the keys [s L / S, (s + 1) L / S) of the row's L = len[n] + len_add.
// A key's D values are 16-byte pieces over D / 8 lanes, so a wave reads 64 / (D / 8) keys per step (4 at D = 128, 8 at
// 64) and its four waves interleave those steps; every lane group carries its own online-softmax state (max, sum,
// eight output values), merged over the wave's groups by shuffles, over the waves through LDS in wave order and -- when
// S > 1 -- over the splits by attn_merge_kernel in split order.  exp2 throughout, the scale folded with log2 e.
constexpr float kNegBig = -1.0e30f;

// The arithmetic of a (row, head), stated once for attn_decode_kernel and attn_decode_shared_kernel -- the two give the
// same bits because they call these four in the same order per row.  Every multiply-add is an explicit fmaf: left as
// a * b + c * d, the compiler chooses per inlined copy which product it fuses (or none, where it packs two lanes), and
// two kernels that share the expression still differ in the last bit.
// One key (this lane's eight values of K and of V) into a lane group's online-softmax state.  SCALED (the e4m3 cache):
// the key is kf 2^a, vf 2^b with ks = 2^a, vs = 2^b given apart -- ks multiplies the reduced score and vs multiplies p
// before the p v products (not l).  A power of two commutes with every rounding of the chain while nothing is subnormal,
// so the state is, bit for bit, what the unscaled form makes of the multiplied-out key.
template <int LPK, bool SCALED>
__device__ __forceinline__ void attn_key_apply(const float (&qf)[8], const float (&kf)[8], const float (&vf)[8], float ks,
                                               float vs, bool on, float &m, float &l, float (&o)[8]) {
  float sc = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) sc = fmaf(qf[e], kf[e], sc);
#pragma unroll
  for (int x = 1; x < LPK; x <<= 1) sc += __shfl_xor(sc, x);
  if (SCALED) sc *= ks;
  if (on) {
    const float mn = fmaxf(m, sc);
    const float f = exp2f(m - mn), p = exp2f(sc - mn);
    l = fmaf(l, f, p);
    const float pv = SCALED ? p * vs : p;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(o[e], f, pv * vf[e]);
    m = mn;
  }
}

// A lane's piece of one cache slot as the decode attention reads it: eight values of K and eight of V.
struct KvPieceBf16 {
  uint4 k, v;
};
struct KvPieceE4m3 {
  uint2 k, v;          // eight OCP e4m3 codes each
  float ks, vs;        // the (slot, head)'s scales 2^(b - 127)
};
__device__ __forceinline__ void unpack8_e4m3(uint2 c, float (&f)[8]) {
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
  const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), g = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = d[0]; f[5] = d[1]; f[6] = g[0]; f[7] = g[1];
}
__device__ __forceinline__ float e8m0_scale(unsigned char b) { return __uint_as_float((unsigned)b << 23); }

template <int LPK>
__device__ __forceinline__ void attn_key_update(const float (&qf)[8], const KvPieceBf16 &c, bool on, float &m, float &l,
                                                float (&o)[8]) {
  float kf[8], vf[8];
  unpack8(c.k, kf);
  unpack8(c.v, vf);
  attn_key_apply<LPK, false>(qf, kf, vf, 1.f, 1.f, on, m, l, o);
}
template <int LPK>
__device__ __forceinline__ void attn_key_update(const float (&qf)[8], const KvPieceE4m3 &c, bool on, float &m, float &l,
                                                float (&o)[8]) {
  float kf[8], vf[8];
  unpack8_e4m3(c.k, kf);
  unpack8_e4m3(c.v, vf);
  attn_key_apply<LPK, true>(qf, kf, vf, c.ks, c.vs, on, m, l, o);
}

// K / V planes (rows, slots, H, D) and how a lane loads its piece of slot `sl` (an index over rows x slots) of head h.
// e4m3: codes in the bf16 planes' shape, and the exponents (rows, slots, lde) bytes, lde >= H.
struct KvPlanesBf16 {
  const u16 *k, *v;
  using Piece = KvPieceBf16;
  static constexpr int kRowsInFlight = 4;      // attn_decode_kernel's U
  template <int D>
  __device__ __forceinline__ Piece load(size_t sl, int H, int h, int piece) const {
    const size_t off = (sl * H + h) * D + 8 * piece;
    return Piece{*reinterpret_cast<const uint4 *>(k + off), *reinterpret_cast<const uint4 *>(v + off)};
  }
};
struct KvPlanesE4m3 {
  const unsigned char *k, *v, *ke, *ve;
  int lde;
  using Piece = KvPieceE4m3;
  static constexpr int kRowsInFlight = 8;
  template <int D>
  __device__ __forceinline__ Piece load(size_t sl, int H, int h, int piece) const {
    const size_t off = (sl * H + h) * D + 8 * piece, eo = sl * lde + h;
    return Piece{*reinterpret_cast<const uint2 *>(k + off), *reinterpret_cast<const uint2 *>(v + off), e8m0_scale(ke[eo]),
                 e8m0_scale(ve[eo])};
  }
};

// the wave's lane groups (same dims, different keys): butterfly over the group index -- every lane of a dim ends with the
// same value, in an order fixed by the lane numbers
template <int LPK>
__device__ __forceinline__ void attn_group_merge(int lane, float &m, float &l, float (&o)[8]) {
#pragma unroll
  for (int x = LPK; x < 64; x <<= 1) {
    const float m2 = __shfl_xor(m, x), l2 = __shfl_xor(l, x);
    const float mn = fmaxf(m, m2);
    // (both factors from the lower and the upper partner in the same roles on both sides: a + b with a from the lower lane)
    const bool low = (lane & x) == 0;
    const float fa = exp2f((low ? m : m2) - mn), fb = exp2f((low ? m2 : m) - mn);
    l = fmaf(low ? l : l2, fa, (low ? l2 : l) * fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float o2 = __shfl_xor(o[e], x);
      o[e] = fmaf(low ? o[e] : o2, fa, (low ? o2 : o[e]) * fb);
    }
    m = mn;
  }
}

// the four waves' states of dim d out of LDS, in wave order
__device__ __forceinline__ void attn_wave_merge(const float *sm, const float *sl, const float *so, int ld_so, int d, float &mm,
                                                float &ll, float &oo) {
  mm = sm[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) mm = fmaxf(mm, sm[w]);
  ll = 0.f, oo = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float f = exp2f(sm[w] - mm);
    ll = fmaf(sl[w], f, ll);
    oo = fmaf(so[w * ld_so + d], f, oo);
  }
}

// dim d of (row n, head h): a split's partial state, or the output when there is one split
template <int D>
__device__ __forceinline__ void attn_store(int n, int h, int H, int s, int S, int d, float mm, float ll, float oo,
                                           u16 *__restrict__ out, int ldo, float *__restrict__ part) {
  if (part) {
    float *pp = part + (((size_t)n * H + h) * S + s) * (D + 2);
    if (d == 0) { pp[0] = mm; pp[1] = ll; }
    pp[2 + d] = oo;
  } else {
    out[(size_t)n * ldo + (size_t)h * D + d] = f2bf(ll > 0.f ? oo / ll : 0.f);       // no visible key: 0
  }
}

// Planes = KvPlanesBf16 or KvPlanesE4m3: the same walk -- D / 8 lanes a key, eight values a lane, the same keys per lane
// group in the same order -- on 16-byte or 8-byte pieces.  U wave steps of loads are in flight before the first is used;
// the e4m3 form takes twice as many, the same bytes (U changes when a key is loaded, not the order it is applied in).
template <int D, class Planes>
__global__ __launch_bounds__(256) void attn_decode_kernel(int Tmax, int H, const u16 *__restrict__ q, int ldq,
                                                          const Planes cache,
                                                          const int *__restrict__ len, int len_add,
                                                          const unsigned char *__restrict__ keep, float scale_log2,
                                                          u16 *__restrict__ out, int ldo, float *__restrict__ part) {
  constexpr int LPK = D / 8, KPW = 64 / LPK;
  __shared__ float sm[4], sl[4], so[4][D];
  const int h = blockIdx.x, n = blockIdx.y, s = blockIdx.z, S = gridDim.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int piece = lane % LPK, grp = lane / LPK;
  const int L = min(max(len[n] + len_add, 0), Tmax);
  const int t0 = (int)(((long long)L * s) / S), t1 = (int)(((long long)L * (s + 1)) / S);
  float qf[8];
  unpack8(*reinterpret_cast<const uint4 *>(q + (size_t)n * ldq + (size_t)h * D + 8 * piece), qf);
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] *= scale_log2;
  float m = kNegBig, l = 0.f, o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  const size_t row0 = (size_t)n * Tmax;
  const unsigned char *kp = keep ? keep + row0 : nullptr;
  constexpr int U = Planes::kRowsInFlight;
  for (int tb = t0 + wave * KPW; tb < t1; tb += 4 * KPW * U) {
    typename Planes::Piece c[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tb + u * 4 * KPW + grp;
      on[u] = t < t1 && (!kp || kp[t]);
      c[u] = cache.template load<D>(row0 + (on[u] ? t : t0), H, h, piece);        // (t0 < t1 <= Tmax here: in bounds)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) attn_key_update<LPK>(qf, c[u], on[u], m, l, o);
  }
  attn_group_merge<LPK>(lane, m, l, o);
  if (grp == 0) {
    if (piece == 0) { sm[wave] = m; sl[wave] = l; }
#pragma unroll
    for (int e = 0; e < 8; ++e) so[wave][8 * piece + e] = o[e];
  }
  __syncthreads();
  if (threadIdx.x < D) {
    const int d = threadIdx.x;
    float mm, ll, oo;
    attn_wave_merge(sm, sl, &so[0][0], D, d, mm, ll, oo);
    attn_store<D>(n, h, H, s, S, d, mm, ll, oo, out, ldo, part);
  }
}

template <int D>
__global__ __launch_bounds__(D) void attn_merge_kernel(int H, int S, const float *__restrict__ part, u16 *__restrict__ out,
                                                       int ldo) {
  const int h = blockIdx.x, n = blockIdx.y, d = threadIdx.x;
  const float *pp = part + ((size_t)n * H + h) * S * (D + 2);
  float mm = kNegBig;
  for (int s = 0; s < S; ++s) mm = fmaxf(mm, pp[(size_t)s * (D + 2)]);
  float ll = 0.f, oo = 0.f;
  for (int s = 0; s < S; ++s) {
    const float f = exp2f(pp[(size_t)s * (D + 2)] - mm);
    ll += pp[(size_t)s * (D + 2) + 1] * f;
    oo += pp[(size_t)s * (D + 2) + 2 + d] * f;
  }
  out[(size_t)n * ldo + (size_t)h * D + d] = f2bf(ll > 0.f ? oo / ll : 0.f);
}

// ---- decode attention, the prompt's keys stored once per prompt ---------------------------------------------------
// The G rows of prompt b (beams) share its T prompt slots (`prompt`: planes (B, T, H, D); pkeep (B, T)) and differ only in
// their tails (`tails`: planes (B G, Ttail, H, D)); Planes as in attn_decode_kernel; all G have the same length
// L = T + tail, so the split bounds and the key -> (wave, lane group) assignment of attn_decode_kernel are the same for
// all of them.  grid (H, B ceil(G / 8), S): a workgroup
// serves R <= 8 rows of one prompt (R = G up to 8 rows; above that chunks of 8, the last one partly idle), with every
// row's online-softmax state in registers.  It walks the keys exactly as attn_decode_kernel does for ONE row -- the same
// waves, steps and lane groups -- and applies each key to its R queries with the helpers above: per row the same
// operations on the same values in the same order, so the bits of attn_decode_kernel on the materialised cache.  A wave
// step (KPW keys) that lies wholly inside the prompt issues one K and one V load for all R rows; one that straddles T or
// lies in the tail loads per row.
template <int D, int R, class Planes>
__global__ __launch_bounds__(256) void attn_decode_shared_kernel(int G, int T, int Ttail, int H, const u16 *__restrict__ q,
                                                                 int ldq, const Planes prompt,
                                                                 const unsigned char *__restrict__ pkeep,
                                                                 const Planes tails,
                                                                 const int *__restrict__ tail_len, int len_add,
                                                                 float scale_log2, u16 *__restrict__ out, int ldo,
                                                                 float *__restrict__ part) {
  constexpr int LPK = D / 8, KPW = 64 / LPK;
  __shared__ float sm[R][4], sl[R][4], so[R][4][D];
  const int h = blockIdx.x, s = blockIdx.z, S = gridDim.z;
  const int chunks = (G + 7) / 8;
  const int b = blockIdx.y / chunks, g0 = (blockIdx.y % chunks) * 8;
  const int nr = min(R, G - g0);                      // live rows of this workgroup (< R only in the last chunk of G > 8)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int piece = lane % LPK, grp = lane / LPK;
  const int L = T + min(max(tail_len[b] + len_add, 0), Ttail);
  const int t0 = (int)(((long long)L * s) / S), t1 = (int)(((long long)L * (s + 1)) / S);
  float qf[R][8], m[R], l[R], o[R][8];
  size_t trow[R];                                     // the row's first tail slot; an idle row reads the chunk's last live one
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const size_t n = (size_t)b * G + g0 + min(r, nr - 1);
    trow[r] = n * Ttail;
    unpack8(*reinterpret_cast<const uint4 *>(q + n * ldq + (size_t)h * D + 8 * piece), qf[r]);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[r][e] *= scale_log2;
    m[r] = kNegBig, l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[r][e] = 0.f;
  }
  const size_t prow = (size_t)b * T;
  const unsigned char *pk = pkeep ? pkeep + prow : nullptr;
  constexpr int U = 4;
  for (int tb = t0 + wave * KPW; tb < t1; tb += 4 * KPW * U) {
    if (tb + (U - 1) * 4 * KPW + KPW <= T) {          // (wave-uniform) all U steps inside the prompt: U loads in flight
      typename Planes::Piece c[U];
      bool on[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = tb + u * 4 * KPW + grp;
        on[u] = t < t1 && (!pk || pk[t]);
        c[u] = prompt.template load<D>(prow + (on[u] ? t : t0), H, h, piece);     // (t0 <= tb < T here: in bounds)
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) attn_key_update<LPK>(qf[r], c[u], on[u], m[r], l[r], o[r]);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ts = tb + u * 4 * KPW, t = ts + grp;
        if (ts >= t1) break;                          // (wave-uniform)
        if (ts + KPW <= T) {
          const bool on = t < t1 && (!pk || pk[t]);
          // (T >= 1: slot 0 exists)
          const typename Planes::Piece c = prompt.template load<D>(prow + (on ? t : 0), H, h, piece);
#pragma unroll
          for (int r = 0; r < R; ++r) attn_key_update<LPK>(qf[r], c, on, m[r], l[r], o[r]);
        } else {
          // a lane's key is a prompt slot (t < T) or the row's own tail slot t - T < Ttail (t < t1 <= L); a lane
          // without a key reads prompt slot 0
          const bool tail = t >= T;
          const bool on = t < t1 && (tail || !pk || pk[t]);
          typename Planes::Piece c[R];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool tl = on && tail;
            c[r] = (tl ? tails : prompt).template load<D>(tl ? trow[r] + (size_t)(t - T) : prow + (on ? t : 0), H, h, piece);
          }
#pragma unroll
          for (int r = 0; r < R; ++r) attn_key_update<LPK>(qf[r], c[r], on, m[r], l[r], o[r]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    attn_group_merge<LPK>(lane, m[r], l[r], o[r]);
    if (grp == 0) {
      if (piece == 0) { sm[r][wave] = m[r]; sl[r][wave] = l[r]; }
#pragma unroll
      for (int e = 0; e < 8; ++e) so[r][wave][8 * piece + e] = o[r][e];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nr * D; i += 256) {
    const int r = i / D, d = i % D;
    float mm, ll, oo;
    attn_wave_merge(sm[r], sl[r], &so[r][0][0], D, d, mm, ll, oo);
    attn_store<D>(b * G + g0 + r, h, H, s, S, d, mm, ll, oo, out, ldo, part);
  }
}

// ---- cache gather -----------------------------------------------------------------------------------------------
// dst[p][n][t] = src[p][idx[n]][t], t < len[idx[n]], for every plane p (layers x {k, v}); 16-byte pieces.
__global__ __launch_bounds__(256) void kv_reorder_kernel(int N, int Tmax, int row_vec, const uint4 *__restrict__ src,
                                                         uint4 *__restrict__ dst, const int *__restrict__ idx,
                                                         const int *__restrict__ len) {
  const int n = blockIdx.y, p = blockIdx.z;
  const int from = idx[n];
  if (from < 0 || from >= N) return;                 // not a row of the cache: nothing is read or written
  const long long count = (long long)min(max(len[from], 0), Tmax) * row_vec;
  const uint4 *s = src + ((size_t)p * N + from) * Tmax * row_vec;
  uint4 *d = dst + ((size_t)p * N + n) * Tmax * row_vec;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) d[i] = s[i];
}

// ---- candidate selection ----------------------------------------------------------------------------------------
// One workgroup per row, the row's V scores in LDS as fp32.  order 0 (greedy, transformers' _sample): the processors act
// on the raw logits, then log-softmax; order 1 (transformers' _beam_search): log-softmax first, the processors on the
// log-probabilities.  Then + beam_score[n] and k rounds of arg-max, ties to the lower token id.
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void decode_select_kernel(int V, const u16 *__restrict__ logits, int ldl,
                                                            const long long *__restrict__ prev, int ldprev,
                                                            const int *__restrict__ n_prev, int prev_cap, float penalty,
                                                            int min_length, int eos, const float *__restrict__ beam_score,
                                                            int order, int k, float *__restrict__ out_val,
                                                            int *__restrict__ out_tok) {
  extern __shared__ float sc[];                     // the row's V scores
  __shared__ float rv[4];
  __shared__ int ri[4];
  __shared__ float bcast[2];
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const u16 *lg = logits + (size_t)n * ldl;
  const int np = n_prev ? min(max(n_prev[n], 0), prev_cap) : 0;
  const long long *pv = prev + (size_t)n * ldprev;
  for (int v = tid; v < V; v += 256) sc[v] = bf2f(lg[v]);
  __syncthreads();
  if (order == 0) {
    // every occurrence of a token writes the same value (computed from the unprocessed logit): applied once
    if (penalty != 1.0f)
      for (int i = tid; i < np; i += 256) {
        const long long t = pv[i];
        if (t < 0 || t >= V) continue;
        const float x = bf2f(lg[t]);
        sc[t] = x < 0.f ? x * penalty : x / penalty;
      }
    __syncthreads();
    if (tid == 0 && np < min_length && eos >= 0 && eos < V) sc[eos] = -INFINITY;
    __syncthreads();
  }
  // log-softmax of what is in sc
  float mx = -INFINITY;
  for (int v = tid; v < V; v += 256) mx = fmaxf(mx, sc[v]);
  for (int x = 32; x > 0; x >>= 1) mx = fmaxf(mx, __shfl_xor(mx, x));
  if (lane == 0) rv[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
  __syncthreads();
  float sum = 0.f;
  for (int v = tid; v < V; v += 256) sum += expf(sc[v] - mx);
  for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x);
  if (lane == 0) rv[wave] = sum;
  __syncthreads();
  if (tid == 0) bcast[0] = mx + logf(((rv[0] + rv[1]) + rv[2]) + rv[3]);
  __syncthreads();
  const float lse = bcast[0];
  const float add = beam_score ? beam_score[n] : 0.f;
  if (order == 0) {
    for (int v = tid; v < V; v += 256) sc[v] = (sc[v] - lse) + add;
    __syncthreads();
  } else {
    for (int v = tid; v < V; v += 256) sc[v] = sc[v] - lse;
    __syncthreads();
    if (penalty != 1.0f) {
      for (int i = tid; i < np; i += 256) {
        const long long t = pv[i];
        if (t < 0 || t >= V) continue;
        const float x = bf2f(lg[t]) - lse;             // from the unprocessed value: every occurrence writes the same
        sc[t] = x < 0.f ? x * penalty : x / penalty;
      }
    }
    __syncthreads();
    if (tid == 0 && np < min_length && eos >= 0 && eos < V) sc[eos] = -INFINITY;
    __syncthreads();
    for (int v = tid; v < V; v += 256) sc[v] += add;
    __syncthreads();
  }
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY;
    int bi = V;                                       // V = nothing found yet (taken entries are NaN and never compare)
    for (int v = tid; v < V; v += 256) {
      const float x = sc[v];
      if (x == x && (bi == V || better(x, v, bv, bi))) { bv = x; bi = v; }
    }
    for (int x = 32; x > 0; x >>= 1) {
      const float ov = __shfl_xor(bv, x);
      const int oi = __shfl_xor(bi, x);
      if (oi < V && (bi == V || better(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      bv = rv[0]; bi = ri[0];
      for (int w = 1; w < 4; ++w)
        if (ri[w] < V && (bi == V || better(rv[w], ri[w], bv, bi))) { bv = rv[w]; bi = ri[w]; }
      out_val[(size_t)n * k + r] = bi < V ? bv : -INFINITY;
      out_tok[(size_t)n * k + r] = bi < V ? bi : 0;
      if (bi < V) sc[bi] = __int_as_float(0x7fc00000);
    }
    __syncthreads();
  }
}

// the instantiation for `rows_per_wg` = min(G, 8) rows a workgroup
template <int D, class Planes>
void attn_decode_shared_launch(int rows_per_wg, dim3 grid, hipStream_t st, int G, int T, int Ttail, int H, const u16 *q,
                               int ldq, Planes prompt, const unsigned char *pkeep, Planes tails, const int *tail_len,
                               int len_add, float sl2, u16 *out, int ldo, float *part) {
#define MSR3D_ADS(R)                                                                                                   \
  case R:                                                                                                              \
    attn_decode_shared_kernel<D, R, Planes><<<grid, 256, 0, st>>>(G, T, Ttail, H, q, ldq, prompt, pkeep, tails, tail_len,  \
                                                                  len_add, sl2, out, ldo, part);                       \
    break;
  switch (rows_per_wg) {
    MSR3D_ADS(1) MSR3D_ADS(2) MSR3D_ADS(3) MSR3D_ADS(4) MSR3D_ADS(5) MSR3D_ADS(6) MSR3D_ADS(7)
    default:
      attn_decode_shared_kernel<D, 8, Planes><<<grid, 256, 0, st>>>(G, T, Ttail, H, q, ldq, prompt, pkeep, tails, tail_len,
                                                                    len_add, sl2, out, ldo, part);
  }
#undef MSR3D_ADS
}

// msr3d_attn_decode and msr3d_attn_decode_e4m3 behind their own checks of the planes: the same splits, workspace and
// merge launch
template <class Planes>
int attn_decode_launch(int N, int Tmax, int H, int D, const void *q, int ldq, Planes cache, const int *len,
                              int len_add, const unsigned char *key_keep, float scale, void *out, int ldo,
                              float *workspace, long long workspace_floats, msr3d_stream_t stream) {
  if (N > 65535 || !q || !len || !out || !al16(q)) return MSR3D_EINVAL;
  int S = workspace ? msr3d_attn_decode_splits(N, H) : 1;
  if (S > 1 && workspace_floats < (long long)N * H * S * (D + 2)) return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float sl2 = scale * 1.4426950408889634f;
  const dim3 grid(H, N, S);
  float *part = S > 1 ? workspace : nullptr;
  if (D == 128)
    attn_decode_kernel<128, Planes><<<grid, 256, 0, st>>>(Tmax, H, (const u16 *)q, ldq, cache, len, len_add, key_keep, sl2,
                                                          (u16 *)out, ldo, part);
  else
    attn_decode_kernel<64, Planes><<<grid, 256, 0, st>>>(Tmax, H, (const u16 *)q, ldq, cache, len, len_add, key_keep, sl2,
                                                         (u16 *)out, ldo, part);
  if (S > 1) {
    if (D == 128) attn_merge_kernel<128><<<dim3(H, N), 128, 0, st>>>(H, S, part, (u16 *)out, ldo);
    else attn_merge_kernel<64><<<dim3(H, N), 64, 0, st>>>(H, S, part, (u16 *)out, ldo);
  }
  return (int)hipGetLastError();
}

// msr3d_attn_decode_shared and msr3d_attn_decode_shared_e4m3 behind their own checks of the planes
bool attn_decode_shared_args(int B, int G, int T, int Ttail, int H, int D, int ldq, int ldo, int splits) {
  return !(B < 0 || G <= 0 || T <= 0 || Ttail < 0 || H <= 0 || (D != 64 && D != 128) || ldq < H * D || (ldq % 8) ||
           ldo < H * D || splits < 0 || splits > MSR3D_ATTN_DECODE_MAX_SPLITS);
}

template <class Planes>
int attn_decode_shared_launch_checked(int B, int G, int T, int Ttail, int H, int D, const void *q, int ldq,
                                             Planes prompt, const unsigned char *prompt_keep, Planes tails,
                                             const int *tail_len, int len_add, float scale, void *out, int ldo,
                                             float *workspace, long long workspace_floats, int splits,
                                             msr3d_stream_t stream) {
  const long long N = (long long)B * G, gy = (long long)B * ((G + 7) / 8);
  if (N > 65535 || gy > 65535 || !q || !tail_len || !out || !al16(q)) return MSR3D_EINVAL;
  // splits 0: what msr3d_attn_decode takes for these N rows (one split without a workspace)
  const int S = splits ? splits : (workspace ? msr3d_attn_decode_splits((int)N, H) : 1);
  if (S > 1 && (!workspace || workspace_floats < N * H * S * (D + 2))) return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float sl2 = scale * 1.4426950408889634f;
  const dim3 grid(H, (unsigned)gy, S);
  float *part = S > 1 ? workspace : nullptr;
  const int rows_per_wg = G < 8 ? G : 8;
  if (D == 128)
    attn_decode_shared_launch<128>(rows_per_wg, grid, st, G, T, Ttail, H, (const u16 *)q, ldq, prompt, prompt_keep, tails,
                                   tail_len, len_add, sl2, (u16 *)out, ldo, part);
  else
    attn_decode_shared_launch<64>(rows_per_wg, grid, st, G, T, Ttail, H, (const u16 *)q, ldq, prompt, prompt_keep, tails,
                                  tail_len, len_add, sl2, (u16 *)out, ldo, part);
  if (S > 1) {
    if (D == 128) attn_merge_kernel<128><<<dim3(H, (unsigned)N), 128, 0, st>>>(H, S, part, (u16 *)out, ldo);
    else attn_merge_kernel<64><<<dim3(H, (unsigned)N), 64, 0, st>>>(H, S, part, (u16 *)out, ldo);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Both skinny entries: `max_m` is the entry's row limit.  M <= 32 takes the one- and two-tile kernels under the tile rule
// they always had (the bits of msr3d_bf16_skinny_lowrank do not depend on which entry was called); 33 .. 64 rows take the
// three- and four-tile instantiations under the wide rule below.
// `fz` (msr3d_bf16_skinny_fused, its own checks made, at least one of nw, res, H set): the fused instantiations, under the
// same tile rule (the bits do not depend on it).
static int skinny_launch(int max_m, int M, int K, int R, const void *P, int ldp, const void *P2, int ldp2, int njobs,
                         const msr3d_skinny_job_t *jobs, int swiglu, msr3d_stream_t stream,
                         const SkinnyFused *fz = nullptr) {
  if (M < 0 || M > max_m || K <= 0 || (K % 128) || R < 0 || (R % 32) || njobs < 1 || njobs > 3 || !jobs)
    return MSR3D_EINVAL;
  if (!P || ldp < K || (ldp % 8) || !al16(P)) return MSR3D_EINVAL;
  if (R > 0 && (!P2 || ldp2 < R || (ldp2 % 8) || !al16(P2))) return MSR3D_EINVAL;
  if (swiglu && (njobs != 2 || jobs[0].N != jobs[1].N || !jobs[0].C)) return MSR3D_EINVAL;
  const bool rope = fz && fz->H > 0;
  long long rows = 0;
  bool pairs = true;                                  // every job's N a multiple of 32: two tiles a workgroup possible
  for (int j = 0; j < njobs; ++j) {
    const msr3d_skinny_job_t &jb = jobs[j];
    if (jb.N <= 0 || (jb.N % 16) || !jb.W || jb.ldw < K || (jb.ldw % 8) || !al16(jb.W)) return MSR3D_EINVAL;
    if (R > 0 && jb.B2 && (jb.ldb2 < R || (jb.ldb2 % 8) || !al16(jb.B2))) return MSR3D_EINVAL;
    // (the rotation writes k and v into the cache planes alone)
    if (!(swiglu && j == 1) && !(rope && j > 0) && (!jb.C || jb.ldc < jb.N)) return MSR3D_EINVAL;
    rows += jb.N;
    if (jb.N % 32) pairs = false;
  }
  if (M == 0) return 0;
  const int mt = (M + 15) / 16;
  int tn;
  if (mt <= 2) {
    // two 16-row tiles of W per workgroup where that still leaves every CU several workgroups (the activations are read
    // once per workgroup); gate | up with the SwiGLU epilogue is always the pair
    tn = (swiglu || (rows >= 16384 && pairs)) ? 2 : 1;
  } else {
    // 33 .. 64 rows: a workgroup reads M K activations out of L2 for 16 tn rows of W out of HBM, M / (16 tn) bytes for
    // one, so the pair halves the L2 traffic -- but only pays where it still gives every CU a workgroup.  Measured at
    // 64 rows: the head 95 us against 147 and q | k | v (384 workgroups as pairs) 51 against 61 with the
    // pair; o and down (N = 4096: 128 workgroups as pairs) 28 against 23 and 69 against 55, so those keep one tile.
    tn = (swiglu || (pairs && rows / 32 >= kSkinnyWideMinWg)) ? 2 : 1;
  }
  SkinnyJobs sj{};
  sj.njobs = njobs;
  long long grid = 0;
  for (int j = 0; j < njobs; ++j) {
    sj.W[j] = (const u16 *)jobs[j].W; sj.B2[j] = R > 0 ? (const u16 *)jobs[j].B2 : nullptr; sj.C[j] = (u16 *)jobs[j].C;
    sj.N[j] = jobs[j].N; sj.ldw[j] = jobs[j].ldw; sj.ldb2[j] = jobs[j].ldb2; sj.ldc[j] = jobs[j].ldc;
    sj.tiles[j] = swiglu ? jobs[j].N / 16 : jobs[j].N / (16 * tn);
    grid += sj.tiles[j];
  }
  if (swiglu) grid = sj.tiles[0];
  hipStream_t st = (hipStream_t)stream;
  const u16 *p = (const u16 *)P, *p2 = (const u16 *)P2;
// (the template arguments behind MT: TN, SWIGLU and, for the fused kernel, NORM, RES, ROPE)
#define MSR3D_SK(MT, ...) skinny_kernel<MT, __VA_ARGS__><<<(unsigned)grid, 256, 0, st>>>(M, K, R, p, ldp, p2, ldp2, sj)
#define MSR3D_SKF(MT, ...) skinny_fused_kernel<MT, __VA_ARGS__><<<(unsigned)grid, 256, 0, st>>>(M, K, p, ldp, sj, *fz)
#define MSR3D_SK_MT(LAUNCH, ...)                                                                                       \
  switch (mt) {                                                                                                        \
    case 1: LAUNCH(1, __VA_ARGS__); break;                                                                             \
    case 2: LAUNCH(2, __VA_ARGS__); break;                                                                             \
    case 3: LAUNCH(3, __VA_ARGS__); break;                                                                             \
    default: LAUNCH(4, __VA_ARGS__); break;                                                                            \
  }
  if (fz) {
    const bool norm = fz->nw != nullptr, res = fz->res != nullptr;
    if (swiglu) { MSR3D_SK_MT(MSR3D_SKF, 2, true, true, false, false) }
    else if (rope && tn == 2 && norm) { MSR3D_SK_MT(MSR3D_SKF, 2, false, true, false, true) }
    else if (rope && tn == 2) { MSR3D_SK_MT(MSR3D_SKF, 2, false, false, false, true) }
    else if (rope && norm) { MSR3D_SK_MT(MSR3D_SKF, 1, false, true, false, true) }
    else if (rope) { MSR3D_SK_MT(MSR3D_SKF, 1, false, false, false, true) }
    else if (tn == 2 && norm && res) { MSR3D_SK_MT(MSR3D_SKF, 2, false, true, true, false) }
    else if (tn == 2 && norm) { MSR3D_SK_MT(MSR3D_SKF, 2, false, true, false, false) }
    else if (tn == 2) { MSR3D_SK_MT(MSR3D_SKF, 2, false, false, true, false) }
    else if (norm && res) { MSR3D_SK_MT(MSR3D_SKF, 1, false, true, true, false) }
    else if (norm) { MSR3D_SK_MT(MSR3D_SKF, 1, false, true, false, false) }
    else { MSR3D_SK_MT(MSR3D_SKF, 1, false, false, true, false) }
  }
  else if (swiglu) { MSR3D_SK_MT(MSR3D_SK, 2, true) }
  else if (tn == 2) { MSR3D_SK_MT(MSR3D_SK, 2, false) }
  else { MSR3D_SK_MT(MSR3D_SK, 1, false) }
#undef MSR3D_SK_MT
#undef MSR3D_SKF
#undef MSR3D_SK
  return (int)hipGetLastError();
}

int msr3d_bf16_skinny_fused(int M, int K, int R, const void *P, int ldp, const void *P2, int ldp2, int njobs,
                            const msr3d_skinny_job_t *jobs, int swiglu, const void *norm_w, float eps, const void *res,
                            int ldres, int H, int D, const int *pos, const int *len, const float *cos_td,
                            const float *sin_td, int table_rows, void *k_plane, void *v_plane, int Tmax,
                            msr3d_stream_t stream) {
  if (R != 0 || H < 0 || njobs < 1 || njobs > 3 || !jobs) return MSR3D_EINVAL;
  SkinnyFused fz{};
  if (norm_w) {
    if ((K % 512) || K > 8192 || K <= 0 || !al16(norm_w)) return MSR3D_EINVAL;     // the norm's own domain
    fz.nw = (const u16 *)norm_w; fz.eps = eps; fz.inv_k = 1.0f / (float)K;
  }
  if (res) {
    // one job, and a fresh output: the operand is read element by element while other workgroups store
    if (njobs != 1 || swiglu || H > 0 || ldres < jobs[0].N || !al16(res) || res == jobs[0].C) return MSR3D_EINVAL;
    fz.res = (const u16 *)res; fz.ldres = ldres;
  }
  if (H > 0) {
    if (D <= 0 || (D % 32) || njobs != 3 || swiglu || Tmax <= 0 || table_rows <= 0) return MSR3D_EINVAL;
    for (int j = 0; j < 3; ++j)
      if (jobs[j].N != (long long)H * D) return MSR3D_EINVAL;
    if (!pos || !len || !cos_td || !sin_td || !k_plane || !v_plane) return MSR3D_EINVAL;
    if (!al16(cos_td) || !al16(sin_td) || !al16(k_plane) || !al16(v_plane)) return MSR3D_EINVAL;
    fz.H = H; fz.D = D; fz.table_rows = table_rows; fz.Tmax = Tmax; fz.pos = pos; fz.len = len; fz.cs = cos_td;
    fz.sn = sin_td; fz.kc = (u16 *)k_plane; fz.vc = (u16 *)v_plane;
  }
  // SwiGLU without the prologue, or nothing set: the plain entry's launch
  const bool fused = H > 0 || res || norm_w;
  return skinny_launch(MSR3D_SKINNY_WIDE_MAX_M, M, K, 0, P, ldp, nullptr, 0, njobs, jobs, swiglu, stream,
                       fused ? &fz : nullptr);
}

int msr3d_bf16_skinny_lowrank(int M, int K, int R, const void *P, int ldp, const void *P2, int ldp2, int njobs,
                              const msr3d_skinny_job_t *jobs, int swiglu, msr3d_stream_t stream) {
  return skinny_launch(MSR3D_SKINNY_MAX_M, M, K, R, P, ldp, P2, ldp2, njobs, jobs, swiglu, stream);
}

int msr3d_bf16_skinny_lowrank_wide(int M, int K, int R, const void *P, int ldp, const void *P2, int ldp2, int njobs,
                                   const msr3d_skinny_job_t *jobs, int swiglu, msr3d_stream_t stream) {
  return skinny_launch(MSR3D_SKINNY_WIDE_MAX_M, M, K, R, P, ldp, P2, ldp2, njobs, jobs, swiglu, stream);
}

int msr3d_rope_positions(int B, int T, int H, int D, void *x0, void *x1, const int *pos, const float *cos_td,
                         const float *sin_td, int table_rows, msr3d_stream_t stream) {
  if (B < 0 || T <= 0 || H <= 0 || D <= 0 || (D % 16) || table_rows <= 0) return MSR3D_EINVAL;
  if (B == 0) return 0;
  if (!x0 || !pos || !cos_td || !sin_td || !al16(x0) || !al16(x1) || !al16(cos_td) || !al16(sin_td)) return MSR3D_EINVAL;
  const long long n = (long long)B * T * H * (D / 16);
  rope_positions_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n, H, D, (u16 *)x0, (u16 *)x1, pos,
                                                                                    table_rows, cos_td, sin_td);
  return (int)hipGetLastError();
}

int msr3d_rope_kv_append(int N, int H, int D, int Tmax, void *q, const void *k, const void *v, int ld, const int *pos,
                         const int *len, const float *cos_td, const float *sin_td, int table_rows, void *k_cache,
                         void *v_cache, msr3d_stream_t stream) {
  if (N < 0 || H <= 0 || D <= 0 || (D % 16) || Tmax <= 0 || table_rows <= 0 || ld < H * D || (ld % 8)) return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!q || !k || !v || !pos || !len || !cos_td || !sin_td || !k_cache || !v_cache) return MSR3D_EINVAL;
  if (!al16(q) || !al16(k) || !al16(v) || !al16(cos_td) || !al16(sin_td) || !al16(k_cache) || !al16(v_cache))
    return MSR3D_EINVAL;
  const long long n = (long long)N * H * (D / 16);
  if (n > 0x7fffffffLL) return MSR3D_EINVAL;
  rope_kv_append_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      (int)n, H, D, Tmax, (u16 *)q, (const u16 *)k, (const u16 *)v, ld, pos, len, table_rows, cos_td, sin_td, (u16 *)k_cache,
      (u16 *)v_cache);
  return (int)hipGetLastError();
}

int msr3d_kv_quantize_e4m3(int rows, int H, int D, const void *x, int ldx, void *codes, void *exps, int lde,
                           msr3d_stream_t stream) {
  if (rows < 0 || H <= 0 || (D != 64 && D != 128) || ldx < H * D || (ldx % 8) || lde < H) return MSR3D_EINVAL;
  if (rows == 0) return 0;
  if (!x || !codes || !exps || !al16(x) || !al16(codes)) return MSR3D_EINVAL;
  const long long n = (long long)rows * H * (D / 8);
  if ((n + 255) / 256 > 0x7fffffffLL) return MSR3D_EINVAL;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (D == 128)
    kv_quantize_kernel<128><<<grid, 256, 0, st>>>(n, H, (const u16 *)x, ldx, (unsigned char *)codes, (unsigned char *)exps, lde);
  else
    kv_quantize_kernel<64><<<grid, 256, 0, st>>>(n, H, (const u16 *)x, ldx, (unsigned char *)codes, (unsigned char *)exps, lde);
  return (int)hipGetLastError();
}

int msr3d_rope_kv_append_e4m3(int N, int H, int D, int Tmax, void *q, const void *k, const void *v, int ld, const int *pos,
                              const int *len, const float *cos_td, const float *sin_td, int table_rows, void *k_codes,
                              void *v_codes, void *k_exps, void *v_exps, int lde, msr3d_stream_t stream) {
  if (N < 0 || H <= 0 || (D != 64 && D != 128) || Tmax <= 0 || table_rows <= 0 || ld < H * D || (ld % 8) || lde < H)
    return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!q || !k || !v || !pos || !len || !cos_td || !sin_td || !k_codes || !v_codes || !k_exps || !v_exps) return MSR3D_EINVAL;
  if (!al16(q) || !al16(k) || !al16(v) || !al16(cos_td) || !al16(sin_td) || !al16(k_codes) || !al16(v_codes))
    return MSR3D_EINVAL;
  const long long n = (long long)N * H * (D / 16);
  if (n > 0x7fffffffLL) return MSR3D_EINVAL;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  using B8 = unsigned char *;
  if (D == 128)
    rope_kv_append_e4m3_kernel<128><<<grid, 256, 0, st>>>((int)n, H, Tmax, (u16 *)q, (const u16 *)k, (const u16 *)v, ld, pos,
                                                          len, table_rows, cos_td, sin_td, (B8)k_codes, (B8)v_codes,
                                                          (B8)k_exps, (B8)v_exps, lde);
  else
    rope_kv_append_e4m3_kernel<64><<<grid, 256, 0, st>>>((int)n, H, Tmax, (u16 *)q, (const u16 *)k, (const u16 *)v, ld, pos,
                                                         len, table_rows, cos_td, sin_td, (B8)k_codes, (B8)v_codes,
                                                         (B8)k_exps, (B8)v_exps, lde);
  return (int)hipGetLastError();
}

int msr3d_attn_decode_splits(int N, int H) {
  if (N <= 0 || H <= 0) return 1;
  const long long wg = (long long)N * H;
  if (wg >= 256) return 1;
  const int s = (int)((512 + wg - 1) / wg);
  return s > MSR3D_ATTN_DECODE_MAX_SPLITS ? MSR3D_ATTN_DECODE_MAX_SPLITS : s;
}

int msr3d_attn_decode(int N, int Tmax, int H, int D, const void *q, int ldq, const void *k_cache, const void *v_cache,
                      const int *len, int len_add, const unsigned char *key_keep, float scale, void *out, int ldo,
                      float *workspace, long long workspace_floats, msr3d_stream_t stream) {
  if (N < 0 || Tmax <= 0 || H <= 0 || (D != 64 && D != 128) || ldq < H * D || (ldq % 8) || ldo < H * D) return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!k_cache || !v_cache || !al16(k_cache) || !al16(v_cache)) return MSR3D_EINVAL;
  return attn_decode_launch(N, Tmax, H, D, q, ldq, KvPlanesBf16{(const u16 *)k_cache, (const u16 *)v_cache}, len, len_add,
                            key_keep, scale, out, ldo, workspace, workspace_floats, stream);
}

int msr3d_attn_decode_e4m3(int N, int Tmax, int H, int D, const void *q, int ldq, const void *k_codes, const void *v_codes,
                           const void *k_exps, const void *v_exps, int lde, const int *len, int len_add,
                           const unsigned char *key_keep, float scale, void *out, int ldo, float *workspace,
                           long long workspace_floats, msr3d_stream_t stream) {
  if (N < 0 || Tmax <= 0 || H <= 0 || (D != 64 && D != 128) || ldq < H * D || (ldq % 8) || ldo < H * D || lde < H)
    return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!k_codes || !v_codes || !k_exps || !v_exps || !al16(k_codes) || !al16(v_codes)) return MSR3D_EINVAL;
  const KvPlanesE4m3 cache{(const unsigned char *)k_codes, (const unsigned char *)v_codes, (const unsigned char *)k_exps,
                           (const unsigned char *)v_exps, lde};
  return attn_decode_launch(N, Tmax, H, D, q, ldq, cache, len, len_add, key_keep, scale, out, ldo, workspace,
                            workspace_floats, stream);
}

int msr3d_attn_decode_shared(int B, int G, int T, int Ttail, int H, int D, const void *q, int ldq, const void *k_prompt,
                             const void *v_prompt, const unsigned char *prompt_keep, const void *k_tail, const void *v_tail,
                             const int *tail_len, int len_add, float scale, void *out, int ldo, float *workspace,
                             long long workspace_floats, int splits, msr3d_stream_t stream) {
  if (!attn_decode_shared_args(B, G, T, Ttail, H, D, ldq, ldo, splits)) return MSR3D_EINVAL;
  if (B == 0) return 0;
  if (!k_prompt || !v_prompt || !al16(k_prompt) || !al16(v_prompt)) return MSR3D_EINVAL;
  if (Ttail > 0 && (!k_tail || !v_tail || !al16(k_tail) || !al16(v_tail))) return MSR3D_EINVAL;
  return attn_decode_shared_launch_checked(B, G, T, Ttail, H, D, q, ldq,
                                           KvPlanesBf16{(const u16 *)k_prompt, (const u16 *)v_prompt}, prompt_keep,
                                           KvPlanesBf16{(const u16 *)k_tail, (const u16 *)v_tail}, tail_len, len_add, scale,
                                           out, ldo, workspace, workspace_floats, splits, stream);
}

int msr3d_attn_decode_shared_e4m3(int B, int G, int T, int Ttail, int H, int D, const void *q, int ldq,
                                  const void *k_prompt, const void *v_prompt, const void *ke_prompt, const void *ve_prompt,
                                  const unsigned char *prompt_keep, const void *k_tail, const void *v_tail,
                                  const void *ke_tail, const void *ve_tail, int lde, const int *tail_len, int len_add,
                                  float scale, void *out, int ldo, float *workspace, long long workspace_floats, int splits,
                                  msr3d_stream_t stream) {
  if (!attn_decode_shared_args(B, G, T, Ttail, H, D, ldq, ldo, splits) || lde < H) return MSR3D_EINVAL;
  if (B == 0) return 0;
  if (!k_prompt || !v_prompt || !ke_prompt || !ve_prompt || !al16(k_prompt) || !al16(v_prompt)) return MSR3D_EINVAL;
  if (Ttail > 0 && (!k_tail || !v_tail || !ke_tail || !ve_tail || !al16(k_tail) || !al16(v_tail))) return MSR3D_EINVAL;
  using B8 = const unsigned char *;
  return attn_decode_shared_launch_checked(B, G, T, Ttail, H, D, q, ldq,
                                           KvPlanesE4m3{(B8)k_prompt, (B8)v_prompt, (B8)ke_prompt, (B8)ve_prompt, lde},
                                           prompt_keep, KvPlanesE4m3{(B8)k_tail, (B8)v_tail, (B8)ke_tail, (B8)ve_tail, lde},
                                           tail_len, len_add, scale, out, ldo, workspace, workspace_floats, splits, stream);
}

int msr3d_kv_reorder(int planes, int N, int Tmax, int row_elems, const void *src, void *dst, const int *beam_idx,
                     const int *len, msr3d_stream_t stream) {
  if (planes < 0 || N < 0 || Tmax <= 0 || row_elems <= 0 || (row_elems % 8)) return MSR3D_EINVAL;
  if (planes == 0 || N == 0) return 0;
  if (planes > 65535 || N > 65535 || !src || !dst || src == dst || !beam_idx || !len || !al16(src) || !al16(dst))
    return MSR3D_EINVAL;
  const long long per_row = (long long)Tmax * (row_elems / 8);       // 16-byte pieces of a full row; a block takes ~8 per thread
  long long gx = (per_row + 2047) / 2048;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  kv_reorder_kernel<<<dim3((unsigned)gx, N, planes), 256, 0, (hipStream_t)stream>>>(N, Tmax, row_elems / 8, (const uint4 *)src,
                                                                               (uint4 *)dst, beam_idx, len);
  return (int)hipGetLastError();
}

int msr3d_decode_select(int N, int V, const void *logits, int ldl, const long long *prev_tokens, int ld_prev,
                        const int *n_prev, float repetition_penalty, int min_length, int eos_id, const float *beam_score,
                        int order, int k, float *out_val, int *out_tok, msr3d_stream_t stream) {
  if (N < 0 || V <= 0 || V > MSR3D_DECODE_SELECT_MAX_V || ldl < V || k <= 0 || k > V || k > MSR3D_DECODE_SELECT_MAX_K ||
      (order != 0 && order != 1) || !(repetition_penalty > 0.f) || ld_prev < 0)
    return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!logits || !out_val || !out_tok || (n_prev && !prev_tokens)) return MSR3D_EINVAL;
  if ((size_t)V * sizeof(float) > 48 * 1024) {
    // more dynamic LDS than the default limit: 160 KB a workgroup on this part, 160 000 bytes at the largest V
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(decode_select_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, MSR3D_DECODE_SELECT_MAX_V * 4);
    if (e != hipSuccess) return (int)e;
  }
  decode_select_kernel<<<N, 256, (size_t)V * sizeof(float), (hipStream_t)stream>>>(
      V, (const u16 *)logits, ldl, prev_tokens, ld_prev, n_prev, ld_prev, repetition_penalty, min_length, eos_id, beam_score,
      order, k, out_val, out_tok);
  return (int)hipGetLastError();
}

}  // extern "C"
