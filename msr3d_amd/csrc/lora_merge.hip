// lora_merge.hip -- the LoRA pairs of a whole stack folded into copies of their frozen weights, in ONE launch
// (peft's merge_and_unload for the LoraConfig targets of the reference's model/msr3d/msr3d.py:103-112):
//
//     out[n][k] = bf16_rne( W[n][k] + scale * sum_r B[n][r] A[r][k] )      W (N, K) bf16, A (r, K), B (N, r) fp32 masters
//
// Evaluation runs on frozen weights: with the merged planes a decode step's products are plain weight streams (the
// R = 0 forms of msr3d_bf16_skinny_lowrank / msr3d_bf16_gemm_lowrank) and the r-row products leave the step.
//
// The kernel is a stream -- 2 bytes read and 2 written per element; the A slice and the B rows come out of L2 -- so it is
// laid out around 16-byte accesses of W and out, and the rank-r term is put where it costs the stream least:
// v_mfma_f32_16x16x4_f32, fp32 in and out (a k-ordered fmaf chain, no reduced precision).  A wave owns a tile of
// kTileRows x 128 columns and keeps its A slice (r x 128 fp32) in registers as MFMA operands for the whole tile:
//
//   * the 16-row side of the instruction is sixteen COLUMNS k, the 16-column side sixteen weight ROWS n, so a lane's four
//     accumulators are four consecutive k of one row; two instructions whose column maps interleave in fours
//     (k = 32 p + 8 (m / 4) + 4 t + m % 4 for row m of instruction t of pair p) leave lane (i, g) with the EIGHT consecutive
//     columns 32 p + 8 g .. + 7 of row i: exactly the 16 bytes it loaded from W and the 16 bytes it stores;
//   * the reduction index is free (any order): k-slot g of step s takes r = (R / 4) g + s, so a lane's share of a B row is
//     R / 4 consecutive floats -- one or two 16-byte loads;
//   * 8 R / 4 instructions of 32 cycles per 16 x 128 elements: 2 (r = 16) or 1 (r = 32) elements a clock and SIMD, at the
//     packed-FMA peak of the VALU, which stays free for the unpack / fma / round / pack of the epilogue (the plain-FMA
//     form was r + 6 VALU operations an element in ONE pipe).
//
// Tiles of all jobs are numbered through (column block fastest, so the waves of a workgroup read neighbouring 256-byte
// pieces of the same rows) and dealt round-robin over every wave of the grid: one launch covers 4096 x 4096 and
// 11008 x 4096 jobs evenly.  W is read non-temporally (13 GB at 7B: nothing of it is read again soon); `out` is stored
// plainly: a wave's store covers 64 bytes of a row, two of them fill a 128-byte line, and with non-temporal stores the
// launch over a 4-layer stack took 883 us against 782 (a device copy of the same bytes: 649).
// No atomics, every element has one owner, the order of the sum is fixed: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/msr3d_hip.h"

namespace {

using u16 = unsigned short;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// the job table hands over generic pointers; everything they point to is global memory (global_load, not flat_load)
#define MSR3D_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ const MSR3D_GLOBAL T *as_global(const void *p) {
  return (const MSR3D_GLOBAL T *)(uintptr_t)p;
}

constexpr int kTileCols = 128;     // four pairs of 16-column instructions: 8 columns a lane and pair
constexpr int kTileRows = 128;     // rows a wave walks with one A slice in registers (8 steps of 16)

__device__ __forceinline__ unsigned f2bf(float f) {        // round to nearest even
  unsigned u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

template <int R>
__device__ __forceinline__ void merge_tile(const msr3d_lora_merge_job_t &jb, int rb, int cb, int lane) {
  constexpr int S = R / 4;                        // instructions per 16 x 16 tile; k-slot g of step s is r = S g + s
  const int i = lane & 15, g = lane >> 4;
  const int K = jb.K, N = jb.N;
  const MSR3D_GLOBAL u16 *W = as_global<u16>(jb.W);
  const MSR3D_GLOBAL float *A = as_global<float>(jb.A), *B = as_global<float>(jb.B);
  MSR3D_GLOBAL u16 *out = (MSR3D_GLOBAL u16 *)(uintptr_t)jb.out;
  const int k0 = cb * kTileCols;
  float a[4][2][S];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int k = k0 + 32 * p + 8 * (i >> 2) + 4 * t + (i & 3);
#pragma unroll
      for (int s = 0; s < S; ++s) a[p][t][s] = k < K ? A[(size_t)(S * g + s) * K + k] : 0.f;
    }
  const int kl = k0 + 8 * g;                      // + 32 p: this lane's eight columns of pair p (K % 8 == 0: all or none)
  const int n_end = min(N, (rb + 1) * kTileRows);
  const float scale = jb.scale;

  struct Step { u32x4 w[4]; float b[S]; };
  auto fetch = [&](Step &st, int n0) {
    const int n = n0 + i;
    const MSR3D_GLOBAL f32x4 *bp = (const MSR3D_GLOBAL f32x4 *)(B + (size_t)min(n, N - 1) * R + S * g);
#pragma unroll
    for (int q = 0; q < S / 4; ++q) {
      const f32x4 v = bp[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) st.b[4 * q + e] = v[e];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      st.w[p] = u32x4{0u, 0u, 0u, 0u};
      if (n < N && kl + 32 * p < K)
        st.w[p] = __builtin_nontemporal_load((const MSR3D_GLOBAL u32x4 *)(W + (size_t)n * K + kl + 32 * p));
    }
  };
  auto finish = [&](const Step &st, int n0) {
    const int n = n0 + i;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      f32x4 lo = f32x4{0.f, 0.f, 0.f, 0.f}, hi = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < S; ++s) {
        lo = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][0][s], st.b[s], lo, 0, 0, 0);
        hi = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][1][s], st.b[s], hi, 0, 0, 0);
      }
      // columns kl + 32 p + 0..3 from `lo`, + 4..7 from `hi`; one rounding for scale * sum + W, one to bf16
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const unsigned w0 = st.w[p][e], w1 = st.w[p][2 + e];
        o[e] = f2bf(fmaf(scale, lo[2 * e], __uint_as_float(w0 << 16))) |
               (f2bf(fmaf(scale, lo[2 * e + 1], __uint_as_float(w0 & 0xffff0000u))) << 16);
        o[2 + e] = f2bf(fmaf(scale, hi[2 * e], __uint_as_float(w1 << 16))) |
                   (f2bf(fmaf(scale, hi[2 * e + 1], __uint_as_float(w1 & 0xffff0000u))) << 16);
      }
      if (n < N && kl + 32 * p < K) *(MSR3D_GLOBAL u32x4 *)(out + (size_t)n * jb.ldo + kl + 32 * p) = o;
    }
  };

  // the next 16 rows' loads go out before this step's instructions
  Step cur, nxt;
  int n0 = rb * kTileRows;
  fetch(cur, n0);
  for (; n0 < n_end; n0 += 16) {
    const bool more = n0 + 16 < n_end;            // (wave-uniform)
    if (more) fetch(nxt, n0 + 16);
    finish(cur, n0);
    if (more) cur = nxt;
  }
}

// WIDE = false: every job of the table has r = 16 (the host has read it), and the kernel carries half the A slice
template <bool WIDE>
__global__ __launch_bounds__(256) void lora_merge_kernel(int njobs, const msr3d_lora_merge_job_t *__restrict__ jobs) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long stride = (long long)gridDim.x * 4;
  long long tile = (long long)blockIdx.x * 4 + wave;     // over all jobs; `base`: the first tile of job j
  long long base = 0;
  for (int j = 0; j < njobs; ++j) {
    const msr3d_lora_merge_job_t jb = jobs[j];
    const int ncb = (jb.K + kTileCols - 1) / kTileCols, nrb = (jb.N + kTileRows - 1) / kTileRows;
    const long long end = base + (long long)ncb * nrb;
    for (; tile < end; tile += stride) {
      const int t = (int)(tile - base);
      if (!WIDE || jb.r == 16) merge_tile<16>(jb, t / ncb, t % ncb, lane);
      else merge_tile<32>(jb, t / ncb, t % ncb, lane);
    }
    base = end;
  }
}

inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int msr3d_lora_merge(int njobs, const msr3d_lora_merge_job_t *jobs_device, msr3d_stream_t stream) {
  if (njobs < 0) return MSR3D_EINVAL;
  if (njobs == 0) return 0;
  if (!jobs_device) return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // The table is read back once to be checked before anything is written through its pointers, and to size the grid:
  // a merge runs once per weight version, not per step, so the one small synchronous copy is not on a hot path.
  std::vector<msr3d_lora_merge_job_t> h((size_t)njobs);
  hipError_t e = hipMemcpyAsync(h.data(), jobs_device, sizeof(msr3d_lora_merge_job_t) * (size_t)njobs, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  long long tiles = 0;
  bool wide = false;
  for (const msr3d_lora_merge_job_t &j : h) {
    if ((j.r != 16 && j.r != 32) || j.N <= 0 || j.K <= 0 || (j.K % 8) || j.ldo < j.K || (j.ldo % 8)) return MSR3D_EINVAL;
    if (!j.W || !j.A || !j.B || !j.out || !al16(j.W) || !al16(j.A) || !al16(j.B) || !al16(j.out)) return MSR3D_EINVAL;
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(j.W), w1 = w0 + 2 * (uintptr_t)j.N * (uintptr_t)j.K;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(j.out);
    const uintptr_t o1 = o0 + 2 * ((uintptr_t)(j.N - 1) * (uintptr_t)j.ldo + (uintptr_t)j.K);
    if (o0 < w1 && w0 < o1) return MSR3D_EINVAL;           // out must not alias W (no merging in place)
    wide = wide || j.r == 32;
    tiles += (long long)((j.K + kTileCols - 1) / kTileCols) * ((j.N + kTileRows - 1) / kTileRows);
  }
  // four wave tiles a workgroup; at most 1024 workgroups (four a CU: sixteen waves, as many as the registers allow)
  const long long wgs = (tiles + 3) / 4;
  const unsigned grid = (unsigned)(wgs < 1024 ? wgs : 1024);
  if (wide) lora_merge_kernel<true><<<grid, 256, 0, st>>>(njobs, jobs_device);
  else lora_merge_kernel<false><<<grid, 256, 0, st>>>(njobs, jobs_device);
  return (int)hipGetLastError();
}
