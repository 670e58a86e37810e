// image_tokens.hip -- the 2D image branch of MSR3D.build_embeds (the reference's model/msr3d/msr3d.py:98-100
// `llm_proj_img`, :233-252):
//     img_embeds = llm_proj_img(image_encoder(pixel_values[img_mask]))            (fp32, outside autocast)
//     inputs_embeds[where(input_ids == img_sp_token)] = img_embeds.to(inputs_embeds.dtype)
// The boolean-mask compaction and the torch.where are a host sync each.  Here a one-block kernel builds both maps on
// the device (k-th placeholder <- k-th real image, both in row-major order), a second kernel gathers the real images'
// features through the map, multiplies them with the weight on f32-input MFMA, adds the bias, casts and scatters; the
// backward walks the same map.  Launch geometry is sized by the capacity B*N; the live count n is read from device memory.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/msr3d_hip.h"

namespace {

using f32x4v = __attribute__((ext_vector_type(4))) float;

// One 256-wide step of a block-wide ordered compaction: returns the rank (among all hits so far, `running` included) of
// this thread's hit; advances `running` by the step's hits.  Every thread of the block calls it.
__device__ __forceinline__ int compact_step(bool hit, int *wave_cnt, int *running) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long m = __ballot(hit);
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = *running;
  for (int w = 0; w < wave; ++w) before += wave_cnt[w];
  const int k = before + __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (tid == 0) *running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  __syncthreads();
  return k;
}

// dest[k] = flat (b*T + t) position of the k-th placeholder, src[k] = flat slot of the k-th source (mode 0: the k-th slot
// whose mask byte is set; mode 1: slot k), k < cap = B*N; counts[0] = placeholders found, counts[1] = sources.
__global__ __launch_bounds__(256) void image_map_kernel(int B, int T, int cap, int mode,
                                                        const long long *__restrict__ ids, long long token,
                                                        const unsigned char *__restrict__ masks,
                                                        int *__restrict__ dest, int *__restrict__ src,
                                                        int *__restrict__ counts) {
  __shared__ int wave_cnt[4];
  __shared__ int running;
  const int tid = threadIdx.x;
  if (tid == 0) running = 0;
  __syncthreads();
  for (int b = 0; b < B; ++b) {
    for (int t0 = 0; t0 < T; t0 += 256) {
      const int t = t0 + tid;
      const bool hit = t < T && ids[(size_t)b * T + t] == token;
      const int k = compact_step(hit, wave_cnt, &running);
      if (hit && k < cap) dest[k] = b * T + t;
    }
  }
  if (tid == 0) { counts[0] = running; running = 0; }
  __syncthreads();
  if (mode == 1) {
    for (int s = tid; s < cap; s += 256) src[s] = s;
    if (tid == 0) counts[1] = cap;
    return;
  }
  for (int s0 = 0; s0 < cap; s0 += 256) {
    const int s = s0 + tid;
    const bool hit = s < cap && masks[s] != 0;
    const int k = compact_step(hit, wave_cnt, &running);
    if (hit && k < cap) src[k] = s;
  }
  if (tid == 0) counts[1] = running;
}

__device__ __forceinline__ int live_rows(const int *__restrict__ counts, int cap) {
  return max(0, min(min(counts[0], counts[1]), cap));
}

template <typename OutT>
__device__ __forceinline__ OutT cvt(float v);
template <> __device__ __forceinline__ float cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ __half cvt<__half>(float v) { return __float2half(v); }
template <> __device__ __forceinline__ unsigned short cvt<unsigned short>(float v) {   // bf16, RNE
  unsigned u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

template <typename InT>
__device__ __forceinline__ float to_f32(InT v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<__half>(__half v) { return __half2float(v); }
template <> __device__ __forceinline__ float to_f32<unsigned short>(unsigned short v) {
  return __uint_as_float((unsigned)v << 16);
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward.  Workgroup tile: a band of 64 compacted rows x a slab of 128 columns, 4 waves of 64 x 32 (4 x 2 MFMA tiles of
// 16 x 16), K in slabs of 32 through a register-prefetched double buffer in LDS.  v_mfma_f32_16x16x4_f32: an ordered fp32
// fma chain over k, so the product is fp32-class as the reference's Linear outside autocast.  The launch reads W once per
// row band; with a handful of images that is one band.
constexpr int IP_BM = 64, IP_BN = 128, IP_BK = 32;
constexpr int IP_LD = IP_BK + 4;          // floats per LDS row (144 B: float4 fragments stay 16-byte aligned)

// 32-wide K slab of ROWS rows -> registers: ROWS/32 float4 per thread (thread t: row t/8 + 32p, k4 = (t%8)*4).
// rows[] maps a tile row to a row of P (or -1: zeros).
template <int ROWS>
__device__ __forceinline__ void ip_load(const float *__restrict__ P, int ld, const int (&rows)[ROWS / 32], int k0,
                                        float4 (&v)[ROWS / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < ROWS / 32; ++p)
    v[p] = rows[p] >= 0 ? *reinterpret_cast<const float4 *>(P + (size_t)rows[p] * ld + k0 + (t & 7) * 4)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
}
template <int ROWS>
__device__ __forceinline__ void ip_store(float *s, const float4 (&v)[ROWS / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < ROWS / 32; ++p)
    *reinterpret_cast<float4 *>(s + ((t >> 3) + 32 * p) * IP_LD + (t & 7) * 4) = v[p];
}

template <typename OutT>
__global__ __launch_bounds__(256) void image_project_scatter_kernel(
    int cap, int E, int C, int mode, const float *__restrict__ fts, const unsigned char *__restrict__ masks,
    const float *__restrict__ W, const float *__restrict__ bias, const int *__restrict__ dest,
    const int *__restrict__ src, const int *__restrict__ counts, OutT *__restrict__ embeds,
    long long *__restrict__ attn_mask) {
  __shared__ __attribute__((aligned(16))) float sA[2][IP_BM * IP_LD];
  __shared__ __attribute__((aligned(16))) float sB[2][IP_BN * IP_LD];
  const int n = live_rows(counts, cap);
  const int m0 = blockIdx.y * IP_BM, n0 = blockIdx.x * IP_BN;
  if (m0 >= n) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = lane & 15, g = lane >> 4;

  // the rows this thread stages: compacted row -> slot of img_fts (gathered through src), column -> row of W
  int arow[IP_BM / 32], brow[IP_BN / 32];
#pragma unroll
  for (int p = 0; p < IP_BM / 32; ++p) {
    const int m = m0 + (t >> 3) + 32 * p;
    int s = m < n ? src[m] : -1;
    if (s >= cap) s = -1;
    arow[p] = s;
  }
#pragma unroll
  for (int p = 0; p < IP_BN / 32; ++p) brow[p] = n0 + (t >> 3) + 32 * p;      // (E % 128 == 0: always inside W)

  f32x4v acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4v{0.f, 0.f, 0.f, 0.f};

  float4 ra[IP_BM / 32], rb[IP_BN / 32];
  ip_load<IP_BM>(fts, C, arow, 0, ra);
  ip_load<IP_BN>(W, C, brow, 0, rb);
  ip_store<IP_BM>(sA[0], ra);
  ip_store<IP_BN>(sB[0], rb);
  __syncthreads();
  const int nk = C / IP_BK;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      ip_load<IP_BM>(fts, C, arow, (kt + 1) * IP_BK, ra);
      ip_load<IP_BN>(W, C, brow, (kt + 1) * IP_BK, rb);
    }
    // lane (i, g), sub-slab `sub`, step s supplies A[row i][k = 16 sub + 4 g + s] and B[the same k][col i]
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      float4 fa[4], fb[2];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        fa[rt] = *reinterpret_cast<const float4 *>(&sA[cur][(rt * 16 + i) * IP_LD + sub * 16 + g * 4]);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        fb[ct] = *reinterpret_cast<const float4 *>(&sB[cur][(wave * 32 + ct * 16 + i) * IP_LD + sub * 16 + g * 4]);
#define MSR3D_IP_STEP(c)                                                                          \
  _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                \
  _Pragma("unroll") for (int ct = 0; ct < 2; ++ct)                                                \
      acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[rt].c, fb[ct].c, acc[rt][ct], 0, 0, 0);
      MSR3D_IP_STEP(x)
      MSR3D_IP_STEP(y)
      MSR3D_IP_STEP(z)
      MSR3D_IP_STEP(w)
#undef MSR3D_IP_STEP
    }
    if (kt + 1 < nk) {
      ip_store<IP_BM>(sA[cur ^ 1], ra);
      ip_store<IP_BN>(sB[cur ^ 1], rb);
    }
    __syncthreads();
  }

  // epilogue: + bias, cast, scatter.  Lane (i, g) holds rows 16 rt + 4 g + r of column i: 16 lanes write 16 adjacent
  // elements of one destination row.
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int col = n0 + wave * 32 + ct * 16 + i;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + rt * 16 + g * 4 + r;
        if (m < n) embeds[(size_t)dest[m] * E + col] = cvt<OutT>(acc[rt][ct][r] + bv);
      }
  }
  if (mode == 1 && blockIdx.x == 0 && attn_mask && masks && t < IP_BM && m0 + t < n) {
    const int s = src[m0 + t];
    if (s >= 0 && s < cap) attn_mask[dest[m0 + t]] = masks[s] ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  dW[e, c] (+)= sum_k G[k, e] f[src[k], c], db[e] (+)= sum_k G[k, e], G[k, :] = d_inputs_embeds[dest[k], :].
// A workgroup owns a 64 (e) x 32 (c) tile of dW and walks ALL n rows, 16 at a time in ascending order: no partial sums,
// no workspace, nothing to meet -- bit-identical from run to run.  4 waves of 16 x 32 (two 16 x 16 MFMA tiles).
constexpr int IG_BE = 64, IG_BC = 32, IG_BK = 16;
constexpr int IG_LDG = IG_BE + 16, IG_LDF = IG_BC + 16;

template <typename InT>
__global__ __launch_bounds__(256) void image_project_grad_kernel(
    int cap, int C, int E, int BT, const int *__restrict__ dest, const int *__restrict__ src,
    const int *__restrict__ counts, const float *__restrict__ fts, const InT *__restrict__ dE,
    float *__restrict__ dW, float *__restrict__ db, int accumulate) {
  __shared__ __attribute__((aligned(16))) float sG[IG_BK * IG_LDG];
  __shared__ __attribute__((aligned(16))) float sF[IG_BK * IG_LDF];
  const int n = live_rows(counts, cap);
  if (n == 0 && accumulate) return;
  const int e0 = blockIdx.y * IG_BE, c0 = blockIdx.x * IG_BC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = lane & 15, g = lane >> 4;
  f32x4v acc[2] = {f32x4v{0.f, 0.f, 0.f, 0.f}, f32x4v{0.f, 0.f, 0.f, 0.f}};
  float bsum = 0.f;                                       // thread t < 64 (first column of workgroups): db[e0 + t]
  const bool do_bias = db != nullptr && blockIdx.x == 0;

  for (int k0 = 0; k0 < n; k0 += IG_BK) {
    {   // G slab: 16 rows x 64 columns, thread t: row t/16, columns 4 (t%16) .. +3
      const int kk = t >> 4, e4 = (t & 15) * 4;
      const int k = k0 + kk;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < n) {
        const int row = dest[k];
        if (row >= 0 && row < BT) {
          const InT *p = dE + (size_t)row * E + e0 + e4;
          v = make_float4(to_f32<InT>(p[0]), to_f32<InT>(p[1]), to_f32<InT>(p[2]), to_f32<InT>(p[3]));
        }
      }
      *reinterpret_cast<float4 *>(&sG[kk * IG_LDG + e4]) = v;
    }
    if (t < 128) {   // f slab: 16 rows x 32 columns, thread t: row t/8, columns 4 (t%8) .. +3
      const int kk = t >> 3, c4 = (t & 7) * 4;
      const int k = k0 + kk;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < n) {
        const int s = src[k];
        if (s >= 0 && s < cap) v = *reinterpret_cast<const float4 *>(fts + (size_t)s * C + c0 + c4);
      }
      *reinterpret_cast<float4 *>(&sF[kk * IG_LDF + c4]) = v;
    }
    __syncthreads();
    // lane (i, g), step s supplies A[e = i][k = 4 s + g] and B[the same k][c = i]
#pragma unroll
    for (int s = 0; s < IG_BK / 4; ++s) {
      const float a = sG[(4 * s + g) * IG_LDG + wave * 16 + i];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sF[(4 * s + g) * IG_LDF + ct * 16 + i], acc[ct], 0, 0, 0);
    }
    if (do_bias && t < IG_BE) {
#pragma unroll
      for (int kk = 0; kk < IG_BK; ++kk) bsum += sG[kk * IG_LDG + t];
    }
    __syncthreads();
  }

#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float *p = dW + (size_t)(e0 + wave * 16 + g * 4 + r) * C + c0 + ct * 16 + i;
      *p = accumulate ? *p + acc[ct][r] : acc[ct][r];
    }
  if (do_bias && t < IG_BE) db[e0 + t] = accumulate ? db[e0 + t] + bsum : bsum;
}

// rows dest[k], k < n, of d_inputs_embeds <- 0 (after the gradient kernel has read them: same stream)
template <typename InT>
__global__ void image_clear_rows_kernel(int cap, int E, int BT, const int *__restrict__ dest,
                                        const int *__restrict__ counts, InT *__restrict__ dE) {
  const int n = live_rows(counts, cap);
  const int k = blockIdx.x;
  if (k >= n) return;
  const int row = dest[k];
  if (row < 0 || row >= BT) return;
  InT *p = dE + (size_t)row * E;
  for (int c = threadIdx.x; c < E; c += blockDim.x) p[c] = cvt<InT>(0.f);
}

inline bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace

extern "C" {

int msr3d_image_project_scatter(int B, int T, int N, int C, int E, int mode, const long long *input_ids,
                                long long img_token, const float *img_fts, const unsigned char *img_masks,
                                const void *weight, int weight_dtype, const float *bias, int out_dtype,
                                void *inputs_embeds, long long *attention_mask, int *dest, int *src,
                                int *counts, msr3d_stream_t stream) {
  if (B < 0 || T <= 0 || N < 0 || C <= 0 || E <= 0 || C % IP_BK != 0 || E % IP_BN != 0) return MSR3D_EINVAL;
  if (mode != 0 && mode != 1) return MSR3D_EINVAL;
  if (weight_dtype != 0 || out_dtype < 0 || out_dtype > 2) return MSR3D_EINVAL;
  if ((long long)B * T > INT_MAX || (long long)B * N > INT_MAX) return MSR3D_EINVAL;
  if (B == 0 || N == 0) return 0;
  if (!input_ids || !img_fts || !img_masks || !weight || !inputs_embeds || !dest || !src || !counts)
    return MSR3D_EINVAL;
  if (misaligned16(img_fts) || misaligned16(weight) || misaligned16(inputs_embeds)) return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int cap = B * N;
  image_map_kernel<<<1, 256, 0, st>>>(B, T, cap, mode, input_ids, img_token, img_masks, dest, src, counts);
  const dim3 grid(E / IP_BN, (cap + IP_BM - 1) / IP_BM);
  const float *W = (const float *)weight;
  switch (out_dtype) {
    case 0:
      image_project_scatter_kernel<float><<<grid, 256, 0, st>>>(cap, E, C, mode, img_fts, img_masks, W, bias, dest, src,
                                                                 counts, (float *)inputs_embeds, attention_mask);
      break;
    case 1:
      image_project_scatter_kernel<__half><<<grid, 256, 0, st>>>(cap, E, C, mode, img_fts, img_masks, W, bias, dest, src,
                                                                  counts, (__half *)inputs_embeds, attention_mask);
      break;
    default:
      image_project_scatter_kernel<unsigned short><<<grid, 256, 0, st>>>(
          cap, E, C, mode, img_fts, img_masks, W, bias, dest, src, counts, (unsigned short *)inputs_embeds,
          attention_mask);
      break;
  }
  return (int)hipGetLastError();
}

int msr3d_image_project_grad(int cap, int C, int E, int BT, const int *dest, const int *src,
                             const int *counts, const float *img_fts, int g_dtype, void *d_inputs_embeds,
                             float *dW, float *db, int accumulate, int clear_rows, msr3d_stream_t stream) {
  if (cap < 0 || C <= 0 || E <= 0 || BT < 0 || C % IP_BK != 0 || E % IP_BN != 0) return MSR3D_EINVAL;
  if (g_dtype < 0 || g_dtype > 2) return MSR3D_EINVAL;
  if (!counts || !dW) return MSR3D_EINVAL;
  if (cap > 0 && (!dest || !src || !img_fts || !d_inputs_embeds)) return MSR3D_EINVAL;
  if (misaligned16(img_fts) || misaligned16(d_inputs_embeds) || misaligned16(dW)) return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(C / IG_BC, E / IG_BE);
  const int thr = E >= 256 ? 256 : 64;
  switch (g_dtype) {
    case 0:
      image_project_grad_kernel<float><<<grid, 256, 0, st>>>(cap, C, E, BT, dest, src, counts, img_fts,
                                                              (const float *)d_inputs_embeds, dW, db, accumulate);
      if (clear_rows && cap > 0)
        image_clear_rows_kernel<float><<<cap, thr, 0, st>>>(cap, E, BT, dest, counts, (float *)d_inputs_embeds);
      break;
    case 1:
      image_project_grad_kernel<__half><<<grid, 256, 0, st>>>(cap, C, E, BT, dest, src, counts, img_fts,
                                                               (const __half *)d_inputs_embeds, dW, db, accumulate);
      if (clear_rows && cap > 0)
        image_clear_rows_kernel<__half><<<cap, thr, 0, st>>>(cap, E, BT, dest, counts, (__half *)d_inputs_embeds);
      break;
    default:
      image_project_grad_kernel<unsigned short><<<grid, 256, 0, st>>>(
          cap, C, E, BT, dest, src, counts, img_fts, (const unsigned short *)d_inputs_embeds, dW, db, accumulate);
      if (clear_rows && cap > 0)
        image_clear_rows_kernel<unsigned short><<<cap, thr, 0, st>>>(cap, E, BT, dest, counts,
                                                                     (unsigned short *)d_inputs_embeds);
      break;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
