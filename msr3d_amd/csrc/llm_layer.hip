// llm_layer.hip -- the row-local and element-wise kernels of one LoRA-Llama decoder layer (SURVEY.md §8(f)
// rank 4; /root/reference/model/msr3d/msr3d.py:103-112, 409-415: Vicuna-7B under bf16 autocast with peft
// LoRA on q/k/v/o/gate/up/down_proj).  The layer, as transformers' LlamaDecoderLayer computes it:
//
//     h = RMSNorm(x) ; q, k, v = LoRALinear(h) ; RoPE(q, k) ; P = softmax(q k^T / sqrt(d) + causal + padding)
//     x = x + LoRALinear_o(P v) ; h = RMSNorm(x) ; x = x + LoRALinear_down( silu(LoRALinear_gate(h)) * LoRALinear_up(h) )
//
// The seven projections are msr3d_bf16_gemm_lowrank (lora_linear.hip), the attention is fused (llm_attn.hip).
// Here: RMSNorm (+ the residual add in front of it) forward / backward, rotary embedding (forward and its
// transpose) and SwiGLU forward / backward.  bf16 storage, fp32 arithmetic, one rounding per stored value.
// All HBM-bound: algorithmic bytes = the tensors read + written once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/msr3d_hip.h"
#include "llm_rowmath.h"

namespace {

using namespace msr3d::llm;          // u16, bf2f, f2bf, unpack8, pack8, wave_sum, the RMSNorm row arithmetic

// ---- RMSNorm: one wave per row, D <= 8192, D % 512 == 0 (a lane holds D / 64 values as D / 512 x 8) ------
// forward:  s = x (+ delta);  y = w * bf16( s * rsqrt(mean(s^2) + eps) )       (modeling_llama.LlamaRMSNorm)
template <int V>     // V = D / 512 16-byte vectors per lane
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(int M, const u16 *__restrict__ x, const u16 *__restrict__ delta,
                                                          const u16 *__restrict__ w, float eps, u16 *__restrict__ sum_out,
                                                          u16 *__restrict__ y, float *__restrict__ rstd_out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  constexpr int D = V * 512;
  float s[V][8];
  float ss = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const size_t o = (size_t)row * D + (v * 64 + lane) * 8;
    unpack8(*reinterpret_cast<const uint4 *>(x + o), s[v]);
    if (delta) {
      float d[8];
      unpack8(*reinterpret_cast<const uint4 *>(delta + o), d);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[v][e] = residual_add(s[v][e], d[e]);
      if (sum_out) *reinterpret_cast<uint4 *>(sum_out + o) = pack8(s[v]);
    }
    ss = rms_sumsq8(s[v], ss);
  }
  const float rstd = rms_rstd(ss, 1.0f / D, eps);
  if (lane == 0 && rstd_out) rstd_out[row] = rstd;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    float g[8];
    unpack8(*reinterpret_cast<const uint4 *>(w + (v * 64 + lane) * 8), g);
    *reinterpret_cast<uint4 *>(y + (size_t)row * D + (v * 64 + lane) * 8) = rms_scale8(s[v], g, rstd);
  }
}
// backward (w frozen): g = dy * w;  dx = rstd * (g - xh * mean(g * xh)) (+ dres),  xh = s * rstd
template <int V>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(int M, const u16 *__restrict__ dy, const u16 *__restrict__ s_in,
                                                          const u16 *__restrict__ w, const float *__restrict__ rstd_in,
                                                          const u16 *__restrict__ dres, u16 *__restrict__ dx) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  constexpr int D = V * 512;
  const float rstd = rstd_in[row];
  float g[V][8], xh[V][8];
  float c = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const size_t o = (size_t)row * D + (v * 64 + lane) * 8;
    float d[8], ww[8], s[8];
    unpack8(*reinterpret_cast<const uint4 *>(dy + o), d);
    unpack8(*reinterpret_cast<const uint4 *>(w + (v * 64 + lane) * 8), ww);
    unpack8(*reinterpret_cast<const uint4 *>(s_in + o), s);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      g[v][e] = d[e] * ww[e];
      xh[v][e] = s[e] * rstd;
      c = fmaf(g[v][e], xh[v][e], c);
    }
  }
  c = wave_sum(c) * (1.0f / D);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const size_t o = (size_t)row * D + (v * 64 + lane) * 8;
    float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o8[8];
    if (dres) unpack8(*reinterpret_cast<const uint4 *>(dres + o), r);
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = rstd * (g[v][e] - xh[v][e] * c) + r[e];
    *reinterpret_cast<uint4 *>(dx + o) = pack8(o8);
  }
}

// ---- rotary embedding, in place on (B, T, H, D) bf16; cos / sin (T, D) fp32 (position = t) ----------------
// x' = x cos + rotate_half(x) sin, rotate_half(x) = [-x2, x1] (modeling_llama.apply_rotary_pos_emb);
// sign = -1 applies the transpose (the backward): dx = dx' cos - rotate_half(dx' ... ) i.e. sin -> -sin.
__global__ __launch_bounds__(256) void rope_kernel(long long n_pairs, int T, int H, int D, u16 *__restrict__ x,
                                                   const float *__restrict__ cs, const float *__restrict__ sn, float sign) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;     // one (b, t, h, i < D/2) pair per thread
  if (p >= n_pairs) return;
  const int half = D >> 1;
  const int i = (int)(p % half);
  const long long bth = p / half;
  const int t = (int)((bth / H) % T);
  u16 *q = x + bth * D;
  const float a = bf2f(q[i]), b = bf2f(q[i + half]);
  const float c1 = cs[(size_t)t * D + i], c2 = cs[(size_t)t * D + i + half];
  const float s1 = sign * sn[(size_t)t * D + i], s2 = sign * sn[(size_t)t * D + i + half];
  q[i] = f2bf(a * c1 - b * s1);
  q[i + half] = f2bf(b * c2 + a * s2);
}
// D % 16 == 0, H % HG == 0: a thread owns eight adjacent pairs (two 16-byte pieces) of HG heads of one token -- the
// token's cos / sin values are loaded once and used HG times (the pair-per-thread kernel above reads 16 table bytes
// per 4 data bytes, 2-byte accesses: 15 us for 19 MB in place); up to two tensors (q and k) in one launch.
template <int HG>
__global__ __launch_bounds__(256) void rope_vec_kernel(long long n_items, int T, int H, int D, u16 *__restrict__ x0,
                                                       u16 *__restrict__ x1, const float *__restrict__ cs,
                                                       const float *__restrict__ sn, float sign) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= n_items) return;
  const int half = D >> 1, npc = D >> 4, ngr = H / HG;
  const int c = (int)(id % npc);
  const int hg = (int)((id / npc) % ngr);
  const long long bt = id / ((long long)npc * ngr);
  const int t = (int)(bt % T), i0 = 8 * c;
  float c1[8], c2[8], s1[8], s2[8];
  {
    const float *cr = cs + (size_t)t * D + i0, *sr = sn + (size_t)t * D + i0;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const float4 a = *reinterpret_cast<const float4 *>(cr + 4 * v), b = *reinterpret_cast<const float4 *>(cr + half + 4 * v);
      const float4 e = *reinterpret_cast<const float4 *>(sr + 4 * v), f = *reinterpret_cast<const float4 *>(sr + half + 4 * v);
      c1[4 * v] = a.x; c1[4 * v + 1] = a.y; c1[4 * v + 2] = a.z; c1[4 * v + 3] = a.w;
      c2[4 * v] = b.x; c2[4 * v + 1] = b.y; c2[4 * v + 2] = b.z; c2[4 * v + 3] = b.w;
      s1[4 * v] = sign * e.x; s1[4 * v + 1] = sign * e.y; s1[4 * v + 2] = sign * e.z; s1[4 * v + 3] = sign * e.w;
      s2[4 * v] = sign * f.x; s2[4 * v + 1] = sign * f.y; s2[4 * v + 2] = sign * f.z; s2[4 * v + 3] = sign * f.w;
    }
  }
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    u16 *x = which ? x1 : x0;
    if (!x) continue;
    u16 *row = x + (bt * H + (long long)hg * HG) * D + i0;
    uint4 va[HG], vb[HG];
#pragma unroll
    for (int hh = 0; hh < HG; ++hh) {
      va[hh] = *reinterpret_cast<const uint4 *>(row + (size_t)hh * D);
      vb[hh] = *reinterpret_cast<const uint4 *>(row + (size_t)hh * D + half);
    }
#pragma unroll
    for (int hh = 0; hh < HG; ++hh) {
      float a[8], b[8], ya[8], yb[8];
      unpack8(va[hh], a);
      unpack8(vb[hh], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) { ya[e] = a[e] * c1[e] - b[e] * s1[e]; yb[e] = b[e] * c2[e] + a[e] * s2[e]; }
      *reinterpret_cast<uint4 *>(row + (size_t)hh * D) = pack8(ya);
      *reinterpret_cast<uint4 *>(row + (size_t)hh * D + half) = pack8(yb);
    }
  }
}

// ---- SwiGLU: h = silu(gate) * up ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(long long n8, const uint4 *__restrict__ gate, const uint4 *__restrict__ up,
                                                         uint4 *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float g[8], u[8], o[8];
  unpack8(gate[i], g);
  unpack8(up[i], u);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float sg = bf2f(f2bf(g[e] / (1.0f + expf(-g[e]))));      // silu is its own (bf16) op in the reference graph
    o[e] = sg * u[e];
  }
  out[i] = pack8(o);
}
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(long long n8, const uint4 *__restrict__ gate, const uint4 *__restrict__ up,
                                                         const uint4 *__restrict__ dh, uint4 *__restrict__ dgate,
                                                         uint4 *__restrict__ dup) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float g[8], u[8], d[8], og[8], ou[8];
  unpack8(gate[i], g);
  unpack8(up[i], u);
  unpack8(dh[i], d);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float sig = 1.0f / (1.0f + expf(-g[e]));
    const float sl = g[e] * sig;
    ou[e] = d[e] * sl;
    og[e] = d[e] * u[e] * (sig * (1.0f + g[e] * (1.0f - sig)));
  }
  dgate[i] = pack8(og);
  dup[i] = pack8(ou);
}

inline bool al16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

}  // namespace

extern "C" {

int msr3d_rmsnorm_fwd(int M, int D, const void *x, const void *delta, const void *w, float eps, void *sum_out,
                      void *y, float *rstd, msr3d_stream_t stream) {
  // (1536: three vectors a lane, the odd count the fused skinny product's prologue is tested against)
  if (M < 0 || (D != 512 && D != 1024 && D != 1536 && D != 2048 && D != 4096 && D != 5120 && D != 8192))
    return MSR3D_EINVAL;
  if (M == 0) return 0;
  if (!x || !w || !y || !al16(x) || !al16(w) || !al16(y) || (delta && !al16(delta)) || (sum_out && !al16(sum_out)))
    return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int g = (M + 3) / 4;
#define MSR3D_RMS(V)                                                                                              \
  rmsnorm_fwd_kernel<V><<<g, 256, 0, st>>>(M, (const u16 *)x, (const u16 *)delta, (const u16 *)w, eps, (u16 *)sum_out, \
                                           (u16 *)y, rstd)
  switch (D / 512) {
    case 1: MSR3D_RMS(1); break;
    case 2: MSR3D_RMS(2); break;
    case 3: MSR3D_RMS(3); break;
    case 4: MSR3D_RMS(4); break;
    case 8: MSR3D_RMS(8); break;
    case 10: MSR3D_RMS(10); break;
    default: MSR3D_RMS(16); break;
  }
#undef MSR3D_RMS
  return (int)hipGetLastError();
}

int msr3d_rmsnorm_bwd(int M, int D, const void *dy, const void *s, const void *w, const float *rstd,
                      const void *dres, void *dx, msr3d_stream_t stream) {
  if (M < 0 || (D != 512 && D != 1024 && D != 2048 && D != 4096 && D != 5120 && D != 8192)) return MSR3D_EINVAL;
  if (M == 0) return 0;
  if (!dy || !s || !w || !rstd || !dx || !al16(dy) || !al16(s) || !al16(w) || !al16(dx) || (dres && !al16(dres)))
    return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int g = (M + 3) / 4;
#define MSR3D_RMSB(V)                                                                                          \
  rmsnorm_bwd_kernel<V><<<g, 256, 0, st>>>(M, (const u16 *)dy, (const u16 *)s, (const u16 *)w, rstd, (const u16 *)dres, \
                                           (u16 *)dx)
  switch (D / 512) {
    case 1: MSR3D_RMSB(1); break;
    case 2: MSR3D_RMSB(2); break;
    case 4: MSR3D_RMSB(4); break;
    case 8: MSR3D_RMSB(8); break;
    case 10: MSR3D_RMSB(10); break;
    default: MSR3D_RMSB(16); break;
  }
#undef MSR3D_RMSB
  return (int)hipGetLastError();
}

static int rope_launch(int B, int T, int H, int D, void *x0, void *x1, const float *cos_td, const float *sin_td, int transpose,
                       msr3d_stream_t stream) {
  if (B < 0 || T <= 0 || H <= 0 || D <= 0 || (D & 1)) return MSR3D_EINVAL;
  if (B == 0) return 0;
  if (!x0 || !cos_td || !sin_td) return MSR3D_EINVAL;
  const float sign = transpose ? -1.0f : 1.0f;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (D % 16) == 0 && !(reinterpret_cast<uintptr_t>(x0) & 15u) && !(reinterpret_cast<uintptr_t>(x1) & 15u) &&
                   !(reinterpret_cast<uintptr_t>(cos_td) & 15u) && !(reinterpret_cast<uintptr_t>(sin_td) & 15u);
  if (vec) {
    const int hg = (H % 4) == 0 ? 4 : 1;
    const long long n = (long long)B * T * (H / hg) * (D / 16);
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (hg == 4) rope_vec_kernel<4><<<grid, 256, 0, st>>>(n, T, H, D, (u16 *)x0, (u16 *)x1, cos_td, sin_td, sign);
    else rope_vec_kernel<1><<<grid, 256, 0, st>>>(n, T, H, D, (u16 *)x0, (u16 *)x1, cos_td, sin_td, sign);
    return (int)hipGetLastError();
  }
  const long long n = (long long)B * T * H * (D / 2);
  rope_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, T, H, D, (u16 *)x0, cos_td, sin_td, sign);
  if (x1) rope_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, T, H, D, (u16 *)x1, cos_td, sin_td, sign);
  return (int)hipGetLastError();
}

int msr3d_rope_inplace(int B, int T, int H, int D, void *x, const float *cos_td, const float *sin_td, int transpose,
                       msr3d_stream_t stream) {
  return rope_launch(B, T, H, D, x, nullptr, cos_td, sin_td, transpose, stream);
}

int msr3d_rope_inplace2(int B, int T, int H, int D, void *x0, void *x1, const float *cos_td, const float *sin_td,
                        int transpose, msr3d_stream_t stream) {
  if (!x1) return MSR3D_EINVAL;
  return rope_launch(B, T, H, D, x0, x1, cos_td, sin_td, transpose, stream);
}

int msr3d_swiglu_fwd(long long n, const void *gate, const void *up, void *out, msr3d_stream_t stream) {
  if (n < 0 || (n % 8)) return MSR3D_EINVAL;
  if (n == 0) return 0;
  if (!gate || !up || !out || !al16(gate) || !al16(up) || !al16(out)) return MSR3D_EINVAL;
  swiglu_fwd_kernel<<<(unsigned)((n / 8 + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      n / 8, (const uint4 *)gate, (const uint4 *)up, (uint4 *)out);
  return (int)hipGetLastError();
}

int msr3d_swiglu_bwd(long long n, const void *gate, const void *up, const void *dh, void *dgate, void *dup,
                     msr3d_stream_t stream) {
  if (n < 0 || (n % 8)) return MSR3D_EINVAL;
  if (n == 0) return 0;
  if (!gate || !up || !dh || !dgate || !dup || !al16(gate) || !al16(up) || !al16(dh) || !al16(dgate) || !al16(dup))
    return MSR3D_EINVAL;
  swiglu_bwd_kernel<<<(unsigned)((n / 8 + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      n / 8, (const uint4 *)gate, (const uint4 *)up, (const uint4 *)dh, (uint4 *)dgate, (uint4 *)dup);
  return (int)hipGetLastError();
}

}  // extern "C"
