// llm_rowmath.h -- the row-local arithmetic of a LoRA-Llama layer that more than one kernel states: the RMSNorm of
// rmsnorm_fwd_kernel (llm_layer.hip), its residual addition, and the rotation of a rotary pair (rope_rotate,
// llm_decode.hip).  A kernel that applies one of them while it stages a product's operand or stores its sums (the fused
// skinny product, llm_decode.hip) calls the same functions in the same order and so gives the bits of the stand-alone
// launch.  Every multiply-add that the compiler could fuse either way is written out: as an fmaf, or under contract(off).
#pragma once
#include <hip/hip_runtime.h>

namespace msr3d {
namespace llm {

using u16 = unsigned short;

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ u16 f2bf(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}
__device__ __forceinline__ void unpack8(uint4 v, float (&f)[8]) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(w[i] << 16); f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (unsigned)f2bf(f[2 * i]) | ((unsigned)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- RMSNorm of one row held by one wave: lane l owns the 16-byte vectors v * 64 + l, v < D / 512 ----------------------
// the residual stream is stored in bf16: x + delta, rounded
__device__ __forceinline__ float residual_add(float x, float delta) { return bf2f(f2bf(x + delta)); }
// a lane's sum of squares grows one vector at a time, in (v, e) order
__device__ __forceinline__ float rms_sumsq8(const float (&s)[8], float ss) {
#pragma unroll
  for (int e = 0; e < 8; ++e) ss = fmaf(s[e], s[e], ss);
  return ss;
}
// ss: the lane's sum of squares; inv_d = 1 / D as a correctly rounded float -> the row's rstd, in every lane
__device__ __forceinline__ float rms_rstd(float ss, float inv_d, float eps) { return rsqrtf(fmaf(wave_sum(ss), inv_d, eps)); }
// y = w * bf16(s * rstd), rounded: the two roundings of modeling_llama.LlamaRMSNorm under bf16
__device__ __forceinline__ uint4 rms_scale8(const float (&s)[8], const float (&g)[8], float rstd) {
  float o8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = g[e] * bf2f(f2bf(s[e] * rstd));
  return pack8(o8);
}

// ---- one rotary pair (a, b) = (x[i], x[i + D / 2]) with the table values of both halves -------------------------------
// the contraction rope_vec_kernel (llm_layer.hip) compiles to, pinned: the second product rounded, the first fused into
// the sum
__device__ __forceinline__ void rope_pair(float a, float b, float c1, float c2, float s1, float s2, float &ya, float &yb) {
#pragma clang fp contract(off)
  ya = fmaf(a, c1, -(b * s1));
  yb = fmaf(b, c2, a * s2);
}

}  // namespace llm
}  // namespace msr3d
