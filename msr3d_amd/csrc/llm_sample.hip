// llm_sample.hip -- drawing tokens for `generate(do_sample=True)` (msr3d_amd/llm/generate.py: torch_sample_scores +
// torch_sample are the statement):
//
//     msr3d_decode_sample   logits processors, temperature, top-k, top-p, then k draws without replacement per row
//     msr3d_gumbel_noise    the noise the draw uses, written out (the same device function)
//
// One workgroup per live row, the row's V scores in LDS as fp32, like msr3d_decode_select.  There is no sort: the top-k
// value and the top-p cut are found by a radix walk (four 8-bit digits, most significant first) over an order-preserving
// integer image of the scores -- a 256-bin histogram per digit, counted for top-k, weighted by probability mass for
// top-p.  The mass is fixed point (exp(s - max) 2^40 in 64-bit LDS adds), so a histogram does not depend on the order
// its adds arrive in and the cut is the same bits call after call; the total of the first histogram is the softmax's
// denominator in the same fixed point, and the threshold floor((1 - top_p) x total) is computed once from it in double
// (the total, up to V 2^40, is rounded to 53 bits there: a relative 1e-16), after which every comparison of a running
// mass with it is between integers.  1 - top_p is taken from the fp32 top_p the entry receives.  Equal scores are
// ordered by token id (a stable ascending sort): inside the group of equal scores the cut falls in, the lower ids go
// first, found by a count in token-id order.  A draw is the arg-max of w + Gumbel noise; k draws without replacement
// are the k largest keys.  The noise is a counter hash of (seed, step, global row, token): no state, any launch shape.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/msr3d_hip.h"

namespace {

using u16 = unsigned short;
using u32 = unsigned;
using u64 = unsigned long long;

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((u32)v << 16); }

// ---- counter noise ----------------------------------------------------------------------------------------------
// generate.py::counter_uniform_bits restates this in integers.
__device__ __forceinline__ u32 mix32(u32 x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
struct RowKey { u32 a, b; };
__device__ __forceinline__ RowKey row_key(u64 seed, u32 step, u32 row) {
  const u32 lo = (u32)seed, hi = (u32)(seed >> 32);
  RowKey k;
  k.a = mix32(mix32(mix32(lo) ^ step) ^ row);
  k.b = mix32(mix32(mix32(hi ^ 0x85ebca6bu) + row) ^ step);
  return k;
}
__device__ __forceinline__ u32 uniform_bits(RowKey k, u32 tok) { return mix32(mix32(tok ^ k.a) + k.b) >> 8; }
// -log(-log u), u = (bits + 0.5) 2^-24 = (2 bits + 1) 2^-25.  Below 1/2 the odd numerator has at most 24 bits and u is
// exact in fp32; above, 1 - u is, and -log u = -log1p(-(1 - u)) keeps its relative accuracy where u itself would round
// (to 1.0 at the top).  -2.85 <= g <= 17.33.
__device__ __forceinline__ float gumbel(u32 bits) {
  const u32 odd = 2u * bits + 1u;
  const float t = bits < (1u << 23) ? -logf((float)odd * 0x1p-25f) : -log1pf(-((float)((1u << 25) - odd) * 0x1p-25f));
  return -logf(t);
}

// ---- scores -----------------------------------------------------------------------------------------------------
// the order-preserving image: a < b as floats <=> okey(a) < okey(b) (no NaN; -0 never occurs, see temper)
__device__ __forceinline__ u32 okey(float f) {
  const u32 u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float penalise(float x, float penalty) { return x < 0.f ? x * penalty : x / penalty; }
__device__ __forceinline__ float temper(float x, float temperature) {
  const float s = x / temperature;
  return s == 0.f ? 0.f : s;                          // one zero: equal scores have equal images
}
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ u64 mass_of(float s, float mx) { return (u64)(expf(s - mx) * 0x1p40f); }

// what a radix walk leaves behind (LDS)
struct Walk {
  u32 prefix;      // the digits chosen so far, in place
  u32 before_c;    // entries in the bins passed over
  u32 group_c;     // entries in the chosen bin
  u64 T;           // what is left of the threshold inside the chosen bin
  u64 group_w;     // weight of the chosen bin
};

// The walk: over the entries in walk order (ascending image; DESC: descending), find the group of equal scores at which
// the running weight first exceeds T.  MASS: an entry weighs exp(s - mx) 2^40 and T = floor(frac x total weight);
// otherwise it weighs 1 and T = t0 (the t0-th entry, counting from 0, lies in the group found).  Leaves in `wk`:
// prefix = the group's image (DESC: its complement), before_c = entries strictly before the group, T = threshold left
// after the weight before the group, group_c / group_w = the group's entries and weight.  Every thread of the 256 calls
// it; hw / hc are the 256-bin histograms.  Integer adds only: the result does not depend on their order.
template <bool MASS, bool DESC>
__device__ void radix_walk(const float *sc, int V, float mx, u64 t0, double frac, u64 *hw, u32 *hc, Walk *wk) {
  const int tid = threadIdx.x;
  if (tid == 0) { wk->prefix = 0; wk->before_c = 0; wk->T = t0; wk->group_c = 0; wk->group_w = 0; }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const u32 mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    hw[tid] = 0; hc[tid] = 0;
    __syncthreads();
    const u32 prefix = wk->prefix;
    // a thread adds runs of entries that fall into one bin at once: the first digit is the sign and most of the
    // exponent, which nearly every score of a row shares -- one add per run instead of one per entry
    int cb = -1;
    u64 aw = 0;
    u32 ac = 0;
    for (int v = tid; v < V; v += 256) {
      const float s = sc[v];
      u32 key = okey(s);
      if (DESC) key = ~key;
      if ((key & mask) != prefix) continue;
      const int bin = (int)((key >> shift) & 255u);
      if (bin != cb) {
        if (cb >= 0) { atomicAdd(&hw[cb], aw); atomicAdd(&hc[cb], ac); }
        cb = bin; aw = 0; ac = 0;
      }
      aw += MASS ? mass_of(s, mx) : 1ull;
      ac += 1;
    }
    if (cb >= 0) { atomicAdd(&hw[cb], aw); atomicAdd(&hc[cb], ac); }
    __syncthreads();
    if (tid < 64) {                                   // one wave: lane l owns bins 4 l .. 4 l + 3
      u64 w[4];
      u32 c[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { w[j] = hw[4 * tid + j]; c[j] = hc[4 * tid + j]; }
      const u64 lw = (w[0] + w[1]) + (w[2] + w[3]);
      const u32 lc = (c[0] + c[1]) + (c[2] + c[3]);
      u64 iw = lw;
      u32 ic = lc;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u64 ow = __shfl_up(iw, d);
        const u32 oc = __shfl_up(ic, d);
        if (tid >= d) { iw += ow; ic += oc; }
      }
      u64 T = wk->T;
      if (MASS && pass == 0) {
        const u64 total = __shfl(iw, 63);
        T = (u64)((double)total * frac);
      }
      const u64 found = __ballot(iw > T);
      const int first = found ? __ffsll((long long)found) - 1 : 63;
      if (tid == first) {
        u64 ew = iw - lw, gw = w[3];
        u32 ec = ic - lc, gc = c[3];
        int j = 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {                 // (unrolled: w and c stay in registers)
          if (j == 3 && ew + w[i] > T) { j = i; gw = w[i]; gc = c[i]; }
          if (j == 3) { ew += w[i]; ec += c[i]; }
        }
        wk->prefix = prefix | ((u32)(4 * tid + j) << shift);
        wk->before_c += ec;
        wk->T = T > ew ? T - ew : 0;
        wk->group_c = gc;
        wk->group_w = gw;
      }
    }
    __syncthreads();
  }
}

// block-wide sums / maxima in a fixed order (the same bits call after call); rv: 4 floats of LDS
__device__ __forceinline__ float block_max(float x, float *rv) {
  for (int d = 32; d > 0; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
  if ((threadIdx.x & 63) == 0) rv[threadIdx.x >> 6] = x;
  __syncthreads();
  x = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
  __syncthreads();
  return x;
}
__device__ __forceinline__ float block_sum(float x, float *rv) {
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  if ((threadIdx.x & 63) == 0) rv[threadIdx.x >> 6] = x;
  __syncthreads();
  x = ((rv[0] + rv[1]) + rv[2]) + rv[3];
  __syncthreads();
  return x;
}

__global__ __launch_bounds__(256) void decode_sample_kernel(
    int V, const u16 *__restrict__ logits, int ldl, const long long *__restrict__ prev, int ldprev,
    const int *__restrict__ n_prev, int prev_cap, float penalty, int min_length, int eos,
    const float *__restrict__ beam_score, int order, int k, float temperature, int top_k, float top_p, int min_keep,
    const float *__restrict__ noise, int ld_noise, u64 seed, u32 step, u32 row0, float *__restrict__ out_key,
    float *__restrict__ out_val, int *__restrict__ out_tok) {
  extern __shared__ float sc[];                     // the row's V scores
  __shared__ u64 hw[256];
  __shared__ u32 hc[256];
  __shared__ Walk wk;
  __shared__ float rv[4];
  __shared__ int ri[4];
  __shared__ u32 wave_c[4];
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const u16 *lg = logits + (size_t)n * ldl;
  const int np = n_prev ? min(max(n_prev[n], 0), prev_cap) : 0;
  const long long *pv = prev + (size_t)n * ldprev;
  const bool hold_eos = np < min_length && eos >= 0 && eos < V;
  for (int v = tid; v < V; v += 256) sc[v] = bf2f(lg[v]);
  __syncthreads();
  // -- the processors (as decode_select_kernel), then the temperature
  float lse0 = 0.f;                                   // order 1: the log-sum-exp of the raw logits
  if (order == 1) {
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, sc[v]);
    mx = block_max(mx, rv);
    float sum = 0.f;
    for (int v = tid; v < V; v += 256) sum += expf(sc[v] - mx);
    lse0 = mx + logf(block_sum(sum, rv));
    for (int v = tid; v < V; v += 256) sc[v] = sc[v] - lse0;
    __syncthreads();
  }
  if (penalty != 1.0f) {
    // every occurrence of a token writes the same value (computed from the unprocessed logit): applied once
    for (int i = tid; i < np; i += 256) {
      const long long t = pv[i];
      if (t < 0 || t >= V) continue;
      sc[t] = penalise(bf2f(lg[t]) - lse0, penalty);
    }
    __syncthreads();
  }
  if (tid == 0 && hold_eos) sc[eos] = -INFINITY;
  __syncthreads();
  for (int v = tid; v < V; v += 256) sc[v] = temper(sc[v], temperature);
  __syncthreads();
  // -- top-k: everything below the kk-th largest value goes; ties at that value stay
  const int kk = max(top_k, min_keep);
  if (top_k > 0 && kk < V) {
    radix_walk<false, true>(sc, V, 0.f, (u64)(kk - 1), 0.0, hw, hc, &wk);
    const u32 kth = ~wk.prefix;
    __syncthreads();
    for (int v = tid; v < V; v += 256)
      if (okey(sc[v]) < kth) sc[v] = -INFINITY;
    __syncthreads();
  }
  float mx = -INFINITY;
  for (int v = tid; v < V; v += 256) mx = fmaxf(mx, sc[v]);
  mx = block_max(mx, rv);
  // -- top-p: in ascending (score, token id) order, the entries whose running probability is <= 1 - top_p go, but
  // never the last min_keep
  if (top_p < 1.0f) {
    radix_walk<true, false>(sc, V, mx, 0, 1.0 - (double)top_p, hw, hc, &wk);
    u32 cut = wk.prefix, group_c = wk.group_c;
    const u64 q = group_c ? wk.group_w / group_c : 0;           // equal scores have equal mass
    u64 r64 = q ? wk.T / q : (u64)group_c;
    u32 r = r64 < group_c ? (u32)r64 : group_c;                 // entries of the group that go: the lowest ids
    const u32 removed = wk.before_c + r;
    __syncthreads();
    if (removed > (u32)(V - min_keep)) {
      // the cut would leave fewer than min_keep: keep the min_keep last of the order, i.e. the largest scores and,
      // inside the group of equal scores at that rank, the highest ids
      radix_walk<false, true>(sc, V, 0.f, (u64)(min_keep - 1), 0.0, hw, hc, &wk);
      cut = ~wk.prefix;
      group_c = wk.group_c;
      const u32 take = (u32)min_keep - wk.before_c;
      r = group_c > take ? group_c - take : 0;
      __syncthreads();
    }
    if (r >= group_c) {
      for (int v = tid; v < V; v += 256)
        if (okey(sc[v]) <= cut) sc[v] = -INFINITY;
    } else {
      for (int v = tid; v < V; v += 256)
        if (okey(sc[v]) < cut) sc[v] = -INFINITY;
      if (r > 0) {
        __syncthreads();
        // inside the group: a count in token-id order.  Thread t owns the ids [t chunk, (t + 1) chunk) (chunk odd:
        // the lanes' LDS words fall into distinct banks)
        const int chunk = ((V + 255) / 256) | 1;
        const int lo = min(V, tid * chunk), hi = min(V, lo + chunk);
        u32 mine = 0;
        for (int v = lo; v < hi; ++v) mine += okey(sc[v]) == cut;
        u32 inc = mine;
        for (int d = 1; d < 64; d <<= 1) {
          const u32 o = __shfl_up(inc, d);
          if (lane >= d) inc += o;
        }
        if (lane == 63) wave_c[wave] = inc;
        __syncthreads();
        u32 rank = inc - mine;
        for (int w = 0; w < wave; ++w) rank += wave_c[w];
        for (int v = lo; v < hi && rank < r; ++v)
          if (okey(sc[v]) == cut) { sc[v] = -INFINITY; ++rank; }
      }
    }
    __syncthreads();
  }
  // -- w: order 0 renormalises over what is left, order 1 adds the beam's score
  const float add = beam_score ? beam_score[n] : 0.f;
  float lse1 = 0.f;
  if (order == 0) {
    float sum = 0.f;
    for (int v = tid; v < V; v += 256) sum += expf(sc[v] - mx);
    lse1 = mx + logf(block_sum(sum, rv));
  }
  // -- key = w + noise (removed entries stay -inf)
  const RowKey rk = row_key(seed, step, row0 + (u32)n);
  const float *nz = noise ? noise + (size_t)n * ld_noise : nullptr;
  for (int v = tid; v < V; v += 256) {
    const float s = sc[v];
    if (s == -INFINITY) continue;
    const float w = order == 0 ? s - lse1 : s + add;
    sc[v] = w + (nz ? nz[v] : gumbel(uniform_bits(rk, (u32)v)));
  }
  __syncthreads();
  // -- k rounds of arg-max over the keys, ties to the lower token id
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY;
    int bi = V;                                       // V = nothing found (taken entries are NaN and never compare)
    for (int v = tid; v < V; v += 256) {
      const float x = sc[v];
      if (x > -INFINITY && (bi == V || better(x, v, bv, bi))) { bv = x; bi = v; }
    }
    for (int x = 32; x > 0; x >>= 1) {
      const float ov = __shfl_xor(bv, x);
      const int oi = __shfl_xor(bi, x);
      if (oi < V && (bi == V || better(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    bv = rv[0]; bi = ri[0];
    for (int w = 1; w < 4; ++w)
      if (ri[w] < V && (bi == V || better(rv[w], ri[w], bv, bi))) { bv = rv[w]; bi = ri[w]; }
    // w of the winner, from its logit again (the LDS word holds the key): is it one of the penalised tokens?
    int hit = 0;
    if (penalty != 1.0f && bi < V)
      for (int i = tid; i < np; i += 256) hit |= pv[i] == (long long)bi;
    hit = __syncthreads_or(hit);                      // (also: every thread has read rv / ri)
    if (tid == 0) {
      float key = -INFINITY, val = -INFINITY;
      int tok = -1;
      if (bi < V) {
        float s = bf2f(lg[bi]) - lse0;
        if (hit) s = penalise(s, penalty);
        s = temper(s, temperature);
        key = bv;
        val = order == 0 ? s - lse1 : s + add;
        tok = bi;
        sc[bi] = __int_as_float(0x7fc00000);
      }
      out_key[(size_t)n * k + r] = key;
      out_val[(size_t)n * k + r] = val;
      out_tok[(size_t)n * k + r] = tok;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void gumbel_noise_kernel(int V, u64 seed, u32 step, u32 row0, float *__restrict__ out,
                                                           int ld) {
  const int n = blockIdx.y;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  out[(size_t)n * ld + v] = gumbel(uniform_bits(row_key(seed, step, row0 + (u32)n), (u32)v));
}

}  // namespace

extern "C" {

int msr3d_decode_sample(int N, int V, const void *logits, int ldl, const long long *prev_tokens, int ld_prev,
                        const int *n_prev, float repetition_penalty, int min_length, int eos_id, const float *beam_score,
                        int order, int k, float temperature, int top_k, float top_p, int min_keep, const float *noise,
                        int ld_noise, long long seed, int step, int row0, float *out_key, float *out_val, int *out_tok,
                        msr3d_stream_t stream) {
  if (N < 0 || V <= 0 || V > MSR3D_DECODE_SAMPLE_MAX_V || ldl < V || k <= 0 || k > V || k > MSR3D_DECODE_SELECT_MAX_K ||
      (order != 0 && order != 1) || !(repetition_penalty > 0.f) || ld_prev < 0 || !(temperature > 0.f) || top_k < 0 ||
      !(top_p > 0.f && top_p <= 1.f) || min_keep < 1 || min_keep > V || (noise && ld_noise < V) || seed < 0 || step < 0 ||
      row0 < 0 || N > 0x7fffffff - row0)
    return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!logits || !out_key || !out_val || !out_tok || (n_prev && !prev_tokens)) return MSR3D_EINVAL;
  if ((size_t)V * sizeof(float) > 40 * 1024) {
    // more dynamic LDS than the default limit leaves beside the histograms: 160 KB a workgroup on this part
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(decode_sample_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, MSR3D_DECODE_SAMPLE_MAX_V * 4);
    if (e != hipSuccess) return (int)e;
  }
  decode_sample_kernel<<<N, 256, (size_t)V * sizeof(float), (hipStream_t)stream>>>(
      V, (const u16 *)logits, ldl, prev_tokens, ld_prev, n_prev, ld_prev, repetition_penalty, min_length, eos_id, beam_score,
      order, k, temperature, top_k, top_p, min_keep, noise, ld_noise, (u64)seed, (u32)step, (u32)row0, out_key, out_val,
      out_tok);
  return (int)hipGetLastError();
}

int msr3d_gumbel_noise(int N, int V, long long seed, int step, int row0, float *out, int ld, msr3d_stream_t stream) {
  if (N < 0 || V <= 0 || ld < V || seed < 0 || step < 0 || row0 < 0 || N > 65535 || N > 0x7fffffff - row0)
    return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!out) return MSR3D_EINVAL;
  gumbel_noise_kernel<<<dim3((unsigned)((V + 255) / 256), N), 256, 0, (hipStream_t)stream>>>(V, (u64)seed, (u32)step,
                                                                                          (u32)row0, out, ld);
  return (int)hipGetLastError();
}

}  // extern "C"
