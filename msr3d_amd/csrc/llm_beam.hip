// llm_beam.hip -- the bookkeeping of one decoded token on the device (msr3d_amd/llm/search.py states it in torch:
// torch_beam_advance, torch_greedy_advance), so that a token of `generate` is a chain of launches with nothing for the
// host to decide and can be replayed from a captured graph (CachedDecoder.token_loop).
//
//     msr3d_beam_advance     beam search: a step's 2 nb candidates per row -> the next running beams, the kept finished
//                            hypotheses, the stopping heuristic, next_tok / beam_idx for the step that follows
//     msr3d_greedy_advance   greedy search: the chosen token or pad, the row's sequence, `unfinished`
//
// Integer and f32 arithmetic only, written in the statement's order and compiled without contraction: every field of
// the state equals the statement's bit for bit.  Every top-k is a rank by counting under ONE total order -- the larger
// value first, equal values by the lower index (what the first k of a stable descending sort are); values are never
// NaN (msr3d_decode_select writes none).  `cur` and `done` are device words read at entry and written with ordinary
// vector stores by the last launch of an entry; once `done` is set every kernel returns at once and nothing changes.
// No atomics.  Every index that forms an address comes from a rank (< its bound by construction, and the slots are
// preset to 0) or is range-checked first.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/msr3d_hip.h"

namespace {

constexpr int MAX_NB = 32;                       // beams per prompt
constexpr int MAX_K2 = MSR3D_DECODE_SELECT_MAX_K; // 2 nb candidates a row
constexpr int MAX_CAND = MAX_NB * MAX_K2;        // candidates per prompt

// j before i in the stable descending order
__device__ __forceinline__ bool before(float vj, int j, float vi, int i) { return vj > vi || (vj == vi && j < i); }

// One workgroup per prompt b.  work[b]: bit 0 = the prompt's new heuristic, bit 1 = every candidate of it ended.
__global__ __launch_bounds__(256) void beam_advance_kernel(int nb, int L, const float *__restrict__ val,
                                                           const int *__restrict__ tok, long long eos,
                                                           const float *__restrict__ len_div, float *run_scores,
                                                           long long *run_seq, long long *fin_seq, float *fin_scores,
                                                           long long *fin_len, unsigned char *is_fin, unsigned char *heur,
                                                           const int *cur_p, const int *done_p, long long *next_tok,
                                                           int *beam_idx, int *work) {
  __shared__ float sv[MAX_CAND];                 // the prompt's candidates, beam-major
  __shared__ int top_i[MAX_K2];                  // the K2 best, in order
  __shared__ float t_val[MAX_K2], t_lp[MAX_K2];  // their value; value - 1e9 where the candidate ended
  __shared__ long long t_tok[MAX_K2];
  __shared__ int t_src[MAX_K2], t_hit[MAX_K2], t_did[MAX_K2];
  __shared__ float m_sc[MAX_NB + MAX_K2];        // kept scores | this step's finished scores
  __shared__ long long o_len[MAX_NB];            // the kept hypotheses before this step
  __shared__ int o_fin[MAX_NB];
  __shared__ int nxt[MAX_NB], mi[MAX_NB];        // the next running beams (of K2), the kept hypotheses (of nb + K2)
  __shared__ float n_fs[MAX_NB];
  __shared__ int n_fin[MAX_NB];
  if (*done_p != 0) return;
  const int c = *cur_p;
  if (c < 0 || c >= L) return;                   // (a state past its last step: nothing to do, nothing addressed)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K2 = 2 * nb, n = nb * K2, M = nb + K2;
  const bool heur_old = heur[b] != 0;
  const float div = len_div[c];
  const bool last = c + 1 >= L;
  for (int i = tid; i < n; i += 256) sv[i] = val[(size_t)b * n + i];
  if (tid < K2) top_i[tid] = 0;
  if (tid < nb) { nxt[tid] = 0; mi[tid] = 0; }
  __syncthreads();
  // the K2 best of the nb K2 candidates
  for (int i = tid; i < n; i += 256) {
    const float vi = sv[i];
    int r = 0;
    for (int j = 0; j < n && r < K2; ++j) r += before(sv[j], j, vi, i) ? 1 : 0;
    if (r < K2) top_i[r] = i;
  }
  __syncthreads();
  if (tid < K2) {
    const int i = top_i[tid];
    const float tv = sv[i];
    const long long tk = (long long)tok[(size_t)b * n + i];
    const bool hit = tk == eos || last;
    const bool did = hit && tid < nb;             // only a candidate among the first nb may be kept
    t_val[tid] = tv;
    t_tok[tid] = tk;
    t_src[tid] = i / K2;
    t_hit[tid] = hit ? 1 : 0;
    t_did[tid] = did ? 1 : 0;
    t_lp[tid] = tv + (hit ? 1.0f : 0.0f) * -1.0e9f;
    float fl = tv / div;
    fl = fl + (heur_old ? 0.0f : 1.0f) * -1.0e9f;
    fl = fl + (did ? 0.0f : 1.0f) * -1.0e9f;
    m_sc[nb + tid] = fl;
  }
  if (tid < nb) {
    m_sc[tid] = fin_scores[(size_t)b * nb + tid];
    o_len[tid] = fin_len[(size_t)b * nb + tid];
    o_fin[tid] = is_fin[(size_t)b * nb + tid] != 0 ? 1 : 0;
  }
  __syncthreads();
  if (tid < K2) {                                 // the running beams: the nb best that did not just end
    const float vi = t_lp[tid];
    int r = 0;
    for (int j = 0; j < K2; ++j) r += before(t_lp[j], j, vi, tid) ? 1 : 0;
    if (r < nb) nxt[r] = tid;
  }
  if (tid < M) {                                  // the kept hypotheses: the nb best of old | new
    const float vi = m_sc[tid];
    int r = 0;
    for (int j = 0; j < M; ++j) r += before(m_sc[j], j, vi, tid) ? 1 : 0;
    if (r < nb) mi[r] = tid;
  }
  __syncthreads();
  if (tid < nb) {
    const size_t o = (size_t)b * nb + tid;
    const int k = nxt[tid], q = mi[tid];
    run_scores[o] = t_lp[k];
    next_tok[o] = t_tok[k];
    beam_idx[o] = b * nb + t_src[k];
    fin_scores[o] = m_sc[q];
    fin_len[o] = q < nb ? o_len[q] : (long long)(c + 1);
    const int f = q < nb ? o_fin[q] : t_did[q - nb];
    is_fin[o] = (unsigned char)f;
    n_fs[tid] = m_sc[q];
    n_fin[tid] = f;
  }
  // the sequences, in place: column t of the new rows is a gather over the old rows of column t alone, so whole
  // columns are read into registers, a barrier, and written back -- columns 0 .. c (every later one is pad in every row)
  const int cpc = 256 / nb;                       // columns a pass
  const int j = tid % nb, dc = tid / nb;
  const bool mine = dc < cpc;
  const int kr = nxt[j], qf = mi[j];
  long long *rs = run_seq + (size_t)b * nb * L, *fs = fin_seq + (size_t)b * nb * L;
  for (int c0 = 0; c0 <= c; c0 += cpc) {
    const int t = c0 + dc;
    const bool on = mine && t <= c;
    long long rv = 0, fv = 0;
    if (on) {
      rv = t < c ? rs[(size_t)t_src[kr] * L + t] : t_tok[kr];
      if (qf < nb) fv = fs[(size_t)qf * L + t];
      else fv = t < c ? rs[(size_t)t_src[qf - nb] * L + t] : t_tok[qf - nb];
    }
    __syncthreads();
    if (on) {
      rs[(size_t)j * L + t] = rv;
      fs[(size_t)j * L + t] = fv;
    }
  }
  __syncthreads();
  if (tid == 0) {
    // can a running beam still beat the worst kept hypothesis?
    float worst = n_fs[0];
    for (int i = 1; i < nb; ++i) worst = n_fs[i] < worst ? n_fs[i] : worst;
    const float best = t_lp[nxt[0]] / div;
    bool any = false, all_hit = true;
    for (int i = 0; i < nb; ++i) any = any || best > (n_fin[i] ? worst : -1.0e9f);
    for (int i = 0; i < K2; ++i) all_hit = all_hit && t_hit[i] != 0;
    const bool h = heur_old && any;
    heur[b] = h ? 1 : 0;
    work[b] = (h ? 1 : 0) | (all_hit ? 2 : 0);
  }
}

// After every prompt's workgroup: done = no prompt can improve, or every candidate ended; one more token is written.
__global__ __launch_bounds__(64) void beam_close_kernel(int B, int N, const int *__restrict__ work, int *cur_p, int *done_p,
                                                        int *n_prev) {
  if (*done_p != 0) return;
  const int c = *cur_p;
  int any_heur = 0, all_hit = 1;
  for (int b = threadIdx.x; b < B; b += 64) {
    const int w = work[b];
    any_heur |= w & 1;
    all_hit &= (w >> 1) & 1;
  }
  any_heur = __any(any_heur);
  all_hit = __all(all_hit);
  if (n_prev)
    for (int i = threadIdx.x; i < N; i += 64) n_prev[i] = c + 1;
  if (threadIdx.x == 0) {
    *cur_p = c + 1;
    *done_p = (any_heur && !all_hit) ? 0 : 1;
  }
}

// One workgroup for all N rows.
__global__ __launch_bounds__(256) void greedy_advance_kernel(int N, int L, const int *__restrict__ tok, int ld_tok,
                                                             long long eos, long long pad, long long *seq,
                                                             unsigned char *unfinished, int *cur_p, int *done_p,
                                                             long long *next_tok, int *n_prev) {
  if (*done_p != 0) return;
  const int c = *cur_p;
  if (c < 0 || c >= L) return;
  int live = 0;
  for (int n = threadIdx.x; n < N; n += 256) {
    const bool u = unfinished[n] != 0;
    const long long t = u ? (long long)tok[(size_t)n * ld_tok] : pad;
    seq[(size_t)n * L + c] = t;
    next_tok[n] = t;
    const bool u2 = u && t != eos;
    unfinished[n] = u2 ? 1 : 0;
    if (n_prev) n_prev[n] = c + 1;
    live |= u2 ? 1 : 0;
  }
  live = __syncthreads_or(live);                  // (every thread has read cur and done by here)
  if (threadIdx.x == 0) {
    *cur_p = c + 1;
    *done_p = (c + 1 >= L || !live) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

int msr3d_beam_advance(int B, int nb, int L, const float *val, const int *tok, int eos_id, const float *len_div,
                       float *run_scores, long long *run_seq, long long *fin_seq, float *fin_scores, long long *fin_len,
                       unsigned char *is_fin, unsigned char *heur, int *cur, int *done, long long *next_tok, int *beam_idx,
                       int *n_prev, int *work, msr3d_stream_t stream) {
  if (B < 0 || nb < 1 || nb > MAX_NB || 2 * nb > MAX_K2 || L < 1) return MSR3D_EINVAL;
  if (B == 0) return 0;
  if (B > 65535 || !val || !tok || !len_div || !run_scores || !run_seq || !fin_seq || !fin_scores || !fin_len || !is_fin ||
      !heur || !cur || !done || !next_tok || !beam_idx || !work || run_seq == fin_seq)
    return MSR3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  beam_advance_kernel<<<B, 256, 0, st>>>(nb, L, val, tok, (long long)eos_id, len_div, run_scores, run_seq, fin_seq,
                                         fin_scores, fin_len, is_fin, heur, cur, done, next_tok, beam_idx, work);
  beam_close_kernel<<<1, 64, 0, st>>>(B, B * nb, work, cur, done, n_prev);
  return (int)hipGetLastError();
}

int msr3d_greedy_advance(int N, int L, const int *tok, int ld_tok, int eos_id, long long pad_id, long long *seq,
                         unsigned char *unfinished, int *cur, int *done, long long *next_tok, int *n_prev,
                         msr3d_stream_t stream) {
  if (N < 0 || L < 1 || ld_tok < 1) return MSR3D_EINVAL;
  if (N == 0) return 0;
  if (!tok || !seq || !unfinished || !cur || !done || !next_tok) return MSR3D_EINVAL;
  greedy_advance_kernel<<<1, 256, 0, (hipStream_t)stream>>>(N, L, tok, ld_tok, (long long)eos_id, pad_id, seq, unfinished,
                                                            cur, done, next_tok, n_prev);
  return (int)hipGetLastError();
}

}  // extern "C"
