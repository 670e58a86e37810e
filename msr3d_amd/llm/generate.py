"""`generate` for the LoRA-Llama stack: greedy and beam search, sampling and beam sampling over a key / value cache, one
new token per step on the decode kernels of csrc/llm_decode.hip and the draw kernel of csrc/llm_sample.hip (what
transformers' `LlamaForCausalLM.generate(inputs_embeds=..., attention_mask=..., do_sample=..., top_p=..., temperature=...,
num_beams=..., repetition_penalty=..., length_penalty=..., num_return_sequences=...)` computes; the reference's
MSR3D.generate calls exactly that).

Sampling is stated once in torch: `torch_sample_scores` (the processors, temperature, top-k, top-p with ties at the cut
ordered by token id, then log-softmax or the beam score) gives the scores w a token is drawn from, `torch_sample` draws by
Gumbel keys (the k largest w + noise = k draws without replacement), `counter_uniform_bits` is the noise's counter hash in
integers.  `CachedDecoder.sample` is all of it as one kernel (msr3d_decode_sample); `search(draw="multinomial")` draws with
torch.multinomial instead, where transformers does, which pins `search` to transformers on the CPU.

Four pieces:

* `KVCache`        the buffers of one call: K / V (layers, 2, rows, t_max, heads, head_dim) bf16, token-major like the
                   projections' own output, twice when beams are reordered (ping-pong), and per row `len` (cache slots in
                   use), `pos` (the next rotary position = number of unmasked tokens so far) and `keep` (key padding).
                   Allocated once per call, never resized.  layout "shared" (`prompt_cache="shared"`): the prompt's K / V
                   once per PROMPT (layers, 2, prompts, T, heads, head_dim), never reordered, and only the generated
                   tails per row -- the beams of a prompt read one copy (msr3d_attn_decode_shared), the same bits.
* `CachedDecoder`  the engine: `prefill` runs the existing layer forward kernels over the padded prompt (positions =
                   cumsum(mask) - 1, clamped at 0: what transformers' generate feeds Llama when it is given a mask) and
                   writes every layer's K / V into the cache; `step` runs one token per live row: per layer RMSNorm,
                   q | k | v as ONE skinny launch, rotation + cache append, decode attention, o, RMSNorm, gate | up with the
                   SwiGLU epilogue, down; then the final norm and the head.  No host synchronisation inside `step`: lengths
                   and positions live in device memory.  Up to `max_rows` = 64 live rows (batch x beams).
                   `lora="merged"`: the same walks on the stack's merged planes bf16(W + s B A) (one msr3d_lora_merge
                   launch per weight version): every product is its R = 0 form and the r-row launches are gone.
                   `weights="e4m3"`: a base="fp8" stack on its own e4m3 weights (csrc/llm_decode_fp8.hip): the same
                   launches, the step's projections at half the weight bytes.
* `search`         greedy / beam search and sampling with transformers' semantics, written against the engine interface alone
                   (`reserve`, `prefill`, `expand`, `step`, and optionally `select` and `sample`), so it runs on the CPU with any
                   engine: that is how its logic is checked exactly against transformers.  A batch with more live rows
                   than `engine.max_rows` runs as `prompt_groups` of whole prompts, one group after another.
* `rank_answers`   closed-set answer ranking (the reference's MSR3D.predict_answers): the prompt is prefilled ONCE per
                   row (`prefill(positions="arange")`: the positions of the full forward), the candidate answers run
                   through `CachedDecoder.score` as B x C short suffixes that attend to that one cached prefix
                   (msr3d_attn_prefix_fwd, csrc/llm_attn.hip) instead of C copies of prompt + answer through the full
                   forward.  Written against the engine interface alone (`prefill`, `score`), like `search`.

`max_length` counts GENERATED tokens (the prompt travels as embeddings and has no ids).  GPU only for the engine."""
import ctypes
import math

import torch

from .. import _lib
from .._lib import call, current_stream_ptr, ptr
from .decoder import MergedModuleProducts, ModuleProducts, _AttentionFn, decoder_stack, rope_tables
from .lora import PAD_R, LoRALinear, _skinny, refresh_shadows


def _append_bos(embed_fn, x, mask, bos_id):
    """The embedding of bos_id and a mask column of ones appended to every prompt."""
    bos = embed_fn(torch.full((x.shape[0],), int(bos_id), dtype=torch.int64, device=x.device)).to(x.dtype)
    return torch.cat([x, bos[:, None]], 1), torch.cat([mask, torch.ones_like(mask[:, :1])], 1)


def _pad_tokens(x, keep, n):
    """x (..., t, hidden), keep (..., t) bool -> both with n token slots: the n - t appended ones are zero and masked."""
    t = keep.shape[-1]
    if n == t:
        return x, keep
    return (torch.cat([x, x.new_zeros((*x.shape[:-2], n - t, x.shape[-1]))], -2),
            torch.cat([keep, keep.new_zeros((*keep.shape[:-1], n - t))], -1))


def _embed_fn(embed_tokens):
    """embed_tokens: the (V, hidden) table, or already a callable ids -> embeddings."""
    return embed_tokens if callable(embed_tokens) else (lambda ids: torch.nn.functional.embedding(ids, embed_tokens))


# ------------------------------------------------------------------------------------------------ selection, in torch
def torch_select(logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, k):
    """The fp32 statement of msr3d_decode_select, device-agnostic: per row the top k (value, token) of
    order 0: log_softmax(processors(logits)) + beam_score;  order 1: processors(log_softmax(logits)) + beam_score,
    processors = transformers' RepetitionPenaltyLogitsProcessor over prev (N, n_prev) then MinLengthLogitsProcessor."""
    x = logits.float()
    if order == 0:
        s = torch.log_softmax(_processors(x, prev, repetition_penalty, min_length, eos_id), dim=-1)
    else:
        s = _processors(torch.log_softmax(x, dim=-1), prev, repetition_penalty, min_length, eos_id)
    if beam_score is not None:
        s = s + beam_score.float()[:, None]
    val, tok = torch.topk(s, k, dim=-1)
    return val, tok


def _processors(s, prev, repetition_penalty, min_length, eos_id):
    """transformers' RepetitionPenaltyLogitsProcessor over prev (N, n_prev), then MinLengthLogitsProcessor."""
    if repetition_penalty != 1.0 and prev.shape[1] > 0:
        g = torch.gather(s, 1, prev)
        g = torch.where(g < 0, g * repetition_penalty, g / repetition_penalty)
        s = s.scatter(1, prev, g)
    if prev.shape[1] < min_length and eos_id is not None and eos_id >= 0:
        s = s.clone()
        s[:, eos_id] = -math.inf
    return s


# ------------------------------------------------------------------------------------------------- sampling, in torch
def torch_sample_scores(logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, temperature, top_k, top_p,
                        min_keep):
    """-> w (N, V): the scores a token is drawn from, P(token) ~ exp(w); the statement of msr3d_decode_sample before its
    noise.  torch_select's processor chain, then transformers' warpers in transformers' order:
      s = processors(logits) (order 0) or processors(log_softmax(logits)) (order 1); beam_score not yet added
      s / temperature                                                                     (TemperatureLogitsWarper)
      top_k (0 or >= V: off): s < the max(top_k, min_keep)-th largest value -> -inf; ties at that value all stay
      top_p (>= 1: off): in ascending order, every entry whose cumulative softmax is <= 1 - top_p -> -inf, except the
        last min_keep (TopPLogitsWarper).  EQUAL SCORES ARE ORDERED BY TOKEN ID, as a stable ascending sort orders
        them: the lower id is removed first and min_keep protects the higher ids.  (bf16 logits tie all the time; a
        sort that breaks ties any other way gives another kept set.)  The threshold is written as transformers writes
        it, `cum <= 1 - top_p` on the Python float; msr3d_decode_sample receives top_p as fp32 and compares with
        1 - fp32(top_p) (0.10000002 for 0.9), 2e-8 away -- below what an fp32 cumulative sum resolves.
      order 0: w = log_softmax(filtered);  order 1: w = filtered + beam_score[:, None] -- not renormalised: a prompt's
        beams x V entries share ONE softmax, which is what transformers' `_beam_search` hands to its multinomial.
    fp32, or float64 when the logits are (the tests' statement)."""
    x = logits if logits.dtype == torch.float64 else logits.float()
    if order == 0:
        s = _processors(x, prev, repetition_penalty, min_length, eos_id)
    else:
        s = _processors(torch.log_softmax(x, dim=-1), prev, repetition_penalty, min_length, eos_id)
    s = s / temperature
    V = s.shape[1]
    kk = max(int(top_k), int(min_keep))
    if top_k > 0 and kk < V:
        s = s.masked_fill(s < torch.topk(s, kk, dim=-1)[0][:, -1:], -math.inf)
    if top_p < 1.0:
        ss, idx = torch.sort(s, dim=-1, descending=False, stable=True)
        gone = ss.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        gone[:, -int(min_keep):] = False
        s = s.masked_fill(gone.scatter(1, idx, gone), -math.inf)
    if order == 0:
        return torch.log_softmax(s, dim=-1)
    return s if beam_score is None else s + beam_score.to(s.dtype)[:, None]


_M32 = 0xFFFFFFFF


def _mix32(x):
    """A 32-bit integer mixer on values held in int64 (a tensor or an int): csrc/llm_sample.hip::mix32."""
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & _M32
    return x ^ (x >> 16)


def counter_uniform_bits(seed, step, row0, N, V):
    """-> (N, V) int64 on the CPU, values in [0, 2^24): the counter hash of (seed, step, global row row0 + n, token v)
    msr3d_decode_sample draws from, restated exactly in integers.  A pure function: no state, any N.
    u = (bits + 0.5) 2^-24 is never 0 or 1."""
    seed, step, row0 = int(seed), int(step), int(row0)
    if seed < 0 or seed >= 1 << 63 or step < 0 or row0 < 0:
        raise ValueError("counter_uniform_bits: 0 <= seed < 2^63, step >= 0, row0 >= 0")
    lo, hi = seed & _M32, seed >> 32
    rows = (row0 + torch.arange(int(N), dtype=torch.int64)) & _M32
    a = _mix32(_mix32(_mix32(lo) ^ (step & _M32)) ^ rows)
    b = _mix32(_mix32((_mix32(hi ^ 0x85ebca6b) + rows) & _M32) ^ (step & _M32))
    tok = torch.arange(int(V), dtype=torch.int64)
    return _mix32((_mix32(tok[None] ^ a[:, None]) + b[:, None]) & _M32) >> 8


def gumbel_from_bits(bits):
    """-> float64 -log(-log u), u = (bits + 0.5) 2^-24."""
    return -torch.log(-torch.log((bits.double() + 0.5) * 2.0 ** -24))


def torch_sample(w, k, noise):
    """w, noise (N, V) -> key, val (N, k) and tok (N, k) int64: per row the k largest key = w + noise in descending
    order, ties to the lower token id; val = w at those tokens.  Gumbel noise makes them k successive draws without
    replacement from softmax(w).  A row with fewer than k finite keys: key = val = -inf, tok = -1 in the rest."""
    key = w + noise.to(w.dtype)
    sk, tok = torch.sort(key, dim=-1, descending=True, stable=True)
    sk, tok = sk[:, :k].contiguous(), tok[:, :k].contiguous()
    if sk.shape[1] < k:
        sk = torch.nn.functional.pad(sk, (0, k - sk.shape[1]), value=-math.inf)
        tok = torch.nn.functional.pad(tok, (0, k - tok.shape[1]), value=0)
    val = torch.gather(w, 1, tok)
    none = sk == -math.inf
    return sk, val.masked_fill(none, -math.inf), tok.masked_fill(none, -1)


# ----------------------------------------------------------------------------------------------------------- search
def prompt_groups(B, rows_per_prompt, max_rows):
    """-> [(start, stop), ...]: B prompts of `rows_per_prompt` live rows each as contiguous ranges of whole prompts, the
    fewest for which every range has at most `max_rows` rows, sizes differing by at most one, the larger ones first."""
    B, per, cap = int(B), int(rows_per_prompt), int(max_rows)
    if per < 1 or per > cap:
        raise ValueError(f"prompt_groups: {per} rows per prompt do not fit {cap} live rows")
    if B <= 0:
        return []
    groups = -(-B // (cap // per))
    small, extra = divmod(B, groups)
    out, start = [], 0
    for g in range(groups):
        stop = start + small + (1 if g < extra else 0)
        out.append((start, stop))
        start = stop
    return out


@torch.no_grad()
def search(engine, embed_fn, inputs_embeds, attention_mask, bos_id=None, eos_id=2, pad_id=2, num_beams=1, max_length=256,
           min_length=1, repetition_penalty=1.0, length_penalty=1.0, do_sample=False, top_p=1.0, top_k=0, temperature=1.0,
           num_return_sequences=1, seed=None, draw=None):
    """-> (B n, <= max_length) int64, n = num_return_sequences, a prompt's rows adjacent: the generated tokens (the
    prompt is not part of the result).
    engine: `prefill(inputs_embeds (B, T, H), attention_mask (B, T)) -> (B, V)` logits of the last position,
    `expand(beams)` (every prompt row becomes `beams` adjacent rows), `step(embeds (N, H), beam_idx=None) -> (N, V)`
    (beam_idx (N,): row n continues the cache of row beam_idx[n]); optionally `reserve(rows_per_prompt, new_tokens)`
    called first and `select(...)` with torch_select's signature, and `max_rows`: the most live rows (B x num_beams)
    the engine takes at once -- a larger batch runs as `prompt_groups` of whole prompts one after another, each with its
    own reserve / prefill / expand, the results concatenated and padded with pad_id to the longest (the one-call
    result: a prompt's tokens depend on no other prompt).  embed_fn: token ids (N,) -> embeddings (N, H).
    bos_id: its embedding and a mask column of ones are appended to the prompt first (the reference's generate does that
    itself).  Semantics are transformers' (`do_sample=False`, `early_stopping=False`): greedy rows that have emitted eos
    go on as pad_id; beam search keeps 2 x beams candidates a step, scores finished hypotheses
    sum_logprobs / len ** length_penalty and stops when no running beam can beat the worst kept hypothesis.
    One host synchronisation per step (the done test), as transformers has.

    num_return_sequences = n <= num_beams without sampling: the n best finished hypotheses of every prompt.
    do_sample (transformers' `do_sample=True`; temperature, top_k (0 = off), top_p as `torch_sample_scores` states them):
      num_beams == 1: every prompt is prefilled once and becomes n adjacent rows; each step draws one token per row
        (order 0, min_keep 1); finished rows go on as pad_id.
      num_beams > 1 (beam sampling): a step's 2 x beams candidates of a prompt are a draw WITHOUT replacement from the
        joint softmax over its beams x V entries of w (order 1, min_keep 2), kept in draw order -- the rest of the loop
        reads positions exactly as in beam search.  A drawn candidate without probability (the nucleus of the only live
        beam holds fewer than 2 x beams tokens; transformers' multinomial raises there) raises ValueError.
    draw = "multinomial" (the default for an engine without `sample`): torch.multinomial on softmax(w) from torch's
      global generator, exactly where transformers calls it -- what pins this function to transformers on the CPU.
    draw = "counter" (the default for an engine with `sample`): key = w + Gumbel noise, a draw is the arg-max of the
      keys and k draws without replacement are the k largest keys in that order (per row, then across a prompt's
      beams) -- the same distribution.  The noise is a counter hash of (seed, step, global live row, token id)
      (`counter_uniform_bits`), global live row = prompt index x rows per prompt + r: a prompt's tokens do not depend
      on how `prompt_groups` cut the batch.  `engine.sample(logits, prev, repetition_penalty, min_length, eos_id,
      beam_score, order, temperature, top_k, top_p, min_keep, k, seed, step, row0) -> (key, val, tok)` draws (one
      kernel on the GPU); without it `torch_sample_scores` + `torch_sample` do.  seed = None takes 63 bits from torch's
      CPU generator: torch.manual_seed makes a call reproducible.
    Live rows per prompt are max(num_beams, n)."""
    nb, n_ret, L = int(num_beams), int(num_return_sequences), int(max_length)
    if nb < 1 or L < 1:
        raise ValueError("num_beams >= 1 and max_length >= 1")
    if n_ret < 1 or (n_ret > 1 and nb == 1 and not do_sample):
        raise ValueError("num_return_sequences > 1 needs beams or sampling (greedy search has one result)")
    if nb > 1 and n_ret > nb:
        raise ValueError("num_return_sequences must not exceed num_beams")
    if not 0.0 < top_p <= 1.0:
        raise ValueError("top_p in (0, 1]")
    if not temperature > 0.0:
        raise ValueError("temperature > 0")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError("top_k >= 0 (0 = off)")
    if draw is None:
        draw = "counter" if hasattr(engine, "sample") else "multinomial"
    if draw not in ("counter", "multinomial"):
        raise ValueError("draw is 'counter' or 'multinomial'")
    if do_sample and draw == "counter" and seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    per = max(nb, n_ret)                                   # live rows per prompt
    x, mask = inputs_embeds, attention_mask
    max_rows = getattr(engine, "max_rows", None)
    if max_rows is not None and x.shape[0] * per > max_rows:
        # more live rows than the engine takes at once: whole prompts in groups, one after another on the same engine.
        # A prompt's tokens depend on no other prompt (the counter draw is told the group's first global row) and
        # finished rows are already padded with pad_id, so this is the one-call result.
        groups = prompt_groups(x.shape[0], per, int(max_rows))
    else:
        groups = [(0, x.shape[0])]
    sampler = None
    if do_sample:
        sampler = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), draw=draw, seed=seed)
    outs = [_search_group(engine, embed_fn, x[a:b], mask[a:b], bos_id, eos_id, pad_id, nb, L, min_length, repetition_penalty,
                          length_penalty, n_ret, sampler, a * per) for a, b in groups]
    if len(outs) == 1:
        return outs[0]
    width = max(o.shape[1] for o in outs)
    return torch.cat([torch.nn.functional.pad(o, (0, width - o.shape[1]), value=int(pad_id)) for o in outs], 0)


def _sample_rows(engine, sampler, logits, prev, repetition_penalty, min_length, eos, beam_score, order, min_keep, k, step,
                 row0):
    """The counter draw of one step: per live row the k largest keys -> (key, val, tok) (N, k)."""
    t, tk, tp, seed = sampler["temperature"], sampler["top_k"], sampler["top_p"], sampler["seed"]
    if hasattr(engine, "sample"):
        return engine.sample(logits, prev, repetition_penalty, min_length, eos, beam_score, order, t, tk, tp, min_keep, k,
                             seed, step, row0)
    w = torch_sample_scores(logits, prev, repetition_penalty, min_length, eos, beam_score, order, t, tk, tp, min_keep)
    bits = counter_uniform_bits(seed, step, row0, w.shape[0], w.shape[1])
    return torch_sample(w, k, gumbel_from_bits(bits).to(w.device))


def _search_group(engine, embed_fn, x, mask, bos_id, eos_id, pad_id, nb, L, min_length, repetition_penalty, length_penalty,
                  n_ret, sampler, row0):
    """`search` for one group of whole prompts that fits the engine; row0: the global index of its first live row."""
    dev = x.device
    if bos_id is not None:
        x, mask = _append_bos(embed_fn, x, mask, bos_id)
    B, per = x.shape[0], max(nb, n_ret)
    if hasattr(engine, "reserve"):
        engine.reserve(per, L)
    select = getattr(engine, "select", torch_select)
    logits = engine.prefill(x, mask)
    engine.expand(per)
    eos = -1 if eos_id is None else int(eos_id)

    if nb == 1:
        B = B * per                                        # sampling: a prompt's n rows are rows of their own from here
        logits = logits.repeat_interleave(per, 0) if per > 1 else logits
        seq = torch.full((B, L), int(pad_id), dtype=torch.int64, device=dev)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        for cur in range(L):
            if sampler is None:
                _, tok = select(logits, seq[:, :cur], repetition_penalty, min_length, eos, None, 0, 1)
            elif sampler["draw"] == "counter":
                _, _, tok = _sample_rows(engine, sampler, logits, seq[:, :cur], repetition_penalty, min_length, eos, None, 0,
                                         1, 1, cur, row0)
            else:
                w = torch_sample_scores(logits, seq[:, :cur], repetition_penalty, min_length, eos, None, 0,
                                        sampler["temperature"], sampler["top_k"], sampler["top_p"], 1)
                tok = torch.multinomial(torch.softmax(w, dim=-1), num_samples=1)
            nxt = torch.where(unfinished, tok[:, 0].long(), torch.full_like(tok[:, 0].long(), int(pad_id)))
            seq[:, cur] = nxt
            unfinished = unfinished & (nxt != eos)
            if cur + 1 >= L or not bool(unfinished.any()):
                break
            logits = engine.step(embed_fn(nxt))
        return seq[:, :cur + 1]

    K2 = 2 * nb
    f32 = torch.float32
    run_scores = torch.zeros((B, nb), dtype=f32, device=dev)
    run_scores[:, 1:] = -1.0e9
    run_seq = torch.full((B, nb, L), int(pad_id), dtype=torch.int64, device=dev)
    fin_seq = run_seq.clone()
    fin_scores = torch.full((B, nb), -1.0e9, dtype=f32, device=dev)
    fin_len = torch.zeros((B, nb), dtype=torch.int64, device=dev)
    is_fin = torch.zeros((B, nb), dtype=torch.bool, device=dev)
    heur = torch.ones((B, 1), dtype=torch.bool, device=dev)
    top_mask = torch.arange(K2, device=dev) < nb
    offs = (torch.arange(B, device=dev) * nb)[:, None]
    logits = logits.repeat_interleave(nb, 0)

    def take(t, i):                       # t (B, n, ...), i (B, m) -> (B, m, ...)
        return torch.gather(t, 1, i.view(*i.shape, *([1] * (t.dim() - 2))).expand(*i.shape, *t.shape[2:]))

    for cur in range(L):
        prev = run_seq.view(B * nb, L)[:, :cur]
        if sampler is None:
            val, tok = select(logits, prev, repetition_penalty, min_length, eos, run_scores.view(-1), 1, K2)
            top_val, top_i = torch.topk(val.view(B, nb * K2).float(), K2, dim=1)
            src_beam = top_i // K2
            tok_k = torch.gather(tok.view(B, nb * K2).long(), 1, top_i)
        elif sampler["draw"] == "counter":
            # each row's K2 largest keys, then the K2 largest across the prompt's beams: the K2 largest of beams x V,
            # in draw order (ties to the lower beam, then the lower token, as one arg-max over beams x V has them)
            key, val, tok = _sample_rows(engine, sampler, logits, prev, repetition_penalty, min_length, eos,
                                         run_scores.view(-1), 1, 2, K2, cur, row0)
            top_i = torch.sort(key.reshape(B, nb * K2).float(), dim=1, descending=True, stable=True)[1][:, :K2]
            top_val = torch.gather(val.reshape(B, nb * K2).float(), 1, top_i)
            src_beam = top_i // K2
            tok_k = torch.gather(tok.reshape(B, nb * K2).long(), 1, top_i)
        else:
            w = torch_sample_scores(logits, prev, repetition_penalty, min_length, eos, run_scores.view(-1), 1,
                                    sampler["temperature"], sampler["top_k"], sampler["top_p"], 2)
            V = w.shape[1]
            w = w.view(B, nb * V)
            try:
                top_i = torch.multinomial(torch.softmax(w, dim=-1), num_samples=K2)
            except RuntimeError as e:
                # fewer than K2 entries with probability: the CPU multinomial refuses itself (on the GPU it returns
                # entries without probability, which `no_mass` below catches)
                raise ValueError("search: fewer than 2 x num_beams tokens are left to the live beams after top_k / top_p "
                                 f"(torch.multinomial: {e}); widen them or use fewer beams") from e
            top_val = torch.gather(w, 1, top_i)
            src_beam, tok_k = top_i // V, top_i % V
        # (sampling: a drawn candidate without probability -- see the docstring; read with the done test below)
        no_mass = (top_val <= -1.0e8).any() if sampler is not None else None
        top_seq = take(run_seq, src_beam)
        top_seq[:, :, cur] = tok_k
        hits = tok_k == eos
        if cur + 1 >= L:
            hits = torch.ones_like(hits)
        # the running beams of the next step: the best candidates that did not just end
        run_lp = top_val + hits.to(f32) * -1.0e9
        nxt_i = torch.topk(run_lp, nb, dim=1)[1]
        run_seq, run_scores, beam_sel = take(top_seq, nxt_i), take(run_lp, nxt_i), take(src_beam, nxt_i)
        # finished hypotheses: only a candidate among the first `beams` may be kept
        did = hits & top_mask[None]
        fl = top_val / ((cur + 1) ** length_penalty)
        fl = fl + (~heur).to(f32) * -1.0e9
        fl = fl + (~did).to(f32) * -1.0e9
        m_scores = torch.cat([fin_scores, fl], 1)
        mi = torch.topk(m_scores, nb, dim=1)[1]
        fin_seq = take(torch.cat([fin_seq, top_seq], 1), mi)
        fin_len = take(torch.cat([fin_len, torch.full_like(tok_k, cur + 1)], 1), mi)
        is_fin = take(torch.cat([is_fin, did], 1), mi)
        fin_scores = take(m_scores, mi)
        # can a running beam still beat the worst kept hypothesis?  (early_stopping = False: judged at the current length)
        best_running = run_scores[:, :1] / ((cur + 1) ** length_penalty)
        worst_fin = torch.where(is_fin, fin_scores.min(1, keepdim=True)[0], torch.full_like(fin_scores, -1.0e9))
        heur = heur & (best_running > worst_fin).any(-1, keepdim=True)
        go_on = heur.any() & ~hits.all()
        if sampler is not None:
            go_on, no_mass = torch.stack([go_on, no_mass]).tolist()        # one synchronisation for both
            if no_mass:
                raise ValueError("search: a step drew a candidate without probability -- fewer than 2 x num_beams tokens "
                                 "are left to the live beams after top_k / top_p; widen them or use fewer beams")
        if not bool(go_on):
            break
        logits = engine.step(embed_fn(run_seq[:, :, cur].reshape(-1)), (beam_sel + offs).reshape(-1))
    if n_ret == 1:
        return fin_seq[:, 0, :int(fin_len[:, 0].max())]
    return fin_seq[:, :n_ret, :int(fin_len[:, :n_ret].max())].reshape(B * n_ret, -1)


# ---------------------------------------------------------------------------------------------------- answer ranking
@torch.no_grad()
def rank_answers(engine, embed_fn, inputs_embeds, attention_mask, answer_ids, answer_mask, num_ans_candidates=128,
                 bos_id=None):
    """Closed-set answer ranking, the reference's MSR3D.predict_answers step for step, on ONE cached copy of each prompt.
    engine: `prefill(inputs_embeds (B, T, H), attention_mask (B, T), positions="arange") -> (B, V)` logits of the last
    position and `score(token_embeds (B, C, S, H), token_keep (B, C, S)) -> (B, C, S, V)` logits after each suffix token.
    answer_ids (A, S) int64 right-padded, answer_mask (A, S); every answer starts with the same token (bos), which is the
    LAST slot of the cached prompt: with `bos_id` given it is appended here (its embedding and a mask column of ones),
    without it the prompt must already end with it.
    1. p = softmax(prefill logits); first_prob = p[:, answer_ids[:, 1]]; the C = min(num_ans_candidates, A) most
       probable answers of every prompt -> topk_ids (B, C);
    2. loss[b, c] = the mean over the real tokens a_1 .. of candidate c of the cross-entropy of predicting each from its
       predecessor (a_1 from the prefill logits, the others from `score`), fp32 log-sum-exp;
    3. answers_id[b] = topk_ids[b, argmin_c loss[b, c]].
    -> dict(answers_id (B,), topk_ids (B, C) int64, loss (B, C) fp32, first_prob (B, A) fp32)."""
    from .losses import seq_mean_cross_entropy
    x, mask = inputs_embeds, attention_mask
    dev = x.device
    ids = answer_ids.to(dev).long()
    am = answer_mask.to(dev).bool()
    if ids.dim() != 2 or ids.shape != am.shape or ids.shape[1] < 2 or ids.shape[0] < 1:
        raise ValueError("rank_answers: answer_ids / answer_mask (A, S) with S >= 2 (bos + at least one token)")
    first = int(ids[0, 0])
    if not bool((ids[:, 0] == first).all()) or (bos_id is not None and first != int(bos_id)):
        raise ValueError("rank_answers: every answer must start with the same token (bos)")
    if not bool(am[:, 1].all()):
        raise ValueError("rank_answers: an answer without a real token after bos (its mean loss would be 0 / 0)")
    if bos_id is not None:
        x, mask = _append_bos(embed_fn, x, mask, first)
    B, A = x.shape[0], ids.shape[0]
    C = min(int(num_ans_candidates), A)
    if C < 1:
        raise ValueError("rank_answers: num_ans_candidates >= 1")
    if hasattr(engine, "reserve"):
        engine.reserve(1, 0)                                                      # one cache row per prompt, no new slots
    logits0 = engine.prefill(x, mask, positions="arange")                         # (B, V)
    first_prob = torch.softmax(logits0.float(), dim=1).index_select(1, ids[:, 1])  # (B, A)
    topk_ids = first_prob.topk(C, dim=1)[1]                                       # (B, C)
    suffix, keep = ids[:, 1:][topk_ids], am[:, 1:][topk_ids]                      # (B, C, S - 1)
    S = suffix.shape[2]
    emb = embed_fn(suffix.reshape(-1)).view(B, C, S, -1)
    lg = engine.score(emb, keep)                                                  # (B, C, S, V)
    V = lg.shape[-1]
    # per candidate the sequence [prefill logits, suffix logits] against the targets [-, a_1, a_2, ..]: logits[t] is read
    # against targets[t + 1], so the last suffix position's logits and targets[0] take no part
    seq = torch.cat([logits0.to(lg.dtype)[:, None, None].expand(B, C, 1, V), lg], 2).reshape(B * C, S + 1, V)
    tg = torch.where(keep, suffix, torch.full_like(suffix, -100))
    tg = torch.cat([torch.full_like(tg[:, :, :1], -100), tg], 2).reshape(B * C, S + 1)
    loss = seq_mean_cross_entropy(seq, tg).float().view(B, C)
    best = loss.argmin(dim=1)
    return dict(answers_id=topk_ids.gather(1, best[:, None])[:, 0], topk_ids=topk_ids, loss=loss, first_prob=first_prob)


# ------------------------------------------------------------------------------------------------------------ cache
class KVCache:
    """layout "rows": kv[side] (layers, 2, rows, t_max, heads, head_dim) bf16, side = `cur` is the live one (two sides only
    with `pingpong`: msr3d_kv_reorder gathers from one into the other); len, pos (rows) int32; keep (rows, t_max) uint8.

    layout "shared" (`prompts` prompts of rows / prompts adjacent rows each, `t_prompt` prompt slots): a prompt's keys
    are written once by the prefill and are the same in all of its rows for ever, so they are stored once --
    prompt_kv (layers, 2, prompts, t_prompt, heads, head_dim), one side, never reordered, with prompt_keep (prompts,
    t_prompt) -- and only the generated tail is per row: kv[side] (layers, 2, rows, t_max - t_prompt, heads, head_dim),
    ping-ponged like the rows layout's.  `len` (rows) counts TAIL slots (what msr3d_rope_kv_append and msr3d_kv_reorder
    read on the tail planes) and `tail_len` (prompts) is the same number per prompt (what msr3d_attn_decode_shared
    reads): all rows of a prompt have the same length at every step, and a reorder permutes rows within a prompt, so
    neither is reordered.  `pos` is as in the rows layout."""

    def __init__(self, layers, rows, t_max, heads, head_dim, device, pingpong=False, layout="rows", prompts=None,
                 t_prompt=None):
        if layout not in ("rows", "shared"):
            raise ValueError(f"KVCache: layout is 'rows' or 'shared', not {layout!r}")
        self.layers, self.rows, self.t_max, self.heads, self.head_dim = layers, rows, t_max, heads, head_dim
        self.layout = layout
        sides = 2 if pingpong else 1
        bf = torch.bfloat16
        mk = lambda *s, dt: [torch.zeros(s, dtype=dt, device=device) for _ in range(sides)]     # noqa: E731
        self._pos = mk(rows, dt=torch.int32)
        if layout == "rows":
            self.kv = [torch.zeros((layers, 2, rows, t_max, heads, head_dim), dtype=bf, device=device) for _ in range(sides)]
            self._len = mk(rows, dt=torch.int32)
            self._keep = [torch.ones((rows, t_max), dtype=torch.uint8, device=device) for _ in range(sides)]
        else:
            if not prompts or rows % prompts or not t_prompt or not 0 < t_prompt < t_max:
                raise ValueError("KVCache: layout='shared' takes prompts (a divisor of rows) and 0 < t_prompt < t_max")
            self.prompts, self.t_prompt, self.t_tail = int(prompts), int(t_prompt), int(t_max - t_prompt)
            self.prompt_kv = torch.zeros((layers, 2, prompts, t_prompt, heads, head_dim), dtype=bf, device=device)
            self.prompt_keep = torch.ones((prompts, t_prompt), dtype=torch.uint8, device=device)
            self.kv = [torch.zeros((layers, 2, rows, self.t_tail, heads, head_dim), dtype=bf, device=device)
                       for _ in range(sides)]
            # one buffer, so that one add_ advances both views: [rows tail lengths | prompts tail lengths]
            self._lens = torch.zeros(rows + prompts, dtype=torch.int32, device=device)
        self.cur = 0
        splits = _lib.load().msr3d_attn_decode_splits(rows, heads)
        self.workspace = (torch.empty(rows * heads * splits * (head_dim + 2), dtype=torch.float32, device=device)
                          if splits > 1 else None)

    len = property(lambda self: self._len[self.cur] if self.layout == "rows" else self._lens[:self.rows])
    pos = property(lambda self: self._pos[self.cur])
    keep = property(lambda self: self._keep[self.cur])
    tail_len = property(lambda self: self._lens[self.rows:])

    @property
    def nbytes(self):
        """The bytes of the K / V planes allocated (every side, and the prompt planes of the shared layout); the lengths,
        positions, key padding and the split workspace beside them are KB."""
        n = sum(t.numel() * t.element_size() for t in self.kv)
        return n + (self.prompt_kv.numel() * self.prompt_kv.element_size() if self.layout == "shared" else 0)

    def advance(self):
        """One more slot in use and one more position, in every row."""
        (self._len[self.cur] if self.layout == "rows" else self._lens).add_(1)
        self.pos.add_(1)

    def k(self, layer):
        return self.kv[self.cur][layer, 0]

    def v(self, layer):
        return self.kv[self.cur][layer, 1]

    def reorder(self, beam_idx):
        """Row n continues row beam_idx[n]: one launch for every layer's K and V, into the other side.  Shared layout:
        the tail planes alone, and beam_idx[n] must be a row of n's own prompt (what beam search produces)."""
        if len(self.kv) < 2:
            raise RuntimeError("KVCache: allocated without the second side (pingpong=True) a reorder needs")
        idx = beam_idx.to(torch.int32).contiguous()
        src, dst = self.kv[self.cur], self.kv[1 - self.cur]
        dev = src.device
        with torch.cuda.device(dev):
            call("msr3d_kv_reorder", self.layers * 2, self.rows, src.shape[3], self.heads * self.head_dim, ptr(src), ptr(dst),
                 ptr(idx), ptr(self.len), current_stream_ptr(dev))
        il = idx.long()
        for pair in ((self._len, self._pos, self._keep) if self.layout == "rows" else (self._pos,)):
            torch.index_select(pair[self.cur], 0, il, out=pair[1 - self.cur])
        self.cur = 1 - self.cur


# --------------------------------------------------------------------------------------- the products of a decode step
def _skinny_entry(M):
    """The weight-stream product for M live rows: up to 32 the entry every call has used so far (the same bits), the
    wide one (three or four activation tiles) for 33 .. 64."""
    return "msr3d_bf16_skinny_lowrank" if M <= 32 else "msr3d_bf16_skinny_lowrank_wide"


def _skinny_project(h, mods, swiglu, planes):
    """The projections `mods` of the same activations h (M, K) -> list of (M, N) bf16 (one tensor with swiglu), one launch
    per input group.  planes None: W and the low-rank pair side by side (the r-row product s h A^T first, R = 64);
    planes {module: bf16(W + s B A)}: the merged plane alone, R = 0 -- no r-row product, no low-rank activation."""
    M, K = h.shape
    dev = h.device
    R = PAD_R if planes is None else 0
    outs, calls = [None] * len(mods), {}
    for j, m in enumerate(mods):
        if planes is None:
            m._sync_weight_t()
        calls.setdefault(id(m._group) if m._group is not None else id(m), []).append(j)
    if swiglu and len(calls) != 1:
        # gate and up without a shared low-rank activation (modules moved to the device after construction leave
        # their input group): two products and the stand-alone SwiGLU launch
        gate, up = _skinny_project(h, mods, False, planes)
        act = torch.empty_like(gate)
        with torch.cuda.device(dev):
            call("msr3d_swiglu_fwd", gate.numel(), ptr(gate), ptr(up), ptr(act), current_stream_ptr(dev))
        return [act]
    for js in calls.values():
        u = None
        if planes is None:
            m0 = mods[js[0]]
            a_op = m0._group["a_cat"] if m0._group is not None else m0._shadows(forward=True)[0]
            u = torch.empty((M, PAD_R), dtype=torch.bfloat16, device=dev)
            _skinny(M, a_op.shape[0], K, h, a_op, u, PAD_R, m0.scaling, dev)
        jobs = (_lib.SkinnyJob * len(js))()
        for n, j in enumerate(js):
            m = mods[j]
            w = m.weight if planes is None else planes[m]
            b2 = m._shadows(forward=True)[1].data_ptr() if planes is None else 0
            if not (swiglu and n == 1):
                outs[j] = torch.empty((M, m.out_features), dtype=torch.bfloat16, device=dev)
            jobs[n] = _lib.SkinnyJob(w.data_ptr(), K, b2, R, outs[j].data_ptr() if outs[j] is not None else 0,
                                     m.out_features, m.out_features)
        with torch.cuda.device(dev):
            call(_skinny_entry(M), M, K, R, ptr(h), K, ptr(u), R, len(js), jobs, int(swiglu), current_stream_ptr(dev))
    return outs


class SkinnyProducts:
    """decoder.ModuleProducts' operations for the M <= 64 live rows of one decode step: every product streams its weight
    once (msr3d_bf16_skinny_lowrank), members of one input group share the low-rank activation and ONE launch, gate | up
    carry the SwiGLU epilogue.  No autograd, bf16 base weights."""

    @staticmethod
    def project(h, mods, swiglu=False):
        return _skinny_project(h, mods, swiglu, None)

    @staticmethod
    def gated(h, gate, up):
        return _skinny_project(h, (gate, up), True, None)[0]

    @staticmethod
    def head(h, lm_head):
        lm_head._sync()
        M, K, V = h.shape[0], lm_head.in_features, lm_head.out_features
        logits = torch.empty((M, V), dtype=torch.bfloat16, device=h.device)
        job = (_lib.SkinnyJob * 1)(_lib.SkinnyJob(lm_head.weight.data_ptr(), K, 0, 0, logits.data_ptr(), V, V))
        with torch.cuda.device(h.device):
            call(_skinny_entry(M), M, K, 0, ptr(h), K, ptr(None), 0, 1, job, 0, current_stream_ptr(h.device))
        return logits


class MergedSkinnyProducts:
    """SkinnyProducts on merged weights (lora="merged"): the same launches -- the same input groups, gate | up with the
    SwiGLU epilogue -- with R = 0 on the planes bf16(W + s B A) of LoRALlamaStack.merged_weights()."""

    def __init__(self, planes):
        self.planes = planes

    def project(self, h, mods, swiglu=False):
        return _skinny_project(h, mods, swiglu, self.planes)

    def gated(self, h, gate, up):
        return _skinny_project(h, (gate, up), True, self.planes)[0]

    head = staticmethod(SkinnyProducts.head)


# ------------------------------------------------------------------------------------------- the same on e4m3 weights
E4M3_SLAB = 64          # MSR3D_SKINNY_WIDE_MAX_M: the rows one msr3d_fp8_skinny_lowrank launch takes
E4M3_WIDE_MIN = 128     # from here up LoRALinear's own forward multiplies on e4m3 (msr3d_fp8_gemm_lowrank's domain)


def _e4m3_skinny_project(h, mods, swiglu, scratch=None):
    """_skinny_project for base="fp8" modules on their e4m3 images: per input group ONE msr3d_bf16_gemm_skinny_quant launch
    (the r-row activation u = s h A^T, the e4m3 codes of h and their row scales) and ONE msr3d_fp8_skinny_lowrank launch
    that streams weight_q / weight_scale of every member -- the launches of the bf16 step, half the weight bytes.
    h (M <= 64, K) bf16 contiguous.  scratch: a dict that keeps (u, codes, scales) per (M, K) between calls -- nothing
    reads them after the group's second launch, and the launches of an engine are ordered on one stream, so a step
    allocates its outputs alone (at a few rows a step is bounded by its host time)."""
    M, K = h.shape
    dev = h.device
    outs, calls = [None] * len(mods), {}
    for j, m in enumerate(mods):
        m._sync_weight_t()                                  # (requantises weight_q when the bf16 weight was written)
        if m.base != "fp8" or m.weight_q is None:
            raise RuntimeError("weights='e4m3': a projection without an e4m3 image (base='fp8' modules on the GPU only)")
        calls.setdefault(id(m._group) if m._group is not None else id(m), []).append(j)
    if swiglu and len(calls) != 1:
        # gate and up without a shared low-rank activation (see _skinny_project): two products and the SwiGLU launch
        gate, up = _e4m3_skinny_project(h, mods, False, scratch)
        act = torch.empty_like(gate)
        with torch.cuda.device(dev):
            call("msr3d_swiglu_fwd", gate.numel(), ptr(gate), ptr(up), ptr(act), current_stream_ptr(dev))
        return [act]
    for js in calls.values():
        m0 = mods[js[0]]
        a_op = m0._group["a_cat"] if m0._group is not None else m0._shadows(forward=True)[0]
        buf = scratch.get((M, K, dev)) if scratch is not None else None
        if buf is None:
            buf = (torch.empty((M, PAD_R), dtype=torch.bfloat16, device=dev),
                   torch.empty((M, K), dtype=torch.uint8, device=dev), torch.empty((M,), dtype=torch.float32, device=dev))
            if scratch is not None:
                scratch[(M, K, dev)] = buf
        u, hq, sh = buf
        with torch.cuda.device(dev):
            call("msr3d_bf16_gemm_skinny_quant", M, a_op.shape[0], K, ptr(h), K, ptr(a_op), K, ptr(u), PAD_R, PAD_R,
                 ctypes.c_float(m0.scaling), ptr(hq), K, ptr(sh), current_stream_ptr(dev))
        jobs = (_lib.Fp8SkinnyJob * len(js))()
        for n, j in enumerate(js):
            m = mods[j]
            if not (swiglu and n == 1):
                outs[j] = torch.empty((M, m.out_features), dtype=torch.bfloat16, device=dev)
            jobs[n] = _lib.Fp8SkinnyJob(m.weight_q.data_ptr(), K, m.weight_scale.data_ptr(),
                                        m._shadows(forward=True)[1].data_ptr(), PAD_R,
                                        outs[j].data_ptr() if outs[j] is not None else 0, m.out_features, m.out_features)
        with torch.cuda.device(dev):
            call("msr3d_fp8_skinny_lowrank", M, K, PAD_R, ptr(hq), K, ptr(sh), ptr(u), PAD_R, len(js), jobs, int(swiglu),
                 current_stream_ptr(dev))
    return outs


class E4m3SkinnyProducts:
    """SkinnyProducts for a base="fp8" stack (weights="e4m3"): the same input groups and the same launch count, every
    LoRA projection on msr3d_fp8_skinny_lowrank -- the activations quantised per row in the r-row launch, the weight read
    as e4m3 codes.  The head is a FrozenLinear without an e4m3 image and stays on the bf16 kernel.  One per engine: it
    keeps the groups' scratch tensors between steps."""

    def __init__(self):
        self.scratch = {}

    def project(self, h, mods, swiglu=False):
        return _e4m3_skinny_project(h, mods, swiglu, self.scratch)

    def gated(self, h, gate, up):
        return _e4m3_skinny_project(h, (gate, up), True, self.scratch)[0]

    head = staticmethod(SkinnyProducts.head)


class E4m3ModuleProducts:
    """ModuleProducts for an e4m3 engine's prefill and `score`: every LoRA projection multiplies on e4m3, whatever the
    number of token rows.  From 128 rows up that is the modules' own forward (msr3d_fp8_gemm_lowrank) -- the stack's
    full forward bit for bit; below, where LoRALinear falls back to its bf16 plane, the rows go through
    msr3d_fp8_skinny_lowrank in slabs of at most 64.  The two kernels add the same exact e4m3 products in different
    orders: a walk of fewer than 128 rows may differ from a larger one in last bits.  Evaluation only (no autograd)."""

    @staticmethod
    def _slabs(h, mods, swiglu):
        if torch.is_grad_enabled() and h.requires_grad:
            raise RuntimeError("E4m3ModuleProducts: evaluation only (no backward); call under torch.no_grad()")
        if not h.is_cuda:
            raise RuntimeError("LoRALinear runs on the GPU only (no CPU fallback)")
        x2 = h.to(torch.bfloat16).reshape(-1, h.shape[-1])
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        cols = None                                         # per output, its slabs in row order
        for s in range(0, x2.shape[0], E4M3_SLAB):
            part = [o for o in _e4m3_skinny_project(x2[s:s + E4M3_SLAB], mods, swiglu) if o is not None]
            cols = [[o] for o in part] if cols is None else [c + [o] for c, o in zip(cols, part)]
        return [c[0] if len(c) == 1 else torch.cat(c, 0) for c in cols]

    @classmethod
    def project(cls, h, mods):
        if h.numel() // h.shape[-1] >= E4M3_WIDE_MIN:
            return ModuleProducts.project(h, mods)
        return cls._slabs(h, mods, False)

    @classmethod
    def gated(cls, h, gate, up):
        if h.numel() // h.shape[-1] >= E4M3_WIDE_MIN:
            return ModuleProducts.gated(h, gate, up)
        return cls._slabs(h, (gate, up), True)[0]

    head = staticmethod(ModuleProducts.head)


# ----------------------------------------------------------------------------------------------------------- engine
class CachedDecoder:
    """The decoding engine of a LoRALlamaStack (see the module docstring).  At most `max_rows` live rows (batch x beams)
    per prefill; `search` splits a larger batch into groups of whole prompts.
    weights = "bf16" (default): every product reads the bf16 base weights; a base="fp8" stack is refused.
    weights = "e4m3": a stack whose projections are all base="fp8" decodes on its own e4m3 images -- what its training
    forward multiplies on: a step streams weight_q / weight_scale through msr3d_fp8_skinny_lowrank (E4m3SkinnyProducts:
    the same launch count, half the weight bytes; the head stays bf16), prefill and `score` keep every product on e4m3
    (E4m3ModuleProducts: the modules' own forward from 128 token rows up, slabs of 64 rows on the skinny kernel below).
    Those two kernels sum in different orders, so under "e4m3" a `score` chunk or a prefill below 128 rows may differ
    from a larger one in last bits: the results are NOT invariant under chunking and grouping, unlike "bf16".
    Reproducible call to call (no atomics); prompt_cache "rows" and "shared" still give the same bits.  Not with
    lora="merged" (no merged e4m3 planes), not for bf16 stacks (no e4m3 images).
    lora = "separate": the low-rank term beside the frozen weight (ModuleProducts / SkinnyProducts), the training
    graph's arithmetic; "merged": every product on the stack's merged planes (MergedModuleProducts /
    MergedSkinnyProducts; LoRALlamaStack.merged_weights states cost and staleness).  The strategy is chosen at every
    prefill / score -- where the planes are rebuilt if a weight has been written since -- and kept for the steps that
    follow.
    prompt_cache = "rows": every live row carries its own copy of the prompt's keys and values; "shared": with more
    than one row per prompt (beams, captions) the prompt is stored once per prompt and only the generated tail per row
    (KVCache layout "shared"): `expand` copies no K / V, a beam reorder gathers the tails alone, and the step attends
    with msr3d_attn_decode_shared, which loads a prompt key once for up to 8 rows.  Every logit of every step is
    bit-identical to "rows".  With one row per prompt there is nothing to share and the rows layout is used (`score`
    always sees it)."""

    max_rows = 64          # MSR3D_SKINNY_WIDE_MAX_M: the widest skinny product (every other step kernel takes any N)

    def __init__(self, stack, lora="separate", prompt_cache="rows", weights="bf16"):
        if lora not in ("separate", "merged"):
            raise ValueError(f"lora is 'separate' or 'merged', not {lora!r}")
        if prompt_cache not in ("rows", "shared"):
            raise ValueError(f"prompt_cache is 'rows' or 'shared', not {prompt_cache!r}")
        if weights not in ("bf16", "e4m3"):
            raise ValueError(f"weights is 'bf16' or 'e4m3', not {weights!r}")
        self.stack, self.lora, self.prompt_cache, self.weights = stack, lora, prompt_cache, weights
        self.mods = [m for m in stack.modules() if isinstance(m, LoRALinear)]
        if weights == "bf16":
            if any(m.base == "fp8" for m in self.mods):
                raise NotImplementedError("CachedDecoder: base='fp8' stacks are not supported on bf16 products (weights='bf16' "
                                          "reads the bf16 weights); pass weights='e4m3' to decode on their e4m3 images")
        else:
            if lora == "merged":
                raise NotImplementedError("CachedDecoder: weights='e4m3' with lora='merged' is not supported (base='fp8': a "
                                          "merged plane requantised to e4m3 would round LoRA deltas below e4m3's 2^-4 "
                                          "resolution away)")
            if not self.mods or any(m.base != "fp8" for m in self.mods):
                raise ValueError("CachedDecoder: weights='e4m3' needs a stack built with base='fp8' (a bf16 stack has no "
                                 "e4m3 images)")
        if not stack.layers:
            raise ValueError("CachedDecoder: a stack without layers")
        l0 = stack.layers[0]
        self.H, self.D, self.hidden = l0.num_heads, l0.head_dim, l0.hidden_size
        self.cache, self._plan, self._tables = None, (1, 256), None
        if weights == "e4m3":
            self._wide, self._skinny = E4m3ModuleProducts, E4m3SkinnyProducts()
        else:
            self._wide, self._skinny = ModuleProducts, SkinnyProducts

    def _products(self):
        """The strategies of this call, on current weights: bf16 images of the pairs, or the merged planes (the e4m3
        images of the frozen weights are requantised by the modules themselves when a weight was written)."""
        if self.lora == "merged":
            planes = self.stack.merged_weights()
            self._wide, self._skinny = MergedModuleProducts(planes), MergedSkinnyProducts(planes)
        else:
            refresh_shadows(self.mods, False)
        return self._wide

    def reserve(self, rows_per_prompt, new_tokens):
        self._plan = (int(rows_per_prompt), int(new_tokens))

    # -- prefill ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, inputs_embeds, attention_mask, positions="mask"):
        """-> (B, V) logits of the last position; every layer's K / V of the prompt go into the cache.
        positions = "mask": slot t is rotated by cumsum(mask)[t] - 1 and the next position is the number of unmasked
        tokens (what transformers' `generate` feeds Llama); "arange": slot t is rotated by t and the next position is T
        (what transformers' LlamaModel.forward does when it is called with a mask and no position_ids, i.e. what
        LoRALlamaStack.logits computes: the full forward `score` continues).  The two differ when the prompt has masked
        slots inside it."""
        st = self.stack
        if not inputs_embeds.is_cuda:
            raise RuntimeError("CachedDecoder runs on the GPU only (no CPU fallback)")
        x = inputs_embeds.to(torch.bfloat16)
        B, T, Hd = x.shape
        H, D, dev = self.H, self.D, x.device
        beams, new_tokens = self._plan
        if B * beams > self.max_rows:
            raise ValueError(f"CachedDecoder: at most {self.max_rows} live rows (batch x beams), got {B} x {beams}; "
                             "`search` splits larger batches with prompt_groups")
        Tp = -(-T // 64) * 64                                  # the attention's key tiles; the extra slots are masked
        x, mask = _pad_tokens(x, attention_mask.to(dev).bool(), Tp)
        x = x.contiguous()
        keep = mask.to(torch.uint8).contiguous()
        if positions == "mask":
            pos = (mask.long().cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()
        elif positions == "arange":
            pos = torch.arange(Tp, dtype=torch.int32, device=dev)[None].expand(B, Tp).contiguous()
        else:
            raise ValueError("CachedDecoder.prefill: positions is 'mask' or 'arange'")
        t_max = T + new_tokens
        shared = self.prompt_cache == "shared" and beams > 1 and new_tokens > 0       # (one row a prompt: nothing to share)
        if shared:
            cache = KVCache(len(st.layers), B * beams, t_max, H, D, dev, pingpong=True, layout="shared", prompts=B, t_prompt=T)
        else:
            cache = KVCache(len(st.layers), B * beams, t_max, H, D, dev, pingpong=beams > 1)
        self.cache = cache
        rows = max(t_max, Tp)
        cos, sin = rope_tables(rows, D, st.layers[0].theta, dev)
        self._tables = (cos, sin, rows)
        products = self._products()
        first = slice(0, B * beams, beams)                     # a prompt's first row; expand() fills the others

        def attend(layer, i, h):              # q, k, v; the rotation by `pos`; the cache write; the full attention
            a = layer.self_attn
            q, k, v = products.project(h, (a["q_proj"], a["k_proj"], a["v_proj"]))
            with torch.cuda.device(dev):
                call("msr3d_rope_positions", B, Tp, H, D, ptr(q), ptr(k), ptr(pos), ptr(cos), ptr(sin), rows,
                     current_stream_ptr(dev))
            q, k, v = q.view(B, Tp, H, D), k.view(B, Tp, H, D), v.view(B, Tp, H, D)
            if shared:                        # straight into the prompt planes: the one copy every row of the prompt reads
                cache.prompt_kv[i, 0] = k[:, :T]
                cache.prompt_kv[i, 1] = v[:, :T]
            else:
                cache.k(i)[first, :T] = k[:, :T]
                cache.v(i)[first, :T] = v[:, :T]
            return _AttentionFn.apply(q, k, v, keep)

        logits = decoder_stack(st, x, attend, products, slice(T - 1, T))           # only the last position's are wanted
        cache.pos[first] = mask.sum(-1).to(torch.int32) if positions == "mask" else T
        if shared:                            # (the tails are empty: len and tail_len stay 0)
            cache.prompt_keep.copy_(keep[:, :T])
        else:
            cache.len[first] = T
            cache.keep[first, :T] = keep[:, :T]
        return logits[:, 0]

    def expand(self, beams):
        c = self.cache
        if c is None or beams != self._plan[0]:
            raise RuntimeError("CachedDecoder.expand: call reserve(beams, new_tokens) and prefill first")
        if beams == 1:
            return
        B, T = c.rows // beams, int(c.t_max - self._plan[1])
        if c.layout == "shared":              # no K / V to copy: the prompt planes serve every row
            rows = (c.pos,)
        else:
            kv = c.kv[c.cur].view(c.layers, 2, B, beams, c.t_max, c.heads, c.head_dim)
            kv[:, :, :, 1:, :T] = kv[:, :, :, :1, :T]
            rows = (c.len, c.pos, c.keep)
        for t in rows:
            g = t.view(B, beams, *t.shape[1:])
            g[:, 1:] = g[:, :1]

    # -- many suffixes on one cached prefix ---------------------------------------------------------------------------
    @torch.no_grad()
    def score(self, token_embeds, token_keep, max_rows=8192):
        """token_embeds (B, C, S, hidden), token_keep (B, C, S) (0 = padded slot) -> logits (B, C, S, V) bf16: row
        (b, c, j) is the next-token distribution after prompt b (the cache a `prefill` with one row per prompt left)
        followed by tokens 0 .. j of candidate c, at rotary positions pos[b] + j.  Every layer runs over the B C S suffix
        rows alone with the layer forward's kernels; attention is msr3d_attn_prefix_fwd against the cached prefix.  The
        cache is read, never written: `score` may be called again after one `prefill`.  Candidates are walked in chunks of
        at most `max_rows` suffix rows (every row's arithmetic is its own: the result does not depend on the chunking --
        except under weights="e4m3", where a chunk of fewer than 128 rows multiplies on another kernel than a larger one
        and may differ in last bits)."""
        st, c = self.stack, self.cache
        if c is None:
            raise RuntimeError("CachedDecoder.score before prefill")
        if self._plan[0] != 1:
            raise RuntimeError("CachedDecoder.score: the cache holds beams (prefill with one row per prompt)")
        if not token_embeds.is_cuda:
            raise RuntimeError("CachedDecoder runs on the GPU only (no CPU fallback)")
        B, C, S, Hd = token_embeds.shape
        if B != c.rows or Hd != self.hidden or tuple(token_keep.shape) != (B, C, S):
            raise ValueError("CachedDecoder.score: token_embeds (rows, C, S, hidden) and token_keep (rows, C, S)")
        if not 1 <= S <= 64:
            raise ValueError("CachedDecoder.score: 1 .. 64 suffix tokens")
        H, D, HD, dev = self.H, self.D, self.H * self.D, token_embeds.device
        Sp = 16 if S <= 16 else (32 if S <= 32 else 64)         # the kernel's suffix sizes; the extra slots are masked
        x_all, keep_all = _pad_tokens(token_embeds.to(torch.bfloat16), token_keep.to(dev).bool(), Sp)
        cos, sin, rows = self._tables
        if rows < c.t_max + Sp:                                # (positions are at most len + Sp - 1 <= t_max + Sp - 1)
            rows = c.t_max + Sp
            cos, sin = rope_tables(rows, D, st.layers[0].theta, dev)
            self._tables = (cos, sin, rows)
        products = self._products()
        scale = 1.0 / math.sqrt(D)
        V = st.lm_head.out_features
        out = torch.empty((B, C, S, V), dtype=torch.bfloat16, device=dev)
        step = max(1, int(max_rows) // (B * Sp))
        wanted = slice(0, S) if Sp != S else None              # the padded slots' logits are not wanted
        for c0 in range(0, C, step):
            Cc = min(step, C - c0)
            N = B * Cc
            x = x_all[:, c0:c0 + Cc].reshape(N, Sp, Hd).contiguous()
            skeep = keep_all[:, c0:c0 + Cc].reshape(N, Sp).to(torch.uint8).contiguous()
            pos = (c.pos[:, None, None] + torch.arange(Sp, dtype=torch.int32, device=dev)).expand(B, Cc, Sp)
            pos = pos.reshape(N, Sp).contiguous()

            def attend(layer, i, h):          # q, k, v; the rotation by `pos`; the suffix rows against the cached prefix
                a = layer.self_attn
                q, k, v = products.project(h, (a["q_proj"], a["k_proj"], a["v_proj"]))
                ctx = torch.empty((N * Sp, HD), dtype=torch.bfloat16, device=dev)
                with torch.cuda.device(dev):
                    s = current_stream_ptr(dev)
                    call("msr3d_rope_positions", N, Sp, H, D, ptr(q), ptr(k), ptr(pos), ptr(cos), ptr(sin), rows, s)
                    call("msr3d_attn_prefix_fwd", B, Cc, Sp, c.t_max, H, D, ptr(q), ptr(k), ptr(v), HD, ptr(c.k(i)),
                         ptr(c.v(i)), ptr(c.len), ptr(c.keep), ptr(skeep), ctypes.c_float(scale), ptr(ctx), HD, s)
                return ctx

            out[:, c0:c0 + Cc] = decoder_stack(st, x, attend, products, wanted).view(B, Cc, S, V)
        return out

    # -- one token ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, embeds, beam_idx=None):
        """embeds (N, hidden): the embeddings of the tokens just chosen -> logits (N, V) bf16 of the next position."""
        st, c = self.stack, self.cache
        if c is None:
            raise RuntimeError("CachedDecoder.step before prefill")
        x = embeds.to(torch.bfloat16).contiguous()
        N, dev = x.shape[0], x.device
        if N != c.rows or x.shape[1] != self.hidden:
            raise ValueError("CachedDecoder.step: embeds must be (rows, hidden)")
        if beam_idx is not None:
            c.reorder(beam_idx)
        H, D, HD = self.H, self.D, self.H * self.D
        cos, sin, rows = self._tables
        scale = 1.0 / math.sqrt(D)
        ws = c.workspace
        products = self._skinny

        def attend(layer, i, h):              # q | k | v in one launch; rotation + cache append; the decode attention
            a = layer.self_attn
            q, k, v = products.project(h, (a["q_proj"], a["k_proj"], a["v_proj"]))
            ctx = torch.empty((N, HD), dtype=torch.bfloat16, device=dev)
            with torch.cuda.device(dev):
                s = current_stream_ptr(dev)
                if c.layout == "shared":      # the append on the tail planes; splits 0 = what the rows layout takes
                    call("msr3d_rope_kv_append", N, H, D, c.t_tail, ptr(q), ptr(k), ptr(v), HD, ptr(c.pos), ptr(c.len),
                         ptr(cos), ptr(sin), rows, ptr(c.k(i)), ptr(c.v(i)), s)
                    call("msr3d_attn_decode_shared", c.prompts, N // c.prompts, c.t_prompt, c.t_tail, H, D, ptr(q), HD,
                         ptr(c.prompt_kv[i, 0]), ptr(c.prompt_kv[i, 1]), ptr(c.prompt_keep), ptr(c.k(i)), ptr(c.v(i)),
                         ptr(c.tail_len), 1, ctypes.c_float(scale), ptr(ctx), HD, ptr(ws),
                         ws.numel() if ws is not None else 0, 0, s)
                    return ctx
                call("msr3d_rope_kv_append", N, H, D, c.t_max, ptr(q), ptr(k), ptr(v), HD, ptr(c.pos), ptr(c.len), ptr(cos),
                     ptr(sin), rows, ptr(c.k(i)), ptr(c.v(i)), s)
                call("msr3d_attn_decode", N, c.t_max, H, D, ptr(q), HD, ptr(c.k(i)), ptr(c.v(i)), ptr(c.len), 1, ptr(c.keep),
                     ctypes.c_float(scale), ptr(ctx), HD, ptr(ws), ws.numel() if ws is not None else 0, s)
            return ctx

        logits = decoder_stack(st, x, attend, products)
        c.advance()
        return logits

    def select(self, logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, k):
        """msr3d_decode_select on the step's logits; `prev` (N, n_prev) int64: the rows' generated tokens."""
        if not logits.is_cuda:
            raise RuntimeError("CachedDecoder.select runs on the GPU only")
        lg = logits.to(torch.bfloat16).contiguous()
        N, V = lg.shape
        dev = lg.device
        has_prev = prev.shape[1] > 0                      # (no token yet: NULL, which the entry reads as "none")
        prev = prev.contiguous() if has_prev else None
        n_prev = torch.full((N,), prev.shape[1], dtype=torch.int32, device=dev) if has_prev else None
        val = torch.empty((N, k), dtype=torch.float32, device=dev)
        tok = torch.empty((N, k), dtype=torch.int32, device=dev)
        bs = None if beam_score is None else beam_score.float().contiguous()
        with torch.cuda.device(dev):
            call("msr3d_decode_select", N, V, ptr(lg), V, ptr(prev), prev.shape[1] if has_prev else 0, ptr(n_prev),
                 ctypes.c_float(repetition_penalty), int(min_length), int(-1 if eos_id is None else eos_id), ptr(bs),
                 int(order), int(k), ptr(val), ptr(tok), current_stream_ptr(dev))
        return val, tok

    max_sample_vocab = 39936    # MSR3D_DECODE_SAMPLE_MAX_V

    def sample(self, logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, temperature, top_k, top_p,
               min_keep, k, seed, step, row0, noise=None):
        """msr3d_decode_sample on the step's logits: per row k draws without replacement from softmax(w), w =
        torch_sample_scores(...) -> key, val (N, k) fp32 and tok (N, k) int32 (see torch_sample).  The noise is the
        counter hash of (seed, step, row0 + n, token), or `noise` (N, V) fp32 when given (a test seam)."""
        if not logits.is_cuda:
            raise RuntimeError("CachedDecoder.sample runs on the GPU only")
        lg = logits.to(torch.bfloat16).contiguous()
        N, V = lg.shape
        if V > self.max_sample_vocab:
            raise ValueError(f"CachedDecoder.sample: a vocabulary of {V} does not fit the draw kernel's LDS row "
                             f"(at most {self.max_sample_vocab})")
        dev = lg.device
        has_prev = prev.shape[1] > 0                      # (no token yet: NULL, which the entry reads as "none")
        prev = prev.contiguous() if has_prev else None
        n_prev = torch.full((N,), prev.shape[1], dtype=torch.int32, device=dev) if has_prev else None
        key = torch.empty((N, k), dtype=torch.float32, device=dev)
        val = torch.empty((N, k), dtype=torch.float32, device=dev)
        tok = torch.empty((N, k), dtype=torch.int32, device=dev)
        bs = None if beam_score is None else beam_score.float().contiguous()
        if noise is not None:
            noise = noise.float().contiguous()
            if tuple(noise.shape) != (N, V) or noise.device != dev:
                raise ValueError("CachedDecoder.sample: noise must be (N, V) on the logits' device")
        with torch.cuda.device(dev):
            call("msr3d_decode_sample", N, V, ptr(lg), V, ptr(prev), prev.shape[1] if has_prev else 0, ptr(n_prev),
                 ctypes.c_float(repetition_penalty), int(min_length), int(-1 if eos_id is None else eos_id), ptr(bs),
                 int(order), int(k), ctypes.c_float(temperature), int(top_k), ctypes.c_float(top_p), int(min_keep),
                 ptr(noise), V if noise is not None else 0, int(seed), int(step), int(row0), ptr(key), ptr(val), ptr(tok),
                 current_stream_ptr(dev))
        return key, val, tok

    @staticmethod
    def gumbel_noise(N, V, seed, step, row0, device="cuda"):
        """msr3d_gumbel_noise -> (N, V) fp32: the noise `sample` generates for these arguments."""
        out = torch.empty((N, V), dtype=torch.float32, device=device)
        with torch.cuda.device(out.device):
            call("msr3d_gumbel_noise", N, V, int(seed), int(step), int(row0), ptr(out), V, current_stream_ptr(out.device))
        return out


@torch.no_grad()
def generate(stack, inputs_embeds, attention_mask, embed_tokens, lora="separate", prompt_cache="rows", weights="bf16",
             **search_kwargs):
    """LoRALlamaStack.generate: embed_tokens is the (V, hidden) table (or a callable ids -> embeddings); lora: the
    engine's products, "separate" or "merged", and prompt_cache: its cache layout, "rows" or "shared" -- the same tokens
    either way (CachedDecoder); weights: "bf16", or "e4m3" for a base="fp8" stack on its own e4m3 weights;
    search_kwargs: everything `search` takes (do_sample, top_p, top_k, temperature, num_return_sequences, seed, draw
    among them)."""
    return search(CachedDecoder(stack, lora=lora, prompt_cache=prompt_cache, weights=weights), _embed_fn(embed_tokens),
                  inputs_embeds, attention_mask, **search_kwargs)


@torch.no_grad()
def predict_answers(stack, inputs_embeds, attention_mask, embed_tokens, answer_ids, answer_mask, lora="separate",
                    weights="bf16", **rank_kwargs):
    """LoRALlamaStack.predict_answers: `rank_answers` on a CachedDecoder(lora=lora, weights=weights); rank_kwargs:
    num_ans_candidates, bos_id."""
    return rank_answers(CachedDecoder(stack, lora=lora, weights=weights), _embed_fn(embed_tokens), inputs_embeds,
                        attention_mask, answer_ids, answer_mask, **rank_kwargs)
