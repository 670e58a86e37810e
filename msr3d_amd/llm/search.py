"""The engine-agnostic half of decoding, in torch alone: `search` (greedy / beam search and sampling with transformers'
semantics) and `rank_answers` (closed-set answer ranking, the reference's MSR3D.predict_answers, on ONE cached copy of
each prompt) are written against an engine interface, so they run on the CPU with any engine -- that is how their logic
is checked exactly against transformers -- and on the GPU with generate.CachedDecoder.  Sampling is stated once:
`torch_sample_scores` (the processors, temperature, top-k, top-p with ties at the cut ordered by token id, then
log-softmax or the beam score) gives the scores w a token is drawn from, `torch_sample` draws by Gumbel keys (the k
largest w + noise = k draws without replacement), `counter_uniform_bits` is the noise's counter hash in integers.
`CachedDecoder.sample` is all of it as one kernel (msr3d_decode_sample); `search(draw="multinomial")` draws with
torch.multinomial instead, where transformers does, which pins `search` to transformers on the CPU.
`torch_beam_advance` / `torch_greedy_advance` state the bookkeeping of one token on a state that holds `cur` and `done`
itself: `search(loop="device")`, whose host reads `done` every `poll` tokens (csrc/llm_beam.hip: the same as two kernels)."""
import math

import torch


def _append_bos(embed_fn, x, mask, bos_id):
    """The embedding of bos_id and a mask column of ones appended to every prompt."""
    bos = embed_fn(torch.full((x.shape[0],), int(bos_id), dtype=torch.int64, device=x.device)).to(x.dtype)
    return torch.cat([x, bos[:, None]], 1), torch.cat([mask, torch.ones_like(mask[:, :1])], 1)


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
           num_return_sequences=1, seed=None, draw=None, loop="host", poll=4):
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
    Live rows per prompt are max(num_beams, n).

    loop = "host" (default): the token loop above, one synchronisation a token.  loop = "device" (greedy and beam search
    with n <= num_beams; not sampling): the bookkeeping between two steps is `torch_greedy_advance` /
    `torch_beam_advance` on a state that lives on the engine's device, `done` included, and the host reads `done` only
    every `poll` tokens -- a token has nothing for the host to decide.  An engine with `token_loop(state, logits,
    embed_fn, eos_id=, pad_id=, min_length=, repetition_penalty=, len_div=, poll=)` runs the tokens itself
    (CachedDecoder: captured graphs, the two advances as kernels); for any other engine the statement is called step by
    step around `engine.step`.  Either way at most max_length tokens run in all; tokens run after `done` (at most
    poll - 1) change nothing.  Every top-k of the device loop is the first k of a STABLE descending sort (ties to the
    lower beam, then `select`'s order), where the host loop's torch.topk leaves ties open; the length divisor is an f32
    table applied by IEEE division."""
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
    if loop not in ("host", "device"):
        raise ValueError(f"loop is 'host' or 'device', not {loop!r}")
    if int(poll) != poll or poll < 1:
        raise ValueError("poll >= 1 (tokens between two reads of `done`)")
    if loop == "device" and do_sample:
        raise NotImplementedError("search: loop='device' does not sample -- the draw kernel takes `step` as a launch "
                                  "argument, which a replayed graph cannot change; use loop='host' with do_sample")
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
    if loop == "device":
        outs = [_device_group(engine, embed_fn, x[a:b], mask[a:b], bos_id, eos_id, pad_id, nb, L, min_length,
                              repetition_penalty, length_penalty, n_ret, int(poll)) for a, b in groups]
    else:
        outs = [_search_group(engine, embed_fn, x[a:b], mask[a:b], bos_id, eos_id, pad_id, nb, L, min_length,
                              repetition_penalty, length_penalty, n_ret, sampler, a * per) for a, b in groups]
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


# ------------------------------------------------------------------------------------- the token loop on the device
def length_divisors(L, length_penalty, device=None):
    """-> (L) f32: d[cur] = (cur + 1) ** length_penalty, made once on the host (Python floats, rounded to f32); a
    finished hypothesis' score is sum_logprobs / d[cur] by IEEE division."""
    return torch.tensor([float((c + 1) ** length_penalty) for c in range(int(L))], dtype=torch.float32, device=device)


def beam_state(B, nb, L, pad_id, device=None):
    """The state of beam search for one group of B prompts x nb beams before its first token, as `_search_group` has it;
    cur (tokens written) and done are one int32 each, on the device like the rest."""
    f32, dev = torch.float32, device
    run_scores = torch.zeros((B, nb), dtype=f32, device=dev)
    run_scores[:, 1:] = -1.0e9
    run_seq = torch.full((B, nb, L), int(pad_id), dtype=torch.int64, device=dev)
    return dict(run_scores=run_scores, run_seq=run_seq, fin_seq=run_seq.clone(),
                fin_scores=torch.full((B, nb), -1.0e9, dtype=f32, device=dev),
                fin_len=torch.zeros((B, nb), dtype=torch.int64, device=dev),
                is_fin=torch.zeros((B, nb), dtype=torch.bool, device=dev), heur=torch.ones((B,), dtype=torch.bool, device=dev),
                cur=torch.zeros((1,), dtype=torch.int32, device=dev), done=torch.zeros((1,), dtype=torch.int32, device=dev))


def greedy_state(N, L, pad_id, device=None):
    """The state of greedy search over N rows before its first token."""
    return dict(seq=torch.full((N, L), int(pad_id), dtype=torch.int64, device=device),
                unfinished=torch.ones((N,), dtype=torch.bool, device=device),
                cur=torch.zeros((1,), dtype=torch.int32, device=device), done=torch.zeros((1,), dtype=torch.int32, device=device))


def _first_k(x, k):
    """The indices of the k largest along dim 1 as the first k of a stable descending sort: ties to the lower index."""
    return torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]


def _take(t, i):                          # t (B, n, ...), i (B, m) -> (B, m, ...)
    return torch.gather(t, 1, i.view(*i.shape, *([1] * (t.dim() - 2))).expand(*i.shape, *t.shape[2:]))


def torch_beam_advance(state, val, tok, eos_id, len_div):
    """THE statement of msr3d_beam_advance, device-agnostic and without a synchronisation: one token of beam search's
    bookkeeping, what `_search_group` does between `select` and `engine.step` when it does not sample.
    state: `beam_state`'s dict; val, tok (B nb, 2 nb): the step's candidates from `select` (order 1, run_scores as the
    beam score); len_div: `length_divisors`.  -> (new state, next_tok (B nb) int64, beam_idx (B nb) int32, global rows);
    the state given is not written.  Stated, not left to torch: every top-k is the first k of a stable descending sort
    (`_first_k`); the length divisor is len_div[cur], applied by IEEE division; with `done` set the state returned equals
    the one given, `done` included (next_tok / beam_idx are then meaningless): a loop may overrun."""
    f32 = torch.float32
    run_seq, heur, cur, done = state["run_seq"], state["heur"], state["cur"], state["done"]
    B, nb, L = run_seq.shape
    K2 = 2 * nb
    dev = run_seq.device
    c = cur.long().clamp(0, L - 1)                                  # (1,): the column this token is written to
    last = (cur + 1 >= L)                                           # (1,) bool
    div = len_div[c]                                                # (1,) f32
    flat = val.reshape(B, nb * K2).float()
    top_i = _first_k(flat, K2)
    top_val = torch.gather(flat, 1, top_i)
    src_beam = top_i // K2
    tok_k = torch.gather(tok.reshape(B, nb * K2).long(), 1, top_i)
    top_seq = _take(run_seq, src_beam).scatter(2, c.view(1, 1, 1).expand(B, K2, 1), tok_k[:, :, None])
    hits = (tok_k == int(eos_id)) | last
    # the running beams of the next step: the best candidates that did not just end
    run_lp = top_val + hits.to(f32) * -1.0e9
    nxt_i = _first_k(run_lp, nb)
    n_run_seq, n_run_scores, beam_sel = _take(top_seq, nxt_i), _take(run_lp, nxt_i), _take(src_beam, nxt_i)
    # finished hypotheses: only a candidate among the first `beams` may be kept
    did = hits & (torch.arange(K2, device=dev) < nb)[None]
    fl = top_val / div
    fl = fl + (~heur)[:, None].to(f32) * -1.0e9
    fl = fl + (~did).to(f32) * -1.0e9
    m_scores = torch.cat([state["fin_scores"], fl], 1)
    mi = _first_k(m_scores, nb)
    n_fin_seq = _take(torch.cat([state["fin_seq"], top_seq], 1), mi)
    n_fin_len = _take(torch.cat([state["fin_len"], (cur.long() + 1).expand(B, K2)], 1), mi)
    n_is_fin = _take(torch.cat([state["is_fin"], did], 1), mi)
    n_fin_scores = _take(m_scores, mi)
    # can a running beam still beat the worst kept hypothesis?  (judged at the current length)
    best_running = n_run_scores[:, :1] / div
    worst_fin = torch.where(n_is_fin, n_fin_scores.min(1, keepdim=True)[0], torch.full_like(n_fin_scores, -1.0e9))
    n_heur = heur & (best_running > worst_fin).any(-1)
    go_on = n_heur.any() & ~hits.all()
    new = dict(run_scores=n_run_scores, run_seq=n_run_seq, fin_seq=n_fin_seq, fin_scores=n_fin_scores, fin_len=n_fin_len,
               is_fin=n_is_fin, heur=n_heur, cur=cur + 1, done=(~go_on).to(torch.int32).view(1))
    stop = done != 0                                                # after `done`: nothing changes
    new = {k: torch.where(stop, state[k], v) for k, v in new.items()}
    next_tok = torch.gather(tok_k, 1, nxt_i).reshape(-1)
    offs = (torch.arange(B, device=dev) * nb)[:, None]
    return new, next_tok, (beam_sel + offs).reshape(-1).to(torch.int32)


def torch_greedy_advance(state, tok, eos_id, pad_id):
    """THE statement of msr3d_greedy_advance: one token of greedy search's bookkeeping.  state: `greedy_state`'s dict;
    tok (N, 1): the step's `select` (order 0, k = 1).  -> (new state, next_tok (N) int64): finished rows go on as pad_id;
    done = the last column was written or no row is unfinished; with `done` set the state returned equals the one given."""
    seq, unfinished, cur, done = state["seq"], state["unfinished"], state["cur"], state["done"]
    N, L = seq.shape
    c = cur.long().clamp(0, L - 1)
    nxt = torch.where(unfinished, tok[:, 0].long(), torch.full_like(tok[:, 0].long(), int(pad_id)))
    n_unfinished = unfinished & (nxt != int(eos_id))
    n_done = ((cur + 1 >= L) | ~n_unfinished.any()).to(torch.int32).view(1)
    new = dict(seq=seq.scatter(1, c.view(1, 1).expand(N, 1), nxt[:, None]), unfinished=n_unfinished, cur=cur + 1, done=n_done)
    stop = done != 0
    return {k: torch.where(stop, state[k], v) for k, v in new.items()}, nxt


def _statement_loop(engine, state, logits, embed_fn, eos_id, pad_id, min_length, repetition_penalty, len_div, poll):
    """The device loop for an engine without `token_loop`: the statement step by step around `engine.step`.  -> state."""
    select = getattr(engine, "select", torch_select)
    beams = "run_seq" in state
    L = (state["run_seq"] if beams else state["seq"]).shape[-1]
    for n in range(L):                                     # (never more than L tokens; cur == n until `done`)
        if beams:
            N = state["run_scores"].numel()
            nb = state["run_scores"].shape[1]
            val, tok = select(logits, state["run_seq"].view(N, L)[:, :n], repetition_penalty, min_length, eos_id,
                              state["run_scores"].view(-1), 1, 2 * nb)
            state, nxt, beam_idx = torch_beam_advance(state, val, tok, eos_id, len_div)
        else:
            _, tok = select(logits, state["seq"][:, :n], repetition_penalty, min_length, eos_id, None, 0, 1)
            state, nxt = torch_greedy_advance(state, tok, eos_id, pad_id)
            beam_idx = None
        if ((n + 1) % poll == 0 or n + 1 == L) and int(state["done"]):
            break
        if n + 1 < L:                                      # (after an unread `done` the step is wasted work, nothing else)
            logits = engine.step(embed_fn(nxt), beam_idx)
    return state


def _device_group(engine, embed_fn, x, mask, bos_id, eos_id, pad_id, nb, L, min_length, repetition_penalty, length_penalty,
                  n_ret, poll):
    """`search(loop="device")` for one group of whole prompts that fits the engine."""
    dev = x.device
    if bos_id is not None:
        x, mask = _append_bos(embed_fn, x, mask, bos_id)
    B = x.shape[0]
    if hasattr(engine, "reserve"):
        engine.reserve(nb, L)
    logits = engine.prefill(x, mask)
    engine.expand(nb)
    eos = -1 if eos_id is None else int(eos_id)
    if nb == 1:
        state, len_div = greedy_state(B, L, pad_id, dev), None
    else:
        state, len_div = beam_state(B, nb, L, pad_id, dev), length_divisors(L, length_penalty, dev)
        logits = logits.repeat_interleave(nb, 0)
    loop = getattr(engine, "token_loop", None)
    if loop is not None:
        state = loop(state, logits, embed_fn, eos_id=eos, pad_id=int(pad_id), min_length=int(min_length),
                     repetition_penalty=float(repetition_penalty), len_div=len_div, poll=poll)
    else:
        state = _statement_loop(engine, state, logits, embed_fn, eos, int(pad_id), int(min_length),
                                float(repetition_penalty), len_div, poll)
    if nb == 1:
        return state["seq"][:, :int(state["cur"])]
    fin_seq, fin_len = state["fin_seq"], state["fin_len"]
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

