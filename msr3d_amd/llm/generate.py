"""`generate` for the LoRA-Llama stack: greedy and beam search, sampling and beam sampling over a key / value cache, one
new token per step on the decode kernels of csrc/llm_decode.hip and the draw kernel of csrc/llm_sample.hip (what
transformers' `LlamaForCausalLM.generate(inputs_embeds=..., attention_mask=..., do_sample=..., top_p=..., temperature=...,
num_beams=..., repetition_penalty=..., length_penalty=..., num_return_sequences=...)` computes; the reference's
MSR3D.generate calls exactly that).

Four pieces, one module each:

* kv_cache.py  `KVCache`: the buffers of one call and every operation that depends on their layout.
* products.py  how a walk multiplies a layer's projections, per weight source (separate, merged, e4m3) and width.
* search.py    `search` and `rank_answers`, in torch against the engine interface alone, and sampling stated in torch.
* here         `CachedDecoder`, the engine: `prefill` runs the layer forward kernels over the padded prompt (positions =
               cumsum(mask) - 1, clamped at 0: what transformers' generate feeds Llama when it is given a mask) and
               writes every layer's K / V into the cache; `step` runs one token per live row: per layer RMSNorm,
               q | k | v as ONE skinny launch, rotation + cache append, decode attention, o, RMSNorm, gate | up with the
               SwiGLU epilogue, down; then the final norm and the head.  No host synchronisation inside `step`: lengths
               and positions live in device memory.  `score` runs B x C short suffixes against one cached prefix
               (msr3d_attn_prefix_fwd, csrc/llm_attn.hip).  `token_loop` is `search(loop="device")`'s tokens as
               replays of captured graphs, the bookkeeping on the kernels of csrc/llm_beam.hip.  And the two doors,
               `generate` and `predict_answers`.

`max_length` counts GENERATED tokens (the prompt travels as embeddings and has no ids).  GPU only for the engine."""
import ctypes
import math
import time

import torch

from .._lib import call, current_stream_ptr, ptr
from .decoder import _AttentionFn, decoder_stack, rope_tables
from .kv_cache import KVCache
from .lora import LoRALinear, refresh_shadows, shadows_are_fresh
from .products import FUSED_MAX_ROWS, E4m3Products, MergedModuleProducts, SeparateProducts
from .search import (_embed_fn, counter_uniform_bits, gumbel_from_bits, prompt_groups, rank_answers,  # noqa: F401
                     search, torch_sample, torch_sample_scores, torch_select)


def _pad_tokens(x, keep, n):
    """x (..., t, hidden), keep (..., t) bool -> both with n token slots: the n - t appended ones are zero and masked."""
    t = keep.shape[-1]
    if n == t:
        return x, keep
    return (torch.cat([x, x.new_zeros((*x.shape[:-2], n - t, x.shape[-1]))], -2),
            torch.cat([keep, keep.new_zeros((*keep.shape[:-1], n - t))], -1))


class CachedDecoder:
    """The decoding engine of a LoRALlamaStack (see the module docstring).  At most `max_rows` live rows (batch x beams)
    per prefill; `search` splits a larger batch into groups of whole prompts.  THE statement of the five keywords
    (LoRALlamaStack.generate and MSR3DFullStep.generate pass them on):
    weights = "bf16" (default): every product reads the bf16 base weights; a base="fp8" stack is refused.
    weights = "e4m3": a stack whose projections are all base="fp8" decodes on its own e4m3 images -- what its training
    forward multiplies on (products.E4m3Products states the kernels): the step's launch count at half the weight bytes
    (the head stays bf16), prefill and `score` on e4m3 as well, on one of two kernels that sum in different orders:
    under "e4m3" a `score` chunk or a prefill below 128 rows may differ from a larger one in last bits -- the results
    are NOT invariant under chunking and grouping, unlike "bf16".  Reproducible call to call (no atomics); prompt_cache
    "rows" and "shared" still give the same bits.  Not with lora="merged" (no merged e4m3 planes), not for bf16 stacks.
    lora = "separate": the low-rank term beside the frozen weight (products.SeparateProducts), the training graph's
    arithmetic; "merged": every product on the stack's merged planes (products.MergedModuleProducts;
    LoRALlamaStack.merged_weights states cost and staleness).  `products` is set at every prefill / score -- where the
    planes are rebuilt if a weight has been written since -- and kept for the steps that follow.
    prompt_cache = "rows": every live row carries its own copy of the prompt's keys and values; "shared": with more
    than one row per prompt (beams, captions) the prompt is stored once per prompt and only the generated tail per row
    (KVCache states the layout): `expand` copies no K / V, a beam reorder gathers the tails alone, and the step's
    attention loads a prompt key once for up to 8 rows.  Every logit of every step is bit-identical to "rows".  With
    one row per prompt there is nothing to share and the rows layout is used (`score` always sees it).
    kv = "bf16" (default) or "e4m3": the cache holds OCP e4m3 codes with one power-of-two scale per (slot, head)
    (kv_cache.torch_kv_quantize states the format): half the bytes of the planes, of every step's attention stream and
    of a beam reorder.  Only what is STORED is rounded, so the prefill's logits are those of "bf16"; a step's differ
    (about 3 % rel-L2 on the test fixture) and tokens may, so "e4m3" is pinned to a statement of itself: with
    `kv_kernels=False` the cache keeps bf16 planes on the bf16 kernels and rounds every write through the format in
    torch, and the e4m3 kernels give that engine's logits bit for bit.  Combines with every value of the other three
    keywords, with sampling and with prompt groups.  `score` refuses it (its cache is one prompt row read once per 64
    suffix rows: nothing to gain), so `predict_answers` has no such keyword.
    step = "split" (default): a layer of `step` is eight launches under lora="merged" -- the norm, q | k | v, the
    rotation + cache append, the attention, o, the norm, gate | up, down; "fused": the three that move no weights ride
    inside the products on msr3d_bf16_skinny_fused (`_fused_stack` states the walk): five launches a layer and the head,
    six on an e4m3 cache, which keeps its append.  Every logit of every step and every byte written to the cache is
    bit-identical to "split" on the same settings, so tokens, beam scores and draws are too.  Needs lora="merged" and
    weights="bf16" (the other sources' r-row product reads the normed activations as a tensor); with every prompt_cache,
    kv and loop.  Above products.FUSED_MAX_ROWS live rows the step runs its split launches (the same bits: a scheduling
    choice, measured in profiles/generate_fused.txt).  `score` runs no decode step, so `predict_answers` has no such
    keyword."""

    max_rows = 64          # MSR3D_SKINNY_WIDE_MAX_M: the widest skinny product (every other step kernel takes any N)

    def __init__(self, stack, lora="separate", prompt_cache="rows", weights="bf16", kv="bf16", kv_kernels=True,
                 step="split"):
        if lora not in ("separate", "merged"):
            raise ValueError(f"lora is 'separate' or 'merged', not {lora!r}")
        if prompt_cache not in ("rows", "shared"):
            raise ValueError(f"prompt_cache is 'rows' or 'shared', not {prompt_cache!r}")
        if weights not in ("bf16", "e4m3"):
            raise ValueError(f"weights is 'bf16' or 'e4m3', not {weights!r}")
        if kv not in ("bf16", "e4m3"):
            raise ValueError(f"kv is 'bf16' or 'e4m3', not {kv!r}")
        if step not in ("split", "fused"):
            raise ValueError(f"step is 'split' or 'fused', not {step!r}")
        self.stack, self.lora, self.prompt_cache, self.weights = stack, lora, prompt_cache, weights
        self.kv, self.kv_kernels, self.step_form = kv, bool(kv_kernels), step
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
        if step == "fused" and (lora != "merged" or weights != "bf16"):
            raise ValueError("CachedDecoder: step='fused' needs lora='merged' (and weights='bf16'): the r-row product of the "
                             "separate and e4m3 sources reads the normed activations as a tensor, so the norm launch stays")
        if not stack.layers:
            raise ValueError("CachedDecoder: a stack without layers")
        l0 = stack.layers[0]
        self.H, self.D, self.hidden = l0.num_heads, l0.head_dim, l0.hidden_size
        self.cache, self._plan, self._tables = None, (1, 256), None
        self.capture_seconds = []         # host seconds of every graph capture of `token_loop`, in order (for benches)
        # the products of this call (merged: made at prefill / score, on the planes of that moment)
        self.products = E4m3Products() if weights == "e4m3" else (SeparateProducts() if lora == "separate" else None)

    def _current_products(self):
        """On current weights: bf16 images of the pairs, or the merged planes (the modules requantise e4m3 images)."""
        if self.lora == "merged":
            return MergedModuleProducts(self.stack.merged_weights())
        refresh_shadows(self.mods, False)
        return self.products

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
        # the layout, decided here and nowhere else (one row a prompt: nothing to share)
        fmt = dict(dtype=self.kv, kernels=self.kv_kernels)
        if self.prompt_cache == "shared" and beams > 1 and new_tokens > 0:
            cache = KVCache(len(st.layers), B * beams, t_max, H, D, dev, pingpong=True, layout="shared", prompts=B, t_prompt=T,
                            **fmt)
        else:
            cache = KVCache(len(st.layers), B * beams, t_max, H, D, dev, pingpong=beams > 1, **fmt)
        self.cache = cache
        rows = max(t_max, Tp)
        cos, sin = rope_tables(rows, D, st.layers[0].theta, dev)
        self._tables = (cos, sin, rows)
        products = self.products = self._current_products()

        def attend(layer, i, h):              # q, k, v; the rotation by `pos`; the cache write; the full attention
            a = layer.self_attn
            q, k, v = products.project(h, (a["q_proj"], a["k_proj"], a["v_proj"]))
            with torch.cuda.device(dev):
                call("msr3d_rope_positions", B, Tp, H, D, ptr(q), ptr(k), ptr(pos), ptr(cos), ptr(sin), rows,
                     current_stream_ptr(dev))
            q, k, v = q.view(B, Tp, H, D), k.view(B, Tp, H, D), v.view(B, Tp, H, D)
            cache.write_prompt(i, k[:, :T], v[:, :T])
            return _AttentionFn.apply(q, k, v, keep)

        logits = decoder_stack(st, x, attend, products, slice(T - 1, T))           # only the last position's are wanted
        cache.close_prompt(mask.sum(-1).to(torch.int32) if positions == "mask" else T, keep[:, :T])
        return logits[:, 0]

    def expand(self, beams):
        c = self.cache
        if c is None or beams != self._plan[0]:
            raise RuntimeError("CachedDecoder.expand: call reserve(beams, new_tokens) and prefill first")
        if beams > 1:
            c.expand(beams, int(c.t_max - self._plan[1]))

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
        if self.kv != "bf16":
            raise ValueError("CachedDecoder.score reads a bf16 cache (msr3d_attn_prefix_fwd); kv='e4m3' is for generate")
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
        products = self.products = self._current_products()
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
        if x.shape[0] != c.rows or x.shape[1] != self.hidden:
            raise ValueError("CachedDecoder.step: embeds must be (rows, hidden)")
        if beam_idx is not None:
            c.reorder(beam_idx)
        cos, sin, rows = self._tables
        scale = 1.0 / math.sqrt(self.D)
        if self.step_form == "fused" and x.shape[0] <= FUSED_MAX_ROWS:
            logits = self._fused_stack(x, cos, sin, rows, scale)
            c.advance()
            return logits
        products = self.products.skinny

        def attend(layer, i, h):              # q | k | v in one launch; rotation + cache append; the decode attention
            a = layer.self_attn
            q, k, v = products.project(h, (a["q_proj"], a["k_proj"], a["v_proj"]))
            return c.attend(i, q, k, v, cos, sin, rows, scale)

        logits = decoder_stack(st, x, attend, products)
        c.advance()
        return logits

    def _fused_stack(self, x, cos, sin, table_rows, scale):
        """step="fused": decoder.decoder_stack -- THE statement, which `step` walks above -- with every launch that moves no
        weights folded into the product beside it (products.FusedSkinnyProducts; include/msr3d_hip.h,
        msr3d_bf16_skinny_fused): per layer q | k | v under the input norm with the rotation and the cache append behind it,
        the decode attention, o with the residual addition, gate | up under the second norm with SwiGLU, down with the
        residual addition -- five launches where the split step has eight; then the head under the final norm.  The
        residual stream is materialised by the products (x1 = x + o, x2 = x1 + y, each a fresh tensor: `x`, the caller's
        embeddings at layer 0, is read only), so decoder_layer's `delta` never forms: bf16(x1 + y) is what the next
        norm's launch would have stored.  Every logit and every byte written to the cache equals the split step's
        (tests/test_generate_fused_gpu.py).  An e4m3 cache keeps its own append launch (the quantiser needs a whole head's
        amax; the statement engine rounds the slot in torch): six launches a layer."""
        st, c, H, D = self.stack, self.cache, self.H, self.D
        p = self.products.fused
        for i, layer in enumerate(st.layers):
            a, m = layer.self_attn, layer.mlp
            qkv, norm = (a["q_proj"], a["k_proj"], a["v_proj"]), (layer.input_layernorm_weight, layer.eps)
            if self.kv == "bf16":
                ck, cv, t_max = c.planes(i)
                q, = p.project(x, qkv, norm=norm, rope=(H, D, c.pos, c.len, cos, sin, table_rows, ck, cv, t_max))
                ctx = c.attend_appended(i, q, scale)
            else:
                q, k, v = p.project(x, qkv, norm=norm)
                ctx = c.attend(i, q, k, v, cos, sin, table_rows, scale)
            x1, = p.project(ctx, (a["o_proj"],), residual=x)
            act = p.gated(x1, m["gate_proj"], m["up_proj"], (layer.post_attention_layernorm_weight, layer.eps))
            x, = p.project(act, (m["down_proj"],), residual=x1)
        return p.head(x, st.lm_head, (st.norm_weight, st.eps))

    # -- the token loop on the device ---------------------------------------------------------------------------------
    @torch.no_grad()
    def token_loop(self, state, logits, embed_fn, eos_id, pad_id, min_length, repetition_penalty, len_div, poll=4):
        """`search(loop="device")`'s tokens on this engine, after prefill / expand: state (search.beam_state or
        greedy_state, on the GPU) is advanced IN PLACE until `done`, and returned.  logits (rows, V): the prefill's,
        one row per live row.  A token is msr3d_decode_select on the static logits buffer -> msr3d_beam_advance /
        msr3d_greedy_advance (the state, next_tok, beam_idx, n_prev, cur, done) -> embed_fn(next_tok) -> the cache
        reorder by the device beam_idx (beams) -> `step` -> the logits buffer: one linear chain on one stream in which
        every operand is a static buffer or allocated by the chain itself, and nothing is decided on the host.
        The first token runs eagerly (the warm-up: LoRA shadow tables, per-kernel attributes); from the second on a
        token is a replay of a graph captured with torch.cuda.graph ON THE SAME STREAM, one graph per cache side --
        a reorder gathers from side `cur` into the other, so a token captured on side 0 holds other pointers than one
        captured on side 1: two graphs for beams, replayed in turn as the sides alternate, one for greedy search (no
        reorder, one side).  The graphs live as long as this call (one group of `search`).  The host reads `done` every
        `poll` tokens.
        Bounds: the loop runs at most L = the state's sequence length tokens, whatever `done` says, and `reserve` was
        given new_tokens >= L (checked), so the cache has a slot for every step: token i (0-based) appends at slot
        T + i <= T + L - 1 < t_max.  Tokens run after `done` (at most poll - 1) leave the state alone (the advance
        kernels return at once) and cost a wasted select and step within those L; msr3d_rope_kv_append and the decode
        attention clamp `len` to the cache besides."""
        c = self.cache
        if c is None:
            raise RuntimeError("CachedDecoder.token_loop before prefill")
        beams = "run_seq" in state
        seqs = state["run_seq"] if beams else state["seq"]
        L, N, dev = int(seqs.shape[-1]), c.rows, logits.device
        if seqs.numel() != N * L or tuple(logits.shape[:1]) != (N,) or not seqs.is_cuda:
            raise ValueError("CachedDecoder.token_loop: the state and the logits must have the cache's rows, on the GPU")
        if self._plan[1] < L:
            raise ValueError(f"CachedDecoder.token_loop: {L} tokens do not fit the {self._plan[1]} slots reserved")
        if int(poll) < 1:
            raise ValueError("poll >= 1")
        i32 = torch.int32
        lg = logits.to(torch.bfloat16).contiguous().clone()            # THE logits buffer: every token reads and rewrites it
        V = lg.shape[1]
        k = 2 * state["run_scores"].shape[1] if beams else 1
        val = torch.empty((N, k), dtype=torch.float32, device=dev)
        tok = torch.zeros((N, k), dtype=i32, device=dev)
        n_prev = torch.zeros((N,), dtype=i32, device=dev)
        next_tok = torch.zeros((N,), dtype=torch.int64, device=dev)
        cur, done = state["cur"], state["done"]
        if beams:
            B, nb = state["run_scores"].shape
            beam_idx = torch.arange(N, dtype=i32, device=dev)
            work = torch.zeros((B,), dtype=i32, device=dev)
            is_fin, heur = state["is_fin"].view(torch.uint8), state["heur"].view(torch.uint8)
            score = state["run_scores"]
        else:
            unfinished = state["unfinished"].view(torch.uint8)
        rp, ml = ctypes.c_float(repetition_penalty), int(min_length)

        def token():
            with torch.cuda.device(dev):
                s = current_stream_ptr(dev)
                call("msr3d_decode_select", N, V, ptr(lg), V, ptr(seqs), L, ptr(n_prev), rp, ml, int(eos_id),
                     ptr(score) if beams else ptr(None), 1 if beams else 0, k, ptr(val), ptr(tok), s)
                if beams:
                    call("msr3d_beam_advance", B, nb, L, ptr(val), ptr(tok), int(eos_id), ptr(len_div), ptr(score),
                         ptr(seqs), ptr(state["fin_seq"]), ptr(state["fin_scores"]), ptr(state["fin_len"]), ptr(is_fin),
                         ptr(heur), ptr(cur), ptr(done), ptr(next_tok), ptr(beam_idx), ptr(n_prev), ptr(work), s)
                else:
                    call("msr3d_greedy_advance", N, L, ptr(tok), k, int(eos_id), int(pad_id), ptr(seqs), ptr(unfinished),
                         ptr(cur), ptr(done), ptr(next_tok), ptr(n_prev), s)
            lg.copy_(self.step(embed_fn(next_tok), beam_idx if beams else None))

        side = torch.cuda.Stream(device=dev)                           # the capture's stream, the eager token's as well
        here = torch.cuda.current_stream(dev)
        side.wait_stream(here)
        graphs = {}
        with torch.cuda.stream(side):
            n = 0
            while n < L:
                if n == 0:
                    token()
                else:
                    p = c.cur
                    g = graphs.get(p)
                    if g is None:
                        g = graphs[p] = torch.cuda.CUDAGraph()
                        # (the pairs' bf16 images are those of the prefill: no weight is written during a call, so the
                        # graph holds no refresh of them -- what a captured TRAINING step needs and LoRALinear would add)
                        t0 = time.perf_counter()
                        with shadows_are_fresh(self.mods), \
                                torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                            token()
                        self.capture_seconds.append(time.perf_counter() - t0)
                        if beams:
                            c.flip()                                   # (the capture moved nothing: the data is on side p)
                    g.replay()
                    if beams:
                        c.flip()
                n += 1
                if (n % poll == 0 or n == L) and int(done):            # (a synchronisation: every replay so far is over)
                    break
            side.synchronize()
        here.wait_stream(side)
        return state

    @staticmethod
    def _logits_operands(who, logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, k):
        """-> N, V, device, the arguments msr3d_decode_select and msr3d_decode_sample both begin with (the bf16 logits,
        `prev` with every row's count, the processors' scalars, the beam score, order, k), the tensors those point into."""
        if not logits.is_cuda:
            raise RuntimeError(f"CachedDecoder.{who} runs on the GPU only")
        lg = logits.to(torch.bfloat16).contiguous()
        N, V = lg.shape
        dev = lg.device
        has_prev = prev.shape[1] > 0                      # (no token yet: NULL, which the entry reads as "none")
        prev = prev.contiguous() if has_prev else None
        n_prev = torch.full((N,), prev.shape[1], dtype=torch.int32, device=dev) if has_prev else None
        bs = None if beam_score is None else beam_score.float().contiguous()
        return N, V, dev, (N, V, ptr(lg), V, ptr(prev), prev.shape[1] if has_prev else 0, ptr(n_prev),
                           ctypes.c_float(repetition_penalty), int(min_length), int(-1 if eos_id is None else eos_id),
                           ptr(bs), int(order), int(k)), (lg, prev, n_prev, bs)

    def select(self, logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, k):
        """msr3d_decode_select on the step's logits; `prev` (N, n_prev) int64: the rows' generated tokens."""
        N, V, dev, operands, held = self._logits_operands("select", logits, prev, repetition_penalty, min_length, eos_id,
                                                          beam_score, order, k)
        val = torch.empty((N, k), dtype=torch.float32, device=dev)
        tok = torch.empty((N, k), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            call("msr3d_decode_select", *operands, ptr(val), ptr(tok), current_stream_ptr(dev))
        return val, tok

    max_sample_vocab = 39936    # MSR3D_DECODE_SAMPLE_MAX_V

    def sample(self, logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, temperature, top_k, top_p,
               min_keep, k, seed, step, row0, noise=None):
        """msr3d_decode_sample on the step's logits: per row k draws without replacement from softmax(w), w =
        torch_sample_scores(...) -> key, val (N, k) fp32 and tok (N, k) int32 (see torch_sample).  The noise is the
        counter hash of (seed, step, row0 + n, token), or `noise` (N, V) fp32 when given (a test seam)."""
        N, V, dev, operands, held = self._logits_operands("sample", logits, prev, repetition_penalty, min_length, eos_id,
                                                          beam_score, order, k)
        if V > self.max_sample_vocab:
            raise ValueError(f"CachedDecoder.sample: a vocabulary of {V} does not fit the draw kernel's LDS row "
                             f"(at most {self.max_sample_vocab})")
        key = torch.empty((N, k), dtype=torch.float32, device=dev)
        val = torch.empty((N, k), dtype=torch.float32, device=dev)
        tok = torch.empty((N, k), dtype=torch.int32, device=dev)
        if noise is not None:
            noise = noise.float().contiguous()
            if tuple(noise.shape) != (N, V) or noise.device != dev:
                raise ValueError("CachedDecoder.sample: noise must be (N, V) on the logits' device")
        with torch.cuda.device(dev):
            call("msr3d_decode_sample", *operands, ctypes.c_float(temperature), int(top_k), ctypes.c_float(top_p),
                 int(min_keep), ptr(noise), V if noise is not None else 0, int(seed), int(step), int(row0), ptr(key),
                 ptr(val), ptr(tok), current_stream_ptr(dev))
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
             kv="bf16", step="split", **search_kwargs):
    """LoRALlamaStack.generate: embed_tokens is the (V, hidden) table (or a callable ids -> embeddings); lora,
    prompt_cache, weights, kv, step: as CachedDecoder states them; search_kwargs: everything `search` takes."""
    return search(CachedDecoder(stack, lora=lora, prompt_cache=prompt_cache, weights=weights, kv=kv, step=step),
                  _embed_fn(embed_tokens), inputs_embeds, attention_mask, **search_kwargs)


@torch.no_grad()
def predict_answers(stack, inputs_embeds, attention_mask, embed_tokens, answer_ids, answer_mask, lora="separate",
                    weights="bf16", **rank_kwargs):
    """LoRALlamaStack.predict_answers: `rank_answers` on a CachedDecoder(lora=lora, weights=weights); rank_kwargs:
    num_ans_candidates, bos_id."""
    return rank_answers(CachedDecoder(stack, lora=lora, weights=weights), _embed_fn(embed_tokens), inputs_embeds,
                        attention_mask, answer_ids, answer_mask, **rank_kwargs)
