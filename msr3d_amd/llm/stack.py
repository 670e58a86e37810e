"""The language-model side of one MSR3D training step, assembled from the C-ABI pieces
(/root/reference/model/msr3d/msr3d.py:95-112 peft LoRA on q/k/v/o/gate/up/down, :409-415 the LLM forward from
`inputs_embeds` under bf16 autocast, :426-441 the per-sequence mean cross-entropy):

    inputs_embeds (B, T, H) -> n x LoRALlamaDecoderLayer -> RMSNorm -> lm_head (frozen, bf16) -> logits (B, T, V) bf16
                            -> seq_mean_cross_entropy(logits, targets)  (B,)

Everything frozen is bf16 and stays frozen (embeddings are not part of the step: the caller scatters the scene
tokens into `inputs_embeds`, msr3d.py:277-287); the only trainable tensors are the layers' lora_A / lora_B (fp32),
which is what a data-parallel step has to exchange: 14 small tensors per layer.  GPU only."""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .decoder import LoRALlamaDecoderLayer, ModuleProducts, causal_attention, decoder_stack
from .lora import LoRALinear, _gemm as _lora_gemm, merge_pairs, refresh_shadows, shadows_are_fresh
from .losses import seq_mean_cross_entropy


def _gemm(M, N, K, P, Q, C, dev):
    """C (M, N) bf16 = P (M, K) Q (N, K)^T, bf16 operands: lora._gemm without a low-rank term."""
    _lora_gemm(M, N, K, 0, P, K, Q, K, None, 0, None, 0, C, N, 0, 1.0, dev)


class _FrozenLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod):
        K, N = mod.in_features, mod.out_features
        x2 = x.reshape(-1, K)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        y = torch.empty((x2.shape[0], N), dtype=torch.bfloat16, device=x.device)
        _gemm(x2.shape[0], N, K, x2, mod.weight, y, x.device)
        ctx.mod, ctx.shape = mod, x.shape
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        mod = ctx.mod
        K, N = mod.in_features, mod.out_features
        dy2 = dy.reshape(-1, N).to(torch.bfloat16)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        M = dy2.shape[0]
        S = next((c for c in (10, 8, 5, 4) if N % (64 * c) == 0), 0)
        if M <= 1024 and N >= 8192 and S:
            # few rows against a long reduction (the 32000-way head over the answer span: 260 x 4096 x 32000): one tile per
            # 128 x 128 of the output is 96 workgroups walking 500 K steps each (507 us); the reduction cut into S chunks
            # as a batch with fp32 partials puts 10 x as many workgroups on it, the partials are added in chunk order
            part = torch.empty((S, M, K), dtype=torch.float32, device=dy.device)
            with torch.cuda.device(dy.device):
                _lib.call("msr3d_bf16_gemm_batched", S, 1, M, K, N // S, _lib.ptr(dy2), N, N // S, 0, _lib.ptr(mod.weight_t),
                          N, N // S, 0, _lib.ptr(part), K, M * K, 0, 1, ctypes.c_float(1.0),
                          _lib.current_stream_ptr(dy.device))
            dx = part.sum(0).to(torch.bfloat16)
        else:
            dx = torch.empty((M, K), dtype=torch.bfloat16, device=dy.device)
            _gemm(M, K, N, dy2, mod.weight_t, dx, dy.device)
        return dx.view(ctx.shape), None


class FrozenLinear(nn.Module):
    """nn.Linear(in_features, out_features, bias=False) with a frozen bf16 weight, kept in both orientations
    (forward and dx read k-contiguous rows): the language-model head."""

    def __init__(self, in_features, out_features, device=None):
        super().__init__()
        if in_features % 64 or out_features % 64:
            raise ValueError("feature sizes must be multiples of 64")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.empty((out_features, in_features), dtype=torch.bfloat16, device=device))
        self.register_buffer("weight_t", torch.empty((in_features, out_features), dtype=torch.bfloat16, device=device),
                             persistent=False)
        self._wt_version = None

    def _sync(self):
        key = (self.weight._version, self.weight.data_ptr())
        if self._wt_version != key:
            with torch.no_grad():
                self.weight_t.copy_(self.weight.t())
            self._wt_version = (self.weight._version, self.weight.data_ptr())

    def load_weight(self, w):
        self.weight.copy_(w.to(torch.bfloat16))
        self._sync()

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("FrozenLinear runs on the GPU only (no CPU fallback)")
        self._sync()
        return _FrozenLinearFn.apply(x.to(torch.bfloat16), self)


class LoRALlamaStack(nn.Module):
    """`layers` decoder layers + final RMSNorm + head.  Own state-dict keys: `layers.i.*` (see LoRALlamaDecoderLayer),
    `norm_weight`, `lm_head.weight`; Hugging Face LlamaForCausalLM / peft checkpoints load through
    msr3d_amd/llm/checkpoint.py::load_hf_state_dict (and save through hf_state_dict / peft_adapter_state_dict)."""

    def __init__(self, num_layers, hidden_size=4096, num_heads=32, intermediate_size=11008, vocab_size=32000, r=16,
                 lora_alpha=16, rms_eps=1e-6, rope_theta=10000.0, device=None, base="bf16"):
        """base = "fp8": the decoder layers' frozen projections on e4m3 operands (LoRALinear); the head stays bf16."""
        super().__init__()
        self.layers = nn.ModuleList([LoRALlamaDecoderLayer(hidden_size, num_heads, intermediate_size, r, lora_alpha,
                                                           rms_eps, rope_theta, device=device, base=base)
                                     for _ in range(num_layers)])
        self.register_buffer("norm_weight", torch.ones(hidden_size, dtype=torch.bfloat16, device=device))
        self.lm_head = FrozenLinear(hidden_size, vocab_size, device=device)
        self.eps = rms_eps
        self._lora_mods = None
        self._merged = None           # (key, {module: plane}) of merged_weights()

    def lora_parameters(self):
        return [p for p in self.parameters() if p.requires_grad]

    def _pairs(self):
        if self._lora_mods is None:
            self._lora_mods = [m for m in self.modules() if isinstance(m, LoRALinear)]
        return self._lora_mods

    def merged_weights(self):
        """-> {LoRALinear: plane (N, K) bf16 = bf16(W + s B A)} for every projection of the stack: peft's
        merge_and_unload, from the fp32 masters of A / B, which `generate` / `predict_answers` with lora="merged" and
        checkpoint.hf_state_dict(merged=True) read.  The planes are allocated once and live on the stack -- an engine is
        built per call -- and are rebuilt, all in ONE launch (msr3d_lora_merge), only when stale: when any pair's
        `_pair_key()` or any base weight's (version, data_ptr) differs from what they were built from, or a module's
        `invalidate_shadows()` has been called (FlatAdamW.mark_written moves the pair key).  A call on fresh planes costs
        that key comparison and nothing else.
        MEMORY: one more copy of the seven projections of every layer -- 13 GB for a 7B model -- until
        `release_merged()`.  base="fp8" stacks are refused."""
        mods = self._pairs()
        if any(m.base == "fp8" for m in mods):
            raise NotImplementedError("LoRALlamaStack.merged_weights: base='fp8' stacks are not supported (their products "
                                      "read e4m3 weights; merged e4m3 decoding is not implemented)")
        key = tuple(m._merge_key() for m in mods)
        if self._merged is not None and self._merged[0] == key:
            return self._merged[1]
        planes = self._merged[1] if self._merged is not None else {}
        if any(m not in planes or planes[m].device != m.weight.device for m in mods):
            planes = {m: torch.empty_like(m.weight) for m in mods}
        self._merged = None                                    # (a failed merge leaves no half-built planes behind)
        with torch.no_grad():
            merge_pairs(mods, [planes[m] for m in mods])
        self._merged = (key, planes)
        return planes

    def release_merged(self):
        """Free the merged planes (the next lora="merged" call builds them again)."""
        self._merged = None

    def logits(self, inputs_embeds, attention_mask=None, from_position=0):
        """from_position = p: only the logits of positions p .. T-1 (B, T - p, V) -- the attention of every layer still runs
        over all T tokens; the LAST layer's token-local half (second norm + MLP), the final norm and the head only over that
        tail (nothing else ever reads the other rows of those)."""
        if not inputs_embeds.is_cuda:
            raise RuntimeError("LoRALlamaStack runs on the GPU only (no CPU fallback)")
        x = inputs_embeds.to(torch.bfloat16)
        # the bf16 images of all 7 x layers LoRA pairs: ONE launch per optimiser step (224 pairs x 4 copies before)
        mods = self._pairs()
        capturing = x.is_cuda and torch.cuda.is_current_stream_capturing()
        refresh_shadows(mods, capturing)
        with shadows_are_fresh(mods, capturing):
            # the last layer's token-local half (second norm + MLP), the final norm and the head only over the positions
            # the caller reads
            return decoder_stack(self, x, causal_attention(attention_mask), ModuleProducts,
                                 slice(from_position, None) if from_position > 0 else None)

    def generate(self, inputs_embeds, attention_mask, embed_tokens, lora="separate", prompt_cache="rows", weights="bf16",
                 kv="bf16", step="split", **search_kwargs):
        """Greedy / beam search or sampling from prompt embeddings over a key / value cache (msr3d_amd/llm/generate.py)
        -> (B x num_return_sequences, <= max_length) int64 generated tokens, a prompt's rows adjacent.  embed_tokens: the
        (V, hidden) embedding table (or a callable ids -> embeddings); search_kwargs: bos_id, eos_id, pad_id, num_beams,
        max_length (GENERATED tokens), min_length, repetition_penalty, length_penalty, and do_sample, top_p, top_k,
        temperature, num_return_sequences, seed, draw (`search` states them: nucleus / top-k sampling and beam sampling
        with transformers' semantics, drawn by msr3d_decode_sample from counter noise -- the same seed, the same tokens).
        Any batch: up to 64 live rows (B x max(num_beams, num_return_sequences)) decode in one pass, more in groups of
        whole prompts one after another (the same tokens).
        lora = "separate" (default): the low-rank term is computed beside the frozen weight, as in training;
        lora = "merged": every product streams the merged plane bf16(W + s B A) of `merged_weights()` alone (no r-row
        launches; one more copy of the projections in memory; the weights rounded once more, so other bits).
        prompt_cache = "rows" (default): every live row has its own copy of the prompt's keys and values;
        prompt_cache = "shared": one copy per prompt and the generated tail per row (a beam reorder moves the tails
        alone, the attention loads a prompt key once for a prompt's rows) -- the same bits, so the same tokens.
        weights = "bf16" (default): the products read the bf16 base weights (a base="fp8" stack is refused);
        weights = "e4m3": a base="fp8" stack decodes on its own e4m3 weights, the ones its training forward multiplies
        on (CachedDecoder states what that changes: half the step's weight stream; last bits may move with the batch's
        grouping; not with lora="merged").
        kv = "bf16" (default): the key / value cache holds what the projections wrote;
        kv = "e4m3": it holds e4m3 codes with a power-of-two scale per (slot, head) -- half the cache, half the bytes
        every step's attention and every beam reorder move; the logits move by about 3 % rel-L2 (CachedDecoder and
        kv_cache.torch_kv_quantize state the format and what it is pinned to).  With every value of the other keywords.
        loop = "host" (default): one host decision and synchronisation per token; loop = "device" (greedy and beam
        search, not sampling): a token is a replay of a captured graph, the beam bookkeeping two kernels
        (msr3d_beam_advance / msr3d_greedy_advance), and the host reads `done` every `poll` (default 4) tokens --
        `search` and CachedDecoder.token_loop state it; ties go to the lower index, where the host loop leaves them open.
        step = "split" (default): a layer of the decode step is its products and, between them, two norms and the
        rotation + cache append as launches of their own; step = "fused" (lora="merged" only): those ride inside the
        products (msr3d_bf16_skinny_fused) -- five launches a layer for eight, six on an e4m3 cache, up to
        products.FUSED_MAX_ROWS live rows (above: the split step) -- every logit and cache byte the same bits, so the same
        tokens (CachedDecoder states it; profiles/generate_fused.txt has what it measured)."""
        from .generate import generate
        return generate(self, inputs_embeds, attention_mask, embed_tokens, lora=lora, prompt_cache=prompt_cache,
                        weights=weights, kv=kv, step=step, **search_kwargs)

    def predict_answers(self, inputs_embeds, attention_mask, embed_tokens, answer_ids, answer_mask, lora="separate",
                        weights="bf16", **rank_kwargs):
        """Closed-set answer ranking on one cached copy of every prompt (msr3d_amd/llm/search.py::rank_answers) ->
        dict(answers_id (B,), topk_ids (B, C), loss (B, C) fp32, first_prob (B, A)).  answer_ids / answer_mask (A, S):
        the tokenised answer list, bos first, right-padded; rank_kwargs: num_ans_candidates, bos_id; lora and weights: as
        in `generate` (under weights="e4m3" the losses may move in last bits with num_ans_candidates, which sets the
        number of suffix rows a `score` chunk multiplies at once)."""
        from .generate import predict_answers
        return predict_answers(self, inputs_embeds, attention_mask, embed_tokens, answer_ids, answer_mask, lora=lora,
                               weights=weights, **rank_kwargs)

    def forward(self, inputs_embeds, attention_mask=None, targets=None, supervised_from=None):
        """-> logits (B, T, V) bf16, or with `targets` (B, T) int64 (negative = not supervised) the per-sequence mean
        cross-entropy (B,) of msr3d.py:426-441.
        supervised_from = p (with targets): the caller GUARANTEES targets[:, :p] < 0 (msr3d.py:384-392 builds them that
        way: -100 over the whole prompt, p = its length).  The loss reads logits[t] against targets[t + 1], so only the
        logits of positions p - 1 .. T - 2 can contribute: final norm, the 32000-way head and the cross-entropy then run
        over T - p + 1 positions instead of T (65 of 576 in the benchmarked shape) -- same loss, same gradients (the
        skipped rows' d logits are exactly zero), 0.9 ms of a step's head products not spent on rows nothing reads."""
        if targets is None:
            return self.logits(inputs_embeds, attention_mask)
        p0 = 0 if supervised_from is None else max(int(supervised_from) - 1, 0)
        lg = self.logits(inputs_embeds, attention_mask, from_position=p0)
        return seq_mean_cross_entropy(lg, targets[:, p0:] if p0 else targets)
