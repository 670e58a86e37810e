"""One LoRA-Llama decoder layer on the HIP kernels: what >99 % of a full MSR3D
training step spends its time in (/root/reference/model/msr3d/msr3d.py:103-112 LoRA on q/k/v/o/gate/up/down,
:409-415 the LLM forward under bf16 autocast).  Same computation graph as
transformers.models.llama.modeling_llama.LlamaDecoderLayer with eager attention:

    h = RMSNorm(x); q, k, v = proj(h); RoPE(q, k); P = softmax(q k^T / sqrt(d) + causal + key padding)
    x = x + o_proj(P v); h = RMSNorm(x); x = x + down_proj(silu(gate_proj(h)) * up_proj(h))

with every projection a LoRALinear (msr3d_bf16_gemm_lowrank: frozen bf16 weight + rank-r update riding as one
extra K step), the attention fused (msr3d_attn_fwd / _bwd, csrc/llm_attn.hip: the scores never leave the registers),
and the row-local pieces on csrc/llm_layer.hip.  bf16 storage, fp32 accumulation.
Forward + backward: dx, and dA / dB of the seven LoRA pairs (the base weights and norm weights are frozen).
GPU only."""
import ctypes
import math

import torch
import torch.nn as nn

from .._lib import call, current_stream_ptr, ptr
from .lora import PAD_R, LoRALinear, group_inputs


class _RMSNormFn(torch.autograd.Function):
    """(x, delta, w) -> (s = x + delta, y = RMSNorm(s) w); delta may be None (then s is x)."""

    @staticmethod
    def forward(ctx, x, delta, w, eps):
        D = x.shape[-1]
        x2 = x.reshape(-1, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        M, dev = x2.shape[0], x.device
        d2 = None
        if delta is not None:
            d2 = delta.reshape(-1, D)
            d2 = d2 if d2.is_contiguous() else d2.contiguous()
        s = torch.empty_like(x2) if delta is not None else x2
        y = torch.empty_like(x2)
        rstd = torch.empty(M, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("msr3d_rmsnorm_fwd", M, D, ptr(x2), ptr(d2), ptr(w), ctypes.c_float(eps),
                 ptr(s) if delta is not None else ptr(None), ptr(y), ptr(rstd), current_stream_ptr(dev))
        ctx.save_for_backward(s, w, rstd)
        ctx.has_delta = delta is not None
        ctx.shape = x.shape
        return s.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, ds, dy):
        s, w, rstd = ctx.saved_tensors
        M, D = s.shape
        dev = s.device
        dy2 = dy.reshape(M, D).contiguous() if dy is not None else torch.zeros_like(s)
        ds2 = ds.reshape(M, D).contiguous() if ds is not None else None
        dx = torch.empty_like(s)
        with torch.cuda.device(dev):
            call("msr3d_rmsnorm_bwd", M, D, ptr(dy2), ptr(s), ptr(w), ptr(rstd), ptr(ds2), ptr(dx),
                 current_stream_ptr(dev))
        dx = dx.view(ctx.shape)
        return dx, (dx if ctx.has_delta else None), None, None


class _Rope2Fn(torch.autograd.Function):
    """Rotary embedding IN PLACE on the q and k projections' outputs, one launch each way (msr3d_rope_inplace2), and in
    place on the incoming gradients in backward: no copies (nothing else reads those tensors: _LoRAFn saves its inputs,
    not its output).  Takes the projections' OWN output tensors (tokens, H D) -- not views of them: an in-place op on a
    view of a custom function's output is rebased by autograd (CopySlices), which costs two full copies per call in
    backward (round 4: 128 copies a step)."""

    @staticmethod
    def forward(ctx, q, k, cos, sin, B, T, H, D):
        for x in (q, k):
            if not x.is_contiguous() or x.numel() != B * T * H * D:
                raise RuntimeError("_Rope2Fn: contiguous (B T, H D) tensors expected")
        with torch.cuda.device(q.device):
            call("msr3d_rope_inplace2", B, T, H, D, ptr(q), ptr(k), ptr(cos), ptr(sin), 0,
                 current_stream_ptr(q.device))
        ctx.mark_dirty(q, k)
        ctx.save_for_backward(cos, sin)
        ctx.dims = (B, T, H, D)
        return q, k

    @staticmethod
    def backward(ctx, gq, gk):
        cos, sin = ctx.saved_tensors
        B, T, H, D = ctx.dims
        gq, gk = gq.contiguous(), gk.contiguous()
        with torch.cuda.device(gq.device):
            call("msr3d_rope_inplace2", B, T, H, D, ptr(gq), ptr(gk), ptr(cos), ptr(sin), 1,
                 current_stream_ptr(gq.device))
        return gq, gk, None, None, None, None, None, None


class _AttentionFn(torch.autograd.Function):
    """q, k, v (B, T, H, D) bf16 (RoPE applied), keep (B, T) uint8 or None -> context (B, T, H D) bf16.
    Fused (csrc/llm_attn.hip): the scores stay in registers -- online softmax forward, the row's log-sum-exp kept; the
    backward recomputes the probabilities from it (one kernel for dq, one for dk / dv).  Round 4 ran seven batched
    GEMMs, two softmax launches and six transposes per layer through 85 MB of fp32 scores."""

    @staticmethod
    def forward(ctx, q, k, v, keep):
        B, T, H, D = q.shape
        if T % 64 or D not in (64, 128):
            raise ValueError("attention: sequence length a multiple of 64, head size 64 or 128")
        for t in (q, k, v):
            if not t.is_contiguous():
                raise RuntimeError("attention: contiguous (B, T, H, D) tensors expected")
        dev, HD = q.device, H * D
        scale = 1.0 / math.sqrt(D)
        out = torch.empty((B, T, HD), dtype=torch.bfloat16, device=dev)
        lse = torch.empty((B, H, T), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("msr3d_attn_fwd", B, T, H, D, ptr(q), ptr(k), ptr(v), HD, ptr(keep), ctypes.c_float(scale), ptr(out),
                 ptr(lse), current_stream_ptr(dev))
        ctx.save_for_backward(q, k, v, out, lse, keep)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, do):
        q, k, v, out, lse, keep = ctx.saved_tensors
        B, T, H, D = q.shape
        dev, HD = q.device, H * D
        do = do.reshape(B, T, HD)
        do = do if do.is_contiguous() else do.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty_like(lse)
        with torch.cuda.device(dev):
            call("msr3d_attn_bwd", B, T, H, D, ptr(q), ptr(k), ptr(v), ptr(out), ptr(do), HD, ptr(keep),
                 ctypes.c_float(ctx.scale), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), current_stream_ptr(dev))
        return dq, dk, dv, None


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        gate, up = gate.contiguous(), up.contiguous()
        out = torch.empty_like(gate)
        with torch.cuda.device(gate.device):
            call("msr3d_swiglu_fwd", gate.numel(), ptr(gate), ptr(up), ptr(out), current_stream_ptr(gate.device))
        ctx.save_for_backward(gate, up)
        return out

    @staticmethod
    def backward(ctx, dh):
        gate, up = ctx.saved_tensors
        dh = dh.contiguous()
        dg, du = torch.empty_like(gate), torch.empty_like(up)
        with torch.cuda.device(gate.device):
            call("msr3d_swiglu_bwd", gate.numel(), ptr(gate), ptr(up), ptr(dh), ptr(dg), ptr(du),
                 current_stream_ptr(gate.device))
        return dg, du


def rope_tables(T, D, theta=10000.0, device=None):
    """cos / sin (T, D) fp32 for positions 0..T-1 (modeling_llama.LlamaRotaryEmbedding, default rope type)."""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32, device=device) / D))
    fr = torch.arange(T, dtype=torch.float32, device=device)[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


class ModuleProducts:
    """How a walk multiplies a layer's projections.  A products strategy has two operations, both -> (tokens, N) bf16:
    `project(h, mods)`, the projections `mods` of the same activations h, one tensor each, and `gated(h, gate, up)`,
    silu(gate(h)) * up(h); and `head(h, lm_head)`, the logits.  This one is the module call (LoRALinear on the tiled
    GEMMs, _SwiGLUFn, FrozenLinear; differentiable): training, the full forward, `CachedDecoder.prefill` and `.score`.
    The others are products.py's: the decoding engine's weight sources, each also as the launches of one decode step."""

    @staticmethod
    def project(h, mods):
        # forward2d: the autograd function's own output, which the rotation may go on to write in place
        return [m.forward2d(h) for m in mods]

    @staticmethod
    def gated(h, gate, up):
        return _SwiGLUFn.apply(gate(h), up(h))

    @staticmethod
    def head(h, lm_head):
        return lm_head(h)


def __getattr__(name):            # (products.py imports this module: its MergedModuleProducts is re-exported lazily)
    if name != "MergedModuleProducts":
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    from .products import MergedModuleProducts
    return MergedModuleProducts


def decoder_layer(layer, i, x, delta, attend, products, rows=None):
    """THE statement of layer `i` of a stack, for every walk (training, prefill, score, step):

        x0 = x + delta; h = RMSNorm(x0); x1 = x0 + o_proj(attend(layer, i, h)); y = down(silu(gate(h2)) * up(h2)),
        h2 = RMSNorm(x1)                                                      -> (x1, y): the layer's output is x1 + y

    x (..., hidden) bf16; delta: a residual term still to be added to x (the previous layer's y) or None -- the input
    norm's launch adds it, as the second norm's adds o, so a stack has no stand-alone add kernels either way.
    attend(layer, i, h) -> context rows (tokens, H D): the attention half, which owns all that differs between the
    walks -- the q / k / v products, the rotation, the cache write or append, the attention entry.
    products: how the projections are multiplied (ModuleProducts).
    rows: a slice of dimension 1 (the LAST layer of a stack whose head only reads those positions): the attention
    still runs over every token, the second norm and the MLP -- token-local -- only over x[:, rows]."""
    a, m = layer.self_attn, layer.mlp
    # (x0 = x + delta; with delta None it is x itself -- and the ONLY use of the layer input from here on, so its
    # gradient arrives in one piece through the norm's backward)
    x0, h = _RMSNormFn.apply(x, delta, layer.input_layernorm_weight, layer.eps)
    o, = products.project(attend(layer, i, h), (a["o_proj"],))
    if o.dim() != x0.dim():
        o = o.view(x0.shape)
    if rows is not None:
        x0, o = x0[:, rows].contiguous(), o[:, rows].contiguous()
    x1, h2 = _RMSNormFn.apply(x0, o, layer.post_attention_layernorm_weight, layer.eps)
    y, = products.project(products.gated(h2, m["gate_proj"], m["up_proj"]), (m["down_proj"],))
    return x1, (y if y.dim() == x1.dim() else y.view(x1.shape))


def decoder_stack(stack, x, attend, products, rows=None):
    """THE walk of a LoRALlamaStack: every layer with its MLP output left to the NEXT norm's launch (decoder_layer's
    `delta`), `rows` selected in the last layer only, the final norm, the head -> logits."""
    delta, last = None, len(stack.layers) - 1
    for i, layer in enumerate(stack.layers):
        x, delta = decoder_layer(layer, i, x, delta, attend, products, rows if i == last else None)
    if rows is not None and last < 0:
        x = x[:, rows].contiguous()
    _, h = _RMSNormFn.apply(x, delta, stack.norm_weight, stack.eps)
    return products.head(h, stack.lm_head)


def causal_attention(attention_mask):
    """The attention half of training and the full forward: q, k, the rotation of both by their slots 0 .. T-1 in one
    launch, v, the fused causal attention over all T tokens under the key padding attention_mask (B, T) or None."""
    keep = None if attention_mask is None else attention_mask.to(torch.uint8).contiguous()     # once, not per layer

    def attend(layer, i, h):
        B, T, _ = h.shape
        H, D = layer.num_heads, layer.head_dim
        a = layer.self_attn
        cos, sin = layer._tables(T, h.device)
        q, k = ModuleProducts.project(h, (a["q_proj"], a["k_proj"]))
        q, k = _Rope2Fn.apply(q, k, cos, sin, B, T, H, D)
        v, = ModuleProducts.project(h, (a["v_proj"],))
        return _AttentionFn.apply(q.view(B, T, H, D), k.view(B, T, H, D), v.view(B, T, H, D), keep)
    return attend


class LoRALlamaDecoderLayer(nn.Module):
    """State-dict keys: `self_attn.{q,k,v,o}_proj.{weight, lora_A.weight, lora_B.weight}`, `mlp.{gate,up,down}_proj.*`,
    and the two norm weights as buffers of the layer (`input_layernorm_weight`, `post_attention_layernorm_weight`).
    Hugging Face / peft spell these `input_layernorm.weight`, `q_proj.base_layer.weight`, `lora_A.default.weight`:
    msr3d_amd/llm/checkpoint.py maps both ways (load_hf_state_dict, hf_state_dict, peft_adapter_state_dict)."""

    def __init__(self, hidden_size=4096, num_heads=32, intermediate_size=11008, r=16, lora_alpha=16, rms_eps=1e-6,
                 rope_theta=10000.0, device=None, base="bf16"):
        super().__init__()
        if hidden_size % num_heads or (hidden_size // num_heads) % 64:
            raise ValueError("head size must be a multiple of 64")
        self.hidden_size, self.num_heads, self.head_dim = hidden_size, num_heads, hidden_size // num_heads
        self.eps, self.theta = rms_eps, rope_theta
        mk = lambda i, o: LoRALinear(i, o, r=r, lora_alpha=lora_alpha, device=device, base=base)     # noqa: E731
        self.self_attn = nn.ModuleDict(dict(q_proj=mk(hidden_size, hidden_size), k_proj=mk(hidden_size, hidden_size),
                                            v_proj=mk(hidden_size, hidden_size), o_proj=mk(hidden_size, hidden_size)))
        self.mlp = nn.ModuleDict(dict(gate_proj=mk(hidden_size, intermediate_size), up_proj=mk(hidden_size, intermediate_size),
                                      down_proj=mk(intermediate_size, hidden_size)))
        if device is not None and torch.device(device).type == "cuda":
            # one x A^T product per input: as many members as fit the 64 columns of the shared low-rank activation
            # (r = 16: q, k, v and gate, up; r = 32: q, k and gate, up -- v keeps its own product).  When ALL consumers of
            # the norm's output are members, they also share one d-input buffer in backward; with v outside the group
            # its gradient reaches autograd between two members, so every member then returns its own.
            fit = max(1, PAD_R // r)
            for names, table in ((("q_proj", "k_proj", "v_proj"), self.self_attn), (("gate_proj", "up_proj"), self.mlp)):
                mods = [table[n] for n in names][:fit]
                if len(mods) > 1:
                    group_inputs(mods, shared_grad=len(mods) == len(names))
        self.register_buffer("input_layernorm_weight", torch.ones(hidden_size, dtype=torch.bfloat16, device=device))
        self.register_buffer("post_attention_layernorm_weight", torch.ones(hidden_size, dtype=torch.bfloat16, device=device))
        self._rope = None

    def _tables(self, T, dev):
        if self._rope is None or self._rope[0] != (T, str(dev)):
            self._rope = ((T, str(dev)), rope_tables(T, self.head_dim, self.theta, dev))
        return self._rope[1]

    def forward(self, x, attention_mask=None, delta=None, defer_residual=False, tail_from=0):
        """x (B, T, hidden) bf16; attention_mask (B, T) (1 / True = real token) or None.
        delta: a residual term still to be added to x (the previous layer's MLP output): the input norm's launch
        adds it.  defer_residual: return (x_after_attention, mlp_output) instead of their sum, for the next layer's
        `delta` -- a stack of layers then has no stand-alone add kernels in forward or backward.
        tail_from = p > 0 (the LAST layer of a stack whose head only reads positions >= p): the attention still runs over
        all T tokens, but the second norm and the MLP -- token-local -- only over positions p .. T-1; the outputs are
        (B, T - p, hidden)."""
        if not x.is_cuda:
            raise RuntimeError("LoRALlamaDecoderLayer runs on the GPU only (no CPU fallback)")
        x1, y = decoder_layer(self, 0, x.to(torch.bfloat16), delta, causal_attention(attention_mask), ModuleProducts,
                              slice(tail_from, None) if tail_from > 0 else None)
        if defer_residual:
            return x1, y
        return x1 + y

