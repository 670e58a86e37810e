"""Helpers shared by the generate tests and tests/golden/make_golden_generate.py: the fixture's transformers model
(LlamaForCausalLM, eager attention, peft's LoRA formula on all seven projections, weights from
tests/helpers.py::llama_stack_weights), the seeded bf16-rounded embedding table, transformers' own `generate` called
from `inputs_embeds`, and an fp32 CPU engine with the interface msr3d_amd/llm/generate.py::search is written against
(prefill / expand / step), built on the same transformers model with its own key / value cache.  CPU only."""
import os

import numpy as np
import torch

from tests.golden.make_golden_llama_layer import NAMES, LoRA
from tests.helpers import _bf16_round, llama_stack_weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = dict(layers=2, hidden=512, heads=8, inter=1024, vocab=1024, r=16, alpha=16, eps=1e-6, theta=10000.0)


def embed_table(seed, vocab=CFG["vocab"], hidden=CFG["hidden"]):
    """(vocab, hidden) fp32, bf16-representable: the token embedding table of the fixture's model."""
    rng = np.random.default_rng(seed + 4242)
    return _bf16_round((0.5 * rng.standard_normal((vocab, hidden))).astype(np.float32))


def hf_model(seed, max_positions=256):
    from transformers.models.llama.modeling_llama import LlamaConfig, LlamaForCausalLM
    c = CFG
    cfg = LlamaConfig(hidden_size=c["hidden"], num_attention_heads=c["heads"], num_key_value_heads=c["heads"],
                      intermediate_size=c["inter"], num_hidden_layers=c["layers"], vocab_size=c["vocab"],
                      rms_norm_eps=c["eps"], rope_theta=c["theta"], max_position_embeddings=max_positions,
                      attention_bias=False, mlp_bias=False, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    model = LlamaForCausalLM(cfg).float().eval()
    w = llama_stack_weights(seed, c["layers"], c["hidden"], c["inter"], c["r"], c["vocab"])
    s = c["alpha"] / c["r"]
    with torch.no_grad():
        for i, layer in enumerate(model.model.layers):
            lw = w["layers"][i]
            for n in NAMES:
                parent = layer.self_attn if n in ("q_proj", "k_proj", "v_proj", "o_proj") else layer.mlp
                setattr(parent, n, LoRA(torch.from_numpy(lw[n]), torch.from_numpy(lw[n + ".A"]),
                                        torch.from_numpy(lw[n + ".B"]), s))
            layer.input_layernorm.weight.copy_(torch.from_numpy(lw["ln1"]))
            layer.post_attention_layernorm.weight.copy_(torch.from_numpy(lw["ln2"]))
        model.model.norm.weight.copy_(torch.from_numpy(w["norm"]))
        model.lm_head.weight.copy_(torch.from_numpy(w["head"]))
        model.model.embed_tokens.weight.copy_(torch.from_numpy(embed_table(seed)))
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def prompt(seed, B=3, T=24, left_pad=5, hole=(6, 10)):
    """-> inputs_embeds (B, T, hidden) fp32 bf16-representable and attention_mask (B, T) int64.  Row 0 has no padding,
    row 1 is left-padded, row 2 (when B > 2) has masked slots INSIDE the prompt -- what the reference's object mask
    produces at the scene-token positions.  The last column is the bos embedding (token 1), mask 1."""
    rng = np.random.default_rng(seed + 3000)
    x = _bf16_round((0.5 * rng.standard_normal((B, T, CFG["hidden"]))).astype(np.float32))
    x[:, -1] = embed_table(seed)[1]
    keep = np.ones((B, T), np.int64)
    if B > 1:
        keep[1, :left_pad] = 0
    if B > 2:
        keep[2, hole[0]:hole[1]] = 0
    return torch.from_numpy(x), torch.from_numpy(keep)


def hf_generate(model, x, keep, max_new_tokens, num_beams=1, repetition_penalty=1.0, length_penalty=1.0,
                min_length=0, eos_id=2, pad_id=2, full=False):
    """transformers' generate from `inputs_embeds`.  The installed version subtracts the prompt's length from `max_length`
    AND `min_length` when it is given embeddings; `max_new_tokens` / `min_new_tokens` ask it for what this library's
    `max_length` / `min_length` mean (generated tokens alone)."""
    from transformers import GenerationConfig
    gc = GenerationConfig(do_sample=False, num_beams=num_beams, max_new_tokens=max_new_tokens, min_new_tokens=min_length or None,
                          repetition_penalty=repetition_penalty, length_penalty=length_penalty, eos_token_id=eos_id,
                          pad_token_id=pad_id, bos_token_id=1, use_cache=True, output_logits=full, output_scores=full,
                          return_dict_in_generate=True)
    with torch.no_grad():
        out = model.generate(inputs_embeds=x, attention_mask=keep, generation_config=gc)
    return out if full else out.sequences


def positions_of(mask):
    return (mask.long().cumsum(-1) - 1).clamp_min(0)


class HFEngine:
    """The engine interface of msr3d_amd.llm.generate.search on the fixture's fp32 transformers model (CPU)."""

    def __init__(self, model):
        self.model, self.cache, self.mask = model, None, None

    @torch.no_grad()
    def prefill(self, inputs_embeds, attention_mask):
        from transformers import DynamicCache
        self.cache = DynamicCache(config=self.model.config)
        self.mask = attention_mask.long().clone()
        out = self.model(inputs_embeds=inputs_embeds.float(), attention_mask=self.mask,
                         position_ids=positions_of(self.mask), past_key_values=self.cache, use_cache=True)
        return out.logits[:, -1].float()

    def expand(self, beams):
        if beams > 1:
            self.cache.batch_repeat_interleave(beams)
            self.mask = self.mask.repeat_interleave(beams, 0)

    @torch.no_grad()
    def step(self, embeds, beam_idx=None):
        if beam_idx is not None:
            self.cache.reorder_cache(beam_idx.long())
            self.mask = self.mask[beam_idx.long()]
        self.mask = torch.cat([self.mask, torch.ones_like(self.mask[:, :1])], 1)
        out = self.model(inputs_embeds=embeds.float()[:, None], attention_mask=self.mask,
                         position_ids=positions_of(self.mask)[:, -1:], past_key_values=self.cache, use_cache=True)
        return out.logits[:, -1].float()


def gpu_stack(seed, base="bf16"):
    """The fixture's model as a LoRALlamaStack on cuda, and its embedding table (vocab, hidden) bf16."""
    from msr3d_amd.llm import LoRALlamaStack
    c = CFG
    w = llama_stack_weights(seed, c["layers"], c["hidden"], c["inter"], c["r"], c["vocab"])
    net = LoRALlamaStack(c["layers"], c["hidden"], c["heads"], c["inter"], c["vocab"], r=c["r"], lora_alpha=c["alpha"],
                         rms_eps=c["eps"], rope_theta=c["theta"], device="cuda", base=base)
    with torch.no_grad():
        for i, layer in enumerate(net.layers):
            lw = w["layers"][i]
            for n in NAMES:
                m = (layer.self_attn if n in layer.self_attn else layer.mlp)[n]
                m.load_base_weight(torch.from_numpy(lw[n]).cuda())
                m.lora_A.weight.copy_(torch.from_numpy(lw[n + ".A"]))
                m.lora_B.weight.copy_(torch.from_numpy(lw[n + ".B"]))
            layer.input_layernorm_weight.copy_(torch.from_numpy(lw["ln1"]))
            layer.post_attention_layernorm_weight.copy_(torch.from_numpy(lw["ln2"]))
        net.norm_weight.copy_(torch.from_numpy(w["norm"]))
        net.lm_head.load_weight(torch.from_numpy(w["head"]).cuda())
    return net, torch.from_numpy(embed_table(seed)).cuda().to(torch.bfloat16)


def full_forward_logits(net, emb, x, keep, tokens):
    """The full forward (LoRALlamaStack.logits, arange positions) over prompt + the embeddings of `tokens` (B, S), padded
    to a multiple of 64 with masked rows -> the logits (B, S + 1, V) of the last prompt position and of every token."""
    B, T = x.shape[:2]
    S = tokens.shape[1]
    xs = torch.cat([x.cuda().to(torch.bfloat16), emb[tokens.cuda()]], 1)
    ks = torch.cat([keep.cuda().to(torch.uint8), torch.ones((B, S), dtype=torch.uint8, device="cuda")], 1)
    Tp = -(-(T + S) // 64) * 64
    xs = torch.cat([xs, torch.zeros((B, Tp - T - S, xs.shape[2]), dtype=xs.dtype, device="cuda")], 1).contiguous()
    ks = torch.cat([ks, torch.zeros((B, Tp - T - S), dtype=torch.uint8, device="cuda")], 1).contiguous()
    with torch.no_grad():
        lg = net.logits(xs, ks)
    return lg[:, T - 1:T + S].float()
