"""checkpoint.hf_state_dict(stack, embed, merged=True): the merged planes bf16(W + s B A) under plain Hugging Face keys
load into an fp32 LlamaForCausalLM that needs no peft and computes the adapted model: its logits on the fixture prompt
against the fixture's own transformers model (peft's formula on separate fp32 A / B), over the unmasked rows, within
rel-L2 1e-2 -- twice the 0.0051 that rounding the merged weights to bf16 costs on the host (the GPU merge differs from
the host's only inside the tie window of tests/test_lora_merge_gpu.py)."""
import pytest
import torch

from tests.generate_helpers import CFG, gpu_stack, hf_model, prompt

pytestmark = pytest.mark.gpu


def test_merged_state_dict_is_a_plain_llama_checkpoint_of_the_adapted_model():
    from transformers.models.llama.modeling_llama import LlamaConfig, LlamaForCausalLM

    from msr3d_amd.llm.checkpoint import hf_state_dict
    seed, c = 0, CFG
    net, emb = gpu_stack(seed)
    sd = hf_state_dict(net, emb, merged=True)
    assert not any("lora_" in k for k in sd)
    plain = hf_state_dict(net, emb)
    assert sorted(sd) == sorted(plain)
    changed = [k for k in sd if not torch.equal(sd[k], plain[k])]
    assert len(changed) == 7 * c["layers"] and all("_proj.weight" in k for k in changed)
    cfg = LlamaConfig(hidden_size=c["hidden"], num_attention_heads=c["heads"], num_key_value_heads=c["heads"],
                      intermediate_size=c["inter"], num_hidden_layers=c["layers"], vocab_size=c["vocab"],
                      rms_norm_eps=c["eps"], rope_theta=c["theta"], max_position_embeddings=256, attention_bias=False,
                      mlp_bias=False, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    model = LlamaForCausalLM(cfg).float().eval()
    missing, unexpected = model.load_state_dict({k: v.float().cpu() for k, v in sd.items()}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    x, keep = prompt(seed)
    ref_model = hf_model(seed)
    with torch.no_grad():
        got = model(inputs_embeds=x, attention_mask=keep).logits
        ref = ref_model(inputs_embeds=x, attention_mask=keep).logits
    rows = keep.bool()
    err = float((got[rows].double() - ref[rows].double()).norm() / ref[rows].double().norm())
    print("merged checkpoint in fp32 transformers against the peft-formula model: rel-L2 %.5f over %d rows, max abs %.4f"
          % (err, int(rows.sum()), float((got[rows] - ref[rows]).abs().max())))
    assert err <= 1e-2
    # and the default export is unchanged by the keyword: the frozen weights themselves
    assert torch.equal(plain["model.layers.0.self_attn.q_proj.weight"], net.layers[0].self_attn["q_proj"].weight)
