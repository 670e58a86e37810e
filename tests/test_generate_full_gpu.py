"""F. End to end: MSR3DFullStep.generate on the configuration of tests/golden/full_step_seed0.npz -- hot path, prompt
embeddings with the scene tokens scattered in, bos embedding, KV-cached search, the reference's post-processing."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_OUT = 24


def _model(base="bf16"):
    from tests.test_full_step_gpu import build_model, make_batch
    g = dict(np.load(os.path.join(GOLD, "full_step_seed0.npz"), allow_pickle=False))
    model, c = build_model(g, base=base)
    return model, make_batch(g, c), c


def _check_tokens(tok, B):
    assert tok.shape == (B, MAX_OUT) and tok.dtype == torch.int64
    assert not bool((tok == 0).any())
    t = tok.cpu()
    for row in t:
        ends = (row == 2).nonzero()
        if len(ends):
            assert bool((row[int(ends[0]):] == 2).all())          # everything after the first 2 is 2


def test_generate_end_to_end_and_the_model_is_left_as_it_was(monkeypatch):
    """The two training steps run with ordered reductions (hipops' deterministic mode, as
    tests/test_train_step_gpu.py::test_deterministic_mode_gives_bit_identical_weights sets it): in the default mode the
    hot path's split-K sums meet by float atomics and the same step on the same weights already differs in its last bits
    from run to run, so "the same loss bits" would say nothing about generate.  generate switches that mode on for its own
    hot-path forward."""
    import torch.nn.functional as F

    from msr3d_amd import hipops
    from msr3d_amd.full_step import FullTrainStep
    monkeypatch.setattr(hipops, "_deterministic", [True])
    from msr3d_amd.model.scene_embeds import MSR3DHotPath, scatter_scene_embeds_
    model, batch, c = _model()
    ts = FullTrainStep(model, lr=0.0, weight_decay=0.0, zero_in_optimizer=False)
    loss0 = ts(dict(batch)).detach().clone()
    model.eval()
    kw = dict(max_length=16, max_out_len=MAX_OUT, min_length=1, repetition_penalty=3.0, length_penalty=1.0)
    greedy = model.generate(dict(batch), num_beams=1, **kw)["output_tokens"]
    beam = model.generate(dict(batch), num_beams=5, **kw)["output_tokens"]
    print("F: greedy", greedy[:, :16].tolist(), "beams", beam[:, :16].tolist())
    _check_tokens(greedy, c["B"])
    _check_tokens(beam, c["B"])
    assert torch.equal(model.generate(dict(batch), num_beams=1, **kw)["output_tokens"], greedy)     # a second call
    assert torch.equal(model.generate(dict(batch), num_beams=5, **kw)["output_tokens"], beam)
    # the same embeddings straight into the stack
    with torch.no_grad():
        d = MSR3DHotPath.forward(model, dict(batch))
        ids = batch["input_ids"].contiguous()
        am = batch["attention_mask"].to(torch.int64).contiguous().clone()
        emb = F.embedding(ids, model.embed_tokens).contiguous()
        scatter_scene_embeds_(emb, am, ids, d["scene_embeds"].detach(), d["obj_masks"], model.scene_sp_token)
        assert int((am == 0).sum()) > 0                             # masked object slots sit INSIDE the prompt
        out = model.llm_model.generate(emb, am, model.embed_tokens, bos_id=1, eos_id=2, pad_id=2, num_beams=1, max_length=16,
                                       min_length=1, repetition_penalty=3.0, length_penalty=1.0)
    out = torch.where(out == 0, torch.full_like(out, 2), out)
    assert torch.equal(greedy[:, :out.shape[1]], out) and bool((greedy[:, out.shape[1]:] == 2).all())
    model.train()
    loss1 = ts(dict(batch)).detach()
    print("F: loss before / after", float(loss0), float(loss1))
    assert torch.equal(loss0, loss1), (loss0, loss1)                # nothing of the model was modified


def test_generate_refuses_fp8_base_weights():
    model, batch, _ = _model(base="fp8")
    model.eval()
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate(dict(batch), num_beams=1, max_length=4, max_out_len=8)
