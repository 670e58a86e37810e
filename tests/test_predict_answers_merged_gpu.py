"""lora="merged" for closed-set answer ranking: tests/test_predict_answers_gpu.py::test_fixture_ranking's three
assertions on the merged planes (the selected sets, the winners, the loss within 2 x parent_loss_dev of the fp32
fixture), and MSR3DFullStep.generate / .predict_answers end to end with lora="merged" on the configuration of
tests/golden/full_step_seed0.npz.
Measured on an MI355X (printed): the loss deviates from the fp32 fixture by at most 0.018441 / 0.016574 / 0.022210 on the
three prompt rows, against the bound 2 x parent_loss_dev = 0.048088; sets and winners are the fixture's."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, gpu_stack
from tests.predict_helpers import answer_set

pytestmark = pytest.mark.gpu


def test_fixture_ranking_on_merged_weights():
    paths = sorted(glob.glob(os.path.join(GOLD, "predict_answers_seed*.npz")))
    assert paths, "the predict_answers fixture is missing"
    g = dict(np.load(paths[0], allow_pickle=False))
    net, emb = gpu_stack(int(g["seed"]))
    x, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"].astype(np.int64))
    ids, am = torch.from_numpy(g["answer_ids"]), torch.from_numpy(g["answer_mask"].astype(np.int64))
    C = int(g["num_ans_candidates"])
    out = net.predict_answers(x.cuda(), keep.cuda(), emb, ids.cuda(), am.cuda(), num_ans_candidates=C, lora="merged")
    top, loss = out["topk_ids"].cpu(), out["loss"].cpu()
    ref_top, ref_loss = torch.from_numpy(g["topk_ids"]), torch.from_numpy(g["loss"])
    B = x.shape[0]
    aligned = torch.stack([torch.tensor([float(loss[b][top[b] == a][0]) if bool((top[b] == a).any()) else float("nan")
                                         for a in ref_top[b]]) for b in range(B)])
    print("R (merged): rank_answers against the fixture: loss max abs deviation per prompt row %s (bound 2 x %.6f); answers "
          "%s (fixture %s)" % ([round(float(v), 6) for v in (aligned - ref_loss).abs().max(1)[0]], float(g["parent_loss_dev"]),
                               out["answers_id"].tolist(), g["answers_id"].tolist()))
    for b in range(B):                                               # membership: the order inside the top C means nothing
        assert sorted(top[b].tolist()) == sorted(ref_top[b].tolist()), b
    assert out["answers_id"].cpu().tolist() == g["answers_id"].tolist()
    assert float((aligned - ref_loss).abs().max()) <= 2 * float(g["parent_loss_dev"])


def test_full_step_generate_and_predict_answers_end_to_end_on_merged_weights():
    from tests.test_full_step_gpu import build_model, make_batch
    g = dict(np.load(os.path.join(GOLD, "full_step_seed0.npz"), allow_pickle=False))
    model, c = build_model(g)
    batch = make_batch(g, c)
    model.eval()
    kw = dict(max_length=12, max_out_len=16, min_length=1, repetition_penalty=3.0, length_penalty=1.0, lora="merged")
    for beams in (1, 5):
        tok = model.generate(dict(batch), num_beams=beams, **kw)["output_tokens"]
        assert tok.shape == (c["B"], 16) and tok.dtype == torch.int64 and tok.is_cuda
        assert int(tok.min()) >= 1 and int(tok.max()) < c["vocab"]                   # (id 0 is mapped to 2)
        assert torch.equal(model.generate(dict(batch), num_beams=beams, **kw)["output_tokens"], tok)
    ids, am = answer_set(5, A=24, S=6, vocab=c["vocab"])
    d = model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, lora="merged")
    a = d["answers_id"]
    assert a.shape == (c["B"],) and a.dtype == torch.int64 and a.is_cuda
    assert int(a.min()) >= 0 and int(a.max()) < 24
    assert d["answers_topk_ids"].shape == (c["B"], 8) and d["answers_topk_ids"].dtype == torch.int64
    assert int(d["answers_topk_ids"].min()) >= 0 and int(d["answers_topk_ids"].max()) < 24
    assert d["answers_loss"].shape == (c["B"], 8) and d["answers_loss"].dtype == torch.float32
    assert bool(torch.isfinite(d["answers_loss"]).all())
    d2 = model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, lora="merged")
    assert torch.equal(d2["answers_id"], a) and torch.equal(d2["answers_loss"], d["answers_loss"])
    with pytest.raises(ValueError, match="lora"):
        model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, lora="both")
