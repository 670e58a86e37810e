"""CPU: the logic of msr3d_amd/llm/generate.py::rank_answers (closed-set answer ranking on ONE cached copy of each prompt)
against the literal procedure of the reference's MSR3D.predict_answers (every candidate as a full copy of prompt + answer
through the whole model), both on the fp32 transformers fixture model of tests/generate_helpers.py.  fp32 against fp32:
the selections must be identical and the losses agree to 1e-5 (only the summation order differs).  The prompt rows are
unpadded, left-padded and with masked slots INSIDE the prompt; the third is where positions taken from the mask instead of
the slot index give another result.  No GPU."""
import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, embed_table, hf_model, prompt
from tests.predict_helpers import BOS, HFScoreEngine, answer_set, literal_predict_answers

SEED, A, C, S = 0, 40, 16, 8


@pytest.fixture(scope="module")
def case():
    model = hf_model(SEED)
    x, keep = prompt(SEED)
    ids, am = answer_set(SEED, A=A, S=S)
    return model, x, keep, ids, am, literal_predict_answers(model, x, keep, ids, am, C)


def _embed(seed):
    emb = torch.from_numpy(embed_table(seed))
    return lambda t: emb[t]


def test_answer_set_is_a_real_selection_problem(case):
    _, _, _, ids, am, ref = case
    assert ids.shape == (A, S) and A > C
    n = am.sum(1)
    assert int(n.min()) == 2 and int(n.max()) == S and len(set(n.tolist())) > 3          # different lengths, right-padded
    assert bool((am[:, :-1] >= am[:, 1:]).all()) and bool((ids[:, 0] == BOS).all())
    assert ref["topk_ids"].shape == (3, C) and ref["loss"].shape == (3, C)
    assert len({tuple(sorted(r.tolist())) for r in ref["topk_ids"]}) > 1                 # the prompts select differently


def test_rank_answers_equals_the_literal_procedure(case):
    from msr3d_amd.llm.generate import rank_answers
    model, x, keep, ids, am, ref = case
    out = rank_answers(HFScoreEngine(model), _embed(SEED), x, keep, ids, am, num_ans_candidates=C)
    assert torch.equal(out["topk_ids"], ref["topk_ids"])
    assert torch.equal(out["answers_id"], ref["answers_id"])
    assert out["loss"].dtype == torch.float32 and out["answers_id"].dtype == torch.int64
    dev = (out["loss"] - ref["loss"]).abs().max(1)[0]
    print("loss deviation per prompt row:", dev.tolist())
    assert float(dev.max()) <= 1e-5                                    # every row, the one with masked slots included
    assert float((out["first_prob"] - ref["first_prob"]).abs().max()) <= 1e-6


def test_bos_id_appends_the_bos_column(case):
    """bos_id given: the prompt comes without its bos column, rank_answers appends embedding and mask itself."""
    from msr3d_amd.llm.generate import rank_answers
    model, x, keep, ids, am, ref = case
    out = rank_answers(HFScoreEngine(model), _embed(SEED), x[:, :-1], keep[:, :-1], ids, am, num_ans_candidates=C, bos_id=BOS)
    assert torch.equal(out["topk_ids"], ref["topk_ids"]) and torch.equal(out["answers_id"], ref["answers_id"])
    assert float((out["loss"] - ref["loss"]).abs().max()) <= 1e-5


def test_more_candidates_than_answers_ranks_them_all(case):
    from msr3d_amd.llm.generate import rank_answers
    model, x, keep, ids, am, _ = case
    ref = literal_predict_answers(model, x, keep, ids[:10], am[:10], 128)
    out = rank_answers(HFScoreEngine(model), _embed(SEED), x, keep, ids[:10], am[:10], num_ans_candidates=128)
    assert out["topk_ids"].shape == (3, 10) and torch.equal(out["topk_ids"], ref["topk_ids"])
    assert torch.equal(out["answers_id"], ref["answers_id"])
    assert float((out["loss"] - ref["loss"]).abs().max()) <= 1e-5


def test_positions_from_the_mask_miss_the_row_with_masked_slots(case):
    """The control: an engine that rotates by cumsum(mask) - 1 (what `generate` feeds the model) agrees on the unpadded and
    the left-padded row (a constant shift of every position leaves RoPE's relative angles alone) and NOT on the row with
    masked slots inside the prompt -- which is why prefill has positions="arange"."""
    from msr3d_amd.llm.generate import rank_answers
    model, x, keep, ids, am, ref = case
    out = rank_answers(HFScoreEngine(model, force_positions="mask"), _embed(SEED), x, keep, ids, am, num_ans_candidates=C)
    rows = []
    for b in range(3):
        # (the selections may differ on row 2: compare the losses of the answers both selected)
        common = sorted(set(out["topk_ids"][b].tolist()) & set(ref["topk_ids"][b].tolist()))
        lo = {int(a): float(v) for a, v in zip(out["topk_ids"][b], out["loss"][b])}
        lr = {int(a): float(v) for a, v in zip(ref["topk_ids"][b], ref["loss"][b])}
        rows.append(max(abs(lo[a] - lr[a]) for a in common))
    print("loss deviation with positions from the mask:", rows)
    assert rows[0] <= 1e-5 and rows[1] <= 1e-4
    assert rows[2] > 1e-3


def test_refusals(case):
    from msr3d_amd.llm.generate import rank_answers
    model, x, keep, ids, am, _ = case
    eng, emb = HFScoreEngine(model), _embed(SEED)
    bad = ids.clone()
    bad[3, 0] = 5
    with pytest.raises(ValueError, match="same token"):
        rank_answers(eng, emb, x, keep, bad, am, num_ans_candidates=C)
    with pytest.raises(ValueError, match="same token"):
        rank_answers(eng, emb, x[:, :-1], keep[:, :-1], ids, am, num_ans_candidates=C, bos_id=2)
    empty = am.clone()
    empty[7, 1:] = 0
    with pytest.raises(ValueError, match="without a real token"):
        rank_answers(eng, emb, x, keep, ids, empty, num_ans_candidates=C)
    with pytest.raises(ValueError):
        rank_answers(eng, emb, x, keep, ids[:, :1], am[:, :1], num_ans_candidates=C)


def test_fixture_is_the_literal_procedure_and_has_its_margins():
    """tests/golden/predict_answers_seed*.npz: reproduced here from its own inputs, and every prompt row's margins (best
    against second-best loss; C-th against (C+1)-th first-token logit) are at least the recorded 4 x parent deviation."""
    import glob
    import os
    paths = sorted(glob.glob(os.path.join(GOLD, "predict_answers_seed*.npz")))
    assert paths, "no predict_answers fixture"
    for path in paths:
        g = np.load(path)
        seed, Cg = int(g["seed"]), int(g["num_ans_candidates"])
        model = hf_model(seed)
        x, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"].astype(np.int64))
        ids, am = torch.from_numpy(g["answer_ids"]), torch.from_numpy(g["answer_mask"].astype(np.int64))
        ref = literal_predict_answers(model, x, keep, ids, am, Cg)
        assert np.array_equal(ref["topk_ids"].numpy(), g["topk_ids"]) and np.array_equal(ref["answers_id"].numpy(), g["answers_id"])
        assert np.abs(ref["loss"].numpy() - g["loss"]).max() <= 1e-5
        assert np.abs(ref["logits0"].numpy() - g["logits0"]).max() <= 1e-4
        two = np.sort(g["loss"], 1)[:, :2]
        assert ((two[:, 1] - two[:, 0]) >= 4 * float(g["parent_loss_dev"])).all()
        sc = np.sort(g["logits0"][:, g["answer_ids"][:, 1]], 1)[:, ::-1]
        assert ((sc[:, Cg - 1] - sc[:, Cg]) >= 4 * float(g["parent_logit_dev"])).all()
        assert x.shape[0] == 3 and ids.shape[0] > Cg


def test_prefix_attention_entry_validates_without_a_device():
    """msr3d_attn_prefix_fwd: bad arguments give the EINVAL status before anything is launched; empty problems are a no-op."""
    import ctypes

    from msr3d_amd import _lib
    h, null, one = _lib.load(), ctypes.c_void_p(0), ctypes.c_float(1.0)
    call = lambda B, C, S, Tmax, H, D, ld: h.msr3d_attn_prefix_fwd(B, C, S, Tmax, H, D, null, null, null, ld, null, null, null,   # noqa: E731
                                                                   null, null, one, null, ld, null)
    assert call(2, 4, 16, 100, 8, 64, 512) == -22          # null pointers
    assert call(2, 4, 24, 100, 8, 64, 512) == -22          # S outside {16, 32, 64}
    assert call(2, 4, 16, 100, 8, 96, 768) == -22          # head size
    assert call(2, 4, 16, 100, 8, 64, 256) == -22          # row stride below H D
    assert call(2, 4, 16, -1, 8, 64, 512) == -22
    assert call(0, 4, 16, 100, 8, 64, 512) == 0 and call(2, 0, 16, 100, 8, 64, 512) == 0
    assert _lib.ABI_VERSION == h.msr3d_abi_version() >= 31
