"""KV-cached decoding on 33 .. 64 live rows, and batches beyond that (msr3d_amd/llm/generate.py on the wide skinny
product of csrc/llm_decode.hip).  The fixtures of tests/test_generate_gpu.py, tiled: every kernel of a step computes a
row from that row alone, in an order that does not depend on the row's index, so a copy of a prompt must give what the
prompt gives -- within `BOUND` of the fp32 fixture where logits are compared (the bound of tests/test_generate_gpu.py),
token for token where tokens are.

D45 / D36. teacher-forced: the 5-beam fixture 3 x (45 rows; fed tokens tiled, beam indices offset by 15 per copy, so the
    cache reorder runs across all 45 rows) and the greedy fixture 12 x (36 rows): every step, every row within rel-L2
    2e-2 of the fixture's logits.  Before the row limit was raised these stopped in `prefill`.
E34. free-running: the gap fixture (every step decided by >= 4 x the measured deviation) 17 x = 34 rows: every copy
    gives the fixture's tokens.
B35 / B60. beam search on 7 and 12 prompts x 5 beams: a second call gives the same tokens, and copies of one prompt
    inside a call give the same tokens as one another.
G. 14 prompts x 5 beams = 70 rows runs as prompt_groups(14, 5, 64) = two groups of 7: equal, bit for bit, to generate
    on each range, padded; 13 greedy prompts are one group and give the gap fixture's tokens.
F40. MSR3DFullStep.generate on the full-step fixture's batch 4 x (8 prompts x 5 beams): shape, no id 0, 2s after the
    first 2, every copy equal to the untiled call."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, gpu_stack, prompt

pytestmark = pytest.mark.gpu
BOUND = 2e-2
BEAM_KW = dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0, max_length=12, min_length=1)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


@pytest.fixture(scope="module")
def seed0():
    """The seed-0 fixture model, built once for the tests that share it."""
    return gpu_stack(0)


def _gap_fixtures():
    paths = sorted(glob.glob(os.path.join(GOLD, "generate_gap_seed*.npz")))
    assert paths, "the free-running fixture is missing"
    return [dict(np.load(p, allow_pickle=False)) for p in paths]


def _gap_generate(net, emb, g, idx):
    """net.generate with the gap fixture's arguments on its prompts `idx` (a list of fixture rows, repeats allowed)."""
    x, keep = torch.from_numpy(g["x"]).cuda()[idx], torch.from_numpy(g["keep"]).cuda()[idx]
    out = net.generate(x, keep, emb, eos_id=int(g["eos"]), pad_id=int(g["eos"]), num_beams=1, max_length=g["sequences"].shape[1],
                       min_length=0, repetition_penalty=float(g["repetition_penalty"]))
    assert out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("name,beams,copies", [("generate_seed0_beam5.npz", 5, 3), ("generate_seed0_greedy.npz", 1, 12)])
def test_teacher_forced_logits_of_tiled_prompts_match_the_fixture_on_every_row(seed0, name, beams, copies):
    from msr3d_amd.llm.generate import CachedDecoder
    g = _load(name)
    assert int(g["seed"]) == 0
    net, emb = seed0
    B = g["x"].shape[0]
    per = B * beams                                                      # live rows of one copy
    rows = per * copies
    assert 32 < rows <= CachedDecoder.max_rows
    x = torch.from_numpy(g["x"]).cuda().repeat(copies, 1, 1)
    keep = torch.from_numpy(g["keep"]).cuda().repeat(copies, 1)
    steps = g["logits"].shape[0]
    ref = torch.from_numpy(g["logits"]).repeat(1, copies, 1)             # (steps, rows, V)
    eng = CachedDecoder(net)
    eng.reserve(beams, steps)
    lg = eng.prefill(x, keep)
    eng.expand(beams)
    got = [lg.repeat_interleave(beams, 0).float().cpu()]
    for s in range(steps - 1):
        if beams == 1:
            lg = eng.step(emb[torch.from_numpy(g["sequences"][:, s]).cuda().repeat(copies)])
        else:
            tok = torch.from_numpy(g["feed_tokens"][s]).cuda().repeat(copies)
            idx = torch.from_numpy(g["feed_beam_idx"][s]).cuda().repeat(copies)
            idx = idx + per * torch.arange(copies, device="cuda").repeat_interleave(per).to(idx.dtype)
            lg = eng.step(emb[tok], idx)
        assert lg.shape[0] == rows
        got.append(lg.float().cpu())
    errs = torch.tensor([[rel(got[s][n], ref[s, n]) for n in range(rows)] for s in range(steps)])
    print("D%d: %s x %d: rel-L2 worst %.5f over %d steps x %d rows" % (rows, name, copies, float(errs.max()), steps, rows))
    assert float(errs.max()) < BOUND, errs
    # and a copy's rows carry the bits of the first copy's rows: a row is computed from that row alone
    for s in range(steps):
        assert torch.equal(got[s].view(copies, per, -1), got[s][:per].expand(copies, per, -1)), s


def test_free_running_copies_of_the_gap_fixture_above_32_rows_give_its_tokens():
    for g in _gap_fixtures():
        assert float(g["gaps"].min()) >= float(g["m_gap"]) == 4 * float(g["parent_dev"])
        net, emb = gpu_stack(int(g["seed"]))
        B = g["x"].shape[0]
        copies = 32 // B + 1                                             # the smallest row count above 32
        out = _gap_generate(net, emb, g, list(range(B)) * copies)
        assert out.shape[0] == B * copies > 32
        assert np.array_equal(out, np.tile(g["sequences"], (copies, 1))), (out, g["sequences"])


@pytest.mark.parametrize("prompts", [7, 12])
def test_beam_search_on_35_and_60_rows_repeats_and_copies_of_a_prompt_agree(seed0, prompts):
    net, emb = seed0
    x3, keep3 = prompt(0)
    idx = [i % 3 for i in range(prompts)]
    x, keep = x3[idx].cuda(), keep3[idx].cuda()
    a = net.generate(x, keep, emb, **BEAM_KW)
    b = net.generate(x, keep, emb, **BEAM_KW)
    assert a.shape[0] == prompts and 1 <= a.shape[1] <= 12 and torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < emb.shape[0]
    for i in range(3, prompts):
        assert torch.equal(a[i], a[i % 3]), (i, a[i], a[i % 3])


def test_a_batch_of_70_rows_runs_in_groups_and_equals_generate_on_each_group(seed0):
    from msr3d_amd.llm.generate import CachedDecoder, prompt_groups
    net, emb = seed0
    x3, keep3 = prompt(0)
    idx = [i % 3 for i in range(14)]
    x, keep = x3[idx].cuda(), keep3[idx].cuda()
    groups = prompt_groups(14, 5, CachedDecoder.max_rows)
    assert groups == [(0, 7), (7, 14)]
    kw = dict(BEAM_KW, eos_id=2, pad_id=2)
    whole = net.generate(x, keep, emb, **kw)
    parts = [net.generate(x[a:b], keep[a:b], emb, **kw) for a, b in groups]
    width = max(p.shape[1] for p in parts)
    want = torch.cat([torch.nn.functional.pad(p, (0, width - p.shape[1]), value=2) for p in parts], 0)
    assert whole.shape == want.shape and torch.equal(whole, want), (whole, want)


def test_13_greedy_prompts_are_one_group_and_give_the_gap_fixtures_tokens():
    from msr3d_amd.llm.generate import CachedDecoder, prompt_groups
    assert prompt_groups(13, 1, CachedDecoder.max_rows) == [(0, 13)]
    for g in _gap_fixtures():
        net, emb = gpu_stack(int(g["seed"]))
        B = g["x"].shape[0]
        idx = [i % B for i in range(13)]
        assert np.array_equal(_gap_generate(net, emb, g, idx), g["sequences"][idx])


def test_more_live_rows_than_max_rows_are_refused_by_prefill_with_the_number(seed0):
    from msr3d_amd.llm.generate import CachedDecoder
    net, _ = seed0
    x3, keep3 = prompt(0)
    eng = CachedDecoder(net)
    assert eng.max_rows == 64
    eng.reserve(5, 4)
    with pytest.raises(ValueError, match="at most 64 live rows"):
        eng.prefill(x3[[0] * 13].cuda(), keep3[[0] * 13].cuda())


def test_full_step_generate_on_8_prompts_of_5_beams_equals_the_untiled_call():
    from tests.test_full_step_gpu import build_model, make_batch
    max_out = 24
    g = dict(np.load(os.path.join(GOLD, "full_step_seed0.npz"), allow_pickle=False))
    model, c = build_model(g)
    batch = make_batch(g, c)
    model.eval()
    B = c["B"]
    copies = 8 // B
    assert B * copies == 8
    tiled = {k: (torch.cat([v] * copies, 0) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B else v)
             for k, v in batch.items()}
    assert tiled["input_ids"].shape[0] == 8
    kw = dict(num_beams=5, max_length=16, max_out_len=max_out, min_length=1, repetition_penalty=3.0, length_penalty=1.0)
    one = model.generate(dict(batch), **kw)["output_tokens"]
    tok = model.generate(tiled, **kw)["output_tokens"]
    print("F40: untiled", one[:, :16].tolist(), "tiled", tok[:, :16].tolist())
    assert tok.shape == (8, max_out) and tok.dtype == torch.int64
    assert not bool((tok == 0).any())
    for row in tok.cpu():
        ends = (row == 2).nonzero()
        if len(ends):
            assert bool((row[int(ends[0]):] == 2).all())              # everything after the first 2 is 2
    assert torch.equal(tok, one.repeat(copies, 1)), (tok, one)
