"""prompt_cache="shared" (msr3d_amd/llm/generate.py: KVCache layout "shared", msr3d_attn_decode_shared) against the
default "rows" on the existing fixtures (tests/generate_helpers.py: 2 layers, hidden 512, 3 prompts -- one without
padding, one left-padded, one with masked slots inside the prompt).

The contract is bit identity: where the prompt's bytes live changes, no logit does.
A. teacher-forced along the 5-beam transformers fixture (its tokens and beam indices are fed, so the tail reorder is on
   the path): the logits of every step are torch.equal between the two layouts, and within BOUND = 2e-2 rel-L2 of the
   fixture on every row (the bound tests/test_generate_gpu.py puts on the same walk).
B. `net.generate` returns the same tokens under both layouts for beams, sampled captions, beam sampling, merged weights
   and a batch that runs as two prompt_groups.
C. cache.nbytes: prompts x T + 2 sides x rows x new_tokens token-rows under "shared", less than "rows"' 2 x rows x
   (T + new_tokens); with one row per prompt "shared" is the rows layout."""
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import CFG, GOLD, gpu_stack, prompt

pytestmark = pytest.mark.gpu
BOUND = 2e-2


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def seed0():
    """The seed-0 fixture model, built once for the tests that share it."""
    return gpu_stack(0)


def _walk(net, emb, g, beams, prompt_cache):
    """Teacher-forced: -> [logits (N, V) bf16 cuda] per step of the fixture, and the engine."""
    from msr3d_amd.llm.generate import CachedDecoder
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    steps = g["logits"].shape[0]
    eng = CachedDecoder(net, prompt_cache=prompt_cache)
    eng.reserve(beams, steps)
    lg = eng.prefill(x, keep)
    eng.expand(beams)
    out = [lg.repeat_interleave(beams, 0)]
    for s in range(steps - 1):
        out.append(eng.step(emb[torch.from_numpy(g["feed_tokens"][s]).cuda()], torch.from_numpy(g["feed_beam_idx"][s]).cuda()))
    return out, eng


def test_teacher_forced_logits_are_the_rows_layouts_bits_and_match_the_transformers_fixture():
    g = dict(np.load(os.path.join(GOLD, "generate_seed0_beam5.npz"), allow_pickle=False))
    assert int(g["seed"]) == 0
    net, emb = gpu_stack(0)
    shared, eng = _walk(net, emb, g, 5, "shared")
    rows, eng_rows = _walk(net, emb, g, 5, "rows")
    assert eng.cache.layout == "shared" and eng_rows.cache.layout == "rows"
    for s, (a, b) in enumerate(zip(shared, rows)):
        assert torch.equal(a, b), (s, float((a.float() - b.float()).abs().max()))
    ref = torch.from_numpy(g["logits"])
    N = ref.shape[1]
    errs = torch.tensor([[rel(shared[s][n].float(), ref[s, n]) for n in range(N)] for s in range(len(shared))])
    print("A: shared vs the transformers fixture: rel-L2 worst %.5f over %d steps x %d rows" % (float(errs.max()), *errs.shape))
    assert float(errs.max()) < BOUND, errs
    # the tails hold one slot per fed step, the same number in every row and prompt
    steps = len(shared) - 1
    assert eng.cache.tail_len.tolist() == [steps] * 3 and eng.cache.len.tolist() == [steps] * 15
    assert torch.equal(eng.cache.pos, eng_rows.cache.pos)


@pytest.mark.parametrize("kw", [
    dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0),                           # the reference's arguments
    dict(num_beams=2, length_penalty=2.0),
    dict(do_sample=True, top_p=0.9, top_k=50, temperature=1.5, seed=4, num_return_sequences=3),       # sampled captions
    dict(num_beams=3, do_sample=True, top_p=0.95, top_k=50, seed=11, num_return_sequences=2),         # beam sampling
    dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0, lora="merged"),
], ids=["beams5", "beams2_lp2", "captions3", "beam_sampling", "merged"])
def test_generate_returns_the_same_tokens_under_both_layouts(seed0, kw):
    net, emb = seed0
    x, keep = prompt(0)
    x, keep = x.cuda(), keep.cuda()
    a = net.generate(x, keep, emb, max_length=12, min_length=1, prompt_cache="rows", **kw)
    b = net.generate(x, keep, emb, max_length=12, min_length=1, prompt_cache="shared", **kw)
    print("B: %s -> tokens %s under both layouts" % (kw, tuple(a.shape)))
    assert a.shape[0] == 3 * kw.get("num_return_sequences", 1) and 1 <= a.shape[1] <= 12
    assert torch.equal(a, b), (a, b)


def test_a_batch_of_two_prompt_groups_returns_the_same_tokens_under_both_layouts(seed0):
    from msr3d_amd.llm.generate import CachedDecoder, prompt_groups
    net, emb = seed0
    x3, keep3 = prompt(0)
    idx = [i % 3 for i in range(14)]
    x, keep = x3[idx].cuda(), keep3[idx].cuda()
    assert prompt_groups(14, 5, CachedDecoder.max_rows) == [(0, 7), (7, 14)]
    kw = dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0, max_length=8, min_length=1, eos_id=2, pad_id=2)
    a = net.generate(x, keep, emb, prompt_cache="rows", **kw)
    b = net.generate(x, keep, emb, prompt_cache="shared", **kw)
    assert a.shape[0] == 14 and torch.equal(a, b), (a, b)


def test_cache_bytes_follow_the_layout(seed0):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = seed0
    x, keep = prompt(0)
    x, keep = x.cuda(), keep.cuda()
    B, T = keep.shape
    beams, new = 5, 16
    token_row = CFG["layers"] * 2 * CFG["hidden"] * 2                   # K and V of every layer, bf16
    got = {}
    for layout in ("rows", "shared"):
        eng = CachedDecoder(net, prompt_cache=layout)
        eng.reserve(beams, new)
        eng.prefill(x, keep)
        assert eng.cache.layout == layout
        got[layout] = eng.cache.nbytes
    assert got["shared"] == (B * T + 2 * B * beams * new) * token_row
    assert got["rows"] == 2 * B * beams * (T + new) * token_row
    assert got["shared"] < got["rows"]
    # one row per prompt: nothing to share, the rows layout (what `score` reads)
    eng = CachedDecoder(net, prompt_cache="shared")
    eng.reserve(1, new)
    eng.prefill(x, keep)
    assert eng.cache.layout == "rows" and eng.cache.nbytes == B * (T + new) * token_row


def test_unknown_layouts_and_fp8_stacks_are_refused(seed0):
    from msr3d_amd.llm import LoRALlamaStack
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = seed0
    x, keep = prompt(0)
    with pytest.raises(ValueError, match="prompt_cache"):
        net.generate(x.cuda(), keep.cuda(), emb, max_length=2, prompt_cache="pages")
    fp8 = LoRALlamaStack(1, 512, 4, 1024, 1024, device="cuda", base="fp8")
    with pytest.raises(NotImplementedError, match="fp8"):
        CachedDecoder(fp8, prompt_cache="shared")
