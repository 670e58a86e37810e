"""Sampling end to end on the GPU: `search` on the CachedDecoder draws with msr3d_decode_sample (csrc/llm_sample.hip), and
the same run with the draw replaced by its torch statement (torch_sample_scores + torch_sample, fed the noise
msr3d_gumbel_noise writes) must return the same tokens; seeds; MSR3DFullStep.generate's sampling keywords and
num_captions; more than 64 live rows.  Fixture stack: tests/generate_helpers.py::gpu_stack(0), at most 12 new tokens."""
import pytest
import torch

from tests.generate_helpers import gpu_stack, prompt

pytestmark = pytest.mark.gpu
N_NEW = 12
# chosen on an MI355X: with this seed the statement-side run's smallest key gap (what decides a draw) is 1.32e-2 for
# num_beams = 1 and 1.00e-3 for num_beams = 5, against the 1e-4 the test asserts first (seeds 1 and 2 give 1.4e-4 and
# 4.1e-5 at 5 beams: equal tokens too, but no margin to speak of)
SEED = 20261020


@pytest.fixture(scope="module")
def stack():
    net, emb = gpu_stack(0)
    x, keep = prompt(0)
    return net, (lambda ids: emb[ids]), x.cuda(), keep.cuda()


def _search(stack, engine=None, B=None, **kw):
    from msr3d_amd.llm.generate import CachedDecoder, search
    net, embed_fn, x, keep = stack
    if B is not None:
        x, keep = (t.cuda() for t in prompt(0, B=B))
    args = dict(max_length=N_NEW, min_length=0, repetition_penalty=3.0, do_sample=True, top_p=0.9, top_k=50, temperature=1.5)
    args.update(kw)
    return search(engine or CachedDecoder(net), embed_fn, x, keep, **args)


class _StatementSampler:
    """CachedDecoder.sample's signature, computed by the torch statement from the kernel's own noise; keeps the smallest
    gap between keys whose order decides a draw: per prompt, among the k + 1 largest keys of its `rows` live rows."""

    def __init__(self, rows):
        self.rows, self.gap = rows, float("inf")

    def __call__(self, logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, temperature, top_k, top_p,
                 min_keep, k, seed, step, row0, noise=None):
        from msr3d_amd.llm.generate import CachedDecoder, torch_sample, torch_sample_scores
        N, V = logits.shape
        w = torch_sample_scores(logits, prev, repetition_penalty, min_length, eos_id, beam_score, order, temperature, top_k,
                                top_p, min_keep)
        key, val, tok = torch_sample(w, k + 1, CachedDecoder.gumbel_noise(N, V, seed, step, row0, device=logits.device))
        joint = torch.sort(key.view(N // self.rows, -1), dim=1, descending=True)[0][:, :k + 1]
        gap = joint[:, :-1] - joint[:, 1:]
        gap = gap[torch.isfinite(joint[:, :-1]) & torch.isfinite(joint[:, 1:])]
        if gap.numel():
            self.gap = min(self.gap, float(gap.min()))
        return key[:, :k], val[:, :k], tok[:, :k].int()


@pytest.mark.parametrize("beams", [1, 5])
def test_the_kernel_draw_is_its_statement(stack, beams):
    from msr3d_amd.llm.generate import CachedDecoder
    net = stack[0]
    got = _search(stack, num_beams=beams, seed=SEED)
    eng = CachedDecoder(net)
    eng.sample = _StatementSampler(beams)
    want = _search(stack, engine=eng, num_beams=beams, seed=SEED)
    print("sampling, num_beams", beams, "seed", SEED, "smallest key gap", eng.sample.gap, "tokens", got.tolist())
    assert eng.sample.gap >= 1e-4, eng.sample.gap          # a precondition of the comparison: it fails loudly
    assert got.dtype == torch.int64 and got.shape == want.shape and torch.equal(got, want), (got, want)
    assert int(got.min()) >= 0


def test_the_seed_decides_the_tokens(stack):
    for beams, n in ((1, 2), (2, 2)):
        a = _search(stack, num_beams=beams, num_return_sequences=n, seed=5)
        b = _search(stack, num_beams=beams, num_return_sequences=n, seed=5)
        c = _search(stack, num_beams=beams, num_return_sequences=n, seed=6)
        assert a.shape[0] == 3 * n and torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(3)
    a = _search(stack)
    torch.manual_seed(3)
    assert torch.equal(a, _search(stack))                  # seed=None: 63 bits from torch's CPU generator


def test_more_than_64_live_rows(stack):
    """14 prompts x 5 samples run as two groups of 7 prompts; the first 7 prompts alone are the first group: the draw is
    told every group's first global row, so the first 35 rows are the same tokens."""
    kw = dict(num_return_sequences=5, seed=77, max_length=8, min_length=8)
    both = _search(stack, B=14, **kw)
    first = _search(stack, B=7, **kw)
    assert both.shape == (70, 8) and first.shape == (35, 8)
    assert torch.equal(both[:35], first)
    assert len({tuple(r) for r in both[:5].tolist()}) > 1  # a prompt's samples are not one sample five times


# --------------------------------------------------------------------------------------------- MSR3DFullStep.generate
@pytest.fixture(scope="module")
def full():
    from tests.test_generate_full_gpu import _model
    model, batch, c = _model()
    model.eval()
    return model, batch, c


MAX_OUT = 24


def test_top_k_1_sampling_is_greedy_search(full, monkeypatch):
    from msr3d_amd.llm.generate import CachedDecoder
    model, batch, c = full
    seen = []
    select = CachedDecoder.select

    def spy(self, logits, *a, **kw):
        seen.append(logits.float())
        return select(self, logits, *a, **kw)

    # Twelve tokens.  At the fourth step of this model's greedy run row 0's two leading logits are one bf16 value (2.6562)
    # -- the case the precondition below exists to exclude -- so row 0's own third token serves as eos (as
    # tests/test_generate_search_cpu.py::_early_eos picks one): row 0 ends after three tokens and goes on as padding, the
    # other row runs all twelve steps, and sampling is also seen to end a row and pad it as greedy search does.
    kw = dict(num_beams=1, max_length=12, max_out_len=MAX_OUT, min_length=1, repetition_penalty=3.0)
    eos = int(model.generate(dict(batch), use_nucleus_sampling=False, **kw)["output_tokens"][0, 2])
    kw["eos_id"] = eos
    monkeypatch.setattr(CachedDecoder, "select", spy)
    greedy = model.generate(dict(batch), use_nucleus_sampling=False, **kw)["output_tokens"]
    monkeypatch.setattr(CachedDecoder, "select", select)
    assert len(seen) == 12 and bool((greedy[0, 2:12] == eos).all()) and not bool((greedy[1:, :11] == eos).any())
    # with two leaders exactly equal both would stay under top_k = 1 and the draw would choose between them
    for t, lg in enumerate(seen):
        live = (greedy[:, :t] != eos).all(1)                # rows that had not ended before step t
        top2 = torch.topk(lg, 2, dim=-1)[0]
        assert bool((top2[live, 0] > top2[live, 1]).all()), ("a tie between the two leaders at step", t)
    for seed in (0, 1):
        drawn = model.generate(dict(batch), use_nucleus_sampling=True, top_k=1, seed=seed, **kw)["output_tokens"]
        assert torch.equal(drawn, greedy), (drawn, greedy)


def test_num_captions_and_the_defaults(full):
    model, batch, c = full
    B = c["B"]
    kw = dict(max_length=12, max_out_len=MAX_OUT)
    out = model.generate(dict(batch), use_nucleus_sampling=True, num_beams=1, num_captions=3, temperature=1.5, seed=4,
                         **kw)["output_tokens"]
    assert out.shape == (3 * B, MAX_OUT) and out.dtype == torch.int64 and not bool((out == 0).any())
    per_prompt = out.view(B, 3, MAX_OUT)
    assert any(not torch.equal(p[0], p[1]) or not torch.equal(p[0], p[2]) for p in per_prompt)     # not all equal
    again = model.generate(dict(batch), use_nucleus_sampling=True, num_beams=1, num_captions=3, temperature=1.5, seed=4,
                           **kw)["output_tokens"]
    assert torch.equal(out, again)
    for row in out.cpu():                                   # the same padding: everything after the first 2 is 2
        ends = (row == 2).nonzero()
        if len(ends):
            assert bool((row[int(ends[0]):] == 2).all())
    # the n best beams: the best one is what num_captions = 1 returns
    best = model.generate(dict(batch), **kw)["output_tokens"]
    two = model.generate(dict(batch), num_captions=2, **kw)["output_tokens"]
    assert two.shape == (2 * B, MAX_OUT) and torch.equal(two[0::2], best)
    # the defaults are the call as it was: the old arguments spelled out
    old = model.generate(dict(batch), num_beams=5, max_length=12, min_length=1, repetition_penalty=3.0, length_penalty=1.0,
                         max_out_len=MAX_OUT, bos_id=1, eos_id=2)["output_tokens"]
    assert best.shape == (B, MAX_OUT) and torch.equal(best, old)
