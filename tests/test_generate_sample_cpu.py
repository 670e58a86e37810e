"""Sampling in `search` (msr3d_amd/llm/generate.py) against transformers' own `generate(do_sample=True)`, exactly, on
the CPU: with draw="multinomial" `search` calls torch.multinomial where transformers does, so under one torch.manual_seed
both consume the generator alike and the tokens must be EQUAL (fp32 on both sides, tests/generate_helpers.py::HFEngine).
Then the statement of the draw kernel piece by piece: the kept set of `torch_sample_scores` against transformers'
warpers, the tie rule, the counter noise (`counter_uniform_bits`, a pure integer function), and that a prompt's sampled
tokens do not depend on how `prompt_groups` cut the batch."""
import math
import warnings

import pytest
import torch

from tests.generate_helpers import HFEngine, embed_table, hf_generate, hf_model, prompt

warnings.filterwarnings("ignore")
N_NEW = 12


@pytest.fixture(scope="module")
def case():
    model = hf_model(0)
    emb = torch.from_numpy(embed_table(0))
    x, keep = prompt(0)
    return model, (lambda ids: emb[ids]), x, keep


@pytest.fixture(scope="module")
def early_eos(case):
    """tests/test_generate_search_cpu.py::_early_eos: a token the greedy run emits in row 0 at step 5."""
    model, _, x, keep = case
    return int(hf_generate(model, x, keep, 24)[0, 5])


def _hf_sample(model, x, keep, seed, num_beams, n, temperature, top_k, eos, min_length, top_p=0.9, do_sample=True):
    from transformers import GenerationConfig
    gc = GenerationConfig(do_sample=do_sample, num_beams=num_beams, num_return_sequences=n, max_new_tokens=N_NEW,
                          min_new_tokens=min_length or None, repetition_penalty=3.0, length_penalty=1.0, eos_token_id=eos,
                          pad_token_id=eos, bos_token_id=1, use_cache=True, return_dict_in_generate=True,
                          **(dict(temperature=temperature, top_k=top_k, top_p=top_p) if do_sample else {}))
    torch.manual_seed(seed)
    with torch.no_grad():
        return model.generate(inputs_embeds=x, attention_mask=keep, generation_config=gc).sequences


def _ours(case, seed, num_beams, n, temperature, top_k, eos, min_length):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    torch.manual_seed(seed)
    return search(HFEngine(model), embed_fn, x, keep, eos_id=eos, pad_id=eos, num_beams=num_beams, max_length=N_NEW,
                  min_length=min_length, repetition_penalty=3.0, do_sample=True, top_p=0.9, top_k=top_k,
                  temperature=temperature, num_return_sequences=n, draw="multinomial")


# every value of every factor, beams 1 with n in {1, 3} and beams {2, 5} with n in {1, 2}, over three seeds
CASES = [
    # seed, beams, n, temperature, top_k, min_length
    (0, 1, 1, 0.7, 0, 0), (1, 1, 3, 1.5, 50, 3), (2, 1, 3, 0.7, 50, 0), (0, 1, 1, 1.5, 0, 3),
    (0, 2, 1, 0.7, 50, 0), (1, 2, 2, 1.5, 0, 3), (2, 2, 2, 0.7, 0, 0),
    (0, 5, 1, 1.5, 50, 3), (1, 5, 2, 0.7, 50, 0), (2, 5, 2, 1.5, 50, 3), (2, 5, 1, 0.7, 50, 0),
    # the pure nucleus with five beams, and beam sampling under min_length at the lower temperature
    (1, 5, 2, 1.5, 0, 0), (0, 5, 1, 0.7, 0, 3), (2, 2, 1, 0.7, 50, 3), (1, 5, 1, 0.7, 50, 3),
]


@pytest.mark.parametrize("seed,beams,n,temperature,top_k,min_length", CASES)
def test_sampling_equals_transformers(case, early_eos, seed, beams, n, temperature, top_k, min_length):
    model, _, x, keep = case
    ref = _hf_sample(model, x, keep, seed, beams, n, temperature, top_k, early_eos, min_length)
    got = _ours(case, seed, beams, n, temperature, top_k, early_eos, min_length)
    assert got.dtype == torch.int64 and got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.equal(got, ref), (got, ref)
    assert got.shape[0] == x.shape[0] * n


def test_beam_search_returns_the_n_best(case, early_eos):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    for eos in (2, early_eos):
        ref = _hf_sample(model, x, keep, 0, 5, 2, None, None, eos, 0, do_sample=False)
        got = search(HFEngine(model), embed_fn, x, keep, eos_id=eos, pad_id=eos, num_beams=5, max_length=N_NEW, min_length=0,
                     repetition_penalty=3.0, num_return_sequences=2)
        assert got.shape == ref.shape == (2 * x.shape[0], ref.shape[1]) and torch.equal(got, ref), (got, ref)


# ------------------------------------------------------------------------------------------------ the kept set
def _hf_kept(s, temperature, top_k, top_p, min_keep):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = TemperatureLogitsWarper(temperature)(None, s)
    if top_k > 0:
        s = TopKLogitsWarper(top_k, min_tokens_to_keep=min_keep)(None, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p, min_tokens_to_keep=min_keep)(None, s)
    return s > -math.inf


@pytest.mark.parametrize("V", [50, 1000])
@pytest.mark.parametrize("min_keep", [1, 2])
def test_the_kept_set_is_transformers_warpers(V, min_keep):
    from msr3d_amd.llm.generate import torch_sample_scores
    g = torch.Generator().manual_seed(V + min_keep)
    x = 3.0 * torch.randn((16, V), generator=g)
    x[0, 7] += 40.0                                         # one token alone exceeds top_p
    prev = torch.zeros((16, 0), dtype=torch.int64)
    for order in (0, 1):
        for temperature, top_k, top_p in ((0.7, 0, 0.9), (1.5, 50, 0.9), (0.7, 20, 1.0), (1.5, 0, 0.5), (1.0, 0, 1.0)):
            w = torch_sample_scores(x, prev, 1.0, 0, -1, None, order, temperature, top_k, top_p, min_keep)
            base = x if order == 0 else torch.log_softmax(x, dim=-1)
            want = _hf_kept(base, temperature, top_k, top_p, min_keep)
            assert torch.equal(w > -math.inf, want), (order, temperature, top_k, top_p)
            if top_p < 1.0:
                assert int((w[0] > -math.inf).sum()) == min_keep
            if order == 0:                                  # renormalised over the kept set
                assert torch.allclose(torch.exp(w).sum(-1), torch.ones(16), atol=1e-5)


def test_ties_at_the_cut_go_by_token_id():
    """Eight equal scores straddle the cut: the lower ids are removed first, min_keep protects the higher ids."""
    from msr3d_amd.llm.generate import torch_sample_scores
    V = 16
    x = torch.full((1, V), -30.0)
    tied = [1, 3, 4, 6, 9, 10, 12, 15]
    x[0, tied] = 0.0                                        # eight tokens of probability 1/8 each
    prev = torch.zeros((1, 0), dtype=torch.int64)
    # 1 - top_p = 0.45: the running mass reaches 1/8, 2/8, 3/8 <= 0.45 < 4/8 -- three of the eight go, the lowest ids
    w = torch_sample_scores(x, prev, 1.0, 0, -1, None, 0, 1.0, 0, 0.55, 1)
    assert torch.nonzero(w[0] > -math.inf)[:, 0].tolist() == tied[3:]
    assert torch.allclose(w[0, tied[3:]], torch.full((5,), -math.log(5.0)), atol=1e-6)
    # top_p so small that everything would go: min_keep keeps the highest ids of the tie
    for min_keep in (1, 2):
        w = torch_sample_scores(x, prev, 1.0, 0, -1, None, 1, 1.0, 0, 1e-4, min_keep)
        assert torch.nonzero(w[0] > -math.inf)[:, 0].tolist() == tied[-min_keep:]
    # top_k ties at the k-th value all stay
    w = torch_sample_scores(x, prev, 1.0, 0, -1, None, 0, 1.0, 3, 1.0, 1)
    assert torch.nonzero(w[0] > -math.inf)[:, 0].tolist() == tied


# ------------------------------------------------------------------------------------------------ the counter draw
def test_counter_uniform_bits_is_a_pure_function():
    from msr3d_amd.llm.generate import counter_uniform_bits
    a = counter_uniform_bits(1234567890123, 3, 5, 4, 33)
    assert a.dtype == torch.int64 and a.shape == (4, 33) and int(a.min()) >= 0 and int(a.max()) < 1 << 24
    assert torch.equal(a, counter_uniform_bits(1234567890123, 3, 5, 4, 33))
    # a row is its global index: the same bits whatever the call's first row and row count
    assert torch.equal(a[2:], counter_uniform_bits(1234567890123, 3, 7, 2, 33))
    assert not torch.equal(a, counter_uniform_bits(1234567890123, 4, 5, 4, 33))
    assert not torch.equal(a, counter_uniform_bits(1234567890124, 3, 5, 4, 33))
    assert not torch.equal(a, counter_uniform_bits(1234567890123 + (1 << 40), 3, 5, 4, 33))
    pinned = [int(counter_uniform_bits(0, 0, 0, 1, 1)[0, 0]), int(a[0, 0]), int(a[3, 32])]
    assert pinned == PINNED_BITS, pinned


# (seed 0, step 0, row 0, token 0), (seed 1234567890123, step 3, row 5, token 0), (the same seed and step, row 8, token 32):
# worked out by hand with Python integers from the mixer's definition
PINNED_BITS = [12107414, 10862749, 3912706]


def test_counter_draw_frequencies():
    """20 000 rows of one V = 32 distribution, one draw each: every token's count within 5 sigma (+ 1) of N p."""
    from msr3d_amd.llm.generate import counter_uniform_bits, gumbel_from_bits, torch_sample
    N, V = 20000, 32
    p = torch.softmax(torch.linspace(-2.0, 2.0, V, dtype=torch.float64), 0)
    w = torch.log(p)[None].expand(N, V).contiguous()
    _, val, tok = torch_sample(w, 1, gumbel_from_bits(counter_uniform_bits(99, 0, 0, N, V)))
    assert torch.equal(val[:, 0], w[0][tok[:, 0]])
    count = torch.bincount(tok[:, 0], minlength=V).double()
    bound = 5.0 * torch.sqrt(N * p * (1 - p)) + 1.0
    assert bool(((count - N * p).abs() <= bound).all()), (count - N * p, bound)


def test_torch_sample_orders_ties_and_pads():
    from msr3d_amd.llm.generate import torch_sample
    w = torch.tensor([[0.0, 1.0, 1.0, -math.inf, 0.5], [-math.inf, -math.inf, 2.0, -math.inf, -math.inf]])
    key, val, tok = torch_sample(w, 3, torch.zeros_like(w))
    assert tok.tolist() == [[1, 2, 4], [2, -1, -1]]
    assert val.tolist() == [[1.0, 1.0, 0.5], [2.0, -math.inf, -math.inf]] and torch.equal(key, val)


# -------------------------------------------------------------------------------------------------- group invariance
@pytest.mark.parametrize("beams", [1, 2])
def test_sampled_tokens_do_not_depend_on_the_grouping(case, beams):
    from msr3d_amd.llm.generate import search
    model, embed_fn, _, _ = case
    x, keep = prompt(0, B=7)

    class Capped(HFEngine):
        max_rows = 6

    kw = dict(num_beams=beams, max_length=6, min_length=0, repetition_penalty=3.0, do_sample=True, top_p=0.9, top_k=50,
              temperature=1.5, num_return_sequences=3 if beams == 1 else 2, seed=20261020, draw="counter")
    # (n = 3 samples per prompt without beams; with 2 beams n <= num_beams, so the 2 best)
    whole = search(HFEngine(model), embed_fn, x, keep, **kw)
    cut = search(Capped(model), embed_fn, x, keep, **kw)
    assert whole.shape[0] == 7 * kw["num_return_sequences"] and torch.equal(whole, cut), (whole, cut)
    again = search(HFEngine(model), embed_fn, x, keep, **kw)
    assert torch.equal(whole, again)
    other = search(HFEngine(model), embed_fn, x, keep, **{**kw, "seed": 7})
    assert not torch.equal(whole, other)


def test_seed_none_draws_from_the_cpu_generator(case):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    kw = dict(max_length=5, min_length=0, do_sample=True, top_p=0.9, temperature=1.5, draw="counter")
    torch.manual_seed(5)
    a = search(HFEngine(model), embed_fn, x, keep, **kw)
    torch.manual_seed(5)
    b = search(HFEngine(model), embed_fn, x, keep, **kw)
    assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [
    dict(num_return_sequences=2),                                     # greedy has one result
    dict(num_beams=2, num_return_sequences=3),
    dict(num_beams=2, num_return_sequences=3, do_sample=True),
    dict(do_sample=True, top_p=0.0), dict(do_sample=True, top_p=1.5),
    dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=-1.0),
    dict(do_sample=True, top_k=-1),
    dict(do_sample=True, draw="philox"),
])
def test_refusals(case, kw):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    with pytest.raises(ValueError):
        search(HFEngine(model), embed_fn, x, keep, max_length=2, **kw)


def test_a_nucleus_too_small_for_the_beams_raises(case):
    """Beam sampling needs 2 x beams candidates from the only live beam at the first step: top_k = 3 leaves three."""
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    for draw in ("counter", "multinomial"):
        with pytest.raises(ValueError):
            search(HFEngine(model), embed_fn, x, keep, max_length=4, min_length=0, num_beams=5, do_sample=True, top_k=3,
                   seed=1, draw=draw)


def test_the_engine_vocabulary_cap_is_the_header_constant():
    import os
    import re

    from msr3d_amd.llm.generate import CachedDecoder
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msr3d_hip.h")
    cap = int(re.search(r"#define\s+MSR3D_DECODE_SAMPLE_MAX_V\s+(\d+)", open(header).read()).group(1))
    assert CachedDecoder.max_sample_vocab == cap and cap >= 32768
