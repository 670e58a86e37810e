"""Batches with more live rows than the engine takes at once (msr3d_amd/llm/generate.py): `prompt_groups` as a pure
function, and `search` on an fp32 engine that states a row limit (tests/generate_helpers.py::HFEngine with `max_rows`)
against transformers' own `generate` on the WHOLE batch, token for token -- a prompt's tokens depend on no other prompt,
so walking the batch in groups is the one-call result.  Five prompts of seed 0 (the three of the other CPU search tests
plus two without padding), the arguments of tests/test_generate_search_cpu.py; an eos that ends row 0 early makes the
groups return different lengths, so the padding to the longest is on the path.  Seed 0 has no near-tie that flips
between a batch of 5 and batches of 2 and 1 in fp32 on the CPU: the tokens are equal."""
import warnings

import pytest
import torch

from tests.generate_helpers import HFEngine, embed_table, hf_generate, hf_model, prompt

warnings.filterwarnings("ignore")


def test_prompt_groups():
    from msr3d_amd.llm.generate import prompt_groups
    assert prompt_groups(14, 5, 64) == [(0, 7), (7, 14)]
    assert prompt_groups(13, 1, 64) == [(0, 13)]
    assert [b - a for a, b in prompt_groups(3, 5, 10)] == [2, 1]
    assert prompt_groups(12, 5, 64) == [(0, 12)] and prompt_groups(13, 5, 64) == [(0, 7), (7, 13)]
    assert prompt_groups(64, 1, 64) == [(0, 64)] and prompt_groups(1, 64, 64) == [(0, 1)]
    with pytest.raises(ValueError, match="65"):
        prompt_groups(2, 65, 64)
    for B in range(1, 40):
        for per in (1, 2, 5, 7, 64):
            for cap in (64, 32, 10, 7):
                if per > cap:
                    with pytest.raises(ValueError):
                        prompt_groups(B, per, cap)
                    continue
                gs = prompt_groups(B, per, cap)
                assert gs[0][0] == 0 and gs[-1][1] == B
                assert all(gs[i][1] == gs[i + 1][0] for i in range(len(gs) - 1))         # 0 .. B, no gap, no overlap
                sizes = [b - a for a, b in gs]
                assert all(1 <= s and s * per <= cap for s in sizes)
                assert sizes == sorted(sizes, reverse=True) and sizes[0] - sizes[-1] <= 1
                assert len(gs) == -(-B // (cap // per))                                  # the fewest that fit


class _Limited(HFEngine):
    """HFEngine with a row limit: refuses what a limited engine refuses, and counts its prefills."""

    def __init__(self, model, max_rows=None):
        super().__init__(model)
        if max_rows is not None:
            self.max_rows = max_rows
        self.beams, self.prefills = 1, []

    def reserve(self, rows_per_prompt, new_tokens):
        self.beams = rows_per_prompt

    def prefill(self, inputs_embeds, attention_mask):
        rows = inputs_embeds.shape[0] * self.beams
        assert rows <= getattr(self, "max_rows", rows), "search passed the engine more live rows than it takes"
        self.prefills.append(inputs_embeds.shape[0])
        return super().prefill(inputs_embeds, attention_mask)


@pytest.fixture(scope="module")
def case():
    model = hf_model(0)
    emb = torch.from_numpy(embed_table(0))
    x, keep = prompt(0, B=5)
    early = int(hf_generate(model, x, keep, 24)[0, 5])            # as eos it ends row 0 at step 5
    return model, (lambda ids: emb[ids]), x, keep, early


def _grouped(case, max_rows, n_new, **kw):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep, _ = case
    eng = _Limited(model, max_rows)
    got = search(eng, embed_fn, x, keep, eos_id=kw.get("eos_id", 2), pad_id=kw.get("pad_id", 2),
                 num_beams=kw.get("num_beams", 1), max_length=n_new, min_length=kw.get("min_length", 0),
                 repetition_penalty=kw.get("repetition_penalty", 1.0), length_penalty=kw.get("length_penalty", 1.0))
    ref = hf_generate(model, x, keep, n_new, **kw)
    assert got.dtype == torch.int64 and got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.equal(got, ref), (got, ref)
    return eng, ref


def test_five_prompts_of_five_beams_on_an_engine_of_ten_rows_equal_transformers_on_the_whole_batch(case):
    e = case[4]
    eng, _ = _grouped(case, 10, 10, num_beams=5, repetition_penalty=3.0)
    assert eng.prefills == [2, 2, 1]
    _grouped(case, 10, 24, num_beams=5, length_penalty=2.0, eos_id=e, pad_id=e)
    _grouped(case, 10, 24, num_beams=5, repetition_penalty=3.0, eos_id=e, pad_id=e, min_length=3)


def test_greedy_on_an_engine_of_two_rows_equals_transformers_on_the_whole_batch(case):
    e = case[4]
    eng, _ = _grouped(case, 2, 24)
    assert eng.prefills == [2, 2, 1]
    _, ref = _grouped(case, 2, 24, eos_id=e, pad_id=7)
    assert bool((ref[0, 6:] == 7).all()) and ref.shape[1] > 6      # row 0's group ended early and was padded to the longest
    _grouped(case, 2, 24, repetition_penalty=3.0, eos_id=e, pad_id=e, min_length=8)


def test_an_engine_without_a_row_limit_and_a_batch_within_it_run_as_one_call(case):
    eng, _ = _grouped(case, None, 10, num_beams=5, repetition_penalty=3.0)
    assert eng.prefills == [5]
    eng, _ = _grouped(case, 25, 10, num_beams=5, repetition_penalty=3.0)
    assert eng.prefills == [5]
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep, _ = case
    with pytest.raises(ValueError, match="5 rows per prompt"):
        search(_Limited(model, 4), embed_fn, x, keep, num_beams=5, max_length=4)
