"""`search` (msr3d_amd/llm/generate.py) against transformers' own `generate`, exactly, on the CPU: an fp32 engine with the
interface `search` is written against (tests/generate_helpers.py::HFEngine: the fixture's transformers model with its own
key / value cache) drives it, and the returned tokens must EQUAL what the installed transformers returns for the same
model, prompt and arguments -- both sides compute in fp32 from the same weights, so there is no tolerance.  The prompt has
a left-padded row and a row with masked slots inside it."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, HFEngine, embed_table, hf_generate, hf_model, prompt

warnings.filterwarnings("ignore")
N_NEW = 24


@pytest.fixture(scope="module")
def case():
    model = hf_model(0)
    emb = torch.from_numpy(embed_table(0))
    x, keep = prompt(0)
    return model, (lambda ids: emb[ids]), x, keep


def _both(case, n_new=N_NEW, **kw):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    ref = hf_generate(model, x, keep, n_new, **kw)
    got = search(HFEngine(model), embed_fn, x, keep, eos_id=kw.get("eos_id", 2), pad_id=kw.get("pad_id", 2),
                 num_beams=kw.get("num_beams", 1), max_length=n_new, min_length=kw.get("min_length", 0),
                 repetition_penalty=kw.get("repetition_penalty", 1.0), length_penalty=kw.get("length_penalty", 1.0))
    assert got.dtype == torch.int64 and got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.equal(got, ref), (got, ref)
    return ref


def _early_eos(case):
    """A token the reference's greedy run emits in row 0 at step 5: as eos it ends that row early."""
    model, _, x, keep = case
    return int(hf_generate(model, x, keep, N_NEW)[0, 5])


def test_greedy_equals_transformers_and_the_fixture(case):
    ref = _both(case)
    g = np.load(os.path.join(GOLD, "generate_seed0_greedy.npz"))
    assert np.array_equal(ref.numpy(), g["sequences"])


def test_greedy_with_repetition_penalty(case):
    ref = _both(case, repetition_penalty=3.0)
    g = np.load(os.path.join(GOLD, "generate_seed0_greedy_rep.npz"))
    assert np.array_equal(ref.numpy(), g["sequences"])


def test_an_early_eos_ends_one_row_and_pads_it(case):
    e = _early_eos(case)
    ref = _both(case, eos_id=e, pad_id=e)
    assert bool((ref[0, 5:] == e).all()) and not bool((ref[1:] == e).all(1).any())
    ref = _both(case, eos_id=e, pad_id=7)
    assert bool((ref[0, 6:] == 7).all())


@pytest.mark.parametrize("min_length", [8, 12])
def test_min_length_holds_the_eos_back(case, min_length):
    e = _early_eos(case)
    ref = _both(case, eos_id=e, pad_id=e, min_length=min_length)
    assert not bool((ref[0, :min_length] == e).any())
    _both(case, eos_id=e, pad_id=e, min_length=min_length, repetition_penalty=3.0)


@pytest.mark.parametrize("length_penalty", [1.0, 2.0])
@pytest.mark.parametrize("beams", [2, 5])
def test_beam_search_equals_transformers(case, beams, length_penalty):
    e = _early_eos(case)
    _both(case, num_beams=beams, length_penalty=length_penalty)
    _both(case, num_beams=beams, length_penalty=length_penalty, eos_id=e, pad_id=e)
    _both(case, num_beams=beams, length_penalty=length_penalty, repetition_penalty=3.0, eos_id=e, pad_id=e, min_length=3)


def test_the_reference_call_beams_5_penalty_3_and_the_fixture(case):
    ref = _both(case, n_new=10, num_beams=5, repetition_penalty=3.0)
    g = np.load(os.path.join(GOLD, "generate_seed0_beam5.npz"))
    assert np.array_equal(ref.numpy(), g["sequences"])


def test_bos_is_appended_as_an_embedding(case):
    """bos_id: search appends the bos embedding and a mask column itself; the fixture's prompt already ends with it."""
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    a = search(HFEngine(model), embed_fn, x[:, :-1], keep[:, :-1], bos_id=1, max_length=6, min_length=0)
    b = search(HFEngine(model), embed_fn, x, keep, max_length=6, min_length=0)
    assert torch.equal(a, b)
