"""`search(loop="device")` on the CPU: the token loop whose bookkeeping is the statement (torch_greedy_advance /
torch_beam_advance, msr3d_amd/llm/search.py) on a state with `cur` and `done` inside it, read by the host every `poll`
tokens.  On tests/generate_helpers.py::HFEngine (fp32, the fixture's transformers model) its tokens must EQUAL the host
loop's and transformers' own `generate` -- no tolerance: all three compute in fp32 from the same weights, and the stable
ties and the f32 divisor table the device loop states move no token of these cases."""
import warnings

import pytest
import torch

from tests.generate_helpers import HFEngine, embed_table, hf_generate, hf_model, prompt

warnings.filterwarnings("ignore")
N_NEW = 24


@pytest.fixture(scope="module")
def case():
    model = hf_model(0)
    emb = torch.from_numpy(embed_table(0))
    x, keep = prompt(0)
    return model, (lambda ids: emb[ids]), x, keep


@pytest.fixture(scope="module")
def early_eos(case):
    """A token the reference's greedy run emits in row 0 at step 5: as eos it ends that row early."""
    model, _, x, keep = case
    return int(hf_generate(model, x, keep, N_NEW)[0, 5])


def _search(case, loop, n_new=N_NEW, poll=8, **kw):
    from msr3d_amd.llm.generate import search
    model, embed_fn, x, keep = case
    kw.setdefault("min_length", 0)
    return search(HFEngine(model), embed_fn, x, keep, max_length=n_new, loop=loop, **({"poll": poll} if loop == "device" else {}),
                  **kw)


def _three(case, n_new=N_NEW, polls=(8,), **kw):
    """device == host == transformers, token for token; the device loop at every `poll` given."""
    model, _, x, keep = case
    ref = hf_generate(model, x, keep, n_new, **{k: v for k, v in kw.items()})
    host = _search(case, "host", n_new, **kw)
    assert torch.equal(host, ref)
    for poll in polls:
        dev = _search(case, "device", n_new, poll=poll, **kw)
        assert dev.dtype == torch.int64 and dev.shape == ref.shape, (poll, dev.shape, ref.shape)
        assert torch.equal(dev, ref), (poll, dev, ref)
    return ref


def test_greedy(case):
    _three(case, polls=(1, 3, 8))


def test_greedy_with_repetition_penalty(case):
    _three(case, repetition_penalty=3.0)


def test_an_early_eos_ends_one_row(case, early_eos):
    e = early_eos
    ref = _three(case, polls=(1, 3, 8), eos_id=e, pad_id=e)
    assert bool((ref[0, 5:] == e).all()) and not bool((ref[1:] == e).all(1).any())
    ref = _three(case, eos_id=e, pad_id=7)
    assert bool((ref[0, 6:] == 7).all())


@pytest.mark.parametrize("min_length", [8, 12])
def test_min_length(case, early_eos, min_length):
    e = early_eos
    ref = _three(case, eos_id=e, pad_id=e, min_length=min_length)
    assert not bool((ref[0, :min_length] == e).any())
    _three(case, eos_id=e, pad_id=e, min_length=min_length, repetition_penalty=3.0)


@pytest.mark.parametrize("length_penalty", [1.0, 2.0])
@pytest.mark.parametrize("beams", [2, 5])
def test_beam_search(case, early_eos, beams, length_penalty):
    e = early_eos
    _three(case, num_beams=beams, length_penalty=length_penalty)
    _three(case, polls=(1, 3, 8), num_beams=beams, length_penalty=length_penalty, eos_id=e, pad_id=e)
    _three(case, num_beams=beams, length_penalty=length_penalty, repetition_penalty=3.0, eos_id=e, pad_id=e, min_length=3)


def test_the_reference_call_beams_5_penalty_3(case):
    _three(case, n_new=10, polls=(1, 3, 8), num_beams=5, repetition_penalty=3.0)


def test_num_return_sequences_3_of_5(case, early_eos):
    from transformers import GenerationConfig
    model, _, x, keep = case
    e = early_eos
    gc = GenerationConfig(do_sample=False, num_beams=5, num_return_sequences=3, max_new_tokens=N_NEW, eos_token_id=e,
                          pad_token_id=e, bos_token_id=1, use_cache=True, return_dict_in_generate=True)
    with torch.no_grad():
        ref = model.generate(inputs_embeds=x, attention_mask=keep, generation_config=gc).sequences
    kw = dict(num_beams=5, num_return_sequences=3, eos_id=e, pad_id=e)
    host = _search(case, "host", **kw)
    assert host.shape[0] == 9 and torch.equal(host, ref)
    for poll in (1, 3, 8):
        assert torch.equal(_search(case, "device", poll=poll, **kw), ref)


def _equal_states(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_a_state_advanced_after_done_is_unchanged():
    """Walk both statements on made-up candidates until `done`, then advance again: every field stays, `done` too."""
    from msr3d_amd.llm.search import (beam_state, greedy_state, length_divisors, torch_beam_advance,
                                      torch_greedy_advance)
    g = torch.Generator().manual_seed(3)
    B, nb, L, eos = 2, 3, 6, 1
    st, d = beam_state(B, nb, L, 0), length_divisors(L, 2.0)
    for step in range(L):
        val = torch.randn((B * nb, 2 * nb), generator=g).sort(1, descending=True)[0] + st["run_scores"].view(-1, 1)
        tok = torch.randint(0, 4, (B * nb, 2 * nb), generator=g, dtype=torch.int32)
        st, _, _ = torch_beam_advance(st, val, tok, eos, d)
        assert int(st["cur"]) == step + 1
        if int(st["done"]):
            break
    assert int(st["done"]) == 1
    again, _, _ = torch_beam_advance(st, val + 1.0, tok, eos, d)
    _equal_states(again, st)

    st = greedy_state(4, 5, 9)
    for step in range(5):
        tok = torch.tensor([[3], [1 if step == 1 else 4], [1 if step == 2 else 5], [1 if step == 2 else 6]], dtype=torch.int32)
        st, nxt = torch_greedy_advance(st, tok, 1, 9)
        if int(st["done"]):
            break
    assert int(st["done"]) == 1 and int(st["cur"]) == 5            # row 0 never ends: the last column stops the walk
    assert st["seq"].tolist()[1] == [4, 1, 9, 9, 9] and st["seq"].tolist()[2] == [5, 5, 1, 9, 9]
    again, _ = torch_greedy_advance(st, tok + 1, 1, 9)
    _equal_states(again, st)


def test_sampling_is_refused_with_the_reason(case):
    with pytest.raises(NotImplementedError, match="launch argument"):
        _search(case, "device", do_sample=True, top_p=0.9)
    with pytest.raises(ValueError):
        _search(case, "other")
