"""step="fused" on the generate fixture (2 layers, hidden 512, 8 heads, vocabulary 1024): every logit of every step and every
byte of the cache equal to step="split" on the same engine settings, so the tokens of every search are equal too.  No
tolerance: bf16 tensors are compared as int16 views."""
import pytest
import torch

from tests.generate_helpers import gpu_stack, prompt

pytestmark = pytest.mark.gpu
L = 12
BEAM = dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0, max_length=L, min_length=1)
GREEDY = dict(num_beams=1, repetition_penalty=3.0, max_length=L, min_length=1)


@pytest.fixture(scope="module")
def seed0():
    return gpu_stack(0)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _cache_tensors(c):
    out = {f"kv{i}": t for i, t in enumerate(c.kv)}
    out.update({f"pos{i}": t for i, t in enumerate(c._pos)})
    if c.codes:
        out.update({f"kve{i}": t for i, t in enumerate(c.kve)})
    if c.shared:
        out.update(prompt_kv=c.prompt_kv, prompt_keep=c.prompt_keep, lens=c._lens)
        if c.codes:
            out["prompt_kve"] = c.prompt_kve
    else:
        out.update({f"len{i}": t for i, t in enumerate(c._len)})
        out.update({f"keep{i}": t for i, t in enumerate(c._keep)})
    out.update(len=c.len, pos=c.pos)
    return out


@pytest.mark.parametrize("cache", ["rows", "shared"])
@pytest.mark.parametrize("kv,kv_kernels", [("bf16", True), ("e4m3", True), ("e4m3", False)])
def test_side_by_side_every_logit_and_every_cache_byte(seed0, cache, kv, kv_kernels):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = seed0
    x, keep = prompt(0)
    beams, steps = 5, 6
    N = x.shape[0] * beams
    engines = [CachedDecoder(net, lora="merged", prompt_cache=cache, kv=kv, kv_kernels=kv_kernels, step=s)
               for s in ("split", "fused")]
    logits = []
    for eng in engines:
        eng.reserve(beams, steps + 2)
        lg = [eng.prefill(x.cuda(), keep.cuda())]
        eng.expand(beams)
        logits.append(lg)
    assert _same(logits[0][0], logits[1][0])
    g = torch.arange(N)
    perms = torch.tensor([[1, 0, 3, 2, 4], [4, 3, 2, 1, 0], [0, 0, 2, 2, 2], [2, 4, 1, 3, 0]])
    for s in range(steps):
        tok = emb[((g * 7 + 13 * s) % 1000 + 3).cuda()].contiguous()
        beam_idx = None if s == 0 else ((g // beams) * beams + perms[s % 4][g % beams]).cuda()
        before = tok.clone()
        a, b = (eng.step(tok, beam_idx) for eng in engines)
        assert _same(a, b), f"step {s}"
        assert _same(tok, before)                     # the caller's embeddings: read only (the residual goes elsewhere)
    ca, cb = (_cache_tensors(eng.cache) for eng in engines)
    assert engines[0].cache.layout == engines[1].cache.layout == (cache if beams > 1 else "rows")
    assert ca.keys() == cb.keys()
    for name in ca:
        assert _same(ca[name], cb[name]), name
    assert int(engines[1].cache.len.min()) == steps + (0 if cache == "shared" else x.shape[1])


def _both(net, emb, x, keep, **kw):
    a = net.generate(x, keep, emb, lora="merged", **kw)
    b = net.generate(x, keep, emb, lora="merged", step="fused", **kw)
    assert a.shape == b.shape and torch.equal(a, b), (a, b)
    return a


@pytest.mark.parametrize("kw", [
    GREEDY, BEAM,
    dict(max_length=L, min_length=0, repetition_penalty=3.0, do_sample=True, top_p=0.9, top_k=50, temperature=1.5, seed=11),
    dict(max_length=L, min_length=0, repetition_penalty=3.0, do_sample=True, top_p=0.9, top_k=50, temperature=1.5, seed=11,
         num_beams=5),
    dict(GREEDY, loop="device"), dict(BEAM, loop="device"),
    dict(BEAM, prompt_cache="shared", kv="e4m3"), dict(BEAM, prompt_cache="shared", loop="device"),
], ids=["greedy", "beams", "sample", "beam_sample", "greedy_device", "beams_device", "beams_shared_e4m3",
        "beams_shared_device"])
def test_generate_gives_the_split_steps_tokens(seed0, kw):
    net, emb = seed0
    x, keep = prompt(0)
    out = _both(net, emb, x.cuda(), keep.cuda(), **kw)
    assert out.shape[0] == x.shape[0] and out.shape[1] >= 1


@pytest.mark.parametrize("prompts", [7, 12, 14])
def test_generate_on_the_wide_tiles_and_over_two_groups(seed0, prompts):
    """35 and 60 live rows (three and four activation tiles), and 70 = two groups of whole prompts."""
    net, emb = seed0
    x3, keep3 = prompt(0)
    idx = [i % 3 for i in range(prompts)]
    out = _both(net, emb, x3[idx].cuda(), keep3[idx].cuda(), eos_id=2, pad_id=2, **BEAM)
    assert out.shape[0] == prompts


def test_refusals(seed0):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = seed0
    x, keep = prompt(0)
    with pytest.raises(ValueError, match="merged"):
        CachedDecoder(net, lora="separate", step="fused")
    with pytest.raises(ValueError, match="lora='merged'"):
        net.generate(x.cuda(), keep.cuda(), emb, max_length=2, step="fused")
    # a bf16 stack under weights="e4m3": the error it always was, with and without the new keyword
    for extra in ({}, dict(step="fused")):
        with pytest.raises(ValueError, match="base='fp8'"):
            CachedDecoder(net, weights="e4m3", **extra)
        with pytest.raises(NotImplementedError, match="lora='merged' is not supported"):
            CachedDecoder(net, weights="e4m3", lora="merged", **extra)
    for bad in ("both", None):
        with pytest.raises(ValueError, match="step is"):
            CachedDecoder(net, lora="merged", step=bad)
        with pytest.raises(ValueError, match="step is"):
            net.generate(x.cuda(), keep.cuda(), emb, max_length=2, lora="merged", step=bad)


def test_full_step_generate_equals_split():
    from tests.test_generate_full_gpu import MAX_OUT, _check_tokens, _model
    model, batch, c = _model()
    model.eval()
    kw = dict(max_length=16, max_out_len=MAX_OUT, min_length=1, repetition_penalty=3.0, length_penalty=1.0, lora="merged")
    for beams in (1, 5):
        split = model.generate(dict(batch), num_beams=beams, **kw)["output_tokens"]
        fused = model.generate(dict(batch), num_beams=beams, step="fused", **kw)["output_tokens"]
        _check_tokens(fused, c["B"])
        assert torch.equal(split, fused), (split, fused)
    with pytest.raises(ValueError, match="step is"):
        model.generate(dict(batch), num_beams=1, max_length=4, max_out_len=8, lora="merged", step="both")
