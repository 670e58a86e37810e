"""`generate(kv="e4m3")`: the key / value cache as OCP e4m3 codes with one power-of-two scale per (slot, head), on
tests/generate_helpers.py's gpu_stack (2 layers, hidden 512, 8 heads of 64, V 1024) and prompt (3 prompts of 24 slots:
one full, one left-padded, one with a hole), 12 new tokens.

a. The keyword: default "bf16", refused values, `score`, uint8 planes at <= 0.52 of the bf16 cache's bytes (exponents
   padded to 16 bytes a slot at H = 8, D = 64: 528 / 1024), and a step reads the codes.
b. Prefill logits are kv="bf16"'s bits: only what is stored is rounded.
c. Engine = statement: CachedDecoder(kv="e4m3") against CachedDecoder(kv="e4m3", kv_kernels=False) -- bf16 planes, the
   bf16 kernels, every write rounded through torch_kv_quantize / torch_kv_dequantize in torch -- tokens and every
   step's logits bit for bit, under every other keyword, sampling and prompt groups, each call twice.
d. prompt_cache="shared" gives the bits of "rows"; loop="device" equals the loop statement.
e. Accuracy, teacher-forced along the transformers fixtures as tests/test_generate_gpu.py walks them.  e8 / e_b: worst
   step-and-row rel-L2 of kv="e4m3" / kv="bf16" from the fp32 fixture logits; e_q: the fixture's own fp32 model on the
   CPU with its cache rounded through the statement after every write, against the same logits.  e8 <= M (e_q + e_b):
   the sum would be a triangle bound if GPU and CPU rounded the same codes; they do not (k differs in bf16 bits, so codes
   near a midpoint flip), hence the factor M = the worst measured ratio rounded up to the next 0.25, at most 2.
   Measured on an MI355X (MEASURED below): greedy walk e8 0.03906, e_b 0.01047, e_q 0.03518, ratio 0.8557; 5-beam walk
   e8 0.04179, e_b 0.01087, e_q 0.04529, ratio 0.7441.  So M = 1.0: the sum itself holds.
f. MSR3DFullStep.generate(kv="e4m3") runs on the small model of tests/test_generate_full_gpu.py and repeats."""
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, HFEngine, gpu_stack, hf_model, prompt

pytestmark = pytest.mark.gpu
L = 12
BEAM = dict(num_beams=5, repetition_penalty=3.0)
# e. as measured (printed by the test; profiles/generate_kv_e4m3.txt): walk -> (e8, e_b, e_q, e8 / (e_q + e_b))
MEASURED = {"generate_seed0_greedy.npz": (0.03906, 0.01047, 0.03518, 0.8557),
            "generate_seed0_beam5.npz": (0.04179, 0.01087, 0.04529, 0.7441)}
M = 1.0


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def bf16_seed0():
    return gpu_stack(0)


class _Logged:
    """A CachedDecoder behind its own interface that keeps a copy of every logits tensor prefill and step return.  No
    `token_loop`: `search` drives it token by token."""

    def __init__(self, engine):
        self._e, self.logits = engine, []

    def __getattr__(self, name):
        if name == "token_loop":
            raise AttributeError(name)
        return getattr(self._e, name)

    def prefill(self, *a, **kw):
        lg = self._e.prefill(*a, **kw)
        self.logits.append(lg.clone())
        return lg

    def step(self, *a, **kw):
        lg = self._e.step(*a, **kw)
        self.logits.append(lg.clone())
        return lg


def _search(net, emb, x, keep, engine_kw, **kw):
    from msr3d_amd.llm.generate import CachedDecoder, _embed_fn, search
    eng = _Logged(CachedDecoder(net, **engine_kw))
    out = search(eng, _embed_fn(emb), x.cuda(), keep.cuda(), max_length=L, min_length=1, **kw)
    return out, eng.logits


def _engine_equals_statement(net, emb, x, keep, engine_kw=None, **kw):
    engine_kw = dict(engine_kw or {}, kv="e4m3")
    tok, lg = _search(net, emb, x, keep, engine_kw, **kw)
    tok_s, lg_s = _search(net, emb, x, keep, dict(engine_kw, kv_kernels=False), **kw)
    tok_2, lg_2 = _search(net, emb, x, keep, engine_kw, **kw)
    assert torch.equal(tok, tok_s), (tok, tok_s)
    assert len(lg) == len(lg_s) > 1
    for s, (a, b) in enumerate(zip(lg, lg_s)):
        assert torch.equal(a, b), (s, rel(a, b))
    assert torch.equal(tok, tok_2) and all(torch.equal(a, b) for a, b in zip(lg, lg_2))
    return tok, lg


# ------------------------------------------------------------------------------------------------------------ a. keyword
def test_the_keyword_and_the_cache_it_allocates(bf16_seed0):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = bf16_seed0
    x, keep = prompt(0)
    assert CachedDecoder(net).kv == "bf16"
    for bad in ("fp8", "e5m2", None, 8):
        with pytest.raises(ValueError, match="kv is"):
            CachedDecoder(net, kv=bad)
        with pytest.raises(ValueError, match="kv is"):
            net.generate(x.cuda(), keep.cuda(), emb, max_length=2, kv=bad)
    sizes = {}
    for cache in ("rows", "shared"):
        for kv in ("bf16", "e4m3"):
            eng = CachedDecoder(net, prompt_cache=cache, kv=kv)
            eng.reserve(5, L)
            eng.prefill(x.cuda(), keep.cuda())
            eng.expand(5)
            c = eng.cache
            sizes[cache, kv] = c.nbytes
            planes = list(c.kv) + ([c.prompt_kv] if c.shared else [])
            assert c.shared == (cache == "shared")
            assert all(p.dtype == (torch.uint8 if kv == "e4m3" else torch.bfloat16) for p in planes)
        assert sizes[cache, "e4m3"] <= 0.52 * sizes[cache, "bf16"], sizes
    print("cache.nbytes:", sizes)
    eng = CachedDecoder(net, kv="e4m3")
    eng.reserve(1, L)
    eng.prefill(x.cuda(), keep.cuda())
    with pytest.raises(ValueError, match="kv='e4m3'"):
        eng.score(torch.zeros((3, 2, 4, 512), device="cuda"), torch.ones((3, 2, 4), device="cuda"))


def test_a_step_reads_the_codes(bf16_seed0):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = bf16_seed0
    x, keep = prompt(0)
    tok = torch.tensor([5, 6, 7], device="cuda")

    def two_steps(spoil):
        eng = CachedDecoder(net, kv="e4m3")
        eng.reserve(1, L)
        eng.prefill(x.cuda(), keep.cuda())
        first = eng.step(emb[tok]).clone()
        if spoil:
            eng.cache.kv[0][:, 1, :, 23] ^= 0x80               # every V code of the prompt's last slot changes sign
        return first, eng.step(emb[tok]).clone()

    a1, a2 = two_steps(False)
    b1, b2 = two_steps(True)
    assert torch.equal(a1, b1) and not torch.equal(a2, b2)


# ------------------------------------------------------------------------------------------------------------ b. prefill
@pytest.mark.parametrize("cache", ["rows", "shared"])
def test_prefill_logits_are_the_bf16_caches_bits(bf16_seed0, cache):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = bf16_seed0
    x, keep = prompt(0)
    got = {}
    for kv in ("bf16", "e4m3"):
        eng = CachedDecoder(net, prompt_cache=cache, kv=kv)
        eng.reserve(5, L)
        got[kv] = eng.prefill(x.cuda(), keep.cuda()).clone()
    assert torch.equal(got["bf16"], got["e4m3"])


# ------------------------------------------------------------------------------------------------- c. engine = statement
@pytest.mark.parametrize("engine_kw,kw", [
    (dict(), dict()),
    (dict(), BEAM),
    (dict(prompt_cache="shared"), BEAM),
    (dict(lora="merged"), dict()),
    (dict(lora="merged", prompt_cache="shared"), BEAM),
    (dict(), dict(do_sample=True, top_p=0.9, seed=11)),
    (dict(), dict(do_sample=True, top_p=0.9, seed=11, num_beams=5)),
    (dict(prompt_cache="shared"), dict(do_sample=True, top_p=0.9, seed=11, num_beams=5)),
], ids=["greedy", "beam5_rep3", "shared", "merged", "merged_shared", "sample", "beam_sample", "beam_sample_shared"])
def test_the_kernels_equal_the_statement_in_every_logit(bf16_seed0, engine_kw, kw):
    net, emb = bf16_seed0
    x, keep = prompt(0)
    _engine_equals_statement(net, emb, x, keep, engine_kw, **kw)


def test_the_kernels_equal_the_statement_on_e4m3_weights():
    net, emb = gpu_stack(0, base="fp8")
    x, keep = prompt(0)
    for cache in ("rows", "shared"):
        _engine_equals_statement(net, emb, x, keep, dict(weights="e4m3", prompt_cache=cache), **BEAM)
    _engine_equals_statement(net, emb, x, keep, dict(weights="e4m3"))


def test_the_kernels_equal_the_statement_over_two_prompt_groups(bf16_seed0):
    """14 prompts x 5 beams = 70 live rows > 64: two groups of 7 prompts, each with its own cache."""
    net, emb = bf16_seed0
    x, keep = prompt(0, B=14)
    whole, _ = _engine_equals_statement(net, emb, x, keep, **BEAM)
    first, _ = _search(net, emb, x[:7], keep[:7], dict(kv="e4m3"), **BEAM)
    assert torch.equal(whole[:7, :first.shape[1]], first) and bool((whole[:7, first.shape[1]:] == 2).all())


# ------------------------------------------------------------------------------------------- d. shared layout, device loop
@pytest.mark.parametrize("kw", [BEAM, dict(num_beams=5, length_penalty=2.0, num_return_sequences=3)],
                         ids=["beam5_rep3", "ret3"])
def test_shared_prompt_cache_gives_the_rows_layouts_bits(bf16_seed0, kw):
    net, emb = bf16_seed0
    x, keep = prompt(0)
    tok_r, lg_r = _search(net, emb, x, keep, dict(kv="e4m3"), **kw)
    tok_s, lg_s = _search(net, emb, x, keep, dict(kv="e4m3", prompt_cache="shared"), **kw)
    assert torch.equal(tok_r, tok_s) and len(lg_r) == len(lg_s)
    assert all(torch.equal(a, b) for a, b in zip(lg_r, lg_s))


@pytest.mark.parametrize("cache", ["rows", "shared"])
def test_the_device_loop_equals_its_statement(bf16_seed0, cache):
    from tests.test_generate_loop_gpu import _graph_equals_statement
    net, emb = bf16_seed0
    x, keep = prompt(0)
    graph = _graph_equals_statement(net, emb, x, keep, engine_kw=dict(kv="e4m3", prompt_cache=cache), **BEAM)
    # ... and the replays read what the host loop's steps read: the statement cache under the same loop, the same tokens
    from tests.test_generate_loop_gpu import _run
    stated, _ = _run(net, emb, x, keep, "device", engine_kw=dict(kv="e4m3", kv_kernels=False, prompt_cache=cache), **BEAM)
    assert torch.equal(graph, stated)
    if cache == "rows":
        _graph_equals_statement(net, emb, x, keep, engine_kw=dict(kv="e4m3"))


# ----------------------------------------------------------------------------------------------------------- e. accuracy
def _load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


def _feeds(g, beams, s):
    if beams == 1:
        return torch.from_numpy(g["sequences"][:, s]), None
    return torch.from_numpy(g["feed_tokens"][s]), torch.from_numpy(g["feed_beam_idx"][s])


def _walk_gpu(net, emb, g, beams, kv):
    from msr3d_amd.llm.generate import CachedDecoder
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    steps = g["logits"].shape[0]
    eng = CachedDecoder(net, kv=kv)
    eng.reserve(beams, steps)
    lg = eng.prefill(x, keep)
    eng.expand(beams)
    out = [lg.repeat_interleave(beams, 0).float().cpu()]
    for s in range(steps - 1):
        tok, idx = _feeds(g, beams, s)
        out.append(eng.step(emb[tok.cuda()], None if idx is None else idx.cuda()).float().cpu())
    return out


def _walk_cpu_rounded(g, beams):
    """The fixture's fp32 transformers model with every layer's cache rounded through the statement after every write."""
    from msr3d_amd.llm.kv_cache import torch_kv_dequantize, torch_kv_quantize
    model = hf_model(int(g["seed"]))
    table = model.model.embed_tokens.weight
    eng = HFEngine(model)

    def round_cache():
        for layer in eng.cache.layers:                       # keys, values (rows, heads, slots, head_dim): per (slot, head)
            for name in ("keys", "values"):
                t = getattr(layer, name)
                t.copy_(torch_kv_dequantize(*torch_kv_quantize(t)).float())

    steps = g["logits"].shape[0]
    lg = eng.prefill(torch.from_numpy(g["x"]), torch.from_numpy(g["keep"]))
    round_cache()
    eng.expand(beams)
    out = [lg.repeat_interleave(beams, 0)]
    for s in range(steps - 1):
        tok, idx = _feeds(g, beams, s)
        out.append(eng.step(table[tok], idx))
        round_cache()
    return out


def _worst(got, ref):
    return max(rel(got[s][n], ref[s, n]) for s in range(len(got)) for n in range(ref.shape[1]))


@pytest.mark.parametrize("name,beams", [("generate_seed0_greedy.npz", 1), ("generate_seed0_beam5.npz", 5)])
def test_teacher_forced_logits_stay_within_the_roundings_of_cache_and_engine(bf16_seed0, name, beams):
    g = _load(name)
    assert int(g["seed"]) == 0
    net, emb = bf16_seed0
    ref = torch.from_numpy(g["logits"])
    e8 = _worst(_walk_gpu(net, emb, g, beams, "e4m3"), ref)
    e_b = _worst(_walk_gpu(net, emb, g, beams, "bf16"), ref)
    e_q = _worst(_walk_cpu_rounded(g, beams), ref)
    print("E: %s: e8 %.5f  e_b %.5f  e_q %.5f  e8 / (e_q + e_b) %.4f" % (name, e8, e_b, e_q, e8 / (e_q + e_b)))
    assert e8 <= M * (e_q + e_b), (e8, e_b, e_q)


# ---------------------------------------------------------------------------------------------------------- f. full model
def test_full_step_generate_runs_and_repeats_token_for_token():
    from tests.test_generate_full_gpu import MAX_OUT, _check_tokens, _model
    model, batch, c = _model()
    model.eval()
    kw = dict(max_length=16, max_out_len=MAX_OUT, min_length=1, repetition_penalty=3.0, length_penalty=1.0, kv="e4m3")
    for beams, cache in ((1, "rows"), (5, "rows"), (5, "shared")):
        tok = model.generate(dict(batch), num_beams=beams, prompt_cache=cache, **kw)["output_tokens"]
        _check_tokens(tok, c["B"])
        assert torch.equal(model.generate(dict(batch), num_beams=beams, prompt_cache=cache, **kw)["output_tokens"], tok)
    with pytest.raises(ValueError, match="kv is"):
        model.generate(dict(batch), num_beams=1, max_length=4, max_out_len=8, kv="int8")
