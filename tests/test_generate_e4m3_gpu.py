"""weights="e4m3": KV-cached decoding and answer ranking of a base="fp8" stack on its own e4m3 weights
(msr3d_amd/llm/generate.py: E4m3SkinnyProducts / E4m3ModuleProducts on msr3d_fp8_skinny_lowrank, csrc/llm_decode_fp8.hip),
on the fixtures of tests/generate_helpers.py (2 layers, hidden 512, 3 prompts: one without padding, one left-padded, one
with masked slots inside the prompt).

a. The keyword: the default still refuses an fp8 stack; "e4m3" refuses a bf16 stack (ValueError), lora="merged"
   (NotImplementedError naming fp8) and unknown values (ValueError naming `weights`).
b. Teacher-forced `step` logits along the greedy and the 5-beam transformers fixtures against the fp32 logits, all rows.
   Bound: 2 x the deviation of the full forward of the SAME fp8 stack (LoRALlamaStack.logits, which multiplies on e4m3
   from 128 rows up: the path that existed before) from the same fixture, worst step-and-row rel-L2 against worst --
   the factor tests/test_predict_answers_gpu.py allows two realisations of the same arithmetic.  The parent's worst is
   taken over prompts 0 and 1 only (on prompt 2 the full forward's arange positions are another computation than the
   fixture's, so its distance there is no rounding error and would only widen the bound); the engine's over all rows.
c. A step reads the e4m3 images: with weight_q of layer 0's down_proj zeroed after the prefill (the bf16 plane
   untouched) the step logits change; with the codes restored the walk gives its first bits again.
d. prompt_cache="shared" against "rows" with 5 beams: every step's logits bit-identical.
e. net.generate(weights="e4m3") greedy and with 5 beams, twice: equal tokens inside the vocabulary.
f. `score` / rank_answers against the fp32 fixture predict_answers_seed*.npz: prefill logits within 2 x the deviation of
   the fp8 stack's full forward on the repeated sequences, every loss within 2 x that parent's loss deviation -- with
   `score` in one chunk (768 rows: the modules' own forward) and in chunks of 96 rows (two 64-row slabs on the skinny
   kernel).  Selected sets and winners are not asserted: the fixture's margins were sized for the bf16 deviation.
g. MSR3DFullStep.generate / .predict_answers with weights="e4m3" on the configuration of full_step_seed0.npz, base="fp8".

Measured on an MI355X (printed by the tests):
b. worst rel-L2 over steps and rows, e4m3 engine | the fp8 stack's full forward on prompts 0 and 1 (bound: 2 x that):
   greedy 0.10507 | 0.10231 (per prompt 0.105 / 0.098 / 0.099 | 0.102 / 0.098 and, not comparable, 0.402 on prompt 2);
   5 beams 0.11926 | 0.11873 (per prompt 0.113 / 0.119 / 0.104 | 0.113 / 0.119, 0.572 on prompt 2); means 0.089 / 0.091 |
   0.090 / 0.091; the engine's largest absolute deviation 0.486 / 0.434 on logits of unit spread.  (The bf16 engine sits at
   0.0105 / 0.0109 on the same fixtures: this distance is the e4m3 rounding of weights and activations, not the kernel.)
f. parent: loss max abs deviation 0.205592, prefill logits worst rel-L2 0.10142; rank_answers under "e4m3", one chunk and
   chunks of 96 rows alike: 0.205592 and 0.10142 (48 of 48 candidates shared; answers [10, 5, 5] = the fixture's)."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, full_forward_logits, gpu_stack
from tests.predict_helpers import answer_set

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


@pytest.fixture(scope="module")
def fp8_seed0():
    """The seed-0 fixture model with base="fp8", built once for the tests that share it (none leaves it changed)."""
    return gpu_stack(0, base="fp8")


def _walk(net, emb, g, beams=1, steps=None, after_prefill=None, **engine_kw):
    """Teacher-forced along fixture g on an e4m3 engine -> [logits (N, V) bf16 cuda] per step."""
    from msr3d_amd.llm.generate import CachedDecoder
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    steps = g["logits"].shape[0] if steps is None else steps
    eng = CachedDecoder(net, weights="e4m3", **engine_kw)
    eng.reserve(beams, steps)
    lg = eng.prefill(x, keep)
    eng.expand(beams)
    if after_prefill is not None:
        after_prefill()
    out = [lg.repeat_interleave(beams, 0)]
    for s in range(steps - 1):
        if beams == 1:
            lg = eng.step(emb[torch.from_numpy(g["sequences"][:, s]).cuda()])
        else:
            lg = eng.step(emb[torch.from_numpy(g["feed_tokens"][s]).cuda()], torch.from_numpy(g["feed_beam_idx"][s]).cuda())
        out.append(lg)
    return out, eng


def _parent_logits(net, emb, g, beams):
    """The path that existed before, along the same fixture: the full forward of the fp8 stack over prompt + the tokens
    fed so far -> [logits (N, V) float cpu] per step."""
    x, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"])
    steps = g["logits"].shape[0]
    if beams == 1:
        full = full_forward_logits(net, emb, x, keep, torch.from_numpy(g["sequences"])[:, :steps - 1]).cpu()
        return [full[:, s] for s in range(steps)]
    xs, ks = x.repeat_interleave(beams, 0), keep.repeat_interleave(beams, 0)
    hist = torch.zeros((xs.shape[0], 0), dtype=torch.int64)           # every live row's own tokens so far
    out = [full_forward_logits(net, emb, xs, ks, hist)[:, -1].cpu()]
    for s in range(steps - 1):
        hist = torch.cat([hist[torch.from_numpy(g["feed_beam_idx"][s])], torch.from_numpy(g["feed_tokens"][s])[:, None]], 1)
        out.append(full_forward_logits(net, emb, xs, ks, hist)[:, -1].cpu())
    return out


# ---------------------------------------------------------------------------------------------------------- the keyword
def test_the_keyword_is_opt_in_and_refuses_what_it_cannot_do(fp8_seed0):
    from msr3d_amd.llm.generate import CachedDecoder
    net, emb = fp8_seed0
    g = _load("generate_seed0_greedy.npz")
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    with pytest.raises(NotImplementedError, match="fp8.*weights='e4m3'"):
        CachedDecoder(net)                                             # the default: as before, and it names the way out
    with pytest.raises(NotImplementedError, match="fp8"):
        net.generate(x, keep, emb, max_length=2)
    with pytest.raises(NotImplementedError, match="fp8"):
        CachedDecoder(net, weights="e4m3", lora="merged")
    with pytest.raises(NotImplementedError, match="fp8"):
        net.generate(x, keep, emb, max_length=2, weights="e4m3", lora="merged")
    for bad in ("fp8", "E4M3", None):
        with pytest.raises(ValueError, match="weights"):
            CachedDecoder(net, weights=bad)
    bf16_net, _ = gpu_stack(0)
    with pytest.raises(ValueError, match="e4m3"):
        CachedDecoder(bf16_net, weights="e4m3")
    with pytest.raises(ValueError, match="e4m3"):
        bf16_net.predict_answers(x, keep, emb, *answer_set(5, A=8, S=4), weights="e4m3")
    eng = CachedDecoder(net, weights="e4m3", prompt_cache="shared")
    assert eng.weights == "e4m3" and eng.max_rows == 64


# ------------------------------------------------------------------------------------------------------ step logits
@pytest.mark.parametrize("name,beams", [("generate_seed0_greedy.npz", 1), ("generate_seed0_beam5.npz", 5)])
def test_teacher_forced_logits_stay_within_twice_the_full_forwards_deviation(fp8_seed0, name, beams):
    g = _load(name)
    assert int(g["seed"]) == 0
    net, emb = fp8_seed0
    got, _ = _walk(net, emb, g, beams)
    parent = _parent_logits(net, emb, g, beams)
    ref = torch.from_numpy(g["logits"])
    N = ref.shape[1]
    e_new = torch.tensor([[rel(got[s][n].float(), ref[s, n]) for n in range(N)] for s in range(len(got))])
    e_par = torch.tensor([[rel(parent[s][n], ref[s, n]) for n in range(N)] for s in range(len(got))])
    # The full forward rotates slot t by t, the fixture (and the engine) by cumsum(mask) - 1: the same attention for the
    # row without padding and the left-padded one (rotary attention is relative), ANOTHER computation for prompt 2, whose
    # masked slots lie inside the prompt (tests/test_generate_gpu.py, test C).  Its distance there is no rounding error, so
    # the parent's deviation is taken over prompts 0 and 1 alone; the engine is held to it on every row.
    per_prompt = lambda e: [round(float(v), 5) for v in e.view(len(got), -1, beams).amax((0, 2))]     # noqa: E731
    same_positions = e_par.view(len(got), -1, beams)[:, :2]
    a_new = max(float((got[s].float().cpu() - ref[s]).abs().max()) for s in range(len(got)))
    print("b: %s: rel-L2 worst over %d steps x %d rows: e4m3 engine %.5f (mean %.5f; per prompt %s) | the fp8 stack's full "
          "forward, prompts 0 and 1: %.5f (mean %.5f; per prompt, 2 included: %s); engine max abs %.4f"
          % (name, *e_new.shape, float(e_new.max()), float(e_new.mean()), per_prompt(e_new), float(same_positions.max()),
             float(same_positions.mean()), per_prompt(e_par), a_new))
    assert bool(torch.isfinite(e_new).all())
    assert float(e_new.max()) <= 2 * float(same_positions.max())


def test_a_step_reads_the_e4m3_images_not_the_bf16_plane(fp8_seed0):
    g = _load("generate_seed0_greedy.npz")
    net, emb = fp8_seed0
    down = net.layers[0].mlp["down_proj"]
    first, _ = _walk(net, emb, g, steps=4)
    codes, plane = down.weight_q.clone(), down.weight.clone()
    try:
        zeroed, _ = _walk(net, emb, g, steps=4, after_prefill=down.weight_q.zero_)
        assert torch.equal(down.weight, plane)                         # the bf16 plane is as it was
    finally:
        down.weight_q.copy_(codes)
    assert torch.equal(zeroed[0], first[0])                            # the prefill ran before the codes went
    for s in range(1, 4):
        assert not torch.equal(zeroed[s], first[s]), s
    again, _ = _walk(net, emb, g, steps=4)
    for a, b in zip(again, first):
        assert torch.equal(a, b)


def test_shared_prompt_cache_gives_the_rows_layouts_bits(fp8_seed0):
    g = _load("generate_seed0_beam5.npz")
    net, emb = fp8_seed0
    shared, eng = _walk(net, emb, g, 5, prompt_cache="shared")
    rows, eng_rows = _walk(net, emb, g, 5, prompt_cache="rows")
    assert eng.cache.layout == "shared" and eng_rows.cache.layout == "rows"
    for s, (a, b) in enumerate(zip(shared, rows)):
        assert torch.equal(a, b), (s, float((a.float() - b.float()).abs().max()))


def test_generate_runs_greedy_and_beams_and_repeats_token_for_token(fp8_seed0):
    g = _load("generate_seed0_greedy.npz")
    net, emb = fp8_seed0
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    for kw in (dict(num_beams=1, repetition_penalty=3.0), dict(num_beams=5, repetition_penalty=3.0),
               dict(num_beams=5, repetition_penalty=3.0, prompt_cache="shared")):
        a = net.generate(x, keep, emb, max_length=12, min_length=1, weights="e4m3", **kw)
        b = net.generate(x, keep, emb, max_length=12, min_length=1, weights="e4m3", **kw)
        assert a.dtype == torch.int64 and a.shape[0] == 3 and 1 <= a.shape[1] <= 12 and torch.equal(a, b)
        assert int(a.min()) >= 0 and int(a.max()) < emb.shape[0]


# -------------------------------------------------------------------------------------------------------------- ranking
def test_score_and_rank_answers_stay_within_twice_the_full_forwards_deviation(fp8_seed0):
    from msr3d_amd import _lib
    from msr3d_amd.llm.generate import CachedDecoder, rank_answers, _embed_fn
    paths = sorted(glob.glob(os.path.join(GOLD, "predict_answers_seed*.npz")))
    assert paths, "the predict_answers fixture is missing"
    g = dict(np.load(paths[0], allow_pickle=False))
    net, emb = fp8_seed0 if int(g["seed"]) == 0 else gpu_stack(int(g["seed"]), base="fp8")
    x, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"].astype(np.int64))
    ids, am = torch.from_numpy(g["answer_ids"]), torch.from_numpy(g["answer_mask"].astype(np.int64))
    C = int(g["num_ans_candidates"])
    ref_top, ref_loss, ref_l0 = torch.from_numpy(g["topk_ids"]), torch.from_numpy(g["loss"]), torch.from_numpy(g["logits0"])
    B = x.shape[0]
    # the parent: the fp8 stack's full forward + loss on the B C repeated sequences of the fixture's candidates
    # (tests/test_predict_answers_gpu.py::test_fixture_ranking builds them the same way)
    suf_ids, suf_am = ids[ref_top.view(-1)], am[ref_top.view(-1)]
    S = suf_ids.shape[1]
    xs = torch.cat([x.repeat_interleave(C, 0)[:, :-1].cuda().to(torch.bfloat16), emb[suf_ids.cuda()]], 1)
    ks = torch.cat([keep.repeat_interleave(C, 0)[:, :-1], suf_am], 1).cuda()
    tg = torch.full(ks.shape, -100, dtype=torch.int64)
    tg[:, -S:] = torch.where(suf_am.bool(), suf_ids, torch.full_like(suf_ids, -100))
    tg[:, -S] = -100
    T = x.shape[1]
    Tp = -(-xs.shape[1] // 64) * 64
    pad = Tp - xs.shape[1]
    xs = torch.cat([xs, torch.zeros((B * C, pad, xs.shape[2]), dtype=xs.dtype, device="cuda")], 1).contiguous()
    ks = torch.cat([ks, torch.zeros((B * C, pad), dtype=ks.dtype, device="cuda")], 1).contiguous()
    tg = torch.cat([tg, torch.full((B * C, pad), -100, dtype=torch.int64)], 1).cuda().contiguous()
    with torch.no_grad():
        parent_loss = net(xs, attention_mask=ks, targets=tg).float().cpu().view(B, C)
        # (position T - 1 holds bos in every copy: the logits after the prompt; one copy per prompt is read)
        parent_l0 = net.logits(xs, ks)[::C, T - 1].float().cpu()
    p_loss = float((parent_loss - ref_loss).abs().max())
    p_l0 = max(rel(parent_l0[b], ref_l0[b]) for b in range(B))
    print("f: parent (the fp8 stack's full forward on the %d repeated sequences) against the fp32 fixture: loss max abs "
          "deviation %.6f, prefill logits worst rel-L2 %.5f" % (B * C, p_loss, p_l0))
    for max_rows in (8192, 96):
        eng = CachedDecoder(net, weights="e4m3")
        eng.score = functools.partial(eng.score, max_rows=max_rows)
        out = rank_answers(eng, _embed_fn(emb), x.cuda(), keep.cuda(), ids.cuda(), am.cuda(), num_ans_candidates=C)
        l0 = eng.prefill(x.cuda(), keep.cuda(), positions="arange").float().cpu()
        e_l0 = max(rel(l0[b], ref_l0[b]) for b in range(B))
        top, loss = out["topk_ids"].cpu(), out["loss"].cpu()
        assert bool(torch.isfinite(loss).all())
        dev, shared = 0.0, 0
        for b in range(B):                                             # the candidates both selections hold
            for j, a in enumerate(ref_top[b].tolist()):
                hit = (top[b] == a).nonzero()
                if len(hit):
                    dev, shared = max(dev, abs(float(loss[b, int(hit[0])]) - float(ref_loss[b, j]))), shared + 1
        print("f: score in chunks of <= %d rows: prefill logits worst rel-L2 %.5f, loss max abs deviation %.6f over %d of "
              "%d candidates; answers %s (fixture %s)" % (max_rows, e_l0, dev, shared, B * C, out["answers_id"].tolist(),
                                                          g["answers_id"].tolist()))
        assert shared >= B * C // 2, "too few common candidates to say anything"
        assert e_l0 <= 2 * p_l0
        assert dev <= 2 * p_loss
        # which kernel multiplied: the wide e4m3 GEMM for the one chunk of 768 rows, the skinny entry for chunks of 96
        suf, sk = ids[:, 1:][top], am[:, 1:][top]
        sink = {}
        _lib.set_timing_sink(sink, census=True)
        try:
            eng.score(emb[suf.cuda()], sk.cuda())
            torch.cuda.synchronize()
        finally:
            _lib.set_timing_sink(None)
        wide, skinny = "msr3d_fp8_gemm_lowrank" in sink, "msr3d_fp8_skinny_lowrank" in sink
        assert (wide, skinny) == ((True, False) if max_rows == 8192 else (False, True)), sorted(sink)
        # and no LoRA projection on its bf16 plane: per chunk the head is the only bf16 product (14 projections would be)
        chunks = -(-C // max(1, max_rows // (B * 16)))
        assert len(sink.get("msr3d_bf16_gemm_lowrank", ())) <= chunks, {k: len(v) for k, v in sink.items()}


# ----------------------------------------------------------------------------------------------------------- end to end
def _model():
    from tests.test_full_step_gpu import build_model, make_batch
    g = dict(np.load(os.path.join(GOLD, "full_step_seed0.npz"), allow_pickle=False))
    model, c = build_model(g, base="fp8")
    return model, make_batch(g, c), c


def test_full_step_generate_and_predict_answers_on_an_fp8_model():
    model, batch, c = _model()
    model.eval()
    kw = dict(max_length=16, max_out_len=24, min_length=1, repetition_penalty=3.0, length_penalty=1.0, weights="e4m3")
    tok = model.generate(dict(batch), num_beams=5, **kw)["output_tokens"]
    assert tok.shape == (c["B"], 24) and tok.dtype == torch.int64 and not bool((tok == 0).any())
    for row in tok.cpu():
        ends = (row == 2).nonzero()
        if len(ends):
            assert bool((row[int(ends[0]):] == 2).all())               # everything after the first 2 is 2
    assert torch.equal(model.generate(dict(batch), num_beams=5, **kw)["output_tokens"], tok)
    ids, am = answer_set(5, A=24, S=6, vocab=c["vocab"])
    d = model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, weights="e4m3")
    a = d["answers_id"]
    print("g: tokens", tok[:, :16].tolist(), "answers", a.tolist(), "loss", d["answers_loss"].tolist())
    assert a.shape == (c["B"],) and a.dtype == torch.int64 and a.is_cuda
    assert d["answers_topk_ids"].shape == (c["B"], 8) and d["answers_topk_ids"].dtype == torch.int64
    assert d["answers_loss"].shape == (c["B"], 8) and d["answers_loss"].dtype == torch.float32
    assert bool(torch.isfinite(d["answers_loss"]).all())
    assert torch.equal(a, d["answers_topk_ids"].gather(1, d["answers_loss"].argmin(1)[:, None])[:, 0])
    d2 = model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, weights="e4m3")
    assert torch.equal(d2["answers_id"], a) and torch.equal(d2["answers_loss"], d["answers_loss"])
    with pytest.raises(NotImplementedError, match="fp8"):              # the default arguments still refuse the model
        model.generate(dict(batch), num_beams=1, max_length=4, max_out_len=8)
