"""lora="merged": KV-cached decoding on the merged planes bf16(W + s B A) (LoRALlamaStack.merged_weights, one
msr3d_lora_merge launch; generate.MergedSkinnyProducts / decoder.MergedModuleProducts: the R = 0 forms of the products).

a. The same bits as the existing path on a pre-merged stack: stack S with lora="merged" against stack S' -- S's merged
   planes loaded as base weights, every lora_B zero -- with lora="separate": prefill, every teacher-forced step of the
   greedy and the 5-beam fixture (the beam reorder on the path), one `score` call, torch.equal.  The separate path on S'
   adds the low-rank stage with B = 0: exact zeros into the same fp32 accumulators (skinny_kernel adds k steps on wave 3
   only when R > 0, the tiled GEMM only adds K stages, and neither picks its tile by R: R = 0 and R = 64 are both
   multiples of its stage).
b. Against transformers: tests/test_generate_gpu.py's walk over the three fixtures, all rows, its BOUND = 2e-2.
   Measured on an MI355X (printed): worst rel-L2 over steps and rows 0.01130 greedy, 0.01130 greedy with the repetition
   penalty, 0.01163 with 5 beams; largest absolute deviation 0.0412 / 0.0412 / 0.0454 (the separate path on the same
   fixtures: 0.0105 / 0.0109 and 0.045).
c. Free-running: the gap fixtures token for token.
d. Staleness: a written lora_B (version bump), a raw .data write + invalidate_shadows(), release_merged().
e. fp8 stacks and unknown values of `lora` are refused; greedy, beam and sampled calls repeat token for token."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, gpu_stack

pytestmark = pytest.mark.gpu
BOUND = 2e-2


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


def _walk(net, emb, g, beams, lora):
    """Teacher-forced along fixture g -> [logits (N, V) bf16 cuda] per step."""
    from msr3d_amd.llm.generate import CachedDecoder
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    steps = g["logits"].shape[0]
    eng = CachedDecoder(net, lora=lora)
    eng.reserve(beams, steps)
    lg = eng.prefill(x, keep)
    eng.expand(beams)
    out = [lg.repeat_interleave(beams, 0)]
    for s in range(steps - 1):
        if beams == 1:
            lg = eng.step(emb[torch.from_numpy(g["sequences"][:, s]).cuda()])
        else:
            lg = eng.step(emb[torch.from_numpy(g["feed_tokens"][s]).cuda()], torch.from_numpy(g["feed_beam_idx"][s]).cuda())
        out.append(lg)
    return out


def _premerged(seed):
    """S and S': S' holds S's merged planes as its base weights and B = 0 in every pair."""
    from msr3d_amd.llm.lora import LoRALinear
    net, emb = gpu_stack(seed)
    pre, _ = gpu_stack(seed)
    planes = net.merged_weights()
    mods = [m for m in net.modules() if isinstance(m, LoRALinear)]
    pmods = [m for m in pre.modules() if isinstance(m, LoRALinear)]
    assert len(mods) == len(pmods) == 14 and len(planes) == 14
    with torch.no_grad():
        for m, p in zip(mods, pmods):
            assert not torch.equal(planes[m], m.weight), "a merge that changes nothing tests nothing"
            p.load_base_weight(planes[m])
            p.lora_B.weight.zero_()
    return net, pre, emb


def test_merged_engine_gives_the_bits_of_the_separate_engine_on_a_premerged_stack():
    from msr3d_amd.llm.generate import CachedDecoder
    g = _load("generate_seed0_greedy.npz")
    net, pre, emb = _premerged(int(g["seed"]))
    for name, beams in (("generate_seed0_greedy.npz", 1), ("generate_seed0_beam5.npz", 5)):
        g = _load(name)
        a, b = _walk(net, emb, g, beams, "merged"), _walk(pre, emb, g, beams, "separate")
        assert len(a) == len(b) == g["logits"].shape[0]
        for s, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u.view(torch.int16), v.view(torch.int16)), (name, "step", s)
    # one `score` call: 2 candidates of 5 tokens after each prompt (padded to the kernel's 16), one slot masked
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    gen = torch.Generator().manual_seed(3)
    tok = torch.randint(3, emb.shape[0], (x.shape[0], 2, 5), generator=gen).cuda()
    tk = torch.ones(tok.shape, dtype=torch.bool, device="cuda")
    tk[1, 0, 4] = False
    res = []
    for stack, lora in ((net, "merged"), (pre, "separate")):
        eng = CachedDecoder(stack, lora=lora)
        eng.reserve(1, 0)
        l0 = eng.prefill(x, keep, positions="arange")
        res.append((l0, eng.score(emb[tok], tk)))
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16))


@pytest.mark.parametrize("name,beams", [("generate_seed0_greedy.npz", 1), ("generate_seed0_greedy_rep.npz", 1),
                                        ("generate_seed0_beam5.npz", 5)])
def test_merged_teacher_forced_logits_match_the_transformers_fixture_on_every_row(name, beams):
    g = _load(name)
    net, emb = gpu_stack(int(g["seed"]))
    got = [t.float().cpu() for t in _walk(net, emb, g, beams, "merged")]
    ref = torch.from_numpy(g["logits"])
    N = ref.shape[1]
    errs = torch.tensor([[rel(got[s][n], ref[s, n]) for n in range(N)] for s in range(len(got))])
    dev = max(float((got[s] - ref[s]).abs().max()) for s in range(len(got)))
    print("D (merged): %s: rel-L2 worst %.5f (per prompt row: %s), max abs deviation %.4f"
          % (name, float(errs.max()), [round(float(v), 5) for v in errs.view(len(got), -1, beams).amax((0, 2))], dev))
    assert float(errs.max()) < BOUND, errs


def test_merged_free_running_tokens_equal_the_reference_where_every_step_is_decided():
    paths = sorted(glob.glob(os.path.join(GOLD, "generate_gap_seed*.npz")))
    assert paths, "the free-running fixture is missing"
    for path in paths:
        g = dict(np.load(path, allow_pickle=False))
        net, emb = gpu_stack(int(g["seed"]))
        x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
        steps = g["sequences"].shape[1]
        out = net.generate(x, keep, emb, eos_id=int(g["eos"]), pad_id=int(g["eos"]), num_beams=1, max_length=steps,
                           min_length=0, repetition_penalty=float(g["repetition_penalty"]), lora="merged")
        assert out.dtype == torch.int64 and out.is_cuda
        assert np.array_equal(out.cpu().numpy(), g["sequences"]), (out.cpu().numpy(), g["sequences"])


def test_merged_planes_follow_the_weights():
    from msr3d_amd.llm.generate import CachedDecoder
    g = _load("generate_seed0_greedy.npz")
    seed = int(g["seed"])
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()

    def prefill(stack):
        return CachedDecoder(stack, lora="merged").prefill(x, keep).clone()

    def fresh(times):                 # a new stack holding the weights after `times` additions of 0.05
        stack, _ = gpu_stack(seed)
        with torch.no_grad():
            for _ in range(times):
                stack.layers[0].self_attn["q_proj"].lora_B.weight.add_(0.05)
        return prefill(stack)

    net, _ = gpu_stack(seed)
    l0 = prefill(net)
    planes = net.merged_weights()
    ptrs = {m: p.data_ptr() for m, p in planes.items()}
    assert net.merged_weights() is planes and torch.equal(prefill(net), l0)          # fresh planes: nothing is rebuilt
    mod = net.layers[0].self_attn["q_proj"]
    with torch.no_grad():
        mod.lora_B.weight.add_(0.05)                                                  # moves the pair key
    l1 = prefill(net)
    assert not torch.equal(l1, l0)
    assert torch.equal(l1, fresh(1))
    assert {m: p.data_ptr() for m, p in net.merged_weights().items()} == ptrs         # rebuilt in place, not reallocated
    mod.lora_B.weight.data.add_(0.05)                                                 # a raw write: no version moves
    mod.invalidate_shadows()
    l2 = prefill(net)
    assert not torch.equal(l2, l1)
    assert torch.equal(l2, fresh(2))
    # a written BASE weight is seen as well
    with torch.no_grad():
        mod.weight.mul_(0.5)
    assert not torch.equal(prefill(net), l2)
    with torch.no_grad():
        mod.weight.mul_(2.0)                                                          # (exact in bf16)
    assert torch.equal(prefill(net), l2)
    net.release_merged()
    assert net._merged is None
    assert torch.equal(prefill(net), l2) and net._merged is not None


def test_merged_refusals_and_repeatable_calls():
    from msr3d_amd.llm import LoRALlamaStack
    from msr3d_amd.llm.generate import CachedDecoder
    g = _load("generate_seed0_greedy.npz")
    net, emb = gpu_stack(int(g["seed"]))
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    fp8 = LoRALlamaStack(1, 512, 4, 1024, 1024, device="cuda", base="fp8")
    with pytest.raises(NotImplementedError, match="fp8"):
        fp8.generate(x, keep, emb, max_length=2, lora="merged")
    with pytest.raises(NotImplementedError, match="fp8"):
        fp8.merged_weights()
    with pytest.raises(ValueError, match="lora"):
        net.generate(x, keep, emb, max_length=2, lora="bogus")
    with pytest.raises(ValueError, match="lora"):
        CachedDecoder(net, lora=None)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="evaluation"):
        from msr3d_amd.llm.decoder import MergedModuleProducts
        h = torch.zeros((1, 64, 512), dtype=torch.bfloat16, device="cuda", requires_grad=True)
        MergedModuleProducts(net.merged_weights()).project(h, (net.layers[0].self_attn["q_proj"],))
    for kw in (dict(num_beams=1, repetition_penalty=3.0), dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0),
               dict(do_sample=True, top_p=0.9, top_k=50, seed=7, num_return_sequences=2)):
        a = net.generate(x, keep, emb, max_length=12, min_length=1, lora="merged", **kw)
        b = net.generate(x, keep, emb, max_length=12, min_length=1, lora="merged", **kw)
        assert a.shape[0] == 3 * kw.get("num_return_sequences", 1) and 1 <= a.shape[1] <= 12 and torch.equal(a, b)
        assert int(a.min()) >= 0 and int(a.max()) < emb.shape[0]
