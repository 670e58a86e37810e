"""KV-cached decoding (msr3d_amd/llm/generate.py::CachedDecoder on csrc/llm_decode.hip) on the GPU.

C. cached == recomputed: teacher-forced along the greedy fixture, the logits `step` returns against
   LoRALlamaStack.logits (the full forward, arange positions) on the same prefix, for the row without padding, where both
   rotate by the same positions.  Two bf16 pipelines that differ in summation order: rel-L2 2e-2, the bound
   tests/test_llama_stack_gpu.py puts on logits.
D. against transformers: the same walk, ALL rows (the left-padded one and the one with masked slots inside the prompt:
   this pins positions = cumsum(mask) - 1), greedy and the 5-beam fixture (its tokens and beam indices are fed, so the
   cache reorder is on the path): unprocessed logits within rel-L2 2e-2 of the fp32 fixture's at every step.
E. free-running: the gap fixture (every reference step decided by a margin >= 4 x the measured deviation of the full
   forward from fp32) token for token, every step.
Measured on an MI355X (printed by the tests): C worst step rel-L2 0.0097 (row 0), 0.0107 (the left-padded row); D worst
step and row 0.0105 greedy, 0.0109 with 5 beams (largest absolute deviation 0.045 on logits of unit spread; the full
forward's own deviation from the same fixture is 0.045)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, full_forward_logits, gpu_stack

pytestmark = pytest.mark.gpu
BOUND = 2e-2


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _load(name):
    return dict(np.load(os.path.join(GOLD, name), allow_pickle=False))


def _walk(net, emb, g, beams=1):
    """Teacher-forced: -> [logits (N, V) float cpu] per step of the fixture."""
    from msr3d_amd.llm.generate import CachedDecoder
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    steps = g["logits"].shape[0]
    eng = CachedDecoder(net)
    eng.reserve(beams, steps)
    lg = eng.prefill(x, keep)
    eng.expand(beams)
    out = [lg.repeat_interleave(beams, 0).float().cpu()]
    for s in range(steps - 1):
        if beams == 1:
            lg = eng.step(emb[torch.from_numpy(g["sequences"][:, s]).cuda()])
        else:
            lg = eng.step(emb[torch.from_numpy(g["feed_tokens"][s]).cuda()], torch.from_numpy(g["feed_beam_idx"][s]).cuda())
        out.append(lg.float().cpu())
    return out


def test_cached_step_equals_the_full_forward_on_the_same_prefix():
    g = _load("generate_seed0_greedy.npz")
    net, emb = gpu_stack(int(g["seed"]))
    got = _walk(net, emb, g)
    x, keep, seq = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"]), torch.from_numpy(g["sequences"])
    full = full_forward_logits(net, emb, x, keep, seq[:, :-1]).cpu()          # (B, steps, V)
    errs = [rel(got[s][0], full[0, s]) for s in range(len(got))]
    print("C: cached vs full forward, row 0, rel-L2 per step: worst %.5f mean %.5f" % (max(errs), sum(errs) / len(errs)))
    assert max(errs) < BOUND, errs
    # the left-padded row rotates by other positions in the two paths, but rotary attention is relative: the same bound
    errs1 = [rel(got[s][1], full[1, s]) for s in range(len(got))]
    print("C: row 1 (left-padded): worst %.5f" % max(errs1))
    assert max(errs1) < BOUND, errs1


@pytest.mark.parametrize("name,beams", [("generate_seed0_greedy.npz", 1), ("generate_seed0_greedy_rep.npz", 1),
                                        ("generate_seed0_beam5.npz", 5)])
def test_teacher_forced_logits_match_the_transformers_fixture_on_every_row(name, beams):
    g = _load(name)
    net, emb = gpu_stack(int(g["seed"]))
    got = _walk(net, emb, g, beams)
    ref = torch.from_numpy(g["logits"])
    N = ref.shape[1]
    errs = torch.tensor([[rel(got[s][n], ref[s, n]) for n in range(N)] for s in range(len(got))])
    dev = max(float((got[s] - ref[s]).abs().max()) for s in range(len(got)))
    print("D: %s: rel-L2 worst %.5f (per prompt row: %s), max abs deviation %.4f"
          % (name, float(errs.max()), [round(float(v), 5) for v in errs.view(len(got), -1, beams).amax((0, 2))], dev))
    assert float(errs.max()) < BOUND, errs


def test_free_running_tokens_equal_the_reference_where_every_step_is_decided():
    paths = sorted(glob.glob(os.path.join(GOLD, "generate_gap_seed*.npz")))
    assert paths, "the free-running fixture is missing"
    for path in paths:
        g = dict(np.load(path, allow_pickle=False))
        assert float(g["gaps"].min()) >= float(g["m_gap"]) == 4 * float(g["parent_dev"])
        net, emb = gpu_stack(int(g["seed"]))
        x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
        steps = g["sequences"].shape[1]
        out = net.generate(x, keep, emb, eos_id=int(g["eos"]), pad_id=int(g["eos"]), num_beams=1, max_length=steps,
                           min_length=0, repetition_penalty=float(g["repetition_penalty"]))
        assert out.dtype == torch.int64 and out.is_cuda
        assert np.array_equal(out.cpu().numpy(), g["sequences"]), (out.cpu().numpy(), g["sequences"])


def test_greedy_and_beam_search_run_on_the_engine_and_repeat_bit_for_bit():
    """The whole loop on the kernels (select included), twice: the same tokens; beams = 5 with the reference's arguments."""
    g = _load("generate_seed0_greedy.npz")
    net, emb = gpu_stack(int(g["seed"]))
    x, keep = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["keep"]).cuda()
    for kw in (dict(num_beams=1, repetition_penalty=3.0), dict(num_beams=5, repetition_penalty=3.0, length_penalty=1.0),
               dict(num_beams=2, length_penalty=2.0)):
        a = net.generate(x, keep, emb, max_length=12, min_length=1, **kw)
        b = net.generate(x, keep, emb, max_length=12, min_length=1, **kw)
        assert a.shape[0] == 3 and 1 <= a.shape[1] <= 12 and torch.equal(a, b)
        assert int(a.min()) >= 0 and int(a.max()) < emb.shape[0]


def test_fp8_stacks_are_refused():
    from msr3d_amd.llm import LoRALlamaStack
    from msr3d_amd.llm.generate import CachedDecoder
    net = LoRALlamaStack(1, 512, 4, 1024, 1024, device="cuda", base="fp8")
    with pytest.raises(NotImplementedError, match="fp8"):
        CachedDecoder(net)
