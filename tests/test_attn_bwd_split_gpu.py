"""The attention backward block as two workgroups per (scene, head) (csrc/scene_block.hip, scene_attn_bwd3_kernel<2>,
MSR3D_ATTN_BWD_SPLIT=1) against the one-workgroup form it replaces (<1>, =0): the SAME BITS -- torch.equal on every buffer
of the blocks schedule and on every parameter gradient whose bits the one-workgroup form itself reproduces, and at
every shape on the launch's own outputs.  What that
form computes is pinned against float64 and against the strips schedule by tests/test_scene_blocks_gpu.py and
tests/test_fused_model_gpu.py; the switch is read by msr3d_scene_block at every call, so both forms run in this process.

Six gradients cannot be held to their bits by any form: the column sums of the front's backward
(csrc/prompter_rows.hip, pos_embed_bwd_kernel: dga, dba, dgb, dbb, cs1, cs2) meet by float atomicAdd over B L / 16
workgroups, in arrival order.  Measured at (8, 60), E = 256: two runs of the ONE-workgroup form on the same inputs differ in
exactly these six of the 81 gradients and in no buffer, and so do the two forms.  That launch runs no changed code and reads
d_xacc0 .. 2, which ARE compared bit for bit; its six sums are held to the 5e-5 rel-L2 at which
tests/test_scene_blocks_gpu.py holds every parameter gradient between schedules at this width."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
_ENV = "MSR3D_ATTN_BWD_SPLIT"
# the six destinations of pos_embed_bwd_kernel's atomic column sums (LayerNorms of the location / size embeddings, the
# column sums behind the orientation feature and the type embedding)
_ATOMIC_SUMS = ("visual_prompter.object_orientation_feat", "visual_prompter.object_type_embedding.weight",
                "visual_prompter.loc_embedding_encoder.1.weight", "visual_prompter.loc_embedding_encoder.1.bias",
                "visual_prompter.size_embedding_encoder.1.weight", "visual_prompter.size_embedding_encoder.1.bias")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


class _form:
    """MSR3D_ATTN_BWD_SPLIT = `v` inside the block, what it was behind it."""

    def __init__(self, v):
        self.v = str(v)

    def __enter__(self):
        self.prev = os.environ.get(_ENV)
        os.environ[_ENV] = self.v

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop(_ENV, None)
        else:
            os.environ[_ENV] = self.prev


def _both_forms(B, O, E, masks=None):
    """-> [(buffers, gradients) of form 0, of form 1] of one step on the same inputs and dropout keys"""
    import sys
    sys.path.insert(0, "tools")
    from dbg_blocks import run
    from msr3d_amd import fused_model
    from tests.test_fused_model_gpu import _setup
    model, dp, batch = _setup(0.1, B=B, O=O, E=E)
    if masks is not None:
        batch["obj_masks"] = masks(batch["obj_masks"])
    res = []
    try:
        for v in (0, 1):
            with _form(v):
                res.append(run(model, dp, batch, "blocks"))
            assert model._schedule.use_blocks() and model._schedule._ran_blocks
    finally:
        fused_model.set_mode("blocks")
    return res


def _assert_same_bits(res):
    (b0, g0), (b1, g1) = res
    assert set(b0) == set(b1) and set(g0) == set(g1)
    for i in range(3):
        assert f"d_qkvc{i}" in b0 and f"d_xacc{i}" in b0
    assert all(k in g0 for k in _ATOMIC_SUMS)
    diff = [k for k in b0 if not torch.equal(b0[k], b1[k])]
    diff += [k for k in g0 if k not in _ATOMIC_SUMS and not torch.equal(g0[k], g1[k])]
    assert not diff, diff
    for k in _ATOMIC_SUMS:
        print(k, _rel(g1[k], g0[k]))
        assert _rel(g1[k], g0[k]) < 5e-5, (k, _rel(g1[k], g0[k]))
    # (the step did something: the gradients the block feeds are neither zero nor NaN)
    assert float(b0["d_qkvc0"].abs().max()) > 0 and all(bool(torch.isfinite(v).all()) for v in g0.values())


def _launch_both_forms(found):
    """A stand-in for scene_blocks.launch_block: an attention backward launch runs under form 0, then -- its outputs saved and
    overwritten with a sentinel -- under form 1 on the very same inputs; `found` collects (launch, output, differing words)."""
    from msr3d_amd import scene_blocks
    from msr3d_amd._lib import BLK
    orig = scene_blocks.launch_block

    def launch(stream, **kw):
        if kw["kind"] != BLK["attn_bwd"]:
            return orig(stream, **kw)
        outs = {"part": kw["part"][:kw["H"]], "dqkvc": kw["dqkvc"]}      # every word of both is the launch's to write
        got = []
        for v in (0, 1):
            for t in outs.values():
                t.fill_(7.0)
            with _form(v):
                orig(stream, **kw)
            torch.cuda.synchronize()
            got.append({k: t.clone() for k, t in outs.items()})
        for k in outs:
            assert not bool((got[0][k] == 7.0).all())
            found.append((len(found) // 2, k, int((got[0][k].view(torch.int32) != got[1][k].view(torch.int32)).sum())))
    return orig, launch


# The launch itself, at every shape, on the same inputs under both forms -- its two outputs, the head slabs of `part` and
# d_qkvc, word for word: (8, 60) scene-major placement, both halves full | (3, 60) plain placement | (2, 40) the second half
# holds 8 rows, 16-byte probability rows | (3, 37) odd L, the scalar probability path, 5 rows | (2, 33) one row | (4, 32),
# (4, 13) the second workgroup owns nothing and leaves at once.  (At small batches the object projection's K splits meet by
# float atomics: measured at (2, 40), two runs of the one-workgroup form differ from x0 on, in every buffer, so a whole step
# there says nothing about a form; the launch on the same inputs does.)
@pytest.mark.parametrize("B,O", [(8, 60), (3, 60), (2, 40), (3, 37), (2, 33), (4, 32), (4, 13)])
def test_split_launch_writes_the_one_workgroup_forms_bits(B, O):
    import sys
    sys.path.insert(0, "tools")
    from dbg_blocks import run
    from msr3d_amd import fused_model, scene_blocks
    from tests.test_fused_model_gpu import _setup
    model, dp, batch = _setup(0.1, B=B, O=O, E=256)
    found = []
    orig, scene_blocks.launch_block = _launch_both_forms(found)
    try:
        run(model, dp, batch, "blocks")
    finally:
        scene_blocks.launch_block = orig
        fused_model.set_mode("blocks")
    assert model._schedule._ran_blocks and len(found) == 6, found         # three layers, two outputs each
    assert all(n == 0 for _, _, n in found), found


# the whole step, every buffer and gradient, where the one-workgroup form reproduces its own bits
def test_split_form_gives_the_one_workgroup_forms_bits_through_the_step():
    _assert_same_bits(_both_forms(8, 60, 256))


def _hand_masks(m):
    m = m.clone()
    m[:] = True
    m[1, 32:] = False                       # every valid object in the first half
    m[1, 5] = False
    m[2, :32] = False                       # rows 32 .. 59 valid, the first half padded except row 0
    m[2, 0] = True
    m[5, 1::2] = False                      # alternating
    m[7, 50:] = False                       # (an ordinary padded tail)
    assert bool(m.any(1).all())             # a softmax over no keys is not defined
    return m


def test_split_form_under_hand_set_pad_masks():
    _assert_same_bits(_both_forms(8, 60, 256, _hand_masks))


def test_split_form_in_the_bf16_variant():
    from msr3d_amd import scene_blocks
    prev = scene_blocks.set_train_mma("bf16")
    try:
        res = _both_forms(8, 60, 256)
        assert scene_blocks.train_mma() == "bf16"
    finally:
        scene_blocks.set_train_mma(prev)
    _assert_same_bits(res)


def test_captured_train_step_under_both_forms():
    """HotPathTrainStep, use_graph=True, B = 8, O = 60, two steps; a graph keeps the form it was captured with.  The first
    step's loss and, behind its update, every parameter but the six of _ATOMIC_SUMS: the same bits.  From there on the six
    carry their arrival-order noise into everything, and the second step is held as
    tests/test_fused_model_gpu.py::test_train_step_through_the_schedule_in_a_graph holds a replayed step to an eager one:
    the loss to 1e-4, the parameters to 3 lr."""
    from msr3d_amd import hipops
    from msr3d_amd.synth import synth_batch
    from msr3d_amd.train_step import HotPathTrainStep
    from tests.test_fused_model_gpu import _setup
    res = []
    for v in (0, 1):
        with _form(v):
            model, dp, _ = _setup(0.1, seed=4, B=8, O=60, E=256)
            opt = model._test_opt
            batches = [synth_batch(70 + i, 8, O=60, P=1024, device="cuda") for i in range(2)]
            hipops.seed_word(torch.device("cuda", torch.cuda.current_device())).fill_(12345)
            hipops._salt_counter[0] = 500

            def loss_fn(out):
                y = out["scene_embeds"]
                return (y * y).mean()
            step = HotPathTrainStep(model, opt, dp, loss_fn, batches[0], use_graph=True)
            step.capture(batches[0])
            losses, params = [], []
            for b in batches:
                losses.append(step(b).detach().clone())
                torch.cuda.synchronize()
                params.append({k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad})
            assert step.graph is not None and model._schedule._ran_blocks
            res.append((losses, params, opt.flat_p.detach().clone()))
    (l0, p0, f0), (l1, p1, f1) = res
    assert torch.equal(l0[0], l1[0]), (float(l0[0]), float(l1[0]))
    diff = [k for k in p0[0] if k not in _ATOMIC_SUMS and not torch.equal(p0[0][k], p1[0][k])]
    assert not diff, diff
    assert abs(float(l0[1]) - float(l1[1])) <= 1e-4 * abs(float(l0[1])), (float(l0[1]), float(l1[1]))
    for k in p0[1]:
        assert torch.allclose(p0[1][k], p1[1][k], rtol=1e-3, atol=3e-3), k
    assert torch.allclose(f0, f1, rtol=1e-3, atol=3e-3) and bool(torch.isfinite(f0).all())
