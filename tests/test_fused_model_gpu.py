"""The whole-trainable-part schedule (msr3d_amd/fused_model.py) against the per-layer node
(msr3d_amd/fused_layer.py) and the modular path (separate autograd nodes): same forward, same
gradients for EVERY trainable parameter.  Without dropout: <= 2e-5 rel-L2 against the modular path
(different split-K arrival orders and fusion boundaries, same arithmetic).  With dropout the schedule and
the per-layer node draw their masks from the same (seed, salt, index) hash at the same call-site
order, so with the salt counter reset they must agree just as tightly; the modular path draws at
other call sites and is not comparable there."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _setup(dropout, seed=0, B=3, O=20, E=128, situation_type="as_transform_for_objects", lr=1e-3, weight_decay=0.05):
    import msr3d_amd.model  # noqa: F401
    import msr3d_amd.modules  # noqa: F401
    from msr3d_amd import hipops
    from msr3d_amd.config import AttrDict, default_prompter_cfg
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.model import build_model
    from msr3d_amd.optim import FlatAdamW
    from msr3d_amd.synth import synth_batch
    torch.manual_seed(seed)
    cfg = AttrDict({"prompter": default_prompter_cfg(dropout=dropout, situation_type=situation_type), "llm_hidden_size": E,
                    "model": {"name": "MSR3DHotPath"}})
    model = build_model(cfg).cuda().train()
    # the zero-initialised constants would hide their gradient paths' forward effect
    with torch.no_grad():
        model.visual_prompter.object_orientation_feat.normal_(std=0.5)
        if situation_type == "as_object":
            model.visual_prompter.anchor_size.uniform_(0.5, 1.5)      # (a constant the module never trains)
    params = [p for p in model.parameters() if p.requires_grad]
    dp = FlatGradAllReduce(params, pack_groups=hipops.collect_pack_groups(model))
    opt = FlatAdamW(dp, lr=lr, weight_decay=weight_decay)         # (0.05: FlatAdamW's own default)
    assert hipops.attach_packed_views(model, dp, opt) == 3
    assert model._schedule is not None
    model._test_opt = opt
    batch = synth_batch(31, B, O=O, P=1024, device="cuda")
    with torch.no_grad():
        batch["obj_embeds"] = model.visual_prompter.encode_objects(batch["obj_fts"]).clone()
    return model, dp, batch


def _run(model, dp, batch, mode):
    from msr3d_amd import hipops
    model._schedule.enabled = mode == "schedule"
    for l in model.visual_prompter.spatial_encoder:
        l.use_fused_layer = mode != "modular"
    seed = hipops.seed_word(torch.device("cuda", torch.cuda.current_device()))
    seed.fill_(12345)
    hipops._salt_counter[0] = 500
    dp.zero_grad()
    out = model(dict(batch))
    y = out["scene_embeds"]
    w = torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)
    (y * w).sum().backward()
    dp.finish()
    torch.cuda.synchronize()
    return (y.detach().clone(), out["obj_tokens"].detach().clone(),
            {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.requires_grad})


def _compare(a, b, tol):
    (ya, ta, ga), (yb, tb, gb) = a, b
    assert rel(ya, yb) < tol and rel(ta, tb) < tol
    assert sorted(ga) == sorted(gb)
    for k in gb:
        if k.endswith("w_ks.bias"):              # mathematically zero (softmax shift invariance)
            assert ga[k].abs().max() < 1e-3
            continue
        if gb[k].abs().max() == 0:               # parameters this configuration does not use
            assert ga[k].abs().max() == 0, k
            continue
        assert rel(ga[k], gb[k]) < tol, (k, rel(ga[k], gb[k]))


@pytest.mark.parametrize("B,O", [(3, 20), (2, 60), (5, 13)])
def test_schedule_matches_modular_and_per_layer_paths_without_dropout(B, O):
    model, dp, batch = _setup(0.0, B=B, O=O)
    assert model._schedule.eligible(dict(batch))
    s = _run(model, dp, batch, "schedule")
    m = _run(model, dp, batch, "modular")
    l = _run(model, dp, batch, "layer")
    _compare(s, m, 2e-5)
    _compare(s, l, 2e-5)
    # every parameter the configuration uses received a gradient
    used = [k for k, v in m[2].items() if v.abs().max() > 0]
    assert len(used) >= 60


def test_schedule_draws_the_per_layer_nodes_masks_with_dropout():
    model, dp, batch = _setup(0.1, seed=2)
    s = _run(model, dp, batch, "schedule")
    l = _run(model, dp, batch, "layer")
    _compare(s, l, 5e-5)
    s2 = _run(model, dp, batch, "schedule")       # same seed word, same salts: same masks
    assert rel(s2[0], s[0]) < 1e-5
    from msr3d_amd import hipops
    model._schedule.enabled = True
    hipops._salt_counter[0] = 500                 # but a bumped seed word draws new ones
    hipops.bump_seed(torch.device("cuda", torch.cuda.current_device()))
    y = model(dict(batch))["scene_embeds"].detach()
    assert rel(y, s[0]) > 1e-3


def test_schedule_is_skipped_where_it_does_not_apply():
    model, dp, batch = _setup(0.0)
    model.eval()
    with torch.no_grad():
        assert not model._schedule.eligible(dict(batch))
        y = model(dict(batch))["scene_embeds"]
    model.train()
    s = _run(model, dp, batch, "schedule")
    assert rel(y, s[0]) < 1e-5                    # dropout 0: eval == train forward


def test_train_step_through_the_schedule_in_a_graph():
    """HotPathTrainStep captures the schedule; replayed steps equal eager steps."""
    from msr3d_amd.synth import synth_batch
    from msr3d_amd.train_step import HotPathTrainStep
    results = []
    for use_graph in (False, True):
        model, dp, _ = _setup(0.0, seed=4, B=2, O=12, E=64)
        opt = model._test_opt
        batches = [synth_batch(70 + i, 2, O=12, P=1024, device="cuda") for i in range(3)]

        def loss_fn(out):
            y = out["scene_embeds"]
            return (y * y).mean()
        step = HotPathTrainStep(model, opt, dp, loss_fn, batches[0], use_graph=use_graph)
        step.capture(batches[0])
        losses = [float(step(b)) for b in batches]
        results.append((losses, {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad}))
    (l0, p0), (l1, p1) = results
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    # split-K sums meet by atomicAdd (arrival order differs run to run) and AdamW's normalisation turns
    # a noise-only gradient (w_ks.bias: mathematically zero) into O(lr) steps of random sign: exclude it,
    # compare the rest at 3 lr (as tests/test_train_step_gpu.py does)
    for k in p0:
        if k.endswith("w_ks.bias"):
            continue
        assert torch.allclose(p0[k], p1[k], rtol=1e-3, atol=3e-3), k


@pytest.mark.parametrize("B,O,E", [(3, 20, 128), (2, 60, 256), (5, 13, 128), (16, 60, 4096), (2, 63, 256), (2, 120, 256),
                                   (3, 64, 128)])
def test_as_object_schedule_matches_the_modular_path(B, O, E):
    """situation_type 'as_object' (configs/leo_3_dataset_pure_txt.yaml's prompter: the agent is a token of its own in
    front of the objects, /root/reference/model/ose3d_situation.py:334-353) on the scene-block schedule (round 6:
    msr3d_anchor_front_fwd / _bwd + the blocks) against the per-module path under autograd: outputs, the returned mask
    and EVERY parameter gradient -- anchor_feat, orientation_encoder, loc_layers and both rows of the type table among
    them.  O = 63: L = 64, a full block; O = 64, 120 (BASELINE's stress configuration): more tokens than a block holds --
    the hybrid schedule with the same front and back."""
    model, dp, batch = _setup(0.0, B=B, O=O, E=E, situation_type="as_object")
    sched = model._schedule
    assert sched.anchor and sched.eligible(dict(batch))
    a = _run(model, dp, batch, "schedule")
    # O + 1 <= 64: a scene is a block; beyond: the hybrid schedule (row-local halves on the block kernels over 64-row tiles,
    # attention on the strip kernels)
    assert sched._ran_blocks and sched.hybrid == (O + 1 > 64) and sched.dims["L"] == O + 1 and a[1].shape[1] == O + 1
    mask_s = model(dict(batch))["obj_masks"].clone()
    b = _run(model, dp, batch, "modular")
    sched.enabled = False
    mask_m = model(dict(batch))["obj_masks"].clone()
    assert torch.equal(mask_s, mask_m) and mask_s.shape == (B, O + 1) and bool(mask_s[:, 0].all())
    for k in ("anchor_feat", "orientation_encoder.weight", "loc_layers.0.0.weight", "object_type_embedding.weight"):
        assert float(b[2]["visual_prompter." + k].abs().max()) > 0, k
    # (E = 4096: the modular path meets its K-splits by float atomics over a 4096-wide reduction)
    _compare(a, b, 2e-5 if E <= 512 else 1.5e-4)


def test_as_object_schedule_with_dropout_draws_the_same_masks_from_the_same_seed():
    """Dropout on: two runs from the same seed word and salts draw the same masks -> the same values up to the
    projection's split-K arrival order (float atomics: ~1e-7), and they differ from the dropout-free result."""
    model, dp, batch = _setup(0.1, B=4, O=60, E=256, situation_type="as_object")
    a = _run(model, dp, batch, "schedule")
    b = _run(model, dp, batch, "schedule")
    assert model._schedule._ran_blocks and bool(torch.isfinite(a[0]).all())
    _compare(a, b, 2e-5)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    c = _run(model, dp, batch, "schedule")
    assert rel(a[1], c[1]) > 1e-2


@pytest.mark.parametrize("situation_type", ["as_object", "as_transform_for_objects"])
@pytest.mark.parametrize("B,O,E", [(2, 120, 256), (3, 70, 128), (8, 120, 5120)])
def test_hybrid_and_strip_schedules_match_the_modular_path_beyond_64_tokens(situation_type, B, O, E):
    """A scene of more than 64 tokens (BASELINE's stress configuration: 120 objects, E = 5120): the HYBRID schedule
    (feed-forward / projector halves, every rows launch and the weight gradients on the block kernels over 64-row tiles
    that ignore scene boundaries -- msr3d_scene_block_t.rows_total; the attention on the strip kernels) and round 2's
    strip schedule, each against the per-module path: outputs and every parameter gradient.  (8, 120, 5120): 968 rows =
    15 whole tiles + one of 8 rows, a 20-slab projector."""
    from msr3d_amd import fused_model
    model, dp, batch = _setup(0.0, B=B, O=O, E=E, situation_type=situation_type)
    sched = model._schedule
    ref = _run(model, dp, batch, "modular")
    tol = 2e-5 if E <= 512 else 1.5e-4
    try:
        hy = _run(model, dp, batch, "schedule")
        assert sched._ran_blocks and sched.hybrid and sched.tiles == (B * sched.dims["L"] + 63) // 64
        _compare(hy, ref, tol)
        fused_model.set_mode("strips")
        st = _run(model, dp, batch, "schedule")
        assert not sched._ran_blocks
        _compare(st, ref, tol)
    finally:
        fused_model.set_mode("blocks")


@pytest.mark.parametrize("mode,tol_out,tol_grad", [("bf16", 2e-2, 6e-2), ("fp8_bf16", 5e-2, 1.5e-1)])
def test_labelled_reduced_precision_attention_on_the_hybrid_schedule(mode, tol_out, tol_grad):
    """BASELINE.json configs[4] names "fp8 MFMA object-attention" for the stress shape (120 objects + the agent: L = 121).
    `hipops.set_attention_mma('fp8_bf16')` is its TRAINING form -- QK^T / PV of the forward on OCP e4m3 MFMA, the
    backward's four products on bf16 operands, softmax / spatial term / accumulation fp32 -- and 'bf16' north_star's
    wording; both are LABELLED variants (never the default), honoured by the hybrid schedule's attention half (the strip
    kernels).  Stated tolerances against the fp32-accurate path: outputs 2e-2 (BASELINE.md's figure) / 5e-2, parameter
    gradients 6e-2 / 1.5e-1 rel-L2; and they must differ from it (the variant really ran)."""
    from msr3d_amd import hipops
    model, dp, batch = _setup(0.0, B=2, O=120, E=256, situation_type="as_object")
    sched = model._schedule
    ref = _run(model, dp, batch, "schedule")
    assert sched._ran_blocks and sched.hybrid
    prev = hipops.set_attention_mma(mode)
    try:
        got = _run(model, dp, batch, "schedule")
        assert sched._ran_blocks and sched.hybrid
    finally:
        hipops.set_attention_mma(prev)
    assert 1e-6 < rel(got[0], ref[0]) < tol_out and rel(got[1], ref[1]) < tol_out
    worst = 0.0
    for k, g in ref[2].items():
        if k.endswith("w_ks.bias") or g.abs().max() == 0:
            continue
        worst = max(worst, rel(got[2][k], g))
    assert worst < tol_grad, worst
    # the inference-only form still refuses a schedule that will run backward
    prev = hipops.set_attention_mma("fp8")
    try:
        with pytest.raises(RuntimeError, match="forward-only"):
            _run(model, dp, batch, "schedule")
    finally:
        hipops.set_attention_mma(prev)
