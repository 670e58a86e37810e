"""The HIP-graph-captured HotPathTrainStep the way the benchmark drives it: one capture, then resident batches of
DIFFERENT padding rotating through the replays, the next batch's frozen encoder prefetched on the side stream.

A replay reads everything through fixed addresses (static obj_embeds, the buffers the schedule's prologue stages per
batch -- key mask, pairwise / Fourier rows, loc6, the returned mask --, the one prefetch buffer, the weight-gradient
plans).  A row or mask byte written only for valid objects would keep the previous batch's value when a scene
shrinks; the step would still run and its loss would still be finite.  So every replay is compared, tensor by tensor,
with an independent path: a twin model from the same seed (lr = 0: the two never diverge) that encodes the batch on
its own and runs the per-module path under autograd -- no schedule, no static buffer, no graph.

Rotation (B = 2; n_valid per scene; twice round, 8 steps):
    R0  [O, O]             the capture batch: no padding at all
    R1  [17, 48] / [33, 97]
    R2  [1, O]             scene 1's objects 3 and 40 masked out and their obj_locs rows zeroed
    R3  [33, 16] / [65, 64]
Per scene the count shrinks and grows between consecutive steps and crosses the 16 / 32 / 48 key-tile edges.

What is compared how:
  * against the modular path, every step: obj_embeds, obj_tokens, scene_embeds and every parameter gradient at
    2e-5 rel-L2 (the bound the schedule meets against that path on one batch, tests/test_fused_model_gpu.py), the
    returned mask exactly.
  * second visit of a batch against the first (a value left over from the batch in between breaks that), and the
    pipelined form against the sequential one ("results are identical to the sequential order", train_step.py).
    hipops.set_deterministic(True) promises run-to-run identical bits, but PrompterSchedule.eligible() declines the
    whole schedule in that mode (msr3d_amd/fused_model.py): under it the captured step is the per-layer path with
    inputs staged by copies, not what the benchmark runs.  So both are tested:
      - deterministic mode (test_rotation_in_deterministic_mode_repeats_bit_for_bit): torch.equal on EVERY cloned
        tensor;
      - default mode, the schedule itself, as far as its launches reduce in a fixed order.  obj_embeds and the mask:
        torch.equal everywhere (the encoder, the side lane's GEMM, the prologue).  as_transform_for_objects on the
        scene blocks: the loss, obj_tokens, scene_embeds and every gradient torch.equal (block partials are stored
        per workgroup and summed in order), except the six column sums msr3d_pos_embed_bwd meets by float atomics
        (POS_SUMS).  as_object: the front of that schedule meets partial sums by float atomics, in an order that
        differs from launch to launch (msr3d_gemm_multi_f32's K-splits of the object projection and the agent's
        orientation term accumulate into the zero-filled arena; msr3d_anchor_front_bwd adds its column sums the same
        way), so obj_tokens already differ in their last bits (measured 1e-7) and everything behind them with them:
        obj_tokens, scene_embeds and the loss are held to 1e-6 rel-L2 (a GEMM output under two K-split arrival
        orders, tests/test_gemm_gpu.py).  Gradients that pass through such atomics are
        column sums over B x L rows of mixed sign: their rel-L2 between two arrival orders is rounding times the
        cancellation of the sum (measured up to 2.2e-6 on POS_SUMS, up to 5.9e-6 on the as_object biases), which no
        figure for a GEMM output bounds -- they are held to 2e-5, what two runs of one schedule are held to in
        tests/test_fused_model_gpu.py, i.e. for them the modular comparison above is the check that bites.
    A stale row or mask byte is a different INPUT, not a different summation order: orders of magnitude above any
    of these (the self-test at the end of the rotation tests).
"""
import functools

import pytest
import torch

from tests.test_fused_model_gpu import _compare, _run, _setup, rel

pytestmark = pytest.mark.gpu

SEED = 5
B, P, E = 2, 1024, 256
N_VALID = {60: ([60, 60], [17, 48], [1, 60], [33, 16]),
           120: ([120, 120], [33, 97], [1, 120], [65, 64])}
HOLES = (3, 40)
VISITS = [0, 1, 2, 3, 0, 1, 2, 3]
ATOMIC = 1e-6          # a GEMM output whose K-splits met in two different orders (tests/test_gemm_gpu.py)
ATOMIC_SUMS = 2e-5     # a gradient whose column partials met in two different orders (tests/test_fused_model_gpu.py)
# msr3d_pos_embed_bwd's six column sums: one float atomic per column and workgroup (csrc/prompter_rows.hip)
POS_SUMS = ("loc_embedding_encoder.1.weight", "loc_embedding_encoder.1.bias", "size_embedding_encoder.1.weight",
            "size_embedding_encoder.1.bias", "object_orientation_feat", "object_type_embedding.weight")


@functools.lru_cache(maxsize=None)
def _rotation(O, pad_holes=False):
    """The four resident batches (kept alive for the module: the prefetch is keyed by tensor identity; never
    written after this).  pad_holes: the two masked-out slots of R2 hold the dataset's padding cloud, as every
    masked slot must for an encoder with skip_padded (pcd_pointnet_encoder.py) -- otherwise they keep their real
    clouds, features the key mask alone has to hide."""
    from msr3d_amd.synth import synth_batch
    out = []
    for i, nv in enumerate(N_VALID[O]):
        b = synth_batch(400 + i, B, O=O, P=P, n_valid=list(nv), device="cuda")
        if i == 2:
            for o in HOLES:
                b["obj_masks"][1, o] = False
                b["obj_locs"][1, o] = 0
                if pad_holes:
                    b["obj_fts"][1, o] = 1.0
            nv = [nv[0], nv[1] - len(HOLES)]
        assert b["obj_masks"].sum(1).tolist() == list(nv)
        out.append(b)
    return tuple(out)


def _loss_weights(y):
    return torch.linspace(-1, 1, y.numel(), device=y.device).view_as(y)


class _seed_state:
    """_run() and the dropout steps move the device's dropout seed word and the salt counter: put both back."""

    def __enter__(self):
        from msr3d_amd import hipops
        self.word = hipops.seed_word(torch.device("cuda", torch.cuda.current_device()))
        self.saved = (self.word.clone(), hipops._salt_counter[0])
        return self.word

    def __exit__(self, *a):
        from msr3d_amd import hipops
        self.word.copy_(self.saved[0])
        hipops._salt_counter[0] = self.saved[1]


@functools.lru_cache(maxsize=None)
def _reference(situation_type, O, pad_holes=False):
    """Per batch, once: the twin's own full encoding and the per-module path under autograd on it."""
    from msr3d_amd import hipops
    was = hipops.set_deterministic(False)
    try:
        with _seed_state():
            twin, dp, _ = _setup(0.0, seed=SEED, B=B, O=O, E=E, situation_type=situation_type, lr=0.0, weight_decay=0.0)
            refs = []
            for b in _rotation(O, pad_holes):
                with torch.no_grad():
                    emb = twin.visual_prompter.encode_objects(b["obj_fts"]).clone()
                rb = dict(b, obj_embeds=emb)
                y, tok, grads = _run(twin, dp, rb, "modular")
                with torch.no_grad():
                    masks = twin(dict(rb))["obj_masks"].clone()        # (_run left the twin on the modular path)
                w = _loss_weights(y)
                refs.append({"embeds": emb, "tok": tok, "scene": y, "grads": grads, "masks": masks,
                             "loss": (y.double() * w.double()).sum(), "loss_scale": float(y.double().norm() * w.double().norm())})
    finally:
        hipops.set_deterministic(was)
    # the test can fail: the four batches give results far apart
    for i in range(4):
        for j in range(i):
            assert rel(refs[i]["tok"], refs[j]["tok"]) > 1e-2 and rel(refs[i]["scene"], refs[j]["scene"]) > 1e-2
    return tuple(refs)


def _drive(situation_type, O, form, skip_padded=False, deterministic=False, steps=8, after_capture=None):
    """Capture on R0, then `steps` replays round the rotation; -> what every step left, cloned."""
    from msr3d_amd import hipops
    from msr3d_amd.train_step import HotPathTrainStep
    was = hipops.set_deterministic(deterministic)
    try:
        with _seed_state():
            model, dp, _ = _setup(0.0, seed=SEED, B=B, O=O, E=E, situation_type=situation_type, lr=0.0, weight_decay=0.0)
            if skip_padded:
                model.visual_prompter.obj_encoder.skip_padded = True
            R = _rotation(O, skip_padded)
            seen = {}

            def loss_fn(out):
                y = out["scene_embeds"]
                if "w" not in seen:
                    seen["w"] = _loss_weights(y)
                seen["tok"], seen["scene"], seen["masks"] = out["obj_tokens"], y, out["obj_masks"]
                return (y * seen["w"]).sum()

            step = HotPathTrainStep(model, model._test_opt, dp, loss_fn, R[0], use_graph=True)
            step.capture(R[0])
            if after_capture is not None:
                after_capture(model, step, R)
            recs = []
            for i in range(steps):
                b = R[VISITS[i]]
                nb = R[VISITS[(i + 1) % len(VISITS)]] if form == "pipelined" else None
                loss = step(b, nb)
                torch.cuda.synchronize()
                # (the next replay rewrites every one of these buffers)
                rec = {"loss": loss.clone(), "tok": seen["tok"].detach().clone(), "scene": seen["scene"].detach().clone(),
                       "masks": seen["masks"].clone(), "embeds": step.static["obj_embeds"].clone(),
                       "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}}
                recs.append(rec)
            torch.cuda.synchronize()
            sched = model._schedule
            assert step.graph is not None
            if deterministic:
                assert not step._sched_direct          # (the schedule declines the ordered mode: the per-layer path ran)
            else:
                assert step._sched_direct and sched._ran_blocks
                assert sched.hybrid == (sched.dims["L"] > 64) and sched.dims["L"] == O + (situation_type == "as_object")
            return recs
    finally:
        hipops.set_deterministic(was)


@functools.lru_cache(maxsize=None)
def _stepped(situation_type, O, form, skip_padded=False, deterministic=False):
    return tuple(_drive(situation_type, O, form, skip_padded, deterministic))


def _against_modular(rec, ref, worst=None):
    """obj_embeds, obj_tokens, scene_embeds, gradients, mask -- in that order: the first wrong buffer is named."""
    figures = {"obj_embeds": rel(rec["embeds"], ref["embeds"]), "obj_tokens": rel(rec["tok"], ref["tok"]),
               "scene_embeds": rel(rec["scene"], ref["scene"])}
    for k, g in ref["grads"].items():
        if not k.endswith("w_ks.bias") and g.abs().max() > 0:
            figures["grad"] = max(figures.get("grad", 0.0), rel(rec["grads"][k], g))
    if worst is not None:
        for k, v in figures.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert figures["obj_embeds"] <= 2e-5, figures
    assert figures["obj_tokens"] < 2e-5, figures
    assert figures["scene_embeds"] < 2e-5, figures
    _compare((rec["scene"], rec["tok"], rec["grads"]), (ref["scene"], ref["tok"], ref["grads"]), 2e-5)
    # |<dy, w>| <= |dy| |w|
    assert abs(float(rec["loss"]) - float(ref["loss"])) <= 2e-5 * ref["loss_scale"]
    assert torch.equal(rec["masks"], ref["masks"])


def _same_step(a, b, loss_scale, how, worst=None):
    """Two runs of one step on one batch (second visit against first, pipelined against sequential).
    how = "exact": every tensor bit for bit.  "blocks" / "anchor": the module docstring's split."""
    assert torch.equal(a["embeds"], b["embeds"]), int((a["embeds"] != b["embeds"]).sum())
    assert torch.equal(a["masks"], b["masks"])
    assert sorted(a["grads"]) == sorted(b["grads"])
    if how != "anchor":
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["tok"], b["tok"]) and torch.equal(a["scene"], b["scene"])
    fig = {"obj_tokens": rel(a["tok"], b["tok"]), "scene_embeds": rel(a["scene"], b["scene"]), "grad": 0.0}
    for k, g in b["grads"].items():
        if how == "exact" or (how == "blocks" and not k.endswith(POS_SUMS)):
            assert torch.equal(a["grads"][k], g), (k, rel(a["grads"][k], g))
        elif k.endswith("w_ks.bias"):                # mathematically zero: rounding noise on both sides
            assert a["grads"][k].abs().max() < 1e-3
        elif g.abs().max() == 0:                     # a parameter the configuration does not use
            assert a["grads"][k].abs().max() == 0, k
        else:
            fig["grad"] = max(fig["grad"], rel(a["grads"][k], g))
            assert rel(a["grads"][k], g) < ATOMIC_SUMS, (k, rel(a["grads"][k], g))
    if worst is not None:
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    if how == "anchor":
        assert fig["obj_tokens"] <= ATOMIC and fig["scene_embeds"] <= ATOMIC, fig
        assert abs(float(a["loss"]) - float(b["loss"])) <= ATOMIC * loss_scale       # |<dy, w>| <= |dy| |w|


def _how(situation_type):
    return "anchor" if situation_type == "as_object" else "blocks"


CASES = [("as_transform_for_objects", 60), ("as_object", 60), ("as_object", 120)]


@pytest.mark.parametrize("form", ["sequential", "pipelined"])
@pytest.mark.parametrize("situation_type,O", CASES)
def test_every_replay_of_the_rotation_matches_the_modular_path(situation_type, O, form):
    refs = _reference(situation_type, O)
    recs = _stepped(situation_type, O, form)
    worst, again = {}, {}
    for i, rec in enumerate(recs):
        _against_modular(rec, refs[VISITS[i]], worst)
    print(f"rotation {situation_type} O {O} {form}: worst rel-L2 against the modular path "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for i in range(4):                                # no stale state: the second visit repeats the first
        _same_step(recs[i + 4], recs[i], refs[i]["loss_scale"], _how(situation_type), worst=again)
    print(f"rotation {situation_type} O {O} {form}: second visit against the first "
          + " ".join(f"{k} {v:.2e}" for k, v in again.items()))


@pytest.mark.parametrize("situation_type,O", CASES)
def test_pipelined_rotation_equals_the_sequential_one(situation_type, O):
    """train_step.py: "Results are identical to the sequential order"."""
    refs = _reference(situation_type, O)
    seq, pip = _stepped(situation_type, O, "sequential"), _stepped(situation_type, O, "pipelined")
    worst = {}
    for i in range(len(VISITS)):
        _same_step(pip[i], seq[i], refs[VISITS[i]]["loss_scale"], _how(situation_type), worst=worst)
    print(f"rotation {situation_type} O {O}: pipelined against sequential " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("situation_type,O", CASES)
def test_rotation_in_deterministic_mode_repeats_bit_for_bit(situation_type, O):
    """hipops.set_deterministic(True): "same seed + same data => identical weights, run after run".  The rotation
    through the captured step in that mode (per-layer path, inputs staged by copies into the static buffers, the same
    prefetch buffer): the second visit of every batch and the pipelined form give the first visit's / the sequential
    form's bits on EVERY cloned tensor, and every step still meets the modular path."""
    st = situation_type
    refs = _reference(st, O)
    seq = _stepped(st, O, "sequential", deterministic=True)
    pip = _stepped(st, O, "pipelined", deterministic=True)
    for i in range(len(VISITS)):
        _against_modular(seq[i], refs[VISITS[i]])
        _same_step(pip[i], seq[i], None, "exact")
    for i in range(4):
        _same_step(seq[i + 4], seq[i], None, "exact")


def test_rotation_with_padding_slots_skipped_by_the_encoder():
    """skip_padded on the stepped model only: a masked slot receives the cached padding feature instead of being
    encoded, into whichever buffer the pass writes (the prefetch buffer here) -- a slot that kept another batch's
    feature would differ from the twin's full encoding, which it must equal bit for bit
    (test_padding_slots_skipped_gives_identical_features)."""
    st, O = "as_transform_for_objects", 60
    refs = _reference(st, O, True)
    recs = _stepped(st, O, "pipelined", True)
    worst = {}
    for i, rec in enumerate(recs):
        assert torch.equal(rec["embeds"], refs[VISITS[i]]["embeds"]), (i, int((rec["embeds"] != refs[VISITS[i]]["embeds"]).sum()))
        _against_modular(rec, refs[VISITS[i]], worst)
    print(f"rotation {st} O {O} pipelined skip_padded: worst rel-L2 against the modular path "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for i in range(4):
        _same_step(recs[i + 4], recs[i], refs[i]["loss_scale"], "blocks")


def test_the_checker_notices_a_stale_mask_and_stale_locations():
    """From the second step on the schedule's prologue is handed R0's obj_masks and obj_locs (values only: mask bytes
    and six floats per object) with the current embeddings -- what a replay reading the capture batch's staged
    buffers would compute.  Step 1 (R0 itself) passes, step 2 must not."""
    st, O = "as_transform_for_objects", 60
    refs = _reference(st, O)
    calls = []

    def mutate(model, step, R):
        sched = model._schedule
        real = sched.stage

        def stale(d, anchor_out=None):
            calls.append(1)
            if len(calls) >= 2:
                d = dict(d, obj_masks=R[0]["obj_masks"], obj_locs=R[0]["obj_locs"])
            return real(d, anchor_out=anchor_out)
        sched.stage = stale

    recs = _drive(st, O, "sequential", steps=2, after_capture=mutate)
    assert len(calls) == 2
    _against_modular(recs[0], refs[0])
    with pytest.raises(AssertionError):
        _against_modular(recs[1], refs[1])


# ---- the update switched on -------------------------------------------------------------------------------------

def _train(form, use_graph, deterministic=False, steps=8):
    from msr3d_amd import hipops
    from msr3d_amd.train_step import HotPathTrainStep
    was = hipops.set_deterministic(deterministic)
    try:
        with _seed_state():
            model, dp, _ = _setup(0.0, seed=SEED, B=B, O=60, E=E, lr=1e-3, weight_decay=0.05)
            opt = model._test_opt
            assert opt.max_grad_norm == 5.0
            R = _rotation(60)
            w = {}

            def loss_fn(out):
                y = out["scene_embeds"]
                if "w" not in w:
                    w["w"] = _loss_weights(y)
                return (y * w["w"]).sum()

            start = opt.flat_p.detach().clone()
            step = HotPathTrainStep(model, opt, dp, loss_fn, R[0], use_graph=use_graph)
            step.capture(R[0])
            assert torch.equal(opt.flat_p, start)      # the warm-up was rolled back
            losses = []
            for i in range(steps):
                nb = R[VISITS[(i + 1) % len(VISITS)]] if form == "pipelined" else None
                losses.append(step(R[VISITS[i]], nb).clone())
            torch.cuda.synchronize()
            assert (step.graph is not None) == use_graph and bool(step._sched_direct) == (not deterministic)
            assert float((opt.flat_p - start).abs().max()) > 1e-3         # the steps did something
            return ([float(l) for l in losses], opt.flat_p.detach().clone(),
                    {k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad})
    finally:
        hipops.set_deterministic(was)


def _params_close(pa, pb):
    for k in pb:
        if k.endswith("w_ks.bias"):                  # a noise-only gradient: AdamW makes O(lr) steps of random sign of it
            continue
        assert torch.allclose(pa[k], pb[k], rtol=1e-3, atol=3e-4), (k, float((pa[k] - pb[k]).abs().max()))


def test_training_round_the_rotation_graph_and_pipelined_equals_eager():
    """AdamW on (lr 1e-3, weight decay 0.05, clip 5): 8 captured, pipelined steps round the rotation end where 8
    eager, sequential steps from the same seed end -- the bounds of test_graph_replay_equals_eager.  Captured
    sequential steps likewise: in the default mode the gradients' last bits follow the arrival order of the schedule's
    float atomics and AdamW's first updates are lr * sign(g) where g is rounding noise, so flat_p cannot repeat bit
    for bit there; the deterministic mode's test below holds that."""
    le, _, pe = _train("sequential", False)
    lp, fp, pp = _train("pipelined", True)
    ls, fs, ps = _train("sequential", True)
    print(f"training rotation: graph pipelined against graph sequential flat_p rel-L2 {rel(fp, fs):.2e}, "
          f"max abs {float((fp - fs).abs().max()):.2e}")
    assert lp == pytest.approx(le, rel=1e-4, abs=1e-6)
    _params_close(pp, pe)
    assert lp == pytest.approx(ls, rel=1e-4, abs=1e-6)
    _params_close(pp, ps)
    assert all(bool(torch.isfinite(v).all()) for v in pp.values())


def test_training_round_the_rotation_pipelined_equals_sequential_bit_for_bit():
    """Deterministic mode: graph + pipelined == graph + sequential on the optimiser's whole parameter buffer."""
    lp, fp, _ = _train("pipelined", True, deterministic=True)
    ls, fs, _ = _train("sequential", True, deterministic=True)
    assert torch.equal(fp, fs), int((fp != fs).sum())
    assert lp == ls


# ---- dropout on ---------------------------------------------------------------------------------------------------

def test_dropout_seed_word_through_capture_and_replays():
    """Dropout 0.1: capture()'s warm-up steps advance the device seed word and are rolled back; every replay advances
    it exactly as an eagerly issued step does (the schedule's first launch bumps it); a scene with one valid key
    stays finite; two consecutive replays of one batch draw different masks."""
    from msr3d_amd import hipops
    from msr3d_amd.train_step import HotPathTrainStep
    R = _rotation(60)
    order = [R[1], R[1], R[2], R[3]]
    start = 0x5EED0123
    words, toks = {}, []
    with _seed_state() as word:
        for use_graph in (True, False):
            model, dp, _ = _setup(0.1, seed=SEED, B=B, O=60, E=E, lr=0.0, weight_decay=0.0)
            seen = {}

            def loss_fn(out, seen=seen):
                y = out["scene_embeds"]
                if "w" not in seen:
                    seen["w"] = _loss_weights(y)
                seen["tok"], seen["scene"] = out["obj_tokens"], y
                return (y * seen["w"]).sum()

            word.fill_(start)
            step = HotPathTrainStep(model, model._test_opt, dp, loss_fn, R[0], use_graph=use_graph)
            step.capture(R[0])
            torch.cuda.synchronize()
            assert int(word.item()) == start          # the warm-up was rolled back
            words[use_graph] = []
            for b in order:
                loss = step(b)
                torch.cuda.synchronize()
                words[use_graph].append(int(word.item()))
                if use_graph:
                    toks.append(seen["tok"].detach().clone())
                    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(seen["tok"]).all())
                    assert bool(torch.isfinite(seen["scene"]).all())
                    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.requires_grad)
            assert (step.graph is not None) == use_graph and step._sched_direct and model._schedule._ran_blocks
    assert words[True] == words[False] and len(set(words[True] + [start])) == 5
    assert rel(toks[1], toks[0]) > 1e-3               # fresh masks per replay
