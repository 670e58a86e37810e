"""The launch sequence of every form of the prompter schedule (msr3d_amd/fused_model.py), pinned: one eager forward +
backward per form -- blocks (projector as a block | as a strip GEMM), blocks with the agent token, hybrid, hybrid with
the agent token, strips, an unfrozen encoder, a step without a gradient for scene_embeds -- recorded at the library's
door (`_lib._Entry.fn`, which every schedule launch passes, the ones of scene_blocks included) and compared with the
sequences written below.  A change of the schedule's host code that moves, drops or adds a launch fails here by name.

`record()` also returns every launch's full argument list with pointers replaced by (buffer, byte offset), for comparing
two versions of the host code launch by launch (same library, same arguments: same computation)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, W, FF = 256, 8, 3 * 256 + 8 * 6, 2048      # hidden size, heads, packed q | k | v | cond rows, feed-forward width
NFF = FF // 128                                   # partial slabs of a feed-forward block

BLOCK, ROWS, STRIP, MULTI = "msr3d_scene_block", "msr3d_scene_rows", "msr3d_strip_gemm_f32", "msr3d_gemm_multi_f32"
ATTN_F, ATTN_B = ("msr3d_spatial_attn_fwd",), ("msr3d_spatial_attn_bwd",)


# ---------------------------------------------------------------------------------------------- recording
def _snap(arg, typ):
    """One argument as plain data; pointers as ("ptr", address or None) until `_label` names them."""
    if typ is ctypes.c_void_p:
        v = getattr(arg, "value", arg)
        return ("ptr", v or None)
    if isinstance(typ, type) and issubclass(typ, ctypes._Pointer):          # struct by reference | array of structs
        structs = [arg._obj] if hasattr(arg, "_obj") else list(arg)
        return [{f[0]: _snap(getattr(s, f[0]), f[1]) for f in s._fields_} for s in structs]
    if isinstance(typ, type) and issubclass(typ, ctypes.Array):
        return list(arg)
    v = getattr(arg, "value", arg)
    return ctypes.c_float(v).value if typ is ctypes.c_float else int(v)


def _coarse(name, args):
    from msr3d_amd import _lib
    blk = {v: k for k, v in _lib.BLK.items()}
    pro = {v: k for k, v in _lib.PRO.items()}
    epi = {v: k for k, v in _lib.EPI.items()}
    if name == BLOCK:
        return (name, blk[args[0][0]["kind"]], args[0][0]["N"])
    if name == ROWS:
        return (name, pro[args[0][0]["pro"]], args[0][0]["nslab"])
    if name == STRIP:
        return (name, pro[args[0][0]["pro"]], epi[args[0][0]["epi"]], args[0][0]["N"])
    if name == MULTI:
        return (name, args[0])
    if name.startswith("msr3d_wgrad_"):       # stream | mixed | colsum | plain: chosen by CU count and msr3d_wgrad_form
        return ("wgrad",)
    return (name,)


def _label(trace, buffers):
    """("ptr", address) -> (buffer name, byte offset) inside a known buffer, else ("?", ordinal of first appearance)."""
    spans = [(k, t.data_ptr(), t.numel() * t.element_size()) for k, t in buffers.items() if t is not None and t.numel()]
    seen = {}

    def one(v):
        if isinstance(v, tuple) and len(v) == 2 and v[0] == "ptr":
            p = v[1]
            if p is None:
                return None
            for k, start, n in spans:
                if start <= p < start + n:
                    return (k, p - start)
            return ("?", seen.setdefault(p, len(seen)))
        if isinstance(v, list):
            return [one(x) for x in v]
        if isinstance(v, dict):
            return {k: one(x) for k, x in v.items()}
        return v
    return [(name, one(args)) for name, args in trace]


def record(model, dp, batch, loss="scene"):
    """One eager forward + backward through the model -> (coarse records, labelled full trace)."""
    from msr3d_amd import _lib, hipops
    lib = _lib.load()
    entries = [e for e in (getattr(lib, n) for n in _lib._SIGNATURES) if isinstance(e, _lib._Entry)]
    saved = [e.fn for e in entries]
    trace = []

    def wrap(e, fn):
        types = _lib._SIGNATURES[e.name]

        def f(*a):
            trace.append((e.name, [_snap(x, t) for x, t in zip(a, types)]))
            return fn(*a)
        return f
    seed = hipops.seed_word(torch.device("cuda", torch.cuda.current_device()))
    seed.fill_(12345)
    hipops._salt_counter[0] = 500
    dp.zero_grad()
    try:
        for e, fn in zip(entries, saved):
            e.fn = wrap(e, fn)
        out = model(dict(batch))
        y = out["scene_embeds"] if loss == "scene" else out["obj_tokens"]
        (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
    finally:
        for e, fn in zip(entries, saved):
            e.fn = fn
    dp.finish()
    torch.cuda.synchronize()
    sched = model._schedule
    buffers = {"arena": sched.arena.buf, "params": model._test_opt.flat_p, "grads": dp.flat, "pad": sched.pad,
               "valid": sched.valid, "seed": seed}
    if sched.packs is not None:
        buffers["xp"] = sched.xp
        buffers.update({"pack:" + k: v for k, v in sched.packs.bufs.items()})
    buffers.update({"batch:" + k: v for k, v in batch.items() if isinstance(v, torch.Tensor) and v.is_cuda})
    return [_coarse(n, a) for n, a in trace], _label(trace, buffers)


# ---------------------------------------------------------------------------------------------- the sequences
def _blocks(anchor, hybrid, E, g_scene=True, d_emb=False):
    """forward_blocks + backward_blocks; hybrid: the attention half on the strip kernels."""
    llm_blocks = E % 256 == 0
    if hybrid:
        attn_f = [(STRIP, "plain", "bias", W), ATTN_F, (STRIP, "plain", "bias", D), (ROWS, "ln2", 0)]
        attn_b = [(STRIP, "plain", "bias", D), ATTN_B, (MULTI, 1)]
        slabs = 0                                      # the attention half hands over a whole matrix, no partial slabs
    else:
        attn_f = [(BLOCK, "attn_fwd", 0), (ROWS, "ln2", H)]
        attn_b = [(BLOCK, "attn_bwd", 0)]
        slabs = H
    layer_f = attn_f + [(BLOCK, "ffn_fwd", 0)]
    fwd = ([("msr3d_scene_prologue_agent",) if anchor else ("msr3d_scene_prologue",),
            ("msr3d_split_pack_begin",), (MULTI, 2 if anchor else 1),
            ("msr3d_anchor_front_fwd",) if anchor else ("msr3d_pos_embed_tokens_fwd",)]
           + layer_f + 2 * ([(ROWS, "ln", NFF)] + layer_f)
           + [(ROWS, "ln", NFF), (BLOCK, "linear", E) if llm_blocks else (STRIP, "plain", "bias", E)])

    def layer_b(n):
        return [(ROWS, "lnbwd", n), (BLOCK, "ffn_bwd", 0), (ROWS, "ln2bwd", NFF)] + attn_b
    if not g_scene:
        top, n_top = [], 0
    elif llm_blocks:
        top, n_top = [(BLOCK, "linear_ksplit", 0)], E // 256
    else:
        top, n_top = [(MULTI, 1)], 0
    bwd = (top + layer_b(n_top) + 2 * layer_b(slabs)
           + [(ROWS, "plain", slabs), ("msr3d_anchor_front_bwd",) if anchor else ("msr3d_pos_embed_bwd",), ("wgrad",)]
           + ([(MULTI, 1)] if d_emb else []))
    return fwd + bwd


def _strips(anchor, E, g_scene=True, d_emb=False):
    """forward + backward of the strip schedule."""
    def layer_f(first):
        return [(STRIP, first, "bias", W), ATTN_F, (STRIP, "plain", "bias", D), (STRIP, "ln2", "gelu", FF), (MULTI, 1)]
    fwd = ([("msr3d_scene_prologue_agent",) if anchor else ("msr3d_scene_prologue",),
            ("msr3d_step_begin",), (MULTI, 2 if anchor else 1),
            ("msr3d_anchor_front_fwd",) if anchor else ("msr3d_pos_embed_fwd",)]
           + layer_f("plain" if anchor else "add") + 2 * layer_f("ln") + [(STRIP, "ln", "bias", E)])
    layer_b = [(STRIP, "lnbwd", "gelubwd", FF), (MULTI, 3), (STRIP, "ln2bwd", "bias", D), ATTN_B, (MULTI, 3)]
    bwd = (([(MULTI, 2)] if g_scene else []) + 3 * layer_b
           + ([("msr3d_anchor_front_bwd",), (MULTI, 3)] if anchor else [("msr3d_pos_embed_bwd",), (MULTI, 4 if d_emb else 3)]))
    return fwd + bwd


ATO, AO = "as_transform_for_objects", "as_object"
# id: (mode, situation_type, B, O, E, unfrozen, loss, expected sequence, hybrid)
CASES = {
    "blocks-llm_blocks": ("blocks", ATO, 2, 6, 256, False, "scene", _blocks(False, False, 256), False),
    "blocks-strip_llm_proj": ("blocks", ATO, 2, 6, 128, False, "scene", _blocks(False, False, 128), False),
    "blocks-anchor": ("blocks", AO, 2, 6, 256, False, "scene", _blocks(True, False, 256), False),
    "hybrid": ("blocks", ATO, 1, 70, 256, False, "scene", _blocks(False, True, 256), True),
    "hybrid-anchor": ("blocks", AO, 1, 64, 256, False, "scene", _blocks(True, True, 256), True),          # L = 65
    "strips": ("strips", ATO, 2, 6, 128, False, "scene", _strips(False, 128), False),
    "strips-anchor": ("strips", AO, 2, 6, 128, False, "scene", _strips(True, 128), False),
    "blocks-unfrozen": ("blocks", ATO, 2, 6, 128, True, "scene", _blocks(False, False, 128, d_emb=True), False),
    "strips-unfrozen": ("strips", ATO, 2, 6, 128, True, "scene", _strips(False, 128, d_emb=True), False),
    "blocks-no_g_scene": ("blocks", ATO, 2, 6, 256, False, "tokens", _blocks(False, False, 256, g_scene=False), False),
    "strips-no_g_scene": ("strips", ATO, 2, 6, 256, False, "tokens", _strips(False, 256, g_scene=False), False),
}


def run_case(name):
    """-> (schedule, coarse records, labelled full trace) of one case of CASES."""
    from msr3d_amd import fused_model
    from tests.test_fused_model_gpu import _setup
    mode, situation_type, B, O, E, unfrozen, loss = CASES[name][:7]
    model, dp, batch = _setup(0.1, B=B, O=O, E=E, situation_type=situation_type)
    if unfrozen:
        batch["obj_embeds"].requires_grad_()
    sched = model._schedule
    assert sched.eligible(dict(batch))
    try:
        fused_model.set_mode(mode)
        coarse, full = record(model, dp, batch, loss)
    finally:
        fused_model.set_mode("blocks")
    return sched, coarse, full


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_of_the_schedule(name):
    mode, situation_type, B, O = CASES[name][:4]
    want, hybrid = CASES[name][7:]
    sched, got, _ = run_case(name)
    assert sched._ran_blocks == (mode == "blocks") and sched.hybrid == hybrid
    dm = sched.dims
    assert (dm["D"], dm["H"], dm["W"], dm["FF"], dm["nl"]) == (D, H, W, FF, 3)
    assert dm["L"] == O + (situation_type == AO) and sched.anchor == (situation_type == AO)
    assert len(sched.salts) == 3 and all(len(set(s)) == 4 for s in sched.salts)
    assert len(sched.ps) == 3 and all(p == (0.1, 0.1, 0.1, 0.1) for p in sched.ps)
    if name == "blocks-no_g_scene":             # llm_proj's weight-gradient problem is switched off for this step
        assert sched.wgrad.probs[sched.wg_llm].M == 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: {g} where {w} is expected\n" + "\n".join(map(str, got))
    assert len(got) == len(want), "\n".join(map(str, got[len(want):]))
