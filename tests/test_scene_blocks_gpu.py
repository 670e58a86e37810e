"""Scene-local fused blocks (csrc/scene_block.hip, csrc/wgrad_split.hip; round 3): the split/pack kernel
bit for bit against a numpy restatement of the exact three-way bf16 split, the weight-gradient launch
against float64, and the blocks schedule against round 2's strips schedule on every intermediate."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bf16_rne(x):
    """fp32 array -> (bf16 bit patterns uint16, value as fp32)"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return r.astype(np.uint16), (r << 16).astype(np.uint32).view(np.float32)


def _split3(x):
    planes, rem = [], x.astype(np.float32)
    for k in range(3):
        bits, val = _bf16_rne(rem)
        planes.append(bits)
        rem = (rem - val).astype(np.float32)
    return planes


def _pack_ref(op):
    """op (rows, k) fp32 -> [k/32][rows/16][3][64][8] uint16 in MFMA fragment order."""
    rows, k = op.shape
    out = np.zeros((k // 32, rows // 16, 3, 64, 8), np.uint16)
    planes = _split3(op)
    for p in range(3):
        pl = planes[p].reshape(rows // 16, 16, k // 32, 4, 8)      # tile, j, slab, g, e
        out[:, :, p] = pl.transpose(2, 0, 3, 1, 4).reshape(k // 32, rows // 16, 64, 8)   # lane = j + 16 g
    return out


def test_split_pack_matches_the_exact_split_bit_for_bit():
    from msr3d_amd import _lib
    from msr3d_amd.scene_blocks import WeightPacks, head_segments
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((816, 256)) * np.exp(rng.uniform(-6, 6, (816, 256)))).astype(np.float32)
    wt = torch.from_numpy(w).cuda()
    pk = WeightPacks(wt.device)
    pk.add("plain", wt[:256], 256, 256, False)
    pk.add("trans", wt[:512], 256, 512, True)
    segs = head_segments(3)
    pk.add("head", wt, 128, 256, False, segs)
    pk.add("head_t", wt, 256, 128, True, segs)
    pk.launch(_lib.current_stream_ptr(wt.device))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().view(np.uint16) for k, v in pk.bufs.items()}
    head = np.zeros((128, 256), np.float32)
    for d, n, s in segs:
        head[d:d + n] = w[s:s + n]
    want = {"plain": _pack_ref(w[:256]), "trans": _pack_ref(np.ascontiguousarray(w[:512].T)),
            "head": _pack_ref(head), "head_t": _pack_ref(np.ascontiguousarray(head.T))}
    for k in want:
        assert np.array_equal(got[k], want[k].reshape(-1)), k
    # and the three terms reproduce the value to 2^-24 relative
    pl = _split3(w)
    back = sum((p.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for p in pl)
    assert np.max(np.abs(back - w) / np.abs(w)) < 2.0 ** -23


@pytest.mark.parametrize("M,n_out,k_in", [(960, 256, 2048), (976, 816, 256), (150, 256, 63), (37, 256, 3), (960, 4096, 256)])
def test_wgrad_split_vs_float64(M, n_out, k_in):
    from msr3d_amd import _lib
    from msr3d_amd.scene_blocks import WgradTable
    torch.manual_seed(M + n_out)
    dy = torch.randn(M, n_out, device="cuda")
    xw = torch.randn(M, k_in + 5, device="cuda")
    x = xw[:, 2:2 + k_in]                                # unaligned, strided rows
    dW0 = torch.randn(n_out, k_in, device="cuda")
    db0 = torch.randn(n_out, device="cuda")
    dW, db = dW0.clone(), db0.clone()
    t = WgradTable(dy.device)
    t.add(dy.data_ptr(), n_out, n_out, x.data_ptr(), xw.stride(0), k_in, M, dW.data_ptr(), k_in, db.data_ptr())
    t.launch(_lib.current_stream_ptr(dy.device))
    torch.cuda.synchronize()
    want = dW0.double() + dy.double().t() @ x.double()
    wantb = db0.double() + dy.double().sum(0)
    assert float((dW.double() - want).norm() / want.norm()) < 2e-6
    assert float((db.double() - wantb).norm() / wantb.norm()) < 2e-6
    dW2, db2 = dW0.clone(), db0.clone()                  # bit-reproducible: no atomics, no split-K
    t.set_ptr(0, "dW", dW2.data_ptr())
    t.set_ptr(0, "db", db2.data_ptr())
    t.launch(_lib.current_stream_ptr(dy.device))
    torch.cuda.synchronize()
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


@pytest.mark.parametrize("mixed", [False, True, "stream"])
def test_wgrad_pipe_form_gives_the_bits_of_the_loader_multiplier_form(mixed):
    """Round 6's tile kernel (eight waves that load, split, stash AND multiply; the next half-slab's fragment reads under
    the current half-slab's MFMAs) against rounds 4-5's eight loader + eight multiplier waves, on the bench step's problem
    set (whole tiles, and the mixed launch with its half-reductions): the same products summed in the same order --
    torch.equal on every dW and db, odd shapes and unaligned rows included."""
    from msr3d_amd import _lib
    from msr3d_amd.scene_blocks import WgradTable
    lib = _lib.load()
    dev = torch.device("cuda")
    shapes = [(960, 4096, 256), (960, 256, 2048), (960, 2048, 256), (960, 816, 256), (960, 256, 256), (960, 256, 63),
              (960, 256, 3), (957, 256, 768)]
    torch.manual_seed(5)
    ops = []
    for M, n_out, k_in in shapes:
        dy = torch.randn(M, n_out, device=dev)
        xw = torch.randn(M, k_in + 5, device=dev)
        ops.append((dy, xw, xw[:, 1:1 + k_in] if k_in % 2 else xw[:, 2:2 + k_in], torch.randn(n_out, k_in, device=dev),
                    torch.randn(n_out, device=dev)))
    prev = lib.msr3d_wgrad_form(-1)
    out = {}
    try:
        for form in (0, 1):
            assert lib.msr3d_wgrad_form(form) == form
            t = WgradTable(dev)
            t.mixed = bool(mixed)
            t.stream = mixed == "stream" and form == 1      # (the stream launch: the pipe tile dealt to a persistent grid)
            res = []
            for dy, xw, x, dW0, db0 in ops:
                dW, db = dW0.clone(), db0.clone()
                res.append((dW, db))
                t.add(dy.data_ptr(), dy.shape[1], dy.shape[1], x.data_ptr(), xw.stride(0), x.shape[1], dy.shape[0],
                      dW.data_ptr(), x.shape[1], db.data_ptr())
            t.launch(_lib.current_stream_ptr(dev))
            torch.cuda.synchronize()
            if t.stream:
                assert t._stream_plan is not None and t._stream_plan[4] > 100       # (it ran the deal, with cut tiles)
            out[form] = res
    finally:
        lib.msr3d_wgrad_form(prev)
    for (dy, xw, x, dW0, db0), (a, ab), (b, bb) in zip(ops, out[0], out[1]):
        if mixed != "stream":        # (the stream deal cuts other tiles at other slabs than the mixed launch: other sums)
            assert torch.equal(a, b) and torch.equal(ab, bb), (dy.shape, x.shape)
        want = dW0.double() + dy.double().t() @ x.double()
        assert float((b.double() - want).norm() / want.norm()) < 2e-6
        wantb = db0.double() + dy.double().sum(0)
        assert float((bb.double() - wantb).norm() / wantb.norm()) < 2e-6


def test_wgrad_stream_launch_is_bit_reproducible():
    """msr3d_wgrad_stream twice on the same operands: identical bits (parked partials are added by the fixup launch in a
    fixed order: no atomics, no arrival order anywhere)."""
    from msr3d_amd import _lib
    from msr3d_amd.scene_blocks import WgradTable
    dev = torch.device("cuda")
    torch.manual_seed(11)
    shapes = [(960, 4096, 256), (960, 256, 2048), (960, 2048, 256), (960, 816, 256), (960, 256, 768)]
    ops = [(torch.randn(M, n, device=dev), torch.randn(M, k, device=dev)) for M, n, k in shapes]
    outs = []
    for rep in range(2):
        t = WgradTable(dev)
        t.stream = True
        res = []
        for dy, x in ops:
            dW, db = torch.ones(dy.shape[1], x.shape[1], device=dev), torch.ones(dy.shape[1], device=dev)
            res.append((dW, db))
            t.add(dy.data_ptr(), dy.shape[1], dy.shape[1], x.data_ptr(), x.shape[1], x.shape[1], dy.shape[0], dW.data_ptr(),
                  x.shape[1], db.data_ptr())
        t.launch(_lib.current_stream_ptr(dev))
        torch.cuda.synchronize()
        assert t.stream and t._stream_plan is not None and t._stream_plan[4] > 50
        outs.append(res)
    for (a, ab), (b, bb) in zip(*outs):
        assert torch.equal(a, b) and torch.equal(ab, bb)


def test_wgrad_stream_plans_keep_their_device_tensors_across_token_count_changes():
    """A problem's token count toggling between M and 0 (fused_model does it to llm_proj's in a step without an upstream
    gradient) alternates between two stream plans.  A captured graph holds the raw addresses of a plan's device tensors, so
    a replay is safe only if every plan ever launched keeps its tensors, where they are, with their contents, whatever key is
    launched afterwards: the plans of key A at the third launch ARE those of the first, key B's stay alive beside them, and
    the first and third launches give the same bits."""
    from msr3d_amd import _lib
    from msr3d_amd.scene_blocks import WgradTable
    dev = torch.device("cuda")
    st = _lib.current_stream_ptr(dev)
    torch.manual_seed(23)
    ops = []
    for M, n_out, k_in in [(256, 256, 2048), (256, 2048, 256), (256, 256, 256)]:
        ops.append((torch.randn(M, n_out, device=dev), torch.randn(M, k_in, device=dev), torch.randn(n_out, k_in, device=dev),
                    torch.randn(n_out, device=dev)))
    t = WgradTable(dev)
    t.stream = True
    for dy, x, dW0, db0 in ops:
        t.add(dy.data_ptr(), dy.shape[1], dy.shape[1], x.data_ptr(), x.shape[1], x.shape[1], dy.shape[0], 0, x.shape[1], 0)

    def launch(m_third):
        res = [(dW0.clone(), db0.clone()) for _, _, dW0, db0 in ops]          # fresh clones of the same initial values
        for i, (dW, db) in enumerate(res):
            t.set_ptr(i, "dW", dW.data_ptr())
            t.set_ptr(i, "db", db.data_ptr())
        t.set_ptr(2, "M", m_third)
        t.launch(st)
        torch.cuda.synchronize()
        plan = t._stream_plan
        assert plan is not None and plan[4] > 0                               # (a real deal, with cut tiles, for both keys)
        tensors = [plan[0], plan[1], plan[7]]                                 # pieces, wg_first, slot_piece
        return res, tensors, t._stream_key, [(x.data_ptr(), x.cpu().clone()) for x in tensors]

    res_a, tens_a, key_a, snap_a = launch(256)
    _, _, key_b, snap_b = launch(0)                     # (key B's tensors are held by the table alone from here on)
    assert key_b != key_a and not {p for p, _ in snap_a} & {p for p, _ in snap_b}
    res_c, tens_c, key_c, _ = launch(256)
    assert key_c == key_a
    for xa, xc, (pa, ha) in zip(tens_a, tens_c, snap_a):
        assert xc is xa and xc.data_ptr() == pa and torch.equal(xc.cpu(), ha)
    plan_b = t._stream_plans[key_b]
    for xb, (pb, hb) in zip([plan_b[0], plan_b[1], plan_b[7]], snap_b):
        assert xb.data_ptr() == pb and torch.equal(xb.cpu(), hb)
    for (a, ab), (c, cb) in zip(res_a, res_c):
        assert torch.equal(a, c) and torch.equal(ab, cb)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# (0.1, 16, 60, 4096) IS the benchmarked shape -- 16 scenes x 60 objects, Vicuna-7B projector width: the 16-slab
# LINEAR_KSPLIT, the 360-tile weight-gradient grid, the 5,056-workgroup pack; (0.1, 20, 60, 4096) the window step's
# (0.1, 3, 37, 256) / (0.1, 2, 40, 256): the split attention forward's second workgroup with 5 / 8 query rows, its pairwise
# rows on the unaligned (scalar) and on the 16-byte path; O = 20, 13: that workgroup has no rows and leaves at once
@pytest.mark.parametrize("dropout,B,O,E", [(0.0, 3, 20, 256), (0.1, 2, 60, 512), (0.1, 4, 13, 128), (0.1, 3, 37, 256),
                                           (0.1, 2, 40, 256), (0.1, 16, 60, 4096), (0.1, 20, 60, 4096)])
def test_blocks_schedule_matches_strips_schedule_on_every_intermediate(dropout, B, O, E):
    """Same inputs, same dropout keys: every buffer both schedules produce agrees to fp32 rounding
    (<= 2e-5 rel-L2; bf16x3 products vs f32-MFMA products, different summation orders)."""
    import sys
    sys.path.insert(0, "tools")
    from dbg_blocks import run
    from tests.test_fused_model_gpu import _setup
    from msr3d_amd import fused_model
    model, dp, batch = _setup(dropout, B=B, O=O, E=E)
    try:
        sb, sg = run(model, dp, batch, "strips")
        bb, bg = run(model, dp, batch, "blocks")
    finally:
        fused_model.set_mode("blocks")
    assert model._schedule.use_blocks() and model._schedule._ran_blocks and model._schedule.llm_blocks == (E % 256 == 0)
    names = ["x0", "pos", "tok", "scene", "d_la", "d_lb"]
    for i in range(3):
        names += [f"xin{i}", f"qkvc{i}", f"probs{i}", f"ctx{i}", f"s1_{i}", f"s2_{i}", f"t{i}", f"pre{i}", f"h{i}", f"ffn{i}"]
    for k in names:
        assert _rel(bb[k], sb[k]) < 2e-5, (k, _rel(bb[k], sb[k]))
    for i in range(3):
        assert _rel(bb[f"fcacc{i}"], sb[f"fc{i}"]) < 2e-5
        assert _rel(bb[f"d_xacc{i}"], sb[f"d_xin{i}"]) < 5e-5, i
    for k, kb in (("d_ffn", "d_ffn0"), ("d_pre", "d_pre0"), ("d_t", "d_t0"), ("d_fc", "d_fc0"), ("d_qkvc", "d_qkvc0")):
        assert _rel(bb[kb], sb[k]) < 5e-5, k
    # parameter gradients: column sums over B x O token rows of quantities that came through the E-wide reduction
    # d tok = d scene W_llm -- at E = 4096 both schedules carry ~2.5e-5 of fp32 summation-order noise there (the strips meet
    # their K-splits by float atomics), measured 5.2e-5 / 5.6e-5 between them on the last layer's norm2.bias
    gtol = 5e-5 if E <= 512 else 1.5e-4
    for k in sg:
        if k.endswith("w_ks.bias"):
            continue
        if float(sg[k].abs().max()) == 0:
            assert float(bg[k].abs().max()) == 0, k
        else:
            assert _rel(bg[k], sg[k]) < gtol, (k, _rel(bg[k], sg[k]))
