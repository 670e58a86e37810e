"""The language-model attention kernels under masks that hide WHOLE 64-key blocks (left padding by hundreds of tokens,
the scene slots of padded objects inside the prompt), measured per row.  Reference side: tests/attn_mask_ref.py (float64,
and a float64 emulation of the roundings the kernels state; tests/test_attn_mask_ref_cpu.py shows that the checker rejects
planted defects).

A. msr3d_attn_fwd / msr3d_attn_bwd (csrc/llm_attn.hip) on the five cases of attn_mask_ref.CASES: every live row of out, dq,
   dk, dv within 2 x the emulation's own worst row (the factor 2: fp32 accumulation order, which the emulation does not
   model), dq and dk a second time against the cancellation-free row scales of attn_mask_ref.grad_row_scales; whole-tensor rel-L2 4e-3 / 8e-3 and lse 2e-3 absolute as in tests/test_llama_layer_gpu.py; EXACT zeros on dead
   query rows (out, dq; lse == +inf) and masked keys (dk, dv); rows whose exact gradient is identically zero (one visible
   key) within the stated fp32 noise; no NaN.  Bit for bit: other finite content in masked k / v rows and dead q / dout
   rows changes no output; keep bytes 2 and 255 are 1; q | k | v | out and dout | dq | dk | dv as column blocks of two
   (B, T, 4 H D) buffers (ld = 4 H D) and every tensor in a buffer of its own with ld = H D + 8 give the bits of the
   contiguous call and write nothing outside their blocks; a second run repeats.
B. msr3d_attn_decode (csrc/llm_decode.hip), split and unsplit: waves and whole splits whose share of the keys is masked.
   Per (row, head) within 2 x a float64 result rounded to bf16 (the kernel is fp32 throughout), whole-tensor 4e-3, the row
   without a visible key exactly 0, content independence on masked slots and slots >= len, run-to-run identity.
C. msr3d_attn_prefix_fwd: cache blocks without a kept key; a prompt whose whole prefix is invisible.  Rule K of
   tests/test_predict_answers_gpu.py (2 x msr3d_attn_fwd on the materialised problem), whole tensor and per row.
D. Through the stack: tests/golden/llama_stack_longpad_seed0*.npz (T 256, a 40-slot hole across a block edge, a row
   left-padded by 200) with the bounds of tests/test_llama_stack_gpu.py (loss rtol 1e-2, gradients 3e-2 on kept rows);
   supervised_from = 210 gives the same loss bits.
E. Through the cache: tests/golden/generate_longpad_seed0.npz (200-slot prompts, a row left-padded by 140, a row with 25
   masked slots inside) with checks C and D of tests/test_generate_gpu.py, bound 2e-2.

Measured on an MI355X (printed by the tests):
A (worst row | the emulation's worst row on the same inputs; whole-tensor rel-L2; the ratio of the two worst rows is
   1.00 in every line but one (dv of pads-63-128-192-255: 0.95) -- the stated roundings account for the kernels' error):
     case                  out                dq                  dk                  dv               lse     dq / dk vs scale
     pads-0-64-65-129      2.98e-3  1.79e-3   1.84     3.01e-3   8.36e-2  2.88e-3   4.17e-3  2.28e-3  1.4e-6  1.31e-2 / 1.21e-2
     pads-63-128-192-255   2.71e-3  1.76e-3   1.93e-1  3.03e-3   1.38e-2  2.96e-3   4.00e-3  2.29e-3  1.5e-6  3.20e-2 / 3.73e-3
     pads-130-512          3.15e-3  1.80e-3   2.16e-1  3.07e-3   2.05e-1  3.04e-3   3.85e-3  2.31e-3  1.2e-6  1.06e-2 / 4.55e-3
     all-padded-row        2.98e-3  1.77e-3   4.98e-1  3.26e-3   1.28e-2  3.15e-3   3.70e-3  2.23e-3  2.2e-6  1.27e-2 / 4.01e-3
     holes                 2.79e-3  1.78e-3   3.53e-1  2.91e-3   7.29e-3  2.90e-3   3.81e-3  2.32e-3  1.4e-6  9.02e-3 / 3.64e-3
   (dq / dk worst rows against ||exact row|| are ill-conditioned rows, see tests/test_attn_mask_ref_cpu.py; the last column
   is the worst row against attn_mask_ref.grad_row_scales, again equal to the emulation's.)  Rows whose exact gradient is
   zero hold at most 6.1e-6 (dq) and 0 (dk) where the stated noise bound is 0.8-4.7e-3.
B worst (row, head) 1.932e-3 (D 64) and 1.917e-3 (D 128), split and unsplit alike: exactly the bf16 rounding of the float64
   result (ratio 1.00); whole-tensor rel-L2 6.2e-4 / 5.6e-4.
C prefix kernel | msr3d_attn_fwd on the materialised problem, rel-L2, max-abs, worst row (the two agree to every digit):
   D  64 S 16: 0.001732 0.006885 3.06e-3     D 128 S 16: 0.001766 0.007708 2.95e-3
   D  64 S 64: 0.001897 0.006773 3.15e-3     D 128 S 64: 0.001885 0.007582 2.90e-3
D logits rel-L2 0.00834; loss relative deviation -2.5e-4 / +5.9e-5; dx 0.01041 on kept rows; worst LoRA gradient
   dA/1/q_proj 0.01628 (bound 3e-2).
E against the fixture: worst step and row 0.01015 (per prompt row 0.00842 / 0.01015 / 0.00934), largest absolute deviation
   0.0402; cached against the full forward: row 0 0.00804, row 1 (left-padded by 140) 0.00997 (bound 2e-2).
No kernel defect was found: every state named above computes what the float64 statement says."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import attn_mask_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUND = 2e-2                                     # tests/test_generate_gpu.py: two bf16 pipelines
NAMES5 = ("out", "lse", "dq", "dk", "dv")


def _ptr(t, col=0):
    return ctypes.c_void_p(t.data_ptr() + col * t.element_size())


def _lib():
    from msr3d_amd import _lib as L
    return L


def _call(name, *a):
    rc = getattr(_lib().load(), name)(*a)
    assert rc == 0, (name, rc)


# ===================================================================================================== A. fwd / bwd
@functools.lru_cache(maxsize=None)
def _solved(name):
    """-> (case on the GPU, exact, emulated): computed once per case, shared by the tests, never written to."""
    c = R.make_case(name, device="cuda")
    args = (c["q"], c["k"], c["v"], c["keep"], c["scale"], c["dout"])
    return c, R.attention_fp64(*args), R.attention_emulated(*args)


def _run(c, q=None, k=None, v=None, dout=None, keep=None, layout="contiguous"):
    """msr3d_attn_fwd + msr3d_attn_bwd -> dict of out, dq, dk, dv (B, T, H, D), lse (B, H, T).
    layout: "contiguous" (ld = H D); "packed" (q | k | v | out column blocks of one (B, T, 4 H D) buffer, dout | dq | dk | dv
    of another, ld = 4 H D); "padded" (every tensor in a (B, T, H D + 8) buffer of its own, ld = H D + 8, the 8 extra
    columns hold a sentinel).  The strided layouts also assert that nothing outside an output's block was written."""
    B, T, H, D = (c[n] for n in "BTHD")
    q, k, v, dout = (c[n] if t is None else t for n, t in (("q", q), ("k", k), ("v", v), ("dout", dout)))
    keep = c["keep"] if keep is None else keep
    HD, dev = H * D, "cuda"
    st = _lib().current_stream_ptr(torch.device(dev))
    lse, delta = torch.empty(B, H, T, device=dev), torch.empty(B, H, T, device=dev)
    SENT = -3.0
    if layout == "contiguous":
        ld = HD
        bufs = {n: t.reshape(B, T, HD).contiguous() for n, t in (("q", q), ("k", k), ("v", v), ("dout", dout))}
        for n in ("out", "dq", "dk", "dv"):
            bufs[n] = torch.empty(B, T, HD, dtype=torch.bfloat16, device=dev)
        P = {n: _ptr(t) for n, t in bufs.items()}
        views = bufs
    elif layout == "packed":
        ld = 4 * HD
        fwd = torch.full((B, T, 4 * HD), SENT, dtype=torch.bfloat16, device=dev)
        bwd = torch.full((B, T, 4 * HD), SENT, dtype=torch.bfloat16, device=dev)
        slots = {"q": (fwd, 0), "k": (fwd, 1), "v": (fwd, 2), "out": (fwd, 3), "dout": (bwd, 0), "dq": (bwd, 1), "dk": (bwd, 2),
                 "dv": (bwd, 3)}
        for n, t in (("q", q), ("k", k), ("v", v), ("dout", dout)):
            buf, i = slots[n]
            buf[:, :, i * HD:(i + 1) * HD] = t.reshape(B, T, HD)
        P = {n: _ptr(buf, i * HD) for n, (buf, i) in slots.items()}
        views = {n: buf[:, :, i * HD:(i + 1) * HD] for n, (buf, i) in slots.items()}
        before = (fwd.clone(), bwd.clone())
    else:
        ld = HD + 8
        bufs = {n: torch.full((B, T, ld), SENT, dtype=torch.bfloat16, device=dev) for n in ("q", "k", "v", "dout", "out", "dq",
                                                                                           "dk", "dv")}
        for n, t in (("q", q), ("k", k), ("v", v), ("dout", dout)):
            bufs[n][:, :, :HD] = t.reshape(B, T, HD)
        P = {n: _ptr(t) for n, t in bufs.items()}
        views = {n: t[:, :, :HD] for n, t in bufs.items()}
    sc = ctypes.c_float(c["scale"])
    _call("msr3d_attn_fwd", B, T, H, D, P["q"], P["k"], P["v"], ld, _ptr(keep), sc, P["out"], _ptr(lse), st)
    _call("msr3d_attn_bwd", B, T, H, D, P["q"], P["k"], P["v"], P["out"], P["dout"], ld, _ptr(keep), sc, _ptr(lse), _ptr(delta),
          P["dq"], P["dk"], P["dv"], st)
    torch.cuda.synchronize()
    if layout == "packed":                           # the inputs' blocks are as they were
        assert torch.equal(fwd[:, :, :3 * HD], before[0][:, :, :3 * HD]) and torch.equal(bwd[:, :, :HD], before[1][:, :, :HD])
    elif layout == "padded":                         # the sentinel columns of every buffer, outputs included
        for n, t in bufs.items():
            assert bool((t[:, :, HD:] == SENT).all()), n
    res = {n: views[n].reshape(B, T, H, D).clone() for n in ("out", "dq", "dk", "dv")}
    res["lse"] = lse
    return res


def _same_bits(a, b, what):
    for n in NAMES5:
        assert torch.equal(a[n], b[n]), "%s: %s differs" % (what, n)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_attention_rows_under_whole_masked_blocks(name):
    c, exact, emu = _solved(name)
    got = _run(c)
    live_q, live_k = R.live_queries(c["keep"]), c["keep"].bool()
    R.check_exact_zeros(c["keep"], **got)
    for n, live, whole in (("out", live_q, R.WHOLE_OUT), ("dq", live_q, R.WHOLE_GRAD), ("dk", live_k, R.WHOLE_GRAD),
                           ("dv", live_k, R.WHOLE_GRAD)):
        e_got, _ = R.row_errors(got[n], exact[n], live)
        e_emu, _ = R.row_errors(emu[n], exact[n], live)
        print("A %s %s: worst row %.3e (emulation %.3e, ratio %.2f), whole-tensor rel-L2 %.3e (emulation %.3e)"
              % (name, n, float(e_got.max()), float(e_emu.max()), float(e_got.max() / e_emu.max()),
                 R.rel_l2(got[n], exact[n]), R.rel_l2(emu[n], exact[n])))
        R.check_rows(got[n], exact[n], emu[n], live, whole=whole, what=n)
    # dq, dk once more against denominators without the cancellation of dS (attn_mask_ref.grad_row_scales): against
    # ||exact row|| the emulation's worst row is an ill-conditioned one and 2 x it bounds little
    dq_s, dk_s = R.grad_row_scales(c["q"], c["k"], c["v"], c["dout"], c["keep"], c["scale"])
    for n, live, den in (("dq", live_q, dq_s), ("dk", live_k, dk_s)):
        e_got, _ = R.row_errors(got[n], exact[n], live, den)
        e_emu, _ = R.row_errors(emu[n], exact[n], live, den)
        print("A %s %s against the cancellation-free scale: worst row %.3e (emulation %.3e, ratio %.2f)"
              % (name, n, float(e_got.max()), float(e_emu.max()), float(e_got.max() / e_emu.max())))
        R.check_rows(got[n], exact[n], emu[n], live, whole=R.WHOLE_GRAD, what=n, den=den)
    lv = live_q[:, None, :].expand(exact["lse"].shape)
    print("A %s lse: largest deviation %.3e" % (name, float((got["lse"].double() - exact["lse"])[lv].abs().max())))
    R.check_lse(got["lse"], exact["lse"], live_q)
    # rows whose exact gradient is identically zero: within the fp32 noise of dS = dP - delta (attn_mask_ref)
    dq_b, dk_b = R.single_key_noise_bound(c["q"], c["k"], c["v"], c["dout"], c["keep"], c["scale"])
    for n, b, live in (("dq", dq_b, live_q), ("dk", dk_b, live_k)):
        zero = (exact[n].norm(dim=-1) == 0) & live[..., None]
        if bool(zero.any()):
            norm = got[n].double().norm(dim=-1)
            print("A %s %s: %d rows with an exactly zero gradient hold at most %.3e (bound there %.3e)"
                  % (name, n, int(zero.sum()), float(norm[zero].max()), float(b[zero][norm[zero].argmax()])))
            # (+ half a bf16 step of the bound: the result is stored in bf16)
            assert bool((norm[zero] <= b[zero] * (1 + 2.0 ** -8)).all()), n
    _same_bits(got, _run(c), "second run")


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_attention_does_not_read_what_the_mask_hides(name):
    c, _, _ = _solved(name)
    base = _run(c)
    B, T, H, D = (c[n] for n in "BTHD")
    g = torch.Generator().manual_seed(7)
    other = lambda: (torch.randn(B, T, H, D, generator=g) * 50).to(torch.bfloat16).cuda()      # noqa: E731
    masked, dead = ~c["keep"].bool(), ~R.live_queries(c["keep"])
    assert bool(masked.any())
    k2, v2, q2, do2 = c["k"].clone(), c["v"].clone(), c["q"].clone(), c["dout"].clone()
    k2[masked], v2[masked] = other()[masked], other()[masked]
    _same_bits(base, _run(c, k=k2, v=v2), "other k / v content on masked keys")
    q2[dead], do2[dead] = other()[dead], other()[dead]
    got = _run(c, q=q2, k=k2, v=v2, dout=do2)
    _same_bits(base, got, "other q / dout content on dead query rows")
    R.check_exact_zeros(c["keep"], **got)
    for byte in (2, 255):
        _same_bits(base, _run(c, keep=c["keep"] * byte), "keep bytes of %d" % byte)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_attention_row_strides_beyond_the_heads(name):
    c, _, _ = _solved(name)
    base = _run(c)
    _same_bits(base, _run(c, layout="packed"), "ld = 4 H D")
    _same_bits(base, _run(c, layout="padded"), "ld = H D + 8")


# ======================================================================================================== B. decode
DECODE_ROWS = [(576, (0, 64)), (576, (0, 65)), (576, (0, 500)), (300, (0, 299)), (300, (0, 300)), (70, (0, 64)), (1, None),
               (400, (100, 260))]                # (len, masked slots); (400, 100 .. 259): more than one split's share
DEAD_ROW = 4


def _decode_case(D):
    from tests.test_llm_decode_gpu import _bf
    gen = torch.Generator(device="cuda").manual_seed(900 + D)
    N, H, Tmax = len(DECODE_ROWS), 4, 640
    q, kc, vc = _bf(N, H * D, gen=gen), _bf(N, Tmax, H, D, gen=gen), _bf(N, Tmax, H, D, gen=gen)
    keep = torch.ones(N, Tmax, dtype=torch.uint8, device="cuda")
    for n, (_, m) in enumerate(DECODE_ROWS):
        if m is not None:
            keep[n, m[0]:m[1]] = 0
    ln = torch.tensor([r[0] for r in DECODE_ROWS], dtype=torch.int32, device="cuda")
    return q, kc, vc, keep, ln, H


@pytest.mark.parametrize("D", [64, 128])
def test_decode_with_waves_and_splits_that_see_no_key(D):
    from tests.test_llm_decode_gpu import _attn_ref, _attn_run
    q, kc, vc, keep, ln, H = _decode_case(D)
    N, Tmax = keep.shape
    assert _lib().load().msr3d_attn_decode_splits(N, H) > 2
    ref = _attn_ref(q, kc, vc, keep, ln, H, D).view(N, H, D)
    emu = R.bf16_round(ref)                                  # the kernel is fp32 throughout: only the store rounds
    live = torch.ones(N, dtype=torch.bool, device="cuda")
    live[DEAD_ROW] = False
    hidden = (~keep.bool()) | (torch.arange(Tmax, device="cuda")[None] >= ln[:, None])
    g = torch.Generator().manual_seed(11)
    kc2, vc2 = kc.clone(), vc.clone()
    kc2[hidden] = (torch.randn(N, Tmax, H, D, generator=g) * 50).to(torch.bfloat16).cuda()[hidden]
    vc2[hidden] = (torch.randn(N, Tmax, H, D, generator=g) * 50).to(torch.bfloat16).cuda()[hidden]
    for split in (True, False):
        out = _attn_run(q, kc, vc, keep, ln, H, D, split=split)
        assert not bool(torch.isnan(out.float()).any())
        assert float(out[DEAD_ROW].float().abs().max()) == 0.0           # no visible key: exactly 0
        r = R.check_rows(out.view(N, H, D), ref, emu, live, whole=R.WHOLE_OUT, what="decode")
        print("B D %d split %s: worst (row, head) %.3e (bf16 rounding of the exact result %.3e, ratio %.2f), whole-tensor "
              "rel-L2 %.3e" % (D, split, r["worst_row"], r["emulated_worst_row"], r["ratio"], r["whole"]))
        assert torch.equal(out, _attn_run(q, kc, vc, keep, ln, H, D, split=split)), "second run"
        assert torch.equal(out, _attn_run(q, kc2, vc2, keep, ln, H, D, split=split)), "content of hidden slots was read"


# ======================================================================================================== C. prefix
def _prefix_case(D, S):
    gen = torch.Generator().manual_seed(5000 + 10 * D + S)
    B, H, Tmax = 3, 2, 320
    C = {16: 5, 64: 2}[S]                                    # 80 / 128 suffix rows a prompt: two query tiles
    bf = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)          # noqa: E731
    q, k, v = bf(B, C, S, H, D), bf(B, C, S, H, D), bf(B, C, S, H, D)
    kc, vc = bf(B, Tmax, H, D), bf(B, Tmax, H, D)
    length = torch.tensor([320, 200, 130], dtype=torch.int32)
    pkeep = torch.ones(B, Tmax, dtype=torch.uint8)
    pkeep[0, :64] = 0                                        # a whole leading block
    pkeep[1, 60:200] = 0                                     # the rest of block 0, blocks 1 and 2, the partial last block
    pkeep[2, :130] = 0                                       # the whole prefix: every candidate sees its own suffix only
    skeep = torch.ones(B, C, S, dtype=torch.uint8)
    return dict(B=B, C=C, S=S, H=H, D=D, Tmax=Tmax, q=q, k=k, v=v, kc=kc, vc=vc, length=length, pkeep=pkeep, skeep=skeep,
                scale=1.0 / math.sqrt(D))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [16, 64])
def test_prefix_kernel_with_cache_blocks_that_hold_no_kept_key(D, S):
    from tests.test_predict_answers_gpu import _run_materialised, _run_prefix, prefix_attention_fp64, rel
    c = _prefix_case(D, S)
    ref = prefix_attention_fp64(c["q"], c["k"], c["v"], c["kc"], c["vc"], c["length"], c["pkeep"], c["skeep"], c["scale"])
    assert bool(torch.isfinite(ref).all())
    # prompt 2 sees no prefix key: the contract there is causal attention over the candidate's own suffix
    own = R.attention_fp64(c["q"][2], c["k"][2], c["v"][2], torch.ones(c["C"], S, dtype=torch.uint8), c["scale"])["out"]
    assert float((ref[2] - own).abs().max()) < 1e-12
    got, parent = _run_prefix(c), _run_materialised(c)
    assert bool(torch.isfinite(got.float()).all())
    e_new, e_par = rel(got, ref), rel(parent, ref)
    a_new, a_par = float((got.double() - ref).abs().max()), float((parent.double() - ref).abs().max())
    live = torch.ones(ref.shape[:-1], dtype=torch.bool)
    r = R.check_rows(got, ref, parent.double(), live, whole=R.WHOLE_OUT, what="prefix")
    print("C D %d S %d: prefix kernel rel-L2 %.6f max-abs %.6f worst row %.3e | msr3d_attn_fwd on the materialised problem "
          "%.6f %.6f %.3e" % (D, S, e_new, a_new, r["worst_row"], e_par, a_par, r["emulated_worst_row"]))
    assert e_new <= 2 * e_par and a_new <= 2 * a_par
    assert torch.equal(_run_prefix(c).view(torch.int16), got.view(torch.int16)), "two calls, two results"
    # finite content of masked cache slots and of slots >= len is not read
    hidden = (~c["pkeep"].bool()) | (torch.arange(c["Tmax"])[None] >= c["length"][:, None])
    g = torch.Generator().manual_seed(3)
    c2 = dict(c, kc=c["kc"].clone(), vc=c["vc"].clone())
    for n in ("kc", "vc"):
        c2[n][hidden] = (torch.randn(c["kc"].shape, generator=g) * 50).to(torch.bfloat16)[hidden]
    assert torch.equal(_run_prefix(c2).view(torch.int16), got.view(torch.int16)), "content of hidden cache slots was read"


# ===================================================================================================== D. the stack
def test_stack_loss_and_gradients_with_a_row_left_padded_by_200():
    from tests.test_llama_stack_gpu import NAMES, _stack, rel
    g = {}
    for part in ("", "_dx", "_lora0", "_lora1"):
        g.update(np.load(os.path.join(GOLD, "llama_stack_longpad_seed0%s.npz" % part)))
    net = _stack(g)
    x = torch.from_numpy(g["x"]).cuda().to(torch.bfloat16).requires_grad_(True)
    keep = torch.from_numpy(g["keep"]).cuda()
    targets = torch.from_numpy(g["targets"]).cuda()
    first = int(g["logits_first_at"])
    assert x.shape[1] == 256 and int(keep[1].sum()) == 56 and not bool(keep[0, 90:130].any()) and first == 210
    lg = net(x, attention_mask=keep)
    e_lg = rel(lg[0, first:first + 4].float(), g["logits_first"])
    loss = net(x, attention_mask=keep, targets=targets)
    print("D: logits rel-L2 %.5f; loss %s against %s (relative deviation %s)"
          % (e_lg, loss.tolist(), g["loss"].tolist(), ((loss.detach().cpu().numpy() - g["loss"]) / g["loss"]).tolist()))
    assert e_lg < 2e-2
    assert np.allclose(loss.detach().cpu().numpy(), g["loss"], rtol=1e-2)
    loss.backward(torch.from_numpy(g["grad_loss"]).cuda())
    rows = keep.bool()
    assert bool(torch.isfinite(x.grad.float()).all())
    errs = {"dx": rel(x.grad.float()[rows], torch.from_numpy(g["dx"]).cuda()[rows])}
    for i, layer in enumerate(net.layers):
        for n in NAMES:
            m = (layer.self_attn if n in layer.self_attn else layer.mlp)[n]
            errs[f"dA/{i}/{n}"] = rel(m.lora_A.weight.grad, g[f"dA/{i}/{n}"])
            errs[f"dB/{i}/{n}"] = rel(m.lora_B.weight.grad, g[f"dB/{i}/{n}"])
    worst = max(errs, key=errs.get)
    print("D: dx rel-L2 %.5f on kept rows; worst LoRA gradient %s %.5f" % (errs["dx"], worst, errs[worst]))
    assert all(e < 3e-2 for e in errs.values()), errs
    assert torch.equal(net(x, attention_mask=keep, targets=targets, supervised_from=first).detach(), loss.detach())


# ======================================================================================================= E. generate
def test_cached_decoding_on_long_prompts_with_whole_masked_blocks():
    from tests.generate_helpers import full_forward_logits, gpu_stack
    from tests.test_generate_gpu import _load, _walk, rel
    g = _load("generate_longpad_seed0.npz")
    assert g["x"].shape[1] == 200 and int(g["keep"][1].sum()) == 60 and int(g["keep"][2].sum()) == 175
    net, emb = gpu_stack(int(g["seed"]))
    got = _walk(net, emb, g)
    # D: every row against the fp32 transformers fixture
    ref = torch.from_numpy(g["logits"])
    errs = torch.tensor([[rel(got[s][n], ref[s, n]) for n in range(ref.shape[1])] for s in range(len(got))])
    dev = max(float((got[s] - ref[s]).abs().max()) for s in range(len(got)))
    print("E/D: rel-L2 worst %.5f (per prompt row: %s), max abs deviation %.4f"
          % (float(errs.max()), [round(float(v), 5) for v in errs.amax(0)], dev))
    assert float(errs.max()) < BOUND, errs
    # C: against the full forward on the same prefix, rows 0 and 1 (both paths rotate consistently there: rotary attention
    # is relative; row 2's masked slots inside the prompt are where arange and cumsum(mask) positions legitimately differ)
    x, keep, seq = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"]), torch.from_numpy(g["sequences"])
    full = full_forward_logits(net, emb, x, keep, seq[:, :-1]).cpu()
    for row in (0, 1):
        e = [rel(got[s][row], full[row, s]) for s in range(len(got))]
        print("E/C: cached vs full forward, row %d: worst %.5f" % (row, max(e)))
        assert max(e) < BOUND, (row, e)
