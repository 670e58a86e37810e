"""Closed-set answer ranking on the GPU: msr3d_attn_prefix_fwd (csrc/llm_attn.hip), CachedDecoder.prefill(positions=) /
.score, rank_answers on the engine, MSR3DFullStep.predict_answers.

K. the kernel alone against an fp64 torch statement of its contract (D 64 / 128, S 16 / 32 / 64; len 0, not a multiple of
   64, beyond Tmax; Tmax not a multiple of 64; NaN bit patterns in the cache slots >= len; holes in prefix_keep; padded
   suffix slots; a last 64-row tile that is partly empty; B H not a multiple of 8; a query with no visible key).  Bound:
   2 x the deviation of msr3d_attn_fwd (the existing forward kernel) on the MATERIALISED problem -- every candidate as
   its own sequence prefix + suffix -- from the same fp64 statement, in rel-L2 and in the largest absolute deviation
   (a different block partition of the same bf16 products).
S. `score` against the full forward: logits of the suffix rows after prefill("arange") against LoRALlamaStack.logits on
   the B C repeated sequences, per prompt row (the one with masked slots inside the prompt included): rel-L2 2e-2, the
   bound tests/test_generate_gpu.py and tests/test_llama_stack_gpu.py put on two bf16 pipelines.
R. against the fp32 fixture tests/golden/predict_answers_seed*.npz (every row's selections decided by >= 4 x the parent's
   deviation): the selected set and the winner identical, every loss within 2 x the parent's measured loss deviation.
   The parent's deviation (LoRALlamaStack.forward with targets on the repeated sequences) is measured again and printed.
B. chunked and unchunked `score` give equal bits; prefill(positions="mask") gives the bits of a call without the keyword.
F. MSR3DFullStep.predict_answers end to end on the configuration of tests/golden/full_step_seed0.npz.

Measured on an MI355X (printed by the tests):
K (deviation from the fp64 contract, prefix kernel | msr3d_attn_fwd on the materialised problem):
   D  64 S 16: rel-L2 0.001734 max-abs 0.007133 | 0.001734 0.007133     D 128 S 16: 0.001414 0.007671 | 0.001415 0.007671
   D  64 S 32: rel-L2 0.001818 max-abs 0.006988 | 0.001818 0.006988     D 128 S 32: 0.001156 0.006395 | 0.001156 0.006395
   D  64 S 64: rel-L2 0.001858 max-abs 0.007791 | 0.001858 0.007791     D 128 S 64: 0.001896 0.007016 | 0.001896 0.007016
S (score against the full forward, per prompt row 0 / 1 / 2): suffix rows rel-L2 0.00582 / 0.00651 / 0.00629, worst single
   row 0.00924 / 0.00856 / 0.00847, largest absolute deviation 0.0312; prefill logits rel-L2 0.00000 (the same kernels on the same rows).
R parent (LoRALlamaStack.forward with targets on the 48 repeated sequences) against the fp32 fixture: loss 0.024044,
   prefill logits 0.033945 (0.026171 on the answers' first tokens): the fixture's parent_loss_dev / parent_logit_dev.
   rank_answers against the fixture: loss deviation per prompt row 0.01805 / 0.02223 / 0.02404 (bound 2 x 0.024044);
   selected sets and winners [10, 5, 5] identical."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

from tests.generate_helpers import GOLD, full_forward_logits, gpu_stack
from tests.predict_helpers import answer_set

pytestmark = pytest.mark.gpu
BOUND = 2e-2

def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


# ------------------------------------------------------------------------------------------------------------- kernel
def prefix_attention_fp64(q, k, v, kc, vc, length, pkeep, skeep, scale):
    """The contract in fp64: q, k, v (B, C, S, H, D); kc, vc (B, Tmax, H, D); length (B); pkeep (B, Tmax); skeep (B, C, S)
    -> (B, C, S, H, D).  Cache slots >= min(len, Tmax) are never touched (they may hold NaN)."""
    B, C, S, H, D = q.shape
    Tmax = kc.shape[1]
    out = torch.zeros((B, C, S, H, D), dtype=torch.float64)
    causal = torch.tril(torch.ones((S, S), dtype=torch.bool))
    for b in range(B):
        L = max(0, min(int(length[b]), Tmax))
        kp, vp, mp = kc[b, :L].double(), vc[b, :L].double(), pkeep[b, :L].bool()
        for c in range(C):
            keys = torch.cat([kp, k[b, c].double()], 0)                               # (L + S, H, D)
            vals = torch.cat([vp, v[b, c].double()], 0)
            vis = torch.cat([mp[None].expand(S, L), causal & skeep[b, c].bool()[None]], 1)     # (S, L + S)
            s = torch.einsum("jhd,thd->hjt", q[b, c].double(), keys) * scale
            s = s.masked_fill(~vis[None], -math.inf)
            m = s.max(-1, keepdim=True)[0]
            p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
            den = p.sum(-1, keepdim=True)
            p = torch.where(den > 0, p / den.clamp_min(1e-300), torch.zeros_like(p))
            out[b, c] = torch.einsum("hjt,thd->jhd", p, vals)
    return out


def _kernel_case(D, S, seed=0):
    gen = torch.Generator().manual_seed(1000 * D + S + seed)
    B, H, Tmax = 3, 2, 150
    C = {16: 5, 32: 3, 64: 2}[S]                                   # 80 / 96 rows: the last 64-row tile is partly empty
    bf = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)          # noqa: E731
    q, k, v = bf(B, C, S, H, D), bf(B, C, S, H, D), bf(B, C, S, H, D)
    kc, vc = bf(B, Tmax, H, D), bf(B, Tmax, H, D)
    length = torch.tensor([0, 100, 999], dtype=torch.int32)        # none; partial last block; beyond Tmax (clamped)
    pkeep = (torch.rand(B, Tmax, generator=gen) > 0.2).to(torch.uint8)
    n_real = torch.randint(1, S + 1, (B, C), generator=gen)
    skeep = (torch.arange(S)[None, None] < n_real[:, :, None]).to(torch.uint8)
    skeep[0, 0, 0] = 0                                             # prompt 0 has no prefix: this query sees no key at all
    skeep[1, 1, 2] = 0                                             # a hole inside a suffix
    nan = torch.tensor([0x7FC0, 0xFFFF, 0x7F81], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    for b in range(B):
        L = max(0, min(int(length[b]), Tmax))
        if L < Tmax:                                               # NaN bit patterns in every unused slot
            kc[b, L:] = nan[torch.randint(0, 3, (Tmax - L, H, D), generator=gen)]
            vc[b, L:] = nan[torch.randint(0, 3, (Tmax - L, H, D), generator=gen)]
    return dict(B=B, C=C, S=S, H=H, D=D, Tmax=Tmax, q=q, k=k, v=v, kc=kc, vc=vc, length=length, pkeep=pkeep, skeep=skeep,
                scale=1.0 / math.sqrt(D))


def _run_prefix(c, use_skeep=True):
    from msr3d_amd import _lib
    dev = "cuda"
    t = {n: c[n].to(dev).contiguous() for n in ("q", "k", "v", "kc", "vc", "length", "pkeep", "skeep")}
    out = torch.full((c["B"], c["C"], c["S"], c["H"], c["D"]), float("nan"), dtype=torch.bfloat16, device=dev)
    HD = c["H"] * c["D"]
    rc = _lib.load().msr3d_attn_prefix_fwd(c["B"], c["C"], c["S"], c["Tmax"], c["H"], c["D"], _p(t["q"]), _p(t["k"]), _p(t["v"]),
                                           HD, _p(t["kc"]), _p(t["vc"]), _p(t["length"]), _p(t["pkeep"]),
                                           _p(t["skeep"] if use_skeep else None), ctypes.c_float(c["scale"]), _p(out), HD,
                                           _lib.current_stream_ptr(torch.device(dev)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu()


def _run_materialised(c):
    """The same problem through msr3d_attn_fwd: sequence (b, c) = the prefix rows 0 .. L_b - 1 of cache row b, then the S
    suffix rows of candidate c, padded to a multiple of 64 with masked rows -> the suffix rows' output (B, C, S, H, D)."""
    from msr3d_amd import _lib
    B, C, S, H, D, Tmax = (c[n] for n in ("B", "C", "S", "H", "D", "Tmax"))
    Ls = [max(0, min(int(l), Tmax)) for l in c["length"]]
    Tp = -(-(max(Ls) + S) // 64) * 64
    q = torch.zeros((B, C, Tp, H, D), dtype=torch.bfloat16)
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    keep = torch.zeros((B, C, Tp), dtype=torch.uint8)
    for b, L in enumerate(Ls):
        k[b, :, :L], v[b, :, :L], keep[b, :, :L] = c["kc"][b, :L], c["vc"][b, :L], c["pkeep"][b, :L]
        q[b, :, L:L + S], k[b, :, L:L + S], v[b, :, L:L + S] = c["q"][b], c["k"][b], c["v"][b]
        keep[b, :, L:L + S] = c["skeep"][b]
    q, k, v, keep = (t.view(B * C, *t.shape[2:]).cuda().contiguous() for t in (q, k, v, keep))
    out = torch.empty_like(q)
    lse = torch.empty((B * C, H, Tp), dtype=torch.float32, device="cuda")
    rc = _lib.load().msr3d_attn_fwd(B * C, Tp, H, D, _p(q), _p(k), _p(v), H * D, _p(keep), ctypes.c_float(c["scale"]), _p(out),
                                    _p(lse), _lib.current_stream_ptr(torch.device("cuda")))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = out.cpu().view(B, C, Tp, H, D)
    return torch.stack([out[b, :, L:L + S] for b, L in enumerate(Ls)])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [16, 32, 64])
def test_prefix_kernel_against_its_fp64_contract(D, S):
    c = _kernel_case(D, S)
    ref = prefix_attention_fp64(c["q"], c["k"], c["v"], c["kc"], c["vc"], c["length"], c["pkeep"], c["skeep"], c["scale"])
    assert bool(torch.isfinite(ref).all())
    got, parent = _run_prefix(c), _run_materialised(c)
    e_new, e_par = rel(got, ref), rel(parent, ref)
    a_new, a_par = float((got.double() - ref).abs().max()), float((parent.double() - ref).abs().max())
    print("K: D %d S %d: prefix kernel rel-L2 %.6f max-abs %.6f | msr3d_attn_fwd on the materialised problem rel-L2 %.6f "
          "max-abs %.6f" % (D, S, e_new, a_new, e_par, a_par))
    assert bool(torch.isfinite(got.float()).all()), "a NaN of an unused cache slot (or an unwritten row) reached the result"
    assert bool((got[0, 0, 0] == 0).all()), "a query with no visible key must give 0"
    assert e_new <= 2 * e_par and a_new <= 2 * a_par
    assert torch.equal(_run_prefix(c).view(torch.int16), got.view(torch.int16)), "two calls, two results"
    # suffix_keep NULL = every suffix slot kept
    c1 = dict(c, skeep=torch.ones_like(c["skeep"]))
    assert torch.equal(_run_prefix(c, use_skeep=False).view(torch.int16), _run_prefix(c1).view(torch.int16))


def test_prefix_kernel_rejects_bad_arguments_and_accepts_empty_problems():
    from msr3d_amd import _lib
    h, null, f1 = _lib.load(), ctypes.c_void_p(0), ctypes.c_float(1.0)
    c = _kernel_case(64, 16)
    t = {n: c[n].cuda().contiguous() for n in ("q", "k", "v", "kc", "vc", "length", "pkeep", "skeep")}
    out = torch.empty_like(t["q"])
    args = lambda **o: [o.get("B", 3), o.get("C", 5), o.get("S", 16), o.get("Tmax", 150), 2, o.get("D", 64), _p(t["q"]),    # noqa: E731
                        _p(t["k"]), _p(t["v"]), o.get("ld", 128), o.get("kc", _p(t["kc"])), _p(t["vc"]),
                        o.get("len", _p(t["length"])), _p(t["pkeep"]), _p(t["skeep"]), f1, _p(out), 128, null]
    assert h.msr3d_attn_prefix_fwd(*args(S=8)) == -22 and h.msr3d_attn_prefix_fwd(*args(S=48)) == -22
    assert h.msr3d_attn_prefix_fwd(*args(D=96)) == -22 and h.msr3d_attn_prefix_fwd(*args(ld=120)) == -22
    assert h.msr3d_attn_prefix_fwd(*args(kc=null)) == -22 and h.msr3d_attn_prefix_fwd(*args(len=null)) == -22
    assert h.msr3d_attn_prefix_fwd(*args(B=-1)) == -22
    assert h.msr3d_attn_prefix_fwd(*args(B=0)) == 0 and h.msr3d_attn_prefix_fwd(*args(C=0)) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------- engine and ranking
def _fixture():
    paths = sorted(glob.glob(os.path.join(GOLD, "predict_answers_seed*.npz")))
    assert paths, "the predict_answers fixture is missing"
    return dict(np.load(paths[0], allow_pickle=False))


def _candidates(g):
    """-> x, keep (B, T), suffix tokens (B, C, S - 1) and their keep flags, of the fixture's selected candidates."""
    x, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"].astype(np.int64))
    ids, am = torch.from_numpy(g["answer_ids"]), torch.from_numpy(g["answer_mask"].astype(np.int64))
    top = torch.from_numpy(g["topk_ids"])
    return x, keep, ids[:, 1:][top], am[:, 1:][top].bool()


def test_score_equals_the_full_forward_on_the_repeated_sequences():
    from msr3d_amd.llm.generate import CachedDecoder
    g = _fixture()
    net, emb = gpu_stack(int(g["seed"]))
    x, keep, suf, sk = _candidates(g)
    B, C, S = suf.shape
    eng = CachedDecoder(net)
    eng.reserve(1, 0)
    lg0 = eng.prefill(x.cuda(), keep.cuda(), positions="arange").float().cpu()
    lg = eng.score(emb[suf.cuda()], sk.cuda()).float().cpu()                           # (B, C, S, V)
    full = full_forward_logits(net, emb, x.repeat_interleave(C, 0), keep.repeat_interleave(C, 0), suf.view(B * C, S)).cpu()
    full = full.view(B, C, S + 1, -1)
    for b in range(B):
        e0 = rel(lg0[b], full[b, 0, 0])
        e = rel(lg[b][sk[b]], full[b, :, 1:][sk[b]])
        worst = max(rel(lg[b, c, j], full[b, c, 1 + j]) for c in range(C) for j in range(S) if sk[b, c, j])
        print("S: prompt row %d: prefill rel-L2 %.5f, suffix rows rel-L2 %.5f (worst single row %.5f), max abs %.4f"
              % (b, e0, e, worst, float((lg[b][sk[b]] - full[b, :, 1:][sk[b]]).abs().max())))
        assert e0 < BOUND and e < BOUND and worst < BOUND
    # a second score on the same cache: the cache was only read
    assert torch.equal(eng.score(emb[suf.cuda()], sk.cuda()).float().cpu(), lg)


def test_fixture_ranking():
    from tests.predict_helpers import literal_predict_answers  # noqa: F401  (the fixture's maker; named for the reader)
    g = _fixture()
    net, emb = gpu_stack(int(g["seed"]))
    x, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["keep"].astype(np.int64))
    ids, am = torch.from_numpy(g["answer_ids"]), torch.from_numpy(g["answer_mask"].astype(np.int64))
    C = int(g["num_ans_candidates"])
    out = net.predict_answers(x.cuda(), keep.cuda(), emb, ids.cuda(), am.cuda(), num_ans_candidates=C)
    top, loss = out["topk_ids"].cpu(), out["loss"].cpu()
    ref_top, ref_loss = torch.from_numpy(g["topk_ids"]), torch.from_numpy(g["loss"])
    B = x.shape[0]
    # the parent's own deviation from the fixture, measured again: its full forward + loss on the repeated sequences
    suf_ids, suf_am = ids[ref_top.view(-1)], am[ref_top.view(-1)]                      # (B C, S) whole answers, bos first
    S = suf_ids.shape[1]
    xs = torch.cat([x.repeat_interleave(C, 0)[:, :-1].cuda().to(torch.bfloat16), emb[suf_ids.cuda()]], 1)
    ks = torch.cat([keep.repeat_interleave(C, 0)[:, :-1], suf_am], 1).cuda()
    tg = torch.full(ks.shape, -100, dtype=torch.int64)
    tg[:, -S:] = torch.where(suf_am.bool(), suf_ids, torch.full_like(suf_ids, -100))
    tg[:, -S] = -100
    Tp = -(-xs.shape[1] // 64) * 64
    pad = Tp - xs.shape[1]
    xs = torch.cat([xs, torch.zeros((B * C, pad, xs.shape[2]), dtype=xs.dtype, device="cuda")], 1).contiguous()
    ks = torch.cat([ks, torch.zeros((B * C, pad), dtype=ks.dtype, device="cuda")], 1).contiguous()
    tg = torch.cat([tg, torch.full((B * C, pad), -100, dtype=torch.int64)], 1).cuda().contiguous()
    with torch.no_grad():
        parent_loss = net(xs, attention_mask=ks, targets=tg).float().cpu().view(B, C)
        xp = torch.cat([x, torch.zeros((B, 64 - x.shape[1], x.shape[2]))], 1).cuda().to(torch.bfloat16).contiguous()
        kp = torch.cat([keep, torch.zeros((B, 64 - keep.shape[1]), dtype=keep.dtype)], 1).cuda().contiguous()
        parent_l0 = net.logits(xp, kp)[:, x.shape[1] - 1].float().cpu()
    first = ids[:, 1]
    print("R: parent (full forward on the repeated sequences) against the fp32 fixture: loss max abs deviation %.6f, "
          "first-token logits of the answers %.6f (all logits %.6f); recorded in the fixture: %.6f / %.6f"
          % (float((parent_loss - ref_loss).abs().max()), float((parent_l0[:, first] - torch.from_numpy(g["logits0"])[:, first]).abs().max()),
             float((parent_l0 - torch.from_numpy(g["logits0"])).abs().max()), float(g["parent_loss_dev"]), float(g["parent_logit_dev"])))
    # the new path
    aligned = torch.stack([torch.tensor([float(loss[b][top[b] == a][0]) if bool((top[b] == a).any()) else float("nan")
                                         for a in ref_top[b]]) for b in range(B)])
    print("R: rank_answers against the fixture: loss max abs deviation per prompt row %s; answers %s (fixture %s)"
          % ((aligned - ref_loss).abs().max(1)[0].tolist(), out["answers_id"].tolist(), g["answers_id"].tolist()))
    for b in range(B):                                               # membership: the order inside the top C means nothing
        assert sorted(top[b].tolist()) == sorted(ref_top[b].tolist()), b
    assert out["answers_id"].cpu().tolist() == g["answers_id"].tolist()
    assert float((aligned - ref_loss).abs().max()) <= 2 * float(g["parent_loss_dev"])


def test_chunked_score_and_the_positions_keyword_change_no_bit():
    from msr3d_amd.llm.generate import CachedDecoder
    g = _fixture()
    net, emb = gpu_stack(int(g["seed"]))
    x, keep, suf, sk = _candidates(g)
    B, C, S = suf.shape
    eng = CachedDecoder(net)
    a0 = eng.prefill(x.cuda(), keep.cuda(), positions="arange")
    whole = eng.score(emb[suf.cuda()], sk.cuda())
    parts = eng.score(emb[suf.cuda()], sk.cuda(), max_rows=B * 16 * 3)              # 3 candidates a chunk, the last ragged
    one = eng.score(emb[suf.cuda()], sk.cuda(), max_rows=1)
    assert torch.equal(whole.view(torch.int16), parts.view(torch.int16))
    assert torch.equal(whole.view(torch.int16), one.view(torch.int16))
    e1, e2 = CachedDecoder(net), CachedDecoder(net)
    l1 = e1.prefill(x.cuda(), keep.cuda())
    l2 = e2.prefill(x.cuda(), keep.cuda(), positions="mask")
    assert torch.equal(l1.view(torch.int16), l2.view(torch.int16))
    assert torch.equal(e1.cache.kv[0].view(torch.int16), e2.cache.kv[0].view(torch.int16))
    assert torch.equal(e1.cache.pos, e2.cache.pos) and torch.equal(e1.cache.len, e2.cache.len)
    # and "arange" is another computation on the row with masked slots inside the prompt
    assert not torch.equal(a0[2].view(torch.int16), l1[2].view(torch.int16))
    with pytest.raises(ValueError, match="positions"):
        e1.prefill(x.cuda(), keep.cuda(), positions="other")


# ----------------------------------------------------------------------------------------------------------- end to end
def _model(base="bf16"):
    from tests.test_full_step_gpu import build_model, make_batch
    g = dict(np.load(os.path.join(GOLD, "full_step_seed0.npz"), allow_pickle=False))
    model, c = build_model(g, base=base)
    return model, make_batch(g, c), c


def test_full_step_predict_answers_end_to_end():
    model, batch, c = _model()
    model.eval()
    ids, am = answer_set(5, A=24, S=6, vocab=c["vocab"])
    names = ["answer %d" % i for i in range(24)]
    d = model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, answer_list=names)
    a = d["answers_id"]
    print("F: answers", a.tolist(), "loss", d["answers_loss"].tolist())
    assert a.shape == (c["B"],) and a.dtype == torch.int64 and a.is_cuda
    assert d["answers_topk_ids"].shape == (c["B"], 8) and d["answers_topk_ids"].dtype == torch.int64
    assert d["answers_loss"].shape == (c["B"], 8) and d["answers_loss"].dtype == torch.float32
    assert bool(torch.isfinite(d["answers_loss"]).all())
    assert d["answers"] == [names[i] for i in a.tolist()]
    best = d["answers_loss"].argmin(1)
    assert torch.equal(a, d["answers_topk_ids"].gather(1, best[:, None])[:, 0])
    d2 = model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8, answer_list=names)
    assert torch.equal(d2["answers_id"], a) and torch.equal(d2["answers_loss"], d["answers_loss"])
    assert d2["answers"] == d["answers"]
    assert "answers" not in model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8)
    with pytest.raises(ValueError, match="answer_list"):
        model.predict_answers(dict(batch), ids.cuda(), am.cuda(), answer_list=names[:3])


def test_predict_answers_refuses_fp8_base_weights():
    model, batch, c = _model(base="fp8")
    model.eval()
    ids, am = answer_set(5, A=24, S=6, vocab=c["vocab"])
    with pytest.raises(NotImplementedError, match="fp8"):
        model.predict_answers(dict(batch), ids.cuda(), am.cuda(), num_ans_candidates=8)
