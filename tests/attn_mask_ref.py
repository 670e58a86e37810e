"""The reference side of the masked-attention tests (tests/test_attn_mask_ref_cpu.py, tests/test_llm_padding_gpu.py).
Never calls the library: everything here is float64 torch on the bf16 operands, on whatever device they live.

attention_fp64      softmax(scale q k^T + causal + key mask) v, exact: out, lse (log2 units, +inf on a row with no
                    visible key, whose out is 0) and, given dout, dq / dk / dv by autograd.
attention_emulated  the same computation in float64 with the roundings msr3d_amd/csrc/llm_attn.hip STATES (header and
                    kernel comments), and nothing it does not state:
                      forward   online softmax over 64-key blocks; the unnormalised p = exp2(s - m), m the running
                                maximum at that block, is rounded to bf16 before the P V product (its sum is taken
                                unrounded); the normalised output is rounded to bf16, lse is stored as fp32;
                      backward  delta = rowsum(dO o) on the bf16 output; p = exp2(s - lse) and dS = p (dP - delta) are
                                rounded to bf16 before their products (dV = P^T dO, dQ = scale dS K, dK = scale dS^T Q);
                                dq / dk / dv are rounded to bf16.
                    The fp32 accumulation order of the matrix instructions is NOT modelled: that is the factor 2 below.
check_rows          error per row (last axis) of `got` against `exact`, bounded by 2 x the emulation's own worst row on the
                    same inputs, plus the whole-tensor rel-L2 bound the existing attention tests use.
grad_row_scales     cancellation-free denominators for the rows of dq and dk: check_rows is run on those a second time
                    with them, which is the run that can see one gradient row off by 1 %.
check_exact_zeros   what the kernels promise exactly: a query row with no visible key gives out == 0, lse == +inf and takes
                    no gradient (dq == 0); a masked key takes none either (dk == dv == 0); nothing is NaN.
"""
import math

import numpy as np
import torch

BLK = 64                                     # keys per block of the kernels
LOG2E = 1.4426950408889634
WHOLE_OUT, WHOLE_GRAD, LSE_ABS = 4e-3, 8e-3, 2e-3      # the bounds of tests/test_llama_layer_gpu.py, unchanged


def bf16_round(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def visibility(keep):
    """keep (B, T) -> (B, 1, T, T) bool: key j is visible to query i iff j <= i and keep[j]."""
    T = keep.shape[1]
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=keep.device))
    return causal[None, None] & keep.bool()[:, None, None, :]


def live_queries(keep):
    """(B, T) bool: the query rows that see at least one key."""
    return keep.bool().cumsum(1) > 0


def _heads_first(t, grad=False):
    return t.detach().double().permute(0, 2, 1, 3).contiguous().requires_grad_(grad)      # (B, H, T, D)


def attention_fp64(q, k, v, keep, scale, dout=None):
    """q, k, v (B, T, H, D), keep (B, T) -> dict(out (B, T, H, D), lse (B, H, T) in log2 units[, dq, dk, dv])."""
    qd, kd, vd = (_heads_first(t, dout is not None) for t in (q, k, v))
    vis = visibility(keep)
    s = (qd @ kd.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True)[0]
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m).detach()
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    alive = den > 0
    p = torch.where(alive, p / den.clamp_min(1e-300), torch.zeros_like(p))
    o = p @ vd
    lse = torch.where(alive, (m + torch.log(den.clamp_min(1e-300))) / math.log(2.0), torch.full_like(m, math.inf))
    res = {"out": o.detach().permute(0, 2, 1, 3).contiguous(), "lse": lse.detach()[..., 0]}
    if dout is not None:
        o.backward(_heads_first(dout))
        for n, t in (("dq", qd), ("dk", kd), ("dv", vd)):
            res[n] = t.grad.permute(0, 2, 1, 3).contiguous()
    return res


def attention_emulated(q, k, v, keep, scale, dout=None):
    """As attention_fp64, with the stated roundings of the kernels (module docstring)."""
    qd, kd, vd = (_heads_first(t) for t in (q, k, v))
    B, H, T, D = qd.shape
    assert T % BLK == 0
    c = float(np.float32(scale) * np.float32(LOG2E))          # the kernels fold the scale with log2 e in fp32
    vis = visibility(keep)
    s = (qd @ kd.transpose(-1, -2)) * c
    x = s.masked_fill(~vis, -math.inf)
    m_run = torch.full((B, H, T, 1), -math.inf, dtype=torch.float64, device=qd.device)
    l_run = torch.zeros_like(m_run)
    acc = torch.zeros_like(qd)
    for kb in range(T // BLK):
        xb = x[..., kb * BLK:(kb + 1) * BLK]
        m_new = torch.maximum(m_run, xb.max(-1, keepdim=True)[0])
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m_run - m_use)
        pb = torch.exp2(xb - m_use)
        l_run = l_run * alpha + pb.sum(-1, keepdim=True)
        acc = acc * alpha + bf16_round(pb) @ vd[..., kb * BLK:(kb + 1) * BLK, :]
        m_run = m_new
    alive = l_run > 0
    inv = torch.where(alive, 1.0 / l_run.clamp_min(1e-300), torch.zeros_like(l_run))
    o = bf16_round(acc * inv)
    lse = torch.where(alive, m_run + torch.log2(l_run.clamp_min(1e-300)), torch.full_like(m_run, math.inf))
    lse = lse.float().double()
    res = {"out": o.permute(0, 2, 1, 3).contiguous(), "lse": lse[..., 0]}
    if dout is not None:
        do = _heads_first(dout)
        delta = (do * o).sum(-1, keepdim=True)
        p = torch.where(vis, torch.exp2(s - lse), torch.zeros_like(s))
        ds = bf16_round(p * (do @ vd.transpose(-1, -2) - delta))
        dv = bf16_round(bf16_round(p).transpose(-1, -2) @ do)
        dq = bf16_round((ds @ kd) * scale)
        dk = bf16_round((ds.transpose(-1, -2) @ qd) * scale)
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            res[n] = t.permute(0, 2, 1, 3).contiguous()
    return res


def row_errors(got, exact, live, den=None):
    """-> (errors of the live rows whose exact value is not identically zero, mask of those rows).  A row whose exact
    value IS zero (dq of a query with one visible key: a softmax over one element has no gradient) has no relative
    error; single_key_noise_bound states what such a row may hold.  den: other denominators than ||exact_row||
    (grad_row_scales)."""
    got, exact = got.double(), exact.double()
    live = live.expand(exact.shape[:-1]) if live.dim() == exact.dim() - 1 else live[..., None].expand(exact.shape[:-1])
    den = exact.norm(dim=-1) if den is None else den
    rows = live & (den > 0)
    return ((got - exact).norm(dim=-1)[rows] / den[rows]), rows


def check_rows(got, exact, emulated, live, whole=WHOLE_OUT, what="out", den=None):
    """got, exact, emulated (..., D); live (...) bool, or one axis shorter (broadcast over heads): the rows to measure.
    Asserts every measured row of `got` within 2 x the emulation's worst row, and the whole-tensor rel-L2 over the live rows
    below `whole`; returns the figures."""
    e_got, rows = row_errors(got, exact, live, den)
    e_emu, _ = row_errors(emulated, exact, live, den)
    assert e_got.numel() > 0, what
    worst_got, worst_emu = float(e_got.max()), float(e_emu.max())
    lv = rows[..., None].expand(exact.shape)
    tot = rel_l2(got.double()[lv], exact.double()[lv])
    res = {"worst_row": worst_got, "emulated_worst_row": worst_emu, "ratio": worst_got / max(worst_emu, 1e-300),
           "whole": tot, "emulated_whole": rel_l2(emulated.double()[lv], exact.double()[lv])}
    assert worst_emu > 0, what
    assert worst_got <= 2 * worst_emu, "%s: worst row %.3e above 2 x the emulation's worst row %.3e (row %s)" % (
        what, worst_got, worst_emu, [int(i) for i in torch.nonzero(rows)[int(e_got.argmax())]])
    assert tot < whole, "%s: whole-tensor rel-L2 %.3e above %.1e" % (what, tot, whole)
    return res


def check_lse(lse, exact, live):
    """lse, exact (B, H, T) in log2 units, live (B, T): 2e-3 absolute on the live rows, +inf on the others."""
    lv = live[:, None, :].expand(exact.shape)
    dev = float((lse.double() - exact.double())[lv].abs().max()) if bool(lv.any()) else 0.0
    assert dev < LSE_ABS, "lse: %.3e above %.1e" % (dev, LSE_ABS)
    assert bool((lse[~lv] == math.inf).all()), "lse: a row with no visible key must hold +inf"
    return dev


def check_exact_zeros(keep, out=None, lse=None, dq=None, dk=None, dv=None):
    """Tensors (B, T, H, D) (lse (B, H, T)); keep (B, T).  Exact: see the module docstring."""
    dead, masked = ~live_queries(keep), ~keep.bool()
    for n, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        if t is None:
            continue
        assert not bool(torch.isnan(t.double()).any()), "%s holds a NaN" % n
    for n, t, rows in (("out", out, dead), ("dq", dq, dead), ("dk", dk, masked), ("dv", dv, masked)):
        if t is not None and bool(rows.any()):
            worst = float(t.double()[rows].abs().max())
            assert worst == 0.0, "%s: %.3e on a row that must be exactly 0" % (n, worst)
    if lse is not None and bool(dead.any()):
        assert bool((lse.permute(0, 2, 1)[dead] == math.inf).all()), "lse: a row with no visible key must hold +inf"


def grad_row_scales(q, k, v, dout, keep, scale):
    """||dq_i|| and ||dk_j|| are poor yardsticks for their own rows: dS_ij = P_ij (dP_ij - delta_i) cancels where P is close
    to one-hot, the exact row is then orders of magnitude below its terms, and 2^-9 of a TERM (delta is formed on the
    bf16-rounded output) is a large fraction of it -- the emulation's own worst dq row is off by 0.2 to 1.8 of its norm, so
    2 x that bounds nothing.  The scales here are the same sums without the cancellation,
        dq_i: scale || sum_j P_ij (|dP_ij| + |delta_i|) |k_j| ||     dk_j: scale || sum_i P_ij (|dP_ij| + |delta_i|) |q_i| ||
    (exact float64 quantities): an error measured against them is a fraction of the row's terms.
    -> (dq_scale, dk_scale) (B, T, H), zero on dead query rows / masked keys."""
    qd, kd, vd, do = (_heads_first(t) for t in (q, k, v, dout))
    vis = visibility(keep)
    s = ((qd @ kd.transpose(-1, -2)) * scale).masked_fill(~vis, -math.inf)
    p = torch.softmax(s, -1).nan_to_num(0.0)
    dp = do @ vd.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    a = p * (dp.abs() + delta.abs())
    dq_scale = ((a @ kd.abs()) * scale).norm(dim=-1)
    dk_scale = ((a.transpose(-1, -2) @ qd.abs()) * scale).norm(dim=-1)
    return dq_scale.permute(0, 2, 1).contiguous(), dk_scale.permute(0, 2, 1).contiguous()


def single_key_noise_bound(q, k, v, dout, keep, scale):
    """A query i that sees ONE key j has P = 1 there and dS = dP - delta = <v_j, dO_i> - <o_i, dO_i> with o_i = v_j: zero,
    computed by the kernels as the difference of two fp32 sums of the same D products in different orders.  Each sum is
    within D 2^-24 sum|v dO| of the exact one, so |dS| <= D 2^-23 sum|v_j dO_i| =: e_i (bf16 rounding of dS can only add
    2^-8 of it: the factor 1.01).  -> (dq_bound, dk_bound) (B, T, H): ||dq_i|| <= scale e_i ||k_j||, and key j takes at most
    scale sum_i e_i ||q_i|| from such queries.  Zero for every other row."""
    B, T, H, D = q.shape
    vis = visibility(keep)[:, 0]                                         # (B, T, T)
    single = vis.sum(-1) == 1                                            # (B, T)
    key = vis.to(torch.int8).argmax(-1)                                  # (B, T) the one visible key where single
    idx = key[:, :, None, None].expand(B, T, H, D)
    vj, kj = v.double().gather(1, idx), k.double().gather(1, idx)
    e = 1.01 * D * 2.0 ** -23 * (vj * dout.double()).abs().sum(-1) * single[:, :, None]          # (B, T, H)
    dq_bound = scale * e * kj.norm(dim=-1)
    dk_bound = torch.zeros_like(dq_bound).scatter_add(1, key[:, :, None].expand(B, T, H), scale * e * q.double().norm(dim=-1))
    return dq_bound, dk_bound


# ---- the cases of tests/test_llm_padding_gpu.py part A (B, T, H, D, mask), shared with the CPU self-check -------------
def _pads(*n):
    def f(keep):
        for b, p in enumerate(n):
            keep[b, :p] = 0
    return f


def _holes(keep):
    keep[0, 50:90] = 0                       # a hole across a block edge: the scene slots of padded objects
    keep[1, :70] = 0
    keep[1, 64:128] = 0                      # a whole interior block


CASES = [
    ("pads-0-64-65-129", 4, 256, 2, 64, _pads(0, 64, 65, 129)),
    ("pads-63-128-192-255", 4, 256, 2, 128, _pads(63, 128, 192, 255)),
    ("pads-130-512", 2, 576, 1, 128, _pads(130, 512)),
    ("all-padded-row", 3, 128, 2, 64, _pads(128, 0, 64)),          # row 0 has no real token at all
    ("holes", 2, 192, 2, 128, _holes),
]
CASE_IDS = [c[0] for c in CASES]


def make_case(name, device="cpu"):
    """-> dict(B, T, H, D, q, k, v, dout (B, T, H, D) bf16 = randn 1.5, keep (B, T) uint8, scale)."""
    _, B, T, H, D, mask = CASES[CASE_IDS.index(name)]
    g = torch.Generator().manual_seed(B * 1000 + T + D)
    mk = lambda: (torch.randn(B, T, H, D, generator=g) * 1.5).to(torch.bfloat16).to(device)      # noqa: E731
    q, k, v, dout = mk(), mk(), mk(), mk()
    keep = torch.ones(B, T, dtype=torch.uint8)
    mask(keep)
    return dict(B=B, T=T, H=H, D=D, q=q, k=k, v=v, dout=dout, keep=keep.to(device), scale=1.0 / math.sqrt(D))
