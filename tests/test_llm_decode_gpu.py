"""The decode kernels (csrc/llm_decode.hip), each entry alone against a float64 torch statement of it on bf16-rounded
inputs.  Tolerances are the ones the existing tests state for the same kind of result: a bf16 product against float64
4e-3 rel-L2 (tests/test_lora_gpu.py), the fused attention 4e-3, the rotation's closed form 3e-3, SwiGLU 4e-3
(tests/test_llama_layer_gpu.py).  Argument validation goes through the C ABI without a launch."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _lib():
    from msr3d_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    rc = getattr(L.load(), name)(*args)
    L.check(rc, name)


def _st():
    return _lib().current_stream_ptr(torch.device("cuda"))


def _bf(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen, device="cuda") * scale).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------- attention
def _attn_case(N, H, D, Tmax, lens, gen, pad_frac=0.2, dead_row=None):
    q = _bf(N, H * D, gen=gen)
    kc, vc = _bf(N, Tmax, H, D, gen=gen), _bf(N, Tmax, H, D, gen=gen)
    keep = (torch.rand(N, Tmax, generator=gen, device="cuda") >= pad_frac).to(torch.uint8)
    keep[:, 0] = 1
    if dead_row is not None:
        keep[dead_row] = 0
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    return q, kc, vc, keep, ln


def _attn_run(q, kc, vc, keep, ln, H, D, len_add=0, split=True):
    N, Tmax = kc.shape[:2]
    out = torch.full((N, H * D), 7.0, dtype=torch.bfloat16, device="cuda")
    S = _lib().load().msr3d_attn_decode_splits(N, H) if split else 1
    ws = torch.empty(N * H * S * (D + 2), dtype=torch.float32, device="cuda") if S > 1 else None
    _call("msr3d_attn_decode", N, Tmax, H, D, _p(q), H * D, _p(kc), _p(vc), _p(ln), len_add, _p(keep),
          ctypes.c_float(1.0 / math.sqrt(D)), _p(out), H * D, _p(ws), ws.numel() if ws is not None else 0, _st())
    torch.cuda.synchronize()
    return out


def _attn_ref(q, kc, vc, keep, ln, H, D, len_add=0):
    N, Tmax = kc.shape[:2]
    qd = q.double().view(N, H, 1, D)
    kd, vd = kc.double().permute(0, 2, 1, 3), vc.double().permute(0, 2, 1, 3)              # (N, H, T, D)
    S = (qd @ kd.transpose(-1, -2)) / math.sqrt(D)                                         # (N, H, 1, T)
    vis = (torch.arange(Tmax, device="cuda")[None] < (ln + len_add)[:, None]) & keep.bool()
    P = torch.softmax(S.masked_fill(~vis[:, None, None], float("-inf")), -1).nan_to_num(0.0)
    return (P @ vd).reshape(N, H * D)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [1, 5, 20])
def test_attn_decode_matches_float64_at_every_length(N, D):
    gen = torch.Generator(device="cuda").manual_seed(100 * N + D)
    H, Tmax = 8, 576
    base = [1, 7, 64, 65, 333, 576]
    for shift in range(len(base) if N == 1 else 2):
        lens = [base[(n + shift) % len(base)] for n in range(N)]
        dead = 2 if N > 2 else None
        q, kc, vc, keep, ln = _attn_case(N, H, D, Tmax, lens, gen, dead_row=dead)
        for split in (True, False):
            out = _attn_run(q, kc, vc, keep, ln, H, D, split=split)
            ref = _attn_ref(q, kc, vc, keep, ln, H, D)
            assert rel(out, ref) < 4e-3, (lens, split)
            if dead is not None:
                assert float(out[dead].float().abs().max()) == 0.0           # no visible key: 0, as msr3d_attn_fwd
        assert torch.equal(_attn_run(q, kc, vc, keep, ln, H, D), _attn_run(q, kc, vc, keep, ln, H, D))     # same bits


def test_attn_decode_len_add_and_no_mask():
    gen = torch.Generator(device="cuda").manual_seed(5)
    N, H, D, Tmax = 5, 8, 128, 200
    q, kc, vc, keep, ln = _attn_case(N, H, D, Tmax, [10, 199, 64, 1, 128], gen, pad_frac=0.0)
    out = _attn_run(q, kc, vc, None, ln, H, D, len_add=1)
    assert rel(out, _attn_ref(q, kc, vc, torch.ones_like(keep), ln, H, D, len_add=1)) < 4e-3
    # a length beyond the cache is clamped to it, not followed
    ln2 = torch.full((N,), 100000, dtype=torch.int32, device="cuda")
    out = _attn_run(q, kc, vc, keep, ln2, H, D)
    assert rel(out, _attn_ref(q, kc, vc, keep, torch.full_like(ln2, Tmax), H, D)) < 4e-3


# ----------------------------------------------------------------------------------------------------------- rotation
def _tables(T, D):
    from msr3d_amd.llm.decoder import rope_tables
    return rope_tables(T, D, 10000.0, torch.device("cuda"))


def _rope_closed(x, pos, cs, sn):
    """x (..., H, D) double, pos (...) long."""
    D = x.shape[-1]
    rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    return x * cs.double()[pos][..., None, :] + rot * sn.double()[pos][..., None, :]


@pytest.mark.parametrize("D", [64, 128])
def test_rope_positions_equals_rope_inplace_for_arange_and_the_closed_form_otherwise(D):
    gen = torch.Generator(device="cuda").manual_seed(D)
    B, T, H = 3, 64, 8
    cs, sn = _tables(T, D)
    a, b = _bf(B, T, H, D, gen=gen), _bf(B, T, H, D, gen=gen)
    a1, b1, a2, b2 = a.clone(), b.clone(), a.clone(), b.clone()
    _call("msr3d_rope_inplace2", B, T, H, D, _p(a1), _p(b1), _p(cs), _p(sn), 0, _st())
    pos = torch.arange(T, dtype=torch.int32, device="cuda")[None].repeat(B, 1).contiguous()
    _call("msr3d_rope_positions", B, T, H, D, _p(a2), _p(b2), _p(pos), _p(cs), _p(sn), T, _st())
    assert torch.equal(a1, a2) and torch.equal(b1, b2)
    keep = torch.ones(B, T, dtype=torch.long, device="cuda")
    keep[1, :9] = 0
    keep[2, 6:10] = 0
    pos = (keep.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()
    a3, b3 = a.clone(), b.clone()
    _call("msr3d_rope_positions", B, T, H, D, _p(a3), _p(b3), _p(pos), _p(cs), _p(sn), T, _st())
    assert rel(a3, _rope_closed(a.double(), pos.long(), cs, sn)) < 3e-3
    assert rel(b3, _rope_closed(b.double(), pos.long(), cs, sn)) < 3e-3
    only = a.clone()
    _call("msr3d_rope_positions", B, T, H, D, _p(only), _p(None), _p(pos), _p(cs), _p(sn), T, _st())
    assert torch.equal(only, a3)


@pytest.mark.parametrize("D", [64, 128])
def test_rope_kv_append_rotates_by_the_rows_position_and_writes_the_rows_slot(D):
    gen = torch.Generator(device="cuda").manual_seed(D + 1)
    N, H, Tmax = 5, 8, 40
    HD = H * D
    cs, sn = _tables(Tmax, D)
    qkv = _bf(N, 3 * HD, gen=gen)                     # q | k | v as column blocks of one buffer (ld = 3 H D)
    q0, k0, v0 = (qkv[:, i * HD:(i + 1) * HD].clone() for i in range(3))
    pos = torch.tensor([0, 3, 17, 39, 8], dtype=torch.int32, device="cuda")
    ln = torch.tensor([5, 0, 39, 12, 40], dtype=torch.int32, device="cuda")          # the last row's cache is full
    kc = _bf(N, Tmax, H, D, gen=gen)
    vc = _bf(N, Tmax, H, D, gen=gen)
    kc0, vc0 = kc.clone(), vc.clone()
    _call("msr3d_rope_kv_append", N, H, D, Tmax, _p(qkv), ctypes.c_void_p(qkv.data_ptr() + 2 * HD),
          ctypes.c_void_p(qkv.data_ptr() + 4 * HD), 3 * HD, _p(pos), _p(ln), _p(cs), _p(sn), Tmax, _p(kc), _p(vc), _st())
    torch.cuda.synchronize()
    # bit-identical to msr3d_rope_inplace where the position is the table row it reads: rotate row n as token pos[n]
    for n in range(N):
        t = int(pos[n])
        full_q = torch.zeros(1, Tmax, H, D, dtype=torch.bfloat16, device="cuda")
        full_k = torch.zeros_like(full_q)
        full_q[0, t] = q0[n].view(H, D)
        full_k[0, t] = k0[n].view(H, D)
        _call("msr3d_rope_inplace2", 1, Tmax, H, D, _p(full_q), _p(full_k), _p(cs), _p(sn), 0, _st())
        assert torch.equal(qkv[n, :HD].view(H, D), full_q[0, t])
        assert rel(qkv[n, :HD].view(H, D), _rope_closed(q0[n].view(H, D).double(), pos[n].long(), cs, sn)) < 3e-3
        slot = int(ln[n])
        if slot < Tmax:
            assert torch.equal(kc[n, slot], full_k[0, t]) and torch.equal(vc[n, slot], v0[n].view(H, D))
            kc0[n, slot], vc0[n, slot] = kc[n, slot], vc[n, slot]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)              # nothing else was written
    assert torch.equal(qkv[:, HD:], torch.cat([k0, v0], 1))           # k and v themselves are only read


# ------------------------------------------------------------------------------------------------------------ reorder
def test_kv_reorder_is_an_exact_gather_of_the_live_rows():
    gen = torch.Generator(device="cuda").manual_seed(9)
    planes, N, Tmax, HD = 4, 6, 50, 512
    src = _bf(planes, N, Tmax, HD, gen=gen)
    ln = torch.tensor([50, 1, 17, 0, 33, 49], dtype=torch.int32, device="cuda")
    for idx in ([5, 4, 3, 2, 1, 0], [0, 0, 2, 2, 2, 5]):                                   # a permutation; repeats
        bi = torch.tensor(idx, dtype=torch.int32, device="cuda")
        dst = torch.full_like(src, 3.0)
        _call("msr3d_kv_reorder", planes, N, Tmax, HD, _p(src), _p(dst), _p(bi), _p(ln), _st())
        torch.cuda.synchronize()
        for n, f in enumerate(idx):
            L = int(ln[f])
            assert torch.equal(dst[:, n, :L], src[:, f, :L])
            assert bool((dst[:, n, L:] == 3.0).all())                                      # rows beyond the length: untouched
    bad = torch.tensor([0, 1, 99, -1, 4, 5], dtype=torch.int32, device="cuda")             # not rows of the cache: skipped
    dst = torch.full_like(src, 3.0)
    _call("msr3d_kv_reorder", planes, N, Tmax, HD, _p(src), _p(dst), _p(bad), _p(ln), _st())
    torch.cuda.synchronize()
    assert bool((dst[:, 2] == 3.0).all()) and bool((dst[:, 3] == 3.0).all()) and torch.equal(dst[:, 0], src[:, 0])


# ------------------------------------------------------------------------------------------------------------- skinny
def _skinny(M, K, R, P, P2, jobs, swiglu=0):
    L = _lib()
    arr = (L.SkinnyJob * len(jobs))(*[L.SkinnyJob(W.data_ptr(), K, B2.data_ptr() if B2 is not None else 0, R,
                                                  C.data_ptr() if C is not None else 0, W.shape[0], W.shape[0])
                                      for W, B2, C in jobs])
    _call("msr3d_bf16_skinny_lowrank", M, K, R, _p(P), K, _p(P2), R, len(jobs), arr, swiglu, _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", [1, 5, 16, 20, 32])
@pytest.mark.parametrize("K,N", [(512, 512), (1024, 512), (512, 1024), (4096, 4096), (4096, 11008), (11008, 4096),
                                 (5120, 13824), (13824, 5120), (4096, 32000)])
def test_skinny_lowrank_matches_gemm_lowrank_and_float64(M, K, N):
    from msr3d_amd.llm import lora
    gen = torch.Generator(device="cuda").manual_seed(M * 7 + K + N)
    P, W = _bf(M, K, gen=gen, scale=0.5), _bf(N, K, gen=gen, scale=0.5 / K ** 0.5)
    P2, B2 = _bf(M, 64, gen=gen, scale=0.5), _bf(N, 64, gen=gen, scale=0.5)
    for R in (64, 0):
        C = torch.full((M, N), 9.0, dtype=torch.bfloat16, device="cuda")
        _skinny(M, K, R, P, P2 if R else None, [(W, B2 if R else None, C)])
        want = P.double() @ W.double().t() + (P2.double() @ B2.double().t() if R else 0.0)
        assert rel(C, want) < 4e-3
        G = torch.empty_like(C)
        lora._gemm(M, N, K, R, P, K, W, K, P2 if R else None, R, B2 if R else None, R, G, N, False, 1.0, P.device)
        torch.cuda.synchronize()
        assert rel(C, G.float()) < 4e-3


@pytest.mark.parametrize("M", [1, 5, 20, 32])
def test_skinny_three_weights_in_one_launch_and_the_swiglu_epilogue(M):
    gen = torch.Generator(device="cuda").manual_seed(M)
    K, N = 512, 1024
    P, P2 = _bf(M, K, gen=gen, scale=0.5), _bf(M, 64, gen=gen, scale=0.5)
    Ws = [_bf(n, K, gen=gen, scale=1.0 / K ** 0.5) for n in (512, 512, 1024)]
    Bs = [_bf(n, 64, gen=gen, scale=0.3) for n in (512, 512, 1024)]
    Cs = [torch.empty((M, w.shape[0]), dtype=torch.bfloat16, device="cuda") for w in Ws]
    _skinny(M, K, 64, P, P2, list(zip(Ws, Bs, Cs)))
    for W, B2, C in zip(Ws, Bs, Cs):
        one = torch.empty_like(C)
        _skinny(M, K, 64, P, P2, [(W, B2, one)])
        assert torch.equal(C, one)                                   # a job's result does not depend on its neighbours
        assert rel(C, P.double() @ W.double().t() + P2.double() @ B2.double().t()) < 4e-3
    Wg, Wu, Bg, Bu = _bf(N, K, gen=gen, scale=1.0 / K ** 0.5), _bf(N, K, gen=gen, scale=1.0 / K ** 0.5), Bs[2], _bf(N, 64, gen=gen, scale=0.3)
    act = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    _skinny(M, K, 64, P, P2, [(Wg, Bg, act), (Wu, Bu, None)], swiglu=1)
    gate, up = torch.empty_like(act), torch.empty_like(act)
    _skinny(M, K, 64, P, P2, [(Wg, Bg, gate), (Wu, Bu, up)])
    want = torch.empty_like(act)
    _call("msr3d_swiglu_fwd", act.numel(), _p(gate), _p(up), _p(want), _st())
    torch.cuda.synchronize()
    assert torch.equal(act, want)                                    # the same roundings as the two-launch path
    gd = P.double() @ Wg.double().t() + P2.double() @ Bg.double().t()
    ud = P.double() @ Wu.double().t() + P2.double() @ Bu.double().t()
    assert rel(act, torch.nn.functional.silu(gd) * ud) < 2 * 4e-3    # (a product of two bf16-rounded factors)


# ------------------------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("V,k", [(1024, 1), (1024, 10), (32000, 10), (32000, 1)])
def test_decode_select_values_and_exact_indices(order, V, k):
    from msr3d_amd.llm.generate import torch_select
    gen = torch.Generator(device="cuda").manual_seed(V + k + order)
    N = 5
    if V <= 1024:
        # 1024 pairwise distinct bf16 values: 4 binades x 128 mantissas x 2 signs
        mags = torch.cat([(1.0 + torch.arange(128, device="cuda") / 128.0) * s for s in (0.5, 1.0, 2.0, 4.0)])
        vals = torch.cat([mags, -mags])[:V]
        lg = torch.stack([vals[torch.randperm(V, generator=gen, device="cuda")] for _ in range(N)]).to(torch.bfloat16)
        assert all(len(torch.unique(r.float())) == V for r in lg)
    else:
        lg = (torch.randn(N, V, generator=gen, device="cuda") * 3.0).to(torch.bfloat16)
    n_prev = 6
    prev = torch.randint(0, V, (N, n_prev), generator=gen, device="cuda")
    prev[:, 1] = prev[:, 0]                                          # a token generated twice is penalised once
    top = lg.float().argmax(-1)
    prev[0, 2] = top[0]                                              # the leader itself is penalised in row 0
    eos = int(top[1])                                                # ... and row 1's leader is the masked eos
    lg[3, 77] = lg[3, int(top[3])]                                   # a planted tie with the leader: the lower id wins
    lg[3, 5] = lg[3, int(top[3])]
    bs = torch.tensor([0.0, -1.5, -0.25, -3.0, -20.0], device="cuda")
    val = torch.empty((N, k), dtype=torch.float32, device="cuda")
    tok = torch.empty((N, k), dtype=torch.int32, device="cuda")
    npv = torch.full((N,), n_prev, dtype=torch.int32, device="cuda")
    _call("msr3d_decode_select", N, V, _p(lg), V, _p(prev), n_prev, _p(npv), ctypes.c_float(3.0), 8, eos, _p(bs), order, k,
          _p(val), _p(tok), _st())
    torch.cuda.synchronize()
    # float64 statement
    x = lg.double()

    def proc(s):
        g = torch.gather(s, 1, prev)
        s = s.scatter(1, prev, torch.where(g < 0, g * 3.0, g / 3.0))
        s[:, eos] = -math.inf
        return s
    s = torch.log_softmax(proc(x), -1) if order == 0 else proc(torch.log_softmax(x, -1))
    s = s + bs.double()[:, None]
    # ties to the lower token id: a stable descending sort keeps equal values in index order
    srt = torch.sort(s, dim=1, descending=True, stable=True)
    want_tok, want_val = srt.indices[:, :k], srt.values[:, :k]
    assert torch.equal(tok.long(), want_tok), (tok, want_tok)
    assert torch.allclose(val.double(), want_val, rtol=1e-5, atol=1e-4)
    # and the library's own torch statement of it (what search falls back to on engines without a kernel) agrees
    tv, tt = torch_select(lg, prev, 3.0, 8, eos, bs, order, k)
    if V <= 1024:                                                    # (rows without a tie: torch.topk does not order ties)
        assert torch.equal(tt[:3], tok[:3].long())
    assert torch.allclose(tv, val, rtol=1e-5, atol=1e-4)


def test_decode_select_without_processors_is_log_softmax_top_k():
    gen = torch.Generator(device="cuda").manual_seed(3)
    N, V, k = 20, 32000, 10
    lg = (torch.randn(N, V, generator=gen, device="cuda") * 2.0).to(torch.bfloat16)
    val = torch.empty((N, k), dtype=torch.float32, device="cuda")
    tok = torch.empty((N, k), dtype=torch.int32, device="cuda")
    _call("msr3d_decode_select", N, V, _p(lg), V, _p(None), 0, _p(None), ctypes.c_float(1.0), 0, -1, _p(None), 1, k, _p(val),
          _p(tok), _st())
    torch.cuda.synchronize()
    srt = torch.sort(torch.log_softmax(lg.double(), -1), dim=1, descending=True, stable=True)
    assert torch.equal(tok.long(), srt.indices[:, :k])
    assert torch.allclose(val.double(), srt.values[:, :k], rtol=1e-5, atol=1e-4)


# -------------------------------------------------------------------------------------------------------------- EINVAL
def test_invalid_arguments_are_refused_without_a_launch():
    L = _lib()
    h = L.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    f1 = ctypes.c_float(1.0)
    job = (L.SkinnyJob * 1)(L.SkinnyJob(16, 128, 0, 0, 16, 16, 16))
    assert h.msr3d_bf16_skinny_lowrank(33, 128, 0, one, 128, null, 0, 1, job, 0, null) == -22        # M > 32
    assert h.msr3d_bf16_skinny_lowrank(4, 96, 0, one, 96, null, 0, 1, job, 0, null) == -22           # K % 128
    assert h.msr3d_bf16_skinny_lowrank(4, 128, 64, one, 128, null, 64, 1, job, 0, null) == -22       # R without P2
    assert h.msr3d_bf16_skinny_lowrank(4, 128, 0, one, 128, null, 0, 4, job, 0, null) == -22         # njobs
    assert h.msr3d_bf16_skinny_lowrank(4, 128, 0, one, 128, null, 0, 1, job, 1, null) == -22         # swiglu needs two
    assert h.msr3d_bf16_skinny_lowrank(0, 128, 0, one, 128, null, 0, 1, job, 0, null) == 0           # no rows: a no-op
    assert h.msr3d_rope_positions(1, 8, 2, 24, one, null, one, one, one, 8, null) == -22             # D % 16
    assert h.msr3d_rope_positions(1, 8, 2, 64, one, null, null, one, one, 8, null) == -22            # no positions
    assert h.msr3d_rope_kv_append(1, 2, 64, 8, one, one, one, 64, one, one, one, one, 8, one, one, null) == -22   # ld < H D
    assert h.msr3d_rope_kv_append(1, 2, 64, 8, one, one, one, 128, one, null, one, one, 8, one, one, null) == -22
    assert h.msr3d_attn_decode(1, 8, 2, 96, one, 192, one, one, one, 0, null, f1, one, 192, null, 0, null) == -22  # D
    assert h.msr3d_attn_decode(1, 8, 2, 64, one, 64, one, one, one, 0, null, f1, one, 128, null, 0, null) == -22   # ldq
    assert h.msr3d_attn_decode(1, 8, 2, 64, one, 128, one, one, one, 0, null, f1, one, 128, one, 4, null) == -22   # workspace
    assert h.msr3d_attn_decode(0, 8, 2, 64, null, 128, null, null, null, 0, null, f1, null, 128, null, 0, null) == 0
    assert h.msr3d_kv_reorder(2, 2, 8, 12, one, ctypes.c_void_p(32), one, one, null) == -22           # row_elems % 8
    assert h.msr3d_kv_reorder(2, 2, 8, 16, one, one, one, one, null) == -22                           # src == dst
    assert h.msr3d_decode_select(1, 50000, one, 50000, null, 0, null, f1, 0, 2, null, 0, 1, one, one, null) == -22  # V
    assert h.msr3d_decode_select(1, 100, one, 100, null, 0, null, f1, 0, 2, null, 2, 1, one, one, null) == -22      # order
    assert h.msr3d_decode_select(1, 100, one, 100, null, 0, null, f1, 0, 2, null, 0, 65, one, one, null) == -22     # k
    assert h.msr3d_decode_select(1, 100, one, 100, null, 0, null, ctypes.c_float(0.0), 0, 2, null, 0, 1, one, one, null) == -22
