"""msr3d_bf16_skinny_fused against the launches it replaces, bit for bit: msr3d_rmsnorm_fwd -> msr3d_bf16_skinny_lowrank[_wide]
-> msr3d_rope_kv_append (and msr3d_rmsnorm_fwd's residual sum behind a product).  No tolerance anywhere: bf16 results are
compared as int16 views, so NaN rows compare too.  Every batch has one NaN activation row (rows stay isolated) and the
cache planes start from a sentinel (untouched slots are checked)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [1, 16, 17, 32, 33, 48, 49, 64]          # every tile count, and the clamped rows above M
KS = [512, 1024, 1536]                        # one, two, three chunks a wave; V = 1, 2, 3 vectors a lane in the norm
EPS = 1e-6
TMAX, TABLE = 8, 16
EINVAL = -22
SENTINEL = 0x1234


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16).cuda()


def _acts(gen, M, K):
    x = _rand(gen, M, K)
    if M > 1:
        x[M // 2] = float("nan")
    return x


def _lib():
    from msr3d_amd import _lib
    return _lib


def _stream(dev):
    return _lib().current_stream_ptr(dev)


def _norm(x, w, delta=None):
    """msr3d_rmsnorm_fwd -> (sum_out or x, y)."""
    L = _lib()
    M, D = x.shape
    y = torch.empty_like(x)
    s = torch.empty_like(x) if delta is not None else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    L.call("msr3d_rmsnorm_fwd", M, D, L.ptr(x), L.ptr(delta), L.ptr(w), ctypes.c_float(EPS), L.ptr(s), L.ptr(y), L.ptr(rstd),
           _stream(x.device))
    return (s if delta is not None else x), y


def _jobs(Ws, outs):
    L = _lib()
    K = Ws[0].shape[1]
    jobs = (L.SkinnyJob * len(Ws))()
    for j, W in enumerate(Ws):
        o = outs[j] if j < len(outs) else None
        jobs[j] = L.SkinnyJob(W.data_ptr(), K, 0, 0, o.data_ptr() if o is not None else 0, W.shape[0], W.shape[0])
    return jobs


def _plain(h, Ws, swiglu=False):
    L = _lib()
    M, K = h.shape
    outs = [torch.empty((M, W.shape[0]), dtype=torch.bfloat16, device=h.device) for W in (Ws[:1] if swiglu else Ws)]
    entry = "msr3d_bf16_skinny_lowrank" if M <= 32 else "msr3d_bf16_skinny_lowrank_wide"
    L.call(entry, M, K, 0, L.ptr(h), K, L.ptr(None), 0, len(Ws), _jobs(Ws, outs), int(swiglu), _stream(h.device))
    return outs


def _fused_status(h, Ws, outs, swiglu=False, norm=None, res=None, rope=None, R=0, K=None, ldres=None):
    """The raw call -> status.  rope = (H, D, pos, len, cos, sin, table_rows, k_plane, v_plane, Tmax)."""
    L = _lib()
    M = h.shape[0]
    K = h.shape[1] if K is None else K
    p = L.ptr
    if rope is None:
        tail = (0, 0, p(None), p(None), p(None), p(None), 0, p(None), p(None), 0)
    else:
        tail = (rope[0], rope[1], p(rope[2]), p(rope[3]), p(rope[4]), p(rope[5]), rope[6], p(rope[7]), p(rope[8]), rope[9])
    fn = getattr(L.load(), "msr3d_bf16_skinny_fused")
    with torch.cuda.device(h.device):
        return fn(M, K, R, p(h), h.stride(0), p(None), 0, len(Ws), _jobs(Ws, outs), int(swiglu), p(norm),
                  ctypes.c_float(EPS), p(res), (res.stride(0) if ldres is None else ldres) if res is not None else 0, *tail,
                  _stream(h.device))


def _fused(h, Ws, swiglu=False, norm=None, res=None, rope=None):
    M = h.shape[0]
    n_out = 1 if (swiglu or rope is not None) else len(Ws)
    outs = [torch.empty((M, Ws[j].shape[0]), dtype=torch.bfloat16, device=h.device) for j in range(n_out)]
    assert _fused_status(h, Ws, outs, swiglu, norm, res, rope) == 0
    return outs


def _rope_inputs(M, H, D):
    from msr3d_amd.llm.decoder import rope_tables
    cos, sin = rope_tables(TABLE, D, 10000.0, "cuda")
    n = torch.arange(M)
    ln = torch.tensor([0, 3, TMAX - 1, TMAX, -1])[n % 5].to(torch.int32).cuda()          # a full cache and -1 write nothing
    pos = torch.tensor([2, -3, TABLE + 5, 0, TABLE - 1, 7])[n % 6].to(torch.int32).cuda()  # clamped to the table
    return cos, sin, pos, ln


def _planes(M, H, D):
    return [torch.full((M, TMAX, H, D), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16) for _ in range(2)]


def _append(q, k, v, H, D, pos, ln, cos, sin):
    """msr3d_rope_kv_append on copies -> (q rotated, k plane, v plane)."""
    L = _lib()
    M = q.shape[0]
    q = q.clone()
    kc, vc = _planes(M, H, D)
    L.call("msr3d_rope_kv_append", M, H, D, TMAX, L.ptr(q), L.ptr(k), L.ptr(v), H * D, L.ptr(pos), L.ptr(ln), L.ptr(cos),
           L.ptr(sin), TABLE, L.ptr(kc), L.ptr(vc), _stream(q.device))
    return q, kc, vc


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("H,D", [(8, 64), (4, 128)])
@pytest.mark.parametrize("prologue", [True, False])
def test_qkv_with_the_rotation_and_the_append(M, H, D, prologue):
    gen = torch.Generator().manual_seed(100 * M + D)
    K = 512
    x, w = _acts(gen, M, K), _rand(gen, K)
    Ws = [_rand(gen, H * D, K, scale=K ** -0.5) for _ in range(3)]
    cos, sin, pos, ln = _rope_inputs(M, H, D)
    h = _norm(x, w)[1] if prologue else x
    q, k, v = _plain(h, Ws)
    q_ref, kc_ref, vc_ref = _append(q, k, v, H, D, pos, ln, cos, sin)
    for _ in range(2):                                # (two calls: the same bits)
        kc, vc = _planes(M, H, D)
        q_f, = _fused(x, Ws, norm=w if prologue else None, rope=(H, D, pos, ln, cos, sin, TABLE, kc, vc, TMAX))
        assert _same(q_f, q_ref)
        assert _same(kc, kc_ref) and _same(vc, vc_ref)
    # the guard: rows with len outside 0 .. Tmax - 1 left their planes alone, the others wrote exactly one slot
    wrote = (_bits(kc) != SENTINEL).flatten(2).any(-1).sum(-1).cpu()
    assert torch.equal(wrote, ((ln >= 0) & (ln < TMAX)).long().cpu())


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_head_and_unrotated_qkv_under_the_prologue(M, K):
    gen = torch.Generator().manual_seed(7 * M + K)
    x, w = _acts(gen, M, K), _rand(gen, K)
    head = [_rand(gen, 1024, K, scale=K ** -0.5)]
    qkv = [_rand(gen, 512, K, scale=K ** -0.5) for _ in range(3)]      # (what an e4m3 cache's step launches)
    h = _norm(x, w)[1]
    for Ws in (head, qkv):
        ref = _plain(h, Ws)
        for _ in range(2):
            got = _fused(x, Ws, norm=w)
            assert len(got) == len(ref) and all(_same(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_gate_up_under_the_prologue_with_swiglu(M, K):
    gen = torch.Generator().manual_seed(11 * M + K)
    x, w = _acts(gen, M, K), _rand(gen, K)
    Ws = [_rand(gen, 1024, K, scale=K ** -0.5) for _ in range(2)]
    ref, = _plain(_norm(x, w)[1], Ws, swiglu=True)
    got, = _fused(x, Ws, swiglu=True, norm=w)
    assert _same(got, ref)
    assert _same(_fused(x, Ws, swiglu=True, norm=w)[0], ref)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("prologue", [False, True])
def test_o_and_down_with_the_residual(M, prologue):
    gen = torch.Generator().manual_seed(13 * M + prologue)
    N, K = 512, 1024
    p, res = _acts(gen, M, K), _rand(gen, M, N)
    w_in, w_next = _rand(gen, K), _rand(gen, N)
    Ws = [_rand(gen, N, K, scale=K ** -0.5)]
    o, = _plain(_norm(p, w_in)[1] if prologue else p, Ws)
    ref = _norm(res, w_next, delta=o)[0]              # bf16(res + o): what the next norm's launch stores
    before = res.clone()
    got, = _fused(p, Ws, norm=w_in if prologue else None, res=res)
    assert _same(got, ref)
    assert _same(res, before) and got.data_ptr() != res.data_ptr()
    assert _same(_fused(p, Ws, norm=w_in if prologue else None, res=res)[0], ref)


@pytest.mark.parametrize("M", [1, 17, 33, 64])
def test_everything_off_is_the_plain_entry(M):
    gen = torch.Generator().manual_seed(M)
    K = 640                                           # (no prologue: any K % 128 == 0)
    x = _acts(gen, M, K)
    for Ws, sw in (([_rand(gen, 48, K)], False), ([_rand(gen, 512, K) for _ in range(3)], False),
                   ([_rand(gen, 1024, K) for _ in range(2)], True)):
        ref = _plain(x, Ws, sw)
        got = _fused(x, Ws, sw)
        assert all(_same(a, b) for a, b in zip(got, ref))


def test_what_the_entry_refuses():
    gen = torch.Generator().manual_seed(5)
    M, K, H, D = 5, 512, 8, 64
    x, w = _acts(gen, M, K), _rand(gen, K)
    qkv = [_rand(gen, H * D, K) for _ in range(3)]
    outs = [torch.empty((M, H * D), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    cos, sin, pos, ln = _rope_inputs(M, H, D)
    kc, vc = _planes(M, H, D)
    rope = (H, D, pos, ln, cos, sin, TABLE, kc, vc, TMAX)
    assert _fused_status(x, qkv, outs, norm=w, rope=rope) == 0
    assert _fused_status(x, qkv, outs, norm=w, rope=rope, R=32) == EINVAL             # R > 0
    # a prologue on K % 512 != 0 (the first 640 columns of wider rows)
    wide, w640 = _rand(gen, M, 1024), _rand(gen, 640)
    W640 = [_rand(gen, 512, 640)]
    assert _fused_status(wide, W640, outs[:1], K=640) == 0
    assert _fused_status(wide, W640, outs[:1], K=640, norm=w640) == EINVAL
    # D / 2 not a multiple of 16
    cos16, sin16, _, _ = _rope_inputs(M, 32, 16)
    kc16, vc16 = _planes(M, 32, 16)
    assert _fused_status(x, qkv, outs, rope=(32, 16, pos, ln, cos16, sin16, TABLE, kc16, vc16, TMAX)) == EINVAL
    # misaligned pointers: the norm weight, the residual operand, a table, a plane
    w_off = _rand(gen, K + 8)[1:K + 1]
    assert _fused_status(x, qkv, outs, norm=w_off) == EINVAL
    res_off = _rand(gen, M * 512 + 8)[1:M * 512 + 1].view(M, 512)
    assert _fused_status(x, qkv[:1], outs[:1], res=res_off) == EINVAL
    cos_off = torch.cat([cos.flatten(), cos.new_zeros(4)])[1:cos.numel() + 1].view_as(cos)
    assert _fused_status(x, qkv, outs, rope=(H, D, pos, ln, cos_off, sin, TABLE, kc, vc, TMAX)) == EINVAL
    kc_off = torch.cat([kc.flatten(), kc.new_zeros(8)])[1:kc.numel() + 1].view_as(kc)
    assert _fused_status(x, qkv, outs, rope=(H, D, pos, ln, cos, sin, TABLE, kc_off, vc, TMAX)) == EINVAL
    # the residual: one job, a fresh output, no rotation beside it
    res = _rand(gen, M, H * D)
    assert _fused_status(x, qkv, outs, res=res) == EINVAL
    assert _fused_status(x, qkv[:1], [res], res=res) == EINVAL
    assert _fused_status(x, qkv[:1], outs[:1], res=res, ldres=256) == EINVAL
    assert _fused_status(x, qkv[:1], outs[:1], res=res) == 0
    # more rows than the wide entry takes
    big = _rand(gen, 65, K)
    assert _fused_status(big, qkv[:1], [torch.empty((65, H * D), dtype=torch.bfloat16, device="cuda")], norm=w) == EINVAL
    torch.cuda.synchronize()
