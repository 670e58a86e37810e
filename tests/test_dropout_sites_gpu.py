"""Every kernel entry that draws a dropout mask, alone, against float64 with the mask STATED ON THE HOST
(tests/dropout_ref.py): which elements are dropped, the 1 / (1 - p) scale, forward and backward.

  a. msr3d_dropout_add_ln_fwd / _bwd          (rowops.hip, one tail)
  b. msr3d_dropout_add_ln2_fwd / _bwd         (rowops.hip, two chained tails, two salts, two probabilities)
  c. msr3d_gemm_f32's GELU + dropout epilogue and msr3d_gelu_bwd_f32, as fused_layer.py calls them
  d. the pattern comparison can fail: two deliberately wrong host variants do not match the kernel

Every case runs on the seed word 12345 (high half zero) and on that word bumped twice by msr3d_bump_seed
(0x43f04a6ece53d613: the `+ (unsigned)(seed >> 32)` term of keep_elem), which also checks the bump.

Tolerances.  The pre-norm sum s = a * scale * keep + r is two roundings (product, sum) or one (fma) of exact
inputs: 4 fp32 ulp of |a| * scale + |r|.  y 1e-5, da / dr / dgamma / dbeta 2e-5 rel-L2 and the elementwise
rtol = atol = 1e-5 of the GELU sites are tests/test_rowops_gpu.py's; the product 2e-5 is tests/test_gemm_gpu.py's."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import dropout_ref as R

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(params=["seed_12345", "seed_bumped_twice"])
def seed(request):
    """Sets the device's seed word; yields it as 64 unsigned bits; restores the word and the salt counter."""
    from msr3d_amd import hipops
    dev = torch.device("cuda", torch.cuda.current_device())
    w = hipops.seed_word(dev)
    saved, saved_salt = w.clone(), hipops._salt_counter[0]
    w.fill_(12345)
    want = 12345
    if request.param == "seed_bumped_twice":
        hipops.bump_seed(dev)
        hipops.bump_seed(dev)
        want = R.bump(R.bump(12345))
        assert R.u64(w.item()) == want and want >> 32 != 0
    yield want
    w.copy_(saved)
    hipops._salt_counter[0] = saved_salt


def host_mask(seed, salt, rows, cols, p, **variant):
    return torch.from_numpy(R.keep_mask(seed, salt, rows, cols, cols, p, **variant)).cuda()


def ulp(m):
    m = m.float()
    return (torch.nextafter(m, torch.full_like(m, float("inf"))) - m).double().clamp_min(2.0 ** -149)


def check_sum(s, a, r, keep, p):
    """s == a * scale * keep + r: bit-equal to the residual (0 without one) where dropped, 4 ulp elsewhere."""
    sc = float(R.scale(p))
    r64 = r.double() if r is not None else torch.zeros_like(a, dtype=torch.float64)
    assert torch.equal(s[~keep], r64.float()[~keep])
    want = a.double() * sc * keep + r64
    bound = 4 * ulp(a.double().abs() * sc + r64.abs())
    assert bool(((s.double() - want).abs() <= bound).all()), float(((s.double() - want).abs() / bound).max())
    return want


def make_ln(D):
    ln = torch.nn.LayerNorm(D).cuda()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_()
    ln.weight.grad, ln.bias.grad = torch.zeros_like(ln.weight), torch.zeros_like(ln.bias)
    return ln


def ln64(v, ln, leaves=None):
    g, b = ln.weight.detach().double().requires_grad_(), ln.bias.detach().double().requires_grad_()
    if leaves is not None:
        leaves += [g, b]
    return F.layer_norm(v, (v.shape[-1],), g, b, ln.eps)


@pytest.mark.parametrize("with_r", [True, False])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M", [7, 203])
@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_single_tail_against_float64_with_the_host_mask(seed, D, M, p, with_r):
    from msr3d_amd import fused_layer as fl
    torch.manual_seed(D + M)
    salt = 40 + D // 256
    ln = make_ln(D)
    keep = host_mask(seed, salt, M, D, p)
    # the pattern and the scale, bit for bit: dropout of ones, no residual
    ones = torch.ones(M, D, device="cuda")
    _, s, _ = fl._dal_fwd(ones, None, ln, p, salt)
    assert torch.equal(s, keep.float() * float(R.scale(p)))
    assert 0 < int((~keep).sum()) < keep.numel()
    # values
    a = torch.randn(M, D, device="cuda")
    r = torch.randn(M, D, device="cuda") if with_r else None
    dy = torch.randn(M, D, device="cuda")
    y, s, st = fl._dal_fwd(a, r, ln, p, salt)
    check_sum(s, a, r, keep, p)
    da = torch.full_like(a, float("nan"))
    dr = torch.full_like(a, float("nan")) if with_r else None
    fl._dal_bwd(dy, s, st, ln, p, salt, da, dr, False)
    torch.cuda.synchronize()
    a64 = a.double().requires_grad_()
    r64 = r.double().requires_grad_() if with_r else None
    leaves = []
    v = a64 * float(R.scale(p)) * keep
    y64 = ln64(v + r64 if with_r else v, ln, leaves)
    y64.backward(dy.double())
    assert rel(y, y64) < 1e-5
    assert bool((da[~keep] == 0).all())                       # exactly zero where dropped
    assert rel(da, a64.grad) < 2e-5
    if with_r:                                                # the residual's gradient is not masked
        assert rel(dr, r64.grad) < 2e-5 and rel(dr[~keep], r64.grad[~keep]) < 2e-5
    assert rel(ln.weight.grad, leaves[0].grad) < 2e-5 and rel(ln.bias.grad, leaves[1].grad) < 2e-5


@pytest.mark.parametrize("D", [256, 512])
def test_double_tail_against_float64_with_two_host_masks(seed, D):
    """t = LN2(drop2(LN1(drop1(a) + r)) + r) with p1 = 0.1 / salt 11 and p2 = 0.3 / salt 12: swapped salts or
    swapped probabilities state other masks.  The second tail's dropout input LN1(s1) is not an output of the
    double kernel; the single-tail kernel's y on the same inputs is (tests/test_rowops_gpu.py holds the two
    bit-identical), so s2 is checked to 4 ulp like s1."""
    from msr3d_amd import fused_layer as fl
    torch.manual_seed(D)
    M, p1, p2, salt1, salt2 = 203, 0.1, 0.3, 11, 12
    ln1, ln2 = make_ln(D), make_ln(D)
    a, r, dy = (torch.randn(M, D, device="cuda") for _ in range(3))
    k1, k2 = host_mask(seed, salt1, M, D, p1), host_mask(seed, salt2, M, D, p2)
    assert bool((k1 != k2).any()) and abs(float((~k2).double().mean()) - 0.3) < 0.02
    t, s1, st1, s2, st2 = fl._dal2_fwd(a, r, ln1, p1, salt1, ln2, p2, salt2)
    y1, s1_single, _ = fl._dal_fwd(a, r, ln1, p1, salt1)
    assert torch.equal(s1, s1_single)
    check_sum(s1, a, r, k1, p1)
    check_sum(s2, y1, r, k2, p2)
    da, dr = torch.full_like(a, float("nan")), torch.full_like(a, float("nan"))
    fl._dal2_bwd(dy, s1, st1, ln1, p1, salt1, s2, st2, ln2, p2, salt2, da, dr)
    torch.cuda.synchronize()
    a64, r64 = a.double().requires_grad_(), r.double().requires_grad_()
    leaves = []
    v1 = a64 * float(R.scale(p1)) * k1 + r64
    v2 = ln64(v1, ln1, leaves) * float(R.scale(p2)) * k2 + r64
    t64 = ln64(v2, ln2, leaves)
    t64.backward(dy.double())
    assert rel(s1, v1) < 1e-6 and rel(s2, v2) < 1e-5 and rel(t, t64) < 1e-5
    assert bool((da[~k1] == 0).all())
    assert rel(da, a64.grad) < 2e-5 and rel(dr, r64.grad) < 2e-5
    for got, want in zip((ln1.weight.grad, ln1.bias.grad, ln2.weight.grad, ln2.bias.grad), leaves):
        assert rel(got, want.grad) < 2e-5


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("M,N,K", [(203, 2048, 256), (61, 192, 256)])
def test_gelu_dropout_epilogue_and_its_backward(seed, M, N, K, p):
    """linear1 as fused_layer.py runs it: h = drop(gelu(t W^T + b)) in msr3d_gemm_f32's epilogue, index
    row * N + col; then msr3d_gelu_bwd_f32 regenerates the mask from the flat index."""
    from msr3d_amd import hipops
    torch.manual_seed(N)
    salt = 91
    t = torch.randn(M, K, device="cuda")
    W, b = torch.randn(N, K, device="cuda") / 16, torch.randn(N, device="cuda")
    h = torch.full((M, N), float("nan"), device="cuda")
    pre = torch.full((M, N), float("nan"), device="cuda")
    hipops._gemm(True, True, M, N, K, t, K, W, K, h, N, bias=b, c_pre=pre, flags=1, p_drop=p, salt=salt)
    d_h = torch.randn(M, N, device="cuda")
    d_pre = hipops._gelu_bwd(d_h, pre, p, salt)
    torch.cuda.synchronize()
    keep = host_mask(seed, salt, M, N, p)
    sc = float(R.scale(p))
    assert rel(pre, t.double() @ W.double().T + b.double()) < 2e-5
    assert bool((h[~keep] == 0).all())
    want = F.gelu(pre.double()) * sc
    assert torch.allclose(h.double()[keep], want[keep], rtol=1e-5, atol=1e-5)
    # (a kept element is zero only where gelu underflows: the kept pattern is the host's wherever gelu is visible)
    assert torch.equal((h != 0) | (want.abs() < 1e-4), keep | (want.abs() < 1e-4))
    assert bool((d_pre[~keep] == 0).all())
    want_d = d_h.double() * keep * sc * gelu_grad64(pre.double())
    assert torch.allclose(d_pre.double(), want_d, rtol=1e-5, atol=1e-5)


def test_the_pattern_comparison_can_fail(seed):
    """The kernel's pattern equals the host statement and NOT its two wrong variants (16-bit halves swapped;
    one hash per element instead of one per pair)."""
    from msr3d_amd import fused_layer as fl
    M, D, p, salt = 203, 256, 0.1, 41
    ln = make_ln(D)
    _, s, _ = fl._dal_fwd(torch.ones(M, D, device="cuda"), None, ln, p, salt)
    got = s > 0
    assert torch.equal(got, host_mask(seed, salt, M, D, p))
    for variant in ({"swap_halves": True}, {"per_element": True}):
        wrong = host_mask(seed, salt, M, D, p, **variant)
        assert abs(float((~wrong).double().mean()) - p) < 0.01       # a plausible mask, only another one
        assert float((wrong != got).double().mean()) > 0.1, variant
