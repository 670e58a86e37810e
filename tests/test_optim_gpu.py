"""GPU: the flat-buffer clip + AdamW kernels against torch.optim.AdamW + clip_grad_norm_
(the reference's optimiser stack) over several steps, with and without the LR schedule."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def make(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 64), torch.nn.LayerNorm(64), torch.nn.Linear(64, 5)).cuda()


@pytest.mark.parametrize("sched", ["constant", "warmup_cosine_instructblip"])
def test_flat_adamw_matches_torch(sched):
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    a, b = make(0), make(0)
    dp = FlatGradAllReduce(a.parameters())
    warm, total = 3, 10
    opt_a = FlatAdamW(dp, lr=1e-2, weight_decay=0.05, max_grad_norm=0.5, schedule=sched,
                      warmup_steps=warm, total_steps=total)
    opt_b = torch.optim.AdamW(b.parameters(), lr=1e-2, betas=(0.9, 0.999), weight_decay=0.05)

    def lam(step):
        if sched == "constant":
            return 1.0
        if step <= warm:
            return 1e-3 + step / warm * (1 - 1e-3)
        return 0.5 * (1 + math.cos((step - warm) / (total - warm) * math.pi))
    sch = torch.optim.lr_scheduler.LambdaLR(opt_b, lam)
    for it in range(7):
        x = torch.randn(16, 37, device="cuda", generator=torch.Generator("cuda").manual_seed(it))
        dp.zero_grad()
        (a(x).pow(2).sum() * 10).backward()
        dp.finish()
        opt_a.step()
        opt_b.zero_grad()
        (b(x).pow(2).sum() * 10).backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), 0.5)
        opt_b.step()
        sch.step()
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.allclose(pa, pb, rtol=2e-5, atol=2e-6), it
    assert int(opt_a.step_ctr.item()) == 7
    # parameters are views of the flat buffer and the module still works / saves
    assert all(p.data_ptr() >= opt_a.flat_p.data_ptr() for p in a.parameters())
    assert set(a.state_dict().keys()) == set(b.state_dict().keys())


def test_dot_is_exact_enough_and_bit_reproducible():
    from msr3d_amd import hipops
    g = torch.Generator().manual_seed(3)
    for n in (4, 1024, 960 * 4096, 1000 * 1000):
        a = torch.randn(n, generator=g).cuda()
        b = torch.randn(n, generator=g).cuda()
        want = float((a.double() * b.double()).sum())
        got = [float(hipops.dot(a, b)) for _ in range(3)]
        assert got[0] == got[1] == got[2]
        assert abs(got[0] - want) <= 1e-5 * float((a.double() * b.double()).abs().sum()) + 1e-6


@pytest.mark.parametrize("world", [2, 3, 8])
def test_grad_scale_in_the_optimiser_is_the_separate_averaging_pass_bit_for_bit(world):
    """msr3d_adamw_flat_scaled(grad_scale = 1 / world) on the all-reduced SUM == `grads *= 1 / world` followed
    by the unscaled call: same clip coefficient, same moments, same weights, for a world that is not a power
    of two as well (/root/reference/trainer/leo_trainer.py:50-52: DDP averages, then accelerate clips)."""
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    a, b = make(1), make(1)
    dpa, dpb = FlatGradAllReduce(a.parameters()), FlatGradAllReduce(b.parameters())
    oa = FlatAdamW(dpa, lr=1e-2, weight_decay=0.05, max_grad_norm=0.5)
    ob = FlatAdamW(dpb, lr=1e-2, weight_decay=0.05, max_grad_norm=0.5)
    dpa.world, dpa.scale_in_optimizer = world, True
    for it in range(4):
        x = torch.randn(16, 37, device="cuda", generator=torch.Generator("cuda").manual_seed(it))
        for m, dp in ((a, dpa), (b, dpb)):
            dp.zero_grad()
            (m(x).pow(2).sum() * 10 * world).backward()       # "the sum over ranks"
        dpb.flat.mul_(1.0 / world)
        oa.step(zero_grad=True)
        ob.step()
        assert torch.equal(oa.flat_p, ob.flat_p) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq), it
        assert float(dpa.flat.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------
# The kernels at the size and in the modes the training step runs them.
#
# msr3d_adamw_flat_scaled caps its grid at 1024 blocks of 256 threads = CAP4 float4; above that every thread
# walks a grid-stride loop and adamw_kernel folds 1024 block partials.  The hand-made parameter list below
# comes to n4 = 2 * CAP4 + 624 float4 (two full trips and 2.4 blocks of a third), with sizes that are no
# multiple of 4, so that the layout has alignment gaps and a padded tail.
# ---------------------------------------------------------------------------------------------------------
CAP4 = 1024 * 256
# registration order; the flat buffers hold them reversed, so SHAPES[0] is the LAST parameter of the buffer
SHAPES = [(5, 131), (1024, 937), (3,), (607, 256), (1,), (1023, 959), (607,), (77,), (333, 7)]
RTOL, ATOL = 2e-5, 2e-6                       # the bounds of test_flat_adamw_matches_torch
MAX_NORM = 1.0
# ||g||_2 of the whole gradient at each step: on both sides of MAX_NORM, never near it
NORMS = [4.0, 0.25, 2.5, 0.5, 8.0, 0.125]
WARM, TOTAL, MULT = 6, 40, 4


def _lam(step):
    """optim/scheduler.py:17-20 of the reference (warmup_cosine_instructblip), in scheduler steps."""
    if step <= WARM:
        return 1e-3 + step / WARM * (1 - 1e-3)
    return 0.5 * (1 + math.cos((step - WARM) / (TOTAL - WARM) * math.pi))


def _params(shapes=SHAPES, seed=0):
    g = torch.Generator("cuda").manual_seed(seed)
    return [torch.nn.Parameter(0.1 * torch.randn(s, device="cuda", generator=g)) for s in shapes]


def _gap_mask(dp):
    """True where the flat buffers hold no parameter: alignment gaps and the tail padding."""
    m = torch.ones(dp.flat.numel(), dtype=torch.bool, device=dp.flat.device)
    for p in dp.order:
        m[dp.offset[id(p)]:dp.offset[id(p)] + p.numel()] = False
    return m


def _span(dp, p, flat):
    return flat[dp.offset[id(p)]:dp.offset[id(p)] + p.numel()]


def _close(got, ref, atol, what, worst):
    """assert allclose(got, ref, RTOL, atol) against the float64 `ref`; prints the worst element first and keeps the
    largest |err| / (atol + RTOL |ref|) of the run in worst[0]."""
    got, ref = got.detach().double().reshape(-1), ref.detach().reshape(-1)
    ratio = (got - ref).abs() / (atol + RTOL * ref.abs())
    i = int(ratio.argmax())
    worst[0] = max(worst[0], float(ratio[i]))
    print(f"{what}: worst |err| / bound = {float(ratio[i]):.3g} at element {i}: got {float(got[i])!r}, "
          f"want {float(ref[i])!r}")
    assert torch.allclose(got, ref, rtol=RTOL, atol=atol), what


def _run(schedule="constant", mult=1, max_norm=MAX_NORM, zero_grad=False, unused=(), mask=True, check=True,
         steps=len(NORMS)):
    """`steps` updates of FlatAdamW over SHAPES against float64 torch.optim.AdamW + clip_grad_norm_ + LambdaLR,
    compared after every step.  `unused`: indices into SHAPES of parameters that receive no gradient (their
    gradient views keep the buffer's zeros; .grad is None on the torch side); `mask`: tell FlatAdamW so."""
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    ps = _params()
    dp = FlatGradAllReduce(ps)
    n4 = dp.flat.numel() // 4
    assert 2 * CAP4 < n4 < 3 * CAP4 and (n4 - 2 * CAP4) % 256 and n4 - 2 * CAP4 > 256    # the capped grid, ragged
    init = [p.detach().clone() for p in ps]
    opt = FlatAdamW(dp, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_grad_norm=max_norm,
                    schedule=schedule, warmup_steps=WARM, total_steps=TOTAL, sched_steps_per_update=mult)
    if unused and mask:
        opt.set_unused([ps[i] for i in unused])
    refs = [q.double().requires_grad_() for q in init]
    ropt = torch.optim.AdamW(refs, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    sch = torch.optim.lr_scheduler.LambdaLR(ropt, _lam if schedule != "constant" else (lambda s: 1.0))
    gaps = _gap_mask(dp)
    assert bool(gaps[-1]) and int(gaps[:dp.numel].sum()) > 0          # a padded tail AND inner gaps
    n_live = sum(p.numel() for i, p in enumerate(ps) if i not in unused)
    gen = torch.Generator("cuda").manual_seed(1234)
    clipped, worst = [], [0.0]
    for it in range(steps):
        for i, (p, r) in enumerate(zip(ps, refs)):
            if i in unused:
                r.grad = None
                continue
            p.grad.copy_(torch.randn(p.shape, device="cuda", generator=gen) * (NORMS[it] / math.sqrt(n_live)))
            r.grad = p.grad.double()
        if max_norm:
            clipped.append(float(torch.nn.utils.clip_grad_norm_(refs, max_norm)) > max_norm)
        opt.step(zero_grad=zero_grad)
        ropt.step()
        for _ in range(mult):
            sch.step()
        assert int(opt.step_ctr.item()) == it + 1
        for buf in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq):
            assert not bool(buf[gaps].any()), "a gap or the tail padding was written"
        if zero_grad:
            assert not bool(dp.flat.any()), "zero_grad left a gradient behind"
        if not check:
            continue
        for i, (p, r) in enumerate(zip(ps, refs)):
            if i in unused:
                continue
            st = ropt.state[r]
            _close(p, r, ATOL, f"step {it + 1} param {SHAPES[i]}", worst)
            # the moments are O(g) and O(g^2), not O(1): the same bounds relative to their largest element
            _close(_span(dp, p, opt.exp_avg), st["exp_avg"], ATOL * float(st["exp_avg"].abs().max()),
                   f"step {it + 1} exp_avg {SHAPES[i]}", worst)
            _close(_span(dp, p, opt.exp_avg_sq), st["exp_avg_sq"], ATOL * float(st["exp_avg_sq"].abs().max()),
                   f"step {it + 1} exp_avg_sq {SHAPES[i]}", worst)
    if max_norm and check:
        assert any(clipped) and not all(clipped), clipped          # both branches of the coefficient ran
    print(f"worst |err| / bound of the run: {worst[0]:.3g}")
    return {"ps": ps, "dp": dp, "opt": opt, "init": init, "flat_p": opt.flat_p.clone(),
            "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone()}


_runs = {}


def _run_a():
    if "a" not in _runs:
        _runs["a"] = _run()
    return _runs["a"]


def test_capped_grid_constant_schedule_with_clip():
    """(a) 2.1 M parameters, 6 steps, clip on 3 of them.  The largest |err| / (atol + rtol |ref|) to expect is 0.58,
    on exp_avg_sq: the kernel's 1 - beta2 is 1.0f - 0.999f, 1.3e-5 (relative) off 0.001, against rtol 2e-5; an fp32
    replay of the kernel's arithmetic on the host gives 0.58 there, 0.03 on exp_avg and 0.02 on the parameters.
    Each run prints its own worst figure (pytest -s); none has been recorded from an MI355X yet."""
    _run_a()


def test_capped_grid_scheduler_steps_per_update():
    """(b) the N-GPU learning-rate curve: 4 scheduler steps per update, warm-up of 6 scheduler steps, so update 3
    is past the warm-up and on the cosine."""
    _run(schedule="warmup_cosine_instructblip", mult=MULT)


def test_capped_grid_without_clip_ticks_from_the_tick_kernel():
    """(c) max_grad_norm None: no sumsq_kernel, the counter is advanced after adamw_kernel."""
    _run(max_norm=None)


def test_capped_grid_zero_grad_clears_the_buffer_and_changes_nothing_else():
    """(d) zero_grad=True: the gradient buffer is exactly 0 after every step (asserted in _run) and parameters and
    moments carry the bits of (a)."""
    a, d = _run_a(), _run(zero_grad=True)
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], d[k]), k


def test_capped_grid_repeat_run_is_bit_identical():
    """The same 6 steps from the same state give the same bits: the fixed-order sum of the 1024 block partials
    that data-parallel ranks rely on."""
    a, again = _run_a(), _run(check=False)
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], again[k]), k


def test_clip_norm_partials_are_exact_on_integer_gradients():
    """Gradients from {-1, 0, 1}: sum g^2 <= n < 2^24, so every partial sum is exact in fp32 in any order and the
    1024 partials must add up to the number of non-zeros exactly; block b's own partial must be the count over
    the float4 b * 256 + tid + k * CAP4 it owns."""
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    dp = FlatGradAllReduce(_params())
    opt = FlatAdamW(dp, lr=1e-2, weight_decay=0.05, max_grad_norm=MAX_NORM)
    n = dp.flat.numel()
    assert n < 2 ** 24
    g = torch.randint(-1, 2, (n,), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    dp.flat.copy_(g)
    nz4 = torch.zeros(3 * CAP4, dtype=torch.int64, device="cuda")
    nz4[:n // 4] = (g != 0).view(-1, 4).sum(1)
    per_block = nz4.view(3, 1024, 256).sum((0, 2))
    opt.step()
    got = opt.sumsq[:1024].double()
    assert float(got.sum()) == int((g != 0).sum())
    assert torch.equal(got, per_block.double())


UNUSED = (1, 6, 0)      # (1024, 937): large; (607,): odd, a gap behind it; (5, 131): the last one of the buffer


@pytest.mark.parametrize("zero_grad", [False, True])
def test_unused_parameters_are_left_alone_under_weight_decay(zero_grad):
    """weight_decay 0.05, three parameters without a gradient: the used ones follow float64 AdamW (which skips a
    parameter whose .grad is None), the unused ones and their moments keep their initial bits."""
    r = _run(unused=UNUSED, zero_grad=zero_grad)
    dp, opt = r["dp"], r["opt"]
    assert opt.active is not None
    for i in UNUSED:
        p = r["ps"][i]
        assert torch.equal(p.detach(), r["init"][i]), SHAPES[i]
        assert not bool(_span(dp, p, opt.exp_avg).any()) and not bool(_span(dp, p, opt.exp_avg_sq).any())


def test_unused_parameters_decay_when_the_mask_is_not_set():
    """The control of the test above: the same run without set_unused moves every unused weight (decay alone), so
    the bit-equality there can fail."""
    r = _run(unused=UNUSED, mask=False, check=False, steps=2)
    for i in UNUSED:
        now, init = r["ps"][i].detach(), r["init"][i]
        assert bool((now != init)[init != 0].all()), SHAPES[i]


def _pair(k):
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    a, b = _params([(k,), (k,)], seed=2)
    dp = FlatGradAllReduce([a, b], pack_groups=[[a, b]])
    assert dp.offset[id(a)] == 0 and dp.offset[id(b)] == k
    return a, b, dp, FlatAdamW(dp, lr=1e-2, weight_decay=0.05, max_grad_norm=MAX_NORM)


def test_set_unused_refuses_a_float4_shared_with_a_used_pack_group_member():
    """Members of a pack group sit back to back: with 6 + 6 elements the float4 at 4..7 holds a[4:6] and b[0:2], and
    the per-float4 mask cannot freeze one without the other."""
    a, b, dp, opt = _pair(6)
    with pytest.raises(ValueError, match=r"^set_unused: dp\.order\[1\] "):
        opt.set_unused([b])
    with pytest.raises(ValueError, match=r"^set_unused: dp\.order\[0\] "):
        opt.set_unused([a])
    with pytest.raises(ValueError, match=r"^set_unused: attn\.k\.weight "):
        opt.set_unused([b], names=["attn.q.weight", "attn.k.weight"])
    with pytest.raises(ValueError, match=r"^set_unused: attn\.q\.weight "):
        opt.set_unused([a], names=["attn.q.weight", "attn.k.weight"])
    opt.set_unused([a, b])                       # the neighbour is unused as well: fine
    assert opt.active is not None and opt.active[:3].tolist() == [0, 0, 0] and bool(opt.active[3:].all())
    # a gap or the tail padding in the boundary float4 is fine too
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    c, d = _params([(6,), (5,)], seed=3)
    opt2 = FlatAdamW(FlatGradAllReduce([c, d]), lr=1e-2)
    opt2.set_unused([c])
    opt2.set_unused([d])


def test_set_unused_on_an_aligned_pack_group_freezes_exactly_the_unused_member():
    a, b, dp, opt = _pair(8)
    opt.set_unused([b])
    a0, b0 = a.detach().clone(), b.detach().clone()
    dp.flat[:16].copy_(torch.arange(1, 17, device="cuda") * 0.01)
    opt.step()
    assert bool((a.detach() != a0).all())
    assert torch.equal(b.detach(), b0)
    assert not bool(opt.exp_avg[8:16].any()) and not bool(opt.exp_avg_sq[8:16].any())
    assert bool((opt.exp_avg[:8] != 0).all())


# n -> what it exercises: 1 block; 3 blocks; 256 blocks with a ragged last float4 row; n4 = 4 * CAP4 + CAP4 + 77:
# a second trip of the 4-deep loop whose tail is partly out of range
DOT_SIZES = [4, 12288, 1048576 + 4, 5243188]


def _ternary(n, seed):
    g = torch.Generator("cuda").manual_seed(seed)
    return (torch.randint(-1, 2, (n,), device="cuda", generator=g).float(),
            torch.randint(-1, 2, (n,), device="cuda", generator=g).float())


@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_is_exact_on_ternary_inputs(n):
    """Inputs from {-1, 0, 1}: sum |a b| <= n < 2^24, so the fp32 sum is the integer dot product in ANY order."""
    from msr3d_amd import hipops
    a, b = _ternary(n, n)
    prod = a.long() * b.long()
    assert int(prod.abs().sum()) < 2 ** 24
    assert float(hipops.dot(a, b)) == int(prod.sum())


def test_dot_stays_exact_over_200_queued_launches_of_changing_grids():
    """200 launches on one stream, no host synchronisation in between, block counts 1 -> 3 -> 256 -> 256 on the
    same scratch, every launch on a different slice: a partial left over from the launch before, one not yet
    visible to the last block, or a ticket left non-zero gives a wrong integer."""
    from msr3d_amd import hipops
    launches, shift = 200, 4 * 37                      # slices start 16-byte aligned
    A, B = _ternary(max(DOT_SIZES) + launches * shift, 9)
    assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
    prod = A.long() * B.long()
    assert int(prod.abs().sum()) < 2 ** 24
    cs = torch.cat([prod.new_zeros(1), prod.cumsum(0)])
    plan = [(i * shift, DOT_SIZES[i % 4]) for i in range(launches)]
    want = torch.stack([cs[o + n] - cs[o] for o, n in plan]).cpu()
    assert float((want[1:] != want[:-1]).float().mean()) > 0.9       # consecutive results differ
    hipops.dot(A[:4], B[:4])                           # (the scratch row of this stream exists from here on)
    torch.cuda.synchronize()
    outs = [hipops.dot(A[o:o + n], B[o:o + n]) for o, n in plan]
    got = torch.stack(outs).cpu()                      # the one synchronisation
    torch.cuda.synchronize()
    bad = (got.double() != want.double()).nonzero().flatten().tolist()
    assert not bad, [(i, plan[i][1], float(got[i]), int(want[i])) for i in bad[:8]]
    dev = A.device
    ws = hipops._dot_scratch[(dev, torch.cuda.current_stream(dev).cuda_stream)]
    assert int(ws[1024:1025].view(torch.int32).item()) == 0


def test_graph_replay_advances_the_schedule_from_the_device_counter():
    """opt.step() captured once and replayed == opt.step() called eagerly, bit for bit, over 5 steps on which the
    learning rate (warm-up, then cosine) and the bias corrections change every time: nothing of the step index
    is baked in at capture."""
    from msr3d_amd.dp import FlatGradAllReduce
    from msr3d_amd.optim import FlatAdamW
    shapes = [(607, 33), (3,), (129,)]
    twins = []
    for _ in range(2):
        dp = FlatGradAllReduce(_params(shapes, seed=4))
        twins.append((dp, FlatAdamW(dp, lr=1e-2, weight_decay=0.05, max_grad_norm=MAX_NORM,
                                    schedule="warmup_cosine_instructblip", warmup_steps=3, total_steps=20)))
    (dpa, oa), (dpb, ob) = twins
    gen = torch.Generator("cuda").manual_seed(6)
    grads = [torch.randn(dpa.numel, device="cuda", generator=gen) * s for s in (0.1, 0.001, 0.1, 0.01, 1.0, 0.001)]
    for dp, o in twins:
        dp.flat[:dp.numel].copy_(grads[0])
        o.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    for it, g in enumerate(grads[1:]):
        dpa.flat[:dpa.numel].copy_(g)
        dpb.flat[:dpb.numel].copy_(g)
        graph.replay()
        ob.step()
        for k in ("flat_p", "exp_avg", "exp_avg_sq", "step_ctr"):
            assert torch.equal(getattr(oa, k), getattr(ob, k)), (it, k)
        assert int(oa.step_ctr.item()) == it + 2


def test_invalid_optimiser_and_dot_arguments_are_refused_without_a_launch():
    import ctypes

    from msr3d_amd import _lib
    h = _lib.load()
    null = ctypes.c_void_p(0)
    bufs = [torch.zeros(1024 + 8, device="cuda") for _ in range(5)]
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda t, byte=0: ctypes.c_void_p(t.data_ptr() + byte)
    six = [ptr(t) for t in bufs[:5]] + [ptr(ctr)]       # params, grads, exp_avg, exp_avg_sq, scratch, step counter

    def adamw(n, six=six, sched=0, warm=400, total=1):
        return h.msr3d_adamw_flat_scaled(n, *six, 1e-2, 0.9, 0.999, 1e-8, 0.05, 1.0, sched, warm, total, 0, null,
                                         1.0, null)
    assert adamw(6) == -22                               # n % 4
    assert adamw(-4) == -22
    for i in range(6):
        assert adamw(8, six[:i] + [null] + six[i + 1:]) == -22, i
    assert adamw(8, sched=1, warm=10, total=10) == -22   # total_steps <= warmup_steps
    assert adamw(8, sched=1, warm=10, total=5) == -22
    assert adamw(8, sched=1, warm=0, total=10) == -22    # warmup_steps < 1
    assert adamw(8, sched=1 | (4 << 8), warm=0, total=10) == -22
    assert adamw(0) == 0
    assert adamw(0, [null] * 6) == 0
    a, b, ws, out = bufs[0], bufs[1], bufs[4], bufs[2]
    assert h.msr3d_dot_f32(6, ptr(a), ptr(b), ptr(ws), ptr(out), null) == -22           # n % 4
    assert h.msr3d_dot_f32(-4, ptr(a), ptr(b), ptr(ws), ptr(out), null) == -22
    assert h.msr3d_dot_f32(8, ptr(a, 4), ptr(b), ptr(ws), ptr(out), null) == -22        # not 16-byte aligned
    assert h.msr3d_dot_f32(8, ptr(a), ptr(b, 8), ptr(ws), ptr(out), null) == -22
    assert h.msr3d_dot_f32(8, ptr(a), ptr(b), null, ptr(out), null) == -22              # no scratch
    assert h.msr3d_dot_f32(8, ptr(a), ptr(b), ptr(ws), null, null) == -22               # no out
    torch.cuda.synchronize()
    assert int(ctr.item()) == 0 and not any(bool(t.any()) for t in bufs)                # nothing ran
