"""The reference's own pointnet2 kernels, compiled for gfx950 (oracle/pn2_ref.py -> oracle/_ref/libpn2_ref.so), against
the CPU restatement every bit-exact claim of this project hangs on (oracle/pn2_oracle.c), and against the shipped kernels.

  a. which floating-point contraction the build has: exactly one oracle contract reproduces every bit of the squared
     distances three_nn returns, and it is the one recorded in pn2_ref.CONTRACT;
  b. the oracle AT THAT CONTRACT == the build, bit for bit, for all nine ops (gradients on inputs whose partial sums
     are exact, so the order of the reference's atomicAdd cannot matter; one random-float case each within the bound of
     a reordered float sum);
  c. the shipped kernels (contract 0) == the build on index outputs, on inputs where the oracle says the two contracts
     decide alike -- checked here on the CPU side, with no input excluded -- and three_nn's distances within the
     measured number of units in the last place.

Only oracle/_ref/ is read; the reference's sources are not needed (and not present) where this runs."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from oracle import pn2, pn2_ref

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pn2_ref.available(),
                                 reason="oracle/_ref/libpn2_ref.so is absent: __graft_entry__.build() compiles it where "
                                        "the reference's sources and hipcc are present (oracle/pn2_ref.py::build)")]


@contextlib.contextmanager
def oracle_contract(c):
    pn2.set_contract(c)
    try:
        assert pn2.get_contract() == c
        yield
    finally:
        pn2.set_contract(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def take_rows(xyz, idx):
    return np.take_along_axis(xyz, idx[..., None].astype(np.int64).repeat(3, -1), 1)


# ---------------------------------------------------------------------------------------------- clouds
def unit_ball_cloud(rng, b, n, dup_frac=0.0):
    """tests/test_pn2_ops_gpu.py: centred, max-norm 1, optionally sampled with replacement (exact distance ties)."""
    out = np.empty((b, n, 3), np.float32)
    for i in range(b):
        size = rng.uniform(0.1, 2.0, 3)
        n_raw = n if dup_frac == 0 else min(n, max(8, int(n * (1 - dup_frac))))
        raw = rng.uniform(-0.5, 0.5, (n_raw, 3)) * size
        pts = raw[rng.integers(0, n_raw, n)] if n_raw < n else raw
        pts = pts - pts.mean(0)
        pts = pts / max(np.max(np.linalg.norm(pts, axis=1)), 1e-12)
        out[i] = pts.astype(np.float32)
    return out


def on_sphere(rng, b, n, r2):
    """Points whose exact |p|^2 lies within about two units in the last place of r2: whether the float sum lands above
    or below a threshold at r2 is decided by the rounding of the sum, i.e. by the contraction."""
    d = rng.standard_normal((b, n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    target = r2 * (1.0 + rng.uniform(-2.0, 2.0, (b, n, 1)) * 2.0 ** -23)
    return (d * np.sqrt(target)).astype(np.float32)


def make_cloud(rng, b, n, kind):
    if kind == "ball":
        return unit_ball_cloud(rng, b, n)
    if kind == "dup":
        return unit_ball_cloud(rng, b, n, dup_frac=0.7)
    if kind == "ones":
        return np.ones((b, n, 3), np.float32)
    if kind == "tiny":                                   # mostly skipped
        return (rng.standard_normal((b, n, 3)) * 5e-3).astype(np.float32)
    if kind == "grid":                                   # lattice: massive exact ties
        return rng.integers(-3, 4, (b, n, 3)).astype(np.float32) * 0.25
    if kind == "mixed":                                  # some skipped, some dup, some far
        x = unit_ball_cloud(rng, b, n, dup_frac=0.5)
        x[:, ::3] *= 0.02
        return x
    if kind == "p0small":                                # point 0 inside the skip radius (picked first all the same)
        x = unit_ball_cloud(rng, b, n)
        x[:, 0] = (0.01, -0.02, 0.005)                   # |p|^2 = 5.25e-4 <= 1e-3
        return x
    if kind == "allskip":                                # |p|^2 <= 3e-4 everywhere: every thread reports (-1, 0)
        return rng.uniform(-0.01, 0.01, (b, n, 3)).astype(np.float32)
    if kind == "skipedge":                               # |p|^2 within ulps of the 1e-3 of sampling_gpu.cu:100
        return on_sphere(rng, b, n, 1e-3)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------- a. the contract
def test_the_build_has_exactly_the_recorded_contract():
    """16 x 256 unknowns against one known point each: dist2[..., 0] IS the squared distance of the pair."""
    rng = np.random.default_rng(20240)
    unknown = rng.standard_normal((16, 256, 3)).astype(np.float32)
    known = rng.standard_normal((16, 1, 3)).astype(np.float32)
    d2, _ = pn2_ref.three_nn(dev(unknown), dev(known))
    got = host(d2)[..., 0]
    by_contract = {}
    for c in pn2.REAL_CONTRACTS:
        with oracle_contract(c):
            by_contract[c] = pn2.three_nn(unknown, known)[0][..., 0]
    # the sample tells every pair of contracts apart
    cs = list(by_contract)
    for i, a in enumerate(cs):
        for bb in cs[i + 1:]:
            assert not same_bits(by_contract[a], by_contract[bb]), (a, bb)
    matching = [c for c in cs if same_bits(by_contract[c], got)]
    mism = {c: int((bits(by_contract[c]) != bits(got)).sum()) for c in cs}
    assert matching == [pn2_ref.CONTRACT], (
        f"the reference build's squared distance matches oracle contract(s) {matching}, recorded is "
        f"{pn2_ref.CONTRACT}; distances differing per contract of {got.size}: {mism}.  The compiler's contraction of "
        f"the reference's kernels has changed: re-read it from the device assembly and update oracle/pn2_oracle.c")


# ---------------------------------------------------------------------------------------------- b. oracle == build
FPS_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
             1000, 1024, 2048]          # both sides of every block size 1 .. 512 (2^floor(log2 n)), and n > 512
FPS_KINDS = ["ball", "dup", "ones", "tiny", "grid", "mixed", "p0small", "allskip", "skipedge"]


def fps_m(n):
    return n + 3 if n <= 17 else min(n, 24)          # more picks than points on the small ones


@pytest.mark.parametrize("kind", FPS_KINDS)
def test_fps_oracle_is_the_build(kind):
    rng = np.random.default_rng(1000 + FPS_KINDS.index(kind))
    with oracle_contract(pn2_ref.CONTRACT):
        for n in FPS_SIZES:
            xyz = make_cloud(rng, 2, n, kind)
            m = fps_m(n)
            got = host(pn2_ref.furthest_point_sampling(dev(xyz), m))
            want = pn2.furthest_point_sampling(xyz, m)
            assert got.dtype == np.int32 and np.array_equal(got, want), (kind, n, np.argwhere(got != want)[:5])
            if kind == "allskip":
                assert not got.any()


def test_fps_skip_rule_at_the_threshold():
    """A shell of points whose |p|^2 rounds to either side of 1e-3 depending on the contraction: here the double compare
    and the form of the magnitude sum (not the one of the distances) decide which points can be picked at all.  Half
    the points are picked, so the picks show who was skipped; the contracts do disagree on this input."""
    rng = np.random.default_rng(77)
    xyz = make_cloud(rng, 4, 256, "skipedge")
    xyz[:, 0] = (0.5, 0.5, 0.5)                       # a far first pick: the shell is then ranked by distance to it
    with oracle_contract(0):
        at0 = pn2.furthest_point_sampling(xyz, 128)
    with oracle_contract(pn2_ref.CONTRACT):
        want = pn2.furthest_point_sampling(xyz, 128)
    assert not np.array_equal(at0, want), "the input no longer tells the contracts apart"
    got = host(pn2_ref.furthest_point_sampling(dev(xyz), 128))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_fps_tie_rule_cases():
    # the five closed-form cases of tests/test_pn2_ops_gpu.py::test_fps_tie_rule_kat
    with oracle_contract(pn2_ref.CONTRACT):
        for n, a, bb, want in [(1024, 5, 517, 5), (1024, 3, 514, 514), (1024, 1, 2, 2), (1024, 1, 256, 256),
                               (32, 1, 2, 2)]:
            xyz = np.full((1, n, 3), 0.5, np.float32)
            xyz[0, a] = (0.5, 0.5, 0.9)
            xyz[0, bb] = (0.5, 0.5, 0.9)
            got = host(pn2_ref.furthest_point_sampling(dev(xyz), 2))
            assert got[0, 1] == want and np.array_equal(got, pn2.furthest_point_sampling(xyz, 2)), (n, a, bb)


@pytest.mark.parametrize("n,m1,m2,kind", [(1024, 7, 5, "ball"), (200, 30, 29, "dup"), (3000, 64, 40, "ball"),
                                          (64, 48, 33, "mixed"), (5000, 17, 17, "ball"), (1024, 48, 40, "ball")])
def test_fps_second_level_over_its_own_winners(n, m1, m2, kind):
    """The reference's launch again over the m1 winners: 2^floor(log2 m1) threads, so two points a thread when m1 is no
    power of two."""
    rng = np.random.default_rng(n + m1)
    xyz = make_cloud(rng, 3, n, kind)
    i1 = pn2_ref.furthest_point_sampling(dev(xyz), m1)
    nx1 = pn2_ref.gather_points(dev(xyz.transpose(0, 2, 1)), i1).transpose(1, 2).contiguous()
    i2 = pn2_ref.furthest_point_sampling(nx1, m2)
    with oracle_contract(pn2_ref.CONTRACT):
        w1 = pn2.furthest_point_sampling(xyz, m1)
        wx1 = take_rows(xyz, w1)
        w2 = pn2.furthest_point_sampling(wx1, m2)
    assert np.array_equal(host(i1), w1) and same_bits(host(nx1), wx1) and np.array_equal(host(i2), w2)


BQ_CASES = [
    # (b, n, m, radius, nsample, kind): tests/test_pn2_ops_gpu.py's, radii that catch nothing / everything, nsample 1 and
    # > 64, m no power of two
    (7, 1024, 32, 0.2, 32, "ball"), (5, 1024, 32, 0.2, 32, "dup"), (3, 1024, 32, 0.2, 32, "ones"),
    (6, 32, 16, 0.4, 32, "ball"), (2, 2048, 64, 0.2, 64, "ball"), (2, 1000, 7, 0.05, 5, "ball"),
    (2, 100, 9, 10.0, 16, "ball"), (2, 100, 9, 1e-4, 16, "ball"), (1, 5000, 130, 0.3, 48, "grid"),
    (3, 70, 3, 0.4, 1, "ball"), (1, 9000, 16, 0.1, 100, "ball"), (2, 300, 33, 0.25, 65, "mixed"),
]


@pytest.mark.parametrize("b,n,m,r,ns,kind", BQ_CASES)
def test_ball_query_oracle_is_the_build(b, n, m, r, ns, kind):
    rng = np.random.default_rng(b * 1000003 + n * 101 + m * 7 + ns)
    xyz = make_cloud(rng, b, n, kind)
    cidx = rng.integers(0, n, (b, m))
    new_xyz = np.take_along_axis(xyz, cidx[..., None].repeat(3, -1), 1).copy()
    if kind == "ball":
        new_xyz[:, -1] += 100.0                       # a centre with no neighbour at all -> zero row
    got = host(pn2_ref.ball_query(dev(new_xyz), dev(xyz), r, ns))
    with oracle_contract(pn2_ref.CONTRACT):
        want = pn2.ball_query(new_xyz, xyz, r, ns)
    assert np.array_equal(got, want)
    if r >= 10.0:
        assert np.array_equal(got[:, :-1], np.broadcast_to(np.arange(ns, dtype=np.int32), (b, m - 1, ns)))
    if r <= 1e-4 or kind == "ball":
        assert not got[:, -1, 1:].any()


def test_ball_query_at_the_radius():
    """Points within ulps of the radius around each centre: membership is the rounding of the sum.  The contracts disagree
    on this input; the build must side with its own."""
    rng = np.random.default_rng(5)
    r = 0.25
    r2 = float(np.float32(r) * np.float32(r))
    centre = rng.uniform(-0.5, 0.5, (3, 1, 3)).astype(np.float32)
    xyz = (centre.astype(np.float64) + on_sphere(rng, 3, 512, r2).astype(np.float64)).astype(np.float32)
    with oracle_contract(0):
        at0 = pn2.ball_query(centre, xyz, r, 96)
    with oracle_contract(pn2_ref.CONTRACT):
        want = pn2.ball_query(centre, xyz, r, 96)
    assert not np.array_equal(at0, want), "the input no longer tells the contracts apart"
    assert np.array_equal(host(pn2_ref.ball_query(dev(centre), dev(xyz), r, 96)), want)


GROUP_CASES = [(5, 3, 1024, 32, 32), (4, 128, 32, 16, 32), (2, 7, 50, 5, 3), (1, 259, 16, 1, 16)]


@pytest.mark.parametrize("b,c,n,npoint,ns", GROUP_CASES)
def test_group_and_gather_forward(b, c, n, npoint, ns):
    # the inputs of tests/test_pn2_ops_gpu.py::test_group_gather_exact
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((b, c, n)).astype(np.float32)
    idx = rng.integers(0, n, (b, npoint, ns)).astype(np.int32)
    assert same_bits(host(pn2_ref.group_points(dev(pts), dev(idx))), pn2.group_points(pts, idx))
    gidx = rng.integers(0, n, (b, npoint)).astype(np.int32)
    assert same_bits(host(pn2_ref.gather_points(dev(pts), dev(gidx))), pn2.gather_points(pts, gidx))


NN_CASES = [(3, 500, 64, 16), (2, 64, 2, 4), (2, 1300, 1100, 3), (1, 5, 1, 2)]       # m < 3 twice; duplicated known points


def nn_inputs(b, n, m, c):
    # the inputs of tests/test_pn2_ops_gpu.py::test_three_nn_interpolate
    rng = np.random.default_rng(9)
    unknown = rng.standard_normal((b, n, 3)).astype(np.float32)
    known = rng.standard_normal((b, m, 3)).astype(np.float32)
    if m > 8:
        known[:, 5] = known[:, 2]
    feats = rng.standard_normal((b, c, m)).astype(np.float32)
    w = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
    return rng, unknown, known, feats, w


@pytest.mark.parametrize("b,n,m,c", NN_CASES)
def test_three_nn_and_interpolate_forward(b, n, m, c):
    _, unknown, known, feats, w = nn_inputs(b, n, m, c)
    d2, i = pn2_ref.three_nn(dev(unknown), dev(known))
    with oracle_contract(pn2_ref.CONTRACT):
        d2w, iw = pn2.three_nn(unknown, known)
        out_w = pn2.three_interpolate(feats, iw, w)
    assert np.array_equal(host(i), iw)
    assert same_bits(host(d2), d2w)
    if m < 3:                                         # the unfilled bests: 1e40 stored as float, index 0
        assert np.isinf(d2w[..., m:]).all() and not iw[..., m:].any()
    assert same_bits(host(pn2_ref.three_interpolate(dev(feats), dev(iw), dev(w))), out_w)


def exact_ints(rng, shape):
    return rng.integers(-64, 65, shape).astype(np.float32)


def max_terms(idx, n_dest):
    """Largest number of terms any destination of one batch element receives."""
    flat = idx.reshape(idx.shape[0], -1).astype(np.int64)
    return max(int(np.bincount(r, minlength=n_dest).max()) for r in flat)


@pytest.mark.parametrize("b,c,n,npoint,ns", GROUP_CASES + [(3, 40, 1024, 32, 32)])
def test_group_and_gather_grad_exact_sums(b, c, n, npoint, ns):
    """Integer gradients |v| <= 64 and at most 1024 terms a destination: every partial sum is an integer below 2^24, so
    the atomicAdd order cannot show and the comparison is exact.  The last case sends 1024 terms to 4 destinations."""
    rng = np.random.default_rng(21)
    hi = 4 if c == 40 else n
    idx = rng.integers(0, hi, (b, npoint, ns)).astype(np.int32)
    gidx = rng.integers(0, hi, (b, npoint)).astype(np.int32)
    assert max_terms(idx, n) <= 1024 and max_terms(gidx, n) <= 1024
    go = exact_ints(rng, (b, c, npoint, ns))
    assert same_bits(host(pn2_ref.group_points_grad(dev(go), dev(idx), n)), pn2.group_points_grad(go, idx, n))
    go = exact_ints(rng, (b, c, npoint))
    assert same_bits(host(pn2_ref.gather_points_grad(dev(go), dev(gidx), n)), pn2.gather_points_grad(go, gidx, n))


@pytest.mark.parametrize("b,n,m,c", NN_CASES)
def test_three_interpolate_grad_exact_sums(b, n, m, c):
    """Weights in {0.25, 0.5, 1} times integer gradients |v| <= 64: every term is a multiple of 0.25 of size <= 64 and a
    destination gets at most 1024 of them, so every partial sum is exact."""
    rng, unknown, known, _, _ = nn_inputs(b, n, m, c)
    _, iw = pn2.three_nn(unknown, known)
    assert max_terms(iw, m) <= 1024
    w = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), (b, n, 3))
    go = exact_ints(rng, (b, c, n))
    got = host(pn2_ref.three_interpolate_grad(dev(go), dev(iw), dev(w), m))
    assert same_bits(got, pn2.three_interpolate_grad(go, iw, w, m))


def reorder_bound(terms_abs_sum, counts):
    """Two float32 sums of the same k terms in different orders: each is within (k - 1) * 2^-24 * sum|terms| of the exact
    sum (first order, every partial sum bounded by sum|terms|), so they are within twice that of each other."""
    return 2.0 * np.maximum(counts - 1, 0) * 2.0 ** -24 * terms_abs_sum


def scatter_stats(terms, dest, n_dest):
    """Per (batch, channel, destination): number of terms and sum of |terms|.  terms (b, c, E), dest (b, E)."""
    b, c, _ = terms.shape
    cnt = np.zeros((b, c, n_dest))
    sab = np.zeros((b, c, n_dest))
    for i in range(b):
        cnt[i] += np.bincount(dest[i], minlength=n_dest)[None]
        for l in range(c):
            sab[i, l] = np.bincount(dest[i], weights=np.abs(terms[i, l].astype(np.float64)), minlength=n_dest)
    return cnt, sab


def test_grads_random_floats_within_the_reordering_bound():
    rng = np.random.default_rng(33)
    b, c, n, npoint, ns = 3, 6, 64, 32, 32
    idx = rng.integers(0, n, (b, npoint, ns)).astype(np.int32)
    go = rng.standard_normal((b, c, npoint, ns)).astype(np.float32)
    got = host(pn2_ref.group_points_grad(dev(go), dev(idx), n)).astype(np.float64)
    cnt, sab = scatter_stats(go.reshape(b, c, -1), idx.reshape(b, -1), n)
    assert (np.abs(got - pn2.group_points_grad(go, idx, n)) <= reorder_bound(sab, cnt)).all()

    gidx = rng.integers(0, 8, (b, 500)).astype(np.int32)
    go = rng.standard_normal((b, c, 500)).astype(np.float32)
    got = host(pn2_ref.gather_points_grad(dev(go), dev(gidx), n)).astype(np.float64)
    cnt, sab = scatter_stats(go, gidx, n)
    assert (np.abs(got - pn2.gather_points_grad(go, gidx, n)) <= reorder_bound(sab, cnt)).all()

    nn, m = 300, 20
    iw = rng.integers(0, m, (b, nn, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (b, nn, 3)).astype(np.float32)
    go = rng.standard_normal((b, c, nn)).astype(np.float32)
    got = host(pn2_ref.three_interpolate_grad(dev(go), dev(iw), dev(w), m)).astype(np.float64)
    terms = (go[:, :, :, None] * w[:, None, :, :]).reshape(b, c, -1)          # float32 products, as both sides form them
    cnt, sab = scatter_stats(terms, iw.reshape(b, -1), m)
    assert (np.abs(got - pn2.three_interpolate_grad(go, iw, w, m)) <= reorder_bound(sab, cnt)).all()


# ---------------------------------------------------------------------------------------------- c. shipped kernels == build
M1, M2, RADIUS, NSAMPLE = 32, 16, 0.2, 32            # the encoder's first two levels
THREE_NN_ULP_CAP = 2                                 # measured on the CPU, oracle at 0 against oracle at 6, inputs below


def shipped_inputs():
    """name -> (b, 1024, point_stride) float32: two synthetic scenes with their constant padding clouds, centred
    unit-ball clouds (points inside the skip radius), and the tie-heavy families."""
    from msr3d_amd.synth import synth_batch
    out = {}
    fts = synth_batch(11, 2, O=24, P=1024, n_valid=[20, 23])["obj_fts"]
    out["scenes"] = fts.reshape(-1, 1024, 6).numpy().copy()
    rng = np.random.default_rng(4)
    out["ball"] = make_cloud(rng, 8, 1024, "ball")
    out["dup"] = make_cloud(rng, 4, 1024, "dup")
    out["grid"] = make_cloud(rng, 4, 1024, "grid")
    out["mixed"] = make_cloud(rng, 4, 1024, "mixed")
    return out


def oracle_levels(xyz):
    i1 = pn2.furthest_point_sampling(xyz, M1)
    x1 = take_rows(xyz, i1)
    ball = pn2.ball_query(x1, xyz, RADIUS, NSAMPLE)
    i2 = pn2.furthest_point_sampling(x1, M2)
    x2 = take_rows(x1, i2)
    d2, i3 = pn2.three_nn(xyz, x1)
    return dict(idx1=i1, xyz1=x1, ball=ball, idx2=i2, xyz2=x2, nn_d2=d2, nn_idx=i3)


def ulp_distance(a, b):
    """Non-negative finite floats: their bit patterns are ordered like the values."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def fused_launch(pts):
    from msr3d_amd import _lib
    lib = _lib.load()
    b, n, ps = pts.shape
    i32 = dict(dtype=torch.int32, device="cuda")
    idx1, idx2 = torch.full((b, M1), -1, **i32), torch.full((b, M2), -1, **i32)
    xyz1 = torch.full((b, M1, 3), float("nan"), device="cuda")
    xyz2 = torch.full((b, M2, 3), float("nan"), device="cuda")
    ball = torch.full((b, M1, NSAMPLE), -1, **i32)
    const = torch.full((b,), 7, dtype=torch.uint8, device="cuda")
    rc = lib.msr3d_sa_fps2_query_flags(b, n, ps, M1, M2, pts.data_ptr(), idx1.data_ptr(), xyz1.data_ptr(),
                                       idx2.data_ptr(), xyz2.data_ptr(), None, ctypes.c_float(RADIUS), NSAMPLE,
                                       ball.data_ptr(), const.data_ptr(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return dict(idx1=idx1, xyz1=xyz1, ball=ball, idx2=idx2, xyz2=xyz2)


def test_shipped_kernels_against_the_build():
    """Kernel at contract 0 == oracle at 0 (the rest of the suite) and oracle at 6 == build (above).  Where the oracle
    gives the same indices at 0 and at 6 -- required of EVERY input here, zero excluded -- kernel == build exactly.
    three_nn's distances are two roundings of one sum: at most THREE_NN_ULP_CAP = 2 units in the last place apart, the
    largest difference the oracle shows between contracts 0 and 6 on these inputs (measured on the CPU, no margin)."""
    from msr3d_amd.pointnet2 import _ext
    excluded, worst = [], 0
    for name, pts in shipped_inputs().items():
        xyz = np.ascontiguousarray(pts[..., :3])
        with oracle_contract(0):
            o0 = oracle_levels(xyz)
        with oracle_contract(pn2_ref.CONTRACT):
            o6 = oracle_levels(xyz)
        if not all(np.array_equal(o0[k], o6[k]) for k in ("idx1", "ball", "idx2", "nn_idx")):
            excluded.append(name)
            continue
        worst = max(worst, int(ulp_distance(o0["nn_d2"], o6["nn_d2"]).max()))

        x = dev(xyz)
        r_i1 = pn2_ref.furthest_point_sampling(x, M1)
        r_x1 = pn2_ref.gather_points(x.transpose(1, 2).contiguous(), r_i1).transpose(1, 2).contiguous()
        r_ball = pn2_ref.ball_query(r_x1, x, RADIUS, NSAMPLE)
        r_i2 = pn2_ref.furthest_point_sampling(r_x1, M2)
        r_x2 = pn2_ref.gather_points(r_x1.transpose(1, 2).contiguous(), r_i2).transpose(1, 2).contiguous()
        r_d2, r_i3 = pn2_ref.three_nn(x, r_x1)
        ref = dict(idx1=r_i1, xyz1=r_x1, ball=r_ball, idx2=r_i2, xyz2=r_x2)

        k_i1 = _ext.furthest_point_sampling(x, M1)
        assert torch.equal(k_i1, r_i1), name
        assert torch.equal(_ext.ball_query(r_x1, x, RADIUS, NSAMPLE), r_ball), name
        assert torch.equal(_ext.furthest_point_sampling(r_x1, M2), r_i2), name
        fused = fused_launch(dev(pts))
        for k, v in ref.items():
            assert torch.equal(fused[k], v), (name, k)
        k_d2, k_i3 = _ext.three_nn(x, r_x1)
        assert torch.equal(k_i3, r_i3), name
        d = ulp_distance(host(k_d2), host(r_d2))
        assert int(d.max()) <= THREE_NN_ULP_CAP, (name, int(d.max()))
    assert excluded == [], f"oracle contracts 0 and {pn2_ref.CONTRACT} index these inputs differently: {excluded}"
    assert worst == THREE_NN_ULP_CAP, f"oracle 0 against {pn2_ref.CONTRACT}: {worst} ulp, the stated cap is {THREE_NN_ULP_CAP}"
