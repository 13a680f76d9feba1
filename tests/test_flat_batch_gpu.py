"""hgmm_flat_train_batch on the MI355X: B independent flat fits in one launch set.

Member b of a batch is ``ctx.flat_train`` on that member alone -- its cloud bound (or uploaded with ``set_points``), no
weights in force -- BIT FOR BIT: inv, mu, w, cov, lls (and with it n_iter) and converged, whatever B is and whoever the
neighbours are.  "Bitwise" is equality of the bytes (``tobytes``), so that NaNs compare.  The shapes are the smallest at which
the batched kernels can go wrong: waves without rows, grids below and at the two-per-CU floor, a last wave cut short, every
slot count with a full and a ragged last slot, members that stop at different iterations and take different row loops."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import flat_em

pytestmark = pytest.mark.gpu

FLAVOURS = [("W", "diag"), ("W", "spherical"), ("G", "diag")]
NAMES = ("inv", "mu", "w", "cov", "lls", "converged")


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def cloud(seed, n, k=4, spread=0.05):
    rs = np.random.RandomState(seed)
    c = rs.rand(k, 3)
    return (c[rs.randint(k, size=n)] + spread * rs.randn(n, 3)).astype(np.float32)


def init(seed, J, cov_type="diag", cov=0.1):
    """Initial parameters that do not depend on the cloud (a member may have fewer points than components)."""
    rs = np.random.RandomState(1000 + seed)
    mu = rs.rand(J, 3).astype(np.float32)
    return mu, np.full((J, 3) if cov_type == "diag" else (J,), cov, np.float32), np.full(J, 1.0 / J, np.float32)


def same_bytes(a, b, what):
    """The six outputs of one fit against another's, byte for byte; lls carries n_iter in its length."""
    for name, x, y in zip(NAMES, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, "%s: %s is %s %s, not %s %s" % (what, name, x.shape, x.dtype, y.shape, y.dtype)
        assert x.tobytes() == y.tobytes(), "%s: %s differs in %d elements" % (what, name, int((x != y).sum()))


def serial(ctx, X, max_iter, tol, p, cov_type, variant):
    """The serial side of every comparison: this member alone, no weights."""
    ctx.set_points(X)
    ctx.flat_set_weights(None)
    return ctx.flat_train(max_iter, tol, p[0], p[1], p[2], cov_type, variant)


def batch(ctx, clouds, max_iter, tol, params, cov_type, variant):
    hs = [ctx.points_create(X) for X in clouds]
    try:
        return ctx.flat_train_batch(hs, max_iter, tol, [p[0] for p in params], [p[1] for p in params],
                                    [p[2] for p in params], cov_type, variant)
    finally:
        for h in hs:
            ctx.points_destroy(h)


def check_batch(ctx, clouds, max_iter, tol, params, cov_type, variant, what=""):
    got = batch(ctx, clouds, max_iter, tol, params, cov_type, variant)
    want = [serial(ctx, X, max_iter, tol, p, cov_type, variant) for X, p in zip(clouds, params)]
    assert len(got) == len(clouds)
    for b, (g, w) in enumerate(zip(got, want)):
        same_bytes(g, w, "%s member %d (n = %d)" % (what, b, len(clouds[b])))
    return got, want


# ---- 1 ----------------------------------------------------------------------------------------------------------------
RAGGED = (1, 3, 5, 256, 257, 2049, 5000)


@pytest.mark.parametrize("J", [5, 100])
@pytest.mark.parametrize("variant,cov_type", FLAVOURS)
def test_ragged_sizes_are_bitwise_the_serial_fits(ctx, variant, cov_type, J):
    """n = 1, 3, 5: a workgroup whose later waves own no row; 256 / 257: a grid below the two-per-CU floor and a last wave cut
    short; 2049 at the floor on a 256-CU chip; 5000 above it."""
    clouds = [cloud(10 + i, n) for i, n in enumerate(RAGGED)]
    params = [init(i, J, cov_type) for i in range(len(RAGGED))]
    got, _ = check_batch(ctx, clouds, 5, 0.0, params, cov_type, variant, "J = %d %s/%s" % (J, variant, cov_type))
    assert all(len(g[4]) == 5 and not g[5] for g in got)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [64 * s - d for s in range(1, 17) for d in (1, 0)])
def test_every_slot_count(ctx, J):
    """The sixteen NSLOT instantiations of the batched fused kernel, each with a ragged and a full last slot."""
    clouds = [cloud(30, 300), cloud(31, 301), cloud(32, 1000)]
    params = [init(40 + i, J) for i in range(3)]
    check_batch(ctx, clouds, 2, 0.0, params, "diag", "W", "J = %d" % J)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
# (seed, n, clusters, spread) chosen with oracle/flat_em.train at J = 4, tol = 1e-3, max_iter = 40: the float64 loop stops after
# 5, 10, 14 and 19 iterations, each with the deciding |change| a factor >= 1.3 away from tol on either side
STOPPERS = [(30, 810, 2, 0.01), (10, 470, 6, 0.01), (32, 844, 4, 0.1), (13, 521, 3, 0.2)]


def stopper(seed, n, k, spread):
    return cloud(seed, n, k, spread), (np.random.RandomState(100 + seed).rand(4, 3).astype(np.float32),
                                       np.full((4, 3), 0.1, np.float32), np.full(4, 0.25, np.float32))


def test_the_stopper_clouds_stop_where_they_were_chosen_to():
    """(no GPU work) the recipe above against the oracle it was chosen with"""
    f64 = lambda a: np.asarray(a, np.float64)
    its = []
    for s in STOPPERS:
        X, p = stopper(*s)
        o = flat_em.train(f64(X), 40, 1e-3, f64(p[0]), f64(p[1]), f64(p[2]), "diag", "W")
        assert o[5]
        its.append(len(o[4]))
    assert its == [5, 10, 14, 19]


def test_members_that_stop_at_different_iterations(ctx):
    pairs = [stopper(*s) for s in STOPPERS]
    clouds, params = [p[0] for p in pairs], [p[1] for p in pairs]
    want = [serial(ctx, X, 40, 1e-3, p, "diag", "W") for X, p in zip(clouds, params)]
    its = sorted(len(w[4]) for w in want)
    print("serial n_iter:", [len(w[4]) for w in want])
    assert all(w[5] for w in want) and its[-1] < 40 and min(np.diff(its)) >= 3, its       # the precondition
    got = batch(ctx, clouds, 40, 1e-3, params, "diag", "W")
    for b, (g, w) in enumerate(zip(got, want)):
        same_bytes(g, w, "member %d" % b)
    # the order of the members does not matter either: the early stopper last
    got = batch(ctx, clouds[::-1], 40, 1e-3, params[::-1], "diag", "W")
    for b, (g, w) in enumerate(zip(got, want[::-1])):
        same_bytes(g, w, "reversed member %d" % b)


@pytest.mark.parametrize("max_iter", [0, 1])
def test_no_iteration_and_one(ctx, max_iter):
    pairs = [stopper(*s) for s in STOPPERS[:3]]
    got, _ = check_batch(ctx, [p[0] for p in pairs], max_iter, 1e-3, [p[1] for p in pairs], "diag", "W", "max_iter = %d" % max_iter)
    assert all(len(g[4]) == max_iter for g in got)


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_one_member_on_the_row_maximum_loop(ctx):
    """The recipe of test_train_huge_shift_takes_the_row_maximum_variant (flavour G, cov0 = 1e-15: constants above 2^60) as the
    middle member; its neighbours stay on the constant-shift loop.  The choice is each wave's, from its member's table."""
    rs = np.random.RandomState(22)
    centres = rs.rand(5, 3).astype(np.float32)
    Xh = (np.repeat(centres, 40, axis=0) + (1e-8 * rs.randn(200, 3)).astype(np.float32)).astype(np.float32)
    huge = (centres.copy(), np.full((5, 3), 1e-15, np.float32), np.full(5, 0.2, np.float32))
    clouds = [cloud(50, 700), Xh, cloud(51, 333)]
    params = [init(50, 5), huge, init(51, 5)]
    got, _ = check_batch(ctx, clouds, 2, 0.0, params, "diag", "G")
    assert np.isfinite(got[1][4]).all() and np.isfinite(got[1][1]).all()


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_restarts_of_one_resident_cloud(ctx):
    X = cloud(60, 1500, 6)
    params = [init(60, 12), init(61, 12), init(62, 12), init(60, 12)]           # slots 0 and 3: the same initialisation
    h = ctx.points_create(X)
    try:
        got = ctx.flat_train_batch([h] * 4, 6, 0.0, [p[0] for p in params], [p[1] for p in params], [p[2] for p in params])
    finally:
        ctx.points_destroy(h)
    for b, p in enumerate(params):
        same_bytes(got[b], serial(ctx, X, 6, 0.0, p, "diag", "W"), "restart %d" % b)
    same_bytes(got[0], got[3], "slots 0 and 3")
    assert got[0][1].tobytes() != got[1][1].tobytes()


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_member(ctx):
    clouds = [cloud(70, 900), cloud(71, 640), cloud(72, 1100)]
    clouds[1][123] = np.nan
    params = [init(70 + i, 8) for i in range(3)]
    got, _ = check_batch(ctx, clouds, 3, 0.0, params, "diag", "W")
    assert np.isfinite(got[0][1]).all() and np.isfinite(got[2][1]).all() and np.isfinite(got[0][4]).all()
    assert np.isnan(got[1][4]).any()


# ---- 7 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,cov_type", FLAVOURS)
def test_against_the_oracle_and_the_reference(ctx, variant, cov_type):
    """Not through the serial entry: the fixture member of a batch of three against the float64 oracle and the reference's
    recorded float32 trajectory, with test_train_small's tolerances."""
    g = load_golden("flat_small_%s_%s.npz" % (variant, cov_type))
    X = g["X"]
    p = (g["mu0"], g["cov0"], g["w0"])
    J = len(g["w0"])
    other = init(80, J, cov_type)
    got = batch(ctx, [X[:700].copy(), X, cloud(80, 450)], 5, 0.0, [p, p, other], cov_type, variant)
    inv, mu, w, cov, lls, conv = got[1]
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    o_inv, o_mu, o_w, o_cov, o_lls, _ = flat_em.train(f64(X), 5, 0.0, f64(p[0]), f64(p[1]), f64(p[2]), cov_type, variant)
    assert len(lls) == 5 and not conv
    np.testing.assert_allclose(lls, o_lls, rtol=0, atol=2e-5)
    np.testing.assert_allclose(mu, o_mu, rtol=0, atol=5e-6)
    np.testing.assert_allclose(w, o_w, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(cov, o_cov, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(inv, o_inv, rtol=1e-4)
    np.testing.assert_allclose(lls, g["it5_lls"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(mu, g["it5_mu"], rtol=0, atol=2e-5)


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_a_serial_fit_in_progress_is_left_alone(ctx):
    X = cloud(90, 3000, 6)
    p = init(90, 70)
    others = [cloud(91, 800), cloud(92, 2100)]
    op = [init(91, 70), init(92, 70)]

    def run(interrupt):
        ctx.set_points(X)
        ctx.flat_set_weights(None)
        ctx.flat_train_begin(0.0, p[0], p[1], p[2], lls_capacity=4)
        ctx.flat_train_step(2)
        if interrupt:
            batch(ctx, others, 3, 0.0, op, "diag", "W")
        ctx.flat_train_step(2)
        return ctx.flat_train_end()

    plain, cut = run(False), run(True)
    for name, a, b in zip(NAMES + ("n_iter",), plain, cut):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), name
    assert ctx.num_points == 3000


def test_weights_and_the_bound_cloud_survive_a_batch(ctx):
    X = cloud(93, 1200, 5)
    s = (1 + np.arange(1200) % 3).astype(np.float32)
    s[::7] = 0
    p = init(93, 9)
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    before = ctx.flat_train(4, 0.0, p[0], p[1], p[2])
    inv = before[0]
    e_before = ctx.flat_estep(inv, before[1], before[2], want_lpn=True)
    e_before = (np.float64(e_before[0]), e_before[1].get(), e_before[2].get())
    batch(ctx, [cloud(94, 500), cloud(95, 77)], 3, 0.0, [init(94, 9), init(95, 9)], "diag", "W")
    after = ctx.flat_train(4, 0.0, p[0], p[1], p[2])                          # still weighted, still on X
    same_bytes(after, before, "the weighted serial fit after a batch")
    e_after = ctx.flat_estep(inv, before[1], before[2], want_lpn=True)
    e_after = (np.float64(e_after[0]), e_after[1].get(), e_after[2].get())
    for a, b in zip(e_before, e_after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    ctx.flat_set_weights(None)
    unweighted = ctx.flat_train(4, 0.0, p[0], p[1], p[2])
    assert unweighted[1].tobytes() != before[1].tobytes()                     # (the weights did matter)


# ---- 9 ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    import hgmm_amd
    from hgmm_amd._native import HgmmError
    X = cloud(96, 900)
    p = init(96, 6)
    base = serial(ctx, X, 3, 0.0, p, "diag", "W")
    lib = ctx.lib
    h = ctx.points_create(cloud(97, 400))
    other = hgmm_amd.Context(0)
    h_other = other.points_create(cloud(98, 300))
    vp = C.c_void_p
    i32p = C.POINTER(C.c_int32)

    def call(B=1, clouds="ok", cov_type=0, variant=0, J=6, max_iter=2, null=(), handle=None):
        mu = np.tile(p[0], (max(B, 1), 1, 1)).astype(np.float32)
        cov = np.tile(p[1], (max(B, 1), 1, 1)).astype(np.float32)
        w = np.tile(p[2], (max(B, 1), 1)).astype(np.float32)
        n_it, conv = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
        arr = None if clouds is None else (vp * max(B, 1))(*[(handle or h).value if clouds == "ok" else None] * max(B, 1))
        ptr = lambda name, a: None if name in null else a.ctypes.data_as(vp)
        rc = lib.hgmm_flat_train_batch(ctx.h, B, arr, cov_type, variant, J, max_iter, 0.0, ptr("mu", mu), ptr("cov", cov),
                                       ptr("w", w), None, None,
                                       None if "n_iter" in null else n_it.ctypes.data_as(i32p),
                                       None if "converged" in null else conv.ctypes.data_as(i32p))
        return rc, (lib.hgmm_last_error(ctx.h) or b"").decode()

    ARG, STATE = -2, -3
    cases = [
        ("B = 0", dict(B=0), ARG, "outside 1..4096"),
        ("B = 4097", dict(B=4097), ARG, "outside 1..4096"),
        ("clouds NULL", dict(clouds=None), ARG, "clouds is NULL"),
        ("a NULL member", dict(clouds="null"), ARG, "member 0 is NULL"),
        ("another context's handle", dict(handle=h_other), ARG, "another context"),
        ("mu NULL", dict(null=("mu",)), ARG, "must not be NULL"),
        ("cov NULL", dict(null=("cov",)), ARG, "must not be NULL"),
        ("w NULL", dict(null=("w",)), ARG, "must not be NULL"),
        ("n_iter_out NULL", dict(null=("n_iter",)), ARG, "must not be NULL"),
        ("converged_out NULL", dict(null=("converged",)), ARG, "must not be NULL"),
        ("max_iter < 0", dict(max_iter=-1), ARG, "max_iter < 0"),
        ("bad cov_type", dict(cov_type=2), ARG, "cov_type must be 0 (diag) or 1 (spherical)"),
        ("bad variant", dict(variant=5), ARG, "variant must be 0 (W) or 1 (G)"),
        ("G with spherical", dict(variant=1, cov_type=1), ARG, "diag-only"),
        ("J = 0", dict(J=0), ARG, "stays serial"),
        ("J = 1025", dict(J=1025), ARG, "stays serial"),
    ]
    try:
        for name, kw, code, text in cases:
            rc, msg = call(**kw)
            assert rc == code and text in msg, (name, rc, msg)
            same_bytes(ctx.flat_train(3, 0.0, p[0], p[1], p[2]), base, "the serial fit after refusal '%s'" % name)
            assert ctx.num_points == 900
        # the Python layer turns a refusal into HgmmError
        with pytest.raises(HgmmError, match="stays serial"):
            ctx.flat_train_batch([h], 2, 0.0, [np.zeros((1025, 3), np.float32)], [np.ones((1025, 3), np.float32)],
                                 [np.ones(1025, np.float32)])
    finally:
        other.points_destroy(h_other)
        other.close()
        ctx.points_destroy(h)


def test_refused_under_a_communicator():
    """HGMM_ERR_STATE: a context with the host communicator of one rank attached."""
    import hgmm_amd
    from hgmm_amd._native import HgmmError
    c = hgmm_amd.Context(0)
    try:
        c.comm_init_host(1, 0, "hgmm_flat_batch_w1_%d" % os.getpid())
        X = cloud(99, 500)
        p = init(99, 6)
        c.set_points(X)
        base = c.flat_train(2, 0.0, p[0], p[1], p[2])
        h = c.points_create(X)
        with pytest.raises(HgmmError, match=r"\(-3\).*communicator"):
            c.flat_train_batch([h], 2, 0.0, [p[0]], [p[1]], [p[2]])
        same_bytes(c.flat_train(2, 0.0, p[0], p[1], p[2]), base, "the serial fit after the refusal")
    finally:
        c.close()


# ---- 10 ---------------------------------------------------------------------------------------------------------------
def test_train_gmm_batch_mirrors(ctx):
    import hgmm_amd
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    hgmm_amd.set_default_context(ctx)
    clouds = [cloud(110, 700), cloud(111, 1300), cloud(112, 64)]
    params = [init(110 + i, 10) for i in range(3)]
    dev = W.asarray(clouds[1], ctx)                                        # one member resident, two host arrays
    members = [clouds[0], dev, clouds[2]]
    for mod, kw in ((W, dict(cov_type="diag")), (G, {})):
        got = mod.train_gmm_batch(members, 4, 0.0, [p[0] for p in params], [p[1] for p in params], [p[2] for p in params], **kw)
        for b, X in enumerate(clouds):
            want = mod.train_gmm(X, 4, 0.0, params[b][0], params[b][1], params[b][2], **kw)
            assert len(got[b]) == 5
            for x, y in zip(got[b], want):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    sph = [init(120 + i, 10, "spherical") for i in range(3)]
    got = W.train_gmm_batch(members, 3, 0.0, [p[0] for p in sph], [p[1] for p in sph], [p[2] for p in sph], cov_type="spherical")
    want = W.train_gmm(dev, 3, 0.0, sph[1][0], sph[1][1], sph[1][2], cov_type="spherical")
    for x, y in zip(got[1], want):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    dev.free()


def test_fit_batch_is_the_loop_of_fits(ctx):
    import hgmm_amd
    from hgmm_amd.gmm_waymo.gmm import GMM_GPU_Base
    hgmm_amd.set_default_context(ctx)
    frames = [cloud(130 + i, 500 + 37 * i) for i in range(4)]
    np.random.seed(7)
    loop = [GMM_GPU_Base(12, max_iter=5, tol=1e-4).fit(X) for X in frames]
    np.random.seed(7)
    models = GMM_GPU_Base(12, max_iter=5, tol=1e-4).fit_batch(frames)
    assert len(models) == 4
    for a, b in zip(models, loop):
        for name in ("means_", "covariances_", "weights_", "inv_covs"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert np.asarray(a.lls).tobytes() == np.asarray(b.lls).tobytes()
        assert (a.num_components, a.max_iter, a.tol, a.cov_type) == (b.num_components, b.max_iter, b.tol, b.cov_type)


def test_fit_frames_in_chunks_of_four(ctx):
    from hgmm_amd.replicas import ReplicaPool, fit_frames
    frames = [cloud(140 + i, 400 + 11 * i) for i in range(9)]                 # 4 + 4 + 1
    with ReplicaPool(devices=[0]) as pool:
        np.random.seed(3)
        one = fit_frames(frames, n_components=8, max_iter=4, pool=pool)
        np.random.seed(3)
        four = fit_frames(frames, n_components=8, max_iter=4, pool=pool, batch=4)
    assert len(four) == 9
    for a, b in zip(four, one):
        for name in ("means_", "covariances_", "weights_", "inv_covs"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert np.asarray(a.lls).tobytes() == np.asarray(b.lls).tobytes()


def test_above_1024_components_falls_back_to_the_serial_loop(ctx):
    import hgmm_amd
    from hgmm_amd.gmm_waymo import gmm_impl as W
    hgmm_amd.set_default_context(ctx)
    clouds = [cloud(150, 500), cloud(151, 500)]
    params = [init(150 + i, 1025) for i in range(2)]
    got = W.train_gmm_batch(clouds, 2, 0.0, [p[0] for p in params], [p[1] for p in params], [p[2] for p in params])
    for b in range(2):
        want = W.train_gmm(clouds[b], 2, 0.0, *params[b])
        for x, y in zip(got[b], want):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_a_weighted_member_is_refused_by_name(ctx):
    import hgmm_amd
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmm_waymo.gmm import GMM_GPU_Base
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    hgmm_amd.set_default_context(ctx)
    X = cloud(160, 300)
    p = init(160, 4)
    args = (2, 0.0, [p[0]] * 2, [p[1]] * 2, [p[2]] * 2)
    dev = W.asarray(X, ctx, weights=np.ones(300, np.float32))
    try:
        with pytest.raises(ValueError, match="member 1 brings per-point weights"):
            W.train_gmm_batch([X, dev], *args)
        with pytest.raises(ValueError, match="member 1 brings per-point weights"):
            W.train_gmm_batch([X, WeightedPoints(X, np.ones(300, np.float32))], *args)
        with pytest.raises(ValueError, match="member 1 brings per-point weights"):
            ctx.flat_train_batch([W.asarray(X, ctx), dev], *args)
        with pytest.raises(ValueError, match="frame 0 brings per-point weights"):
            GMM_GPU_Base(4).fit_batch([WeightedPoints(X, np.ones(300, np.float32))])
    finally:
        dev.free()
