"""hgmm_flat_train_batch_weighted and hgmm_flat_train_batch_voxels on the MI355X: the batched flat fit with per-point weights
that belong to a slot of the call -- host arrays, or the counts of a resident voxel result.

Slot b of a weighted batch is ``set_points(X_b)``, ``flat_set_weights(s_b)``, ``flat_train(...)`` BIT FOR BIT (equality of
``tobytes()``): inv, mu, w, cov, lls (and with it n_iter) and converged, whatever B is and whoever the neighbours are.  Slot b
of a voxel batch is ``set_points_from_voxels(vc_b, tree_weights=False, flat_weights=weighted)`` followed by ``flat_train``.
The helpers ``cloud``, ``init`` and ``same_bytes`` are those of test_flat_batch_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import _flat_weight_oracle as fw
from conftest import load_golden

pytestmark = pytest.mark.gpu

FLAVOURS = [("W", "diag"), ("W", "spherical"), ("G", "diag")]
NAMES = ("inv", "mu", "w", "cov", "lls", "converged")
f64 = lambda a: np.asarray(a, dtype=np.float64)


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


def weights(n):
    """1 + (i % 3), every seventh row absent, row 0 present (n = 1 must not be all-zero)."""
    s = (1 + np.arange(n) % 3).astype(np.float32)
    s[::7] = 0
    s[0] = 1
    return s


def serial(ctx, X, s, max_iter, tol, p, cov_type, variant):
    """The serial side of every comparison: this member alone, its weights (or none) in force."""
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    return ctx.flat_train(max_iter, tol, p[0], p[1], p[2], cov_type, variant)


def batch(ctx, clouds, ws, max_iter, tol, params, cov_type, variant):
    hs = [ctx.points_create(X) for X in clouds]
    try:
        return ctx.flat_train_batch(hs, max_iter, tol, [p[0] for p in params], [p[1] for p in params],
                                    [p[2] for p in params], cov_type, variant, weights=ws)
    finally:
        for h in hs:
            ctx.points_destroy(h)


def check_batch(ctx, clouds, ws, max_iter, tol, params, cov_type, variant, what=""):
    got = batch(ctx, clouds, ws, max_iter, tol, params, cov_type, variant)
    want = [serial(ctx, X, s, max_iter, tol, p, cov_type, variant) for X, s, p in zip(clouds, ws, params)]
    assert len(got) == len(clouds)
    for b, (g, w) in enumerate(zip(got, want)):
        same_bytes(g, w, "%s member %d (n = %d)" % (what, b, len(clouds[b])))
    return got, want


# ---- 1 ----------------------------------------------------------------------------------------------------------------
RAGGED = (1, 3, 5, 256, 257, 2049, 5000)


@pytest.mark.parametrize("J", [5, 100])
@pytest.mark.parametrize("variant,cov_type", FLAVOURS)
def test_ragged_sizes_are_bitwise_the_weighted_serial_fits(ctx, variant, cov_type, J):
    """The sizes of test_flat_batch_gpu.py; in the 5000-row member rows 1000..2999 are absent as well, so that whole waves
    skip every row they own."""
    clouds = [cloud(10 + i, n) for i, n in enumerate(RAGGED)]
    ws = [weights(n) for n in RAGGED]
    ws[-1][1000:3000] = 0
    params = [init(i, J, cov_type) for i in range(len(RAGGED))]
    got, _ = check_batch(ctx, clouds, ws, 5, 0.0, params, cov_type, variant, "J = %d %s/%s" % (J, variant, cov_type))
    assert all(len(g[4]) == 5 and not g[5] for g in got)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [64 * s - d for s in range(1, 17) for d in (1, 0)])
def test_every_slot_count(ctx, J):
    """The sixteen <NSLOT, true> instantiations of the batched fused kernel, each with a ragged and a full last slot."""
    clouds = [cloud(30, 300), cloud(31, 301), cloud(32, 1000)]
    params = [init(40 + i, J) for i in range(3)]
    check_batch(ctx, clouds, [weights(len(X)) for X in clouds], 2, 0.0, params, "diag", "W", "J = %d" % J)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
# The STOPPERS clouds and initialisations of test_flat_batch_gpu.py with weights 1 + randint(0, 5), every seventh row absent;
# with tests/_flat_weight_oracle.train at J = 4, tol = 1e-3, max_iter = 40 the float64 loop stops after 5, 9, 13 and 16
# iterations, the deciding change at 0.03, 2e-5, 0.65 and 0.82 of tol and the change before it at 525, 751, 6.2 and 1.29 of tol
# (tests/test_flat_batch_weights_cpu.py restates this)
STOPPERS = [(30, 810, 2, 0.01), (10, 470, 6, 0.01), (32, 844, 4, 0.1), (13, 521, 3, 0.2)]
STOPPER_OFF = (0, 0, 0, 1)


def stopper(seed, n, k, spread, off=0):
    s = (1 + np.random.RandomState(200 + seed + 1000 * off).randint(0, 5, n)).astype(np.float32)
    s[::7] = 0
    return cloud(seed, n, k, spread), s, (np.random.RandomState(100 + seed).rand(4, 3).astype(np.float32),
                                          np.full((4, 3), 0.1, np.float32), np.full(4, 0.25, np.float32))


def test_members_that_stop_at_different_iterations(ctx):
    trio = [stopper(*s, off=o) for s, o in zip(STOPPERS, STOPPER_OFF)]
    clouds, ws, params = [t[0] for t in trio], [t[1] for t in trio], [t[2] for t in trio]
    want = [serial(ctx, X, s, 40, 1e-3, p, "diag", "W") for X, s, p in trio]
    its = sorted(len(w[4]) for w in want)
    print("serial n_iter:", [len(w[4]) for w in want])
    assert all(w[5] for w in want) and its[-1] < 40 and min(np.diff(its)) >= 2, its       # the precondition
    got = batch(ctx, clouds, ws, 40, 1e-3, params, "diag", "W")
    for b, (g, w) in enumerate(zip(got, want)):
        same_bytes(g, w, "member %d" % b)
    got = batch(ctx, clouds[::-1], ws[::-1], 40, 1e-3, params[::-1], "diag", "W")
    for b, (g, w) in enumerate(zip(got, want[::-1])):
        same_bytes(g, w, "reversed member %d" % b)


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_a_mixed_batch(ctx):
    """weighted, NULL, weighted, all-ones: two fused launches per iteration, one table."""
    clouds = [cloud(50, 700), cloud(51, 333), cloud(52, 1201), cloud(51, 333)]
    ws = [weights(700), None, weights(1201), np.ones(333, np.float32)]
    params = [init(50, 70), init(51, 70), init(52, 70), init(51, 70)]
    got, _ = check_batch(ctx, clouds, ws, 4, 0.0, params, "diag", "W", "mixed")
    same_bytes(got[3], got[1], "all-ones against NULL")
    same_bytes(got[3], serial(ctx, clouds[1], None, 4, 0.0, params[1], "diag", "W"), "all-ones against the unweighted serial fit")
    assert got[0][1].tobytes() != serial(ctx, clouds[0], None, 4, 0.0, params[0], "diag", "W")[1].tobytes()


def test_a_weighted_member_on_the_row_maximum_loop(ctx):
    """The middle member of test_one_member_on_the_row_maximum_loop, weighted, between two constant-shift neighbours."""
    rs = np.random.RandomState(22)
    centres = rs.rand(5, 3).astype(np.float32)
    Xh = (np.repeat(centres, 40, axis=0) + (1e-8 * rs.randn(200, 3)).astype(np.float32)).astype(np.float32)
    huge = (centres.copy(), np.full((5, 3), 1e-15, np.float32), np.full(5, 0.2, np.float32))
    clouds = [cloud(50, 700), Xh, cloud(51, 333)]
    params = [init(50, 5), huge, init(51, 5)]
    got, _ = check_batch(ctx, clouds, [weights(700), weights(200), weights(333)], 2, 0.0, params, "diag", "G")
    assert np.isfinite(got[1][4]).all() and np.isfinite(got[1][1]).all()


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_one_handle_four_slots(ctx):
    X = cloud(60, 1500, 6)
    sa = weights(1500)
    sb = (1 + np.random.RandomState(61).randint(0, 4, 1500)).astype(np.float32)
    pa, pb = init(60, 12), init(61, 12)
    slots = [(sa, pa), (sb, pa), (sa, pb), (sa, pa)]                            # slots 0 and 3: the same weights and start
    h = ctx.points_create(X)
    try:
        got = ctx.flat_train_batch([h] * 4, 6, 0.0, [p[0] for _, p in slots], [p[1] for _, p in slots],
                                   [p[2] for _, p in slots], weights=[s for s, _ in slots])
    finally:
        ctx.points_destroy(h)
    for b, (s, p) in enumerate(slots):
        same_bytes(got[b], serial(ctx, X, s, 6, 0.0, p, "diag", "W"), "slot %d" % b)
    same_bytes(got[0], got[3], "slots 0 and 3")
    assert got[0][1].tobytes() != got[1][1].tobytes() and got[0][1].tobytes() != got[2][1].tobytes()


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_nan_rows_of_weight_zero_change_nothing(ctx):
    clouds = [cloud(70, 900), cloud(71, 640), cloud(72, 1100)]
    ws = [weights(len(X)) for X in clouds]
    params = [init(70 + i, 8) for i in range(3)]
    finite = batch(ctx, clouds, ws, 3, 0.0, params, "diag", "W")
    absent = np.flatnonzero(ws[1] == 0)
    assert absent.size > 80
    clouds[1][absent] = np.nan
    got = batch(ctx, clouds, ws, 3, 0.0, params, "diag", "W")
    for b in range(3):
        same_bytes(got[b], finite[b], "member %d" % b)
        assert np.isfinite(got[b][1]).all() and np.isfinite(got[b][4]).all()


# ---- 7 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,cov_type", FLAVOURS)
def test_against_the_restatement(ctx, variant, cov_type):
    """Not through the serial entry: the fixture member, weighted, as the middle slot of three against the float64
    restatement, with the bounds of test_flat_weights_gpu.py::test_train_small_against_the_restatement."""
    g = load_golden("flat_small_%s_%s.npz" % (variant, cov_type))
    X = g["X"]
    p = (g["mu0"], g["cov0"], g["w0"])
    J = len(g["w0"])
    s = fw.standard_weights(len(X))
    got = batch(ctx, [X[:700].copy(), X, cloud(80, 450)], [weights(700), s, None], 5, 0.0, [p, p, init(80, J, cov_type)],
                cov_type, variant)
    inv, mu, w, cov, lls, conv = got[1]
    o_inv, o_mu, o_w, o_cov, o_lls, _ = fw.train(f64(X), s, 5, 0.0, f64(p[0]), f64(p[1]), f64(p[2]), cov_type, variant)
    print("max |dlls| %.3g, |dmu| %.3g, rel dw %.3g, rel dcov %.3g, rel dinv %.3g"
          % (np.abs(lls - o_lls).max(), np.abs(mu - o_mu).max(), np.abs(w / o_w - 1).max(), np.abs(cov / o_cov - 1).max(),
             np.abs(inv / o_inv - 1).max()))
    assert len(lls) == 5 and not conv
    np.testing.assert_allclose(lls, o_lls, rtol=0, atol=2e-5)
    np.testing.assert_allclose(mu, o_mu, rtol=0, atol=5e-6)
    np.testing.assert_allclose(w, o_w, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(cov, o_cov, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(inv, o_inv, rtol=1e-4)


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_a_serial_fit_in_progress_is_left_alone(ctx):
    X = cloud(90, 3000, 6)
    s = weights(3000)
    p = init(90, 70)
    others = [cloud(91, 800), cloud(92, 2100)]
    op = [init(91, 70), init(92, 70)]

    def run(interrupt):
        ctx.set_points(X)
        ctx.flat_set_weights(s)
        ctx.flat_train_begin(0.0, p[0], p[1], p[2], lls_capacity=4)
        ctx.flat_train_step(2)
        if interrupt:
            batch(ctx, others, [weights(800), None], 3, 0.0, op, "diag", "W")
        ctx.flat_train_step(2)
        return ctx.flat_train_end()

    plain, cut = run(False), run(True)
    for name, a, b in zip(NAMES + ("n_iter",), plain, cut):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), name
    assert ctx.num_points == 3000


def test_weights_and_the_bound_cloud_survive_a_weighted_batch(ctx):
    X = cloud(93, 1200, 5)
    s = weights(1200)
    p = init(93, 9)
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    before = ctx.flat_train(4, 0.0, p[0], p[1], p[2])
    e_before = ctx.flat_estep(before[0], before[1], before[2], want_lpn=True)
    e_before = (np.float64(e_before[0]), e_before[1].get(), e_before[2].get())
    batch(ctx, [cloud(94, 500), cloud(95, 77)], [2 * weights(500), weights(77)], 3, 0.0, [init(94, 9), init(95, 9)], "diag", "W")
    after = ctx.flat_train(4, 0.0, p[0], p[1], p[2])                          # still weighted by s, still on X
    same_bytes(after, before, "the weighted serial fit after a weighted batch")
    e_after = ctx.flat_estep(before[0], before[1], before[2], want_lpn=True)
    e_after = (np.float64(e_after[0]), e_after[1].get(), e_after[2].get())
    for a, b in zip(e_before, e_after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_refusals_touch_nothing(ctx):
    from hgmm_amd._native import HgmmError
    X = cloud(96, 900)
    s = weights(900)
    p = init(96, 6)
    base = serial(ctx, X, s, 3, 0.0, p, "diag", "W")
    hs = [ctx.points_create(cloud(97, 400)), ctx.points_create(cloud(98, 300))]
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)

    def call(ws):
        mu, cov, w = (np.tile(a, (2,) + (1,) * a.ndim).astype(np.float32) for a in p)
        n_it, conv = np.zeros(2, np.int32), np.zeros(2, np.int32)
        sp = (vp * 2)(*[None if a is None else a.ctypes.data for a in ws])
        rc = ctx.lib.hgmm_flat_train_batch_weighted(ctx.h, 2, (vp * 2)(*[h.value for h in hs]), sp, 0, 0, 6, 2, 0.0,
                                                    mu.ctypes.data_as(vp), cov.ctypes.data_as(vp), w.ctypes.data_as(vp), None,
                                                    None, n_it.ctypes.data_as(i32p), conv.ctypes.data_as(i32p))
        return rc, (ctx.lib.hgmm_last_error(ctx.h) or b"").decode()

    try:
        bad = weights(300)
        bad[17] = np.nan
        rc, msg = call([weights(400), bad])
        assert rc == -2 and "slot 1" in msg and "weight 17" in msg, (rc, msg)
        same_bytes(ctx.flat_train(3, 0.0, p[0], p[1], p[2]), base, "the serial weighted fit after the NaN refusal")
        for value in (-1.0, np.inf):
            bad = weights(300)
            bad[5] = value
            rc, msg = call([None, bad])
            assert rc == -2 and "slot 1" in msg and "weight 5" in msg, (rc, msg)
        rc, msg = call([np.zeros(400, np.float32), weights(300)])
        assert rc == -2 and "slot 0" in msg and "all 400 weights are zero" in msg, (rc, msg)
        same_bytes(ctx.flat_train(3, 0.0, p[0], p[1], p[2]), base, "the serial weighted fit after the all-zero refusal")
        # a wrong length: the library cannot see it, the Python layer can (a DevicePoints knows its rows)
        import hgmm_amd._flat as _flat
        dev = _flat.DevicePoints(cloud(99, 250), ctx)
        try:
            with pytest.raises(ValueError, match=r"member 0: weights must have shape \[250\]"):
                ctx.flat_train_batch([dev], 2, 0.0, [p[0]], [p[1]], [p[2]], weights=[np.ones(249, np.float32)])
        finally:
            dev.free()
        same_bytes(ctx.flat_train(3, 0.0, p[0], p[1], p[2]), base, "the serial weighted fit after the length refusal")
        assert ctx.num_points == 900
        with pytest.raises(HgmmError, match="stays serial"):                    # the batch entry's own refusals apply
            ctx.flat_train_batch([hs[0]], 2, 0.0, [np.zeros((1025, 3), np.float32)], [np.ones((1025, 3), np.float32)],
                                 [np.ones(1025, np.float32)], weights=[weights(400)])
    finally:
        for h in hs:
            ctx.points_destroy(h)


# ---- 9 ----------------------------------------------------------------------------------------------------------------
VOXEL = 0.17


@pytest.fixture(scope="module")
def scans():
    return [np.random.RandomState(300 + i).rand(3000 + 500 * i, 3) for i in range(4)]       # float64, 3000 .. 4500 rows


@pytest.mark.parametrize("weighted", [True, False])
def test_the_voxel_entry(ctx, scans, weighted):
    from hgmm_amd._native import HgmmError
    X = cloud(170, 777)
    s = weights(777)
    p0 = init(170, 9)
    resident = serial(ctx, X, s, 3, 0.0, p0, "diag", "W")
    result = ctx.voxel_down_sample_batch(scans, VOXEL, download=False)
    assert all(150 <= m <= 600 for m in result.m), result.m
    bytes_before = [a.tobytes() for a in ctx.voxel_down_sample_get()]
    members = [2, 0, 0, 1]
    vcs = [result.member(k) for k in members]
    params = [init(171 + b, 20) for b in range(4)]
    params[2] = params[1]                                                      # member 0 twice, the same start: the same bits
    got = ctx.flat_train_batch_voxels(vcs, 6, 0.0, [p[0] for p in params], [p[1] for p in params], [p[2] for p in params],
                                      weighted=weighted)
    # the resident cloud and its weights are what they were; so is the voxel result
    same_bytes(ctx.flat_train(3, 0.0, p0[0], p0[1], p0[2]), resident, "the resident weighted fit after the voxel batch")
    assert ctx.num_points == 777
    assert [a.tobytes() for a in ctx.voxel_down_sample_get()] == bytes_before
    same_bytes(got[1], got[2], "slots 1 and 2")
    for b, vc in enumerate(vcs):
        ctx.set_points_from_voxels(vc, tree_weights=False, flat_weights=weighted)
        same_bytes(got[b], ctx.flat_train(6, 0.0, params[b][0], params[b][1], params[b][2]), "slot %d (member %d)" % (b, members[b]))
    assert [a.tobytes() for a in ctx.voxel_down_sample_get()] == bytes_before
    if weighted:
        return
    # refusals: a member out of range (the C entry), a stale VoxelCloud (the Python layer)
    mu, cov, w = (np.ascontiguousarray(a[None]) for a in params[0])
    n_it, conv = np.zeros(1, np.int32), np.zeros(1, np.int32)
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    for member in (4, -1):
        rc = ctx.lib.hgmm_flat_train_batch_voxels(ctx.h, 1, (C.c_int32 * 1)(member), 1, 0, 0, 20, 2, 0.0, mu.ctypes.data_as(vp),
                                                  cov.ctypes.data_as(vp), w.ctypes.data_as(vp), None, None,
                                                  n_it.ctypes.data_as(i32p), conv.ctypes.data_as(i32p))
        assert rc == -2 and "the voxel result has 4 members" in ctx.lib.hgmm_last_error(ctx.h).decode()
    ctx.voxel_down_sample_batch(scans[:1], VOXEL, download=False)
    with pytest.raises(HgmmError, match="stale voxel result"):
        ctx.flat_train_batch_voxels(vcs[:1], 2, 0.0, [params[0][0]], [params[0][1]], [params[0][2]])


def test_the_voxel_entry_without_a_result():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    try:
        p = [np.ascontiguousarray(a[None]) for a in init(1, 4)]
        n_it, conv = np.zeros(1, np.int32), np.zeros(1, np.int32)
        vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
        rc = c.lib.hgmm_flat_train_batch_voxels(c.h, 1, (C.c_int32 * 1)(0), 1, 0, 0, 4, 2, 0.0, p[0].ctypes.data_as(vp),
                                                p[1].ctypes.data_as(vp), p[2].ctypes.data_as(vp), None, None,
                                                n_it.ctypes.data_as(i32p), conv.ctypes.data_as(i32p))
        assert rc == -3 and "no voxel result" in c.lib.hgmm_last_error(c.h).decode()
    finally:
        c.close()


# ---- 10 ---------------------------------------------------------------------------------------------------------------
def same_tuple(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_train_gmm_batch_with_the_members_own_weights(ctx):
    import hgmm_amd
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    hgmm_amd.set_default_context(ctx)
    clouds = [cloud(110, 700), cloud(111, 1300), cloud(112, 64)]
    ws = [weights(700), weights(1300), None]
    params = [init(110 + i, 10) for i in range(3)]
    dev = W.asarray(clouds[0], ctx, weights=ws[0])
    members = [dev, WeightedPoints(clouds[1], ws[1]), clouds[2]]
    cols = [[p[k] for p in params] for k in range(3)]
    try:
        for mod, kw in ((W, dict(cov_type="diag")), (G, {})):
            got = mod.train_gmm_batch(members, 4, 0.0, *cols, sample_weight="own", **kw)
            for b in range(3):
                same_tuple(got[b], mod.train_gmm(clouds[b], 4, 0.0, *params[b], sample_weight=ws[b], **kw))
        # a sequence: an explicit array takes precedence over the member's own, None is the member's own
        other = 3 * weights(700)
        got = W.train_gmm_batch(members, 4, 0.0, *cols, sample_weight=[other, None, None])
        same_tuple(got[0], W.train_gmm(clouds[0], 4, 0.0, *params[0], sample_weight=other))
        same_tuple(got[1], W.train_gmm(clouds[1], 4, 0.0, *params[1], sample_weight=ws[1]))
        # the defaults still refuse
        with pytest.raises(ValueError, match="member 0 brings per-point weights"):
            W.train_gmm_batch(members, 4, 0.0, *cols)
        with pytest.raises(ValueError, match="member 0 brings per-point weights"):
            ctx.flat_train_batch([dev], 4, 0.0, *[c[:1] for c in cols])
        # J = 1025: the fall-back loops train_gmm(..., sample_weight=)
        big = [init(150 + i, 1025) for i in range(2)]
        got = W.train_gmm_batch(members[:2], 2, 0.0, *[[p[k] for p in big] for k in range(3)], sample_weight="own")
        for b in range(2):
            same_tuple(got[b], W.train_gmm(clouds[b], 2, 0.0, *big[b], sample_weight=ws[b]))
    finally:
        dev.free()


def models_equal(a, b):
    for name in ("means_", "covariances_", "weights_", "inv_covs"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert np.asarray(a.lls).tobytes() == np.asarray(b.lls).tobytes()


def test_fit_batch_of_voxel_clouds_is_the_loop_of_weighted_fits(ctx, scans):
    import hgmm_amd
    from hgmm_amd.gmm_waymo.gmm import GMM_GPU_Base
    from hgmm_amd.pointcloud_io import voxel_down_sample
    hgmm_amd.set_default_context(ctx)
    host = [voxel_down_sample(X, VOXEL, return_counts=True) for X in scans]
    np.random.seed(7)
    loop = [GMM_GPU_Base(12, max_iter=5, tol=1e-4).fit(cent, sample_weight=cnt) for cent, cnt in host]
    result = ctx.voxel_down_sample_batch(scans, VOXEL, download=False)
    np.random.seed(7)
    models = GMM_GPU_Base(12, max_iter=5, tol=1e-4).fit_batch(result.members())
    assert len(models) == 4
    for a, b in zip(models, loop):
        models_equal(a, b)
    with pytest.raises(ValueError, match="frame 1 is a VoxelCloud"):
        GMM_GPU_Base(12).fit_batch(result.members()[:2], sample_weight=[None, np.ones(len(result.member(1)), np.float32)])
    with pytest.raises(ValueError, match="VoxelClouds and other frames"):
        GMM_GPU_Base(12).fit_batch([result.member(0), scans[0]])


def test_fit_frames_down_sampled_in_chunks_of_four(ctx):
    from hgmm_amd.replicas import ReplicaPool, fit_frames
    frames = [np.random.RandomState(340 + i).rand(1500 + 101 * i, 3) for i in range(9)]       # 4 + 4 + 1
    with ReplicaPool(devices=[0]) as pool:
        np.random.seed(3)
        one = fit_frames(frames, n_components=8, max_iter=4, pool=pool, voxel_size=VOXEL)
        np.random.seed(3)
        four = fit_frames(frames, n_components=8, max_iter=4, pool=pool, batch=4, voxel_size=VOXEL)
        np.random.seed(3)
        plain = fit_frames(frames[:1], n_components=8, max_iter=4, pool=pool)
    assert len(four) == len(one) == 9
    for a, b in zip(four, one):
        models_equal(a, b)
    assert four[0].means_.tobytes() != plain[0].means_.tobytes()             # (the frames were down-sampled)
