"""Per-point weights of the SOURCE cloud in the tree build (hgmm_tree_set_source_weights[_batch]) on the GPU.

A source point i with weight w_i >= 0 counts as w_i points: the moments are sum w gamma (1, x, x x^T), pi = m0 / sum w and a
level's log-likelihood is sum w log(...); the partition and the 1e-15 floor do not see the weight.  The checks: the weighted
build against the float64 oracle (oracle.hgmm_tree.build_tree(w=...)) at the bounds the unweighted build is held to against
its oracle (tests/test_tree_gpu.py), on every driver path and in both precisions; w == 1 bitwise the unweighted build,
w == 2 with doubled ls / ld bitwise the unweighted tables with twice the q trace, NULL and a new cloud take the weights off;
integer weights are repetition; a zero weight is an absent point; a forest's members are bitwise their serial weighted
builds; count-weighted voxel centroids give a tree close to the full scan's; the mirrors; errors and state.

Clouds: 700 and 3 000 bunny points (neither a multiple of the 256-point workgroup), 200 003 points (the two-pass E-step with
two points per log-likelihood thread) and 401 111 points (four points per thread, the 2048-entry table)."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import hgmm_tree

from _tree_helpers import weights_for

pytestmark = pytest.mark.gpu

LS, LD, SIG2 = 20.0, 1e-4, 0.004
HGMM_ERR_ARG, HGMM_ERR_STATE = -2, -3          # include/hgmm.h
# the unweighted build against its oracle (tests/test_tree_gpu.py)
TOL = {"q": (1e-9, 1e-6), "pi": (1e-9, 1e-13), "mu": (1e-9, 1e-12), "cov": (1e-6, 1e-14)}


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def small_cloud(bunny, n, L, seed=5):
    """the clouds of tests/test_tree_source_weights_cpu.py (700 points then 3 000, one seeded generator) with T(L) initial
    means among the points: the CPU file's at the depth it uses (700: L = 2, 3 000: L = 3), a further draw otherwise"""
    rng = np.random.default_rng(seed)
    for m, depth in ((700, 2), (3000, 3)):
        X = bunny[rng.choice(len(bunny), m, replace=False)].astype(np.float64)
        rng.integers(1, 5, m)                                         # (the CPU file's integer weights)
        idx = rng.integers(0, m, hgmm_tree.n_total(depth))
        if m == n:
            if L != depth:
                idx = np.random.default_rng(seed + L).integers(0, m, hgmm_tree.n_total(L))
            return X, X[idx]
    raise KeyError(n)


def big_cloud(bunny, n, seed=3):
    """the bunny tiled with a seeded jitter, shuffled"""
    rs = np.random.RandomState(seed)
    reps = -(-n // len(bunny))
    X = np.tile(bunny.astype(np.float64), (reps, 1)) + 2e-4 * rs.randn(reps * len(bunny), 3)
    return np.ascontiguousarray(X[rs.permutation(len(X))[:n]])


def build(ctx, X, w, L, init_mu, ls=LS, ld=LD, iters=1000, want_leaf=True):
    """points first, then the weights (None: none), then the build -> (pi, mu, cov, leaf, iters, q)"""
    ctx.set_points(X)
    if w is not None:
        ctx.tree_set_source_weights(w)
    return ctx.tree_build(L, ls, ld, init_mu, SIG2, iters, want_leaf=want_leaf)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_close(got, ref, label, q_tol=TOL["q"]):
    """(pi, mu, cov, iters, q) of the GPU against the reference at TOL; prints the largest differences before it asserts"""
    names = ("pi", "mu", "cov")
    for name, a, b in zip(names, got[:3], ref[:3]):
        print("%s %s: largest |difference| %.3g (largest entry %.3g)" % (label, name, np.abs(np.asarray(a) - b).max(), np.abs(b).max()))
    print("%s iterations %s / %s" % (label, list(got[3]), list(ref[3])))
    assert list(got[3]) == list(ref[3]), label
    print("%s q: largest relative difference %.3g" % (label, (np.abs(got[4] - ref[4]) / np.abs(ref[4])).max()))
    np.testing.assert_allclose(got[4], ref[4], rtol=q_tol[0], atol=q_tol[1], err_msg=label)
    for name, a, b in zip(names, got[:3], ref[:3]):
        np.testing.assert_allclose(a, b, rtol=TOL[name][0], atol=TOL[name][1], err_msg="%s %s" % (label, name))


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. against the restatement, on every driver path
# ---------------------------------------------------------------------------------------------------------------------
RESTATED = {"700_L2": (700, 2, 1000), "3000_L3": (3000, 3, 1000), "3000_L4": (3000, 4, 6)}


@pytest.fixture(scope="module")
def restated(bunny):
    """the restatement's weighted builds, computed once: case -> (X, w, init_mu, L, iteration budget, (pi, mu, cov, iters, q))"""
    out = {}
    for case, (n, L, budget) in RESTATED.items():
        X, init_mu = small_cloud(bunny, n, L)
        w = weights_for(n)
        pi, mu, cov, tr = hgmm_tree.build_tree(X, L, LS, LD, None, SIG2, budget, w=w, init_mu=init_mu)
        margin = hgmm_tree.stop_margins(tr.q, tr.iters_per_level, LS)
        print("%s: iterations %s, smallest stop margin %.3g, %d dead nodes" % (case, list(tr.iters_per_level), margin.min(),
                                                                             int((pi == 0).sum())))
        assert margin.min() > 1e-6, case                              # (no stop decision within reach of rounding: else another seed)
        assert (w == 0).sum() > n // 20
        out[case] = (X, w, init_mu, L, budget, (pi, mu, cov, tr.iters_per_level, tr.q), margin.min())
    assert (out["3000_L3"][5][0] == 0).any()                          # dead nodes
    return out


@pytest.mark.parametrize("case", sorted(RESTATED))
def test_weighted_build_against_the_restatement(ctx, restated, case):
    """L = 3 reaches level 0's fused q, the log-likelihood kernels of levels 1 and 2 and dead nodes; L = 4 node tables beyond
    one 256-node LDS tile"""
    X, w, init_mu, L, budget, ref, _ = restated[case]
    pi, mu, cov, leaf, iters, q = build(ctx, X, w, L, init_mu, iters=budget)
    assert_close((pi, mu, cov, iters, q), ref, case)


PATHS = {"overlap_off": {"tree_overlap": 0}, "tickets": {"tree_tickets": 1}, "batch_scheme": {"tree_ahead": 0}}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_driver_path_against_the_restatement(ctx, restated, path):
    X, w, init_mu, L, budget, ref, _ = restated["3000_L3"]
    with ctx.config(**PATHS[path]):
        pi, mu, cov, leaf, iters, q = build(ctx, X, w, L, init_mu)
    assert_close((pi, mu, cov, iters, q), ref, path)


@pytest.mark.parametrize("path", ["default"] + sorted(PATHS))
def test_float32_pdf_mode(ctx, restated, path):
    """the E-step and the moments stay float64: with equal iteration counts the tables are the float64-mode weighted tables
    bit for bit; q stays within 1e-6 relative.  (The float32 pdfs move q by ~5e-8 relative, ~0.01 of ls here: the counts
    must agree when every stop decision of the restatement is further than 1e-3 ls from going the other way.)"""
    X, w, init_mu, L, budget, ref, margin = restated["3000_L3"]
    with ctx.config(**PATHS.get(path, {})):
        f64 = build(ctx, X, w, L, init_mu)
        ctx.tree_set_precision(np.float32)
        try:
            f32 = build(ctx, X, w, L, init_mu)
        finally:
            ctx.tree_set_precision(np.float64)
    print("%s: iterations %s / %s, q relative difference %.3g" % (path, list(f32[4]), list(f64[4]),
                                                                 (np.abs(f32[5] - f64[5]) / np.abs(f64[5])).max()
                                                                 if len(f32[5]) == len(f64[5]) else np.nan))
    if margin > 1e-3:
        assert list(f32[4]) == list(f64[4])
    if list(f32[4]) == list(f64[4]):
        for a, b in zip(f32[:4], f64[:4]):
            assert same_bits(a, b)
        assert_close((f32[0], f32[1], f32[2], f32[4], f32[5]), ref, path + " float32", q_tol=(1e-6, 0.0))
    else:                                                             # (the common part of the traces)
        k = min(len(f32[5]), len(ref[4]), int(min(f32[4][0], ref[3][0])))
        np.testing.assert_allclose(f32[5][:k], ref[4][:k], rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact properties
# ---------------------------------------------------------------------------------------------------------------------
def exact_properties(ctx, X, init_mu, L, ls, ld, iters, config):
    n = len(X)
    with ctx.config(**config):
        ref = build(ctx, X, None, L, init_mu, ls, ld, iters)
        one = build(ctx, X, np.ones(n), L, init_mu, ls, ld, iters)
        for a, b in zip(ref, one):                                    # tables, leaf_idx, iterations, q trace
            assert same_bits(a, b)
        two = build(ctx, X, np.full(n, 2.0), L, init_mu, 2 * ls, 2 * ld, iters)
        for a, b in zip(ref[:5], two[:5]):
            assert same_bits(a, b)
        assert same_bits(2.0 * ref[5], two[5])
        # NULL takes the weights off; so does a new cloud
        w = weights_for(n)
        other = build(ctx, X, w, L, init_mu, ls, ld, iters)
        assert not same_bits(other[0], ref[0])
        ctx.tree_set_source_weights(None)
        off = ctx.tree_build(L, ls, ld, init_mu, SIG2, iters)
        for a, b in zip(ref, off):
            assert same_bits(a, b)
        ctx.tree_set_source_weights(w)
        ctx.set_points(X)
        fresh = ctx.tree_build(L, ls, ld, init_mu, SIG2, iters)
        for a, b in zip(ref, fresh):
            assert same_bits(a, b)
    return ref


@pytest.mark.parametrize("path", ["default"] + sorted(PATHS))
def test_exact_properties_small_cloud(ctx, bunny, path):
    X, init_mu = small_cloud(bunny, 3000, 3)
    ref = exact_properties(ctx, X, init_mu, 3, LS, LD, 1000, PATHS.get(path, {}))
    assert ref[4].min() > 1


@pytest.fixture(scope="module")
def cloud_401111(bunny):
    X = big_cloud(bunny, 401111)
    return X, X[np.random.RandomState(72).randint(len(X), size=hgmm_tree.n_total(2))]


@pytest.mark.parametrize("precision", [np.float64, np.float32])
def test_exact_properties_large_cloud(ctx, cloud_401111, precision):
    """401 111 points, L = 2, ls = 0, three iterations per level: four points per log-likelihood thread, the 2048-entry
    table and the two-pass E-step"""
    X, init_mu = cloud_401111
    ctx.tree_set_precision(precision)
    try:
        ref = exact_properties(ctx, X, init_mu, 2, 0.0, LD, 3, {})
    finally:
        ctx.tree_set_precision(np.float64)
    assert list(ref[4]) == [3, 3]


# ---------------------------------------------------------------------------------------------------------------------
# 4. integer weights are repetition: against the existing unweighted build
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,top", [(200003, 3), (401111, 2)])
def test_integer_weights_are_repeated_points(ctx, bunny, n, top):
    X = big_cloud(bunny, n, seed=7)
    c = np.random.RandomState(13).randint(1, top + 1, n)
    init_mu = X[np.random.RandomState(72).randint(n, size=hgmm_tree.n_total(2))]
    pi, mu, cov, _, iters, q = build(ctx, X, c.astype(np.float64), 2, init_mu, 0.0, LD, 3, want_leaf=False)
    ref = build(ctx, np.repeat(X, c, axis=0), None, 2, init_mu, 0.0, LD, 3, want_leaf=False)
    assert c.sum() > 1.4 * n
    assert_close((pi, mu, cov, iters, q), (ref[0], ref[1], ref[2], ref[4], ref[5]), "n = %d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a zero weight is an absent point
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_weight_points_are_absent(ctx, bunny):
    """300 zero-weight points, half of them inside the cloud and half 10 units away (where every pdf underflows and the
    clamp keeps the logarithm finite): the build of the 3 000 points alone under the same weights"""
    X, init_mu = small_cloud(bunny, 3000, 3)
    w = weights_for(3000)
    rs = np.random.RandomState(4)
    extra = np.r_[X[rs.randint(3000, size=150)] + 1e-3 * rs.randn(150, 3), X[rs.randint(3000, size=150)] + 10.0]
    at = rs.permutation(3300)                                         # the absent points lie among the others
    Xa, wa = np.r_[X, extra][at], np.r_[w, np.zeros(300)][at]
    ref = build(ctx, X, w, 3, init_mu, 0.0, LD, 5)
    got = build(ctx, Xa, wa, 3, init_mu, 0.0, LD, 5)
    assert np.isfinite(got[5]).all()
    assert_close((got[0], got[1], got[2], got[4], got[5]), (ref[0], ref[1], ref[2], ref[4], ref[5]), "absent")
    # the present points go where they went (the tables differ by rounding: a point on a tie may not)
    assert (got[3][np.argsort(at)[:3000]] == ref[3]).mean() > 0.999


# ---------------------------------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [np.float64, np.float32])
def test_forest_members_are_their_serial_weighted_builds(ctx, bunny, precision):
    L, budget = 3, 25
    T = hgmm_tree.n_total(L)
    rng = np.random.default_rng(21)
    sizes = [1500, 255, 257, 1201, 2050]
    clouds = [bunny[rng.choice(len(bunny), n, replace=False)].astype(np.float64) for n in sizes]
    ws = [None if b in (0, 3) else weights_for(n, seed=30 + b) for b, n in enumerate(sizes)]
    init_mu = np.stack([X[rng.integers(0, len(X), T)] for X in clouds])
    ctx.tree_set_precision(precision)
    try:
        ctx.set_points_batch(clouds, weights=ws)
        (pi, mu, cov), iters, traces = ctx.tree_build_batch(sizes, L, LS, LD, init_mu, SIG2, budget, want_trace=True)
        for b, X in enumerate(clouds):
            s = build(ctx, X, ws[b], L, init_mu[b], iters=budget)
            assert same_bits(pi[b], s[0]) and same_bits(mu[b], s[1]) and same_bits(cov[b], s[2]), b
            assert list(iters[b]) == list(s[4]) and same_bits(traces[b], s[5]), b
            if ws[b] is None:                                         # ... which is the unweighted build (no weights resident)
                continue
            u = build(ctx, X, None, L, init_mu[b], iters=budget)
            assert not same_bits(u[0], s[0]), b
        # an all-None list runs the unweighted launches; None takes the weights off
        ctx.set_points_batch(clouds, weights=ws)
        ctx.tree_set_source_weights_batch([None] * len(clouds))
        plain = ctx.tree_build_batch(sizes, L, LS, LD, init_mu, SIG2, budget)
        ctx.tree_set_source_weights_batch(ws)
        ctx.tree_set_source_weights_batch(None)
        off = ctx.tree_build_batch(sizes, L, LS, LD, init_mu, SIG2, budget)
        ctx.set_points_batch(clouds)
        ref = ctx.tree_build_batch(sizes, L, LS, LD, init_mu, SIG2, budget)
        for got in (plain, off):
            assert all(same_bits(a, b) for a, b in zip(got[0], ref[0])) and same_bits(got[1], ref[1])
    finally:
        ctx.tree_set_precision(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# 7. what it buys
# ---------------------------------------------------------------------------------------------------------------------
def test_count_weighted_centroids_give_the_full_scans_tree(ctx, bunny):
    """bun000, L = 2, one explicit init_mu: the level-0 nodes of the tree of 4 mm voxel centroids against those of the full
    scan's tree, with the counts as weights and without (ls scaled by the point ratio, the best an unweighted caller can
    do).  Measured on the CPU restatement: 54x (pi) and 34x (mu) closer with the counts; iterations 36 / 51 against 36 / 46."""
    from hgmm_amd.pointcloud_io import voxel_down_sample
    P = bunny.astype(np.float64)
    cen, cnt = voxel_down_sample(P, 0.004, return_counts=True)
    init_mu = P[np.random.RandomState(72).randint(len(P), size=hgmm_tree.n_total(2))]
    full = build(ctx, P, None, 2, init_mu, want_leaf=False)
    wtd = build(ctx, cen, cnt.astype(np.float64), 2, init_mu, want_leaf=False)
    unw = build(ctx, cen, None, 2, init_mu, ls=LS * len(cen) / len(P), want_leaf=False)
    d = lambda t, k: np.abs(t[k][:8] - full[k][:8]).max()
    print("%d centroids for %d points; iterations full %s weighted %s unweighted %s" % (len(cen), len(P), list(full[4]),
                                                                                      list(wtd[4]), list(unw[4])))
    print("level 0 max|dpi| weighted %.3g unweighted %.3g; max|dmu| weighted %.3g unweighted %.3g" %
          (d(wtd, 0), d(unw, 0), d(wtd, 1), d(unw, 1)))
    assert 5 * d(wtd, 0) <= d(unw, 0) and 5 * d(wtd, 1) <= d(unw, 1)
    assert np.abs(np.asarray(wtd[4], int) - np.asarray(full[4], int)).max() <= 10


# ---------------------------------------------------------------------------------------------------------------------
# 8. mirrors end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_mirrors_end_to_end(ctx, bunny):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, WeightedPoints, buildGMMTree, registration_gmmtree, registration_gmmtree_batch
    from hgmm_amd.pointcloud_io import voxel_down_sample
    P = bunny.astype(np.float64)[::4]
    cen, cnt = voxel_down_sample(P, 0.006, return_counts=True)
    ref = buildGMMTree(cen, 2, LS, LD, ctx=ctx, weights=cnt)
    plain = buildGMMTree(cen, 2, LS, LD, ctx=ctx)
    assert not same_bits(ref[0], plain[0])
    gt = GMMTree(WeightedPoints(cen, cnt), tree_level=2, ctx=ctx)
    assert same_bits(gt._mixingCoeff, ref[0]) and same_bits(gt._mean, ref[1]) and same_bits(gt._covar, ref[2])
    gt = GMMTree(cen, tree_level=2, ctx=ctx, source_weights=cnt)
    assert same_bits(gt._mean, ref[1])
    gt.set_source(cen)                                                # the weights do not outlive their cloud
    assert same_bits(gt._mean, plain[1])
    th = 0.05
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    tgt = cen @ Rz.T + np.array([0.002, -0.001, 0.001])
    res = registration_gmmtree(cen, tgt, tree_level=2, ctx=ctx, source_weights=cnt, target_weights=cnt)
    gt2 = GMMTree(cen, tree_level=2, ctx=ctx, source_weights=cnt)
    want = gt2.registration(tgt, weights=cnt)
    assert same_bits(gt2._mean, ref[1])
    assert same_bits(res.transformation.rot, want.transformation.rot) and same_bits(res.transformation.t, want.transformation.t)
    other = registration_gmmtree(cen, tgt, tree_level=2, ctx=ctx, target_weights=cnt)
    assert not same_bits(other.transformation.t, res.transformation.t)
    # the batch mirror: pair 0 weighted, pair 1 not -- each the serial call's result
    out = registration_gmmtree_batch([(WeightedPoints(cen, cnt), tgt), (cen, tgt)], tree_level=2, ctx=ctx,
                                     target_weights=[cnt, cnt])
    assert same_bits(out[0].transformation.rot, res.transformation.rot) and same_bits(out[0].transformation.t, res.transformation.t)
    assert same_bits(out[1].transformation.rot, other.transformation.rot) and same_bits(out[1].transformation.t, other.transformation.t)


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors and state
# ---------------------------------------------------------------------------------------------------------------------
def _dptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_errors_and_state(bunny):
    import hgmm_amd
    from hgmm_amd import HgmmError
    X, init_mu = small_cloud(bunny, 700, 2)
    n = len(X)
    w = weights_for(n)
    c = hgmm_amd.Context(0)
    try:
        lib, h = c.lib, c.h
        ones = np.ones(n)
        # no cloud: HGMM_ERR_STATE from both entries, also for NULL
        assert lib.hgmm_tree_set_source_weights(h, _dptr(ones), n) == HGMM_ERR_STATE
        assert lib.hgmm_tree_set_source_weights(h, None, 0) == HGMM_ERR_STATE
        ptrs = (ctypes.c_void_p * 1)(ones.ctypes.data)
        cnts = (ctypes.c_int64 * 1)(n)
        assert lib.hgmm_tree_set_source_weights_batch(h, 1, ptrs, cnts) == HGMM_ERR_STATE
        with pytest.raises(HgmmError, match="no cloud"):
            c.tree_set_source_weights(ones)
        c.set_points(X)
        # a serial cloud is not a forest cloud
        assert lib.hgmm_tree_set_source_weights_batch(h, 1, ptrs, cnts) == HGMM_ERR_STATE
        ref_w = c.tree_set_source_weights(w).tree_build(2, LS, LD, init_mu, SIG2)
        bad = {"length": (ones[:-1], b"700"), "negative": (np.r_[ones[:-1], -1e-3], b"699"), "nan": (np.r_[np.nan, ones[1:]], b" 0 "),
               "infinite": (np.r_[ones[:5], np.inf, ones[6:]], b" 5 "), "all zero": (np.zeros(n), b"zero")}
        for name, (v, word) in bad.items():
            v = np.ascontiguousarray(v)
            assert lib.hgmm_tree_set_source_weights(h, _dptr(v), len(v)) == HGMM_ERR_ARG, name
            msg = lib.hgmm_last_error(h)
            assert b"hgmm_tree_set_source_weights" in msg and word in msg, (name, msg)
            with pytest.raises(HgmmError):
                c.tree_set_source_weights(v)
        with pytest.raises(ValueError):
            c.tree_set_source_weights(np.ones((n, 1)))
        # the previous weights survived every refused upload
        again = c.tree_build(2, LS, LD, init_mu, SIG2)
        assert all(same_bits(a, b) for a, b in zip(ref_w, again))
        # whatever changes the resident cloud drops them
        ref = c.set_points(X).tree_build(2, LS, LD, init_mu, SIG2)
        assert not same_bits(ref[0], ref_w[0])
        c.tree_set_source_weights(w)
        c.set_points(X.astype(np.float32))
        c.set_points(X)
        assert all(same_bits(a, b) for a, b in zip(ref, c.tree_build(2, LS, LD, init_mu, SIG2)))
        hd = c.points_create(X)
        c.tree_set_source_weights(w)
        c.points_bind(hd)
        assert all(same_bits(a, b) for a, b in zip(ref, c.tree_build(2, LS, LD, init_mu, SIG2)))
        c.tree_set_source_weights(w)                                  # weights on the bound handle's view
        assert all(same_bits(a, b) for a, b in zip(ref_w, c.tree_build(2, LS, LD, init_mu, SIG2)))
        c.points_destroy(hd)
        with pytest.raises(HgmmError):
            c.tree_set_source_weights(w)                              # no cloud again
        c.set_points(X)
        c.tree_set_source_weights(w)
        c.set_points_batch([X[:300], X[300:]])                        # (the same 700 points as one resident cloud)
        assert all(same_bits(a, b) for a, b in zip(ref, c.tree_build(2, LS, LD, init_mu, SIG2)))
        # the batch entry's own checks
        sizes = [300, 400]
        c.set_points_batch([X[:300], X[300:]])
        ws = [w[:300], w[300:]]
        im = np.stack([init_mu, init_mu])
        ref_b = c.tree_set_source_weights_batch(ws).tree_build_batch(sizes, 2, LS, LD, im, SIG2)

        def raw(ws_, counts):
            p = (ctypes.c_void_p * len(ws_))(*[None if v is None else v.ctypes.data for v in ws_])
            return lib.hgmm_tree_set_source_weights_batch(h, len(ws_), p, (ctypes.c_int64 * len(counts))(*counts))
        assert raw(ws, [300, 400]) == 0
        assert raw(ws[:1], [300]) == HGMM_ERR_ARG
        assert raw(ws, [300, 399]) == HGMM_ERR_ARG
        neg = np.ascontiguousarray(np.r_[w[300:699], -1.0])
        assert raw([ws[0], neg], [300, 400]) == HGMM_ERR_ARG
        msg = lib.hgmm_last_error(h)
        assert b"cloud 1" in msg and b"399" in msg, msg
        assert raw([ws[0], np.zeros(400)], [300, 400]) == HGMM_ERR_ARG
        with pytest.raises(HgmmError):
            c.tree_set_source_weights_batch([ws[0], None, ws[1]])
        again = c.tree_build_batch(sizes, 2, LS, LD, im, SIG2)        # the previous weights are still in force
        assert all(same_bits(a, b) for a, b in zip(again[0], ref_b[0])) and same_bits(again[1], ref_b[1])
        # the build refuses weights that were set for other cloud sizes
        with pytest.raises(HgmmError, match="other cloud sizes"):
            c.tree_build_batch([350, 350], 2, LS, LD, im, SIG2)
    finally:
        c.close()


def _rank_worker(rank, name, q):
    try:
        import hgmm_amd
        bunny = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
        X, init_mu = small_cloud(bunny, 700, 2)
        lo, hi = (0, 350) if rank == 0 else (350, 700)
        ctx = hgmm_amd.Context(0)
        ctx.comm_init_host(2, rank, name)
        ctx.set_points(X[lo:hi])
        ctx.tree_set_source_weights(np.ones(hi - lo))
        try:
            ctx.tree_build(2, LS, LD, init_mu, SIG2, 5, want_leaf=False)
            msg = "the weighted build ran"
        except hgmm_amd.HgmmError as e:
            msg = str(e)
        # without the weights the sharded build runs as before
        ctx.tree_set_source_weights(None)
        iters = ctx.tree_build(2, LS, LD, init_mu, SIG2, 5, want_leaf=False)[4]
        ctx.close()
        q.put((rank, (msg, [int(v) for v in iters])))
    except BaseException as e:                              # the parent must not wait out its timeout for a dead rank
        import traceback
        q.put((rank, "rank %d failed: %r\n%s" % (rank, e, traceback.format_exc())))
        raise


def test_weighted_build_under_a_communicator_is_refused():
    """both ranks refuse before they enqueue a collective: nobody waits for anybody"""
    name = "hgmm_sw_%d" % os.getpid()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_rank_worker, args=(r, name, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
    assert not any(isinstance(v, str) for v in got.values()), got
    assert all(p.exitcode == 0 for p in procs)
    for rank in (0, 1):
        msg, iters = got[rank]
        assert "(%d)" % HGMM_ERR_STATE in msg and "communicator" in msg and "weights" in msg, got[rank]
        assert len(iters) == 2 and min(iters) >= 1
    assert got[0][1] == got[1][1]
