"""Multi-start registration (hgmm_tree_register_multi / hgmm_tree_score_multi, GMMTree.registration_multistart): K start
poses of ONE pair in the launches of one, on the resident tree and target.

The registration moments are 64-bit fixed-point integer sums and the score's shares are added in a fixed order, so the bar
for every hypothesis is ``np.array_equal`` with the serial entry from that start: pose, iteration count, status, q and the
whole per-iteration trace.  What the serial entry itself is held to (the float64 oracle, the reference's records) is in
tests/test_tree_gpu.py and tests/test_tree_reg_depth_gpu.py; the identity hypothesis repeats the records' 1e-8 here.

Numbers the recovery test leans on, from the float64 oracle (oracle/hgmm_tree.py, normal-equation form) on
tests/golden/hgmm_reg_L4.npz, target rot30_target, the 27-start grid of rotation_starts(), maxiter 30, tol 1e-4: 5 of the
27 starts end at fitness 0.937 and at most 1.3 mm from ``points`` (after 12, 17, 23, 23 and 25 iterations); the best of the
other 22 ends at fitness 0.55, about 5.5 cm off; the identity start (index 13) at 0.549."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from test_tree_reg_depth_gpu import LC, ctx, moved, rot_about, synthetic_target, synthetic_tree  # noqa: F401
from test_tree_score_gpu import CHI2

pytestmark = pytest.mark.gpu

I3, Z3 = np.identity(3), np.zeros(3)
HGMM_ERR_ARG = -2                     # include/hgmm.h


def five_starts(centre):
    """the identity and +-10 degrees about two axes, each about ``centre``"""
    rots = [I3, rot_about([1, 0, 0], 10), rot_about([1, 0, 0], -10), rot_about([0, 0, 1], 10), rot_about([0, 0, 1], -10)]
    return np.stack(rots), np.stack([centre - R @ centre for R in rots])


def grid_starts():
    from hgmm_amd.hgmm.hgmm_gpu import rotation_starts
    s = rotation_starts()
    return np.stack([p.rot for p in s]), np.stack([p.t for p in s])


def assert_multi_is_serial(ctx, rot0, t0, lc, maxiter, tol, label):
    """One multi call == K serial calls on the resident tree and target, bit for bit.  -> the multi call's results"""
    K = len(rot0)
    m_rot, m_t, m_it, m_q, m_st, m_tr = ctx.tree_register_multi(rot0, t0, 1.0, lc, maxiter, tol, want_trace=True)
    assert m_rot.shape == (K, 3, 3) and m_t.shape == (K, 3) and len(m_tr) == K
    for k in range(K):
        s_rot, s_t, s_it, s_q, s_st, s_tr = ctx.tree_register(rot0[k], t0[k], 1.0, lc, maxiter, tol, None, want_trace=True)
        what = "%s, hypothesis %d" % (label, k)
        assert (int(m_it[k]), int(m_st[k])) == (s_it, s_st), what
        assert np.array_equal(m_rot[k], s_rot) and np.array_equal(m_t[k], s_t), what
        assert (np.isnan(m_q[k]) and s_q is None) or m_q[k] == s_q, what
        assert m_tr[k].shape == (s_it, 13) and np.array_equal(m_tr[k], s_tr), what
    return m_rot, m_t, m_it, m_q, m_st, m_tr


@pytest.fixture(scope="module")
def records():
    return {2: load_golden("hgmm_reg_L2.npz"), 4: load_golden("hgmm_reg_L4.npz")}


# ---------------------------------------------------------------------------------------------------------------------
# 1. bitwise the serial call: the reference's L = 2 and L = 4 records, synthetic trees at L = 5 and 6
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
def test_multi_is_bitwise_serial_on_the_reference_records(ctx, records, L):
    g = records[L]
    lc = float(g["lambda_c"])
    assert int(g["L"]) == L
    target = g["rot10_target"]
    assert len(target) == {2: 2013, 4: 5032}[L]
    ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(target)
    rot0, t0 = five_starts(target.mean(axis=0))
    n_rec = len(g["rot10_iter_rot"])
    _, _, iters, _, _, traces = assert_multi_is_serial(ctx, rot0, t0, lc, n_rec, 1e-4, "record L=%d" % L)
    # the identity hypothesis against the reference's recorded per-iteration (R, t) (stored as inverses)
    assert iters[0] == n_rec
    for k in range(n_rec):
        r_k, t_k = traces[0][k, :9].reshape(3, 3), traces[0][k, 9:12]
        np.testing.assert_allclose(r_k.T, g["rot10_iter_rot"][k], rtol=0, atol=1e-8)
        np.testing.assert_allclose(-(r_k.T @ t_k), g["rot10_iter_t"][k], rtol=0, atol=1e-8)
    # K = 1
    assert_multi_is_serial(ctx, rot0[3:4], t0[3:4], lc, 7, 1e-4, "record L=%d, K=1" % L)


@pytest.mark.parametrize("L,seed", [(5, 15), (6, 16)])
def test_multi_is_bitwise_serial_on_deep_synthetic_trees(ctx, L, seed):
    pi, mu, cov, live = synthetic_tree(L, seed)
    X = synthetic_target(pi, mu, cov, live, L, 3000, seed)
    target = moved(X, 3.0, [0.2, 1.0, 0.4], [0.01, -0.005, 0.008])
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(target)
    rot0, t0 = five_starts(target[:3000].mean(axis=0))
    _, _, iters, _, _, _ = assert_multi_is_serial(ctx, rot0, t0, LC, 6, 1e-6, "synthetic L=%d" % L)
    assert iters.max() > 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. a partial chunk, an exact chunk, one point over
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 256, 257])
def test_multi_small_targets(ctx, records, n):
    g = records[2]
    ctx.tree_set_nodes(2, g["pi"], g["mu"], g["cov"])
    target = g["rot10_target"][:n]
    ctx.tree_set_target(target)
    rot0, t0 = five_starts(target.mean(axis=0))
    assert_multi_is_serial(ctx, rot0, t0, float(g["lambda_c"]), 6, 1e-6, "%d points" % n)
    sums = ctx.tree_score_multi(rot0, t0, 1.0, float(g["lambda_c"]), CHI2)
    for k in range(len(rot0)):
        assert np.array_equal(sums[k], ctx.tree_score(rot0[k], t0[k], 1.0, float(g["lambda_c"]), CHI2, want=())[0]), (n, k)
    assert (sums[:, 0] == n).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. hypotheses that stop at different iterations inside one call
# ---------------------------------------------------------------------------------------------------------------------
def test_multi_grid_with_different_stop_iterations(ctx, records):
    g = records[4]
    ctx.tree_set_nodes(4, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(g["rot30_target"])
    rot0, t0 = grid_starts()
    _, _, iters, _, status, _ = assert_multi_is_serial(ctx, rot0, t0, float(g["lambda_c"]), 30, 1e-4, "27-start grid")
    print("iterations:", iters.tolist(), "status:", status.tolist())
    assert len(set(iters.tolist())) > 1
    assert (status == 1).sum() >= 2 and len(set(iters[status == 1].tolist())) > 1     # stops by tol, at different iterations


# ---------------------------------------------------------------------------------------------------------------------
# 4. the score of K poses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
def test_score_multi_is_bitwise_the_serial_score(ctx, records, L):
    g = records[L]
    lc = float(g["lambda_c"])
    ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(g["rot30_target"])
    rot0, t0 = grid_starts()
    rot, t, _, _, _, _ = ctx.tree_register_multi(rot0, t0, 1.0, lc, 4, 1e-4)
    for poses in ((rot0, t0), (rot, t)):
        sums = ctx.tree_score_multi(poses[0], poses[1], 1.0, lc, CHI2)
        assert sums.shape == (27, 8)
        for k in range(27):
            assert np.array_equal(sums[k], ctx.tree_score(poses[0][k], poses[1][k], 1.0, lc, CHI2, want=())[0]), k
        assert np.array_equal(sums, ctx.tree_score_multi(poses[0], poses[1], 1.0, lc, CHI2))
    # (another inlier bound and the descent without its stop rule)
    sums = ctx.tree_score_multi(rot[:3], t[:3], 1.0, -1.0, 4.0)
    for k in range(3):
        assert np.array_equal(sums[k], ctx.tree_score(rot[k], t[k], 1.0, -1.0, 4.0, want=())[0]), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. the loop on the device alone
# ---------------------------------------------------------------------------------------------------------------------
def test_multi_with_the_solve_on_the_device(ctx, records):
    g = records[4]
    ctx.tree_set_nodes(4, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(g["rot30_target"])
    rot0, t0 = grid_starts()                 # (the whole grid: five of its starts converge before the budget, see above)
    with ctx.config(reg_device_solve=1):
        _, _, iters, _, status, _ = assert_multi_is_serial(ctx, rot0, t0, float(g["lambda_c"]), 30, 1e-4, "device solve")
    print("device solve, iterations:", iters.tolist(), "status:", status.tolist())
    assert len(set(iters.tolist())) > 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. the documented failure becomes a success, through the public API
# ---------------------------------------------------------------------------------------------------------------------
def test_multistart_recovers_the_30_degree_record(ctx, records):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, MultiStartResult, ScoredResult, registration_gmmtree, rotation_starts
    g = records[4]
    target, points = g["rot30_target"], g["points"]
    gt = GMMTree(None, tree_level=4, lambda_c=float(g["lambda_c"]), ctx=ctx)
    gt.set_nodes(g["pi"], g["mu"], g["cov"])
    win, every = gt.registration_multistart(target, rotation_starts(), maxiter=30, return_all=True)
    fit = [r.score.fitness for r in every]
    off = [np.abs(r.transformation.inverse().transform(target) - points).max() for r in every]
    print("winner %d after %d iterations: fitness %.4f, %.2f mm off; identity start: fitness %.4f; fitness of all: %s"
          % (win.best_index_, win.n_iter_, win.score.fitness, 1e3 * off[win.best_index_], fit[13], np.round(fit, 3).tolist()))
    assert isinstance(win, ScoredResult) and isinstance(win, MultiStartResult) and len(every) == 27
    assert win.best_index_ != 13 and gt.best_index_ == win.best_index_ and gt.n_iter_ == win.n_iter_
    assert every[win.best_index_] is win
    assert win.score.fitness >= 0.9
    assert off[win.best_index_] <= 3e-3
    assert fit[13] < 0.7
    # only the winner carries the per-point arrays
    assert win.score.node.shape == (len(target),) and win.score.maha2.shape == (len(target),)
    assert all(r.score.node is None for k, r in enumerate(every) if k != win.best_index_)
    assert win.score.n_inliers == max(r.score.n_inliers for r in every)
    # without return_all: the same winner, bit for bit
    again = gt.registration_multistart(target, rotation_starts(), maxiter=30)
    assert again.best_index_ == win.best_index_ and np.array_equal(again.transformation.rot, win.transformation.rot)
    assert np.array_equal(again.transformation.t, win.transformation.t) and again.score.fitness == win.score.fitness
    # the one-call form (builds its own, shallow tree)
    res = registration_gmmtree(points, target, maxiter=10, starts=rotation_starts((-15, 15)), tree_level=2, ctx=ctx)
    assert isinstance(res, ScoredResult) and 0 <= res.best_index_ < 8 and res.score.n_points == len(target)


# ---------------------------------------------------------------------------------------------------------------------
# 7. a hypothesis whose normal equations are singular leaves the call (status 2) and is finished on the host path
# ---------------------------------------------------------------------------------------------------------------------
def test_ill_conditioned_hypothesis_leaves_and_is_finished_serially(ctx, bunny):
    """tests/test_tree_batch_gpu.py makes a pair singular with a one-level tree and a target of ONE point (one node with
    mass: rank 3).  A start pose with R = 0 and t = that point does the same to ONE hypothesis: it moves every target point
    onto the one point."""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, RigidTransformation
    b = bunny.astype(np.float64)
    src = b[::10]
    target = moved(src, 4.0, [0, 1, 0], [0.001, 0.001, 0.0])
    kw = dict(tree_level=1, lambda_c=0.01, ls=20, sig2=0.004)
    gt = GMMTree(src, ctx=ctx, **kw)
    c = target.mean(axis=0)
    R1 = rot_about([0, 0, 1], 5)
    rot0 = np.stack([I3, np.zeros((3, 3)), R1])
    t0 = np.stack([Z3, src[0] + 0.001, c - R1 @ c])
    ctx.tree_set_nodes(1, gt._mixingCoeff, gt._mean, gt._covar)
    ctx.tree_set_target(target)
    _, _, iters, _, status, _ = assert_multi_is_serial(ctx, rot0, t0, 0.01, 6, 1e-6, "one singular hypothesis")
    assert status[1] == 2 and iters[1] == 0
    assert status[0] != 2 and status[2] != 2 and iters[0] > 0 and iters[2] > 0
    # through the mirror: every hypothesis is what the serial mirror gives from that start
    starts = [RigidTransformation(rot0[k], t0[k]) for k in range(3)]
    win, every = gt.registration_multistart(target, starts, maxiter=6, tol=1e-6, return_all=True)
    for k in range(3):
        ref = GMMTree(None, ctx=ctx, **kw)
        ref.set_nodes(gt._mixingCoeff, gt._mean, gt._covar)
        ctx.tree_set_nodes(1, gt._mixingCoeff, gt._mean, gt._covar)
        ctx.tree_set_target(target)
        ref._tf_result = starts[k]
        r = ref._registration_in_library(6, 1e-6)
        assert np.array_equal(r.transformation.rot, every[k].transformation.rot), k
        assert np.array_equal(r.transformation.t, every[k].transformation.t), k
        assert np.array_equal(np.ravel(r.q), np.ravel(every[k].q)), k
        if k == win.best_index_:
            assert ref.n_iter_ == win.n_iter_
    assert np.isfinite(every[1].transformation.t).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. neither the serial entries' sums nor a resident forest are disturbed
# ---------------------------------------------------------------------------------------------------------------------
def test_multi_leaves_the_serial_state_and_a_forest_alone(ctx, records, bunny):
    from oracle import hgmm_tree
    g = records[2]
    lc = float(g["lambda_c"])
    b = bunny.astype(np.float64)
    clouds = [b[::40], b[5::50]]
    T = hgmm_tree.n_total(2)
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch(clouds)
    ctx.tree_build_batch([len(a) for a in arrs], 2, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch([moved(c, 5.0, [0, 0, 1], [0.002, 0.0, 0.001]) for c in clouds])
    forest = lambda: ctx.tree_register_batch(np.tile(I3, (2, 1, 1)), np.zeros((2, 3)), 1.0, 0.01, 8, 1e-6, want_trace=True)
    f_before = forest()
    fs_before = ctx.tree_score_batch(f_before[0], f_before[1], 1.0, 0.01)

    ctx.tree_set_nodes(2, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(g["rot10_target"])
    serial = lambda: ctx.tree_register(I3, Z3, 1.0, lc, 8, 1e-6, None, want_trace=True)
    s_before = serial()
    m_before = ctx.tree_reg_estep(T, I3, Z3, 1.0, lc)         # (leaves its [T][10] sums behind in the serial buffer)
    rot0, t0 = grid_starts()
    first = ctx.tree_register_multi(rot0, t0, 1.0, lc, 8, 1e-6, want_trace=True)
    ctx.tree_score_multi(first[0], first[1], 1.0, lc, CHI2)
    s_after = serial()
    for x, y in zip(s_before, s_after):
        assert np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    for x, y in zip(m_before, ctx.tree_reg_estep(T, I3, Z3, 1.0, lc)):
        assert np.array_equal(x, y)
    # a second multi call, of fewer hypotheses, after the serial ones: the same bits as in the first
    second = ctx.tree_register_multi(rot0[:9], t0[:9], 1.0, lc, 8, 1e-6, want_trace=True)
    for x, y in zip(first[:5], second[:5]):
        assert np.array_equal(x[:9], y)
    assert all(np.array_equal(x, y) for x, y in zip(first[5][:9], second[5]))
    # the forest registers and scores as before
    f_after = forest()
    for x, y in zip(f_before[:5], f_after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(f_before[5], f_after[5]))
    assert np.array_equal(fs_before, ctx.tree_score_batch(f_before[0], f_before[1], 1.0, 0.01))


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_multi_errors_name_their_cause():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    try:
        pi, mu, cov, live = synthetic_tree(1, 11)
        X = synthetic_target(pi, mu, cov, live, 1, 500, 11)
        R, t = np.tile(I3, (2, 1, 1)), np.zeros((2, 3))
        for call in (c.tree_register_multi, c.tree_score_multi):
            with pytest.raises(hgmm_amd.HgmmError, match="(?i)no tree"):
                call(R, t)
        c.tree_set_nodes(1, pi, mu, cov)
        for call in (c.tree_register_multi, c.tree_score_multi):
            with pytest.raises(hgmm_amd.HgmmError, match="(?i)no target"):
                call(R, t)
        c.tree_set_target(X)
        for call in (c.tree_register_multi, c.tree_score_multi):
            with pytest.raises(hgmm_amd.HgmmError, match="K = 0"):
                call(np.zeros((0, 3, 3)), np.zeros((0, 3)))
        with pytest.raises(hgmm_amd.HgmmError, match="NaN"):
            c.tree_score_multi(R, t, maha2_max=float("nan"))
        # NULL rot, straight through the C ABI: the code and the text
        q, it, st, out = np.full(2, np.nan), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros((2, 8))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = c.lib.hgmm_tree_register_multi(c.h, 2, None, p(t), 1.0, 0.01, 5, 1e-4, p(q), p(it), p(st), None)
        assert rc == HGMM_ERR_ARG and b"rot" in c.lib.hgmm_last_error(c.h)
        rc = c.lib.hgmm_tree_score_multi(c.h, 2, None, p(t), 1.0, 0.01, CHI2, p(out))
        assert rc == HGMM_ERR_ARG and b"rot" in c.lib.hgmm_last_error(c.h)
        rc = c.lib.hgmm_tree_register_multi(c.h, 2, p(R), p(t), 1.0, 0.01, 5, 1e-4, p(q), None, p(st), None)
        assert rc == HGMM_ERR_ARG and b"NULL" in c.lib.hgmm_last_error(c.h)
        rc = c.lib.hgmm_tree_score_multi(c.h, 2, p(R), p(t), 1.0, 0.01, CHI2, None)
        assert rc == HGMM_ERR_ARG and b"summary_out" in c.lib.hgmm_last_error(c.h)
        # and the context still works
        rot, tt, iters, _, status, _ = c.tree_register_multi(R, t, 1.0, 0.01, 3, 1e-6)
        assert (iters > 0).all() or (status == 2).all()
        assert (c.tree_score_multi(rot, tt)[:, 0] == len(X)).all()
    finally:
        c.close()
