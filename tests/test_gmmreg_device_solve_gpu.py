"""The device BFGS solve of the L2 GMMReg path (hgmm_l2_solve, csrc/gmmreg_l2_kernels.hip + csrc/l2_device.h): bit for bit
the written-down arithmetic (tests/_l2_solve_model.py, given ``Context.l2_cost`` at R = 1 as its evaluator), independent of
its neighbours, its position and the context's history; the mirrors built on it (``RigidCostFunction.solve_many``,
``solver="device"``) against the reference and against themselves."""
import ctypes

import numpy as np
import pytest

import _l2_solve_cases as cases
import _l2_solve_model as model
import l2_scenario as l2s

pytestmark = pytest.mark.gpu

MAX_ITER, GTOL = 10, 1.0e-5
KEYS = ("x", "f", "grad", "nit", "nfev", "status")


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    return hgmm_amd.default_context()


def _device_evaluator(ctx):
    """the model's evaluator: the 13 sums of hgmm_l2_cost at R = 1 on the context's resident pairs"""
    def evaluate(pose, pair, sigma):
        return ctx.l2_cost([pair], [np.array(pose[0]).reshape(3, 3)], [np.array(pose[1])], sigma)[0]
    return evaluate


def _row(out, r):
    """hypothesis r of a ``Context.l2_solve`` result, in the model's form"""
    x, f, grad, nit, nfev, status = out
    return {"x": x[r], "f": f[r], "grad": grad[r], "nit": int(nit[r]), "nfev": int(nfev[r]), "status": int(status[r])}


def _differences(a, b):
    return [k for k in KEYS if not np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                                                  equal_nan=True)]


def _ragged_pairs(rs):
    """the pairs of tests/test_gmmreg_resident_gpu.py -- together they cross the 64-centre source block and the 256-centre
    target split -- and (1, 1)"""
    return [(rs.rand(js, 3), 0.1 + rs.rand(js), rs.rand(jt, 3), 0.1 + rs.rand(jt))
            for js, jt in ((30, 25), (70, 300), (5, 129), (200, 64), (1, 1))]


@pytest.fixture(scope="module")
def ragged(ctx):
    """R = 40 random hypotheses on the ragged pairs, each solved once by the model over ``l2_cost`` (shared, never modified)"""
    rs = np.random.RandomState(17)
    pairs = _ragged_pairs(rs)
    R = 40
    ids = rs.randint(len(pairs), size=R)
    ids[:5] = np.arange(5)                                             # (every pair at least once)
    thetas = np.concatenate([rs.randn(R, 4), rs.uniform(-0.2, 0.2, (R, 3))], axis=1)
    for r in range(R):                                                 # unit quaternions about the cube's centre: the mixtures overlap
        thetas[r, :4] /= np.linalg.norm(thetas[r, :4])
        rot = np.array(model.quat_terms([float(v) for v in thetas[r, :4]])[0]).reshape(3, 3)
        thetas[r, 4:] += 0.5 - rot @ np.full(3, 0.5)
    sigmas = rs.uniform(0.1, 0.4, R)
    ctx.l2_set_pairs(pairs)
    evaluate = _device_evaluator(ctx)
    want = [model.solve(evaluate, thetas[r], int(ids[r]), float(sigmas[r]), MAX_ITER, GTOL) for r in range(R)]
    return pairs, ids, thetas, sigmas, want


def test_bitwise_the_model_at_R_1_and_R_40_and_independent_of_position(ctx, ragged):
    pairs, ids, thetas, sigmas, want = ragged
    R = len(ids)
    ctx.l2_set_pairs(pairs)
    many = ctx.l2_solve(ids, thetas, sigmas, MAX_ITER, GTOL)
    print("status %s" % many[5].tolist())
    print("nit %s\nnfev %s" % (many[3].tolist(), many[4].tolist()))
    assert len(set(many[4].tolist())) > 1                                            # (the hypotheses do differ in length)
    for r in range(R):
        assert not _differences(_row(many, r), want[r]), (r, _differences(_row(many, r), want[r]), _row(many, r), want[r])
    for r in range(R):                                                               # every hypothesis is its own R = 1 call
        alone = ctx.l2_solve([ids[r]], [thetas[r]], sigmas[r], MAX_ITER, GTOL)
        assert not _differences(_row(alone, 0), want[r]), (r, _differences(_row(alone, 0), want[r]))
    # a second call, the hypotheses permuted
    perm = np.random.RandomState(3).permutation(R)
    again = ctx.l2_solve(ids[perm], thetas[perm], sigmas[perm], MAX_ITER, GTOL)
    for at, r in enumerate(perm):
        assert not _differences(_row(again, at), want[r]), (at, r)


@pytest.fixture(scope="module")
def scenario(ctx):
    sc, pair, thetas = cases.scenario_jobs()
    return sc, pair, thetas


def test_unequal_lengths_in_one_call(ctx, scenario):
    sc, pair, thetas = scenario
    ctx.l2_set_pairs([pair])
    sigma = sc["sigma"]
    ended = ctx.l2_solve([0], [thetas[14]], sigma, l2s.OPT_MAXITER, l2s.OPT_TOL)[0][0]
    jobs = [(ended, 10, 1e30),                              # starts where a solve ended; any gradient meets gtol
            (thetas[0], 1, l2s.OPT_TOL),                    # one iteration
            (thetas[0], l2s.OPT_MAXITER, l2s.OPT_TOL),      # start 0 of the scenario: its line search fails
            (np.zeros(7), l2s.OPT_MAXITER, l2s.OPT_TOL)]    # the quaternion (0, 0, 0, 0)
    x0 = np.stack([j[0] for j in jobs])
    out = ctx.l2_solve([0] * 4, x0, sigma, [j[1] for j in jobs], [j[2] for j in jobs])
    print("status %s nit %s nfev %s" % (out[5].tolist(), out[3].tolist(), out[4].tolist()))
    assert out[5].tolist() == [0, 1, 2, 3]
    assert (out[3][0], out[4][0]) == (0, 1) and out[3][1] == 1 and (out[3][3], out[4][3]) == (0, 1)
    assert np.array_equal(out[0][0], ended)
    evaluate = _device_evaluator(ctx)
    for r, (th, max_iter, gtol) in enumerate(jobs):
        want = model.solve(evaluate, th, 0, sigma, max_iter, gtol)
        assert not _differences(_row(out, r), want), (r, _differences(_row(out, r), want), _row(out, r), want)
        alone = ctx.l2_solve([0], [th], sigma, max_iter, gtol)
        assert not _differences(_row(alone, 0), want), r


def test_non_unit_quaternion_is_bitwise_the_model(ctx, scenario):
    """The reference's Jacobian quirks only show off the unit sphere."""
    sc, pair, thetas = scenario
    ctx.l2_set_pairs([pair])
    th = thetas[3].copy()
    th[:4] *= 1.7
    out = ctx.l2_solve([0], [th], sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL)
    want = model.solve(_device_evaluator(ctx), th, 0, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL)
    print("nit %d nfev %d status %d" % (want["nit"], want["nfev"], want["status"]))
    assert want["nit"] >= 1
    assert not _differences(_row(out, 0), want), (_differences(_row(out, 0), want), _row(out, 0), want)


def test_scenario_nit_and_status_are_scipys_and_the_winner_is_start_14(ctx, scenario):
    """The 28 solves on the device against SciPy on the host cost, with the CPU test's yardstick."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    sc, pair, thetas = scenario
    cost = cf.RigidCostFunction(ctx=ctx)
    cost.set_pairs([pair])
    res = cost.solve_many(thetas, 0, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL)
    assert len(res) == 28 and all(set(("x", "fun", "jac", "nit", "nfev", "status", "success", "message")) <= set(r) for r in res)
    for k, (th, r) in enumerate(zip(thetas, res)):
        s = cases.scipy_solve(th, pair, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL)
        sx, sf = cases.spread(th, pair, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL, s)
        dx, df = float(np.abs(r.x - s.x).max()), abs(r.fun - float(s.fun)) / abs(float(s.fun))
        print("start %2d status %d nit %2d nfev %3d: |dx| %.2e (allowed %.2e)  |df|/|f| %.2e (%.2e)"
              % (k, r.status, r.nit, r.nfev, dx, max(10 * sx, cases.X_FLOOR), df, max(10 * sf, cases.F_FLOOR)))
        assert (r.nit, r.status) == (int(s.nit), int(s.status)), k
        assert r.success == (r.status == 0) and isinstance(r.message, str)
        assert dx <= max(10.0 * sx, cases.X_FLOOR) and df <= max(10.0 * sf, cases.F_FLOOR), k
    reg = l2s.registration(cost, sc)
    multi = reg.optimise_multistart(*pair, sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL, solver="device")
    assert reg.best_index_ == 14
    for k in range(27):
        assert np.array_equal(multi[k].x, res[k].x) and multi[k].fun == res[k].fun, k
    assert l2s.angle_deg(cost.to_transformation(multi[14].x).rot, sc["truth_rot"]) < 15.0


def test_device_solver_lands_on_the_reference_pose(ctx):
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, gmmreg
    g, pair, sigma = cases.golden_case()
    allowance, spread10 = cases.golden_allowance(pair, sigma)
    cost = cf.RigidCostFunction(ctx=ctx)
    reg = gmmreg.L2DistRegistration(g["reg_source"], None, cost)
    assert reg._sigma == sigma
    res = reg.optimise_multistart(*pair, [cost.initial()], solver="device")[0]
    tfm = cost.to_transformation(res.x)
    print("allowance %.1e (10 x SciPy's spread %.2e): |rot - reg_rot| %.2e  |t - reg_t| %.2e"
          % (allowance, spread10, np.abs(tfm.rot - g["reg_rot"]).max(), np.abs(tfm.t - g["reg_t"]).max()))
    np.testing.assert_allclose(tfm.rot, g["reg_rot"], rtol=0, atol=allowance)
    np.testing.assert_allclose(tfm.t, g["reg_t"], rtol=0, atol=allowance)


def _batch_pairs():
    from conftest import load_golden
    g = load_golden("gmmreg_l2.npz")
    src, tgt = g["reg_source"], g["reg_target"]
    a = np.deg2rad(10.0)
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = tgt.mean(axis=0)
    return g, [(src, tgt), (src, (tgt - c) @ turn.T + c), (src[::2], tgt[::2])]


def _same_pose(a, b):
    return np.array_equal(a.rot, b.rot, equal_nan=True) and np.array_equal(a.t, b.t, equal_nan=True)


def test_the_mirrors_with_the_device_solver(ctx):
    from hgmm_amd.gmmreg_gpu.gmmreg import registration_gmmreg_batch, registration_gmmreg, RigidGMMReg
    from hgmm_amd.hgmm.hgmm_gpu import rotation_starts
    g, pairs = _batch_pairs()
    # the batch is the list of single-pair batches, and meets the reference as the SciPy batch does
    np.random.seed(3)
    batch = registration_gmmreg_batch(pairs, n_gmm_components=30, solver="device")
    np.random.seed(3)
    singles = [registration_gmmreg_batch([p], n_gmm_components=30, solver="device")[0] for p in pairs]
    for b in range(3):
        assert _same_pose(batch[b], singles[b]), b
    np.testing.assert_allclose(batch[0].rot, g["reg_rot"], atol=5e-3)
    np.testing.assert_allclose(batch[0].t, g["reg_t"], atol=2e-3)
    # registration_gmmreg: with starts it is the registration's own multi-start, without it the one identity start
    src, tgt = pairs[0]
    starts = rotation_starts((-60, 0, 60), centre=src.mean(axis=0))
    np.random.seed(3)
    won = registration_gmmreg(src, tgt, starts=starts, solver="device", n_gmm_components=30)
    np.random.seed(3)
    reg = RigidGMMReg(src, n_gmm_components=30)
    own, every, funs = reg.registration_multistart(tgt, starts, solver="device", return_all=True)
    assert _same_pose(won, own)
    # the winner is the start with the lowest final cost
    assert reg.best_index_ == int(np.argmin(funs)) and _same_pose(own, every[reg.best_index_])
    print("registration_gmmreg(starts=, solver=\"device\"): winner %d of %d" % (reg.best_index_, len(starts)))
    np.random.seed(3)
    one = registration_gmmreg(src, tgt, solver="device", n_gmm_components=30)
    np.random.seed(3)
    assert _same_pose(one, registration_gmmreg_batch([(src, tgt)], n_gmm_components=30, solver="device")[0])
    np.testing.assert_allclose(one.rot, g["reg_rot"], atol=5e-3)
    with pytest.raises(ValueError, match="solver"):
        registration_gmmreg(src, tgt, solver="host")


def test_history_leaves_no_trace(ragged):
    """After a device-loop tree registration of B = 3 > R = 2 pairs and a larger l2_solve, a solve has the bits of the same
    solve on a fresh context."""
    import hgmm_amd
    import _history_ops as H
    pairs, ids, thetas, sigmas, want = ragged
    pick = [1, 7]
    fresh = hgmm_amd.Context(0)
    try:
        fresh.l2_set_pairs(pairs)
        first = fresh.l2_solve(ids[pick], thetas[pick], sigmas[pick], MAX_ITER, GTOL)
    finally:
        fresh.close()
    used = hgmm_amd.Context(0)
    try:
        with used.config(reg_device_solve=1):
            H.OPS["forest_register_large"].fn(used)
        used.l2_set_pairs(pairs)
        used.l2_solve(ids, thetas, sigmas, MAX_ITER, GTOL)
        after = used.l2_solve(ids[pick], thetas[pick], sigmas[pick], MAX_ITER, GTOL)
    finally:
        used.close()
    for a, b in zip(first, after):
        assert a.tobytes() == b.tobytes()
    for at, r in enumerate(pick):
        assert not _differences(_row(after, at), want[r]), r


def test_refusals_name_themselves_and_leave_the_set_usable(ctx, ragged):
    import hgmm_amd
    pairs, ids, thetas, sigmas, _ = ragged
    fresh = hgmm_amd.Context(0)
    try:
        with pytest.raises(hgmm_amd.HgmmError, match="no resident pairs"):
            fresh.l2_solve([0], [thetas[0]], 0.2)
    finally:
        fresh.close()
    ctx.l2_set_pairs(pairs)
    pick = [2, 1]
    before = ctx.l2_solve(ids[pick], thetas[pick], sigmas[pick], MAX_ITER, GTOL)

    def same_bits_as_before():
        again = ctx.l2_solve(ids[pick], thetas[pick], sigmas[pick], MAX_ITER, GTOL)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, before))

    for bad in ([5], [-1]):
        with pytest.raises(hgmm_amd.HgmmError, match="pair out of range"):
            ctx.l2_solve(bad, [thetas[0]], 0.2)
        same_bits_as_before()
    with pytest.raises(hgmm_amd.HgmmError, match="R = 0 outside"):
        ctx.l2_solve([], np.zeros((0, 7)), 0.2)
    with pytest.raises(hgmm_amd.HgmmError, match="R = 4097 outside"):
        ctx.l2_solve(np.zeros(4097, np.int32), np.tile(thetas[0], (4097, 1)), 0.2)
    same_bits_as_before()
    for bad in (0.0, -0.1, np.nan):
        with pytest.raises(hgmm_amd.HgmmError, match="sigma not positive"):
            ctx.l2_solve([0, 1], thetas[:2], [0.2, bad])
    same_bits_as_before()
    for bad in (0, -3):
        with pytest.raises(hgmm_amd.HgmmError, match="max_iter < 1"):
            ctx.l2_solve([0], [thetas[0]], 0.2, bad)
    with pytest.raises(hgmm_amd.HgmmError, match="max_iter < 1"):
        ctx.l2_solve([0, 1], thetas[:2], 0.2, [3, 0], [1e-5, 1e-5])
    for bad in (-1e-5, np.nan):
        with pytest.raises(hgmm_amd.HgmmError, match="gtol negative or NaN"):
            ctx.l2_solve([0], [thetas[0]], 0.2, 10, bad)
    same_bits_as_before()
    # NULL arguments, straight at the C entries (grad_out alone may be NULL)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one, th, sg = np.zeros(1, np.int32), thetas[:1].copy(), np.array([0.2])
    x, f, n1, n2, n3 = np.zeros(7), np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    with pytest.raises(hgmm_amd.HgmmError, match="NULL argument"):
        ctx._check(ctx.lib.hgmm_l2_solve(ctx.h, 1, p(one), None, p(sg), 10, 1e-5, p(x), p(f), None, p(n1), p(n2), p(n3)))
    with pytest.raises(hgmm_amd.HgmmError, match="NULL argument"):
        ctx._check(ctx.lib.hgmm_l2_solve(ctx.h, 1, p(one), p(th), p(sg), 10, 1e-5, p(x), p(f), None, p(n1), p(n2), None))
    with pytest.raises(hgmm_amd.HgmmError, match="NULL argument"):
        ctx._check(ctx.lib.hgmm_l2_solve_each(ctx.h, 1, p(one), p(th), p(sg), None, p(sg), p(x), p(f), None, p(n1), p(n2), p(n3)))
    ctx._check(ctx.lib.hgmm_l2_solve(ctx.h, 1, p(one), p(th), p(sg), 10, 1e-5, p(x), p(f), None, p(n1), p(n2), p(n3)))
    full = ctx.l2_solve([0], th, 0.2)
    assert np.array_equal(x, full[0][0]) and f[0] == full[1][0] and n2[0] == full[4][0]
    same_bits_as_before()
    # a non-finite start is NOT refused: status 3 after one evaluation, its neighbour is what it was
    bad = thetas[pick].copy()
    bad[0, 2] = np.nan
    out = ctx.l2_solve(ids[pick], bad, sigmas[pick], MAX_ITER, GTOL)
    assert out[5][0] == 3 and out[4][0] == 1 and out[3][0] == 0
    assert all(a[1].tobytes() == b[1].tobytes() for a, b in zip(out, before))
    # the records above the 1 GiB cap: (200, 64) -> 4 workgroups of 13 doubles per hypothesis is far below it at any R <= 4096;
    # the cap is reached through a large pair
    big = 1 << 15
    rs = np.random.RandomState(1)
    ctx.l2_set_pairs([(rs.rand(big, 3), np.ones(big), rs.rand(big, 3), np.ones(big))])      # 512 x 128 workgroups a hypothesis
    with pytest.raises(hgmm_amd.HgmmError, match="exceed"):
        ctx.l2_solve(np.zeros(256, np.int32), np.tile(thetas[0], (256, 1)), 0.2)
    ctx.l2_set_pairs(pairs)
    same_bits_as_before()
