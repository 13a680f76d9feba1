"""The resident L2 GMMReg cost (hgmm_l2_set_pairs / hgmm_l2_cost, csrc/gmmreg_l2_kernels.hip) and what is built on it:
``RigidCostFunction.evaluate_many``, the lock-step multi-start and ``registration_gmmreg_batch``."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import l2_scenario as l2s

pytestmark = pytest.mark.gpu

# the kernel's own shape (csrc/gmmreg_l2_kernels.hip): 64 source centres per workgroup, 128 target centres per LDS tile,
# 256 target centres per workgroup
BLOCK, TILE, SPLIT = 64, 128, 256


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    return hgmm_amd.default_context()


def test_evaluate_many_matches_the_reference_goldens(ctx):
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    g = load_golden("gmmreg_l2.npz")
    cost = cf.RigidCostFunction(ctx=ctx)
    cost.set_pairs([(g["mu_s"], g["phi_s"], g["mu_t"], g["phi_t"])])
    f, grad = cost.evaluate_many(g["theta"], 0, float(g["sigma"]))
    assert f.shape == (5,) and grad.shape == (5, 7)
    for r in range(5):
        np.testing.assert_allclose(f[r], g["cost_f"][r], rtol=1e-12)
        np.testing.assert_allclose(grad[r], g["cost_g"][r], rtol=1e-10, atol=1e-12)


def _host_outputs_and_bounds(theta, mu_s, phi_s, mu_t, phi_t, sigma):
    """The 13 outputs as the host's RigidCostFunction forms them (its pose, compute_l2_dist, g.T @ mu_source), and for each
    the sum of the absolute values of the terms it is a sum of, from the same kernel matrix:
        f        sum_ij phis_i w_j e_ij                                        w_j = phit_j / z
        gsum_a   sum_ij phis_i w_j e_ij (|y_ia| + |mut_ja|) / 2 sigma^2        (grad_i = phis_i (g0_i y_i - g1_i) / 2 sigma^2)
        M_ab     the same with |x_ib| as a further factor"""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, transforms as tf
    pose = cf.RigidCostFunction().to_transformation(theta)
    y = pose.transform(mu_s)
    f, g = cf.compute_l2_dist(y, phi_s, mu_t, phi_t, sigma)
    value = np.concatenate([[f], g.sum(axis=0), (g.T @ mu_s).ravel()])
    e = tf.kernel_matrix(mu_t, y, np.sqrt(2.0) * sigma)                                 # [Js, Jt]
    t0 = phi_s[:, None] * (phi_t / np.power(2.0 * np.pi * sigma ** 2, 1.5))[None, :] * e
    ga = np.stack([t0 * (np.abs(y[:, a, None]) + np.abs(mu_t[None, :, a])) for a in range(3)]) / (2.0 * sigma ** 2)   # [3, Js, Jt]
    terms = np.concatenate([[t0.sum()], ga.sum(axis=(1, 2)), np.einsum('aij,ib->ab', ga, np.abs(mu_s)).ravel()])
    return pose, value, terms


EDGES = [(1, 1), (5, 70), (64, 128), (65, 129), (800, 800), (1500, 3000),
         # below the tile; the target split of 256 and its neighbours, with the source block's
         (BLOCK - 1, TILE - 1), (BLOCK - 1, SPLIT - 1), (BLOCK, SPLIT), (BLOCK + 1, SPLIT + 1), (2 * BLOCK + 1, 2 * SPLIT + 1)]


@pytest.mark.parametrize("js,jt", EDGES)
def test_tile_edges_within_the_summation_bound(ctx, js, jt):
    """Random centres in the unit cube, positive weights, sigma = 0.15, three random poses (a random rotation about the
    cube's centre and a shift, so that the mixtures overlap).  Each output is within (Js + Jt + 16) 2^-52 sum |terms| of
    the host's: the float64 summation bound over the Jt + Js additions of either side, 16 for the handful of roundings per
    term (the exponential's last bit on either side among them)."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    rs = np.random.RandomState(1000 * js + jt)
    mu_s, mu_t = rs.rand(js, 3), rs.rand(jt, 3)
    phi_s, phi_t = 0.1 + rs.rand(js), 0.1 + rs.rand(jt)
    sigma = 0.15
    thetas = []
    for _ in range(3):
        q = rs.randn(4)
        q /= np.linalg.norm(q)
        rot = cf.RigidCostFunction().to_transformation(np.concatenate([q, np.zeros(3)])).rot
        thetas.append(np.concatenate([q, 0.5 - rot @ np.full(3, 0.5) + rs.uniform(-0.1, 0.1, 3)]))
    ctx.l2_set_pairs([(mu_s, phi_s, mu_t, phi_t)])
    hosts = [_host_outputs_and_bounds(th, mu_s, phi_s, mu_t, phi_t, sigma) for th in thetas]
    dev = ctx.l2_cost([0, 0, 0], [h[0].rot for h in hosts], [h[0].t for h in hosts], sigma)
    assert dev.shape == (3, 13) and np.isfinite(dev).all()
    worst = 0.0
    for r, (_, value, terms) in enumerate(hosts):
        bound = (js + jt + 16) * 2.0 ** -52 * terms
        worst = max(worst, float((np.abs(dev[r] - value) / bound).max()))
    print("(%d, %d): largest |device - host| / bound = %.3f" % (js, jt, worst))
    for r, (_, value, terms) in enumerate(hosts):
        assert (np.abs(dev[r] - value) <= (js + jt + 16) * 2.0 ** -52 * terms).all(), (r, dev[r], value)
    # evaluate_many is these sums and the host's chain rule
    cost = cf.RigidCostFunction(ctx=ctx)
    cost.set_pairs([(mu_s, phi_s, mu_t, phi_t)])
    f, grad = cost.evaluate_many(thetas, 0, sigma)
    assert np.array_equal(f, dev[:, 0]) and np.array_equal(grad[:, 4:], dev[:, 1:4])
    # (the wiring of the chain rule -- M's layout, the order of the seven -- against the host's: a slip there is an error of
    # order one, the roundings bounded above are of order 1e-12 of the terms)
    f_host, grad_host = cf.RigidCostFunction()(thetas[0], mu_s, phi_s, mu_t, phi_t, sigma)
    np.testing.assert_allclose(grad[0], grad_host, rtol=0, atol=1e-7 * np.abs(grad_host).max())


def _ragged_pairs(rs):
    return [(rs.rand(js, 3), 0.1 + rs.rand(js), rs.rand(jt, 3), 0.1 + rs.rand(jt))
            for js, jt in ((30, 25), (70, 300), (5, 129), (200, 64))]


def _random_pose(rs):
    from hgmm_amd.gmmreg_gpu import so
    q = rs.randn(4)
    return so.quaternion_matrix(q)[:3, :3], rs.uniform(-0.2, 0.2, 3)


def test_a_hypothesis_does_not_depend_on_its_neighbours_or_its_position(ctx):
    rs = np.random.RandomState(7)
    pairs = _ragged_pairs(rs)
    ctx.l2_set_pairs(pairs)
    rot, t = _random_pose(rs)
    alone = ctx.l2_cost([1], [rot], [t], 0.2)                                    # pair 1: two source blocks, two target splits
    assert np.isfinite(alone).all()
    R = 40
    ids = rs.randint(4, size=R)
    poses = [_random_pose(rs) for _ in range(R)]
    rots, ts = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    sigmas = rs.uniform(0.1, 0.4, R)
    for at in (0, 17, 39):
        ids[at], rots[at], ts[at], sigmas[at] = 1, rot, t, 0.2
    many = ctx.l2_cost(ids, rots, ts, sigmas)
    for at in (0, 17, 39):
        assert np.array_equal(many[at], alone[0]), at
    # every other member, too, is its own R = 1 call
    for r in (1, 16, 38):
        assert np.array_equal(many[r], ctx.l2_cost([ids[r]], [rots[r]], [ts[r]], sigmas[r])[0]), r
    # the pair at another index of another set
    ctx.l2_set_pairs([pairs[3], pairs[0], pairs[2], pairs[1], pairs[1]])
    moved = ctx.l2_cost([0, 3, 4], [rots[5], rot, rot], [ts[5], t, t], [0.3, 0.2, 0.2])
    assert np.array_equal(moved[1], alone[0]) and np.array_equal(moved[2], alone[0])


def test_two_cost_functions_on_one_context_keep_their_own_mixtures(ctx):
    """A context holds one resident set; a cost function that finds another's there puts its own back."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    rs = np.random.RandomState(5)
    pairs = _ragged_pairs(rs)
    theta = np.concatenate([rs.randn(4), rs.uniform(-0.2, 0.2, 3)])
    one, other = cf.RigidCostFunction(ctx=ctx), cf.RigidCostFunction(ctx=ctx)
    one.set_pairs(pairs[:2])
    before = one.evaluate_many([theta], 1, 0.2)
    other.set_pairs(pairs[2:])
    theirs = other.evaluate_many([theta], 1, 0.2)
    again = one.evaluate_many([theta], 1, 0.2)
    assert np.array_equal(again[0], before[0]) and np.array_equal(again[1], before[1])
    assert not np.array_equal(theirs[0], before[0])
    ctx.l2_set_pairs(pairs[2:])                                                  # ... also behind a direct call on the context
    again = one.evaluate_many([theta], 1, 0.2)
    assert np.array_equal(again[0], before[0]) and np.array_equal(again[1], before[1])


def test_multistart_on_the_device_is_the_serial_device_solve_of_every_start(ctx):
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, gmmreg
    sc = l2s.scenario()
    cost = cf.RigidCostFunction(ctx=ctx)
    reg = l2s.registration(cost, sc)
    calls = []
    inner = ctx.l2_cost
    ctx.l2_cost = lambda *a: calls.append(len(a[0])) or inner(*a)
    try:
        multi = reg.optimise_multistart(sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"], sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL)
    finally:
        del ctx.l2_cost
    nfev = [m.nfev for m in multi]
    print("nfev: sum %d, max %d; l2_cost calls %d" % (sum(nfev), max(nfev), len(calls)))
    assert len(calls) == max(nfev) and sum(calls) == sum(nfev)
    for k, start in enumerate(sc["starts"]):
        alone = gmmreg.lockstep_solve(cost.evaluate_many, [(cf.theta_from_transformation(start), 0, sc["sigma"])],
                                      l2s.OPT_MAXITER, l2s.OPT_TOL)[0]
        assert np.array_equal(alone.x, multi[k].x) and alone.fun == multi[k].fun and alone.nfev == multi[k].nfev, k
    assert reg.best_index_ == 14
    won = l2s.angle_deg(cost.to_transformation(multi[14].x).rot, sc["truth_rot"])
    print("winner %.1f deg from the truth (f = %.6e)" % (won, multi[14].fun))
    assert won < 15.0


def _batch_pairs():
    g = load_golden("gmmreg_l2.npz")
    src, tgt = g["reg_source"], g["reg_target"]
    a = np.deg2rad(10.0)
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = tgt.mean(axis=0)
    return g, [(src, tgt), (src, (tgt - c) @ turn.T + c), (src[::2], tgt[::2])]


def _same_pose(a, b):
    # (NaN == NaN here: two runs that both break down on a degenerate mixture have still done the same)
    return np.array_equal(a.rot, b.rot, equal_nan=True) and np.array_equal(a.t, b.t, equal_nan=True)


def test_batch_is_the_list_of_single_pair_batches_and_meets_the_reference(ctx):
    from hgmm_amd.gmmreg_gpu.gmmreg import registration_gmmreg_batch
    g, pairs = _batch_pairs()
    np.random.seed(3)
    batch = registration_gmmreg_batch(pairs, n_gmm_components=30)
    np.random.seed(3)
    singles = [registration_gmmreg_batch([p], n_gmm_components=30)[0] for p in pairs]
    assert len(batch) == 3
    for b in range(3):
        assert _same_pose(batch[b], singles[b]), b
    np.testing.assert_allclose(batch[0].rot, g["reg_rot"], atol=5e-3)
    np.testing.assert_allclose(batch[0].t, g["reg_t"], atol=2e-3)
    with pytest.raises(ValueError, match="maxiter"):
        registration_gmmreg_batch(pairs, n_gmm_components=30, maxiter=2)


def test_batch_with_starts_is_every_pairs_own_multistart(ctx):
    from hgmm_amd.gmmreg_gpu.gmmreg import registration_gmmreg_batch, registration_gmmreg, RigidGMMReg
    from hgmm_amd.hgmm.hgmm_gpu import rotation_starts
    _, pairs = _batch_pairs()
    starts = [rotation_starts((-20, 0, 20), centre=pairs[0][0].mean(axis=0))[k] for k in (13, 4, 22)]
    np.random.seed(3)
    tfs, winners = registration_gmmreg_batch(pairs, starts=starts, n_gmm_components=30)
    np.random.seed(3)
    for b, (src, tgt) in enumerate(pairs):
        reg = RigidGMMReg(src, n_gmm_components=30)
        own = reg.registration_multistart(tgt, starts)
        assert reg.best_index_ == winners[b] and _same_pose(own, tfs[b]), b
    np.random.seed(3)
    assert _same_pose(registration_gmmreg(pairs[0][0], pairs[0][1], starts=starts, n_gmm_components=30), tfs[0])


def test_batch_with_differing_component_counts_fits_one_by_one(ctx):
    """A cloud of 30 points caps its mixtures at 24 components: the fits then run serially, in the same order."""
    from hgmm_amd.gmmreg_gpu.gmmreg import registration_gmmreg_batch
    _, pairs = _batch_pairs()
    pairs = [pairs[0], (pairs[0][0][::67], pairs[0][1][::67])]
    assert len(pairs[1][0]) == 31
    batch = registration_gmmreg_batch(pairs, n_gmm_components=30)
    singles = [registration_gmmreg_batch([p], n_gmm_components=30)[0] for p in pairs]
    for b in range(2):
        assert _same_pose(batch[b], singles[b]), b


def test_refusals_name_themselves_and_leave_the_set_as_it_was(ctx):
    import hgmm_amd
    rs = np.random.RandomState(11)
    pairs = _ragged_pairs(rs)
    rot, t = _random_pose(rs)
    fresh = hgmm_amd.Context(0)
    try:
        with pytest.raises(hgmm_amd.HgmmError, match="no resident pairs"):
            fresh.l2_cost([0], [rot], [t], 0.2)
    finally:
        fresh.close()
    ctx.l2_set_pairs(pairs)
    before = ctx.l2_cost([2, 1], [rot, rot], [t, t], [0.2, 0.3])

    def same_bits_as_before():
        assert np.array_equal(ctx.l2_cost([2, 1], [rot, rot], [t, t], [0.2, 0.3]), before)

    for bad in ([4], [-1]):
        with pytest.raises(hgmm_amd.HgmmError, match="pair out of range"):
            ctx.l2_cost(bad, [rot], [t], 0.2)
        same_bits_as_before()
    with pytest.raises(hgmm_amd.HgmmError, match="R = 0 outside"):
        ctx.l2_cost([], np.zeros((0, 3, 3)), np.zeros((0, 3)), 0.2)
    too_many = 4097
    with pytest.raises(hgmm_amd.HgmmError, match="R = 4097 outside"):
        ctx.l2_cost(np.zeros(too_many, np.int32), np.tile(rot, (too_many, 1, 1)), np.tile(t, (too_many, 1)), 0.2)
    same_bits_as_before()
    for bad in (0.0, -0.1, np.nan):
        with pytest.raises(hgmm_amd.HgmmError, match="sigma not positive"):
            ctx.l2_cost([0, 1], [rot, rot], [t, t], [0.2, bad])
        same_bits_as_before()
    # a pair without components, no pairs at all: refused, and the resident set stays
    empty = (np.zeros((0, 3)), np.zeros(0), pairs[0][2], pairs[0][3])
    for bad in ([pairs[0], empty], [(pairs[0][0], pairs[0][1], np.zeros((0, 3)), np.zeros(0))]):
        with pytest.raises(hgmm_amd.HgmmError, match="J < 1"):
            ctx.l2_set_pairs(bad)
        same_bits_as_before()
    with pytest.raises(hgmm_amd.HgmmError, match="B = 0 outside"):
        ctx.l2_set_pairs([])
    same_bits_as_before()
    # NULL arguments, straight at the C entries
    one, d3 = np.ones(1, np.int32), np.ones(3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(hgmm_amd.HgmmError, match="NULL argument"):
        ctx._check(ctx.lib.hgmm_l2_set_pairs(ctx.h, 1, p(one), None, p(d3), p(one), p(d3), p(d3)))
    with pytest.raises(hgmm_amd.HgmmError, match="NULL argument"):
        ctx._check(ctx.lib.hgmm_l2_cost(ctx.h, 1, p(one), p(np.ones(9)), p(d3), p(d3), None))
    same_bits_as_before()
    # a non-finite pose is NOT refused: its outputs are non-finite, its neighbour's are what they were
    bad_t = np.array([np.nan, 0.0, 0.0])
    out = ctx.l2_cost([2, 1, 2], [rot, rot, rot * np.nan], [bad_t, t, t], [0.2, 0.3, 0.2])
    assert not np.isfinite(out[0]).any() and not np.isfinite(out[2]).any() and np.array_equal(out[1], before[1])
