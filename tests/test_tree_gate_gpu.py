"""The Mahalanobis gate of the registration E-step (hgmm_tree_set_reg_gate) on the GPU.

With a finite gate a (point, node) pair that would contribute to the node's moments does so only if its squared Mahalanobis
distance to the node is <= the gate; the descent is untouched.  The checks: the gated E-step and the gated loop against the
float64 oracle (oracle.hgmm_tree.reg_e_step / register with gate=) at the bounds of the ungated tests; off is off and the gated kernels add exactly
what the ungated ones add (bitwise); the batched and multi-start launches are bitwise the serial gated call; on the
project's real scan pair with clutter the gate brings the result closer to the ground truth; errors and state.

Fixtures: hgmm_reg_L2.npz (2 013 points, T = 72: every node in the LDS table) and hgmm_reg_L4 (5 032 points, nodes beyond
584 take the global atomics); neither point count is a multiple of the 256-point workgroup."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import hgmm_tree

pytestmark = pytest.mark.gpu

I3 = np.identity(3)
LDS_NODES = hgmm_tree.level(3)


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    return {2: load_golden("hgmm_reg_L2.npz"), 4: load_golden("hgmm_reg_L4.npz")}


def rot_about(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def resident(ctx, g, target):
    L = int(g["L"])
    ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(target)
    return L, float(g["lambda_c"]), hgmm_tree.n_total(L)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def loop5(ctx, lc):
    """five iterations from the identity, no stop rule -> (rot, t, iterations, q, status, trace [5, 13])"""
    return ctx.tree_register(I3, np.zeros(3), 1.0, lc, 5, 0.0, None, want_trace=True)


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("deg", [10, 30])
@pytest.mark.parametrize("gate", [16.0, 9.0])
def test_gated_estep_matches_the_restatement(ctx, records, L, deg, gate):
    """No point is left out: no descent decision of these targets is a near-tie, and no contributing pair lies within 1e-9
    (relative) of the gate -- the smallest margin over the eight cases is 3.0e-5, far above what the device's rounding of
    the quadratic form can move."""
    g = records[L]
    X = g["rot%d_target" % deg]
    _, lc, T = resident(ctx, g, X)
    assert not hgmm_tree.reg_near_ties(hgmm_tree.reg_descent(X, g["pi"], g["mu"], g["cov"], L, lc)).any()
    o = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, gate=gate, report=True)
    print("L=%d rot%d gate %g: %d of %d contributing pairs gated, margin %.3g" % (L, deg, gate, o.gated, o.pairs, o.margin))
    assert o.margin > 1e-9 and 0 < o.gated < o.pairs
    ctx.tree_set_reg_gate(gate)
    try:
        m0, m1, m2 = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    finally:
        ctx.tree_set_reg_gate(np.inf)
    np.testing.assert_allclose(m0, o.m0, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(m1, o.m1, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(m2, o.m2, rtol=1e-10, atol=1e-12)
    if L == 4:                                   # the gate acted on the global-atomic path as well as on the LDS table
        free = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc)[0]
        assert (o.m0[LDS_NODES:] < free[LDS_NODES:]).any() and (o.m0[:LDS_NODES] < free[:LDS_NODES]).any()


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("deg", [10, 30])
@pytest.mark.parametrize("gate", [16.0, 9.0])
def test_gated_loop_matches_the_restatement(ctx, records, L, deg, gate):
    """Five iterations, tol 0: every pose against the restatement's loop at atol 1e-8 (the bound of the ungated loop tests).
    The margin is taken again at the poses the DEVICE visited: the smallest over all cases and iterations is 3.0e-6."""
    g = records[L]
    X = g["rot%d_target" % deg]
    _, lc, T = resident(ctx, g, X)
    ctx.tree_set_reg_gate(gate)
    try:
        rot, t, done, q, status, trace = loop5(ctx, lc)
    finally:
        ctx.tree_set_reg_gate(np.inf)
    assert done == 5 and status == 0
    o_tr = hgmm_tree.register(X, g["pi"], g["mu"], g["cov"], L, lc, 5, 0.0, gate=gate)[3]
    assert len(o_tr) == 5
    o_rot, o_t = o_tr[-1][:2]                    # the loop's own final pose (register returns its inverse)
    r_prev, t_prev = I3, np.zeros(3)
    margins = []
    for k in range(5):
        e = hgmm_tree.reg_e_step(X @ r_prev.T + t_prev, g["pi"], g["mu"], g["cov"], L, lc, gate=gate, report=True)
        margins.append(e.margin)
        assert e.margin > 1e-9 and e.gated > 0, k
        r_k, t_k = trace[k, :9].reshape(3, 3), trace[k, 9:12]
        np.testing.assert_allclose(r_k, o_tr[k][0], rtol=0, atol=1e-8, err_msg="iteration %d" % k)
        np.testing.assert_allclose(t_k, o_tr[k][1], rtol=0, atol=1e-8, err_msg="iteration %d" % k)
        r_prev, t_prev = r_k, t_k
    print("L=%d rot%d gate %g: gate margins along the device's path %s" % (L, deg, gate, ["%.2g" % m for m in margins]))
    np.testing.assert_allclose(rot, o_rot, rtol=0, atol=1e-8)
    np.testing.assert_allclose(t, o_t, rtol=0, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. bitwise: off is off; the gated instantiation adds what the ungated one adds
# ---------------------------------------------------------------------------------------------------------------------
def everything(c, g, target):
    """moments [T] + [T,3] + [T,3,3], the normal equations' numbers and a five-iteration trace at the context's gate"""
    L, lc, T = resident(c, g, target)
    R = rot_about([0.2, 1.0, 0.1], 3.0)
    t = np.array([0.002, -0.001, 0.0015])
    ata, atb, btb = c.tree_reg_normal(R, t, 1.0, lc)
    rot, tt, done, q, status, trace = loop5(c, lc)
    return c.tree_reg_estep(T, R, t, 1.0, lc) + (ata, atb, np.array(btb), rot, tt, np.array([done, status]), trace)


@pytest.mark.parametrize("L", [2, 4])
def test_off_is_off_and_a_gate_everything_passes_changes_no_bit(ctx, records, L):
    import hgmm_amd
    g = records[L]
    X = g["rot10_target"]
    fresh = hgmm_amd.Context(0)
    try:
        assert fresh.tree_get_reg_gate() == np.inf
        ref = everything(fresh, g, X)
    finally:
        fresh.close()
    assert ctx.tree_get_reg_gate() == np.inf
    ctx.tree_set_reg_gate(16.0)
    gated = everything(ctx, g, X)
    assert not same_bits(gated[:1], ref[:1])                           # (the gate was in force in between)
    ctx.tree_set_reg_gate(np.inf)
    assert same_bits(everything(ctx, g, X), ref)
    # gate 1e300: the GATED kernels, every finite point passes -- the sums are integers, so not a bit may differ
    ctx.tree_set_reg_gate(1e300)
    try:
        assert ctx.tree_get_reg_gate() == 1e300
        wide = everything(ctx, g, X)
    finally:
        ctx.tree_set_reg_gate(np.inf)
    assert len(wide[3]) == 6 and len(wide[4]) == 6                     # (21 + 6 + 1 = the normal equations' 28 numbers)
    for k, (a, b) in enumerate(zip(wide, ref)):
        assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. multi-start and batch: every member bitwise the serial gated call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_solve", [0, 1])
def test_gated_multi_and_batch_are_bitwise_the_serial_gated_call(ctx, records, device_solve):
    g = records[2]
    P, X = g["points"], g["rot10_target"]
    L, lc = int(g["L"]), float(g["lambda_c"])
    T = hgmm_tree.n_total(L)
    c = X.mean(axis=0)
    rots = [I3, rot_about([0, 0, 1], 10), rot_about([0, 0, 1], -10)]
    rot0, t0 = np.stack(rots), np.stack([c - R @ c for R in rots])
    targets = [X, X[:1500], X[:700]]
    idx = np.random.RandomState(72).randint(T, size=T)
    ctx.tree_set_reg_gate(16.0)
    try:
        with ctx.config(reg_device_solve=device_solve):
            # the forest first: the serial calls below replace the context's resident cloud
            arrs = ctx.set_points_batch([P] * 3)
            ctx.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
            ctx.tree_set_targets_batch(targets)
            b_rot, b_t, b_it, b_q, b_st, b_tr = ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 5, 0.0,
                                                                        want_trace=True)
            ctx.set_points(P)
            pi, mu, cov = ctx.tree_build(L, 20.0, 1e-4, P[idx], 0.004)[:3]
            for b, tg in enumerate(targets):
                ctx.tree_set_nodes(L, pi, mu, cov)
                ctx.tree_set_target(tg)
                s_rot, s_t, s_it, s_q, s_st, s_tr = loop5(ctx, lc)
                assert (int(b_it[b]), int(b_st[b])) == (s_it, s_st), b
                assert np.array_equal(b_rot[b], s_rot) and np.array_equal(b_t[b], s_t) and b_q[b] == s_q, b
                assert np.array_equal(b_tr[b], s_tr), b
            # (the tree built here is coarse -- ten nodes take mass -- and the 700-point piece leaves it after two iterations:
            #  status 2, in the batch as in the serial call; the two larger targets run the whole budget)
            assert list(b_it[:2]) == [5, 5] and list(b_st[:2]) == [0, 0] and b_it[2] > 0
            # multi-start on the record's own tree
            resident(ctx, g, X)
            m_rot, m_t, m_it, m_q, m_st, m_tr = ctx.tree_register_multi(rot0, t0, 1.0, lc, 5, 0.0, want_trace=True)
            for k in range(3):
                s_rot, s_t, s_it, s_q, s_st, s_tr = ctx.tree_register(rot0[k], t0[k], 1.0, lc, 5, 0.0, None, want_trace=True)
                assert (int(m_it[k]), int(m_st[k])) == (s_it, s_st) and s_it == 5, k
                assert np.array_equal(m_rot[k], s_rot) and np.array_equal(m_t[k], s_t) and m_q[k] == s_q, k
                assert np.array_equal(m_tr[k], s_tr), k
            gated_trace = m_tr[0]
        ctx.tree_set_reg_gate(np.inf)
        with ctx.config(reg_device_solve=device_solve):
            free = ctx.tree_register_multi(rot0, t0, 1.0, lc, 5, 0.0, want_trace=True)[5][0]
        assert not np.array_equal(free, gated_trace)                   # (the gate was in force in the launches above)
    finally:
        ctx.tree_set_reg_gate(np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# 6. it does what it is for
# ---------------------------------------------------------------------------------------------------------------------
def test_gate_brings_a_cluttered_real_scan_pair_closer_to_the_ground_truth(ctx, bunny):
    """bun000's tree (L = 3, product defaults) <- bun045 at its ground-truth placement of bun_conf.npz, moved by 8 deg /
    5 mm as in test_registration_real_scan_pair_against_bun_conf, plus 30 % uniform clutter in its bounding box.  The error
    is the mean distance of the registered scan (clutter left out) from its ground-truth placement.  The restatement gives
    2.73 mm with gate 16 against 4.74 mm without (ratio 0.58); the bound 0.8 allows for a GPU tree that stops a level one
    iteration apart."""
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    a = bunny.astype(np.float64)
    b = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    conf = load_golden("bun_conf.npz")
    pose = conf["poses"][list(conf["names"]).index("bun045.ply")]
    t, (qx, qy, qz, qw) = pose[:3], pose[3:]
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    world = b @ R + t                      # bun.conf convention: p_world = R(q)^T p + t
    moved = world @ rot_about([0.3, 1.0, 0.2], 8.0).T + np.array([0.005, -0.00375, 0.00625])
    lo, hi = moved.min(axis=0), moved.max(axis=0)
    target = np.concatenate([moved, np.random.RandomState(5).uniform(lo, hi, (int(0.3 * len(moved)), 3))])

    def error(res):
        tf = res.transformation.inverse()                      # the loop's own pose: target -> tree
        return np.linalg.norm(moved @ np.asarray(tf.rot).T + np.asarray(tf.t) - world, axis=1).mean()

    kw = dict(tree_level=3, lambda_c=0.01, ls=20, sig2=0.004)

    def register(c, **gate):
        # (a new object per call: a GMMTree starts its loop from the pose its previous registration ended at)
        return GMMTree(a, ctx=c, **kw).registration(target, 30, 1e-6, **gate)

    gated = register(ctx, maha2_gate=16.0)
    assert ctx.tree_get_reg_gate() == np.inf                   # (the mirror restored the context's gate)
    free = register(ctx)
    e_gated, e_free = error(gated), error(free)
    print("30 %% clutter: %.2f mm without a gate, %.2f mm with gate 16 (ratio %.2f)" % (1e3 * e_free, 1e3 * e_gated, e_gated / e_free))
    assert e_gated <= 0.8 * e_free
    # the ungated call after a gated one == the same call on a context no gate was ever set on
    fresh = hgmm_amd.Context(0)
    try:
        ref = register(fresh)
    finally:
        fresh.close()
    assert np.array_equal(ref.transformation.rot, free.transformation.rot)
    assert np.array_equal(ref.transformation.t, free.transformation.t) and np.array_equal(np.ravel(ref.q), np.ravel(free.q))
    # the constructor's gate and the method's keyword are the same setting
    again = GMMTree(a, ctx=ctx, maha2_gate=16.0, **kw).registration(target, 30, 1e-6)
    assert np.array_equal(again.transformation.rot, gated.transformation.rot) and np.array_equal(again.transformation.t, gated.transformation.t)


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors and state
# ---------------------------------------------------------------------------------------------------------------------
def test_gate_errors_and_state(ctx, records):
    import ctypes
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    HGMM_ERR_ARG = -2                     # include/hgmm.h
    assert ctx.tree_get_reg_gate() == np.inf
    ctx.tree_set_reg_gate(25.0)
    try:
        for bad in (float("nan"), 0.0, -1.0, -np.inf):
            assert ctx.lib.hgmm_tree_set_reg_gate(ctx.h, bad) == HGMM_ERR_ARG
            assert b"gate" in ctx.lib.hgmm_last_error(ctx.h)
            assert ctx.tree_get_reg_gate() == 25.0
            with pytest.raises(hgmm_amd.HgmmError):
                ctx.tree_set_reg_gate(bad)
        assert ctx.lib.hgmm_tree_get_reg_gate(ctx.h, None) == HGMM_ERR_ARG
        out = ctypes.c_double(-1.0)
        assert ctx.lib.hgmm_tree_get_reg_gate(ctx.h, ctypes.byref(out)) == 0 and out.value == 25.0
        for good in (9.0, 1e-300, 1e300, np.inf, 25.0):
            assert ctx.tree_set_reg_gate(good) is ctx and ctx.tree_get_reg_gate() == good
        # a mirror that raises midway puts the context's gate back
        g = records[2]
        gt = GMMTree(None, tree_level=int(g["L"]), lambda_c=float(g["lambda_c"]), ctx=ctx)
        gt.set_nodes(g["pi"], g["mu"], g["cov"])
        seen = []

        def boom(tf):
            seen.append(ctx.tree_get_reg_gate())
            raise RuntimeError("midway")

        gt.set_callbacks([boom])
        with pytest.raises(RuntimeError, match="midway"):
            gt.registration(g["rot10_target"], 5, 1e-4, maha2_gate=9)
        assert seen == [9.0] and ctx.tree_get_reg_gate() == 25.0
        # ... and without a gate of its own it leaves the context's in force
        gt.set_callbacks([lambda tf: seen.append(ctx.tree_get_reg_gate())])
        gt.registration(g["rot10_target"], 2, 0.0)
        assert seen == [9.0, 25.0, 25.0]
    finally:
        ctx.tree_set_reg_gate(np.inf)
