"""Per-point weights of the registration target (hgmm_tree_set_target_weights[_batch]) on the GPU.

A target point i with weight w_i >= 0 adds w_i * gamma where it added gamma; the descent, the stop rule, the 1e-15 floor
and the gate do not see the weight.  The checks: the weighted E-step and the weighted loop against the float64 oracle
(oracle.hgmm_tree.reg_e_step / register with w=) at the bounds of the unweighted and gated tests; w == 1 is bitwise the
unweighted result on every entry, w == 2 exactly twice the moments, NULL and a new target take the weights off; a zero weight is an absent point; the
batched and multi-start launches are bitwise the serial weighted call; the score's sums are the weighted sums of its own
per-point arrays, and the batched and multi-start scores take each member's chunk count and weight sum from its own table
entry; on the project's real scan pair the count-weighted voxel centroids reach the full scan's pose; errors and state;
two ranks with a shard of the weights each.

Fixtures: hgmm_reg_L2.npz (2 013 points, T = 72: every node in the LDS table) and hgmm_reg_L4 (5 032 points, nodes beyond
584 take the global atomics); neither point count is a multiple of the 256-point workgroup."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import hgmm_tree

from _tree_helpers import loop5, resident, same_bits, weights_for

pytestmark = pytest.mark.gpu

I3 = np.identity(3)
LDS_NODES = hgmm_tree.level(3)
HGMM_ERR_ARG, HGMM_ERR_STATE = -2, -3          # include/hgmm.h


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


@pytest.fixture()
def gated(ctx):
    """set the context's gate for a test, +inf afterwards"""
    def set_gate(gate):
        ctx.tree_set_reg_gate(gate)
    yield set_gate
    ctx.tree_set_reg_gate(np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("deg", [10, 30])
@pytest.mark.parametrize("gate", [np.inf, 16.0])
def test_weighted_estep_matches_the_restatement(ctx, records, gated, L, deg, gate):
    """rtol 1e-10 / atol 1e-12, the gate tests' bound: each term is rounded to 2^-F of the extent with F >= 46 at these
    sizes (sum of the weights < 2^14, 62 - 15 bits), so n terms stay below 2^-31 of it.  No descent decision of these
    targets is a near-tie and no contributing pair lies within 1e-9 of the gate (tests/test_tree_gate_gpu.py)."""
    g = records[L]
    X = g["rot%d_target" % deg]
    w = weights_for(len(X))
    assert (w == 0).sum() > 100 and w.sum() < 2 ** 14
    _, lc, T = resident(ctx, g, X, w)
    assert not hgmm_tree.reg_near_ties(hgmm_tree.reg_descent(X, g["pi"], g["mu"], g["cov"], L, lc)).any()
    if np.isfinite(gate):
        assert hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, gate=gate, report=True).margin > 1e-9
    o = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, w, gate)
    gated(gate)
    m = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    for name, a, b in zip(("m0", "m1", "m2"), m, o):
        print("L=%d rot%d gate %g %s: largest difference %.3g" % (L, deg, gate, name, np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12, err_msg=name)
    ctx.tree_set_target_weights(None)
    free = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    assert not np.array_equal(free[0], m[0])
    if L == 4:                                   # the weights acted on the global-atomic path as well as on the LDS table
        for k in range(3):
            assert (m[k][LDS_NODES:] != free[k][LDS_NODES:]).any() and (m[k][:LDS_NODES] != free[k][:LDS_NODES]).any(), k


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("deg", [10, 30])
@pytest.mark.parametrize("gate", [np.inf, 16.0])
def test_weighted_loop_matches_the_restatement(ctx, records, gated, L, deg, gate):
    """Five iterations, tol 0: every pose against the restatement's loop at atol 1e-8, the bound of the ungated and gated
    loop tests."""
    g = records[L]
    X = g["rot%d_target" % deg]
    w = weights_for(len(X))
    _, lc, T = resident(ctx, g, X, w)
    gated(gate)
    rot, t, done, q, status, trace = loop5(ctx, lc)
    assert done == 5 and status == 0
    o_rot_inv, o_t_inv, o_q, o_tr = hgmm_tree.register(X, g["pi"], g["mu"], g["cov"], L, lc, 5, 0.0, w, gate)
    assert len(o_tr) == 5
    worst = 0.0
    for k in range(5):
        r_k, t_k = trace[k, :9].reshape(3, 3), trace[k, 9:12]
        worst = max(worst, np.abs(r_k - o_tr[k][0]).max(), np.abs(t_k - o_tr[k][1]).max())
        np.testing.assert_allclose(r_k, o_tr[k][0], rtol=0, atol=1e-8, err_msg="iteration %d" % k)
        np.testing.assert_allclose(t_k, o_tr[k][1], rtol=0, atol=1e-8, err_msg="iteration %d" % k)
    print("L=%d rot%d gate %g: largest pose difference over five iterations %.3g" % (L, deg, gate, worst))
    np.testing.assert_allclose(rot, o_tr[4][0], rtol=0, atol=1e-8)
    np.testing.assert_allclose(t, o_tr[4][1], rtol=0, atol=1e-8)
    # and the weights steer the loop: the unweighted one ends elsewhere
    ctx.tree_set_target_weights(None)
    assert not np.array_equal(loop5(ctx, lc)[0], rot)


# ---------------------------------------------------------------------------------------------------------------------
# 3. exactness: w == 1 is the unweighted result, bit for bit, on every entry; w == 2 doubles; NULL / a new target: off
# ---------------------------------------------------------------------------------------------------------------------
def everything(c, g, target, w=None):
    """tests/test_tree_gate_gpu.py's helper with the target's weights: moments [T] + [T,3] + [T,3,3], the normal equations'
    numbers, a five-iteration trace -- and the score summary at the loop's last pose"""
    L, lc, T = resident(c, g, target, w)
    R = rot_about([0.2, 1.0, 0.1], 3.0)
    t = np.array([0.002, -0.001, 0.0015])
    ata, atb, btb = c.tree_reg_normal(R, t, 1.0, lc)
    rot, tt, done, q, status, trace = loop5(c, lc)
    summary = c.tree_score(rot, tt, 1.0, lc, want=())[0]
    return c.tree_reg_estep(T, R, t, 1.0, lc) + (ata, atb, np.array(btb), rot, tt, np.array([done, status]), trace, summary)


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("device_solve", [0, 1])
def test_unit_weights_are_the_unweighted_bits_serial(ctx, records, L, device_solve):
    g = records[L]
    X = g["rot10_target"]
    n = len(X)
    with ctx.config(reg_device_solve=device_solve):
        ref = everything(ctx, g, X)
        assert ref[-1][0] == n
        ones = everything(ctx, g, X, np.ones(n))                       # (a) the WEIGHTED kernels, every weight 1
        for k, (a, b) in enumerate(zip(ones, ref)):
            assert np.array_equal(a, b), k
        other = everything(ctx, g, X, weights_for(n))
        assert not same_bits(other[:1], ref[:1]) and not np.array_equal(other[-1], ref[-1])
        ctx.tree_set_target_weights(weights_for(n))                    # (b) NULL: the unweighted bits are back
        ctx.tree_set_target_weights(None)
        L_, lc, T = int(g["L"]), float(g["lambda_c"]), hgmm_tree.n_total(L)
        R, t = rot_about([0.2, 1.0, 0.1], 3.0), np.array([0.002, -0.001, 0.0015])
        assert same_bits(ctx.tree_reg_estep(T, R, t, 1.0, lc), ref[:3])
        assert same_bits(loop5(ctx, lc)[5:], ref[9:10])
        ctx.tree_set_target_weights(np.full(n, 2.0))                   # (c) w == 2: exactly twice the moments
        for a, b in zip(ctx.tree_reg_estep(T, R, t, 1.0, lc), ref[:3]):
            assert np.array_equal(a, 2.0 * b)
        assert ctx.tree_score(None, None, 1.0, lc, want=())[0][0] == 2.0 * n
        ctx.tree_set_target(X)                                         # (d) a new target drops the weights
        assert same_bits(ctx.tree_reg_estep(T, R, t, 1.0, lc), ref[:3])
        assert ctx.tree_score(None, None, 1.0, lc, want=())[0][0] == n


def multi_and_batch(ctx, g, lc, rot0, t0, targets, w_multi, w_batch):
    """K = 3 start poses on the record's tree and B = 3 pairs on a forest built from the record's points, five iterations
    each, with traces and score summaries"""
    L = int(g["L"])
    T = hgmm_tree.n_total(L)
    P = g["points"]
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch([P] * 3)
    ctx.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch(targets, weights=w_batch)
    b = ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 5, 0.0, want_trace=True)
    b_sum = ctx.tree_score_batch(b[0], b[1], 1.0, lc)
    resident(ctx, g, targets[0], w_multi)
    m = ctx.tree_register_multi(rot0, t0, 1.0, lc, 5, 0.0, want_trace=True)
    m_sum = ctx.tree_score_multi(m[0], m[1], 1.0, lc)
    flat = lambda r, s: [r[0], r[1], np.asarray(r[2]), np.asarray(r[3]), np.asarray(r[4])] + list(r[5]) + [s]
    return flat(m, m_sum), flat(b, b_sum)


def starts_for(X):
    c = X.mean(axis=0)
    rots = [I3, rot_about([0, 0, 1], 10), rot_about([0, 0, 1], -10)]
    return np.stack(rots), np.stack([c - R @ c for R in rots])


@pytest.mark.parametrize("device_solve", [0, 1])
def test_unit_weights_are_the_unweighted_bits_multi_and_batch(ctx, records, device_solve):
    g = records[2]
    X = g["rot10_target"]
    lc = float(g["lambda_c"])
    rot0, t0 = starts_for(X)
    targets = [X, X[:1500], X[:700]]
    with ctx.config(reg_device_solve=device_solve):
        m_ref, b_ref = multi_and_batch(ctx, g, lc, rot0, t0, targets, None, None)
        m_one, b_one = multi_and_batch(ctx, g, lc, rot0, t0, targets, np.ones(len(X)), [np.ones(len(tg)) for tg in targets])
        for k, (a, b) in enumerate(zip(m_one, m_ref)):
            assert np.array_equal(a, b, equal_nan=True), ("multi", k)
        for k, (a, b) in enumerate(zip(b_one, b_ref)):
            assert np.array_equal(a, b, equal_nan=True), ("batch", k)
        m_w, b_w = multi_and_batch(ctx, g, lc, rot0, t0, targets, weights_for(len(X)), [weights_for(len(tg)) for tg in targets])
        assert not np.array_equal(m_w[0], m_ref[0]) and not np.array_equal(b_w[0], b_ref[0])   # (weights were in force)
        # NULL takes the batch's weights off again, and so do new targets
        ctx.tree_set_target_weights_batch(None)
        # (the serial tree and target moved in between: only the forest's state is asked here)
        b = ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 5, 0.0, want_trace=True)
        assert np.array_equal(b[0], b_ref[0]) and np.array_equal(b[1], b_ref[1])
        ctx.tree_set_target_weights_batch([weights_for(len(tg)) for tg in targets])
        ctx.tree_set_targets_batch(targets)
        b = ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 5, 0.0, want_trace=True)
        assert np.array_equal(b[0], b_ref[0]) and np.array_equal(b[1], b_ref[1])
        assert np.array_equal(ctx.tree_score_batch(b[0], b[1], 1.0, lc), b_ref[-1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. a zero weight is an absent point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
def test_zero_weight_is_an_absent_point(ctx, records, L):
    """The weighted E-step against the E-step of the sub-cloud X[w > 0] under w[w > 0], and against the restatement, at the
    bound of test 1 (the sub-cloud's extent and weight sum may give another encoding: no bitwise claim)."""
    g = records[L]
    X = g["rot10_target"]
    w = weights_for(len(X))
    pos = w > 0
    assert 0 < (~pos).sum() < len(X)
    _, lc, T = resident(ctx, g, X, w)
    full = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    resident(ctx, g, X[pos], w[pos])
    sub = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    o = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, w)
    o_sub = hgmm_tree.reg_e_step(X[pos], g["pi"], g["mu"], g["cov"], L, lc, w[pos])
    for k in range(3):
        np.testing.assert_allclose(full[k], sub[k], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(full[k], o[k], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(sub[k], o_sub[k], rtol=1e-10, atol=1e-12)
    # and the score: the zero-weight points are in the per-point arrays and absent from the sums
    resident(ctx, g, X, w)
    s_full, arr = ctx.tree_score(None, None, 1.0, lc)
    resident(ctx, g, X[pos], w[pos])
    s_sub, arr_sub = ctx.tree_score(None, None, 1.0, lc)
    assert len(arr["node"]) == len(X) and np.array_equal(arr["node"][pos], arr_sub["node"])
    assert np.array_equal(arr["maha2"][pos], arr_sub["maha2"])
    np.testing.assert_allclose(s_full, s_sub, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. batch and multi-start: every member bitwise the serial weighted call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_solve", [0, 1])
@pytest.mark.parametrize("gate", [np.inf, 16.0])
def test_weighted_multi_and_batch_are_bitwise_the_serial_weighted_call(ctx, records, gated, device_solve, gate):
    """B = 3 ragged pairs cut from the L = 4 target (5 032, 3 001 and 1 777 points: the second and third start at unaligned
    places of the forest's arrays), pair 1 without weights; K = 3 start poses on the record's own tree."""
    g = records[4]
    P, X = g["points"], g["rot10_target"]
    L, lc = int(g["L"]), float(g["lambda_c"])
    T = hgmm_tree.n_total(L)
    rot0, t0 = starts_for(X)
    targets = [X, X[1000:4001], X[3255:]]
    assert [len(tg) for tg in targets] == [5032, 3001, 1777] and all(len(tg) % 256 for tg in targets)
    ws = [weights_for(len(targets[0])), None, weights_for(len(targets[2]))]
    idx = np.random.RandomState(72).randint(T, size=T)
    gated(gate)
    with ctx.config(reg_device_solve=device_solve):
        # the forest first: the serial calls below replace the context's resident cloud
        arrs = ctx.set_points_batch([P] * 3)
        ctx.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
        ctx.tree_set_targets_batch(targets, weights=ws)
        b_rot, b_t, b_it, b_q, b_st, b_tr = ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 5, 0.0,
                                                                    want_trace=True)
        b_sum = ctx.tree_score_batch(b_rot, b_t, 1.0, lc)
        ctx.set_points(P)
        pi, mu, cov = ctx.tree_build(L, 20.0, 1e-4, P[idx], 0.004)[:3]
        finals = []
        for b, tg in enumerate(targets):
            ctx.tree_set_nodes(L, pi, mu, cov)
            ctx.tree_set_target(tg)
            if ws[b] is not None:
                ctx.tree_set_target_weights(ws[b])
            s_rot, s_t, s_it, s_q, s_st, s_tr = loop5(ctx, lc)
            finals.append(s_rot)
            assert (int(b_it[b]), int(b_st[b])) == (s_it, s_st), b
            assert np.array_equal(b_rot[b], s_rot) and np.array_equal(b_t[b], s_t), b
            assert (b_q[b] == s_q) or (np.isnan(b_q[b]) and s_q is None), b
            assert np.array_equal(b_tr[b], s_tr), b
            s_sum = ctx.tree_score(s_rot, s_t, 1.0, lc, want=())[0]
            assert np.array_equal(b_sum[b], s_sum), b
            assert s_sum[0] == (len(tg) if ws[b] is None else np.cumsum(ws[b])[-1]), b       # (the sum in index order)
        assert b_it[0] > 0 and b_it[1] > 0 and b_it[2] > 0
        # the unweighted pair is its unweighted serial call (above), and the weights of its neighbours are not its own:
        ctx.tree_set_nodes(L, pi, mu, cov)
        ctx.tree_set_target(targets[0])
        assert not np.array_equal(loop5(ctx, lc)[0], finals[0])
        # multi-start on the record's own tree: the K hypotheses share the one weight array
        resident(ctx, g, X, ws[0])
        m_rot, m_t, m_it, m_q, m_st, m_tr = ctx.tree_register_multi(rot0, t0, 1.0, lc, 5, 0.0, want_trace=True)
        m_sum = ctx.tree_score_multi(m_rot, m_t, 1.0, lc)
        for k in range(3):
            s_rot, s_t, s_it, s_q, s_st, s_tr = ctx.tree_register(rot0[k], t0[k], 1.0, lc, 5, 0.0, None, want_trace=True)
            assert (int(m_it[k]), int(m_st[k])) == (s_it, s_st) and s_it > 0, k
            assert np.array_equal(m_rot[k], s_rot) and np.array_equal(m_t[k], s_t) and m_q[k] == s_q, k
            assert np.array_equal(m_tr[k], s_tr), k
            assert np.array_equal(m_sum[k], ctx.tree_score(s_rot, s_t, 1.0, lc, want=())[0]), k
        ctx.tree_set_target_weights(None)
        free = ctx.tree_register_multi(rot0, t0, 1.0, lc, 5, 0.0, want_trace=True)[5][0]
        assert not np.array_equal(free, m_tr[0])                       # (the weights were in force in the launches above)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the score under weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
def test_score_summary_is_the_weighted_sum_of_its_per_point_terms(ctx, records, L):
    """Slots 0..6 against NumPy sums of w times the per-point terms of the SAME call (identity pose, so |y - mu|^2 is the
    device's term to the last bit); the per-point arrays are the unweighted call's, bit for bit."""
    from hgmm_amd._native import CHI2_3_99
    g = records[L]
    X = g["rot10_target"]
    w = weights_for(len(X))
    _, lc, T = resident(ctx, g, X)
    s0, a0 = ctx.tree_score(None, None, 1.0, lc)
    ctx.tree_set_target_weights(w)
    s, a = ctx.tree_score(None, None, 1.0, lc)
    for k in ("node", "maha2", "logp"):
        assert np.array_equal(a[k], a0[k]), k
    node, maha2, logp = a["node"], a["maha2"], a["logp"]
    inl = maha2 <= CHI2_3_99
    assert 0 < inl.sum() < len(X)
    d2 = ((X - g["mu"][node]) ** 2).sum(axis=1)
    dead = ~np.isfinite(maha2)
    exp = [w.sum(), w[inl].sum(), (w[inl] * maha2[inl]).sum(), (w[inl] * d2[inl]).sum(), (w[inl] * logp[inl]).sum(),
           w[dead].sum(), w[node < hgmm_tree.level(L - 1)].sum()]
    print("L=%d summary %s\n     numpy   %s" % (L, s[:7], np.array(exp)))
    np.testing.assert_allclose(s[:7], exp, rtol=1e-12, atol=0)
    assert s[7] == 0.0 and s[0] != s0[0] and s0[0] == len(X)
    # the mirror: a WeightedPoints target, fitness = weighted inlier share
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, WeightedPoints
    gt = GMMTree(None, tree_level=L, lambda_c=lc, ctx=ctx)
    gt.set_nodes(g["pi"], g["mu"], g["cov"])
    sc = gt.score(WeightedPoints(X, w))
    assert np.array_equal(sc.maha2, maha2) and sc.fitness == s[1] / s[0]
    assert gt.score(X).fitness == s0[1] / s0[0]                        # (and the next target is not scored under them)


@pytest.mark.parametrize("weighted", [False, True])
def test_score_multi_and_batch_read_chunk_count_and_weight_sum_from_the_table(ctx, records, weighted):
    """The score's finish step takes every member's number of 256-point chunks and its weight sum from the member's table
    entry, for K poses of one pair as for B pairs.  K = 3 poses on targets of 256 points (a full last chunk) and of 257 (a
    last chunk of one point); B = 3 pairs of 100, 256 and 257 points, so that each pair's own chunk count (1, 1, 2) is not
    the launch's (2), the middle pair without weights.  Every summary is the serial call's, bit for bit."""
    g = records[2]
    P, X = g["points"], g["rot10_target"]
    L, lc = int(g["L"]), float(g["lambda_c"])
    T = hgmm_tree.n_total(L)
    rot0, t0 = starts_for(X)
    w_for = lambda n: weights_for(n) if weighted else None
    for n in (256, 257):
        w = w_for(n)
        resident(ctx, g, X[:n], w)
        m_sum = ctx.tree_score_multi(rot0, t0, 1.0, lc)
        for k in range(3):
            s_sum = ctx.tree_score(rot0[k], t0[k], 1.0, lc, want=())[0]
            assert np.array_equal(m_sum[k], s_sum), (n, k)
            assert s_sum[0] == (np.cumsum(w)[-1] if weighted else n) and (s_sum[0] != n) == weighted, (n, k)
    targets = [X[:100], X[300:556], X[700:957]]
    assert [len(tg) for tg in targets] == [100, 256, 257]
    ws = [w_for(100), None, w_for(257)]
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch([P] * 3)
    ctx.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch(targets, weights=ws if weighted else None)
    b_sum = ctx.tree_score_batch(rot0, t0, 1.0, lc)
    for b, tg in enumerate(targets):
        ctx.tree_set_nodes(L, *ctx.tree_get_nodes_batch(b, L))
        ctx.tree_set_target(tg)
        ctx.tree_set_target_weights(ws[b])
        s_sum = ctx.tree_score(rot0[b], t0[b], 1.0, lc, want=())[0]
        assert np.array_equal(b_sum[b], s_sum), b
        assert s_sum[0] == (len(tg) if ws[b] is None else np.cumsum(ws[b])[-1]), b


# ---------------------------------------------------------------------------------------------------------------------
# 7. it does what it is for
# ---------------------------------------------------------------------------------------------------------------------
def test_count_weighted_voxel_centroids_reach_the_full_scans_pose(ctx, bunny):
    """bun000's tree (L = 3, product defaults) <- bun045 placed by bun_conf.npz and moved by 8 deg / 5 mm (tools/gate_probe.py's
    pair), maxiter 30, tol 1e-6.  The figure is the mean distance between the scan at the pose its 4 mm voxel centroids
    (1 986 points) give and at the pose the full 40 097-point scan gives.  The NumPy restatement: 1.98 mm unweighted,
    0.29 mm with the voxel counts as weights (ratio 0.15); the bound is a half."""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, WeightedPoints
    from hgmm_amd.pointcloud_io import voxel_down_sample
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
    cen, cnt = voxel_down_sample(moved, 0.004, return_counts=True)
    assert cnt.sum() == len(moved) == 40097
    built = GMMTree(a, tree_level=3, lambda_c=0.01, ls=20, sig2=0.004, ctx=ctx)

    def placed(target, **kw):
        gt = GMMTree(None, tree_level=3, lambda_c=0.01, ctx=ctx)      # (a GMMTree resumes from its last pose: a new one per run)
        gt.set_nodes(built._mixingCoeff, built._mean, built._covar)
        tf = gt.registration(target, 30, 1e-6, **kw).transformation.inverse()      # the loop's own pose: target -> tree
        return moved @ np.asarray(tf.rot).T + np.asarray(tf.t), int(gt.n_iter_)

    full, it_f = placed(moved)
    unweighted, it_u = placed(cen)
    weighted, it_w = placed(cen, weights=cnt)
    d_u = np.linalg.norm(unweighted - full, axis=1).mean()
    d_w = np.linalg.norm(weighted - full, axis=1).mean()
    print("4 mm voxel centroids (%d points) against the full scan's pose: unweighted %.2f mm (%d iterations), "
          "weights = counts %.2f mm (%d iterations), ratio %.2f; the full scan took %d iterations"
          % (len(cen), 1e3 * d_u, it_u, 1e3 * d_w, it_w, d_w / d_u, it_f))
    assert d_w < 0.5 * d_u
    # the carrier is the keyword, and the next unweighted call is not registered under the counts
    again, _ = placed(WeightedPoints(cen, cnt))
    assert np.array_equal(again, weighted)
    assert np.array_equal(placed(cen)[0], unweighted)


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors and state
# ---------------------------------------------------------------------------------------------------------------------
def _dptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_weight_errors_and_state(records):
    import hgmm_amd
    g = records[2]
    X = g["rot10_target"]
    n = len(X)
    L, lc, T = int(g["L"]), float(g["lambda_c"]), hgmm_tree.n_total(2)
    c = hgmm_amd.Context(0)
    try:
        lib, h = c.lib, c.h
        ones = np.ones(n)
        # no resident target: state errors, for the serial and the batch entry, with and without an array
        assert lib.hgmm_tree_set_target_weights(h, _dptr(ones), n) == HGMM_ERR_STATE
        assert lib.hgmm_tree_set_target_weights(h, None, 0) == HGMM_ERR_STATE
        assert b"hgmm_tree_set_target" in lib.hgmm_last_error(h)
        ptrs = (ctypes.c_void_p * 1)(ones.ctypes.data)
        cnts = (ctypes.c_int64 * 1)(n)
        assert lib.hgmm_tree_set_target_weights_batch(h, 1, ptrs, cnts) == HGMM_ERR_STATE
        with pytest.raises(hgmm_amd.HgmmError):
            c.tree_set_target_weights(ones)
        c.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
        c.tree_set_target(X)
        ref = c.tree_reg_estep(T, None, None, 1.0, lc)
        w = weights_for(n)
        assert c.tree_set_target_weights(w) is c
        held = c.tree_reg_estep(T, None, None, 1.0, lc)
        assert not same_bits(held, ref)
        # every rejected call leaves the previous weights in force
        bad = {}
        for name, value in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf), ("negative", -1e-300)):
            v = w.copy()
            v[1234] = value
            bad[name] = (v, n, b"1234")
        bad["all zero"] = (np.zeros(n), n, b"zero")
        bad["short"] = (w[:-1].copy(), n - 1, b"2012")
        bad["long"] = (np.r_[w, 1.0], n + 1, b"2014")
        for name, (v, count, word) in bad.items():
            assert lib.hgmm_tree_set_target_weights(h, _dptr(v), count) == HGMM_ERR_ARG, name
            msg = lib.hgmm_last_error(h)
            assert b"hgmm_tree_set_target_weights" in msg and word in msg, (name, msg)
            assert same_bits(c.tree_reg_estep(T, None, None, 1.0, lc), held), name
            if count == n:
                with pytest.raises(hgmm_amd.HgmmError, match="weight"):
                    c.tree_set_target_weights(v)
        with pytest.raises(ValueError):
            c.tree_set_target_weights(np.ones((n, 1)))
        assert same_bits(c.tree_reg_estep(T, None, None, 1.0, lc), held)
        # zeros among positive weights are fine; an integer array is taken as it comes
        k = np.random.RandomState(11).randint(0, 4, n)
        c.tree_set_target_weights(k)
        assert c.tree_score(None, None, 1.0, lc, want=())[0][0] == k.sum()
        # the build and the flat entries do not see the weights: the same tree with and without
        P = g["points"]
        idx = np.random.RandomState(72).randint(T, size=T)
        c.set_points(P)
        c.tree_set_target(X)
        c.tree_set_target_weights(w)
        with_w = c.tree_build(L, 20.0, 1e-4, P[idx], 0.004)[:3]
        c.tree_set_target_weights(None)
        assert same_bits(c.tree_build(L, 20.0, 1e-4, P[idx], 0.004)[:3], with_w)
        # ---- the batch entry ----
        targets = [X[:700], X[700:1500], X[1500:]]
        arrs = c.set_points_batch([P] * 3)
        c.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
        c.tree_set_targets_batch(targets)
        run = lambda: c.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 3, 0.0, want_trace=True)[:2]
        b_ref = run()
        ws = [weights_for(700), None, weights_for(len(X) - 1500)]
        assert c.tree_set_target_weights_batch(ws) is c
        b_held = run()
        assert not np.array_equal(b_held[0][0], b_ref[0][0]) and np.array_equal(b_held[0][1], b_ref[0][1])

        def raw(ws_, counts):
            p = (ctypes.c_void_p * len(ws_))(*[None if v is None else v.ctypes.data for v in ws_])
            return lib.hgmm_tree_set_target_weights_batch(h, len(ws_), p, (ctypes.c_int64 * len(counts))(*counts))

        good_counts = [700, 800, len(X) - 1500]
        v = ws[2].copy()
        v[77] = -2.0
        assert raw([ws[0], None, v], good_counts) == HGMM_ERR_ARG
        msg = lib.hgmm_last_error(h)
        assert b"target 2" in msg and b"weight 77" in msg, msg
        assert raw([ws[0], None, np.zeros(good_counts[2])], good_counts) == HGMM_ERR_ARG
        assert raw([ws[0], None, ws[2]], [700, 801, good_counts[2]]) == HGMM_ERR_ARG      # (the unweighted pair's count too)
        assert b"counts[1]" in lib.hgmm_last_error(h)
        assert raw([ws[0], None], good_counts[:2]) == HGMM_ERR_ARG                           # B
        with pytest.raises(hgmm_amd.HgmmError):
            c.tree_set_target_weights_batch([ws[0], None, ws[2][:-1]])
        assert same_bits(run(), b_held)                                # the previous weights stayed through all of them
        c.tree_set_target_weights_batch([None, None, None])            # nothing weighted: the unweighted launches
        assert same_bits(run(), b_ref)
        c.tree_set_target_weights_batch(ws)
        c.tree_set_target_weights_batch(None)
        assert same_bits(run(), b_ref)
    finally:
        c.close()


def test_status_2_host_fallback_follows_the_resident_weights(ctx, records):
    """GMMTree's host M-step (what a status-2 iteration falls back to) takes its moments from hgmm_tree_reg_estep on the
    resident target: with weights resident it is the weighted restatement's iteration."""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    g = records[2]
    X = g["rot10_target"]
    w = weights_for(len(X))
    L, lc = int(g["L"]), float(g["lambda_c"])
    gt = GMMTree(None, tree_level=L, lambda_c=lc, ctx=ctx)
    gt.set_nodes(g["pi"], g["mu"], g["cov"])
    gt._device_mstep = False                                           # every iteration through expectation_step + maximization_step
    res = gt.registration(X, 3, 0.0, weights=w)
    tf = res.transformation.inverse()
    o_tr = hgmm_tree.register(X, g["pi"], g["mu"], g["cov"], L, lc, 3, 0.0, w)[3]
    np.testing.assert_allclose(np.asarray(tf.rot), o_tr[2][0], rtol=0, atol=1e-8)
    np.testing.assert_allclose(np.asarray(tf.t), o_tr[2][1], rtol=0, atol=1e-8)
    free = hgmm_tree.register(X, g["pi"], g["mu"], g["cov"], L, lc, 3, 0.0)[3]
    assert np.abs(np.asarray(tf.t) - free[2][1]).max() > 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 9. two ranks on one GPU, a shard of the target and of its weights each
# ---------------------------------------------------------------------------------------------------------------------
SPLIT = 2300


def _rank_inputs(scale=1.0):
    g = load_golden("hgmm_reg_L4.npz")
    X = g["rot10_target"]
    # multiples of 1/8 (some of them zero): both shards' sums and their total are exact, so the all-reduced sum of the
    # weights is the single context's and the encodings agree.  ``scale`` (a power of two) keeps all of that exact.
    w = np.random.RandomState(11).randint(0, 33, len(X)) / 8.0 * scale
    return g, X, w


def _rank_worker(rank, name, q, scale=1.0):
    try:
        import hgmm_amd
        g, X, w = _rank_inputs(scale)
        lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, len(X))
        ctx = hgmm_amd.Context(0)
        ctx.comm_init_host(2, rank, name)
        L, lc = int(g["L"]), float(g["lambda_c"])
        ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
        ctx.tree_set_target(X[lo:hi])
        ctx.tree_set_target_weights(w[lo:hi])
        R, t = rot_about([0.2, 1.0, 0.1], 3.0), np.array([0.002, -0.001, 0.0015])
        out = ctx.tree_reg_estep(hgmm_tree.n_total(L), R, t, 1.0, lc)
        ctx.tree_set_reg_gate(16.0)
        out = out + ctx.tree_reg_estep(hgmm_tree.n_total(L), R, t, 1.0, lc)
        ctx.close()
        q.put((rank, out))
    except BaseException as e:                              # the parent must not wait out its timeout for a dead rank
        import traceback
        q.put((rank, "rank %d failed: %r\n%s" % (rank, e, traceback.format_exc())))
        raise


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -20], ids=["unscaled", "2^-20"])
def test_two_ranks_with_sharded_weights_match_the_single_context(ctx, records, gated, scale):
    """``scale`` 2^-20: the all-reduced sum of the weights is below 1 (about 2^-7), where the encoding's F follows the sum's
    exponent above 61"""
    g, X, w = _rank_inputs(scale)
    assert (w == 0).any() and w[:SPLIT].sum() + w[SPLIT:].sum() == w.sum()
    _, lc, T = resident(ctx, g, X, w)
    R, t = rot_about([0.2, 1.0, 0.1], 3.0), np.array([0.002, -0.001, 0.0015])
    ref = ctx.tree_reg_estep(T, R, t, 1.0, lc)
    gated(16.0)
    ref = ref + ctx.tree_reg_estep(T, R, t, 1.0, lc)
    assert not np.array_equal(ref[0], ref[3])
    name = "hgmm_w_%d_%d" % (os.getpid(), int(np.log2(scale)))
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_rank_worker, args=(r, name, q, scale)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
    assert not any(isinstance(v, str) for v in got.values()), got
    assert all(p.exitcode == 0 for p in procs)
    for rank in (0, 1):
        for k, (a, b) in enumerate(zip(got[rank], ref)):
            assert np.array_equal(a, b), (rank, k)
