"""The score of a cloud against a GMM tree (hgmm_tree_score / hgmm_tree_score_batch, GMMTree.score / predict) against a
float64 NumPy statement of its definition on the SAME node tables.

Definition (include/hgmm.h): every target point y = scale R x + t descends the tree with the decisions of the registration
E-step (oracle/hgmm_tree.py: reg_descent) and is scored at the LAST node s it reaches:
    maha2 = (y - mu_s)^T Sigma_s^-1 (y - mu_s)                     (+inf for a dead node: pi_s = 0 or det Sigma_s < 1e-15)
    logp  = log(pi_s) - log((2 pi)^3 det Sigma_s) / 2 - maha2 / 2  (-inf for a dead node)
and the summary holds n, the inliers (maha2 <= maha2_max), their sums of maha2, |y - mu_s|^2 and logp, the points in dead
nodes and the points that stopped above the last level.

Bounds (derived, not measured):
  node    exact, after dropping the points whose descent has a decision margin below 1e-9 (reg_descent's gap, den_margin,
          cplx_margin; with lambda_c < 0 the complexity test decides nothing and its margin is left out).  An exact tie
          between sibling nodes with bitwise equal parameters is no such margin (twin_free_gap): those points stay, and
          their label must be the first twin;
  maha2   |d| <= (1e-9 + 64 u cond(Sigma_s)) maha2 + 2 sqrt(maha2 lmax(Sigma_s^-1)) delta + lmax(Sigma_s^-1) delta^2,
          u = 2^-53, delta = 4 sqrt(3) u (|y| + |mu_s|): 1e-9 is the tree tests' bound for pdf-derived quantities, the second
          term the forward error of an inverted 3 x 3 covariance, delta how far the device's fused s R x + t and the
          coordinate difference may lie from NumPy's;
  logp    half of that + 1e-12 (1 + |logp|);
  summary points with |maha2 - maha2_max| inside their own bound are left out on both sides; then the counts are equal and
          the three sums agree to 1e-9 sum |term|.
Dropped points (near-ties + points at the inlier bound) are removed from the target BEFORE the device call, as in
tests/test_tree_reg_depth_gpu.py, and may be at most 0.01 % of it.  Every case prints the largest observed ratio of
difference to bound."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import hgmm_tree
from test_tree_reg_depth_gpu import (FAR, LC, TIE, batch_init_idx, batch_pairs, bun_trees, ctx, rot_about,  # noqa: F401
                                     synthetic_target, synthetic_tree)

pytestmark = pytest.mark.gpu

CHI2 = 11.344866730144373            # 0.99 quantile of chi-square with 3 degrees of freedom
U = 2.0 ** -53


def score_ref(Y, pi, mu, cov, L, lc):
    """The definition in NumPy.  -> (node, maha2, logp, r2 = |y - mu_s|^2, near-tie mask)."""
    desc = hgmm_tree.reg_descent(Y, pi, mu, cov, L, lc)
    depth = (desc.node >= 0).sum(axis=1) - 1
    node = desc.node[np.arange(len(Y)), depth]
    ok, inv, coef = hgmm_tree.node_prep(cov)
    d = Y - mu[node]
    w = pi[node] * coef[node]                      # 0 for a dead node
    with np.errstate(invalid="ignore"):
        maha2 = np.where(w > 0, np.einsum('ni,nij,nj->n', d, inv[node], d), np.inf)
        logp = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)) - 0.5 * maha2, -np.inf)
    margin = np.minimum(twin_free_gap(Y, desc, pi, mu, cov), desc.den_margin)
    if lc > 0:
        margin = np.minimum(margin, desc.cplx_margin)
    return node, maha2, logp, (d * d).sum(axis=1), (margin < TIE).any(axis=1)


def twin_free_gap(Y, desc, pi, mu, cov):
    """reg_descent's ``gap`` with the EXACT ties between twins taken out.  A tree built from fewer distinct initial means
    than nodes has sibling nodes with bitwise equal (pi, mu, cov) below a flat parent (the registration never goes there,
    ``predict`` does): their g are the same number on either side, so "the first maximum" is no matter of rounding and both
    sides must take the first twin.  For a decision with gap == 0 whose maximum is shared by such twins only, the gap
    returned is the one to the best child with OTHER parameters (1 when there is none above 0)."""
    gap = desc.gap.copy()
    ok, inv, coef = hgmm_tree.node_prep(cov)
    for i, l in zip(*np.nonzero(desc.gap == 0.0)):
        kids = hgmm_tree.child(desc.node[i, l - 1] if l else -1) + np.arange(8)
        g = pi[kids] * hgmm_tree.pdf_pairs(Y[i][None, :], mu[kids], inv[kids], coef[kids])
        s = desc.node[i, l]
        twin = np.array([pi[k] == pi[s] and np.array_equal(mu[k], mu[s]) and np.array_equal(cov[k], cov[s]) for k in kids])
        assert twin[s - kids[0]] and g[s - kids[0]] == g.max() and s == kids[np.argmax(g)]
        if (g[twin] == g.max()).all():
            rest = g[~twin].max() if (~twin).any() else 0.0
            gap[i, l] = (g.max() - rest) / g.max()
    return gap


def maha2_bound(Y, node, maha2, mu, cov):
    """The bound of the module docstring, per point (inf where maha2 is)."""
    lam = np.linalg.eigvalsh(cov[node])
    live = np.isfinite(maha2)
    lmin = np.where(live, lam[:, 0], 1.0)
    cond, imax = lam[:, 2] / lmin, 1.0 / lmin
    delta = 4 * np.sqrt(3.0) * U * (np.linalg.norm(Y, axis=1) + np.linalg.norm(mu[node], axis=1))
    m = np.where(live, maha2, 0.0)
    b = (1e-9 + 64 * U * cond) * m + 2 * np.sqrt(m * imax) * delta + imax * delta ** 2
    return np.where(live, b, np.inf)


def summary_ref(node, maha2, logp, r2, pi, cov, L, maha2_max):
    inl = maha2 <= maha2_max
    dead = ~(pi[node] * hgmm_tree.node_prep(cov)[2][node] > 0)
    ints = np.array([len(node), inl.sum(), dead.sum(), (node < hgmm_tree.level(L - 1)).sum()], dtype=np.float64)
    sums = np.array([maha2[inl].sum(), r2[inl].sum(), logp[inl].sum()])
    mags = np.array([np.abs(maha2[inl]).sum(), np.abs(r2[inl]).sum(), np.abs(logp[inl]).sum()])
    return ints, sums, mags


def kept_points(X, R, t, scale, pi, mu, cov, L, lc, maha2_max, label, allow=None):
    """Mask of the target points that stay: no near-tie in the descent, not at the inlier bound.  ``allow``: the largest
    number that may be dropped (default 0.01 % of the target)."""
    Y = scale * (X @ R.T) + t
    node, maha2, logp, r2, tie = score_ref(Y, pi, mu, cov, L, lc)
    edge = np.abs(np.where(np.isfinite(maha2), maha2, np.inf) - maha2_max) <= maha2_bound(Y, node, maha2, mu, cov)
    edge &= np.isfinite(maha2)
    drop = tie | edge
    print("%s: %d near-ties, %d points at the inlier bound, of %d" % (label, tie.sum(), edge.sum(), len(X)))
    assert drop.sum() <= (1e-4 * len(X) if allow is None else allow), label
    return ~drop


def compare(summary, arrays, Y, pi, mu, cov, L, lc, maha2_max, label):
    """Device results for the moved target Y (no near-ties left in it) against the definition."""
    node, maha2, logp, r2, tie = score_ref(Y, pi, mu, cov, L, lc)
    assert not tie.any()
    bound = maha2_bound(Y, node, maha2, mu, cov)
    if "node" in arrays:
        assert arrays["node"].dtype == np.int32
        assert np.array_equal(arrays["node"], node), "%s: %d labels differ" % (label, (arrays["node"] != node).sum())
    fin = np.isfinite(maha2)
    ratio_m = ratio_l = 0.0
    if "maha2" in arrays:
        assert np.array_equal(np.isposinf(arrays["maha2"]), ~fin), label
        dm = np.abs(arrays["maha2"][fin] - maha2[fin])
        ratio_m = float((dm / bound[fin]).max()) if fin.any() else 0.0
        assert (dm <= bound[fin]).all(), "%s maha2: largest difference / bound %.3g" % (label, ratio_m)
    if "logp" in arrays:
        assert np.array_equal(np.isneginf(arrays["logp"]), ~fin), label
        bl = 0.5 * bound[fin] + 1e-12 * (1 + np.abs(logp[fin]))
        dl = np.abs(arrays["logp"][fin] - logp[fin])
        ratio_l = float((dl / bl).max()) if fin.any() else 0.0
        assert (dl <= bl).all(), "%s logp: largest difference / bound %.3g" % (label, ratio_l)
    ints, sums, mags = summary_ref(node, maha2, logp, r2, pi, cov, L, maha2_max)
    s = np.asarray(summary)
    assert s.shape == (8,) and s[7] == 0.0
    assert np.array_equal(s[[0, 1, 5, 6]], ints), "%s: counts %s, definition %s" % (label, s[[0, 1, 5, 6]], ints)
    ds = np.abs(s[2:5] - sums)
    ratio_s = float((ds / np.maximum(1e-9 * mags, 1e-300)).max()) if ints[1] else 0.0
    print("%s: n %d, inliers %d, dead %d, above the leaf level %d; difference / bound: maha2 %.3g, logp %.3g, sums %.3g"
          % (label, ints[0], ints[1], ints[2], ints[3], ratio_m, ratio_l, ratio_s))
    assert (ds <= 1e-9 * mags).all(), "%s: sums %s, definition %s" % (label, s[2:5], sums)
    return node, maha2, ints


def check_score(ctx, pi, mu, cov, L, X, R, t, scale, lc, label, maha2_max=CHI2, allow=None):
    keep = kept_points(X, R, t, scale, pi, mu, cov, L, lc, maha2_max, label, allow)
    X = X[keep]
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(X)
    summary, arrays = ctx.tree_score(R, t, scale, lc, maha2_max)
    assert set(arrays) == {"node", "maha2", "logp"} and all(len(a) == len(X) for a in arrays.values())
    out = compare(summary, arrays, scale * (X @ R.T) + t, pi, mu, cov, L, lc, maha2_max, label)
    # only what is asked for is returned, and the summary does not depend on it
    s2, a2 = ctx.tree_score(R, t, scale, lc, maha2_max, want=("maha2",))
    assert set(a2) == {"maha2"} and s2.tobytes() == summary.tobytes() and a2["maha2"].tobytes() == arrays["maha2"].tobytes()
    s3, a3 = ctx.tree_score(R, t, scale, lc, maha2_max, want=())
    assert a3 == {} and s3.tobytes() == summary.tobytes()
    return out


I3, Z3 = np.identity(3), np.zeros(3)


# ---------------------------------------------------------------------------------------------------------------------
# 1. synthetic trees: stops at every depth, dead nodes, the forced first child
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lc", [LC, -1.0])
@pytest.mark.parametrize("L,seed", [(1, 11), (3, 13), (4, 14), (5, 15), (6, 16)])
def test_score_synthetic_tree_matches_definition(ctx, L, seed, lc):
    pi, mu, cov, live = synthetic_tree(L, seed)
    X = synthetic_target(pi, mu, cov, live, L, 20000, seed)
    # (these inputs have no near-tie and no point at the inlier bound: nothing may be dropped)
    node, maha2, ints = check_score(ctx, pi, mu, cov, L, X, I3, Z3, 1.0, lc, "synthetic L=%d lambda_c=%g" % (L, lc), allow=0)
    lvl = np.searchsorted([hgmm_tree.level(l + 1) for l in range(L)], node, side="right")
    per_level = np.bincount(lvl, minlength=L)
    print("L=%d lambda_c=%g: points per level of their node %s" % (L, lc, per_level.tolist()))
    if lc > 0:
        assert (per_level > 0).all()                       # stops at every depth
    else:
        assert per_level[L - 1] == len(node) and ints[3] == 0
    assert 0 < ints[1] < ints[0]                           # inliers and outliers both occur
    if L > 1:
        assert ints[2] > 0                                 # points end in dead nodes (level 0 has none)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a pose applied on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.5, 2.0])
def test_score_with_pose_and_scale_on_device(ctx, s):
    L = 4
    pi, mu, cov, live = synthetic_tree(L, 14)
    X = synthetic_target(pi, mu, cov, live, L, 20000, 14)
    R = rot_about([0.3, -1.0, 0.5], 17.0)
    t = np.array([0.05, -0.02, 0.03])
    Xs = ((X - t) @ R) / s                                  # s R Xs + t == X up to rounding
    check_score(ctx, pi, mu, cov, L, Xs, R, t, s, LC, "synthetic L=4 scale %g" % s)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the reference's own L = 4 records: the fitness tells the aligned run from the failed one
# ---------------------------------------------------------------------------------------------------------------------
def test_score_reference_records_L4(ctx):
    from hgmm_amd.hgmm.hgmm_gpu import tree_score_from_summary
    g = load_golden("hgmm_reg_L4.npz")
    L, lc = int(g["L"]), float(g["lambda_c"])
    pi, mu, cov = g["pi"], g["mu"], g["cov"]
    expect = {10: ("0.538", "0.940"), 30: ("0.197", "0.457")}
    for deg in (10, 30):
        tag = "rot%d_" % deg
        target = g[tag + "target"]
        # the records hold tf.inverse(); the pose that moves the target onto the tree is its inverse
        R = g[tag + "final_rot"].T
        t = -(R @ g[tag + "final_t"])
        fit = []
        for (Rp, tp), what in (((I3, Z3), "start"), ((R, t), "final")):
            label = "reference L=4 rot%d %s" % (deg, what)
            keep = kept_points(target, Rp, tp, 1.0, pi, mu, cov, L, lc, CHI2, label, allow=0)
            assert keep.all()
            ctx.tree_set_nodes(L, pi, mu, cov)
            ctx.tree_set_target(target)
            summary, arrays = ctx.tree_score(Rp, tp, 1.0, lc, CHI2)
            node, maha2, ints = compare(summary, arrays, target @ Rp.T + tp, pi, mu, cov, L, lc, CHI2, label)
            sc = tree_score_from_summary(summary, arrays)
            assert sc.n_points == len(target) and sc.n_inliers == int(ints[1])
            assert sc.fitness == ints[1] / ints[0]           # counts: exactly the definition's
            fit.append(sc.fitness)
        print("rot%d: fitness %.3f -> %.3f" % (deg, fit[0], fit[1]))
        assert ("%.3f" % fit[0], "%.3f" % fit[1]) == expect[deg]
        assert fit[1] > fit[0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. trees built on the GPU, through GMMTree.score and GMMTree.predict
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["4", "5", "4far"])
def test_score_and_predict_bunny_tree(ctx, bun_trees, key):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, RigidTransformation, node_level
    P, L, pi, mu, cov = bun_trees[key]
    gt = GMMTree(None, tree_level=L, lambda_c=LC, ctx=ctx)
    gt.set_nodes(pi, mu, cov)
    c = P.mean(axis=0)
    R = rot_about([0.2, 1.0, 0.1], 4.0)
    t = c - R @ c + np.array([0.002, -0.001, 0.0015])
    for X, given, label in ((P, None, "bun000 L=%s itself" % key),
                            (P[::2], RigidTransformation(R, t).inverse(), "bun000 L=%s moved by 4 deg" % key)):
        # GMMTree.score takes what registration() returns (the inverse) and inverts it: the pose it applies
        pose = given.inverse() if given is not None else RigidTransformation(I3, Z3)
        Rp, tp, sp = np.asarray(pose.rot), np.asarray(pose.t), float(pose.scale)
        keep = kept_points(X, Rp, tp, sp, pi, mu, cov, L, LC, CHI2, label)
        X = X[keep]
        sc = gt.score(X, given)
        summary = np.array([sc.n_points, sc.n_inliers, 0, 0, 0, sc.n_dead, sc.n_above_leaf, 0], dtype=np.float64)
        node, maha2, logp, r2, _ = score_ref(sp * (X @ Rp.T) + tp, pi, mu, cov, L, LC)
        ints, sums, mags = summary_ref(node, maha2, logp, r2, pi, cov, L, CHI2)
        summary[2:5] = sums                                  # (checked through the three means below)
        compare(summary, {"node": sc.node, "maha2": sc.maha2, "logp": sc.logp}, sp * (X @ Rp.T) + tp, pi, mu, cov, L, LC, CHI2,
                label)
        assert sc.fitness == ints[1] / ints[0]
        np.testing.assert_allclose(sc.mahalanobis_rms, np.sqrt(sums[0] / ints[1]), rtol=1e-9, err_msg=label)
        np.testing.assert_allclose(sc.inlier_rmse, np.sqrt(sums[1] / ints[1]), rtol=1e-9, err_msg=label)
        np.testing.assert_allclose(sc.mean_log_density, sums[2] / ints[1], rtol=1e-9 * mags[2] / abs(sums[2]), err_msg=label)
        assert np.array_equal(node_level(sc.node) < L - 1, sc.node < hgmm_tree.level(L - 1))
        lean = gt.score(X, given, per_point=False)
        assert lean.node is None and lean.maha2 is None and lean.logp is None and lean[:8] == sc[:8]
        print("%s: fitness %.4f, inlier rmse %.3g, Mahalanobis rms %.3f" % (label, sc.fitness, sc.inlier_rmse, sc.mahalanobis_rms))
    # predict: a node of the last level for every point, the definition with lambda_c < 0 -- NOT the build's currentIdx,
    # which assigns within the parent chosen one level up with that level's parameters
    keep = kept_points(P, I3, Z3, 1.0, pi, mu, cov, L, -1.0, CHI2, "bun000 L=%s predict" % key)
    lab = gt.predict(P[keep])
    ref = score_ref(P[keep], pi, mu, cov, L, -1.0)[0]
    assert lab.dtype == np.int32 and np.array_equal(lab, ref)
    assert (lab >= hgmm_tree.level(L - 1)).all() and (node_level(lab) == L - 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism, the batch, and the registration entry points
# ---------------------------------------------------------------------------------------------------------------------
def test_score_is_deterministic(ctx):
    pi, mu, cov, live = synthetic_tree(5, 15)
    X = synthetic_target(pi, mu, cov, live, 5, 20000, 15)
    ctx.tree_set_nodes(5, pi, mu, cov)
    ctx.tree_set_target(X)
    R, t = rot_about([0.3, -1.0, 0.5], 1.0), np.array([0.01, 0.0, -0.01])
    s1, a1 = ctx.tree_score(R, t, 1.0, LC)
    s2, a2 = ctx.tree_score(R, t, 1.0, LC)
    assert s1.tobytes() == s2.tobytes()
    for k in a1:
        assert a1[k].tobytes() == a2[k].tobytes(), k


def test_score_batch_is_bitwise_the_serial_call(ctx, bunny):
    pairs = batch_pairs(bunny)
    L = 4
    idx = batch_init_idx(pairs, L)
    B = len(pairs)
    arrs = ctx.set_points_batch([s for s, _ in pairs])
    ctx.tree_build_batch([len(a) for a in arrs], L, 20, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch([t for _, t in pairs])
    rot, t, iters, q, status, _ = ctx.tree_register_batch(np.tile(I3, (B, 1, 1)), np.zeros((B, 3)), 1.0, LC, 20, 1e-4)
    assert rot.shape == (B, 3, 3) and t.shape == (B, 3)
    sums = ctx.tree_score_batch(rot, t, 1.0, LC)
    again = ctx.tree_score_batch(rot, t, 1.0, LC)
    assert sums.shape == (B, 8) and sums.tobytes() == again.tobytes()
    start = ctx.tree_score_batch(None, None, 1.0, LC)
    for b in range(B):
        ctx.tree_set_nodes(L, *ctx.tree_get_nodes_batch(b, L))
        ctx.tree_set_target(pairs[b][1])
        alone, _ = ctx.tree_score(rot[b], t[b], 1.0, LC)
        assert alone.tobytes() == sums[b].tobytes(), (b, alone, sums[b])
        assert ctx.tree_score(None, None, 1.0, LC, want=())[0].tobytes() == start[b].tobytes(), b
        assert alone[0] == len(pairs[b][1])
        print("pair %d: fitness %.3f at the start, %.3f after %d iterations" % (b, start[b][1] / start[b][0], alone[1] / alone[0], iters[b]))
        assert alone[1] > start[b][1]
    with pytest.raises(ValueError):
        ctx.tree_score_batch(rot[:2], t[:2], 1.0, LC)


def test_registration_scores_batch_serial_and_score_agree(ctx, bunny):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, ScoredResult, TreeScore, registration_gmmtree, registration_gmmtree_batch
    pairs = batch_pairs(bunny)
    L = 4
    kw = {"init_idx": batch_init_idx(pairs, L), "tree_level": L}
    res, info = registration_gmmtree_batch(pairs, maxiter=20, tol=1e-4, ctx=ctx, return_info=True, score=True, **kw)
    plain, plain_info = registration_gmmtree_batch(pairs, maxiter=20, tol=1e-4, ctx=ctx, return_info=True, **kw)
    assert "score" not in plain_info and len(info["score"]) == len(pairs)
    for k, (s, tg) in enumerate(pairs):
        one = registration_gmmtree(s, tg, 20, 1e-4, ctx=ctx, return_score=True, **kw)
        assert isinstance(one, ScoredResult) and isinstance(one.score, TreeScore) and isinstance(info["score"][k], TreeScore)
        assert np.array_equal(one.transformation.rot, res[k].transformation.rot)
        assert np.array_equal(one.transformation.rot, plain[k].transformation.rot)
        # the scalar fields: bit for bit (the per-point arrays are the serial call's alone)
        assert one.score[:8] == info["score"][k][:8], (k, one.score[:8], info["score"][k][:8])
        assert info["score"][k].node is None and len(one.score.node) == len(tg)
        # GMMTree.score of the RETURNED transformation: its inverse's inverse, equal to the loop's pose to rounding
        gt = GMMTree(s, ctx=ctx, **kw)
        sc = gt.score(tg, one.transformation)
        same = sc.node == one.score.node
        assert (~same).sum() <= 1e-4 * len(tg)
        pose = one.transformation.inverse()
        Y = float(pose.scale) * (tg @ np.asarray(pose.rot).T) + np.asarray(pose.t)
        fin = same & np.isfinite(one.score.maha2)
        assert np.array_equal(np.isfinite(sc.maha2[same]), np.isfinite(one.score.maha2[same]))
        bound = maha2_bound(Y, one.score.node, one.score.maha2, gt._mean, gt._covar)
        d = np.abs(sc.maha2[fin] - one.score.maha2[fin])
        print("pair %d: fitness %.4f; score() vs return_score: largest maha2 difference / bound %.3g"
              % (k, one.score.fitness, (d / bound[fin]).max()))
        assert (d <= bound[fin]).all()
        assert abs(sc.n_inliers - one.score.n_inliers) <= 1e-4 * len(tg)
    # the default leaves the return value as it was
    assert not isinstance(registration_gmmtree(pairs[0][0], pairs[0][1], 20, 1e-4, ctx=ctx, **kw), ScoredResult)


def test_register_pairs_forwards_the_score(bunny):
    from hgmm_amd.hgmm.hgmm_gpu import ScoredResult
    from hgmm_amd.replicas import register_pairs
    pairs = batch_pairs(bunny)[:3]
    kw = {"init_idx": batch_init_idx(pairs, 4), "tree_level": 4}
    one = register_pairs(pairs, devices=[0], score=True, **kw)
    batched = register_pairs(pairs, devices=[0], batch=2, score=True, **kw)
    plain = register_pairs(pairs, devices=[0], batch=2, **kw)
    assert len(one) == len(batched) == len(plain) == len(pairs)
    for a, b, c in zip(one, batched, plain):
        assert isinstance(a, ScoredResult) and isinstance(b, ScoredResult) and not isinstance(c, ScoredResult)
        assert np.array_equal(a.transformation.rot, b.transformation.rot) and np.array_equal(a.transformation.rot, c.transformation.rot)
        assert a.score[:8] == b.score[:8] and 0.0 < a.score.fitness <= 1.0
        assert b.score.node is None and a.score.node is not None
    with pytest.raises(ValueError):
        register_pairs(pairs, devices=[0], method="gmmreg", score=True)


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_score_errors_name_their_cause():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    try:
        pi, mu, cov, live = synthetic_tree(1, 11)
        X = synthetic_target(pi, mu, cov, live, 1, 500, 11)
        with pytest.raises(hgmm_amd.HgmmError, match="(?i)target"):
            c.tree_score()
        with pytest.raises(hgmm_amd.HgmmError, match="(?i)forest"):
            c.tree_score_batch()
        c.tree_set_target(X)
        with pytest.raises(hgmm_amd.HgmmError, match="(?i)no tree"):
            c.tree_score()
        c.tree_set_nodes(1, pi, mu, cov)
        with pytest.raises(hgmm_amd.HgmmError, match="NaN"):
            c.tree_score(maha2_max=float("nan"))
        with pytest.raises(ValueError):
            c.tree_score(want=("nodes",))
        summary, _ = c.tree_score()
        assert summary[0] == len(X)
    finally:
        c.close()


def test_score_non_finite_point_is_never_an_inlier(ctx):
    pi, mu, cov, live = synthetic_tree(3, 13)
    X = synthetic_target(pi, mu, cov, live, 3, 2000, 13)
    ctx.tree_set_nodes(3, pi, mu, cov)
    ctx.tree_set_target(X)
    clean, a0 = ctx.tree_score(None, None, 1.0, LC)
    bad = X.copy()
    rows = [5, 700, 1999]
    bad[5, 0] = np.nan
    bad[700, 2] = np.inf
    bad[1999] = [-np.inf, np.nan, 0.0]
    ctx.tree_set_target(bad)
    for bound in (CHI2, np.inf):
        s, a = ctx.tree_score(None, None, 1.0, LC, bound)
        assert not np.isfinite(a["maha2"][rows]).any() and not (a["maha2"][rows] <= bound).any()
        assert not np.isfinite(a["logp"][rows]).any()
        others = np.setdiff1d(np.arange(len(X)), rows)
        for k in a:
            assert np.array_equal(a[k][others], a0[k][others]), k
        assert s[0] == len(X) and s[1] == (a["maha2"][others] <= bound).sum()
    s, a = ctx.tree_score(None, None, 1.0, LC, CHI2)
    assert s[1] == clean[1] - (a0["maha2"][rows] <= CHI2).sum()
