"""Tree registration at the depths the product runs by default (L = 4, 5, 6) against the float64 oracle.

The registration E-step (tree_reg_estep_body) sums the moments of levels 0-2 (nodes < 584) in LDS and every deeper node
through global 64-bit atomics, and the normal-equation pass and the forest tables scale with T = 4 680 / 37 448 / 299 592:
those paths run only at L >= 4.  Every check here compares the HIP path with oracle/hgmm_tree.py on the SAME node tables
(trees built on the GPU or uploaded; the oracle's own build is O(N 8^L)), with the bounds of the L = 2 tests
(test_tree_gpu.py) unless a derivation next to a bound says otherwise.

Near-ties: the device evaluates its exponentials from a table and computes the node complexity its own way, so a point
whose two best children differ by ~1 ulp may legitimately go the other way.  Single-call tests drop the points with a
decision margin below 1e-9 (relative) at any level (hgmm_tree.reg_descent) and assert that these are at most 0.01 % of
the target; loop tests assert that no such point occurs at any pose they visit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import hgmm_tree

pytestmark = pytest.mark.gpu

LC = 0.01
LDS_NODES = hgmm_tree.level(3)            # 584: levels 0-2 are summed in LDS, deeper nodes through global atomics
TIE = 1e-9
FAR = np.array([40.0, -25.0, 3.0])         # a LiDAR-scale offset (m)


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def rot_about(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def moved(P, deg, axis, shift):
    """P rotated by ``deg`` about ``axis`` through its centroid, then shifted."""
    c = P.mean(axis=0)
    return (P - c) @ rot_about(axis, deg).T + c + np.asarray(shift)


@pytest.fixture(scope="module")
def bun_trees(ctx, bunny):
    """Trees the product builds by default (ls = 20, sig2 = 0.004, seed 72) on the full bun000 scan: L = 4 and 5 near the
    origin, L = 4 with the scan moved by FAR."""
    from hgmm_amd.hgmm.hgmm_gpu import buildGMMTree
    P = bunny.astype(np.float64)
    out = {}
    for key, L, off in (("4", 4, 0.0), ("5", 5, 0.0), ("4far", 4, FAR)):
        out[key] = (P + off, L) + tuple(buildGMMTree(P + off, L, 20, 1e-4, sig2=0.004, ctx=ctx))
    return out


def synthetic_tree(L, seed):
    """A node table with every decision of the descent exercised at every level: per level a quarter of the live nodes
    is flat (complexity below lambda_c: the descent stops there), some of them singular (det < 1e-15: pdf 0), some sibling
    groups are dead as a whole and some nodes alone (pi = 0, mu = 0, cov = I, as the build leaves them; the subtree of a
    dead node is dead).  Children sit around their parent at 0.45 of its scale, inside [0.1, 1.5]^3 (coordinates away
    from 0 keep the moments' off-diagonal entries away from 0, where only an absolute bound could hold)."""
    rs = np.random.RandomState(seed)
    T = hgmm_tree.n_total(L)
    pi, mu, cov = np.zeros(T), np.zeros((T, 3)), np.tile(np.eye(3), (T, 1, 1))
    live = np.zeros(T, dtype=bool)
    corners = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], dtype=np.float64) * 2 - 1
    sig0 = 0.5
    for l in range(L):
        j = np.arange(hgmm_tree.level(l), hgmm_tree.level(l + 1))
        parent = j // 8 - 1
        n = len(j)
        if l == 0:
            p_live, p_mu, p_pi = np.ones(n, bool), np.full((n, 3), 0.8), np.ones(n)
        else:
            p_live, p_mu, p_pi = live[parent], mu[parent], pi[parent]
            groups = rs.rand(n // 8) < 0.12                         # whole sibling groups dead
            p_live = p_live & ~np.repeat(groups, 8)
        alive = p_live & ((rs.rand(n) > 0.05) | (l == 0))          # and single nodes
        sig_p = sig0 * 0.45 ** l
        off = sig_p * (0.9 * corners[j % 8] + 0.35 * rs.randn(n, 3))
        w = rs.gamma(2.0, size=(n // 8, 8))
        w = (w / w.sum(axis=1, keepdims=True)).ravel()
        size2 = (sig0 * 0.45 ** (l + 1)) ** 2
        flat = rs.rand(n) < 0.25
        if l == 0:
            flat = np.isin(np.arange(8), (1, 6))                    # (eight nodes: make sure both kinds are there)
        kappa = np.where(flat, LC * rs.uniform(0.05, 0.8, n), rs.uniform(1.5 * LC, 0.2, n))
        kappa = np.where(flat & (rs.rand(n) < 0.2) & (l > 0), 1e-13, kappa)   # singular: det < EPS
        a, b = np.ones(n), rs.uniform(0.5, 1.0, n)
        c = kappa * (a + b) / (1.0 - kappa)
        lam = size2 * np.stack([a, b, c], axis=1)
        Q = np.linalg.qr(rs.randn(n, 3, 3))[0]
        C = np.einsum('nij,nj,nkj->nik', Q, lam, Q)
        mu[j] = np.where(alive[:, None], p_mu + off, 0.0)
        cov[j] = np.where(alive[:, None, None], C, np.eye(3))
        pi[j] = np.where(alive, p_pi * w, 0.0)
        live[j] = alive
    return pi, mu, cov, live


def synthetic_target(pi, mu, cov, live, L, n, seed, n_out=300):
    """Points drawn from live nodes of every level (deep levels favoured), plus far outliers whose normaliser is below
    TREE_EPS at the first level (the descent then takes the first child of every group)."""
    rs = np.random.RandomState(seed + 1000)
    nodes = np.nonzero(live & (pi > 0))[0]
    lvl = np.searchsorted([hgmm_tree.level(l + 1) for l in range(L)], nodes, side="right")
    w = (lvl + 1.0) ** 2
    pick = rs.choice(nodes, size=n, p=w / w.sum())
    lam, vec = np.linalg.eigh(cov[pick])
    z = rs.randn(n, 3) * np.sqrt(np.maximum(lam, 0.0))
    X = mu[pick] + np.einsum('nij,nj->ni', vec, z)
    d = rs.randn(n_out, 3)
    out = 0.8 + 6.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([X, out])


def drop_near_ties(Y, pi, mu, cov, L, label):
    """-> (keep mask, descent of the kept points).  Asserts that at most 0.01 % of the points were dropped."""
    desc = hgmm_tree.reg_descent(Y, pi, mu, cov, L, LC)
    tie = hgmm_tree.reg_near_ties(desc, TIE)
    print("%s: %d of %d target points dropped as near-ties (margin < %g)" % (label, tie.sum(), len(Y), TIE))
    assert tie.sum() <= 1e-4 * len(Y)
    keep = ~tie
    return keep, hgmm_tree.RegDescent(*[a[keep] for a in desc])


def assert_reaches_deep_nodes(desc, L, label, at_least=50):
    """The (point, node) pairs that add to the moments, per level; at L >= 4 enough of them at nodes >= 584."""
    per_level = desc.contrib.sum(axis=0)
    deep = int((desc.contrib & (desc.node >= LDS_NODES)).sum())
    first_child = int((~np.isfinite(desc.gap[:, 0])).sum())
    print("%s: contributing pairs per level %s, at nodes >= %d: %d; forced first child at level 0: %d"
          % (label, per_level.tolist(), LDS_NODES, deep, first_child))
    if L >= 4:
        assert deep >= at_least
    return per_level


def m2_quantum_bound(desc, mu, T, X, R, t, scale):
    """Per node, the most the fixed-point encoding can move m2: the device adds every contribution as integers in units of
    2^-F (m0), D 2^-F (c1 about the node mean) and D^2 2^-F (C2 about the node mean), D = the extent of the moved target
    about any node mean rounded up to a power of two, F = 62 - bits(n) (reg_extent / reg_encoding in csrc/tree_device.h).
    Each rounding is at most half a unit, so m2 = C2 + c1 mu^T + mu c1^T + m0 mu mu^T is off by at most
    k_j 2^-F (D + |mu_j|)^2 / 2 after k_j contributions.  At the bunny's scale (D = 1) this is below the L = 2 bounds; the
    outliers of the synthetic targets push D to 16, and m2 entries of nodes with little mass then need it."""
    D, F = encoding(X, R, t, scale, mu)
    k = np.bincount(desc.node[desc.contrib], minlength=T).astype(np.float64)
    return (k * 2.0 ** -F * (D + np.linalg.norm(mu, axis=1)) ** 2 / 2)[:, None, None], D


def encoding(X, R, t, scale, mu):
    """(D, F) of the registration E-step's fixed-point sums for target X at pose (R, t, scale) (reg_extent / reg_encoding)."""
    ext = abs(scale) * np.sqrt((R * R).sum()) * np.sqrt((X * X).sum(axis=1)).max() + np.linalg.norm(t) + \
        np.sqrt((mu * mu).sum(axis=1)).max()
    return 2.0 ** np.frexp(ext)[1], 62 - int(len(X)).bit_length()


U = np.finfo(np.float64).eps / 2


def solution_tolerance(m0, m1, mu, cov, k, D, F, x):
    """How far the library's twist x may lie from the reference's lstsq solution (max norm):
      1e-9                 the L = 2 bound;
      cond(A^T A) u |x|    the library solves the normal equations, the reference the stacked system by lstsq: the
                           forward error of a normal-equation solution is of order cond(A^T A) u |x| (Higham, Accuracy and
                           Stability of Numerical Algorithms, 20.4), lstsq's smaller by a factor cond(A).
    Near the origin (cond ~ 5e3) the second term is ~1e-13 and the bound is the L = 2 bound.  Far from it (cond ~ 3e10,
    |x| ~ 4) it is ~1.5e-5; the oracle's own normal-equation and lstsq solutions differ there by 1.4e-8.  The fixed-point
    quantum (D 2^-F per c1 term, ``k`` contributions per node) reaches x only through A^T A and A^T b, which check_normal
    holds to the L = 2 bounds at D = 256 as well; its worst case carried through a system of cond 3e10 is not a useful
    bound, so it is not added here."""
    live = np.nonzero(~(m0 < hgmm_tree.F32_EPS))[0]
    if len(live) == 0:
        return 1e-9
    lam = np.linalg.eigvalsh(hgmm_tree.reg_normal_equations(m0, m1, mu, cov)[0])
    return 1e-9 + lam[-1] / lam[0] * U * np.abs(x).max()


def cholesky_gap(ata, x):
    """What the device's solve (reg_device_solve: Cholesky on the normal equations, reg_device_step) may add to
    solution_tolerance: c cond(A^T A) 2^-52 |x| with c = 8 * 6.  Derived, not measured: a Cholesky solve is backward stable
    (Higham, Accuracy and Stability of Numerical Algorithms, 10.1), so its forward error is of order cond(A^T A) u |x| like
    that of the host's elimination, but the two differ from each other and from lstsq by that much; six unknowns and a handful
    of roundings each give the constant.  ``ata``: the oracle's A^T A at that pose, |x| the max norm of its lstsq twist."""
    lam = np.linalg.eigvalsh(ata)
    return 8 * 6 * lam[-1] / lam[0] * 2.0 ** -52 * np.abs(x).max()


def check_estep(ctx, pi, mu, cov, L, X, R, t, scale, label):
    """ctx.tree_reg_estep with (R, t, scale) on the device, and the drop-in gmmTreeRegESTep on the pre-moved cloud, against
    hgmm_tree.reg_e_step of the moved target (the L = 2 bounds: rtol 1e-10, atol 1e-12; for m2 the atol is the larger of
    1e-12 and the encoding's bound, m2_quantum_bound)."""
    from hgmm_amd.hgmm.hgmm_gpu import gmmTreeRegESTep
    T = hgmm_tree.n_total(L)
    Y = scale * (X @ R.T) + t
    keep, desc = drop_near_ties(Y, pi, mu, cov, L, label)
    X, Y = X[keep], Y[keep]
    assert_reaches_deep_nodes(desc, L, label)
    o = hgmm_tree.reg_e_step(Y, pi, mu, cov, L, LC)
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(X)
    a = ctx.tree_reg_estep(T, R, t, scale, LC)
    np.testing.assert_allclose(ctx.tree_node_complexity(T), hgmm_tree.complexity(cov), rtol=1e-9, atol=1e-12)
    b = gmmTreeRegESTep(Y, pi, mu, cov, L, LC, ctx=ctx)
    for (Xe, Re, te, se), m, what in (((X, R, t, scale), a, ""), ((Y, np.identity(3), np.zeros(3), 1.0), b, "drop-in ")):
        q2, D = m2_quantum_bound(desc, mu, T, Xe, Re, te, se)
        np.testing.assert_allclose(m[0], o[0], rtol=1e-10, atol=1e-12, err_msg="%s %sm0" % (label, what))
        np.testing.assert_allclose(m[1], o[1], rtol=1e-10, atol=1e-12, err_msg="%s %sm1" % (label, what))
        assert (np.abs(m[2] - o[2]) <= 1e-10 * np.abs(o[2]) + np.maximum(1e-12, q2)).all(), \
            "%s %sm2: max |diff| %.3g (D = %g)" % (label, what, np.abs(m[2] - o[2]).max(), D)


# ---------------------------------------------------------------------------------------------------------------------
# 1. registration E-step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,seed", [(1, 11), (3, 13), (4, 14), (5, 15), (6, 16)])
def test_reg_estep_synthetic_tree_matches_oracle(ctx, L, seed):
    pi, mu, cov, live = synthetic_tree(L, seed)
    X = synthetic_target(pi, mu, cov, live, L, 20000, seed)
    desc = hgmm_tree.reg_descent(X, pi, mu, cov, L, LC)
    # the table is what it claims to be: stops at every depth, dead groups, the forced first child
    stopped_at = [int(((desc.node[:, l] >= 0) & (hgmm_tree.complexity(cov)[np.maximum(desc.node[:, l], 0)] <= LC)).sum())
                  for l in range(L)]
    print("L=%d: points stopping at each level %s" % (L, stopped_at))
    assert all(s > 0 for s in stopped_at)
    assert (~np.isfinite(desc.gap[:, 0])).sum() >= 250                  # outliers: den <= TREE_EPS
    if L > 1:
        dead_groups = (pi[8:].reshape(-1, 8) == 0).all(axis=1).sum()
        assert dead_groups > 0
    I3 = np.identity(3)
    check_estep(ctx, pi, mu, cov, L, X, I3, np.zeros(3), 1.0, "synthetic L=%d" % L)
    if L == 4:
        # scale != 1 and a non-trivial (R, t): the device moves the uploaded cloud to where the tree is
        R = rot_about([0.3, -1.0, 0.5], 17.0)
        t = np.array([0.05, -0.02, 0.03])
        for s in (0.5, 2.0):
            Xs = ((X - t) @ R) / s                      # s R Xs + t == X up to rounding
            check_estep(ctx, pi, mu, cov, L, Xs, R, t, s, "synthetic L=4 scale %g" % s)


@pytest.mark.parametrize("key", ["4", "5", "4far"])
def test_reg_estep_bunny_tree_matches_oracle(ctx, bun_trees, key):
    """Trees built on the GPU from the full bun000 scan; the target is the scan itself, moved a few degrees.  ``4far``:
    source and target offset by FAR -- the extent is sqrt(3) 47.3 + 47.3 = 129 m, so D = 256 and F = 46 at n = 40 256: the
    quantum is D 2^-F = 3.6e-12 per c1 term and D^2 2^-F = 9.3e-10 per C2 term.  The m0 / m1 bounds are the L = 2 bounds;
    m2 gets max(1e-12, m2_quantum_bound) as everywhere, but its entries are ~|mu|^2 m0 = 2.2e3 m0, so rtol 1e-10
    (2.2e-7 m0) is what binds."""
    P, L, pi, mu, cov = bun_trees[key]
    c = P.mean(axis=0)
    R = rot_about([0.2, 1.0, 0.1], 4.0)
    t = c - R @ c + np.array([0.002, -0.001, 0.0015])
    check_estep(ctx, pi, mu, cov, L, P, np.identity(3), np.zeros(3), 1.0, "bun000 L=%s identity" % key)
    check_estep(ctx, pi, mu, cov, L, P[::2], R, t, 1.0, "bun000 L=%s moved" % key)


# ---------------------------------------------------------------------------------------------------------------------
# 2. normal equations
# ---------------------------------------------------------------------------------------------------------------------
def check_normal(ctx, pi, mu, cov, L, X, R, t, label):
    """hgmm_tree_reg_normal == the reference's stacked system built from the oracle's moments (the comparisons of
    test_registration_normal_equations_on_device); its solution == lstsq of the stacked system within solution_tolerance."""
    Y = X @ R.T + t
    keep, desc = drop_near_ties(Y, pi, mu, cov, L, label)
    X, Y = X[keep], Y[keep]
    assert_reaches_deep_nodes(desc, L, label)
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(X)
    ata, atb, btb = ctx.tree_reg_normal(R, t, 1.0, LC)
    o_m0, o_m1, _ = hgmm_tree.reg_e_step(Y, pi, mu, cov, L, LC)
    h_ata, h_atb, h_btb, A, b = hgmm_tree.reg_normal_equations(o_m0, o_m1, mu, cov)
    scale = np.sqrt(np.outer(np.diag(h_ata), np.diag(h_ata)))
    np.testing.assert_allclose(ata / scale, h_ata / scale, rtol=0, atol=1e-9, err_msg=label)
    np.testing.assert_allclose(atb, h_atb, rtol=1e-8, atol=1e-9 * np.abs(h_atb).max(), err_msg=label)
    np.testing.assert_allclose(btb, h_btb, rtol=1e-9, err_msg=label)
    x_ref = np.linalg.lstsq(A, b, rcond=-1)[0]
    gap = np.abs(np.linalg.solve(h_ata, h_atb) - x_ref).max()
    lam = np.linalg.eigvalsh(h_ata)
    D, F = encoding(X, R, t, 1.0, mu)
    tol = solution_tolerance(o_m0, o_m1, mu, cov, np.bincount(desc.node[desc.contrib], minlength=len(pi)), D, F, x_ref)
    x = np.linalg.solve(ata, atb)
    print("%s: cond(A^T A) %.3g, |x| %.3g, D %g; oracle normal equations vs lstsq %.3g, library vs lstsq %.3g, bound %.3g"
          % (label, lam[-1] / lam[0], np.abs(x_ref).max(), D, gap, np.abs(x - x_ref).max(), tol))
    np.testing.assert_allclose(x, x_ref, rtol=0, atol=tol, err_msg=label)


@pytest.mark.parametrize("key", ["4", "5", "4far"])
def test_reg_normal_equations_bunny_tree(ctx, bun_trees, key):
    P, L, pi, mu, cov = bun_trees[key]
    c = P.mean(axis=0)
    R = rot_about([1.0, 0.2, -0.3], 6.0)
    t = c - R @ c + np.array([0.004, 0.002, -0.006])
    check_normal(ctx, pi, mu, cov, L, P[::2], R, t, "bun000 L=%s" % key)


def test_reg_normal_equations_synthetic_L6(ctx):
    pi, mu, cov, live = synthetic_tree(6, 26)
    X = synthetic_target(pi, mu, cov, live, 6, 20000, 26, n_out=0)
    check_normal(ctx, pi, mu, cov, 6, X, rot_about([0, 0, 1], 2.0), np.array([0.01, 0.0, -0.01]), "synthetic L=6")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the registration loop, one oracle step at a time
# ---------------------------------------------------------------------------------------------------------------------
def oracle_step(target, pi, mu, cov, L, rot, t, device_solve=0):
    """One reference iteration from pose (rot, t), no near-tie allowed: -> (rot', t', q, tolerances of rot' / t' / q for the
    library's result (solution_tolerance carried through the twist: t' = dR t + v moves by |dw| |t| + |dv|; q = btb - x.Atb
    by |dx| |Atb|), pairs at nodes >= 584).  No node with mass (the target left the tree): x = 0, the pose stays.
    ``device_solve``: the library's solve was the device's -- cholesky_gap on top of solution_tolerance."""
    Y = target @ rot.T + t
    desc = hgmm_tree.reg_descent(Y, pi, mu, cov, L, LC)
    assert not hgmm_tree.reg_near_ties(desc, TIE).any()
    m0, m1, m2 = hgmm_tree.reg_e_step(Y, pi, mu, cov, L, LC)
    r1, t1, q = hgmm_tree.reg_m_step(m0, m1, m2, mu, cov, rot, t)
    deep = int((desc.contrib & (desc.node >= LDS_NODES)).sum())
    if not (~(m0 < hgmm_tree.F32_EPS)).any():
        return r1, t1, q, (1e-9, 1e-9, 0.0), deep
    ata, atb, _, A, b = hgmm_tree.reg_normal_equations(m0, m1, mu, cov)
    x = np.linalg.lstsq(A, b, rcond=-1)[0]
    D, F = encoding(target, rot, t, 1.0, mu)
    tol = solution_tolerance(m0, m1, mu, cov, np.bincount(desc.node[desc.contrib], minlength=len(pi)), D, F, x)
    if device_solve:
        tol += cholesky_gap(ata, x)
    return r1, t1, q, (tol, tol * (1 + np.linalg.norm(t)), tol * np.linalg.norm(atb)), deep


def library_loop(ctx, pi, mu, cov, L, target, budget, device_solve):
    """ctx.tree_register from the identity with tol 0 and a trace, under reg_device_solve = ``device_solve``"""
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(target)
    with ctx.config(reg_device_solve=device_solve):
        return ctx.tree_register(np.identity(3), np.zeros(3), 1.0, LC, budget, 0.0, want_trace=True)


def shadow_poses(poses, target, pi, mu, cov, L, label, device_solve):
    """Every pose k from pose k-1 (the identity first) through one oracle_step == pose k.  -> (largest pose difference, largest
    difference / tolerance, deep pairs per iteration)"""
    r_prev, t_prev = np.identity(3), np.zeros(3)
    worst, ratio, deep = 0.0, 0.0, []
    for k, (r_k, t_k, q_k) in enumerate(poses):
        o_r, o_t, o_q, (tol_r, tol_t, tol_q), n_deep = oracle_step(target, pi, mu, cov, L, r_prev, t_prev, device_solve)
        deep.append(n_deep)
        ratio = max(ratio, np.abs(r_k - o_r).max() / tol_r, np.abs(t_k - o_t).max() / tol_t)
        np.testing.assert_allclose(r_k, o_r, rtol=0, atol=tol_r, err_msg="%s iteration %d" % (label, k))
        np.testing.assert_allclose(t_k, o_t, rtol=0, atol=tol_t, err_msg="%s iteration %d" % (label, k))
        if q_k is not None and np.size(o_q):
            np.testing.assert_allclose(q_k, o_q[0], rtol=1e-7, atol=tol_q, err_msg="%s iteration %d" % (label, k))
        worst = max(worst, np.abs(r_k - o_r).max(), np.abs(t_k - o_t).max())
        r_prev, t_prev = r_k, t_k
    return worst, ratio, deep


def shadow_loop(ctx, pi, mu, cov, L, target, budget, label, device_solve=0):
    """ctx.tree_register(..., tol=0, want_trace=True): every iteration k from the device's pose k-1 through one oracle
    E-step + reg_m_step == the device's pose k ((R, t) within 1e-9 plus the oracle's own normal-equations-vs-lstsq gap at
    that pose, see check_normal; q rtol 1e-7).  An iteration the library hands to the host (status 2) is followed through
    GMMTree's Python path with callbacks.  ``device_solve``: the library calls run under reg_device_solve = 1 and the
    tolerances carry cholesky_gap; the iterations the device did before it handed one over are shadowed as well.
    -> (status, iterations done in the library)"""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    rot, t, done, q, status, trace = library_loop(ctx, pi, mu, cov, L, target, budget, device_solve)
    poses = [(trace[k, :9].reshape(3, 3), trace[k, 9:12], trace[k, 12]) for k in range(done)]
    if status == 2:
        if device_solve:
            shadow_poses(poses, target, pi, mu, cov, L, label + " (before the hand-over)", device_solve)
        with ctx.config(reg_device_solve=device_solve):
            gt = GMMTree(None, tree_level=L, lambda_c=LC, ctx=ctx)
            gt.set_nodes(pi, mu, cov)
            rec = []
            gt.set_callbacks([lambda tf: rec.append((tf.rot.T.copy(), -(tf.rot.T @ tf.t)))])
            gt.registration(target, budget, 0.0)
        poses = [(r, tt, None) for r, tt in rec]
        print("%s: the library handed iteration %d to the host; the Python path is shadowed instead" % (label, done + 1))
        device_solve = 0                                      # (the Python path solves on the host)
    assert len(poses) == budget
    worst, ratio, deep = shadow_poses(poses, target, pi, mu, cov, L, label, device_solve)
    print("%s: %d iterations shadowed (status %d after %d in the library), largest pose difference %.3g = %.3g of its bound, "
          "deep pairs per iteration %s" % (label, budget, status, done, worst, ratio, deep[:4] + ["..."]))
    if L >= 4:
        assert deep[0] > 0
    return status, done


def assert_no_ties_along(target, pi, mu, cov, L, o_tr, device_solve=0):
    """No near-tie at any pose the oracle's registration visited (identity, then every pose but the last).  -> the sum over
    its iterations of solution_tolerance (with ``device_solve`` plus cholesky_gap) carried to the pose (see oracle_step):
    what the final pose may differ by on top of the L = 2 bound."""
    poses = [(np.identity(3), np.zeros(3))] + [(e[0], e[1]) for e in o_tr[:-1]]
    total = 0.0
    for k, ((r, t), e) in enumerate(zip(poses, o_tr)):
        desc = hgmm_tree.reg_descent(target @ r.T + t, pi, mu, cov, L, LC)
        assert not hgmm_tree.reg_near_ties(desc, TIE).any(), k
        m0, m1 = e[3], e[4]
        if (~(m0 < hgmm_tree.F32_EPS)).any():
            ata, _, _, A, b = hgmm_tree.reg_normal_equations(m0, m1, mu, cov)
            x = np.linalg.lstsq(A, b, rcond=-1)[0]
            D, F = encoding(target, r, t, 1.0, mu)
            tol = solution_tolerance(m0, m1, mu, cov, np.bincount(desc.node[desc.contrib], minlength=len(pi)), D, F, x) - 1e-9
            if device_solve:
                tol += cholesky_gap(ata, x)
            total += tol * (1 + np.linalg.norm(t))
    return total


def stop_rule_close(o_tr, tol):
    """Whether |dq| came within 1e-6 relative of tol anywhere on the oracle's path (iterations without q never stop)."""
    qs = [float(np.ravel(e[2])[0]) if np.size(e[2]) else np.nan for e in o_tr]
    dq = np.abs(np.diff(qs))
    return bool(np.any(np.abs(dq - tol) <= 1e-6 * tol)), dq


def check_stop_rule(ctx, pi, mu, cov, L, target, label, maxiter=20, tol=1e-4, device_solve=0):
    """GMMTree.registration without callbacks (the library's loop; an iteration it hands to the host runs there) with the
    reference's stop rule == hgmm_tree.register: same iteration count (unless |dq| came within 1e-6 relative of tol on the
    oracle's path) and final (R, t) within 1e-8 (the L = 2 bound).  ``device_solve``: under reg_device_solve = 1, with
    cholesky_gap per iteration on top."""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    o_rot, o_t, o_q, o_tr = hgmm_tree.register(target, pi, mu, cov, L, LC, maxiter, tol)
    extra = assert_no_ties_along(target, pi, mu, cov, L, o_tr, device_solve)
    gt = GMMTree(None, tree_level=L, lambda_c=LC, ctx=ctx)
    gt.set_nodes(pi, mu, cov)
    with ctx.config(reg_device_solve=device_solve):
        res = gt.registration(target, maxiter, tol)
    close, dq = stop_rule_close(o_tr, tol)
    print("%s: %d iterations (oracle %d), |dq| %s" % (label, gt.n_iter_, len(o_tr), np.array2string(dq, precision=3)))
    if not close:
        assert gt.n_iter_ == len(o_tr)
    # (the returned transform is the inverse: its translation -R^T t moves with |t| |dR| + |dt|)
    np.testing.assert_allclose(res.transformation.rot, o_rot, rtol=0, atol=1e-8 + extra, err_msg=label)
    np.testing.assert_allclose(res.transformation.t, o_t, rtol=0, atol=1e-8 + 2 * extra, err_msg=label)


def scan_pair_target(bunny):
    """bun045 placed with its ground-truth pose of data/bun.conf and moved by 8 deg / 5 mm (test_tree_gpu's scan pair),
    about the origin of the scans' frame."""
    b = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    conf = load_golden("bun_conf.npz")
    pose = conf["poses"][list(conf["names"]).index("bun045.ply")]
    t, (qx, qy, qz, qw) = pose[:3], pose[3:]
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    world = b @ R + t
    return world @ rot_about([0.3, 1.0, 0.2], 8.0).T + np.array([0.005, -0.00375, 0.00625])


@pytest.mark.parametrize("device_solve", [0, 1])
@pytest.mark.parametrize("key", ["4", "5", "4far"])
def test_registration_loop_shadows_oracle(ctx, bun_trees, bunny, key, device_solve):
    """``4far``: the reference linearises the rotation about the ORIGIN (twist x = (w, v)), so a cloud 47 m away takes a
    second-order error of ~|w|^2 |c| / 2 per step -- 18 cm at 5 deg, more than the bunny's size.  The oracle itself then
    overshoots: after one or two iterations no node of the tree receives mass, the system is empty, the library hands that
    iteration to the host (status 2), and the Python path with callbacks has to follow the oracle from there on.  A 0.5 deg
    motion (second-order error ~2 mm) converges far from the origin as well, through the library's own loop.
    ``device_solve`` = 1: the same under reg_device_solve (reg_device_step solves, composes the twist, applies the stop rule
    and gives the verdict); an empty system ends the library's loop with status 2 at the iteration at which it ends the
    host path's."""
    P, L, pi, mu, cov = bun_trees[key]
    off = P[0] - bunny[0].astype(np.float64)
    pairs = {"bunny 5 deg": moved(P[::4], 5.0, [0.2, 1.0, 0.3], [0.003, -0.002, 0.001]),
             "bun.conf scans": scan_pair_target(bunny)[::4] + off}
    if key == "4far":
        pairs["bunny 0.5 deg"] = moved(P[::4], 0.5, [0.2, 1.0, 0.3], [0.003, -0.002, 0.001])
    statuses = {}
    for name, target in pairs.items():
        label = "L=%s %s" % (key, name)
        statuses[name], done = shadow_loop(ctx, pi, mu, cov, L, target, 12, label, device_solve)
        if device_solve:
            host = library_loop(ctx, pi, mu, cov, L, target, 12, 0)
            assert (statuses[name], done) == (host[4], host[2]), (label, statuses[name], done, host[4], host[2])
        check_stop_rule(ctx, pi, mu, cov, L, target, label, device_solve=device_solve)
    if key == "4far":
        assert statuses["bunny 5 deg"] == 2 and statuses["bun.conf scans"] == 2
    else:
        assert set(statuses.values()) == {0}


def test_default_depth_registration_through_gmmtree(ctx, bun_trees, bunny):
    """GMMTree(source).registration(target) with NO tree_level: the default depth (5) is what this pins, against the
    oracle's registration on the same tree."""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    P, L, pi, mu, cov = bun_trees["5"]
    target = moved(P[::4], 5.0, [0.2, 1.0, 0.3], [0.003, -0.002, 0.001])
    gt = GMMTree(P, ctx=ctx)
    assert gt._tree_level == 5 and len(gt._mixingCoeff) == hgmm_tree.n_total(5)
    assert np.array_equal(gt._mixingCoeff, pi) and np.array_equal(gt._mean, mu) and np.array_equal(gt._covar, cov)
    res = gt.registration(target)
    o_rot, o_t, o_q, o_tr = hgmm_tree.register(target, pi, mu, cov, 5, LC, 20, 1e-4)
    assert_no_ties_along(target, pi, mu, cov, 5, o_tr)
    if not stop_rule_close(o_tr, 1e-4)[0]:
        assert gt.n_iter_ == len(o_tr)
    np.testing.assert_allclose(res.transformation.rot, o_rot, rtol=0, atol=1e-8)
    np.testing.assert_allclose(res.transformation.t, o_t, rtol=0, atol=1e-8)
    print("default-depth registration: %d iterations" % gt.n_iter_)


# ---------------------------------------------------------------------------------------------------------------------
# the library against the reference's own L = 4 records (tests/golden/hgmm_reg_L4.part*.npz)
# ---------------------------------------------------------------------------------------------------------------------
def test_registration_L4_matches_reference_golden(ctx):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, gmmTreeRegESTep
    g = load_golden("hgmm_reg_L4.npz")
    L, lc = int(g["L"]), float(g["lambda_c"])
    T = hgmm_tree.n_total(L)
    pi, mu, cov = g["pi"], g["mu"], g["cov"]
    ctx.tree_set_nodes(L, pi, mu, cov)
    np.testing.assert_allclose(ctx.tree_node_complexity(T), hgmm_tree.complexity(cov), rtol=1e-9, atol=1e-12)
    for deg in (10, 30):
        tag = "rot%d_" % deg
        target = g[tag + "target"]
        m0, m1, m2 = gmmTreeRegESTep(target, pi, mu, cov, L, lc, ctx=ctx)
        np.testing.assert_allclose(m0, g[tag + "m0"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(m1, g[tag + "m1"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(m2, g[tag + "m2"], rtol=1e-10, atol=1e-12)
        desc = hgmm_tree.reg_descent(target, pi, mu, cov, L, lc)
        assert (desc.contrib & (desc.node >= LDS_NODES)).sum() > 500
        for use_lib in (False, True):
            gt = GMMTree(None, tree_level=L, lambda_c=lc, ctx=ctx)
            gt.set_nodes(pi, mu, cov)
            trace = []
            if not use_lib:
                gt.set_callbacks([lambda tf: trace.append((tf.rot.copy(), tf.t.copy()))])
            res = gt.registration(target, 5, 1.0e-4)
            if not use_lib:
                assert len(trace) == len(g[tag + "iter_rot"])
                for k, (r_k, t_k) in enumerate(trace):
                    np.testing.assert_allclose(r_k, g[tag + "iter_rot"][k], rtol=0, atol=1e-8)
                    np.testing.assert_allclose(t_k, g[tag + "iter_t"][k], rtol=0, atol=1e-8)
            np.testing.assert_allclose(res.transformation.rot, g[tag + "final_rot"], atol=1e-8)
            np.testing.assert_allclose(res.transformation.t, g[tag + "final_t"], atol=1e-8)
            np.testing.assert_allclose(res.q, g[tag + "final_q"], rtol=1e-6)


@pytest.mark.parametrize("device_solve", [0, 1])
def test_split_budget_is_one_call_with_the_stop_rule_across_calls(ctx, device_solve):
    """tree_register with budgets 3 + 3, the pose and q handed on, == one call with budget 6, bit for bit: pose, q, iteration
    count, status and trace rows -- on the host path and under reg_device_solve (has_q of the device's table entry comes
    from the caller's q_prev).  tol = 1000 on the reference's L = 4 records: the oracle's |dq| on rot10_target is 12 589,
    2 033, 380.5, 132, ... (hgmm_tree.register), so the one call stops at its FOURTH iteration -- the first of the second
    half, which stops only if the first half's q reached it; on rot30_target |dq| stays above 1 278 and nothing stops.
    (q agrees with the oracle's to 1e-7 relative, test_registration_L4_matches_reference_golden: 380.5 and 1 278 are far
    from 1000.)"""
    g = load_golden("hgmm_reg_L4.npz")
    L, lc, tol = int(g["L"]), float(g["lambda_c"]), 1000.0
    ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
    I3, Z3 = np.identity(3), np.zeros(3)
    expect = {"rot10_": (4, 1), "rot30_": (6, 0)}
    for tag, (n_iter, st) in expect.items():
        ctx.tree_set_target(g[tag + "target"])
        with ctx.config(reg_device_solve=device_solve):
            r6, t6, d6, q6, s6, tr6 = ctx.tree_register(I3, Z3, 1.0, lc, 6, tol, want_trace=True)
            r1, t1, d1, q1, s1, tr1 = ctx.tree_register(I3, Z3, 1.0, lc, 3, tol, want_trace=True)
            r2, t2, d2, q2, s2, tr2 = ctx.tree_register(r1, t1, 1.0, lc, 3, tol, q_prev=q1, want_trace=True)
        print("%s reg_device_solve %d: one call %d iterations (status %d), split %d + %d (status %d, %d)"
              % (tag, device_solve, d6, s6, d1, d2, s1, s2))
        assert (d6, s6) == (n_iter, st)
        assert (d1, s1) == (3, 0) and (d1 + d2, s2) == (d6, s6)
        assert np.array_equal(r2, r6) and np.array_equal(t2, t6) and q2 == q6
        assert np.array_equal(np.concatenate([tr1, tr2]), tr6)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the batched path at depth
# ---------------------------------------------------------------------------------------------------------------------
def batch_init_idx(pairs, L):
    """The reference's seed-72 draw of T initial means, wrapped into the smallest source (it indexes the source cloud;
    clamped, most of the 37 448 draws of L = 5 would be the same point and the trees would be made of identical siblings)."""
    T = hgmm_tree.n_total(L)
    return np.random.RandomState(72).randint(T, size=T) % min(len(s) for s, _ in pairs)


def batch_pairs(bunny):
    b = bunny.astype(np.float64)
    b45 = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    return [(b[::3], moved(b[1::5], 6.0, [0.2, 1, 0.1], [0.004, -0.002, 0.003])),
            (b45[::4], moved(b45[2::3], 3.0, [1, 0.3, 0.0], [0.001, 0.0, -0.002])),
            (b[2::7], moved(b[::9], 9.0, [0, 0.2, 1], [-0.003, 0.004, 0.0])),
            (b45[1::9], moved(b45[::2], 4.0, [1, 1, 1], [0.002, 0.002, 0.002]))]


@pytest.mark.parametrize("L,solve_on_device", [(4, True), (5, False)])
def test_registration_batch_at_depth_is_bitwise_the_serial_call(ctx, bunny, L, solve_on_device):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree, registration_gmmtree_batch
    pairs = batch_pairs(bunny)
    kw = {"init_idx": batch_init_idx(pairs, L)}
    if L != 5:
        kw["tree_level"] = L                                   # (L = 5: the default depth)
    res, info = registration_gmmtree_batch(pairs, maxiter=20, tol=1e-4, ctx=ctx, return_info=True,
                                           solve_on_device=solve_on_device, **kw)
    assert info["build_iters"].shape == (len(pairs), L)
    for k, (s, t) in enumerate(pairs):
        gt = GMMTree(s, ctx=ctx, solve_on_device=solve_on_device, **kw)
        ref = gt.registration(t, 20, 1e-4)
        assert int(gt.n_iter_) == info["registration_iters"][k], (k, gt.n_iter_, info["registration_iters"])
        assert np.array_equal(ref.transformation.rot, res[k].transformation.rot), k
        assert np.array_equal(ref.transformation.t, res[k].transformation.t), k
        assert np.array_equal(np.ravel(ref.q), np.ravel(res[k].q)), k
    print("L=%d: registration iterations per pair %s" % (L, info["registration_iters"]))


def test_batch_member_at_L5_shadows_oracle_and_node_tables_check_depth(ctx, bunny, monkeypatch):
    """One member of an L = 5 forest: its tables (tree_get_nodes_batch) and its batched trace against the oracle, one step
    at a time.  tree_get_nodes_batch with another L raises before the library writes anything.  The sources are whole
    scans: with fewer points than T = 37 448 the initial means repeat, and identical sibling nodes are exact ties."""
    b45 = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    a = bunny.astype(np.float64)
    pairs = [(a, moved(b45[::3], 4.0, [1, 1, 1], [0.002, 0.002, 0.002])),
             (b45, moved(b45[1::4], 3.0, [1, 0.3, 0.0], [0.001, 0.0, -0.002])),
             (a[::-1].copy(), moved(a[::4], 5.0, [0.2, 1.0, 0.3], [0.003, -0.002, 0.001]))]
    L = 5
    T = hgmm_tree.n_total(L)
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch([s for s, _ in pairs])
    ctx.tree_build_batch([len(a) for a in arrs], L, 20, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
    calls = []
    orig = ctx.lib.hgmm_tree_get_nodes_batch
    monkeypatch.setattr(ctx.lib, "hgmm_tree_get_nodes_batch", lambda *a: calls.append(a) or orig(*a))
    with pytest.raises(ValueError):
        ctx.tree_get_nodes_batch(0, 3)
    assert not calls
    b = 2
    pi, mu, cov = ctx.tree_get_nodes_batch(b, L)
    assert len(calls) == 1 and pi.shape == (T,)
    monkeypatch.undo()
    ctx.tree_set_targets_batch([t for _, t in pairs])
    B = len(pairs)
    budget = 10
    rot, t, iters, q, status, traces = ctx.tree_register_batch(np.tile(np.identity(3), (B, 1, 1)), np.zeros((B, 3)), 1.0, LC,
                                                               budget, 0.0, want_trace=True)
    assert status[b] == 0 and iters[b] == budget
    target = pairs[b][1]
    r_prev, t_prev = np.identity(3), np.zeros(3)
    for k in range(budget):
        o_r, o_t, o_q, (tol_r, tol_t, tol_q), n_deep = oracle_step(target, pi, mu, cov, L, r_prev, t_prev)
        r_k, t_k = traces[b][k, :9].reshape(3, 3), traces[b][k, 9:12]
        np.testing.assert_allclose(r_k, o_r, rtol=0, atol=tol_r)
        np.testing.assert_allclose(t_k, o_t, rtol=0, atol=tol_t)
        np.testing.assert_allclose(traces[b][k, 12], o_q[0], rtol=1e-7, atol=tol_q)
        assert n_deep > 0
        r_prev, t_prev = r_k, t_k
