"""The flat full-covariance fit under per-point weights (hgmm_fullcov_fit_weighted / hgmm_fullcov_estep_weighted) in NumPy:
``oracle.hgmm_tree.build_flat_fullcov`` with the three statements of the weighted tree level changed -- (1) the moments,
(2) pi = m0 / W, (3) the log-likelihood -- and the matching single E-step.  ``w = None`` runs the unweighted statements
themselves.  tests/test_fullcov_weights_cpu.py pins this file to the committed oracle; the GPU tests compare against it."""
import numpy as np

from oracle import hgmm_tree

EPS = hgmm_tree.EPS
LD, SIG2 = 1e-4, 0.0005


def case(bunny):
    """THE cloud and weights of the weighted full-covariance tests: 1300 bunny points, integer weights 0..4 (258 zeros,
    W = 2541)."""
    P = bunny[::30][:1300].astype(np.float64)
    w = np.random.RandomState(5).randint(0, 5, len(P)).astype(np.float64)
    return P, w


def init_rows(w, J, seed=None):
    """J initial rows among the points with w > 0 (distinct while there are enough of them)"""
    nz = np.nonzero(np.asarray(w) > 0)[0]
    return nz[np.random.RandomState(J if seed is None else seed).choice(len(nz), J, replace=len(nz) < J)]


def e_step_w(points, pi, mu, cov, w=None):
    """One E-step of the given parameters -> (m0 [J], m1 [J,3], m2 [J,3,3], labels [N], q): the moments (1) and the
    log-likelihood (3) under ``w``; the floor is tested on gamma and the arg-max does not see the weight."""
    points = np.asarray(points, dtype=np.float64)
    ok, inv, coef = hgmm_tree.node_prep(cov)
    g = pi[None, :] * hgmm_tree.pdf_pairs(points[:, None, :], mu[None], inv[None], coef[None])
    den = g.sum(axis=1)
    good = den > EPS
    gamma = np.where(good[:, None], g / np.where(good, den, 1.0)[:, None], 0.0)
    cur = np.argmax(gamma, axis=1)
    use = np.where(gamma < EPS, 0.0, gamma)
    if w is not None:
        use = use * w[:, None]                                           # (1)
    m0 = use.sum(axis=0)
    m1 = use.T @ points
    m2 = np.einsum('nj,na,nb->jab', use, points, points)
    lg = np.log(np.maximum(g[:, ~(pi < EPS)].sum(axis=1), EPS))
    q = lg.sum() if w is None else (w * lg).sum()                        # (3)
    return m0, m1, m2, cur, q


def build_flat_fullcov_w(points, J, ls, ld, init_idx, sig2=0.00034, max_iters=10000, w=None):
    """``oracle.hgmm_tree.build_flat_fullcov`` statement by statement, with the three marked ones under ``w`` [N] >= 0.
    Returns (pi, mu, cov, q_trace, current_idx)."""
    points = np.asarray(points, dtype=np.float64)
    n = len(points)
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (n,)
    W = float(n) if w is None else hgmm_tree.weight_sum(w)
    pi = np.full(J, 1.0 / J)
    mu = np.array(points[np.asarray(init_idx)], dtype=np.float64)
    cov = np.tile(np.identity(3) * sig2, (J, 1, 1))
    qs = []
    prev_q = 0.0
    cur = None
    while True:
        ok, inv, coef = hgmm_tree.node_prep(cov)
        g = pi[None, :] * hgmm_tree.pdf_pairs(points[:, None, :], mu[None], inv[None], coef[None])
        den = g.sum(axis=1)
        good = den > EPS
        gamma = np.where(good[:, None], g / np.where(good, den, 1.0)[:, None], 0.0)
        cur = np.argmax(gamma, axis=1)
        use = np.where(gamma < EPS, 0.0, gamma)
        if w is not None:
            use = use * w[:, None]                                       # (1)
        m0 = use.sum(axis=0)
        m1 = use.T @ points
        m2 = np.einsum('nj,na,nb->jab', use, points, points)
        for j in range(J):
            if m0[j] < ld:
                pi[j], mu[j], cov[j] = 0.0, 0.0, np.identity(3)
            else:
                pi[j] = m0[j] / (n if w is None else W)                  # (2)
                mu[j] = m1[j] / m0[j]
                cov[j] = m2[j] / m0[j] - np.outer(mu[j], mu[j])
        sel = ~(pi < EPS)
        ok, inv, coef = hgmm_tree.node_prep(cov[sel])
        p = hgmm_tree.pdf_pairs(points[:, None, :], mu[sel][None], inv[None], coef[None])
        lg = np.log(np.maximum((p * pi[sel][None, :]).sum(axis=1), EPS))
        q = lg.sum() if w is None else (w * lg).sum()                    # (3)
        qs.append(q)
        if abs(q - prev_q) < ls or len(qs) >= max_iters:
            break
        prev_q = q
    return pi, mu, cov, np.array(qs), cur


def label_gaps(points, pi, mu, cov):
    """(g_max - g_second) / g_max per point under the given parameters: how close each arg-max is to a tie"""
    ok, inv, coef = hgmm_tree.node_prep(cov)
    g = pi[None, :] * hgmm_tree.pdf_pairs(np.asarray(points)[:, None, :], mu[None], inv[None], coef[None])
    if g.shape[1] < 2:
        return np.full(len(g), np.inf)
    top = np.sort(g, axis=1)[:, -2:]
    return np.where(top[:, 1] > 0, (top[:, 1] - top[:, 0]) / np.where(top[:, 1] > 0, top[:, 1], 1.0), np.inf)
