"""NumPy restatement of the tree build under per-point weights of the SOURCE cloud (hgmm_tree_set_source_weights), for the
tests: ``oracle.hgmm_tree.build_tree`` statement for statement, with the three statements the weights change marked (1)-(3).
Point i with weight w_i >= 0 counts as w_i points.  ``w = None`` runs the unweighted statements themselves, so the result is
``build_tree``'s bit for bit."""
import numpy as np

from oracle import hgmm_tree
from oracle.hgmm_tree import EPS, N_NODE, BuildTrace, child, level, node_prep, pdf_pairs


def weighted_e_step(points, pi, mu, cov, parent_idx, w):
    """hgmm_tree.e_step with (1): ``use = where(gamma < EPS, 0, gamma) * w_i``.  The floor is tested on gamma, the arg-max
    child does not see the weight."""
    T = len(pi)
    j0 = child(np.asarray(parent_idx, dtype=np.int64))
    kid = j0[:, None] + np.arange(N_NODE)[None, :]
    ok, inv, coef = node_prep(cov)
    g = pi[kid] * pdf_pairs(points[:, None, :], mu[kid], inv[kid], coef[kid])
    den = g.sum(axis=1)
    good = den > EPS
    gamma = np.where(good[:, None], g / np.where(good, den, 1.0)[:, None], 0.0)
    cur = j0 + np.argmax(gamma, axis=1)
    use = np.where(gamma < EPS, 0.0, gamma)
    if w is not None:
        use = use * w[:, None]                                       # (1)
    m0 = np.zeros(T)
    m1 = np.zeros((T, 3))
    m2 = np.zeros((T, 3, 3))
    flat = kid.ravel()
    np.add.at(m0, flat, use.ravel())
    np.add.at(m1, flat, (use[:, :, None] * points[:, None, :]).reshape(-1, 3))
    xx = points[:, :, None] * points[:, None, :]
    np.add.at(m2, flat, (use[:, :, None, None] * xx[:, None, :, :]).reshape(-1, 3, 3))
    return m0, m1, m2, cur, gamma


def weighted_log_likelihood(points, pi, mu, cov, lvl, w, chunk=4096):
    """hgmm_tree.log_likelihood with (3): ``q = sum_i w_i log max(sum_j [pi_j >= eps] pi_j N(x_i; j), eps)``."""
    lb, le = level(lvl), level(lvl + 1)
    sel = np.arange(lb, le)
    sel = sel[~(pi[sel] < EPS)]
    ok, inv, coef = node_prep(cov[sel])
    q = 0.0
    for s in range(0, len(points), chunk):
        x = points[s:s + chunk]
        if len(sel):
            p = pdf_pairs(x[:, None, :], mu[sel][None], inv[None], coef[None])
            tot = (p * pi[sel][None, :]).sum(axis=1)
        else:
            tot = np.zeros(len(x))
        lg = np.log(np.maximum(tot, EPS))
        q += lg.sum() if w is None else (w[s:s + chunk] * lg).sum()  # (3)
    return q


def weight_sum(w):
    """W = sum of the weights in float64, in index order (what the library takes on the host at upload)."""
    total = 0.0
    for v in np.asarray(w, dtype=np.float64):
        total += float(v)
    return total


def weighted_build_tree(points, max_level, ls, ld, init_mu, sig2, w=None, max_iters_per_level=10000):
    """hgmm_tree.build_tree with the initial means given as coordinates [T,3] (as the C entry takes them) and the weights
    ``w`` [n] (None: none).  -> (pi, mu, cov, BuildTrace)."""
    points = np.asarray(points, dtype=np.float64)
    T = hgmm_tree.n_total(max_level)
    pi = np.full(T, 1.0 / N_NODE)
    mu = np.array(init_mu, dtype=np.float64).reshape(T, 3)
    cov = np.tile(np.identity(3) * sig2, (T, 1, 1))
    n = len(points)
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (n,)
    n_points = n if w is None else weight_sum(w)                     # (2) pi_j = m0_j / W
    parent = -np.ones(n, dtype=np.int64)
    cur = np.zeros(n, dtype=np.int64)
    q_trace, iters, cur_levels = [], [], []
    for l in range(max_level):
        prev_q = 0.0
        it = 0
        while True:
            m0, m1, m2, cur, _ = weighted_e_step(points, pi, mu, cov, parent, w)
            hgmm_tree.m_step(m0, m1, m2, l, pi, mu, cov, n_points, ld)
            q = weighted_log_likelihood(points, pi, mu, cov, l, w)
            q_trace.append(q)
            it += 1
            if abs(q - prev_q) < ls or it >= max_iters_per_level:
                break
            prev_q = q
        iters.append(it)
        cur_levels.append(cur.copy())
        parent = cur.copy()
    return pi, mu, cov, BuildTrace(np.array(q_trace), np.array(iters), cur_levels)


def stop_margins(q_trace, iters, ls):
    """||dq| - ls| / ls of every stop decision of a build (dq against 0 at a level's first iteration): how far each
    decision was from going the other way."""
    out, at = [], 0
    for it in iters:
        prev = 0.0
        for k in range(int(it)):
            out.append(abs(abs(q_trace[at + k] - prev) - ls) / ls)
            prev = q_trace[at + k]
        at += int(it)
    return np.array(out)
