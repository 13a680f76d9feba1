"""NumPy restatement of the registration E-step under per-point weights of the target (hgmm_tree_set_target_weights), for
the weights' tests.

``weighted_reg_e_step`` is oracle.hgmm_tree.reg_e_step, statement for statement, with one more statement after the 1e-15
floor on the responsibility: ``gs = gs * w[idx][keep]``.  The descent, the stop rule and the floor itself do not see the
weight; with ``w = None`` or ``w == 1`` the result is reg_e_step's bit for bit.  An optional Mahalanobis gate
(hgmm_tree_set_reg_gate, as in tests/_gate_oracle.py) composes with it: the gate is decided on the pair, the weight scales
what passes.

The helpers the weights' test files share are here too (this module is a helper, not a conftest): ``weights_for``,
``resident``, ``loop5``, ``same_bits``."""
import numpy as np

from oracle import hgmm_tree
from oracle.hgmm_tree import EPS, N_NODE, child, complexity, n_total, node_prep, pdf_pairs

I3 = np.identity(3)


def weights_for(n):
    """the tests' weights unless stated otherwise: uniform in [0.25, 4), one in ten exactly zero"""
    rs = np.random.RandomState(11)
    w = rs.uniform(0.25, 4.0, n)
    w[rs.uniform(size=n) < 0.1] = 0.0
    return w


def resident(ctx, g, target, w=None):
    L = int(g["L"])
    ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(target)
    if w is not None:
        ctx.tree_set_target_weights(w)
    return L, float(g["lambda_c"]), hgmm_tree.n_total(L)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def loop5(ctx, lc):
    """five iterations from the identity, no stop rule -> (rot, t, iterations, q, status, trace [5, 13])"""
    return ctx.tree_register(I3, np.zeros(3), 1.0, lc, 5, 0.0, None, want_trace=True)


def weighted_reg_e_step(points, pi, mu, cov, max_level, lc, w=None, gate=np.inf):
    """-> (m0[T], m1[T,3], m2[T,3,3]).  ``w`` [n] >= 0 or None (no weights); ``gate``: squared Mahalanobis gate (inf: off)."""
    points = np.asarray(points, dtype=np.float64)
    T = n_total(max_level)
    ok, inv, coef = node_prep(cov)
    cplx = complexity(cov)
    m0 = np.zeros(T)
    m1 = np.zeros((T, 3))
    m2 = np.zeros((T, 3, 3))
    n = len(points)
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (n,)
    search = -np.ones(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    for _ in range(max_level):
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        x = points[idx]
        j0 = child(search[idx])
        kid = j0[:, None] + np.arange(N_NODE)[None, :]
        g = pi[kid] * pdf_pairs(x[:, None, :], mu[kid], inv[kid], coef[kid])
        den = g.sum(axis=1)
        good = den > EPS
        gamma = np.where(good[:, None], g / np.where(good, den, 1.0)[:, None], 0.0)
        am = np.argmax(gamma, axis=1)
        s = j0 + am
        search[idx] = s
        stop = cplx[s] <= lc
        alive[idx[stop]] = False
        keep = ~stop
        gs = gamma[np.arange(len(idx)), am][keep]
        gs = np.where(gs < EPS, 0.0, gs)
        sk = s[keep]
        xk = x[keep]
        if np.isfinite(gate):                    # (tests/_gate_oracle.py: a NaN form fails the comparison)
            d = xk - mu[sk]
            maha2 = np.einsum('...i,...ij,...j->...', d, inv[sk], d)
            gs = np.where(maha2 <= gate, gs, 0.0)
        if w is not None:
            gs = gs * w[idx][keep]
        np.add.at(m0, sk, gs)
        np.add.at(m1, sk, gs[:, None] * xk)
        np.add.at(m2, sk, gs[:, None, None] * (xk[:, :, None] * xk[:, None, :]))
    return m0, m1, m2


def weighted_register(target, pi, mu, cov, max_level, lc=0.01, maxiter=20, tol=1.0e-4, w=None, gate=np.inf):
    """oracle.hgmm_tree.register with the weighted E-step.  -> (rot_inv, t_inv, q, trace) as register returns them: the
    inverted pose and per iteration (rot, t, q, m0, m1, m2) of the loop's own pose y = rot x + t."""
    target = np.asarray(target, dtype=np.float64)
    rot, t = np.identity(3), np.zeros(3)
    q_prev = None
    trace = []
    q = None
    for _ in range(maxiter):
        tt = target @ rot.T + t
        m0, m1, m2 = weighted_reg_e_step(tt, pi, mu, cov, max_level, lc, w, gate)
        rot, t, q = hgmm_tree.reg_m_step(m0, m1, m2, mu, cov, rot, t)
        trace.append((rot.copy(), t.copy(), np.array(q, copy=True), m0, m1, m2))
        if q_prev is not None and q.size and q_prev.size and abs(q - q_prev) < tol:
            break
        q_prev = q
    return rot.T, -rot.T @ t, q, trace
