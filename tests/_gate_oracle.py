"""NumPy restatement of the registration E-step under a Mahalanobis gate (hgmm_tree_set_reg_gate), for the gate's tests.

``gated_reg_e_step`` is oracle.hgmm_tree.reg_e_step, statement for statement, with one more condition on a (point, node)
pair that would contribute: (y - mu_s)^T Sigma_s^-1 (y - mu_s) <= gate.  The descent, the stop rule and the 1e-15 floor on
the responsibility are untouched; with ``gate = inf`` the result is reg_e_step's bit for bit.  It also reports how close
any contributing pair came to the gate: a pair within rounding of it may fall on either side in another arithmetic, and a
comparison of moments is only meaningful when there is none."""
from collections import namedtuple

import numpy as np

from oracle import hgmm_tree
from oracle.hgmm_tree import EPS, N_NODE, child, complexity, n_total, node_prep, pdf_pairs

GatedEstep = namedtuple("GatedEstep", ["m0", "m1", "m2", "margin", "pairs", "gated"])


def gated_reg_e_step(points, pi, mu, cov, max_level, lc, gate):
    """-> GatedEstep(m0[T], m1[T,3], m2[T,3,3], margin, pairs, gated).
    pairs   the (point, node) pairs that contribute without a gate (not stopped, responsibility >= 1e-15)
    gated   how many of them the gate leaves out
    margin  min |maha2 - gate| / gate over ``pairs`` (inf without pairs or with gate = inf)"""
    points = np.asarray(points, dtype=np.float64)
    T = n_total(max_level)
    ok, inv, coef = node_prep(cov)
    cplx = complexity(cov)
    m0 = np.zeros(T)
    m1 = np.zeros((T, 3))
    m2 = np.zeros((T, 3, 3))
    n = len(points)
    search = -np.ones(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    margin, pairs, gated = np.inf, 0, 0
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
        # the gate: the quadratic form of the node the point moved to (a NaN form fails the comparison)
        d = xk - mu[sk]
        maha2 = np.einsum('...i,...ij,...j->...', d, inv[sk], d)
        contributes = gs > 0.0
        passes = maha2 <= gate
        pairs += int(contributes.sum())
        gated += int((contributes & ~passes).sum())
        if np.isfinite(gate) and contributes.any():
            margin = min(margin, float(np.nanmin(np.abs(maha2[contributes] - gate))) / gate)
        gs = np.where(passes, gs, 0.0)
        np.add.at(m0, sk, gs)
        np.add.at(m1, sk, gs[:, None] * xk)
        np.add.at(m2, sk, gs[:, None, None] * (xk[:, :, None] * xk[:, None, :]))
    return GatedEstep(m0, m1, m2, margin, pairs, gated)


def gated_register(target, pi, mu, cov, max_level, lc, gate, maxiter=20, tol=1.0e-4):
    """oracle.hgmm_tree.register with the gated E-step.  -> (rot, t, trace): the loop's own final pose y = rot x + t (NOT
    inverted) and per iteration (rot, t, q, GatedEstep of the E-step that led there)."""
    target = np.asarray(target, dtype=np.float64)
    rot, t = np.identity(3), np.zeros(3)
    q_prev = None
    trace = []
    for _ in range(maxiter):
        e = gated_reg_e_step(target @ rot.T + t, pi, mu, cov, max_level, lc, gate)
        rot, t, q = hgmm_tree.reg_m_step(e.m0, e.m1, e.m2, mu, cov, rot, t)
        trace.append((rot.copy(), t.copy(), np.array(q, copy=True), e))
        if q_prev is not None and q.size and q_prev.size and abs(q - q_prev) < tol:
            break
        q_prev = q
    return rot, t, trace
