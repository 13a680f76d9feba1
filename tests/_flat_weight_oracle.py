"""NumPy restatement of the flat (diag / spherical) GMM EM under per-point weights (hgmm_flat_set_weights), for the tests.

Point i counts as ``s_i >= 0`` points; ``S = sum_i s_i``.  ``oracle.flat_em``'s functions do the arithmetic; three
statements change and nothing else does:

* M-step (``flat_em.m_step``): ``resp_ij`` becomes ``s_i resp_ij`` in every sum and ``nk / n`` becomes ``nk / S``; the
  ``+ eps`` terms of both flavours stay where they are, after the sums;
* the log-likelihood behind the stop rule (``flat_em.train``): ``mean_i lpn_i`` becomes ``sum_i s_i lpn_i / S``;
* the sufficient statistics (``hgmm_flat_stats``) are the ``s``-weighted sums, ``n_points = S``.

A zero weight makes the row absent whatever its coordinates: such rows are taken out before anything is computed (a row
of NaNs times zero would be NaN), which is what the kernels' wave-uniform skip does.
"""
import numpy as np

from oracle import flat_em

from _tree_helpers import weights_for


def weight_sum(s):
    """S: a float64 sum, in index order, of the float32 values the device holds."""
    return float(np.cumsum(np.asarray(s, np.float32).astype(np.float64))[-1])


def _live(X, s):
    s = np.asarray(s, np.float32).astype(np.float64)
    keep = s > 0
    return np.asarray(X)[keep], s[keep], keep


def e_step(X, s, inv_std, mu, w, cov_type='diag', variant='W'):
    """(sum_i s_i lpn_i / S, log_resp [N,J], lpn [N]); the two arrays do not see the weights (rows of weight zero: NaN
    where the coordinates are NaN, like the kernels')."""
    Xl, sl, keep = _live(X, s)
    _, log_resp, lpn, _ = flat_em.e_step_full(np.asarray(X), inv_std, mu, w, cov_type, variant)
    return float(np.sum(sl * lpn[keep]) / sl.sum()), log_resp, lpn


def m_step(X, s, resp, cov_type='diag', variant='W'):
    """``flat_em.m_step`` with ``s_i resp_ij`` for ``resp_ij`` and ``nk / S`` for ``nk / n``."""
    Xl, sl, keep = _live(X, s)
    w, mu, cov = flat_em.m_step(Xl, sl[:, None] * np.asarray(resp)[keep], cov_type, variant)
    return w * (len(Xl) / sl.sum()), mu, cov          # (flat_em.m_step divided nk by the row count)


def stats(X, s, inv_std, mu, w, cov_type='diag', variant='W'):
    """What hgmm_flat_stats returns: ([J,7] = sum_i s_i r_ij (1, x - mu, (x - mu)^2), sum_i s_i lpn_i, S)."""
    Xl, sl, keep = _live(X, s)
    _, log_resp, lpn, _ = flat_em.e_step_full(Xl, inv_std, mu, w, cov_type, variant)
    r = sl[:, None] * np.exp(log_resp)
    d = Xl[:, None, :] - mu[None]
    out = np.concatenate([r.sum(0)[:, None], (r[:, :, None] * d).sum(0), (r[:, :, None] * d * d).sum(0)], axis=1)
    return out, float(np.sum(sl * lpn)), float(sl.sum())


def train(X, s, max_iter, tol, mu, cov, w, cov_type='diag', variant='W'):
    """``flat_em.train`` with the weighted M-step and ``lls[k] = sum_i s_i lpn_i / S``; returns the same tuple."""
    Xl, sl, keep = _live(X, s)
    S = sl.sum()
    prev = -np.inf
    converged = False
    inv_std = flat_em.inv_std_from_cov(cov, variant, initial=True)
    lls = []
    for _ in range(max_iter):
        _, log_resp, lpn, _ = flat_em.e_step_full(Xl, inv_std, mu, w, cov_type, variant)
        ll = np.sum(sl * lpn) / S
        lls.append(ll)
        w, mu, cov = flat_em.m_step(Xl, sl[:, None] * np.exp(log_resp), cov_type, variant)
        w = w * (len(Xl) / S)
        inv_std = flat_em.inv_std_from_cov(cov, variant)
        change = ll - prev
        prev = ll
        if abs(change) < tol:
            converged = True
            break
    return inv_std, mu, w, cov, lls, converged


def standard_weights(n, seed=11):
    """The suites' standard weights (tests/_tree_helpers.py: weights_for) as the float32 values the flat entry takes."""
    return weights_for(n, seed).astype(np.float32)
