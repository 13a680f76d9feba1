"""CPU oracle for the hierarchical-GMM (8-ary GMM tree) hot path.

TEST INFRASTRUCTURE ONLY.  Nothing in the shipped package may import this
module: only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline``
leg of ``bench.py`` use it, and only as the checker / the timed CPU baseline.

Vectorised NumPy (float64) restatement of the reference's *CPU twin*
``src/python/hgmm/hgmm_cupy_cpu_working.py`` (the canonical HGMM semantics; the
Numba file ``src/python/hgmm/hgmm_gpu.py`` has the empty-node guard commented
out and is not followed where the two differ).  No code is copied: the reference
is an object-per-node pure-Python triple loop, this is array code; every
function cites the lines it follows.

Pinning: ``tests/golden/hgmm_*.npz`` were produced by exec'ing the reference
itself (``tools/gen_golden.py``) and ``tests/test_oracle_golden.py`` checks this
module against them.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

EPS = 1.0e-15           # hgmm_cupy_cpu_working.py:29
N_NODE = 8              # hgmm_cupy_cpu_working.py:30
TWO_PI_POW = (2.0 * np.pi) ** 1.5
F32_EPS = float(np.finfo(np.float32).eps)


def child(j, n_node=N_NODE):
    """First child of node j; root pseudo-parent is -1 (hgmm_cupy_cpu_working.py:93-94)."""
    return (j + 1) * n_node


def level(l, n_node=N_NODE):
    """Index of the first node of level l (hgmm_cupy_cpu_working.py:96-97)."""
    return n_node * (n_node ** l - 1) // (n_node - 1)


def n_total(max_level, n_node=N_NODE):
    return level(max_level, n_node)


# ---------------------------------------------------------------------------
# node tables: pi[T], mu[T,3], cov[T,3,3]   (object-per-node in the reference)
# ---------------------------------------------------------------------------

def det3(c):
    return (c[..., 0, 0] * (c[..., 1, 1] * c[..., 2, 2] - c[..., 1, 2] * c[..., 2, 1])
            - c[..., 0, 1] * (c[..., 1, 0] * c[..., 2, 2] - c[..., 1, 2] * c[..., 2, 0])
            + c[..., 0, 2] * (c[..., 1, 0] * c[..., 2, 1] - c[..., 1, 1] * c[..., 2, 0]))


def inv3(c, det):
    """Adjugate inverse of a batch of 3x3 matrices (det supplied)."""
    out = np.empty_like(c)
    out[..., 0, 0] = c[..., 1, 1] * c[..., 2, 2] - c[..., 1, 2] * c[..., 2, 1]
    out[..., 0, 1] = c[..., 0, 2] * c[..., 2, 1] - c[..., 0, 1] * c[..., 2, 2]
    out[..., 0, 2] = c[..., 0, 1] * c[..., 1, 2] - c[..., 0, 2] * c[..., 1, 1]
    out[..., 1, 0] = c[..., 1, 2] * c[..., 2, 0] - c[..., 1, 0] * c[..., 2, 2]
    out[..., 1, 1] = c[..., 0, 0] * c[..., 2, 2] - c[..., 0, 2] * c[..., 2, 0]
    out[..., 1, 2] = c[..., 0, 2] * c[..., 1, 0] - c[..., 0, 0] * c[..., 1, 2]
    out[..., 2, 0] = c[..., 1, 0] * c[..., 2, 1] - c[..., 1, 1] * c[..., 2, 0]
    out[..., 2, 1] = c[..., 0, 1] * c[..., 2, 0] - c[..., 0, 0] * c[..., 2, 1]
    out[..., 2, 2] = c[..., 0, 0] * c[..., 1, 1] - c[..., 0, 1] * c[..., 1, 0]
    return out / det[..., None, None]


def node_prep(cov):
    """Per-node quantities the reference recomputes per (point,node) pair
    (hgmm_cupy_cpu_working.py:62-70): validity (det >= eps), inverse, 1/(sqrt(det)(2pi)^1.5)."""
    det = det3(cov)
    ok = ~(det < EPS)
    safe = np.where(ok, det, 1.0)
    inv = inv3(cov, safe)
    coef = np.where(ok, 1.0 / (np.sqrt(safe) * TWO_PI_POW), 0.0)
    return ok, inv, coef


def pdf_pairs(x, mu, inv, coef):
    """N(x; mu, cov) for broadcastable batches; 0 where coef == 0 (det < eps).
    hgmm_cupy_cpu_working.py:62-70."""
    d = x - mu
    t = np.einsum('...i,...ij,...j->...', d, inv, d)
    return coef * np.exp(-0.5 * t)


def child_gamma(x, j0, pi, mu, inv, coef):
    """The eight children j0 .. j0+7 of each point's node: kid [n,8], g = pi N(x) [n,8], den = sum g, good = den > EPS and
    gamma = g / den (0 where not good).  hgmm_cupy_cpu_working.py:170-183 and 207-217: the build's E-step and the
    registration descent normalise alike."""
    kid = j0[:, None] + np.arange(N_NODE)[None, :]
    g = pi[kid] * pdf_pairs(x[:, None, :], mu[kid], inv[kid], coef[kid])
    den = g.sum(axis=1)
    good = den > EPS
    gamma = np.where(good[:, None], g / np.where(good, den, 1.0)[:, None], 0.0)
    return kid, g, den, good, gamma


def new_moments(T):
    return np.zeros(T), np.zeros((T, 3)), np.zeros((T, 3, 3))


def add_moments(m0, m1, m2, nodes, g, x):
    """m0[nodes] += g, m1[nodes] += g x, m2[nodes] += g x x^T, pair by pair in index order (accumulate, 99-106).
    ``nodes`` and ``g`` have one shape, ``x`` [..., 3] broadcasts against it."""
    flat = nodes.ravel()                                             # (add.at is slower under a 2-d index)
    np.add.at(m0, flat, g.ravel())
    np.add.at(m1, flat, (g[..., None] * x).reshape(-1, 3))
    np.add.at(m2, flat, (g[..., None, None] * (x[..., :, None] * x[..., None, :])).reshape(-1, 3, 3))


def e_step(points, pi, mu, cov, parent_idx, lvl_nodes=None, w=None):
    """One tree E-step.  hgmm_cupy_cpu_working.py:162-191 (+accumulate 99-106).  ``w`` [N] >= 0: point i counts as w_i
    points (hgmm_tree_set_source_weights); the floor is tested on gamma, the arg-max child does not see the weight.

    Returns (m0[T], m1[T,3], m2[T,3,3], current_idx[N], gamma[N,8]).
    """
    j0 = child(np.asarray(parent_idx, dtype=np.int64))
    kid, _, _, _, gamma = child_gamma(points, j0, pi, mu, *node_prep(cov)[1:])
    cur = j0 + np.argmax(gamma, axis=1)
    use = np.where(gamma < EPS, 0.0, gamma)                          # accumulate() skips gamma < eps
    if w is not None:
        use = use * w[:, None]                                       # (1) of the three statements the weights change
    m = new_moments(len(pi))
    add_moments(*m, kid, use, points[:, None, :])
    return (*m, cur, gamma)


def m_step(m0, m1, m2, lvl, pi, mu, cov, n_points, ld):
    """In-place ML update of the nodes of level ``lvl``.
    hgmm_cupy_cpu_working.py:193-198 with mlEstimator 109-119 (m0 < ld -> pi=0, mu=0, cov=I)."""
    lb, le = level(lvl), level(lvl + 1)
    for j in range(lb, le):
        if m0[j] < ld:
            pi[j] = 0.0
            mu[j] = 0.0
            cov[j] = np.identity(3)
        else:
            pi[j] = m0[j] / n_points
            mu[j] = m1[j] / m0[j]
            cov[j] = m2[j] / m0[j] - np.outer(mu[j], mu[j])


def log_likelihood(points, pi, mu, cov, lvl, chunk=4096, w=None):
    """q = sum_i [w_i] log max(sum_{j in level, pi_j >= eps} pi_j N(x_i; j), eps).
    hgmm_cupy_cpu_working.py:72-85."""
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


def init_nodes(points, max_level, init_idx, sig2, init_mu=None):
    """pi = 1/8, mu = points[idx] (or ``init_mu`` [T,3]), cov = sig2*I  (hgmm_cupy_cpu_working.py:123-136)."""
    T = n_total(max_level)
    pi = np.full(T, 1.0 / N_NODE)
    mu = np.array(points[np.asarray(init_idx)] if init_mu is None else np.reshape(init_mu, (T, 3)), dtype=np.float64)
    cov = np.tile(np.identity(3) * sig2, (T, 1, 1))
    return pi, mu, cov


BuildTrace = namedtuple('BuildTrace', ['q', 'iters_per_level', 'current_idx_per_level'])


def build_tree(points, max_level, ls, ld, init_idx, sig2=0.00034, max_iters_per_level=10000, w=None, init_mu=None,
               ll_chunk=4096):
    """hgmm_cupy_cpu_working.py:122-160.  RNG stays outside (``init_idx`` explicit; the
    reference draws ``randint(nTotal, size=nTotal)`` from CuPy's generator).  ``init_mu`` [T,3] gives the initial means
    as coordinates, as the C entry takes them, in place of ``init_idx``.

    ``w`` [n] >= 0 (hgmm_tree_set_source_weights): point i counts as w_i points.  Three statements change, marked
    (1)-(3): ``use * w`` in :func:`e_step`, ``pi = m0 / W`` here, ``sum w log`` in :func:`log_likelihood`.  ``w = None``
    runs the unweighted statements themselves.  ``ll_chunk``: the points :func:`log_likelihood` takes at a time (its
    ``chunk``; the default is that function's own, so nothing changes) -- deep levels of a small cloud bound memory with it.

    Returns (pi, mu, cov, trace)."""
    points = np.asarray(points, dtype=np.float64)
    pi, mu, cov = init_nodes(points, max_level, init_idx, sig2, init_mu)
    n = n_points = len(points)
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (n,)
        n_points = weight_sum(w)                                     # (2) pi_j = m0_j / W
    parent = -np.ones(n, dtype=np.int64)
    cur = np.zeros(n, dtype=np.int64)
    q_trace, iters, cur_levels = [], [], []
    for l in range(max_level):
        prev_q = 0.0
        it = 0
        while True:
            m0, m1, m2, cur, _ = e_step(points, pi, mu, cov, parent, w=w)
            m_step(m0, m1, m2, l, pi, mu, cov, n_points, ld)
            q = log_likelihood(points, pi, mu, cov, l, chunk=ll_chunk, w=w)
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


def build_flat_fullcov(points, J, ls, ld, init_idx, sig2=0.00034, max_iters=10000):
    """Flat full-covariance EM over J components == ONE tree level with branching J
    (the CPU twin run with its module global ``n_node`` set to J and maxTreeLevel = 1;
    hgmm_cupy_cpu_working.py:30,122-160).  Note pi0 = 1/J and the stop rule on q.

    Returns (pi, mu, cov, q_trace, current_idx)."""
    points = np.asarray(points, dtype=np.float64)
    n = len(points)
    pi = np.full(J, 1.0 / J)
    mu = np.array(points[np.asarray(init_idx)], dtype=np.float64)
    cov = np.tile(np.identity(3) * sig2, (J, 1, 1))
    qs = []
    prev_q = 0.0
    cur = None
    while True:
        ok, inv, coef = node_prep(cov)
        g = pi[None, :] * pdf_pairs(points[:, None, :], mu[None], inv[None], coef[None])
        den = g.sum(axis=1)
        good = den > EPS
        gamma = np.where(good[:, None], g / np.where(good, den, 1.0)[:, None], 0.0)
        cur = np.argmax(gamma, axis=1)
        use = np.where(gamma < EPS, 0.0, gamma)
        m0 = use.sum(axis=0)
        m1 = use.T @ points
        m2 = np.einsum('nj,na,nb->jab', use, points, points)
        for j in range(J):
            if m0[j] < ld:
                pi[j], mu[j], cov[j] = 0.0, 0.0, np.identity(3)
            else:
                pi[j] = m0[j] / n
                mu[j] = m1[j] / m0[j]
                cov[j] = m2[j] / m0[j] - np.outer(mu[j], mu[j])
        sel = ~(pi < EPS)
        ok, inv, coef = node_prep(cov[sel])
        p = pdf_pairs(points[:, None, :], mu[sel][None], inv[None], coef[None])
        q = np.log(np.maximum((p * pi[sel][None, :]).sum(axis=1), EPS)).sum()
        qs.append(q)
        if abs(q - prev_q) < ls or len(qs) >= max_iters:
            break
        prev_q = q
    return pi, mu, cov, np.array(qs), cur


def complexity(cov):
    """smallest eigenvalue / trace (hgmm_cupy_cpu_working.py:87-91; reference uses
    ``np.linalg.eig`` on the symmetric covariance and sorts descending)."""
    lam = np.linalg.eigvalsh(cov)
    return lam[..., 0] / lam.sum(axis=-1)


def _descend(points, pi, mu, cov, max_level, lc):
    """THE tree descent of the registration E-step (hgmm_cupy_cpu_working.py:202-228), one level per step: the points still
    alive normalise gamma over the 8 children of their current node, move to the arg-max child and stop there when its
    covariance is 'flat enough'.  :func:`reg_e_step` and :func:`reg_descent` are its two consumers and nothing else
    restates it.  Yields per level (l, idx, x, g, den, good, s, gs, cs, stop):
      idx [n_l] the points alive at level l, x their coordinates      g [n_l,8], den [n_l], good = den > EPS
      s the child each moves to, gs its gamma, cs its complexity      stop = cs <= lc"""
    n = len(points)
    ok, inv, coef = node_prep(cov)
    cplx = complexity(cov)
    search = -np.ones(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    for l in range(max_level):
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        x = points[idx]
        j0 = child(search[idx])
        _, g, den, good, gamma = child_gamma(x, j0, pi, mu, inv, coef)
        am = np.argmax(gamma, axis=1)
        s = j0 + am
        search[idx] = s
        cs = cplx[s]
        stop = cs <= lc
        alive[idx[stop]] = False
        yield l, idx, x, g, den, good, s, gamma[np.arange(len(idx)), am], cs, stop


GatedEstep = namedtuple('GatedEstep', ['m0', 'm1', 'm2', 'margin', 'pairs', 'gated'])


def reg_e_step(points, pi, mu, cov, max_level, lc, w=None, gate=np.inf, report=False):
    """Registration E-step: descend the tree (:func:`_descend`) and, where a point does not stop, add (g, g x, g x x^T) to
    the node it moved to; g is its gamma there, 0 below the 1e-15 floor.  hgmm_cupy_cpu_working.py:202-228.
    Returns (m0[T], m1[T,3], m2[T,3,3]).

    Two options act on a pair that would contribute, in this order, after the floor; neither is seen by the descent, the
    stop rule or the floor:
      gate   squared Mahalanobis gate (hgmm_tree_set_reg_gate): the pair counts only if (y - mu_s)^T Sigma_s^-1 (y - mu_s)
             <= gate; a NaN form fails the comparison.  ``inf`` is OFF, as in the library: no form is evaluated and no
             comparison is made, so a pair with a NaN form is kept (the earlier gated restatement compared against inf
             and dropped it; none of the fixtures has such a pair).
      w      [n] >= 0 (hgmm_tree_set_target_weights): ``g * w_i`` for g.  ``None`` multiplies nothing.

    ``report=True`` returns GatedEstep(m0, m1, m2, margin, pairs, gated) instead:
      pairs   the (point, node) pairs that contribute without a gate (not stopped, gamma >= 1e-15)
      gated   how many of them the gate leaves out
      margin  min |maha2 - gate| / gate over ``pairs`` (inf without pairs or with the gate off): a pair within rounding of
              the gate may fall on either side in another arithmetic."""
    points = np.asarray(points, dtype=np.float64)
    m = new_moments(n_total(max_level))
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (len(points),)
    inv = node_prep(cov)[1] if np.isfinite(gate) else None
    margin, pairs, gated = np.inf, 0, 0
    for _, idx, x, _, _, _, s, gs, _, stop in _descend(points, pi, mu, cov, max_level, lc):
        keep = ~stop
        gs = gs[keep]
        gs = np.where(gs < EPS, 0.0, gs)
        sk = s[keep]
        xk = x[keep]
        if report:
            contributes = gs > 0.0
            pairs += int(contributes.sum())
        if inv is not None:
            d = xk - mu[sk]
            maha2 = np.einsum('...i,...ij,...j->...', d, inv[sk], d)
            passes = maha2 <= gate
            if report and contributes.any():
                gated += int((contributes & ~passes).sum())
                margin = min(margin, float(np.nanmin(np.abs(maha2[contributes] - gate))) / gate)
            gs = np.where(passes, gs, 0.0)
        if w is not None:
            gs = gs * w[idx][keep]
        add_moments(*m, sk, gs, xk)
    return GatedEstep(*m, margin, pairs, gated) if report else m


# ---------------------------------------------------------------------------
# host-side registration M-step (stays on the host in the product too)
# ---------------------------------------------------------------------------

def skew(x):
    return np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])


def twist_trans(tw):
    """Rodrigues; hgmm_cupy_cpu_working.py:296-314 (non-linear branch)."""
    twd = np.linalg.norm(tw[:3])
    if twd == 0.0:
        return np.identity(3), tw[3:]
    a = tw[:3] / twd
    c, s = np.cos(twd), np.sin(twd)
    return c * np.identity(3) + (1.0 - c) * np.outer(a, a) + s * skew(a), tw[3:]


def twist_mul(tw, rot, t):
    """hgmm_cupy_cpu_working.py:284-294."""
    tr, tt = twist_trans(tw)
    return np.dot(tr, rot), np.dot(t, tr.T) + tt


def reg_m_step(m0, m1, m2, mu, cov, rot, t):
    """Twist least-squares update; hgmm_cupy_cpu_working.py:356-375.
    Returns (rot, t, q) with q = lstsq residual array (may be empty)."""
    n = len(m0)
    amat = np.zeros((n * 3, 6))
    bmat = np.zeros(n * 3)
    for i in range(n):
        if m0[i] < F32_EPS:
            continue
        lam, vec = np.linalg.eigh(cov[i])
        s = m1[i] / m0[i]
        vec = vec * np.sqrt(m0[i] / lam)
        sl = slice(3 * i, 3 * i + 3)
        bmat[sl] = vec.T @ mu[i] - vec.T @ s
        amat[sl, :3] = np.cross(s[None, :], vec.T)
        amat[sl, 3:] = vec.T
    x, q, _, _ = np.linalg.lstsq(amat, bmat, rcond=-1)
    rot, t = twist_mul(x, rot, t)
    return rot, t, q


def register(target, pi, mu, cov, max_level, lc=0.01, maxiter=20, tol=1.0e-4, w=None, gate=np.inf):
    """hgmm_cupy_cpu_working.py:377-391, THE registration loop; ``w`` and ``gate`` go to :func:`reg_e_step`.
    Returns (rot_inv, t_inv, q, trace) where (rot_inv, t_inv) is ``tf.inverse()`` as the reference returns it and
    trace holds per iteration (rot, t, q, m0, m1, m2) of the loop's own pose y = rot x + t (NOT inverted)."""
    target = np.asarray(target, dtype=np.float64)
    rot, t = np.identity(3), np.zeros(3)
    q_prev = None
    trace = []
    q = None
    for _ in range(maxiter):
        tt = target @ rot.T + t
        m0, m1, m2 = reg_e_step(tt, pi, mu, cov, max_level, lc, w, gate)
        rot, t, q = reg_m_step(m0, m1, m2, mu, cov, rot, t)
        trace.append((rot.copy(), t.copy(), np.array(q, copy=True), m0, m1, m2))
        if q_prev is not None and q.size and q_prev.size and abs(q - q_prev) < tol:
            break
        q_prev = q
    return rot.T, -rot.T @ t, q, trace


# ---------------------------------------------------------------------------
# test helpers for deep trees (nothing above depends on them)
# ---------------------------------------------------------------------------

RegDescent = namedtuple('RegDescent', ['node', 'contrib', 'gap', 'den_margin', 'gamma_margin', 'cplx_margin'])


def reg_descent(points, pi, mu, cov, max_level, lc):
    """The decisions of :func:`reg_e_step`, per target point and level, with the margins that decide them.

    All arrays are [N, max_level]; entries of levels a point does not reach (it stopped above) are -1 / False / inf.
      node         the child the point moves to (j0 + argmax gamma; j0 itself when den <= EPS)
      contrib      whether that (point, node) pair adds to the moments (not stopped, gamma >= EPS)
      gap          (g_max - g_second) / g_max of the eight children (inf when den <= EPS: the first child is forced)
      den_margin   |den - EPS| / EPS            (which side of the normaliser test)
      gamma_margin |gamma_chosen - EPS| / EPS   (inf where the point stops: gamma is not used there)
      cplx_margin  |complexity(cov_node) - lc| / lc
    A small margin means that a different but equally valid rounding can take the other branch."""
    points = np.asarray(points, dtype=np.float64)
    shape = (len(points), max_level)
    node = -np.ones(shape, dtype=np.int64)
    contrib = np.zeros(shape, dtype=bool)
    gap, den_m, gam_m, cplx_m = (np.full(shape, np.inf) for _ in range(4))
    for l, idx, _, g, den, good, s, gs, cs, stop in _descend(points, pi, mu, cov, max_level, lc):
        top2 = np.sort(g, axis=1)[:, -2:]
        gap[idx, l] = np.where(good, (top2[:, 1] - top2[:, 0]) / np.where(good, top2[:, 1], 1.0), np.inf)
        den_m[idx, l] = np.abs(den - EPS) / EPS
        cplx_m[idx, l] = np.abs(cs - lc) / lc
        node[idx, l] = s
        gam_m[idx, l] = np.where(stop, np.inf, np.abs(gs - EPS) / EPS)
        contrib[idx, l] = ~stop & ~(gs < EPS)
    return RegDescent(node, contrib, gap, den_m, gam_m, cplx_m)


def reg_near_ties(desc, rel=1e-9):
    """[N] bool: the points whose descent (:func:`reg_descent`) has a margin below ``rel`` at some level."""
    m = np.minimum(np.minimum(desc.gap, desc.den_margin), np.minimum(desc.gamma_margin, desc.cplx_margin))
    return (m < rel).any(axis=1)


def reg_normal_equations(m0, m1, mu, cov):
    """A^T A [6,6], A^T b [6], b^T b and the stacked (A, b) of :func:`reg_m_step`'s least-squares system, built with one
    batched ``eigh`` over the nodes with m0 >= float32 eps instead of a Python loop over all T nodes (the rows of nodes
    without mass are zero in reg_m_step and are left out here)."""
    live = np.nonzero(~(m0 < F32_EPS))[0]
    lam, vec = np.linalg.eigh(cov[live])
    s = m1[live] / m0[live][:, None]
    nT = np.transpose(vec * np.sqrt(m0[live][:, None] / lam)[:, None, :], (0, 2, 1))     # rows: scaled eigenvectors
    A = np.empty((len(live), 3, 6))
    A[:, :, :3] = np.cross(s[:, None, :], nT)
    A[:, :, 3:] = nT
    b = np.einsum('nij,nj->ni', nT, mu[live]) - np.einsum('nij,nj->ni', nT, s)
    A, b = A.reshape(-1, 6), b.reshape(-1)
    return A.T @ A, A.T @ b, float(b @ b), A, b
