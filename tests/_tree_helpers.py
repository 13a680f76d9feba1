"""What the tree tests of the gate and of the per-point weights share (a helper, not a conftest and not an oracle: the
float64 arithmetic they compare against is oracle/hgmm_tree.py alone): ``weights_for``, ``resident``, ``loop5``,
``same_bits``; and what the deep-build tests (test_tree_build_depth_cpu.py / _gpu.py) share: ``deep_cloud``, ``ll_split``,
``build_fairness``, the case tables ``DEEP_CASES`` / ``plan_sizes`` and their cached oracle runs."""
import functools
from collections import namedtuple

import numpy as np

from oracle import hgmm_tree

I3 = np.identity(3)


def weights_for(n, seed=11):
    """the tests' weights unless stated otherwise: uniform in [0.25, 4), one in ten exactly zero"""
    rs = np.random.RandomState(seed)
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


# ---- deep builds (L = 5, 6) and the plan's boundaries in n, held to the oracle ------------------------------------------

def deep_cloud(seed, n=2500, branching=(3, 3, 3, 2, 2), offset=2.5, shrink=2.6, noise=0.03):
    """A seeded cloud whose populated branches go six levels down: a recursive cluster tree (3 sub-clusters per cluster for
    three levels, 2 thereafter: 108 leaf clusters), sub-cluster offsets shrinking by ``shrink`` per level, isotropic noise
    about the leaf centres.  Coordinates of order 1 to 10, so that the covariances of deep nodes keep det far above 1e-15
    (at the bunny's 0.1 m scale they fall below it and a deep test would compare dead nodes only)."""
    rs = np.random.RandomState(seed)
    centres = np.zeros((1, 3))
    for b in branching:
        centres = (centres[:, None, :] + offset * rs.randn(len(centres), b, 3)).reshape(-1, 3)
        offset /= shrink
    return centres[rs.randint(len(centres), size=n)] + noise * rs.randn(n, 3)


def deep_init(seed, n, L):
    """init_idx = RandomState(seed).randint(n, size=T).  T is far above n, so many sibling groups draw the same point twice:
    such siblings stay bitwise equal for ever, their gammas tie exactly, and the first-max arg-max rule decides."""
    return np.random.RandomState(seed).randint(n, size=hgmm_tree.n_total(L))


def integer_weights(n, seed=11):
    """integer weights 0 .. 5: about a sixth of the points carry weight 0, so deep nodes die by weight"""
    return np.random.RandomState(seed).randint(0, 6, size=n).astype(np.float64)


def ll_split(llblocks, n_level, cus, tile=256):
    """tree_ll_split (csrc/tree_device.h) restated: how a level's nodes are split over the log-likelihood grid of a small
    cloud.  -> (chunks, nodes per chunk)"""
    chunks = 1
    if llblocks < 2 * cus and n_level > tile:
        chunks = min((4 * cus + llblocks - 1) // llblocks, (n_level + tile - 1) // tile)
    per_chunk = ((n_level + chunks - 1) // chunks + tile - 1) // tile * tile
    return (n_level + per_chunk - 1) // per_chunk, per_chunk


Fairness = namedtuple('Fairness', ['pi', 'mu', 'cov', 'trace', 'stop', 'ld', 'det', 'den', 'gap', 'ties', 'ties_bitwise',
                                   'forced', 'live', 'leaves'])


def build_fairness(points, L, ls, ld, init_idx, sig2, budget, w=None, ll_chunk=4096):
    """ONE run of the oracle's build -- the loop of hgmm_tree.build_tree over the oracle's own e_step / m_step /
    log_likelihood, bit for bit build_tree(..., ll_chunk=ll_chunk) (test_tree_build_depth_cpu.py checks that) -- which also
    notes how far every decision was from going the other way under a last-bit difference:
      stop   min ||dq| - ls| / ls over the trace (hgmm_tree.stop_margins)
      ld     min |m0 - ld| / ld over the level's nodes with m0 > 0, every M-step
      det    min |det - EPS| / EPS over the level's live nodes (pi > 0), after every M-step
      den    min |den - EPS| / EPS over the points, every E-step
      gap    the smallest NON-ZERO difference of a point's two largest gammas, every E-step
      ties   how many (point, E-step) pairs have the two largest gammas exactly equal (den > EPS); ties_bitwise: whether in
             every one of them all the children at the maximum have bitwise-equal pi, mu and cov (then every arithmetic ties)
      forced how many (point, E-step) pairs have den <= EPS: all gammas are 0 and the first child is taken; the den margin
             covers that decision
      live   per level, the nodes left with pi > 0 and det >= EPS;  leaves: distinct leaves the points reach"""
    o = hgmm_tree
    points = np.asarray(points, dtype=np.float64)
    pi, mu, cov = o.init_nodes(points, L, init_idx, sig2)
    n = len(points)
    n_points = n
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64)
        n_points = o.weight_sum(w)
    parent = -np.ones(n, dtype=np.int64)
    q_trace, iters, cur_levels, live = [], [], [], []
    m_ld = m_det = m_den = m_gap = np.inf
    ties, ties_bitwise, forced = 0, True, 0
    for l in range(L):
        lb, le = o.level(l), o.level(l + 1)
        prev_q, it = 0.0, 0
        while True:
            kid, _, den, good, _ = o.child_gamma(points, o.child(parent), pi, mu, *o.node_prep(cov)[1:])
            m_den = min(m_den, float((np.abs(den - o.EPS) / o.EPS).min()))
            forced += int((~good).sum())
            m0, m1, m2, cur, gamma = o.e_step(points, pi, mu, cov, parent, w=w)
            top = np.sort(gamma, axis=1)[:, -2:]
            d = (top[:, 1] - top[:, 0])[good]
            if (d > 0).any():
                m_gap = min(m_gap, float(d[d > 0].min()))
            for i in np.nonzero(good)[0][d == 0]:
                at = kid[i][gamma[i] == gamma[i].max()]
                ties += 1
                ties_bitwise &= all(pi[j] == pi[at[0]] and np.array_equal(mu[j], mu[at[0]])
                                    and np.array_equal(cov[j], cov[at[0]]) for j in at[1:])
            mass = m0[lb:le]
            m_ld = min(m_ld, float((np.abs(mass[mass > 0] - ld) / ld).min()))
            o.m_step(m0, m1, m2, l, pi, mu, cov, n_points, ld)
            alive = np.nonzero(pi[lb:le] > 0)[0] + lb
            m_det = min(m_det, float((np.abs(o.det3(cov[alive]) - o.EPS) / o.EPS).min())) if len(alive) else m_det
            q = o.log_likelihood(points, pi, mu, cov, l, chunk=ll_chunk, w=w)
            q_trace.append(q)
            it += 1
            if abs(q - prev_q) < ls or it >= budget:
                break
            prev_q = q
        iters.append(it)
        cur_levels.append(cur.copy())
        parent = cur.copy()
        alive = np.nonzero(pi[lb:le] > 0)[0] + lb
        live.append(int((o.det3(cov[alive]) >= o.EPS).sum()))
    trace = o.BuildTrace(np.array(q_trace), np.array(iters), cur_levels)
    stop = float(o.stop_margins(trace.q, trace.iters_per_level, ls).min())
    return Fairness(pi, mu, cov, trace, stop, m_ld, m_det, m_den, m_gap, ties, ties_bitwise, forced, live,
                    len(np.unique(cur_levels[-1])))


def unfair(f):
    """the conditions a Fairness must meet before leaves and iteration counts may be compared exactly -> those it misses"""
    checks = [("stop margin", f.stop, 1e-6), ("ld margin", f.ld, 1e-6), ("det margin", f.det, 1e-6),
              ("den margin", f.den, 1e-6), ("non-zero gamma gap", f.gap, 1e-9)]
    out = ["%s %.3g < %g" % (name, v, bound) for name, v, bound in checks if not v >= bound]
    return out if f.ties_bitwise else out + ["an exact gamma tie between children that are not bitwise equal"]


DEEP_N, DEEP_SIG2, DEEP_LD, DEEP_LL_CHUNK = 2500, 0.5, 1e-4, 512
# name -> (L, cloud seed, ls, ls of the weighted build, budget).  "budget": ls = 1e-30 never stops a level, every level runs to the budget and the
# closing launch decides; "stop": every level is stopped by ls.  (The oracle's Python M-step visits 262 144 nodes per
# level-5 iteration: the L = 6 budget is small, and the L = 6 stop case takes a larger ls so that levels stop early.  The
# weighted build's q is a sum over the total weight, 2.5 n with integer_weights: its ls is larger accordingly.)
DEEP_CASES = {
    "L5_budget": (5, 55, 1e-30, 1e-30, 6),
    "L6_budget": (6, 65, 1e-30, 1e-30, 4),
    "L5_stop": (5, 51, 2.0, 5.0, 40),
    "L6_stop": (6, 61, 20.0, 80.0, 40),
}


def deep_inputs(name, weighted=False):
    """-> (points, L, ls, ld, init_idx, sig2, budget) of a DEEP_CASES row"""
    L, seed, ls, ls_w, budget = DEEP_CASES[name]
    P = deep_cloud(seed, DEEP_N)
    return P, L, (ls_w if weighted else ls), DEEP_LD, deep_init(seed, DEEP_N, L), DEEP_SIG2, budget


@functools.lru_cache(maxsize=None)
def deep_oracle(name, weighted=False):
    """the case's Fairness, computed once per process; the arrays are shared: leave them unchanged"""
    w = integer_weights(DEEP_N) if weighted else None
    return build_fairness(*deep_inputs(name, weighted), w=w, ll_chunk=DEEP_LL_CHUNK)


def order_spread(name, weighted=False):
    """How far two legitimate float64 summation orders of the oracle end up from each other on a deep case: the points in
    index order (deep_oracle) and reversed (weights and initial means reversed with them, so it is the same problem).  Every
    E-step's rounding differs in the last bit and the EM iterations carry that along.  -> for q, pi, mu, cov the largest
    |a - b| / (|b| + floor) with the floors DEPTH_TOL pairs with its rtol, and whether iterations and leaves agree.
    This is where DEPTH_TOL comes from (10 x the largest spread); the suite runs it on the cheapest case only."""
    P, L, ls, ld, idx, sig2, budget = deep_inputs(name, weighted)
    n = len(P)
    w = integer_weights(n) if weighted else None
    a = deep_oracle(name, weighted)
    b = build_fairness(P[::-1].copy(), L, ls, ld, n - 1 - idx, sig2, budget, w=None if w is None else w[::-1].copy(),
                       ll_chunk=DEEP_LL_CHUNK)
    same = (list(a.trace.iters_per_level) == list(b.trace.iters_per_level)
            and all(np.array_equal(x, y[::-1]) for x, y in zip(a.trace.current_idx_per_level, b.trace.current_idx_per_level)))
    out = {}
    for key, x, y in (("q", a.trace.q, b.trace.q), ("pi", a.pi, b.pi), ("mu", a.mu, b.mu), ("cov", a.cov, b.cov)):
        if x.shape == y.shape:
            out[key] = depth_excess(x, y, key, 1.0, DEEP_COORD2)
    return out, same


# ---- tolerances of the deep comparisons ---------------------------------------------------------------------------------
# tests/test_tree_gpu.py holds this path to rtol / atol = 1e-9 / 1e-6 (q), 1e-9 / 1e-13 (pi), 1e-9 / 1e-12 (mu) and 1e-6 /
# 1e-14 (cov, on the bunny's coordinates of order 0.1 .. 1; a covariance is a difference of second moments, its rounding
# grows with the SQUARE of the coordinates, so 1e-14 x 4^2 for the deep clouds, whose coordinates reach 4).  Written as
# |a - b| <= r (|b| + floor) with floor = atol / rtol that is:
DEPTH_RTOL = {"q": 1e-9, "pi": 1e-9, "mu": 1e-9, "cov": 1e-6}
DEPTH_FLOOR = {"q": 1e3, "pi": 1e-4, "mu": 1e-3, "cov": 1e-8}          # (cov: times the squared coordinate scale)
DEEP_COORD2 = 16.0
# At depth these are too tight for ANY second float64 arithmetic: a build is 50 to 140 EM iterations, each carries the
# last-bit differences of the one before along, and small deep nodes (a handful of points) amplify them.  Measured, not
# felt: order_spread() above, the oracle against itself with the points reversed, largest |a - b| / (|b| + floor):
DEEP_SPREAD = {
    ("L5_budget", False): {"q": 4.5e-11, "pi": 3.4e-9, "mu": 3.2e-10, "cov": 2.2e-8},
    ("L5_budget", True): {"q": 1.1e-10, "pi": 1.5e-8, "mu": 2.9e-9, "cov": 2.7e-7},
    ("L6_budget", False): {"q": 5.3e-11, "pi": 7.5e-9, "mu": 1.7e-9, "cov": 1.2e-7},
    ("L6_budget", True): {"q": 7.1e-10, "pi": 5.5e-7, "mu": 7.7e-8, "cov": 3.5e-6},
    ("L5_stop", False): {"q": 8.2e-9, "pi": 1.3e-8, "mu": 6.7e-10, "cov": 9.2e-8},
    ("L5_stop", True): {"q": 1.7e-8, "pi": 6.6e-9, "mu": 4.5e-10, "cov": 6.9e-8},
    ("L6_stop", False): {"q": 5.4e-11, "pi": 3.5e-9, "mu": 8.0e-10, "cov": 2.3e-7},
    ("L6_stop", True): {"q": 3.1e-9, "pi": 1.1e-7, "mu": 8.1e-9, "cov": 2.0e-7},
}
# (iterations and leaves of the two orders agree on every case.)  The device is allowed 10 x the case's spread where that
# is more than the rtol above, and the rtol above where it is not; the plan-boundary cases (two iterations per level) keep
# the tolerances above as they are.


def depth_rtol(case=None):
    """key -> r of |a - b| <= r (|b| + DEPTH_FLOOR[key]); ``case`` = (name, weighted) of DEEP_SPREAD, None: DEPTH_RTOL"""
    if case is None:
        return dict(DEPTH_RTOL)
    return {key: max(DEPTH_RTOL[key], 10.0 * DEEP_SPREAD[case][key]) for key in DEPTH_RTOL}


def depth_excess(a, b, key, r, coord2=1.0):
    """largest |a - b| / (r (|b| + floor)): <= 1 passes.  ``coord2``: the cloud's squared coordinate scale (cov's floor)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    floor = DEPTH_FLOOR[key] * (coord2 if key == "cov" else 1.0)
    return float((np.abs(a - b) / (r * (np.abs(b) + floor))).max())


# ---- the plan's boundaries in n (build_plan, tree_ll_split) -------------------------------------------------------------
PLAN_SIG2, PLAN_BUDGET, PLAN_LS, PLAN_LD = 0.01, 2, 1e-30, 1e-4


def plan_sizes(cus):
    """(tag, n, L, weighted) on either side of: the two-pass E-step (n / 256 > 3 cus), the last split log-likelihood launch
    (ceil(n / 512) >= 2 cus switches it off; needs a level of more than one 256-node tile, so L = 3) and the four-point
    log-likelihood / the end of the overlapped form (n >= 400 000).  The two pairs that do not ask about the split run at
    L = 2, where the oracle costs an eighth."""
    half = 256 * (3 * cus) + 255
    split = 512 * (2 * cus - 1)
    return [("estep_one_pass", half, 2, False), ("estep_two_pass", half + 1, 2, False),
            ("estep_one_pass_w", half, 2, True), ("estep_two_pass_w", half + 1, 2, True),
            ("ll_split_last", split, 3, False), ("ll_unsplit_first", split + 1, 3, False),
            ("ll_two_points", 399_999, 2, False), ("ll_four_points", 400_000, 2, False)]


def plan_cloud(n, seed=7, k=40, spread=0.02):
    """a 40-blob cloud in the unit cube"""
    rs = np.random.RandomState(seed)
    centres = rs.rand(k, 3)
    which = rs.randint(k, size=n)
    return centres[which] + spread * (0.5 + rs.rand(k, 3))[which] * rs.randn(n, 3)


def plan_inputs(n, L):
    P = plan_cloud(n)
    return P, L, PLAN_LS, PLAN_LD, np.random.RandomState(3).randint(n, size=hgmm_tree.n_total(L)), PLAN_SIG2, PLAN_BUDGET


@functools.lru_cache(maxsize=None)
def plan_oracle(n, L, weighted=False):
    w = integer_weights(n) if weighted else None
    return build_fairness(*plan_inputs(n, L), w=w)
