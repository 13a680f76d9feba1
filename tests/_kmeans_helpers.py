"""Inputs and the iteration-by-iteration oracle shared by tests/test_kmeans_lloyd_cpu.py (which proves, on the oracle
alone, that every input is a fair one) and tests/test_kmeans_lloyd_gpu.py (which holds the device to the oracle on them).

``walk`` is ``oracle.kmeans.lloyd`` opened up: the same calls in the same order, with what every iteration saw kept.
The CPU test asserts that it returns exactly what ``lloyd`` returns on every input used, so it cannot drift."""
import functools
from collections import namedtuple

import numpy as np

from conftest import load_golden
from oracle import kmeans as okm

Walk = namedtuple("Walk", "labels margin shift n_empty changed centres_in centres n_iter strict final_labels")


def walk(Xc, init, max_iter, tol_abs):
    """The oracle's Lloyd loop.  Per iteration i (0-based; iteration number i + 1): labels[i], margin[i] = min over
    points of (second smallest d2 - smallest d2) (inf at k = 1), shift[i] = summed squared centre shift, n_empty[i] =
    empty clusters before relocation, changed[i] = labels that differ from the previous iteration's (all n in the
    first), centres_in[i] = the centres the iteration assigned to.  Then the final centres, n_iter, strict and the
    labels ``lloyd`` reports (the last assignment when strict, one more assignment otherwise)."""
    X = np.asarray(Xc, dtype=np.float64)
    centres = np.array(init, dtype=np.float64)
    k = len(centres)
    old = np.full(len(X), -1, dtype=np.int32)
    labels, margin, shift, n_empty, changed, centres_in = [], [], [], [], [], []
    strict = False
    for _ in range(max_iter):
        d = okm._sq_dists(X, centres)
        lab = np.argmin(d, axis=1).astype(np.int32)
        if k > 1:
            p = np.partition(d, 1, axis=1)
            margin.append(float((p[:, 1] - p[:, 0]).min()))
        else:
            margin.append(np.inf)
        sums = np.zeros((k, 3))
        np.add.at(sums, lab, X)
        counts = np.bincount(lab, minlength=k).astype(np.float64)
        n_empty.append(int((counts == 0).sum()))
        okm._relocate_empty(X, centres, sums, counts, lab)
        new = sums.copy()
        pos = counts > 0
        new[pos] *= (1.0 / counts[pos])[:, None]
        s = np.sqrt(((new - centres) ** 2).sum(axis=1))
        shift.append(float((s ** 2).sum()))
        labels.append(lab)
        changed.append(int((lab != old).sum()))
        centres_in.append(centres)
        centres = new
        if np.array_equal(lab, old):
            strict = True
            break
        if shift[-1] <= tol_abs:
            break
        old = lab
    n_iter = len(labels)
    if strict or n_iter == 0:
        final = labels[-1] if n_iter else old
    else:
        final = okm.assign(X, centres)[0]
    return Walk(labels, margin, shift, n_empty, changed, centres_in, centres, n_iter, strict, final)


def step_sums(Xc, labels, k):
    """Per-cluster sums and counts of one assignment, as the oracle accumulates them."""
    sums = np.zeros((k, 3))
    np.add.at(sums, labels, Xc)
    return sums, np.bincount(labels, minlength=k).astype(np.float64)


# -- section 1: one step on a lattice --------------------------------------------------------------
LATTICE_CASES = [(1, 1), (1, 3), (63, 2), (255, 4), (256, 5), (257, 7), (511, 8), (512, 63), (513, 64), (1025, 65),
                 (2000, 129), (3000, 256), (3000, 257), (5000, 1024), (5000, 1025)]
LATTICE_SECOND_STEP = [(513, 64), (3000, 257)]


def duplicate_pairs(k):
    """(earlier, later) positions that hold bitwise the same centre, wherever k has them: inside one group of four,
    across groups, group against the scalar tail, both in the tail, across the 64-centre slot, the 256-centre
    allocation and the 1024-centre pass boundaries."""
    k4 = k & ~3
    pairs = [(0, 1), (2, 7)]
    if k % 4:
        pairs.append((k4 - 1, k4))
    if k % 4 >= 2:
        pairs.append((k - 2, k - 1))
    pairs += [(63, 64), (255, 256), (1023, 1024)]
    out = []
    for a, b in pairs:
        if 0 <= a < b < k and (a, b) not in out:
            out.append((a, b))
    return out


def _lattice(rs, shape):
    return rs.randint(-16, 17, size=shape) * 0.5         # multiples of 1/2 in [-8, 8]


def has_tie(X, C):
    """Per point: exactly equidistant from its two nearest centres of different coordinates (bitwise copies of one
    centre count once)."""
    U = np.unique(C, axis=0)
    if len(U) < 2:
        return np.zeros(len(X), dtype=bool)
    p = np.partition(okm._sq_dists(X, U), 1, axis=1)
    return p[:, 0] == p[:, 1]


@functools.lru_cache(maxsize=None)
def lattice_case(n, k):
    """Points and two centre sets with every coordinate a multiple of 1/2 in [-8, 8]: differences, squares, distances,
    sums and the inertia are exactly representable doubles in any order of evaluation, fused or not.  The centres are
    drawn from the points and then given the duplicates of ``duplicate_pairs`` (the later position copies the earlier
    one, in table order).  B keeps A's even positions and draws the odd ones again, for the step without a reset.
    Returns (X, A, B, pairs); the arrays are read-only."""
    rs = np.random.RandomState(7919 * k + n)
    X = _lattice(rs, (n, 3))
    A = X[rs.choice(n, k, replace=n < k)].copy()
    pairs = duplicate_pairs(k)
    for a, b in pairs:
        A[b] = A[a]
    if len(np.unique(A, axis=0)) >= 2 and not has_tie(X, A).any():
        # (a handful of centres leaves most points without a tie: the last point moves to the first lattice site
        # that is equidistant from its two nearest centres, of different coordinates)
        axis = np.arange(-16, 17) * 0.5
        G = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
        X[n - 1] = G[np.flatnonzero(has_tie(G, A))[0]]
    B = A.copy()
    B[1::2] = X[rs.choice(n, len(B[1::2]), replace=True)]
    for arr in (X, A, B):
        arr.setflags(write=False)
    return X, A, B, pairs


def lattice_expect(X, C):
    """What one step has to give, exactly: labels (np.argmin, first minimum), squared distance to the winner, counts,
    sums, inertia; and the full distance table for the fairness checks."""
    d = okm._sq_dists(X, C)
    lab = np.argmin(d, axis=1).astype(np.int32)
    mind2 = d[np.arange(len(X)), lab]
    sums, counts = step_sums(X, lab, len(C))
    return lab, mind2, counts, sums, float(mind2.sum()), d


# -- section 2: the whole loop at every accumulator layout ---------------------------------------
LOOP_CASES = [(3000, 65), (4000, 200), (5000, 300), (6000, 1100)]
MARGIN_MIN = 1e-10             # five orders above the two sides' summation-order noise (~1e-15 on unit-scale data)


@functools.lru_cache(maxsize=None)
def loop_case(n, k):
    rs = np.random.RandomState(n + k)
    X = rs.rand(n, 3) * [1.0, 2.0, 0.5]
    Xc = X - X.mean(axis=0)
    init = Xc[rs.choice(n, k, replace=False)]
    Xc.setflags(write=False)
    init.setflags(write=False)
    return Xc, init


@functools.lru_cache(maxsize=None)
def loop_walk(n, k):
    Xc, init = loop_case(n, k)
    return walk(Xc, init, 60, 0.0)


def assert_fair(w):
    """The condition under which labels and iteration counts of two float64 implementations must be identical: no
    point within MARGIN_MIN of a tie in any iteration, no cluster ever empty."""
    assert min(w.margin) >= MARGIN_MIN, min(w.margin)
    assert sum(w.n_empty) == 0, w.n_empty


# -- section 3: stop rules on the golden 'uniform' cloud (k = 16); tolerance stops also on 'blobs' (k = 20) ----
BUDGETS = [1, 7, 8, 9, 16, 17]
SPLITS = [(3, 5), (8, 1), (9, 10)]
STRICT_AT = {"uniform": 19, "blobs": 16}
# Iterations at which a tolerance stops the loop: the last of a batch of 8, the first of the next, one inside.
# A tolerance stops at iteration m only if that iteration's shift lies below every earlier one.  The 'uniform'
# trajectory's shift rises from iteration 7 to 8 (8.33e-4 -> 9.62e-4), so no tolerance stops it at 8; 'blobs' allows
# all three (tests/test_kmeans_lloyd_cpu.py asserts both statements).
TOL_STOPS = [("blobs", 8), ("blobs", 9), ("blobs", 12), ("uniform", 9), ("uniform", 12)]


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """Centred cloud and start (the reference's own seeds) of a case of tests/golden/kmeans_init.npz."""
    g = load_golden("kmeans_init.npz")
    X = g[name + "_X"]
    Xc = X - X.mean(axis=0)
    init = Xc[g[name + "_init_indices"]]
    assert len(init) == int(g[name + "_k"])
    Xc.setflags(write=False)
    init.setflags(write=False)
    return Xc, init


@functools.lru_cache(maxsize=None)
def golden_walk(name, max_iter=50, tol_abs=0.0):
    Xc, init = golden_case(name)
    return walk(Xc, init, max_iter, tol_abs)


def tol_for_stop(name, m):
    """A tolerance that stops the trajectory at iteration m and nowhere near a decision: the geometric mean of
    iteration m's shift and the smallest earlier one (iteration m - 1's wherever the shifts fall monotonically)."""
    s = golden_walk(name).shift
    return float(np.sqrt(s[m - 1] * min(s[:m - 1])))


# -- section 4: empty clusters handed to the host -------------------------------------------------
def fit_inputs(X, init):
    """What ``KMeans(init=init, tol=tol).fit(X)`` works on: the centred cloud, the centred start and the absolute
    tolerance, as scikit-learn (and ``oracle.kmeans.fit``) derive them."""
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    return X - mean, np.asarray(init, dtype=np.float64) - mean, float(np.mean(np.var(X, axis=0)) * 1e-4)


RELOC8_ROWS = [0, 40, 80, 120, 160]         # the five distinct start centres (rows of the cloud)
RELOC8_LAYOUT = [0, 1, 0, 2, 3, 1, 4, 3]    # position -> distinct centre: positions 2, 5 and 7 are bitwise copies


@functools.lru_cache(maxsize=None)
def reloc8_case():
    """The 'reloc' golden's cloud with an explicit start of k = 8 in which three centres are bitwise copies of others:
    three clusters are empty in iteration 1.  Returns (X, init) in the cloud's own frame."""
    X = np.array(load_golden("kmeans_init.npz")["reloc_X"], dtype=np.float64)
    init = X[RELOC8_ROWS][RELOC8_LAYOUT].copy()
    X.setflags(write=False)
    init.setflags(write=False)
    return X, init


# (n, k, blobs, spread, seed, iteration of the first empty cluster): three clouds whose first empty cluster comes in
# iteration 2 and the latest one a bounded search turned up (iteration 4; 82 000 blob clouds of six shapes, 240 s of
# CPU, none later -- so nothing here meets its first empty cluster in a later batch of 8)
LATE_EMPTY_CASES = [(60, 20, 5, 0.05, 343, 2), (60, 20, 5, 0.05, 165, 2), (60, 20, 5, 0.05, 39, 2),
                    (120, 40, 6, 0.08, 30, 4)]


@functools.lru_cache(maxsize=None)
def late_empty_case(n, k, blobs, spread, seed):
    """n points in a few blobs, centred, started from k of the points."""
    rs = np.random.RandomState(seed)
    c = rs.rand(blobs, 3) * [1.0, 2.0, 0.5]
    X = c[rs.randint(0, blobs, n)] + rs.randn(n, 3) * spread
    X = X - X.mean(axis=0)
    init = X[np.random.RandomState(seed).choice(n, k, replace=False)]
    X.setflags(write=False)
    init.setflags(write=False)
    return X, init


def relocation_gap(Xc, w):
    """Smallest difference between two of the e + 1 largest point-to-own-centre distances, over the iterations that
    relocate e > 0 empty clusters: which points move, and to which cluster, is decided by their order."""
    gap = np.inf
    for lab, c, e in zip(w.labels, w.centres_in, w.n_empty):
        if e:
            dist = np.sort(((Xc - c[lab]) ** 2).sum(axis=1))[-(e + 1):]
            gap = min(gap, float(np.diff(dist).min()))
    return gap


def first_empty(w):
    """Iteration number (1-based) of the first iteration that met an empty cluster, or None."""
    hit = [i + 1 for i, e in enumerate(w.n_empty) if e]
    return hit[0] if hit else None
