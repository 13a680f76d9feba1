"""The weighted KMeans initialiser restated in NumPy float64, and the inputs shared by tests/test_kmeans_weights_cpu.py
(which proves, on this restatement alone, that every input is a fair one and pins the restatement to live scikit-learn)
and tests/test_kmeans_weights_gpu.py (which holds the device to it).

The contract is scikit-learn 1.7.2's ``KMeans(n_clusters=k, random_state=..., max_iter=..., n_init=1, tol=...)
.fit(X, sample_weight=w)``.  Four statements of the unweighted algorithm (``oracle/kmeans.py``) change, nothing else:

1. the first seed is ``rs.choice(n, p=w / w.sum())``;
2. k-means++: ``closest`` stays the unweighted squared distance; the potential is ``sum w closest``, the candidates are
   ``searchsorted(cumsum(w * closest), u * pot)`` clipped to n - 1, a candidate's potential is
   ``sum w min(closest, d2(., cand))``, first minimum wins;
3. Lloyd: assignment, labels, per-point distance and changed-label count do not see the weights; the per-cluster sums
   are ``sum w x`` and the count becomes the weight in the cluster; centres = sums * (1 / weight) where the weight is
   > 0; the inertia is ``sum w d2``; a cluster is empty when its weight is 0; shift and stop rules unchanged;
4. relocation: the farthest points by the UNWEIGHTED distance to their own old centre, in ``np.argpartition`` order;
   the moved point carries ``w x`` and ``w`` from its old cluster to the new one.

The mean that centres X and the variance that scales ``tol`` stay unweighted; the weights are not rescaled.

Zero weights together with an empty cluster bring in two more statements of scikit-learn 1.7.2 (``_k_means_common.pyx``),
which the unweighted algorithm never reaches because a relocated cluster there always holds one point:

5. ``_average_centers``: a cluster whose weight is STILL 0 after relocation (the point it was given has weight 0) takes the
   row of the heaviest cluster (``np.argmax`` of the weights, first maximum) AS THAT ROW STANDS when the in-order sweep
   over the clusters reaches it: already averaged if the heaviest cluster comes earlier in the table, the raw ``sum w x``
   if it comes later;
6. ``_relocate_empty_clusters_dense`` returns without relocating when the largest distance is 0.

``test_zero_weight_relocation_matches_live_sklearn`` pins both on the ``reloc8_case`` cloud with 30 % zero weights."""
import functools
from collections import namedtuple

import numpy as np

import _kmeans_helpers as H
from oracle import kmeans as okm

SeedTrace = namedtuple("SeedTrace", "thr_margin pot_gap")
WalkW = namedtuple("WalkW", "labels margin shift n_empty changed centres_in centres n_iter strict final_labels inertia")


def kmeans_plusplus_w(X, k, rs, w, uniforms=None, first=None):
    """Statements 1 and 2.  X centred.  ``uniforms`` [(k-1), trials] replaces ``rs.uniform`` and ``first`` the first
    draw (the GPU tests hand both to the device).  Returns (centres, ids, SeedTrace): per step the smallest distance of
    a threshold to its two neighbouring running-sum values and the gap between the best and the second-best DISTINCT
    candidate's potential, both relative to the potential (inf where there is no second candidate)."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = len(X)
    trials = okm.n_local_trials(k)
    if first is None:
        first = rs.choice(n, p=w / w.sum())
    idx = np.full(k, -1, dtype=np.int64)
    idx[0] = first
    closest = ((X - X[first]) ** 2).sum(axis=1)
    pot = (w * closest).sum()
    thr_margin, pot_gap = [], []
    for c in range(1, k):
        u = rs.uniform(size=trials) if uniforms is None else np.asarray(uniforms[c - 1], dtype=np.float64)
        r = u * pot
        cum = np.cumsum(w * closest, dtype=np.float64)
        cand = np.searchsorted(cum, r)
        below = np.where(cand > 0, cum[np.maximum(cand - 1, 0)], 0.0)
        above = cum[np.minimum(cand, n - 1)]
        thr_margin.append(float(np.minimum(np.abs(r - below), np.abs(above - r)).min() / pot))
        np.clip(cand, None, n - 1, out=cand)
        d = np.minimum(closest[None, :], okm._sq_dists(X[cand], X))        # [trials, n]
        pots = (d * w[None, :]).sum(axis=1)
        best = int(np.argmin(pots))
        others = np.array([pots[t] for t in range(trials) if cand[t] != cand[best]])
        pot_gap.append(float((others.min() - pots[best]) / pot) if len(others) else np.inf)
        pot = pots[best]
        closest = d[best]
        idx[c] = cand[best]
    return X[idx].copy(), idx, SeedTrace(thr_margin, pot_gap)


def relocate_empty_w(X, w, centres_old, sums, wsum, labels):
    """Statement 4 (labels are not updated)."""
    empty = np.where(wsum == 0)[0]
    if len(empty) == 0:
        return
    dist = ((X - centres_old[labels]) ** 2).sum(axis=1)
    far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
    if dist.max() == 0:
        return
    for new_id, far_idx in zip(empty, far):
        old_id = labels[far_idx]
        sums[old_id] -= X[far_idx] * w[far_idx]
        sums[new_id] = X[far_idx] * w[far_idx]
        wsum[new_id] = w[far_idx]
        wsum[old_id] -= w[far_idx]


def average_centres_w(sums, wsum):
    """Statements 3 and 5: sums * (1 / weight) where the weight is > 0; a cluster of weight 0 copies the heaviest cluster's
    row as the sweep in table order finds it."""
    new = sums.copy()
    amax = int(np.argmax(wsum))
    for j in range(len(new)):
        if wsum[j] > 0:
            new[j] *= 1.0 / wsum[j]
        else:
            new[j] = new[amax]
    return new


def step_sums_w(X, w, labels, k):
    """Per-cluster ``sum w x`` and weight of one assignment."""
    sums = np.zeros((k, 3))
    np.add.at(sums, labels, X * w[:, None])
    return sums, np.bincount(labels, weights=w, minlength=k).astype(np.float64)


def lloyd_w(X, w, init, max_iter, tol_abs):
    """Statement 3 (+ 4), opened up like ``_kmeans_helpers.walk``: per iteration the labels, the label margin (min over
    points of second smallest d2 - smallest d2; inf at k = 1), the summed squared shift, the clusters of weight 0
    before relocation, the changed labels and the centres assigned to; then centres, n_iter, strict, the labels the
    fit reports and the inertia ``sum w d2`` against the final centres."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
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
        sums, wsum = step_sums_w(X, w, lab, k)
        n_empty.append(int((wsum == 0).sum()))
        relocate_empty_w(X, w, centres, sums, wsum, lab)
        new = average_centres_w(sums, wsum)
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
    inertia = float((w * ((X - centres[final]) ** 2).sum(axis=1)).sum()) if n_iter else 0.0
    return WalkW(labels, margin, shift, n_empty, changed, centres_in, centres, n_iter, strict, final, inertia)


def fit_w(X, w, k, random_state=1, max_iter=50, tol=1e-4, init=None):
    """``KMeans(n_clusters=k, random_state=random_state, max_iter=max_iter, n_init=1, tol=tol[, init=init])
    .fit(X, sample_weight=w)`` -> dict(cluster_centers_, labels_, inertia_, n_iter_, init_indices, walk, seed_trace)."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    tol_abs = 0.0 if tol == 0 else float(np.mean(np.var(X, axis=0)) * tol)
    mean = X.mean(axis=0)
    Xc = X - mean
    if init is None:
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        start, idx, trace = kmeans_plusplus_w(Xc, k, rs, w)
    else:
        start, idx, trace = np.asarray(init, dtype=np.float64) - mean, None, None
    wk = lloyd_w(Xc, w, start, max_iter, tol_abs)
    return {"cluster_centers_": wk.centres + mean, "labels_": wk.final_labels, "inertia_": wk.inertia,
            "n_iter_": wk.n_iter, "init_indices": idx, "walk": wk, "seed_trace": trace}


def assert_fair_w(wk, allow_empty=False):
    """Labels and iteration counts of two float64 implementations must agree: no point within MARGIN_MIN of a tie in any
    iteration and (unless the case is about relocation) no cluster ever of weight 0."""
    assert min(wk.margin) >= H.MARGIN_MIN, min(wk.margin)
    if not allow_empty:
        assert sum(wk.n_empty) == 0, wk.n_empty


# -- the shape cases of seeding + one step: ragged blocks, the 4096-point group boundary, the 64-centre slot, the 256-centre
#    allocation, the 1024-centre pass (LDS accumulator up to k = 1024, register accumulator at k = 1100)
SEED_CASES = [(1, 1), (7, 7), (255, 3), (257, 64), (1000, 65), (4097, 5), (5000, 300), (20000, 1100)]
SEED_MARGIN_MIN = 1e-10     # of the potential: two float64 summation orders of n <= 20 000 non-negative terms differ by at
                            # most n * 2^-53 ~ 2e-12 relative, so the device's block order cannot flip a decision


@functools.lru_cache(maxsize=None)
def seed_case(n, k):
    """(Xc, w, first, uniforms): every draw from ``RandomState(n + k)`` in this order -- the cloud, the count weights 1..39,
    for n >= 255 the zeros (about a quarter) -- and the uniforms from ``RandomState(1)`` (first seed, then the steps)."""
    rs = np.random.RandomState(n + k)
    X = rs.rand(n, 3) * [1.0, 2.0, 0.5]
    Xc = X - X.mean(axis=0)
    w = rs.randint(1, 40, n).astype(np.float64)
    if n >= 255:
        w[rs.rand(n) < 0.25] = 0.0
    ru = np.random.RandomState(1)
    first = int(ru.choice(n, p=w / w.sum()))
    uniforms = ru.uniform(size=(max(k - 1, 0), okm.n_local_trials(k)))
    for a in (Xc, w, uniforms):
        a.setflags(write=False)
    return Xc, w, first, uniforms


@functools.lru_cache(maxsize=None)
def seed_expect(n, k):
    """The oracle's seeds of ``seed_case`` and one Lloyd step from them: (centres, ids, trace, labels, mind2, label margin)."""
    Xc, w, first, uniforms = seed_case(n, k)
    centres, ids, trace = kmeans_plusplus_w(Xc, k, None, w, uniforms=uniforms, first=first)
    d = okm._sq_dists(Xc, centres)
    lab = np.argmin(d, axis=1).astype(np.int32)
    margin = float((np.partition(d, 1, axis=1)[:, 1] - np.partition(d, 1, axis=1)[:, 0]).min()) if k > 1 else np.inf
    return centres, ids, trace, lab, d[np.arange(n), lab], margin


# -- exact arithmetic: lattice points, weights in {0, 1, 2, 4}
LATTICE_W_CASES = [(257, 7), (513, 64), (3000, 257), (5000, 1025)]


@functools.lru_cache(maxsize=None)
def lattice_weights(n, k):
    w = np.random.RandomState(31 * n + k).choice([0.0, 1.0, 2.0, 4.0], size=n)
    w.setflags(write=False)
    return w


# -- whole loop / invariants / stop rules: count weights on the clouds of _kmeans_helpers
@functools.lru_cache(maxsize=None)
def count_weights(n, seed, zeros=False):
    rs = np.random.RandomState(seed)
    w = rs.randint(1, 40, n).astype(np.float64)
    if zeros:
        w[rs.rand(n) < 0.3] = 0.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def loop_walk_w(n, k):
    Xc, init = H.loop_case(n, k)
    return lloyd_w(Xc, count_weights(n, n + k + 1), init, 60, 0.0)


# (the weight seed of the stop-rule trajectory: the 'uniform' cloud converges strictly after 25 iterations under these
#  counts, beyond the largest budget of 17; chosen on this restatement alone -- seeds 70..89 give 12 to 34 iterations)
STOP_WEIGHT_SEED = 73


@functools.lru_cache(maxsize=None)
def golden_walk_w(name, max_iter=50, tol_abs=0.0):
    Xc, init = H.golden_case(name)
    return lloyd_w(Xc, count_weights(len(Xc), STOP_WEIGHT_SEED), init, max_iter, tol_abs)


def tol_for_stop_w(name, m):
    """As ``_kmeans_helpers.tol_for_stop`` on the weighted trajectory: the geometric mean of iteration m's shift and the
    smallest earlier one."""
    s = golden_walk_w(name).shift
    return float(np.sqrt(s[m - 1] * min(s[:m - 1])))


def tol_stops_w(name):
    """Iterations m >= 2 at which a tolerance can stop the weighted trajectory (the shift lies below every earlier one
    and the loop has not converged strictly before): one inside the first batch of 8, one in a later batch."""
    wk = golden_walk_w(name)
    ok = [m for m in range(2, wk.n_iter) if wk.shift[m - 1] < min(wk.shift[:m - 1])]
    inside = [m for m in ok if m < 8]
    across = [m for m in ok if m > 8]
    return inside[-1], across[0]


# -- relocation
@functools.lru_cache(maxsize=None)
def reloc8_weights(zeros=False):
    X, _ = H.reloc8_case()
    return count_weights(len(X), 808, zeros)


@functools.lru_cache(maxsize=None)
def late_empty_pick():
    """The first cloud of ``LATE_EMPTY_CASES`` whose trajectory under count weights (seed = the cloud's) still meets a
    cluster of weight 0 after iteration 1, as (n, k, blobs, spread, seed, iteration) -- or None when none does."""
    for n, k, blobs, spread, seed, _ in H.LATE_EMPTY_CASES:
        Xl, il = H.late_empty_case(n, k, blobs, spread, seed)
        hit = H.first_empty(lloyd_w(Xl, count_weights(n, seed), il, 50, 0.0))
        if hit is not None and hit > 1:
            return n, k, blobs, spread, seed, hit
    return None


# -- the public layers: the bunny's 4 mm centroids with their counts
def voxel_centroids(P, size):
    """(centroids float64 [m,3], counts float64 [m]) of a voxel grid of edge ``size`` anchored at the cloud's minimum, voxels
    in lexicographic order of their integer coordinates."""
    P = np.asarray(P, dtype=np.float64)
    key = np.floor((P - P.min(axis=0)) / size).astype(np.int64)
    _, inv, counts = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(counts), 3))
    np.add.at(sums, inv, P)
    return sums / counts[:, None], counts.astype(np.float64)


@functools.lru_cache(maxsize=None)
def bunny_case():
    """(centroids, counts) of the ``bunny`` fixture at 4 mm, k = 100, and the restatement's fit of them."""
    import os
    from conftest import GOLDEN
    C, cnt = voxel_centroids(np.load(os.path.join(GOLDEN, "bun000_xyz.npy")), 0.004)
    C.setflags(write=False)
    cnt.setflags(write=False)
    return C, cnt, fit_w(C, cnt, BUNNY_K, random_state=1, max_iter=50, tol=1e-4)


BUNNY_K = 100

# -- many groups: the smallest size at which a thread of the seeding tail owns two group sums (more than 1024 groups of 4096)
MANY_N, MANY_K = 4300000, 5
MANY_MARGIN_MIN = 10 * MANY_N * 2.0 ** -53      # ten times the worst case of two summation orders of n non-negative terms


@functools.lru_cache(maxsize=None)
def many_groups_case():
    """(Xc, w, first, uniforms, ids, trace): count weights 1..39 with a quarter zeroed, the draws as in ``seed_case``."""
    n, k = MANY_N, MANY_K
    rs = np.random.RandomState(0)
    X = rs.rand(n, 3) * [1.0, 2.0, 0.5]
    Xc = X - X.mean(axis=0)
    w = rs.randint(1, 40, n).astype(np.float64)
    w[rs.rand(n) < 0.25] = 0.0
    ru = np.random.RandomState(1)
    first = int(ru.choice(n, p=w / w.sum()))
    uniforms = ru.uniform(size=(k - 1, okm.n_local_trials(k)))
    _, ids, trace = kmeans_plusplus_w(Xc, k, None, w, uniforms=uniforms, first=first)
    return Xc, w, first, uniforms, ids, trace
