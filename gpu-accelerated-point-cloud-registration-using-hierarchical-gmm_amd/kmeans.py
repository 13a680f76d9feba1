"""KMeans initialiser of the GMMReg flavour on the device.

The reference seeds its flat EM with ``sklearn.cluster.KMeans(n_clusters=k, random_state=1,
max_iter=50, n_init=1).fit(X).cluster_centers_`` (``src/python/gmmreg_gpu/gmm_impl.py:18-24``).
``KMeans`` below takes the same constructor arguments, exposes the attributes scikit-learn's
estimator leaves behind (``cluster_centers_``, ``labels_``, ``inertia_``, ``n_iter_``) and
follows scikit-learn 1.7's ``KMeans.fit`` step by step; the two O(N k) parts -- greedy k-means++
seeding and the Lloyd assignment / per-cluster sums -- run in HIP kernels
(``csrc/kmeans_kernels.hip``) on the float64 cloud, everything that touches only k x 3 numbers
(random draws, centre update, stop rule, empty-cluster relocation) stays here in NumPy:

* X is centred by its mean first, the mean is added back to the centres at the end;
* ``tol`` is scaled by the mean per-axis variance of X;
* the random stream is NumPy's ``RandomState(random_state)`` consumed in scikit-learn's order
  (one ``choice`` for the first centre, then ``2 + int(log k)`` uniforms per centre), so the same
  points are chosen as seeds;
* Lloyd: first nearest centre, centres = sum * (1 / count), empty clusters take the points
  farthest from their centre (``np.argpartition`` order, like scikit-learn), stop on unchanged
  labels or summed squared centre shift <= tol, one more assignment if the stop was not strict.

Per-point weights (``fit(X, sample_weight=w)``, scikit-learn 1.7.2's semantics): point i counts as ``w[i] >= 0`` points.  Four
statements change and nothing else does -- the first seed is drawn from ``w / w.sum()``; k-means++ sums ``w * closest`` (the
potential, the running sum the thresholds search, a candidate's potential) while ``closest`` itself stays the unweighted
distance; the Lloyd sums are ``sum w x`` over ``sum w``, the inertia is ``sum w d^2`` and a cluster is empty when its weight
is 0 (assignment, labels and the changed-label count do not see the weights); an empty cluster takes the point farthest from
its own centre by the UNWEIGHTED distance, and that point carries ``w x`` and ``w`` along.  The mean that centres X and the
variance that scales ``tol`` stay unweighted, and the weights are not rescaled.  The weighted seeding and Lloyd loop run in the
``_w`` kernels of ``csrc/kmeans_kernels.hip`` under the context's source weights.  Zero weights together with an empty cluster reach two more
statements of scikit-learn's, followed here too: a cluster whose weight is still 0 after relocation (it was given a point of
weight 0) takes the row of the heaviest cluster as the in-order sweep of ``_average_centers`` finds it (averaged if that
cluster comes earlier in the table, the raw sum if later), and nothing is relocated when the largest distance is 0.  Sharded (communicator) weighted fits are not supported.

Arithmetic is float64 whatever the input dtype (scikit-learn keeps float32 input in float32).
With an RCCL communicator attached to the context, X is this rank's shard of one joint clustering:
mean, variance, per-cluster sums, inertia and the changed-label count are all-reduced, the seeds
are drawn on rank 0's shard; empty-cluster relocation stays local to each shard (single-GPU exact).
"""
from __future__ import annotations

import numpy as np

from ._native import Context, default_context


def _random_state(seed):
    if isinstance(seed, np.random.RandomState):
        return seed
    if seed is None:
        return np.random.mtrand._rand
    return np.random.RandomState(seed)


def relocate_empty_sharded(allreduce, rank, labels, dist, Xc, sums, counts):
    """Empty-cluster relocation when the cloud is sharded over ranks: the globally farthest points
    are found with one max-reduction per empty cluster (ties go to the lowest rank), the chosen point
    travels as a sum with zeros elsewhere.  Every rank ends with identical sums / counts.
    ``allreduce(values, op)`` is the communicator's reduction ("sum" / "max")."""
    empty = np.where(counts == 0)[0]
    if len(empty) == 0:
        return
    order = np.argsort(-dist, kind="stable")[:len(empty)]      # local candidates, farthest first
    used = 0
    for new_id in empty:
        d_loc = float(dist[order[used]]) if used < len(order) else -1.0
        d_max = allreduce([d_loc], "max")[0]
        mine = d_loc == d_max
        owner = -allreduce([-float(rank) if mine else -1.0e9], "max")[0]
        payload = np.zeros(4)
        if mine and owner == rank:
            i = order[used]
            used += 1
            payload[:3] = Xc[i]
            payload[3] = labels[i]
        payload = allreduce(payload, "sum")
        old_id = int(round(payload[3]))
        sums[old_id] -= payload[:3]
        sums[new_id] = payload[:3]
        counts[new_id] = 1.0
        counts[old_id] -= 1.0


_cdf_cache = {}


def _uniform_cdf(n):
    """The normalised running sum ``RandomState.choice(n, p=ones/n)`` searches (kept for the last cloud size: frames
    of a stream usually repeat it, and the four passes over n doubles cost as much as 25 Lloyd iterations at 1e5)."""
    if n not in _cdf_cache:
        _cdf_cache.clear()
        w = np.ones(n)
        cdf = (w / w.sum()).cumsum()
        cdf /= cdf[-1]
        _cdf_cache[n] = cdf
    return _cdf_cache[n]


def _weight_cdf(w):
    """The normalised running sum ``RandomState.choice(n, p=w / w.sum())`` searches."""
    cdf = (w / w.sum()).cumsum()
    cdf /= cdf[-1]
    return cdf


def _resolve_weights(X, sample_weight):
    """(points float64 [N,3], weights float64 [N] or None) of ``fit``'s arguments; every refusal that needs no device."""
    if sample_weight is None:
        return np.asarray(X.points if hasattr(X, "points") else X, dtype=np.float64), None
    if isinstance(sample_weight, str):
        if sample_weight != "own":
            raise ValueError("sample_weight must be None, an array [N] or 'own', got %r" % (sample_weight,))
        if hasattr(X, "points") and getattr(X, "weights", None) is not None:
            X, w = X.points, X.weights
        elif hasattr(X, "result") and hasattr(X, "get"):          # a VoxelCloud: centroids and counts, downloaded here
            X, w = X.get()
        else:
            raise ValueError("sample_weight='own' needs an X that brings weights (a WeightedPoints with weights or a "
                             "VoxelCloud), got %s" % type(X).__name__)
    else:
        X, w = (X.points if hasattr(X, "points") else X), sample_weight
    X = np.asarray(X, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 1 or len(w) != len(X):
        raise ValueError("sample_weight must be [N] = [%d], got %s" % (len(X), w.shape))
    bad = np.flatnonzero(~(np.isfinite(w) & (w >= 0)))
    if len(bad):
        raise ValueError("sample_weight[%d] = %r: the weights must be finite and >= 0" % (bad[0], float(w[bad[0]])))
    if not w.sum() > 0:
        raise ValueError("sample_weight: all %d weights are zero" % len(w))
    return X, w


def column_mean_var(X):
    """``X.mean(axis=0)``, ``np.var(X, axis=0)`` and ``X - mean`` of an [N,3] float64 array, bit for bit, at memory
    speed: NumPy reduces a C-ordered [N,3] array over axis 0 row by row (a plain running sum per column, 3 elements
    per inner loop -- 25 ms per million points for the variance alone); the library's host helper
    ``hgmm_kmeans_center_f64`` runs the same three add chains in ~3 ms.  (tests/test_kmeans_cpu.py holds the
    equality.)"""
    import ctypes as C
    from ._native import load_library
    Xd = np.ascontiguousarray(X, dtype=np.float64)
    mean, var, Xc = np.empty(3), np.empty(3), np.empty_like(Xd)
    rc = load_library().hgmm_kmeans_center_f64(Xd.ctypes.data_as(C.c_void_p), len(Xd), mean.ctypes.data_as(C.c_void_p),
                                               var.ctypes.data_as(C.c_void_p), Xc.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError("hgmm_kmeans_center_f64 failed (%d) on an array of shape %s" % (rc, X.shape))
    return mean, var, Xc


class KMeans:
    def __init__(self, n_clusters=8, random_state=None, max_iter=300, n_init=1, tol=1e-4,
                 init="k-means++", ctx: Context | None = None):
        if n_init != 1:
            raise ValueError("only n_init=1 (what the reference uses) is supported")
        if isinstance(init, str) and init != "k-means++":
            raise ValueError("init must be 'k-means++' or an array of centres")
        self.init = init
        self.n_clusters = int(n_clusters)
        self.random_state = random_state
        self.max_iter = int(max_iter)
        self.n_init = 1
        self.tol = float(tol)
        self._ctx = ctx

    # -- seeding -------------------------------------------------------------------------
    def _seed(self, ctx, n, rs, w=None):
        k = self.n_clusters
        trials = 2 + int(np.log(k))
        # == rs.choice(n, p=w / w.sum()) with w = 1 (the draw scikit-learn makes), without choice()'s
        # validation passes over p: one uniform against the normalised running sum of p
        cdf = _uniform_cdf(n) if w is None else _weight_cdf(w)
        first = int(cdf.searchsorted(rs.random_sample(), side='right'))
        rand = rs.uniform(size=(max(k - 1, 0), trials))       # == k-1 successive draws of `trials`
        import time
        t0 = time.perf_counter()
        ids, centres = ctx.kmeans_plusplus(k, first, rand) if w is None else ctx.kmeans_plusplus(k, first, rand, weighted=True)
        self.seeding_ms_ = (time.perf_counter() - t0) * 1e3     # device k-means++ incl. the transfer of the draws
        return ids, centres

    # -- scikit-learn's _relocate_empty_clusters_dense ---------------------------------------
    @staticmethod
    def _relocate_empty(ctx, Xc, sums, counts, w=None):
        empty = np.where(counts == 0)[0]
        if len(empty) == 0:
            return
        labels, dist = ctx.kmeans_labels(with_distances=True)
        if w is not None:
            # weighted: the farthest points by the UNWEIGHTED distance, in the same order; the point carries w x and w
            far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
            if dist.max() == 0:
                return
            for new_id, far_idx in zip(empty, far):
                old_id = labels[far_idx]
                sums[old_id] -= Xc[far_idx] * w[far_idx]
                sums[new_id] = Xc[far_idx] * w[far_idx]
                counts[new_id] = w[far_idx]
                counts[old_id] -= w[far_idx]
            return
        if getattr(ctx, "nranks", 1) > 1:
            relocate_empty_sharded(lambda v, op: ctx.allreduce(v, op=op), ctx.rank, labels, dist, Xc, sums, counts)
            return
        far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
        for new_id, far_idx in zip(empty, far):
            old_id = labels[far_idx]
            sums[old_id] -= Xc[far_idx]
            sums[new_id] = Xc[far_idx]
            counts[new_id] = 1.0
            counts[old_id] -= 1.0

    def fit(self, X, sample_weight=None):
        """``sample_weight``: None -- the unweighted fit (a ``WeightedPoints`` is read for its points only); an array [N] >= 0
        -- point i counts as that many points (module docstring); ``"own"`` -- the weights X brings (a ``WeightedPoints``, or
        a ``VoxelCloud``, whose centroids and counts are downloaded here)."""
        X, w = _resolve_weights(X, sample_weight)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError("expected an [N,3] array, got %s" % (X.shape,))
        n, k = len(X), self.n_clusters
        if n < k:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
        ctx = self._ctx or default_context()
        ranks = getattr(ctx, "nranks", 1)
        if w is not None:
            return self._fit_weighted(ctx, X, w)
        if ranks > 1:
            # X is this rank's shard of one joint clustering: global mean / variance / count
            tot = ctx.allreduce(np.concatenate([[float(n)], X.sum(axis=0), (X * X).sum(axis=0)]))
            mean = tot[1:4] / tot[0]
            var = tot[4:7] / tot[0] - mean * mean
            Xc = X - mean
        else:
            mean, var, Xc = column_mean_var(X)
        tol_abs = 0.0 if self.tol == 0 else float(np.mean(var) * self.tol)
        ctx.set_points(Xc)                            # (the context's own cloud; DevicePoints handles stay valid)
        if isinstance(self.init, str):
            rs = _random_state(self.random_state)
            self.init_indices_, centres = self._seed(ctx, n, rs)
            if ranks > 1:                             # seeds come from rank 0's shard (sum = broadcast)
                centres = ctx.allreduce(centres if ctx.rank == 0 else np.zeros_like(centres))
        else:
            centres = np.array(self.init, dtype=np.float64).reshape(k, 3) - mean
            self.init_indices_ = None

        return self._lloyd_from(ctx, Xc, mean, tol_abs, centres, ranks)

    def _lloyd_from(self, ctx, Xc, mean, tol_abs, centres, ranks=1):
        """The rest of :meth:`fit` from the (centred) start ``centres`` on the resident cloud ``Xc``: Lloyd loop, the last
        assignment, the attributes.  (:meth:`fit_batch` hands a member that met an empty cluster over to it, from its seeds.)"""
        strict = False
        n_iter = 0
        inertia = 0.0
        first = True
        while n_iter < self.max_iter:
            pending = None
            if ranks == 1 and not getattr(ctx, "comm_attached", False):
                # the loop runs on the device until a stop rule fires or a cluster comes up empty (the library's loop is for a
                # context without a communicator; one attached, even of one rank, takes the step-by-step path below)
                centres, done_it, strict, pending = ctx.kmeans_lloyd(centres, self.max_iter - n_iter, tol_abs,
                                                                     reset_labels=first)
                n_iter += done_it
                first = False
                if pending is None:
                    break
                sums, counts, changed = pending
            else:
                sums, counts, inertia, changed = ctx.kmeans_step(centres, reset_labels=first)
                first = False
            # one iteration finished on the host (always under a communicator; after an empty cluster otherwise)
            self._relocate_empty(ctx, Xc, sums, counts)
            new = sums
            pos = counts > 0
            new[pos] *= (1.0 / counts[pos])[:, None]
            shift_tot = float((np.sqrt(((new - centres) ** 2).sum(axis=1)) ** 2).sum())
            centres = new
            n_iter += 1
            if changed == 0:
                strict = True
                break
            if shift_tot <= tol_abs:
                break
        if not strict:
            _, _, inertia, _ = ctx.kmeans_step(centres)
        self.labels_ = ctx.kmeans_labels()
        if strict:
            # labels are those of the last assignment; inertia is measured against the final centres
            inertia = float(((Xc - centres[self.labels_]) ** 2).sum())
            if ranks > 1:
                inertia = float(ctx.allreduce([inertia])[0])
        self.inertia_ = float(inertia)
        self.n_iter_ = n_iter
        self.cluster_centers_ = centres + mean
        return self

    def fit_batch(self, Xs, sample_weight=None):
        """One fit per cloud of ``Xs`` through ONE launch set (``Context.kmeans_fit_batch``: every seeding and Lloyd launch
        serves all clouds) -> a list of fitted estimators of this one's settings, each in the state ``.fit(X_b)`` leaves one
        in, bit for bit: ``cluster_centers_``, ``labels_``, ``inertia_``, ``n_iter_``, ``init_indices_`` (this estimator itself
        stays as it is).  The random stream is consumed cloud by cloud in order, as a loop of ``fit`` consumes it: an int seed
        gives every cloud a fresh ``RandomState(seed)``, a shared ``RandomState`` is drawn from in the loop's order.  ``init``
        may be a list of one array of centres per cloud.  A cloud whose iteration meets an empty cluster leaves the batch and
        is finished by the serial path from its seeds (the relocation stays on the host).  Unweighted only: ``sample_weight``
        is refused, and so is a context with a communicator."""
        if sample_weight is not None:
            raise ValueError("KMeans.fit_batch: the batched initialiser is unweighted (sample_weight / weighted_init are not "
                             "supported); fit weighted clouds one by one with fit(X, sample_weight=)")
        Xs = [np.asarray(X.points if hasattr(X, "points") else X, dtype=np.float64) for X in Xs]
        k, B = self.n_clusters, len(Xs)
        inits = None
        if not isinstance(self.init, str):
            inits = list(self.init)
            if len(inits) != B:
                raise ValueError("KMeans.fit_batch: %d clouds, but init has %d entries (one array of centres per cloud)"
                                 % (B, len(inits)))
        for b, X in enumerate(Xs):
            if X.ndim != 2 or X.shape[1] != 3:
                raise ValueError("KMeans.fit_batch: cloud %d: expected an [N,3] array, got %s" % (b, X.shape))
            if len(X) < k:
                raise ValueError("KMeans.fit_batch: cloud %d: n_samples=%d should be >= n_clusters=%d." % (b, len(X), k))
        if B == 0:
            return []
        ctx = self._ctx or default_context()
        if getattr(ctx, "nranks", 1) > 1 or getattr(ctx, "comm_attached", False):
            raise ValueError("KMeans.fit_batch: the context has a communicator; the batched initialiser is single-rank")
        means, tols, Xcs = [], [], []
        for X in Xs:
            mean, var, Xc = column_mean_var(X)
            means.append(mean)
            tols.append(0.0 if self.tol == 0 else float(np.mean(var) * self.tol))
            Xcs.append(Xc)
        first_ids = rand = start = None
        if inits is None:
            trials = 2 + int(np.log(k))
            first_ids, rand = np.empty(B, np.int64), np.empty((B, max(k - 1, 0), trials))
            for b, Xc in enumerate(Xcs):                        # (the draws of a loop of fit, in its order)
                rs = _random_state(self.random_state)
                first_ids[b] = int(_uniform_cdf(len(Xc)).searchsorted(rs.random_sample(), side='right'))
                rand[b] = rs.uniform(size=(max(k - 1, 0), trials))
        else:
            start = np.stack([np.array(c, dtype=np.float64).reshape(k, 3) - m for c, m in zip(inits, means)])
        ctx.set_points_batch(Xcs)
        res = ctx.kmeans_fit_batch([len(X) for X in Xcs], k, self.max_iter, tols, first_ids=first_ids, rand_vals=rand,
                                   init_centres=start)
        fitted = []
        for b, Xc in enumerate(Xcs):
            est = KMeans(k, self.random_state, self.max_iter, 1, self.tol, self.init if inits is None else inits[b], self._ctx)
            est.init_indices_ = res["ids"][b].copy() if inits is None else None
            if res["status"][b]:
                # an empty cluster: the serial path from the member's own start (its seeds, as the device chose them)
                ctx.set_points(Xc)
                est._lloyd_from(ctx, Xc, means[b], tols[b], res["seeds"][b].copy())
            else:
                centres = res["centres"][b].copy()
                est.labels_ = res["labels"][b].copy()
                if res["strict"][b]:
                    est.inertia_ = float(((Xc - centres[est.labels_]) ** 2).sum())
                else:
                    est.inertia_ = float(res["inertia"][b])
                est.n_iter_ = int(res["n_iter"][b])
                est.cluster_centers_ = centres + means[b]
            fitted.append(est)
        return fitted

    def _fit_weighted(self, ctx, X, w):
        """``fit`` under per-point weights: the loop of the unweighted fit on the weighted entries (single context)."""
        from ._native import HgmmError
        n, k = len(X), self.n_clusters
        if getattr(ctx, "nranks", 1) > 1 or getattr(ctx, "comm_attached", False):
            raise ValueError("KMeans.fit(sample_weight=): the context has a communicator; sharded weighted fits are not "
                             "supported")
        mean, var, Xc = column_mean_var(X)                    # (unweighted, as scikit-learn's X.mean / np.var are)
        tol_abs = 0.0 if self.tol == 0 else float(np.mean(var) * self.tol)
        ctx.set_points(Xc)
        try:
            ctx.tree_set_source_weights(w)
        except HgmmError as e:                                # (a refusal _resolve_weights did not foresee)
            raise ValueError(str(e)) from None
        if isinstance(self.init, str):
            self.init_indices_, centres = self._seed(ctx, n, _random_state(self.random_state), w)
        else:
            centres = np.array(self.init, dtype=np.float64).reshape(k, 3) - mean
            self.init_indices_ = None
        strict = False
        n_iter = 0
        inertia = 0.0
        first = True
        while n_iter < self.max_iter:
            centres, done_it, strict, pending = ctx.kmeans_lloyd(centres, self.max_iter - n_iter, tol_abs,
                                                                 reset_labels=first, weighted=True)
            n_iter += done_it
            first = False
            if pending is None:
                break
            # the iteration that met a cluster of weight 0, finished on the host
            sums, wsum, changed = pending
            self._relocate_empty(ctx, Xc, sums, wsum, w)
            # scikit-learn's _average_centers, in table order: a cluster still of weight 0 copies the heaviest cluster's
            # row as it stands (averaged if that cluster comes earlier, the raw sum if later)
            new = sums
            heaviest = int(np.argmax(wsum))
            for j in range(k):
                if wsum[j] > 0:
                    new[j] *= 1.0 / wsum[j]
                else:
                    new[j] = new[heaviest]
            shift_tot = float((np.sqrt(((new - centres) ** 2).sum(axis=1)) ** 2).sum())
            centres = new
            n_iter += 1
            if changed == 0:
                strict = True
                break
            if shift_tot <= tol_abs:
                break
        if not strict:
            _, _, inertia, _ = ctx.kmeans_step(centres, weighted=True)
        self.labels_ = ctx.kmeans_labels()
        if strict:
            inertia = float((w * ((Xc - centres[self.labels_]) ** 2).sum(axis=1)).sum())
        self.inertia_ = float(inertia)
        self.n_iter_ = n_iter
        self.cluster_centers_ = centres + mean
        return self

    def fit_predict(self, X, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight).labels_


def kmeans_centres(X, k, random_state=1, max_iter=50, ctx: Context | None = None, sample_weight=None):
    """``KMeans(n_clusters=k, random_state=1, max_iter=50, n_init=1).fit(X).cluster_centers_``
    (gmmreg_gpu/gmm_impl.py:20-21) on the device; ``sample_weight`` as in :meth:`KMeans.fit`."""
    return KMeans(n_clusters=k, random_state=random_state, max_iter=max_iter, n_init=1,
                  ctx=ctx).fit(X, sample_weight=sample_weight).cluster_centers_


def kmeans_centres_batch(Xs, k, random_state=1, max_iter=50, ctx: Context | None = None):
    """:func:`kmeans_centres` of every cloud of ``Xs`` through one launch set (:meth:`KMeans.fit_batch`) -> a list of
    ``cluster_centers_``, member b's bit for bit what ``kmeans_centres(Xs[b], k, ...)`` returns."""
    fits = KMeans(n_clusters=k, random_state=random_state, max_iter=max_iter, n_init=1, ctx=ctx).fit_batch(Xs)
    return [f.cluster_centers_ for f in fits]
