"""Host side of the flat GMM EM path, shared by the two reference flavours.

``gmm_waymo/gmm_impl.py`` (variant "W": diag + spherical) and ``gmmreg_gpu/gmm_impl.py``
(variant "G": diag only) are thin, signature-compatible shells over these functions.
All arithmetic on points happens in the HIP kernels (csrc/flat_kernels.hip) through the
C ABI; this module only marshals small parameter arrays.
"""
from __future__ import annotations

import contextlib
import time

import numpy as np

from ._native import Context, DeviceArray, default_context


class DevicePoints:
    """A point cloud resident in HBM on one context (what ``cupy.asarray(X)`` was to the reference,
    gmm_waymo/src/gmm.py:73).  Pass it wherever the API takes ``X``.  Any number of them may be alive on a context
    (hgmm_points_*: each owns its device copy; using one binds it -- a pointer swap, nothing is uploaded again)."""

    def __init__(self, X, ctx: Context | None = None, weights=None):
        """``weights`` [N] >= 0 (default None): per-point weights of the flat fit (``Context.flat_set_weights``) that travel
        with the cloud -- every use of it sets them, an explicit ``sample_weight=`` of the call takes precedence."""
        self.ctx = ctx or default_context()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError("points must have shape [N,3], got %s" % (X.shape,))
        self.weights = _check_weights(weights, X.shape[0])
        self.shape = X.shape
        self.dtype = np.dtype(np.float32)
        self._h = self.ctx.points_create(X)

    def __len__(self):
        return self.shape[0]

    def get(self):
        """The cloud back on the host, float32 [N,3] (``cupy.asnumpy``)."""
        if self._h is None:
            raise RuntimeError("this DevicePoints has been freed")
        return self.ctx.points_download(self._h)

    def bind(self):
        if self._h is None:
            raise RuntimeError("this DevicePoints has been freed")
        self.ctx.points_bind(self._h)
        # (a handle owns no weights on the device: another cloud may have been bound in between, so they are set again)
        self.ctx.flat_set_weights(self.weights)
        return self.ctx

    def free(self):
        if self._h is not None:
            h, self._h = self._h, None
            self.ctx.points_destroy(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def asarray(X, ctx: Context | None = None, weights=None):
    """``weights``: as in :class:`DevicePoints`; a cloud that is resident already keeps the weights it has unless new ones
    are given."""
    if isinstance(X, DevicePoints):
        if weights is not None:
            X.weights = _check_weights(weights, X.shape[0])
        return X
    return DevicePoints(X, ctx, weights)


def _check_weights(s, n):
    """``s`` as the float32 [n] array the library takes, or None.  What the library would refuse (hgmm_flat_set_weights) is
    refused here first, before anything is uploaded: a wrong shape, a NaN, infinite or negative weight, all-zero weights."""
    if s is None:
        return None
    s = np.ascontiguousarray(s, dtype=np.float32)
    if s.ndim != 1 or s.shape[0] != n:
        raise ValueError("sample_weight must have shape [%d], got %s" % (n, s.shape))
    bad = np.flatnonzero(~(np.isfinite(s) & (s >= 0)))
    if bad.size:
        raise ValueError("sample_weight[%d] is %g (weights must be finite and >= 0)" % (bad[0], s[bad[0]]))
    if not (s > 0).any():
        raise ValueError("sample_weight: all %d weights are zero" % n)
    return s


def _ctx_for(X, sample_weight=None) -> Context:
    """Returns the context holding X as its bound cloud: resident clouds are bound (nothing moves), host arrays are
    uploaded into the context's own cloud (like handing NumPy to the reference: a copy per call).  The per-point weights
    in force afterwards are ``sample_weight``, else the resident cloud's own, else none."""
    if isinstance(X, DevicePoints):
        ctx = X.bind()
        if sample_weight is not None:
            ctx.flat_set_weights(_check_weights(sample_weight, X.shape[0]))
        return ctx
    ctx = default_context()
    sample_weight = _check_weights(sample_weight, np.shape(X)[0])
    ctx.set_points(X)
    if sample_weight is not None:
        ctx.flat_set_weights(sample_weight)
    return ctx


def _host(a):
    return np.asarray(a.get() if isinstance(a, DeviceArray) else a)


def _param(a):
    """A parameter array as the E-step takes it: DeviceArrays stay where they are, anything else becomes NumPy."""
    return a if isinstance(a, DeviceArray) else np.asarray(a)


@contextlib.contextmanager
def timer(message, ctx=None):
    """gmm_impl.timer: synchronise, time, print (gmm_waymo/src/gmm_impl.py:43-50).  ``ctx``: the context whose stream
    is waited for (default: the process-wide one, like the reference's null stream)."""
    ctx = ctx or default_context()
    ctx.synchronize()
    start = time.time()
    yield
    ctx.synchronize()
    print('%s:  %f sec' % (message, time.time() - start))


def estimate_log_prob(X, inv_cov, means, cov_type):
    ctx = _ctx_for(X)
    return ctx.flat_log_prob(_host(inv_cov), _host(means), cov_type)


def e_step(X, inv_cov, means, weights, cov_type, variant, sample_weight=None):
    """``sample_weight`` [N] >= 0: the returned mean is ``sum(s * lpn) / sum(s)``; log_resp does not see the weights."""
    ctx = _ctx_for(X, sample_weight)
    # like the reference under CuPy nothing waits here: the mean is a device scalar, read when it is looked at
    # Parameters handed over as DeviceArrays (an earlier m_step's results, arithmetic on them) are used where they are.
    mean_lpn, log_resp, _, _ = ctx.flat_estep(_param(inv_cov), _param(means), _param(weights), cov_type, variant,
                                              lazy_mean=True)
    return mean_lpn, log_resp


def m_step(X, resp, cov_type, variant, centre_hint=None, sample_weight=None):
    """``sample_weight`` [N] >= 0: row i of ``resp`` counts ``sample_weight[i]`` times, the weights are ``nk / sum(s)``.
    Array module in = array module out, like the reference (``xp = cupy.get_array_module(X)``, gmm_impl.py:91):
    responsibilities that live in HBM (a DeviceArray, e.g. ``log_resp.exp()`` of this module's e_step) give
    DeviceArrays -- nothing is downloaded, nothing waits; host responsibilities give NumPy arrays."""
    ctx = _ctx_for(X, sample_weight)
    return ctx.flat_mstep(resp, cov_type, variant, centre_hint, device_out=isinstance(resp, DeviceArray))


def train_gmm(X, max_iter, tol, means, covariances, weights, cov_type, variant, sample_weight=None):
    """``sample_weight`` [N] >= 0 (default: the weights a ``DevicePoints`` brings, else none): point i counts as that many
    points in the M-step and in the log-likelihood behind the stop rule; a zero removes the row (hgmm_flat_set_weights)."""
    ctx = _ctx_for(X, sample_weight)
    inv, mu, w, cov, lls, converged = ctx.flat_train(max_iter, tol, _host(means), _host(covariances),
                                                     _host(weights), cov_type, variant)
    if not converged:
        print('Failed to converge. Increase max-iter or tol.')
    return inv, mu, w, cov, [np.float32(v) for v in lls]


BATCH_MAX_J = 1024        # hgmm_flat_train_batch: only the one-pass fused path is batched


def _batch_member_points(X, b):
    """Member b's cloud without its weights -- or the refusal: the batched fit takes no per-point weights (a handle owns
    none), and weights were silently dropped once in this project."""
    weights = getattr(X, "weights", None)
    if weights is not None:
        raise ValueError("train_gmm_batch: member %d brings per-point weights, which the batched fit does not take: fit it "
                         "with train_gmm(..., sample_weight=)" % b)
    if hasattr(X, "points") and hasattr(X, "weights") and not isinstance(X, DevicePoints):
        return X.points                                          # (a WeightedPoints whose weights are None)
    return X


def _is_voxel_cloud(X):
    from ._native import VoxelCloud
    return isinstance(X, VoxelCloud)


def _batch_member_weighted(X):
    """(points, own weights or None) of a member of a weighted batch: a ``DevicePoints`` stays what it is, a
    ``WeightedPoints(points, weights)`` -- any object with those two fields -- is taken apart."""
    if isinstance(X, DevicePoints):
        return X, X.weights
    if hasattr(X, "points") and hasattr(X, "weights"):
        return X.points, X.weights
    return X, None


def _batch_sample_weights(Xs, sample_weight):
    """``sample_weight`` of train_gmm_batch resolved per member -> (clouds without their weights, [B] arrays or None).
    ``"own"``: each member's own weights, none where it brings none; a sequence: per member, None means its own."""
    B = len(Xs)
    if isinstance(sample_weight, str):
        if sample_weight != "own":
            raise ValueError("train_gmm_batch: sample_weight must be None, 'own' or a sequence, not %r" % (sample_weight,))
        sample_weight = [None] * B
    else:
        sample_weight = list(sample_weight)
        if len(sample_weight) != B:
            raise ValueError("train_gmm_batch: %d clouds, but %d entries in sample_weight" % (B, len(sample_weight)))
    clouds, out = [], []
    for b, X in enumerate(Xs):
        X, own = _batch_member_weighted(X)
        s = own if sample_weight[b] is None else sample_weight[b]
        try:
            n = X.shape[0] if isinstance(X, DevicePoints) else np.shape(X)[0]
            out.append(_check_weights(s, n))
        except (ValueError, IndexError) as e:
            raise ValueError("train_gmm_batch: member %d: %s" % (b, e)) from None
        clouds.append(X)
    return clouds, out


def _report(fits):
    out = []
    for inv, mu, w, cov, lls, converged in fits:
        if not converged:
            print('Failed to converge. Increase max-iter or tol.')
        out.append((inv, mu, w, cov, [np.float32(v) for v in lls]))
    return out


def _train_gmm_batch_voxels(vcs, max_iter, tol, means, covariances, weights, cov_type, variant, sample_weight):
    """train_gmm_batch over ``VoxelCloud`` s: count-weighted, as they are wherever they go, and without a host trip."""
    B = len(vcs)
    if sample_weight is not None and not isinstance(sample_weight, str):
        sample_weight = list(sample_weight)
        if len(sample_weight) != B:
            raise ValueError("train_gmm_batch: %d clouds, but %d entries in sample_weight" % (B, len(sample_weight)))
        for b, s in enumerate(sample_weight):
            if s is not None:
                raise ValueError("train_gmm_batch: member %d is a VoxelCloud, whose weights are its counts: it takes no "
                                 "explicit sample_weight" % b)
    elif isinstance(sample_weight, str) and sample_weight != "own":
        raise ValueError("train_gmm_batch: sample_weight must be None, 'own' or a sequence, not %r" % (sample_weight,))
    ctx = vcs[0].ctx
    for b, vc in enumerate(vcs):
        if vc.ctx is not ctx:
            raise ValueError("train_gmm_batch: member %d is a cloud of another context" % b)
    if np.shape(means[0])[0] > BATCH_MAX_J:
        fits = []
        for b, vc in enumerate(vcs):
            ctx.set_points_from_voxels(vc, tree_weights=False, flat_weights=True)
            fits.append(ctx.flat_train(max_iter, tol, means[b], covariances[b], weights[b], cov_type, variant))
        return _report(fits)
    return _report(ctx.flat_train_batch_voxels(vcs, max_iter, tol, means, covariances, weights, cov_type, variant,
                                               weighted=True))


def train_gmm_batch(Xs, max_iter, tol, means, covariances, weights, cov_type, variant, sample_weight=None):
    """B independent ``train_gmm`` calls through one launch set (``Context.flat_train_batch``) -> a list of ``train_gmm``'s
    tuples, member b's bit for bit what ``train_gmm(Xs[b], ...)`` returns.  ``Xs``: host arrays [N,3] (each uploaded into a
    temporary ``DevicePoints`` and freed afterwards) and / or ``DevicePoints`` of one context (used where they are; one may
    occur several times: restarts of one resident cloud).  ``means``, ``covariances``, ``weights``: one per member, all of
    the same J.  J > 1024, which the batched entry does not take, falls back to a loop of ``train_gmm``.

    ``sample_weight``: None -- no per-point weights, and a member that brings some is refused (ValueError naming it);
    ``"own"`` -- each member's own (``DevicePoints.weights``, ``WeightedPoints.weights``), none where it brings none; a
    sequence of B entries -- an array [n_b] per member, None meaning the member's own.  Member b is then bit for bit
    ``train_gmm(Xs[b], ..., sample_weight=)`` with those weights.

    A list made only of ``VoxelCloud`` s (one live voxel result) is fitted count-weighted without leaving the device
    (``Context.flat_train_batch_voxels``), whatever ``sample_weight`` says short of an explicit array, which is a
    ValueError; so is a list that mixes ``VoxelCloud`` s with other members."""
    Xs = list(Xs)
    B = len(Xs)
    n_vox = sum(1 for X in Xs if _is_voxel_cloud(X))
    if 0 < n_vox < B:
        raise ValueError("train_gmm_batch: VoxelClouds and other members in one batch (%d of %d are VoxelClouds): fit them "
                         "in two calls" % (n_vox, B))
    slot_weights = None
    if n_vox == 0:
        if sample_weight is None:
            Xs = [_batch_member_points(X, b) for b, X in enumerate(Xs)]
        else:
            Xs, slot_weights = _batch_sample_weights(Xs, sample_weight)
    for name, seq in (("means", means), ("covariances", covariances), ("weights", weights)):
        if len(seq) != B:
            raise ValueError("train_gmm_batch: %d clouds, but %d arrays in %s" % (B, len(seq), name))
    if B == 0:
        return []
    means, covariances, weights = [_host(m) for m in means], [_host(c) for c in covariances], [_host(w) for w in weights]
    Js = [np.shape(m)[0] if np.ndim(m) == 2 else -1 for m in means]
    for b, m in enumerate(means):
        if np.ndim(m) != 2 or np.shape(m)[1] != 3:
            raise ValueError("train_gmm_batch: member %d: means must be [J,3], got %s" % (b, np.shape(m)))
        if Js[b] != Js[0]:
            raise ValueError("train_gmm_batch: member %d has J = %d, member 0 has J = %d (the members share J)" % (b, Js[b], Js[0]))
    if n_vox:
        return _train_gmm_batch_voxels(Xs, max_iter, tol, means, covariances, weights, cov_type, variant, sample_weight)
    ctxs = [X.ctx for X in Xs if isinstance(X, DevicePoints)]
    ctx = ctxs[0] if ctxs else default_context()
    for b, X in enumerate(Xs):
        if isinstance(X, DevicePoints) and X.ctx is not ctx:
            raise ValueError("train_gmm_batch: member %d is a cloud of another context" % b)
        if not isinstance(X, DevicePoints) and (np.ndim(X) != 2 or np.shape(X)[1] != 3):
            raise ValueError("train_gmm_batch: member %d: points must have shape [N,3], got %s" % (b, np.shape(X)))
    if Js[0] > BATCH_MAX_J:
        if slot_weights is None:
            return [train_gmm(Xs[b], max_iter, tol, means[b], covariances[b], weights[b], cov_type, variant) for b in range(B)]
        # (a slot without weights is a member that brings none: train_gmm's None finds none either)
        return [train_gmm(Xs[b], max_iter, tol, means[b], covariances[b], weights[b], cov_type, variant,
                          sample_weight=slot_weights[b]) for b in range(B)]
    temporary = []
    try:
        clouds = []
        for X in Xs:
            if not isinstance(X, DevicePoints):
                X = DevicePoints(np.asarray(X), ctx)
                temporary.append(X)
            clouds.append(X)
        if slot_weights is None:
            fits = ctx.flat_train_batch(clouds, max_iter, tol, means, covariances, weights, cov_type, variant)
        else:
            fits = ctx.flat_train_batch(clouds, max_iter, tol, means, covariances, weights, cov_type, variant,
                                        weights=slot_weights)
    finally:
        for X in temporary:
            X.free()
    return _report(fits)


def predict(X, inv_cov, means, weights, cov_type, variant):
    """Array module in = array module out (``xp.argmax``, gmm_impl.py:147-155): a resident cloud gives the labels as a
    DeviceArray (int32 in HBM; nothing is downloaded, nothing waits -- the reference's caller does the
    ``cupy.asnumpy``, run_gmm_static.py:49), a host array gives NumPy int64 like the reference under NumPy."""
    ctx = _ctx_for(X)
    lab = ctx.flat_predict(_param(inv_cov), _param(means), _param(weights), cov_type, variant)
    return lab if isinstance(X, DevicePoints) else lab.get().astype(np.int64)
