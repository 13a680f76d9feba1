"""Drop-in for the reference's ``src/python/hgmm/hgmm_gpu.py`` (and its CPU twin
``hgmm_cupy_cpu_working.py``): ``buildGMMTree``, ``GMMTree``, ``registration_gmmtree``,
``RigidTransformation`` with the same signatures and return values.

What runs where
  * tree construction (E-step, M-step, level log-likelihood, the per-level partition) and the
    registration E-step (tree descent + moment accumulation): HIP kernels, float64
    (csrc/tree_kernels.hip) -- the reference ran the latter as a pure-Python triple loop
    (hgmm_gpu.py:550-577);
  * the rigid update (per-node eigh + 6-dof twist least squares, hgmm_gpu.py:729-752) stays on
    the host in NumPy, as in the reference.

Semantics follow the CPU twin where the two reference files differ (empty-node rule m0 < ld;
the Numba file has it commented out, hgmm_gpu.py:250-256).  Initialisation constants default
to the Numba file's (seed 72, sig2 = 0.004, hgmm_gpu.py:469-477) and can be overridden.
"""
from __future__ import annotations

import contextlib
import itertools
import time
from collections import namedtuple

import numpy as np

from .. import _native
from .._native import CHI2_3_99, CHI2_3_999, Context, VoxelCloud, VoxelResult, default_context  # noqa: F401

eps = np.float32(1.0e-15)     # hgmm_gpu.py:29
n_node = 8                    # hgmm_gpu.py:30


def child2(j):
    return (j + 1) * n_node


def level(l):
    """First node index of level l (hgmm_gpu.py:91-92)."""
    return n_node * (np.power(n_node, l) - 1) / (n_node - 1)


def n_total_nodes(maxTreeLevel):
    return int(n_node * (np.power(n_node, maxTreeLevel) - 1) / (n_node - 1))


def complexity(cov):
    """smallest eigenvalue / trace (hgmm_gpu.py:78-82)."""
    lam = np.linalg.eigvalsh(np.asarray(cov, dtype=np.float64))
    return lam[0] / np.sum(lam)


def _is_voxels(x):
    """A :class:`VoxelCloud`: a member of the voxel result resident on a context (``Context.voxel_down_sample_batch(...,
    download=False)``).  It goes where points go, stays on the device, and its counts are its weights."""
    return isinstance(x, VoxelCloud)


def _points(x):
    """The [N,3] array behind a cloud argument; a :class:`VoxelCloud` is returned as it is (``len()`` and ``dtype`` answer
    for it: it counts as float64 wherever the points' type selects arithmetic)."""
    if _is_voxels(x):
        return x
    return np.asarray(x.points if hasattr(x, "points") else x)


def _gate_arg(maha2_gate):
    """The mirrors' ``maha2_gate`` argument -> None (the mirror leaves the context's gate alone: off unless the caller set one
    on the context) or a float > 0 (``inf``: off for this call).  Anything else is refused here, before the library is touched."""
    if maha2_gate is None:
        return None
    g = float(maha2_gate)
    if not g > 0.0:                                  # (NaN fails the comparison too)
        raise ValueError("maha2_gate must be > 0 (np.inf or None: no gate), got %r" % (maha2_gate,))
    return g


WeightedPoints = namedtuple("WeightedPoints", ["points", "weights"])
WeightedPoints.__doc__ = """A cloud with one weight >= 0 per point: ``WeightedPoints(points [N,3], weights [N])``.  Every
entry that takes a target takes this in its place (any object with ``.points`` and ``.weights`` does) -- the way to hand
weights to :meth:`GMMTree.registration_multistart` and :meth:`GMMTree.score`, whose argument lists are the reference-side
ones; an explicit ``weights=`` / ``target_weights=`` argument, where there is one, takes precedence.

As a SOURCE (``buildGMMTree``, ``GMMTree(source)``, ``set_source``, ``registration_gmmtree`` and the sources of
``registration_gmmtree_batch``) it brings its weights to the tree build: point i counts as ``weights[i]`` points
(``Context.tree_set_source_weights``).  Earlier versions accepted a WeightedPoints source and silently dropped its weights;
pass ``source.points`` to build the unweighted tree.  An explicit ``weights=`` / ``source_weights=`` takes precedence.

:func:`fitFullCovGMM` takes it the same way: the flat full-covariance fit under its weights
(``Context.fullcov_fit(..., weighted=True)``).  Earlier versions unwrapped a WeightedPoints there and silently dropped its
weights; pass ``.points`` for the unweighted fit."""


def _weights_arg(weights, n):
    """The mirrors' ``weights`` argument for a cloud (a target, or a source) of ``n`` points -> None (no weights) or a float64 array [n], every entry
    finite and >= 0 and not all of them zero.  Anything else is refused here, before the library is touched."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] != int(n):
        raise ValueError("weights must be one per point of the cloud: expected shape (%d,), got %s" % (int(n), w.shape))
    bad = np.nonzero(~(np.isfinite(w) & (w >= 0.0)))[0]
    if len(bad):
        raise ValueError("weights must be finite and >= 0: weight %d is %r" % (int(bad[0]), float(w[bad[0]])))
    if not w.sum() > 0.0:
        raise ValueError("weights must not all be zero")
    return w


def _target_weights(target, weights=None):
    """The weights that go with ``target``: the explicit argument, else the target's own ``.weights`` (WeightedPoints), else
    None -- checked against the target's length.  A :class:`VoxelCloud` brings its counts and takes no others."""
    if _is_voxels(target):
        if weights is not None:
            raise ValueError("a VoxelCloud is weighted by its counts: it cannot be combined with explicit weights")
        return None
    if weights is None:
        weights = getattr(target, "weights", None)
    return _weights_arg(weights, len(_points(target)))


def _set_source(ctx, points, weights):
    """Upload ``points`` (float64 [N,3]) as the context's resident cloud, then its weights if it has any (already checked by
    :func:`_weights_arg`).  A new cloud drops the previous one's weights in the library, so a cloud is never built under
    another one's weights.  A :class:`VoxelCloud` is handed over on the device, its counts as the weights."""
    if _is_voxels(points):
        ctx.set_points_from_voxels(points, tree_weights=True)
        return
    ctx.set_points(points)
    if weights is not None:
        ctx.tree_set_source_weights(weights)


def _set_target(ctx, target, weights=None):
    """Upload ``target`` as the context's resident registration target, with its weights if it has any.  A new target drops
    the weights of the previous one in the library, so a target is never registered under another one's weights."""
    w = _target_weights(target, weights)
    if _is_voxels(target):
        ctx.tree_set_target_from_voxels(target, weighted=True)
        return
    ctx.tree_set_target(_points(target))
    if w is not None:
        ctx.tree_set_target_weights(w)


@contextlib.contextmanager
def _reg_gate(ctx, gate):
    """``Context.tree_set_reg_gate(gate)`` for the calls inside, the context's previous gate afterwards (as buildGMMTree does
    with the precision): a shared ``default_context()`` is never left gated.  ``gate`` None: nothing is touched."""
    if gate is None:
        yield
        return
    prev = ctx.tree_get_reg_gate()
    ctx.tree_set_reg_gate(gate)
    try:
        yield
    finally:
        ctx.tree_set_reg_gate(prev)


def buildGMMTree(points, maxTreeLevel, ls, ld, sig2=0.004, seed=72, init_idx=None,
                 max_iters_per_level=1000, ctx: Context | None = None, return_trace=False, dtype=None, pdf_dtype=None,
                 weights=None):
    """-> (mixingCoeff[T], mean[T,3], covar[T,3,3])   (hgmm_gpu.py:466-548).

    ``weights`` [N] >= 0 (no counterpart in the reference; default None: the points' own if they are a
    :class:`WeightedPoints`, else none): point i counts as ``weights[i]`` points -- a voxel centroid with its count
    (``voxel_down_sample(..., return_counts=True)``).  The moments, ``pi`` and the level log-likelihood behind the stop rule
    ``ls`` are weighted; the partition and the 1e-15 floor are not (``Context.tree_set_source_weights``).

    ``init_idx`` (T indices into ``points``) overrides the reference's
    ``np.random.seed(72); randint(nTotal, size=nTotal)`` draw.

    ``dtype``: the reference has this function twice -- float64 in the CPU twin (hgmm_cupy_cpu_working.py:122-160, the
    canonical semantics) and float32 in the GPU file (``points.astype(np.float32)``, float32 node and moment arrays,
    hgmm_gpu.py:472, 478-484).  Default: the points' own type -- float32 points give float32 tables and the float32-pdf
    stop rule (``Context.tree_set_precision``), anything else the float64 path.  ``pdf_dtype`` (default: ``dtype``) sets the
    stop rule's arithmetic alone: :class:`GMMTree` keeps float64 tables for its registration whatever the points' type
    (``dtype=np.float64, pdf_dtype=<the points' type>``).  The context's own precision setting is restored afterwards."""
    ctx = ctx or default_context()
    raw = _points(points)
    weights = _target_weights(points, weights)       # (refused before anything is uploaded)
    dt = np.dtype(dtype) if dtype is not None else (np.dtype(np.float32) if raw.dtype == np.float32 else np.dtype(np.float64))
    pdt = np.dtype(pdf_dtype) if pdf_dtype is not None else dt
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)) or pdt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be float32 or float64")
    # (a VoxelCloud stays on the device: its initial means are gathered there, by row number)
    P = raw if _is_voxels(raw) else np.ascontiguousarray(raw, dtype=np.float64)
    T = n_total_nodes(maxTreeLevel)
    if init_idx is None:
        rs = np.random.RandomState(seed)
        init_idx = rs.randint(T, size=T)
    _set_source(ctx, P, weights)
    init = dict(init_mu=None, init_rows=np.asarray(init_idx)) if _is_voxels(raw) else dict(init_mu=P[np.asarray(init_idx)])
    prev = getattr(ctx, "tree_dtype", np.dtype(np.float64))     # (a precision the caller set on the context survives this call)
    ctx.tree_set_precision(pdt)
    try:
        pi, mu, cov, leaf, iters, q = ctx.tree_build(maxTreeLevel, ls, ld, sig2=sig2, max_iters_per_level=max_iters_per_level,
                                                     want_leaf=bool(return_trace), **init)
    finally:
        ctx.tree_set_precision(prev)
    if dt == np.dtype(np.float32):
        pi, mu, cov = pi.astype(np.float32), mu.astype(np.float32), cov.astype(np.float32)
    if return_trace:
        return pi, mu, cov, {"leaf_idx": leaf, "iters_per_level": iters, "q_trace": q}
    return pi, mu, cov


def gmmTreeEStep(points, mixingCoeff, mean, covar, parentIdx, ctx: Context | None = None):
    """One tree E-step for an arbitrary parent assignment (hgmm_cupy_cpu_working.py:162-191).
    -> (momentsZero[T], momentsOne[T,3], momentsTwo[T,3,3], currentIdx[N])."""
    ctx = ctx or default_context()
    ctx.set_points(np.ascontiguousarray(_points(points), dtype=np.float64))
    return ctx.tree_estep(mixingCoeff, mean, covar, parentIdx)


def gmmTreeMStep(momentsZero, momentsOne, momentsTwo, l, mixingCoeff, mean, covar, n_points, ld,
                 ctx: Context | None = None):
    """ML update of the nodes of level ``l`` (hgmm_cupy_cpu_working.py:193-198 with the m0 < ld
    rule of mlEstimator 109-119).  -> new (mixingCoeff, mean, covar)."""
    ctx = ctx or default_context()
    return ctx.tree_mstep(momentsZero, momentsOne, momentsTwo, int(level(l)), int(level(l + 1)), n_points, ld,
                          mixingCoeff, mean, covar)


def logLikelihoodValue(mixingCoeff, mean, covar, data, j0, j1, ctx: Context | None = None):
    """sum_i log max(sum_{j0 <= j < j1, pi_j >= eps} pi_j N(x_i; j), eps)
    (hgmm_cupy_cpu_working.py:72-85 / the Numba kernel hgmm_gpu.py:107-115 + sum_reduce)."""
    ctx = ctx or default_context()
    ctx.set_points(np.ascontiguousarray(_points(data), dtype=np.float64))
    return ctx.tree_loglik(mixingCoeff, mean, covar, int(j0), int(j1))


def fitFullCovGMM(points, n_components, ls=80.0, ld=1.0e-4, sig2=0.00034, init_idx=None, seed=None,
                  max_iters=1000, ctx: Context | None = None, return_trace=False, dtype=None, weights=None):
    """Flat full-covariance GMM = ONE tree level with branching ``n_components`` (the reference's
    CPU twin run with its module global ``n_node = J`` and ``buildGMMTree(P, 1, ls, ld)``,
    hgmm_cupy_cpu_working.py:30,122-160).  -> (mixingCoeff[J], mean[J,3], covar[J,3,3]).

    ``init_idx``: J indices of the initial means (default: the twin's draw
    ``RandomState(J).randint(J, size=J)`` -- note it only ever picks among the first J points).

    ``dtype=np.float32`` (explicit only; the points' own type does NOT switch it): the float32-tile kernel for this fit
    (``Context.tree_set_precision``; J <= 1024) -- float32 pdfs, tile and matrix-core statistics about the centroid, float64
    row sums / log / M-step; ~25 % faster per iteration at 10^6 x 800, Sigma to ~1e-5 of a variance.  The context's own
    setting is restored afterwards.

    ``weights`` [N] >= 0 (no counterpart in the reference; default None: the points' own if they are a
    :class:`WeightedPoints`, else none): point i counts as ``weights[i]`` points, as in :func:`buildGMMTree` -- the moments,
    ``pi = m0 / sum(weights)`` and the log-likelihood behind the stop rule ``ls`` are weighted; the labels and the 1e-15 floor
    are not (``Context.fullcov_fit(..., weighted=True)``).  A :class:`VoxelCloud` is handed over on the device and fitted
    under its counts; it takes no explicit weights.  A plain array fits as it always did.  Earlier versions accepted a
    WeightedPoints here and silently dropped its weights: pass its ``.points`` for the unweighted fit."""
    ctx = ctx or default_context()
    raw = _points(points)
    weights = _target_weights(points, weights)       # (refused before anything is uploaded)
    # (a VoxelCloud stays on the device: its initial means are read back by row number)
    P = raw if _is_voxels(raw) else np.ascontiguousarray(raw, dtype=np.float64)
    J = int(n_components)
    if init_idx is None:
        init_idx = np.random.RandomState(J if seed is None else seed).randint(J, size=J)
    _set_source(ctx, P, weights)
    weighted = _is_voxels(raw) or weights is not None
    init_mu = ctx.points_rows(np.asarray(init_idx)) if _is_voxels(raw) else P[np.asarray(init_idx)]
    prev = getattr(ctx, "tree_dtype", np.dtype(np.float64))
    if dtype is not None:
        ctx.tree_set_precision(dtype)
    try:
        # (the unweighted call is the one every earlier version made: no weight call, no keyword)
        pi, mu, cov, labels, q = (ctx.fullcov_fit(J, ls, ld, init_mu, sig2, max_iters, weighted=True) if weighted
                                  else ctx.fullcov_fit(J, ls, ld, init_mu, sig2, max_iters))
    finally:
        if dtype is not None:
            ctx.tree_set_precision(prev)
    if return_trace:
        return pi, mu, cov, {"labels": labels, "q_trace": q}
    return pi, mu, cov


def fitFullCovGMM_batch(clouds, n_components, ls=80.0, ld=1.0e-4, sig2=0.00034, init_idx=None, seed=None, max_iters=1000,
                        ctx: Context | None = None, return_trace=False, weights=None):
    """:func:`fitFullCovGMM` of every cloud of ``clouds`` through ONE launch set (``Context.fullcov_fit_batch``): four
    launches per iteration for all of them, every member with its own stop rule.  -> a list of what :func:`fitFullCovGMM`
    returns, member b bit for bit what ``fitFullCovGMM(clouds[b], ...)`` gives.

    ``clouds``: a list of [N_b,3] arrays, :class:`WeightedPoints` (a member brings its own weights) or :class:`VoxelCloud`
    members of one resident voxel result.  A list of VoxelClouds is handed over on the device and fitted count-weighted,
    its initial means gathered there by row number; it takes no explicit weights and cannot be mixed with host arrays.
    ``weights``: a list with one entry per cloud, ``None`` entries allowed (that member is fitted unweighted, bit for bit);
    an entry takes precedence over the member's own.  ``init_idx``: [J] (the same rows for every member) or one [J] per
    member; default: the serial function's draw, per member.  One ``n_components``, ``ls``, ``ld``, ``sig2`` and budget for
    all members; the float32 tile (``dtype=``) has no batched form.

    More than 1024 components (rounded up to a multiple of 16) are beyond the batched kernel: the members are then fitted
    one by one by :func:`fitFullCovGMM` -- the only case that falls back.  Everything else the library refuses is an error."""
    ctx = ctx or default_context()
    clouds = list(clouds)
    B, J = len(clouds), int(n_components)
    if B == 0:
        return []
    if weights is not None and len(weights) != B:
        raise ValueError("%d clouds, but %d weights entries" % (B, len(weights)))
    raws = [_points(x) for x in clouds]
    voxels = [_is_voxels(r) for r in raws]
    if any(voxels) and not all(voxels):
        raise ValueError("VoxelCloud members cannot be mixed with host arrays in one batch")
    ws = [_target_weights(x, None if weights is None else weights[b]) for b, x in enumerate(clouds)]   # (refused before any upload)
    if init_idx is None:
        idx = [np.random.RandomState(J if seed is None else seed).randint(J, size=J) for _ in range(B)]
    else:
        idx = np.asarray(init_idx)
        idx = [idx] * B if idx.ndim == 1 else list(idx)
        if len(idx) != B or any(np.shape(i) != (J,) for i in idx):
            raise ValueError("init_idx must be [%d] or [%d,%d]" % (J, B, J))
    if (J + 15) // 16 * 16 > 1024:
        return [fitFullCovGMM(x, J, ls, ld, sig2, idx[b], None, max_iters, ctx, return_trace, weights=ws[b])
                for b, x in enumerate(clouds)]
    if all(voxels):
        counts = ctx.set_points_batch_from_voxels(raws, weighted=True)
        init, weighted = dict(init_rows=np.stack([np.asarray(i, dtype=np.int64) for i in idx])), True
    else:
        Ps = [np.ascontiguousarray(r, dtype=np.float64) for r in raws]
        weighted = any(w is not None for w in ws)
        Ps = ctx.set_points_batch(Ps, weights=ws if weighted else None)
        counts = [len(P) for P in Ps]
        init = dict(init_mu=np.stack([P[np.asarray(i)] for P, i in zip(Ps, idx)]))
    pi, mu, cov, labels, q = ctx.fullcov_fit_batch(counts, J, ls, ld, sig2=sig2, max_iters=max_iters, weighted=weighted,
                                                   want_labels=bool(return_trace), **init)
    if return_trace:
        return [(pi[b], mu[b], cov[b], {"labels": labels[b], "q_trace": q[b]}) for b in range(B)]
    return [(pi[b], mu[b], cov[b]) for b in range(B)]


def gmmTreeRegESTep(points, mixingCoeff, mean, covar, maxTreeLevel, lc, ctx: Context | None = None):
    """-> (momentsZero[T], momentsOne[T,3], momentsTwo[T,3,3])   (hgmm_gpu.py:550-577)."""
    ctx = ctx or default_context()
    ctx.tree_set_nodes(maxTreeLevel, mixingCoeff, mean, covar)
    ctx.tree_set_target(_points(points))
    return ctx.tree_reg_estep(n_total_nodes(maxTreeLevel), lambda_c=lc)


# RigidTransformation (hgmm_gpu.py:599-618: x -> scale R x + t on row vectors, ``inverse()``) is the same
# object the GMMReg mirror uses
from ..gmmreg_gpu.transforms import Transformation, RigidTransformation  # noqa: E402,F401


def skew(x):
    """[x]_x, the cross-product matrix (hgmm_gpu.py:620-624)."""
    a, b, c = x
    return np.array([[0.0, -c, b], [c, 0.0, -a], [-b, a, 0.0]])


def twist_trans(tw, linear=False):
    """6-twist (omega, v) -> (R, t): exp of omega by Rodrigues' formula, or its first-order form I + [omega]_x with
    ``linear`` (hgmm_gpu.py:646-664).  The translation part is passed through as is."""
    omega, v = np.asarray(tw[:3], dtype=np.float64), tw[3:]
    if linear:
        return np.identity(3) + skew(omega), v
    angle = np.linalg.norm(omega)
    if angle == 0.0:
        return np.identity(3), v
    axis = omega / angle
    k = skew(axis)
    return np.identity(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k), v


def twist_mul(tw, rot, t, linear=False):
    """Compose the twist's motion with (rot, t): (dR rot, dR t + dt)   (hgmm_gpu.py:634-644)."""
    d_rot, d_t = twist_trans(tw, linear=linear)
    return d_rot @ rot, d_rot @ t + d_t


_tp_controller = None


def _small_lapack():
    """The M-step's factorizations are tall-and-skinny (3 n_nodes x 7): a threaded LAPACK spends
    its time synchronising (16 ms on 8 threads vs 0.6 ms on one for 9900 x 7), so they run on one
    thread when threadpoolctl is there to say so.  The controller is built once (inspecting the
    loaded libraries on every call costs more than the factorization)."""
    global _tp_controller
    try:
        if _tp_controller is None:
            from threadpoolctl import ThreadpoolController
            _tp_controller = ThreadpoolController()
        return _tp_controller.limit(limits=1, user_api="blas")
    except Exception:                                   # pragma: no cover - optional dependency
        import contextlib
        return contextlib.nullcontext()


EstepResult = namedtuple('EstepResult', ['momentZero', 'momentOne', 'momentTwo'])
MstepResult = namedtuple('MstepResult', ['transformation', 'q'])
# what registration() returns with return_score=True: MstepResult's two fields, then the TreeScore at the final pose
ScoredResult = namedtuple('ScoredResult', ['transformation', 'q', 'score'])

# Score of a cloud against a tree (Context.tree_score; no counterpart in the reference).  fitness = share of the points
# whose squared Mahalanobis distance to their node is within the inlier bound; inlier_rmse = rms Euclidean distance of the
# inliers to their nodes' means; mahalanobis_rms = rms Mahalanobis distance of the inliers; mean_log_density = mean over the
# inliers of log(pi_s N(y; s)); n_dead = points whose node has pi = 0 or a singular covariance; n_above_leaf = points that
# stopped above the last level; node / maha2 / logp = the per-point arrays, or None where they were not asked for.
TreeScore = namedtuple('TreeScore', ['fitness', 'inlier_rmse', 'mahalanobis_rms', 'mean_log_density', 'n_points',
                                     'n_inliers', 'n_dead', 'n_above_leaf', 'node', 'maha2', 'logp'])


def tree_score_from_summary(summary, arrays=None):
    """The eight sums of ``hgmm_tree_score`` (+ the per-point arrays, a dict or None) -> :class:`TreeScore`.

    With NO inlier there is nothing to average: fitness is 0.0, ``inlier_rmse`` and ``mahalanobis_rms`` are +inf and
    ``mean_log_density`` is -inf ("infinitely far"), so no field is ever NaN through a division by zero and a threshold
    test on any of them rejects such a cloud.  Under per-point weights of the target the sums are weighted: ``n``,
    ``n_inliers`` and the two other counts are then sums of weights (floats unless they happen to be whole numbers)."""
    s = np.asarray(summary, dtype=np.float64).reshape(8)
    arrays = arrays or {}
    count = lambda v: int(v) if v == int(v) else float(v)      # (a sum of weights need not be a whole number)
    n, n_in = count(s[0]), count(s[1])
    if n_in > 0:
        rmse, mrms, mld = float(np.sqrt(s[3] / s[1])), float(np.sqrt(s[2] / s[1])), float(s[4] / s[1])
    else:
        rmse, mrms, mld = float("inf"), float("inf"), float("-inf")
    return TreeScore(float(s[1] / s[0]) if n > 0 else 0.0, rmse, mrms, mld, n, n_in, count(s[5]), count(s[6]),
                     arrays.get("node"), arrays.get("maha2"), arrays.get("logp"))


class MultiStartResult(ScoredResult):
    """What :meth:`GMMTree.registration_multistart` returns for the winner: a :class:`ScoredResult` that also says which start
    won (``best_index_``) and how many iterations its loop took (``n_iter_``)."""
    best_index_ = None
    n_iter_ = None


def best_hypothesis(summaries, rot, t):
    """The winner among K registered hypotheses, deterministic: most inliers (summary[1], an integer), then the smaller sum of
    the inliers' squared Mahalanobis distances (summary[2]), then the lower index.  A hypothesis whose pose (rot[k], t[k]) is
    not finite loses to every finite one.  ``summaries`` [K,8] as :meth:`Context.tree_score_multi` returns them.  -> index."""
    s = np.asarray(summaries, dtype=np.float64).reshape(-1, 8)
    K = len(s)
    if K < 1:
        raise ValueError("best_hypothesis: no hypotheses")
    rot, t = np.asarray(rot, dtype=np.float64).reshape(K, 9), np.asarray(t, dtype=np.float64).reshape(K, 3)
    finite = np.isfinite(rot).all(axis=1) & np.isfinite(t).all(axis=1)

    def key(k):
        if not finite[k]:
            return (1, 0.0, 0.0, k)
        inliers = s[k, 1] if np.isfinite(s[k, 1]) else -1.0
        spread = s[k, 2] if np.isfinite(s[k, 2]) else np.inf
        return (0, -inliers, spread, k)
    return min(range(K), key=key)


def rotation_starts(angles_deg=(-15, 0, 15), centre=None):
    """Start poses for :meth:`GMMTree.registration_multistart`: the rotations Rz(az) Ry(ay) Rx(ax) for (ax, ay, az) in
    ``itertools.product(angles_deg, repeat=3)`` order, each taken about ``centre`` (None: the origin), i.e. t = c - R c.
    -> list of :class:`RigidTransformation`; with the default angles 27 poses, index 13 the identity."""
    c = np.zeros(3) if centre is None else np.asarray(centre, dtype=np.float64).reshape(3)
    out = []
    for ax, ay, az in itertools.product(angles_deg, repeat=3):
        rot = euler_matrix_xyz(*np.deg2rad([float(ax), float(ay), float(az)]))
        out.append(RigidTransformation(rot, c - rot @ c))
    return out


def node_level(node):
    """Tree level (0 = the root's eight children) of node indices: level l holds the nodes 8 (8^l - 1) / 7 .. 8 (8^(l+1) - 1) / 7 - 1."""
    node = np.asarray(node, dtype=np.int64)
    lvl = np.zeros(node.shape, dtype=np.int64)
    first = 8                                    # first node of level 1
    while np.any(node >= first):
        lvl += node >= first
        first = 8 * first + 8
    return lvl if lvl.ndim else int(lvl)


class GMMTree():
    """GMM tree registration (hgmm_gpu.py:669-768).

    Args mirror the reference; ``ls`` / ``ld`` / ``sig2`` / ``init_idx`` expose the constants it
    hard-codes (20, 1e-4, 0.004, seed 72).

    ``maha2_gate`` (no counterpart in the reference; default None: no gate): the Mahalanobis gate of the registration
    E-step (``Context.tree_set_reg_gate``) for this object's registrations -- a (point, node) pair further than this
    squared Mahalanobis distance from the node adds nothing to its moments, which keeps clutter and the non-overlapping
    part of a scan from pulling the nodes.  ``CHI2_3_999`` is a reasonable value.  It is set on the context for the
    object's own calls only; the context's previous gate is restored after each.

    Per-point WEIGHTS of a target (no counterpart in the reference; ``Context.tree_set_target_weights``): a target point
    with weight w adds ``w * gamma`` where it added ``gamma`` -- a voxel centroid with its count
    (``voxel_down_sample(..., return_counts=True)``), a return weighted by range, the caller's own M-estimator weights.
    ``registration(..., weights=)`` takes them as an argument; every method that takes a target (``registration``,
    ``registration_multistart``, ``score``, ``expectation_step``) takes a :class:`WeightedPoints` in its place.  The
    descent, the stop rule and the gate do not see them; the per-point arrays of a score are not weighted, its sums are.

    Per-point WEIGHTS of the source (``source_weights=``, ``set_source(source, weights=)``, or a :class:`WeightedPoints`
    source; ``Context.tree_set_source_weights``): source point i counts as ``w_i`` points in the tree build, see
    :func:`buildGMMTree`."""

    def __init__(self, source=None, tree_level=5, lambda_c=0.01, ls=20, ld=1.0e-4, sig2=0.004,
                 init_idx=None, ctx: Context | None = None, verbose=False, solve_on_device=False, maha2_gate=None,
                 source_weights=None):
        self._maha2_gate = _gate_arg(maha2_gate)
        self._source = None
        self._tree_level = tree_level
        self._lambda_c = lambda_c
        self._ls, self._ld, self._sig2, self._init_idx = ls, ld, sig2, init_idx
        self._tf_type = RigidTransformation
        self._tf_result = self._tf_type()
        self._callbacks = []
        self._ctx_arg = ctx
        self._verbose = verbose
        self._device_mstep = True            # False: every iteration through expectation_step + maximization_step
        # True: the library's loop also solves the 6 x 6 system, composes the twist and applies the stop rule on the device
        # (per-context option reg_device_solve; the host solve is the default and the parity reference)
        self._solve_on_device = bool(solve_on_device)
        self._target_id = None
        if source is not None:
            self.set_source(source, source_weights)
        elif source_weights is not None:
            raise ValueError("source_weights without a source")

    @property
    def _ctx(self):
        if self._ctx_arg is None:
            self._ctx_arg = default_context()
        return self._ctx_arg

    def set_source(self, source, weights=None):
        """Build the tree of ``source``; ``weights`` [N] >= 0 (default None: the source's own if it is a
        :class:`WeightedPoints`, else none) as in :func:`buildGMMTree`."""
        weights = _target_weights(source, weights)   # (refused before anything is uploaded)
        self._source = _points(source)
        self._eig_cache = None                       # node covariances are about to change
        t1 = time.time()
        # float64 tables whatever the points' type: the registration re-uploads them, takes eigh of the covariances and
        # 1 / sqrt of their eigenvalues -- a thin leaf covariance rounded to float32 can turn indefinite.  The
        # stop rule's arithmetic still follows the points' type, as in buildGMMTree.
        pdf = np.float32 if self._source.dtype == np.float32 else np.float64
        self._mixingCoeff, self._mean, self._covar = buildGMMTree(
            self._source, self._tree_level, self._ls, self._ld, sig2=self._sig2,
            init_idx=self._init_idx, ctx=self._ctx, dtype=np.float64, pdf_dtype=pdf, weights=weights)
        if self._verbose:
            print("Build tree Time: ", time.time() - t1)

    def set_nodes(self, mixingCoeff, mean, covar):
        """Use an existing tree (e.g. a saved one) instead of building from a source cloud."""
        self._mixingCoeff = np.asarray(mixingCoeff, dtype=np.float64)
        self._mean = np.asarray(mean, dtype=np.float64)
        self._covar = np.array(covar, dtype=np.float64)        # own copy: the eigh cache below belongs to it
        self._eig_cache = None

    def set_callbacks(self, callbacks):
        self._callbacks = callbacks

    def expectation_step(self, target=None):
        """With ``target`` given: E-step on that (already transformed) cloud, like the reference.
        Inside :meth:`registration` the resident target is transformed on the device instead."""
        T = len(self._mixingCoeff)
        with _reg_gate(self._ctx, self._maha2_gate):
            if target is not None:
                _set_target(self._ctx, target)
                self._target_id = None
                m = self._ctx.tree_reg_estep(T, lambda_c=self._lambda_c)
            else:
                tf = self._tf_result
                m = self._ctx.tree_reg_estep(T, tf.rot, tf.t, tf.scale, self._lambda_c)
        return EstepResult(*m)

    def _node_eig(self):
        """eigh of every node covariance.  The nodes do not change during a registration, so the
        decomposition the reference recomputes per node and per iteration (hgmm_gpu.py:737) is
        done once per tree."""
        if getattr(self, "_eig_cache", None) is None:     # invalidated by set_source / set_nodes
            self._eig_cache = np.linalg.eigh(self._covar)
        return self._eig_cache

    def maximization_step(self, estep_res, trans_p):
        """Twist least squares over the nodes that received mass (hgmm_gpu.py:729-752).

        Same system as the reference's ``np.linalg.lstsq(Amat, bmat)`` with its all-zero rows (nodes
        without mass) left out, solved through one QR of [A | b]: x = R^-1 (Q^T b), q = squared
        residual = R[6,6]^2.  Rank-deficient or tiny systems take the reference's exact call."""
        m0, m1 = estep_res.momentZero, estep_res.momentOne
        n = len(self._mixingCoeff)
        live = np.nonzero(~(m0 < np.finfo(np.float32).eps))[0]
        x = q = None
        if len(live) > 2:
            lmd_all, nn_all = self._node_eig()
            lmd, nn = lmd_all[live], nn_all[live]
            s = m1[live] / m0[live][:, None]
            nn = nn * np.sqrt(m0[live][:, None] / lmd)[:, None, :]
            nnT = np.transpose(nn, (0, 2, 1))
            ab = np.empty((3 * len(live), 7))
            ab[:, :3] = np.cross(s[:, None, :], nnT).reshape(-1, 3)
            ab[:, 3:6] = nnT.reshape(-1, 3)
            ab[:, 6] = (np.einsum('nij,nj->ni', nnT, self._mean[live]) - np.einsum('nij,nj->ni', nnT, s)).ravel()
            if np.isfinite(ab).all():
                with _small_lapack():
                    r = np.linalg.qr(ab, mode='r')
                d = np.abs(np.diag(r)[:6])
                if d.min() > 1e-12 * d.max():
                    x = np.linalg.solve(r[:6, :6], r[:6, 6])
                    q = np.array([r[6, 6] ** 2])
        if x is None:
            amat = np.zeros((n * 3, 6))
            bmat = np.zeros(n * 3)
            if len(live):
                lmd, nn = np.linalg.eigh(self._covar[live])
                s = m1[live] / m0[live][:, None]
                nn = nn * np.sqrt(m0[live][:, None] / lmd)[:, None, :]
                nnT = np.transpose(nn, (0, 2, 1))
                b = np.einsum('nij,nj->ni', nnT, self._mean[live]) - np.einsum('nij,nj->ni', nnT, s)
                rows = (3 * live[:, None] + np.arange(3)[None, :]).ravel()
                bmat[rows] = b.ravel()
                amat[rows, :3] = np.cross(s[:, None, :], nnT).reshape(-1, 3)
                amat[rows, 3:] = nnT.reshape(-1, 3)
            x, q, _, _ = np.linalg.lstsq(amat, bmat, rcond=-1)
        rot, t = twist_mul(x, trans_p.rot, trans_p.t)
        return MstepResult(RigidTransformation(rot, t), q)

    def _device_iteration(self):
        """One registration iteration with E-step AND the M-step's least-squares system on the device: the host
        receives the 6 x 6 normal equations (28 numbers), solves them and composes the twist.  The system is the
        reference's (hgmm_gpu.py:729-752) -- sum_c n_c n_c^T = m0 Sigma^-1 makes the per-node eigh unnecessary.
        Returns None when the system is too ill-conditioned for normal equations (the caller then takes the
        reference's stacked least-squares path)."""
        tf = self._tf_result
        ata, atb, btb = self._ctx.tree_reg_normal(tf.rot, tf.t, tf.scale, self._lambda_c)
        if not (np.isfinite(ata).all() and np.isfinite(atb).all()):
            return None
        lam = np.linalg.eigvalsh(ata)
        if not lam[-1] > 0.0 or lam[0] <= 1e-11 * lam[-1]:
            return None
        x = np.linalg.solve(ata, atb)
        q = np.array([max(btb - float(x @ atb), 0.0)])
        rot, t = twist_mul(x, tf.rot, tf.t)
        return MstepResult(RigidTransformation(rot, t), q)

    def _registration_in_library(self, maxiter, tol, _resume=None):
        """The loop of :meth:`registration` without per-iteration Python: ``hgmm_tree_register`` iterates (E-step and
        normal equations on the device, 6 x 6 solve / twist / stop rule on the library's host side) until it stops or
        meets a system too ill-conditioned for normal equations; that one iteration is then done here with the
        reference's stacked least squares, and the library carries on.  Same arithmetic per iteration as
        :meth:`_device_iteration` (used when callbacks want every intermediate transformation)."""
        tf = self._tf_result
        rot, t = np.asarray(tf.rot, dtype=np.float64), np.asarray(tf.t, dtype=np.float64)
        q = None
        it = 0
        host_step_due = False
        if _resume is not None:                      # (a pair that left a batch at status 2: ``it`` iterations done, last q)
            it, q, host_step_due = _resume
        while it < maxiter:
            if not host_step_due:
                with (self._ctx.config(reg_device_solve=1) if self._solve_on_device else contextlib.nullcontext()):
                    rot, t, done, q_new, status, _ = self._ctx.tree_register(rot, t, tf.scale, self._lambda_c, maxiter - it, tol, q)
                it += done
                if done:
                    q = q_new
                self._tf_result = RigidTransformation(rot, t, tf.scale)
                if status != 2:
                    break
            host_step_due = False
            res = self.maximization_step(self.expectation_step(), self._tf_result)      # host M-step, one iteration
            self._tf_result = res.transformation
            rot, t = np.asarray(res.transformation.rot, dtype=np.float64), np.asarray(res.transformation.t, dtype=np.float64)
            it += 1
            q_host = float(np.ravel(res.q)[0]) if np.size(res.q) else None
            if q is not None and q_host is not None and abs(q_host - q) < tol:
                q = q_host
                break
            q = q_host
        self.n_iter_ = it
        return MstepResult(self._tf_result.inverse(), np.array([q]) if q is not None else np.array([]))

    def _score_resident(self, maha2_max=CHI2_3_99, per_point=True, lambda_c=None):
        """TreeScore of the RESIDENT target against the resident tree at the loop's own pose ``self._tf_result``."""
        tf = self._tf_result
        summary, arrays = self._ctx.tree_score(tf.rot, tf.t, tf.scale, self._lambda_c if lambda_c is None else lambda_c,
                                               maha2_max, ("node", "maha2", "logp") if per_point else ())
        return tree_score_from_summary(summary, arrays)

    def score(self, target, transformation=None, maha2_max=CHI2_3_99, per_point=True):
        """How well does this tree explain ``target``?  -> :class:`TreeScore` (``hgmm_tree_score``).

        ``transformation`` is WHAT :meth:`registration` RETURNED -- the inverse of the pose that moves the target onto the
        tree -- so ``gt.score(target, gt.registration(target).transformation)`` is the natural call; None: the target as
        given.  Every point descends the tree as in the registration E-step with this tree's ``lambda_c`` and is scored at the
        node it stops at.  The returned object is inverted again here, and ``-R (-R^T t)`` rounds: the result agrees with
        ``registration(..., return_score=True)`` (which uses the loop's own pose) to rounding, not bit for bit.
        ``per_point=False`` leaves ``node`` / ``maha2`` / ``logp`` None (nothing N-long is stored or downloaded).
        A :class:`WeightedPoints` target: the sums behind the score are weighted (``n`` is the sum of the weights), the
        per-point arrays are not."""
        self._ctx.tree_set_nodes(self._tree_level, self._mixingCoeff, self._mean, self._covar)
        _set_target(self._ctx, target)
        self._target_id = None
        rot = t = None
        scale = 1.0
        if transformation is not None:
            pose = transformation.inverse()
            rot, t, scale = pose.rot, pose.t, pose.scale
        summary, arrays = self._ctx.tree_score(rot, t, scale, self._lambda_c, maha2_max,
                                               ("node", "maha2", "logp") if per_point else ())
        return tree_score_from_summary(summary, arrays)

    def predict(self, points):
        """Node of the LAST level that explains each point (int32 [N]): the descent of the registration E-step without its
        stop rule (``lambda_c < 0``) -- the tree's counterpart of the flat models' ``predict``.  These are the labels of the
        finished tree; the build's own ``currentIdx`` assigns a point within the parent chosen one level up with that
        level's parameters, and need not agree."""
        self._ctx.tree_set_nodes(self._tree_level, self._mixingCoeff, self._mean, self._covar)
        self._ctx.tree_set_target(_points(points))
        self._target_id = None
        return self._ctx.tree_score(lambda_c=-1.0, want=("node",))[1]["node"]

    def registration(self, target, maxiter=20, tol=1.0e-4, return_score=False, maha2_max=CHI2_3_99, maha2_gate=None,
                     weights=None):
        """-> MstepResult(tf.inverse(), q)   (hgmm_gpu.py:754-768).  ``return_score=True``: ScoredResult(tf.inverse(), q,
        score) with the :class:`TreeScore` of the target at the final pose, taken with the loop's own (R, t).
        ``maha2_gate``: the E-step's Mahalanobis gate for this call (default None: the object's own, see the class).
        ``weights`` [N] >= 0 (default None: the target's own if it is a :class:`WeightedPoints`, else none): per-point
        weights of the target, see the class; the score of ``return_score`` is taken under them too."""
        weights = _target_weights(target, weights)   # (refused before anything is uploaded)
        gate = _gate_arg(maha2_gate)
        prev_gate = self._maha2_gate
        if gate is not None:
            self._maha2_gate = gate                  # (the host M-step's expectation_step inside the loop follows it too)
        try:
            with _reg_gate(self._ctx, self._maha2_gate):
                res = self._registration(target, maxiter, tol, weights)
        finally:
            self._maha2_gate = prev_gate
        if return_score:
            return ScoredResult(res.transformation, res.q, self._score_resident(maha2_max))
        return res

    def registration_multistart(self, target, starts, maxiter=20, tol=1.0e-4, maha2_max=CHI2_3_99, return_all=False):
        """:meth:`registration` from K start poses in the launches of one (``hgmm_tree_register_multi``), scored together
        (``hgmm_tree_score_multi``); the best one wins (:func:`best_hypothesis`).  The registration is a local method: from
        the identity a target turned by 30 degrees ends in a wrong minimum, and the score tells -- a grid of starts
        (:func:`rotation_starts`) turns that into a success.

        ``starts`` are initial values of the loop's OWN pose y = s R x + t, which moves the TARGET onto the tree -- what the
        identity is in :meth:`registration` -- not the inverted object that :meth:`registration` returns; they share one
        scale.  Every hypothesis is bit for bit what the serial loop gives from that start; one whose normal equations turn
        ill-conditioned is finished through the serial path like a pair that leaves a batch.

        -> :class:`MultiStartResult` (a ``ScoredResult(tf.inverse(), q, score)``) of the winner, with ``best_index_`` and
        ``n_iter_`` (also set on this object); with ``return_all`` also a list of K ``ScoredResult``s -- only the winner's
        score carries the per-point arrays (one serial ``hgmm_tree_score``).  The object's ``maha2_gate`` (see the class)
        applies to every hypothesis, and so do the weights of a :class:`WeightedPoints` target (one array, shared)."""
        with _reg_gate(self._ctx, self._maha2_gate):
            return self._registration_multistart(target, starts, maxiter, tol, maha2_max, return_all)

    def _registration_multistart(self, target, starts, maxiter, tol, maha2_max, return_all):
        starts = list(starts)
        if not starts:
            raise ValueError("registration_multistart: no start poses")
        scale = float(starts[0].scale)
        if any(float(s.scale) != scale for s in starts):
            raise ValueError("registration_multistart: the start poses must share one scale")
        ctx = self._ctx
        ctx.tree_set_nodes(self._tree_level, self._mixingCoeff, self._mean, self._covar)
        _set_target(ctx, target)
        rot0 = np.stack([np.asarray(s.rot, dtype=np.float64).reshape(3, 3) for s in starts])
        t0 = np.stack([np.asarray(s.t, dtype=np.float64).reshape(3) for s in starts])
        with (ctx.config(reg_device_solve=1) if self._solve_on_device else contextlib.nullcontext()):
            rot, t, iters, q, status, _ = ctx.tree_register_multi(rot0, t0, scale, self._lambda_c, maxiter, tol)
        iters = [int(v) for v in iters]
        for k in np.nonzero(status == 2)[0]:                      # finish this hypothesis through the serial entries
            self._tf_result = RigidTransformation(rot[k].copy(), t[k].copy(), scale)
            res = self._registration_in_library(maxiter, tol, _resume=(iters[k], None if np.isnan(q[k]) else float(q[k]), True))
            rot[k], t[k] = self._tf_result.rot, self._tf_result.t
            q[k] = float(res.q[0]) if np.size(res.q) else np.nan
            iters[k] = int(self.n_iter_)
        sums = ctx.tree_score_multi(rot, t, scale, self._lambda_c, maha2_max)
        best = best_hypothesis(sums, rot, t)
        poses = [RigidTransformation(rot[k].copy(), t[k].copy(), scale) for k in range(len(starts))]
        qs = [np.array([q[k]]) if not np.isnan(q[k]) else np.array([]) for k in range(len(starts))]
        self._tf_result = poses[best]
        self.best_index_, self.n_iter_ = int(best), iters[best]
        winner = MultiStartResult(poses[best].inverse(), qs[best], self._score_resident(maha2_max))
        winner.best_index_, winner.n_iter_ = int(best), iters[best]
        if not return_all:
            return winner
        every = [winner if k == best else ScoredResult(poses[k].inverse(), qs[k], tree_score_from_summary(sums[k]))
                 for k in range(len(starts))]
        return winner, every

    def _registration(self, target, maxiter, tol, weights=None):
        self._ctx.tree_set_nodes(self._tree_level, self._mixingCoeff, self._mean, self._covar)
        _set_target(self._ctx, target, weights)
        if self._device_mstep and not self._callbacks:
            return self._registration_in_library(maxiter, tol)
        q = None
        res = None
        self.n_iter_ = 0
        for _ in range(maxiter):
            self.n_iter_ += 1
            res = self._device_iteration() if self._device_mstep else None
            if res is None:
                estep_res = self.expectation_step()      # target transformed on the device
                res = self.maximization_step(estep_res, self._tf_result)
            self._tf_result = res.transformation
            for c in self._callbacks:
                c(self._tf_result.inverse())
            if q is not None and np.size(q) and np.size(res.q) and abs(res.q - q) < tol:
                break
            q = res.q
        return MstepResult(self._tf_result.inverse(), res.q)


def euler_matrix_xyz(ai, aj, ak):
    """Static-frame x-y-z Euler angles -> 3x3 rotation (what the absent third-party
    ``transformations.euler_matrix(ai, aj, ak)`` default 'sxyz' returns; hgmm_gpu.py:790)."""
    ci, si, cj, sj, ck, sk = np.cos(ai), np.sin(ai), np.cos(aj), np.sin(aj), np.cos(ak), np.sin(ak)
    rx = np.array([[1, 0, 0], [0, ci, -si], [0, si, ci]])
    ry = np.array([[cj, 0, sj], [0, 1, 0], [-sj, 0, cj]])
    rz = np.array([[ck, -sk, 0], [sk, ck, 0], [0, 0, 1.0]])
    return rz @ ry @ rx


def prepare_source_and_target_rigid_3d(source, noise_amp=0.001, n_random=500,
                                       orientation=np.deg2rad([0.0, 0.0, 30.0]), translation=np.zeros(3),
                                       voxel_size=0.005, rng=None, ctx=None):
    """Noisy, cluttered, rigidly moved copy of a cloud for registration experiments
    (hgmm_gpu.py:772-795 minus Open3D/normals): voxel down-sample, shuffle, add Gaussian noise and
    ``n_random`` uniform outliers in a 1.5x bounding box, then rotate/translate.
    ``source``: [N,3] array or a .ply/.pcd path.  ``ctx`` (default None: on the host): the Context whose device does the
    down-sample (``pointcloud_io.voxel_down_sample(..., ctx=ctx)``, the same values).  -> (source_points, target_points)."""
    from ..pointcloud_io import read_point_cloud, voxel_down_sample
    rng = rng or np.random
    src = read_point_cloud(source) if isinstance(source, str) else np.asarray(source, dtype=np.float64)
    if voxel_size:
        src = voxel_down_sample(src, voxel_size, ctx=ctx)
    tp = src.copy()
    rng.shuffle(tp)
    rg = 1.5 * (tp.max(axis=0) - tp.min(axis=0))
    rands = (rng.rand(n_random, 3) - 0.5) * rg + tp.mean(axis=0)
    tgt = np.r_[tp + noise_amp * rng.randn(*tp.shape), rands]
    rot = euler_matrix_xyz(*orientation)
    return src, tgt @ rot.T + np.asarray(translation)


def _voxel_pairs(ctx, pairs, voxel_size, explicit_weights):
    """``voxel_size=`` of the registration functions: every DISTINCT cloud of ``pairs`` down-sampled on ``ctx``'s device by
    ONE batch call (``Context.voxel_down_sample_batch(..., download=False)``), -> pairs of :class:`VoxelCloud`: the result
    stays on the device and is handed to build and registration there.  Distinct means identity (``is``): a scan that is the
    target of one pair and the source of the next -- the same object -- is one member, down-sampled once; equal arrays that
    are different objects are not merged.  Weights of the caller's own next to a voxel size are refused: they belong to the
    points that are about to be replaced."""
    own = any(getattr(c, "weights", None) is not None for p in pairs for c in p)
    if own or any(w is not None for w in explicit_weights):
        raise ValueError("voxel_size replaces the clouds by their voxel centroids, weighted by the counts: it cannot be "
                         "combined with source_weights / target_weights (or WeightedPoints inputs)")
    if any(_is_voxels(c) for p in pairs for c in p):
        raise ValueError("voxel_size next to a VoxelCloud: that cloud has been down-sampled already")
    distinct, member = [], {}                      # (`distinct` keeps every object alive: its id stays its own)
    for p in pairs:
        for c in p:
            if id(c) not in member:
                member[id(c)] = len(distinct)
                distinct.append(c)
    res = ctx.voxel_down_sample_batch([_points(c) for c in distinct], voxel_size, download=False)
    return [(res.member(member[id(s)]), res.member(member[id(t)])) for s, t in pairs]


def _voxels_to_host(clouds, weights):
    """A list of clouds of which only SOME are :class:`VoxelCloud`s (the batched hand-overs take members only): those come
    to the host as (centroids, counts) -- ``weights`` (a list, changed in place) receives the counts.  Each distinct voxel
    result is downloaded once, whatever the number of its members in the list."""
    if not any(_is_voxels(c) for c in clouds) or all(_is_voxels(c) for c in clouds):
        return clouds
    out, host = list(clouds), {}
    for k, c in enumerate(out):
        if _is_voxels(c):
            if id(c.result) not in host:
                host[id(c.result)] = c.result.get()
            cent, cnt = host[id(c.result)][c.index]
            out[k], weights[k] = cent, cnt.astype(np.float64)
    return out


def registration_gmmtree(source, target, maxiter=20, tol=1.0e-4, callbacks=[], return_score=False, starts=None, **kargs):
    """hgmm_gpu.py:802-807.  ``return_score=True``: ScoredResult(transformation, q, score) -- see :meth:`GMMTree.registration`.
    ``starts`` (a list of start poses, e.g. :func:`rotation_starts`): :meth:`GMMTree.registration_multistart`'s result.
    ``maha2_gate=`` (among :class:`GMMTree`'s arguments): the registration E-step's Mahalanobis gate, with or without ``starts``.
    ``target_weights=`` [N] >= 0 (a keyword of this function, not of :class:`GMMTree`; default: the target's own if it is a
    :class:`WeightedPoints`): per-point weights of the target, with or without ``starts``.
    ``source_weights=`` [N] >= 0 (default: the source's own if it is a :class:`WeightedPoints`): per-point weights of the
    source for the tree build, as in :func:`buildGMMTree`.
    ``voxel_size=`` (a keyword of this function like the weights; default None: the clouds as they are): both clouds are
    voxel-down-sampled on the device first (one ``Context.voxel_down_sample_batch`` call) and the counts travel as source and
    target weights -- bit for bit this call on ``WeightedPoints(*voxel_down_sample(cloud, voxel_size, True))`` inputs; with
    explicit weights: ValueError.  Centroids and counts do not come to the host in between: the clouds become
    :class:`VoxelCloud`s, which ``source`` and ``target`` may also be from the start (``Context.voxel_down_sample(...,
    download=False)``; explicit weights next to one: ValueError)."""
    voxel_size = kargs.pop("voxel_size", None)
    if voxel_size is not None:
        (source, target), = _voxel_pairs(kargs.get("ctx") or default_context(), [(source, target)], voxel_size,
                                         [kargs.get("source_weights"), kargs.get("target_weights")])
    weights = _target_weights(target, kargs.pop("target_weights", None))
    kargs["source_weights"] = _target_weights(source, kargs.pop("source_weights", None))
    gt = GMMTree(_points(source), **kargs)           # (a VoxelCloud: handed over on the device, build and target alike)
    if starts is not None:
        tgt = _points(target) if weights is None else WeightedPoints(_points(target), weights)
        return gt.registration_multistart(tgt, starts, maxiter, tol)
    gt.set_callbacks(callbacks)
    return gt.registration(_points(target), maxiter, tol, return_score=return_score, weights=weights)


BATCH_MAX_POINTS = 400000       # hgmm_tree_build_batch takes clouds below this size (csrc/tree_batch.hip)


def _batch_starts(starts, B):
    """``starts=`` of :func:`registration_gmmtree_batch` -> (B lists of start poses, their common scale).  One list of
    :class:`RigidTransformation`s serves every pair; a list of lists is one list per pair (they may differ in length)."""
    starts = list(starts)
    if starts and all(isinstance(s, (list, tuple)) for s in starts):
        if len(starts) != B:
            raise ValueError("starts must be one list of start poses, or one such list per pair: %d lists for %d pairs"
                             % (len(starts), B))
        per_pair = [list(s) for s in starts]
    else:
        per_pair = [starts] * B
    for b, s in enumerate(per_pair):
        if not s:
            raise ValueError("starts: pair %d has no start pose" % b)
    scale = float(per_pair[0][0].scale)
    for b, ss in enumerate(per_pair):
        if any(float(s.scale) != scale for s in ss):
            raise ValueError("starts: the start poses of a call must share one scale (pair %d differs)" % b)
    return per_pair, scale


def _multistart_info(B):
    return {"build_iters": [None] * B, "registration_iters": [None] * B, "status": [None] * B, "score": [None] * B,
            "hypothesis_iters": [None] * B, "hypothesis_status": [None] * B, "hypothesis_scores": [None] * B}


def _register_batch_multistart(ctx, starts, scale, tgts, ws, tree_level, lambda_c, ls, ld, sig2, maxiter, tol, solve_on_device,
                               gate, maha2_max, clock):
    """The registration half of :func:`registration_gmmtree_batch` with ``starts``: the forest and its targets are resident on
    ``ctx``.  All hypotheses of all pairs in the launches of one (``hgmm_tree_register_batch_multi``, in consecutive rounds
    where the sums' cap demands), those that left at status 2 finished through the serial entries, one
    ``hgmm_tree_score_batch_multi`` at the final poses, the winner per pair by :func:`best_hypothesis`.
    -> (one :class:`MultiStartResult` per pair, per-pair lists of every hypothesis's iterations, status and TreeScore)."""
    B = len(tgts)
    owners = np.repeat(np.arange(B, dtype=np.int32), [len(s) for s in starts])
    flat = [s for ss in starts for s in ss]
    rot = np.stack([np.asarray(s.rot, dtype=np.float64).reshape(3, 3) for s in flat])
    t = np.stack([np.asarray(s.t, dtype=np.float64).reshape(3) for s in flat])
    R = len(flat)
    iters, q, status = np.zeros(R, np.int32), np.full(R, np.nan), np.zeros(R, np.int32)
    rounds = _native.plan_batch_multi_rounds(n_total_nodes(tree_level), owners)
    with _reg_gate(ctx, gate):                                   # (the rounds AND the hypotheses finished serially below)
        with (ctx.config(reg_device_solve=1) if solve_on_device else contextlib.nullcontext()):
            for a, e in rounds:
                rot[a:e], t[a:e], iters[a:e], q[a:e], status[a:e], _ = ctx.tree_register_batch_multi(
                    owners[a:e], rot[a:e], t[a:e], scale, lambda_c, maxiter, tol)
        clock.append(time.perf_counter())
        iters = [int(v) for v in iters]
        serial = {}                                              # hypothesis -> its summary from the serial entry
        for r in np.nonzero(status == 2)[0]:                     # finish this hypothesis through the serial entries
            b = int(owners[r])
            gt = GMMTree(tree_level=tree_level, lambda_c=lambda_c, ls=ls, ld=ld, sig2=sig2, ctx=ctx,
                         solve_on_device=solve_on_device, maha2_gate=gate)
            gt.set_nodes(*ctx.tree_get_nodes_batch(b, tree_level))
            gt._tf_result = RigidTransformation(rot[r].copy(), t[r].copy(), scale)
            ctx.tree_set_nodes(tree_level, gt._mixingCoeff, gt._mean, gt._covar)
            _set_target(ctx, tgts[b], ws[b])
            res = gt._registration_in_library(maxiter, tol, _resume=(iters[r], None if np.isnan(q[r]) else float(q[r]), True))
            rot[r], t[r] = gt._tf_result.rot, gt._tf_result.t
            q[r] = float(res.q[0]) if np.size(res.q) else np.nan
            iters[r] = int(gt.n_iter_)
            serial[int(r)] = ctx.tree_score(rot[r], t[r], scale, lambda_c, maha2_max, ())[0]
    sums = np.concatenate([ctx.tree_score_batch_multi(owners[a:e], rot[a:e], t[a:e], scale, lambda_c, maha2_max)
                           for a, e in rounds])
    for r, summary in serial.items():                            # (its pose moved on: the serial entry, at the final pose)
        sums[r] = summary
    clock.append(time.perf_counter())
    out, every = [], ([], [], [])
    at = 0
    for b in range(B):
        rows = slice(at, at + len(starts[b]))
        at += len(starts[b])
        best = best_hypothesis(sums[rows], rot[rows], t[rows])
        r = rows.start + best
        tf = RigidTransformation(rot[r].copy(), t[r].copy(), scale)
        scores = [tree_score_from_summary(v) for v in sums[rows]]
        win = MultiStartResult(tf.inverse(), np.array([q[r]]) if not np.isnan(q[r]) else np.array([]), scores[best])
        win.best_index_, win.n_iter_ = int(best), iters[r]
        out.append(win)
        every[0].append(iters[rows])
        every[1].append([int(v) for v in status[rows]])
        every[2].append(scores)
    return out, every


def registration_gmmtree_batch(pairs, maxiter=20, tol=1.0e-4, ctx: Context | None = None, tree_level=5, lambda_c=0.01,
                               ls=20, ld=1.0e-4, sig2=0.004, init_idx=None, return_info=False, pdf_dtype=None,
                               solve_on_device=False, score=False, maha2_gate=None, target_weights=None, source_weights=None,
                               voxel_size=None, starts=None, maha2_max=CHI2_3_99):
    """``[registration_gmmtree(s, t, maxiter, tol, tree_level=..., ...) for s, t in pairs]`` (hgmm_gpu.py:802-807 per pair)
    with ALL pairs in the same launches: the B source clouds are one resident forest (``hgmm_tree_build_batch``: levels in
    lock-step, one stop rule per cloud), the B targets are registered against their trees together
    (``hgmm_tree_register_batch``: one E-step + one normal-equations launch per iteration, the 6 x 6 solves on the host).
    Every pair's tree, iteration counts and transformation are bitwise what the serial call returns for it.  A pair whose
    normal equations turn ill-conditioned leaves the batch and is finished by the serial path (stacked least squares on
    the host, like :meth:`GMMTree._registration_in_library`).  Clouds of 400 000 points or more go through the serial call.

    ``pdf_dtype``: the arithmetic of the build's stop rule, as in :class:`GMMTree` -- default: each SOURCE's own type
    (float32 scans, the type of the reference's GPU file, hgmm_gpu.py:472: float32 pdfs; anything else float64); pairs
    of either kind in one call run as two batches.  Tables, E-step, moments and the registration are float64 either way.

    ``score=True`` (with ``return_info``): ``info["score"]`` holds one :class:`TreeScore` per pair, of the target at the pose
    its loop ended at (no per-point arrays) -- one ``hgmm_tree_score_batch`` call after the registration; pairs that ran or
    finished serially are scored through the serial entry.  The same numbers, bit for bit, as
    ``registration_gmmtree(..., return_score=True).score``.

    ``maha2_gate`` (default None: no gate): the registration E-step's Mahalanobis gate for every pair, as in
    :class:`GMMTree`; pairs that run or finish serially are registered under it too.  The context's own gate is restored.

    ``target_weights`` (default None: none): a list with one entry per pair -- per-point weights [N_b] >= 0 of that pair's
    target as in :class:`GMMTree`, or None for a pair without (a target that is a :class:`WeightedPoints` brings its own);
    the scores of ``score=True`` are taken under them, and pairs that run or finish serially follow them too.

    ``source_weights`` (default None: none): likewise a list with one entry per pair -- per-point weights [N_b] >= 0 of that
    pair's SOURCE for the tree build as in :func:`buildGMMTree`, or None for a pair without (a source that is a
    :class:`WeightedPoints` brings its own); an unweighted pair's tree is bitwise its unweighted tree, and the pairs of
    400 000 points or more that run serially are built under their weights too.

    ``voxel_size`` (default None: the clouds as they are): all 2B clouds are voxel-down-sampled on the device first, by ONE
    ``Context.voxel_down_sample_batch`` call, and the counts travel as source and target weights -- bit for bit this call
    on ``WeightedPoints(*voxel_down_sample(cloud, voxel_size, True))`` inputs; with explicit weights: ValueError.  Each
    DISTINCT array object is down-sampled once (a chain ``[(a, b), (b, c)]`` down-samples three clouds), and nothing but the
    results comes back to the host: the clouds travel as :class:`VoxelCloud`s, which the pairs may also hold from the start.

    ``starts`` (default None: every pair from the identity, the call as it was): multi-start for every pair of the batch --
    one list of start poses (e.g. :func:`rotation_starts`) used for every pair, or a list with one such list per pair, which
    may differ in length; all starts of the call share one scale.  The forest is built and uploaded as without; then ALL
    hypotheses of ALL pairs run through the launches of one (``hgmm_tree_register_batch_multi``: hypothesis r names its pair
    and owns its slice of the sums; in consecutive rounds where the sums' cap demands), are scored together
    (``hgmm_tree_score_batch_multi``, inlier bound ``maha2_max``) and the best one per pair wins (:func:`best_hypothesis`).
    The result is one :class:`MultiStartResult` per pair -- ``best_index_``, ``n_iter_`` and a summary-only
    :class:`TreeScore` -- whose ``transformation``, ``q``, ``best_index_``, ``n_iter_`` and score scalars are bitwise those
    of ``registration_gmmtree(s, t, maxiter, tol, starts=..., same keywords)``.  With ``return_info`` the dict's
    ``"score"``, ``"registration_iters"`` and ``"status"`` are the winners', and ``"hypothesis_iters"`` /
    ``"hypothesis_status"`` / ``"hypothesis_scores"`` hold per pair the list over its hypotheses (iterations and status are
    None for a pair of 400 000 points or more, which runs :meth:`GMMTree.registration_multistart` serially).

    -> list of ``MstepResult(transformation, q)`` in the order of ``pairs`` (+ a dict with the per-pair build / registration
    iteration counts with ``return_info``)."""
    gate = _gate_arg(maha2_gate)
    ctx = ctx or default_context()
    pairs = list(pairs)
    if not pairs:
        return ([], {}) if return_info else []
    if starts is not None:                          # (refused before the device is reached)
        starts, starts_scale = _batch_starts(starts, len(pairs))
    if voxel_size is not None:
        pairs = _voxel_pairs(ctx, pairs, voxel_size, [w for ws in (target_weights, source_weights) if ws is not None for w in ws])
    if target_weights is not None and len(target_weights) != len(pairs):
        raise ValueError("target_weights must have one entry (an array or None) per pair: %d entries for %d pairs"
                         % (len(target_weights), len(pairs)))
    ws = [_target_weights(pairs[k][1], None if target_weights is None else target_weights[k]) for k in range(len(pairs))]
    if source_weights is not None and len(source_weights) != len(pairs):
        raise ValueError("source_weights must have one entry (an array or None) per pair: %d entries for %d pairs"
                         % (len(source_weights), len(pairs)))
    sws = [_target_weights(pairs[k][0], None if source_weights is None else source_weights[k]) for k in range(len(pairs))]
    # (from here on the weights travel as lists: the recursive calls below must not read a WeightedPoints' own a second time)
    pairs = [(_points(s), t) for s, t in pairs]
    # (VoxelClouds among host arrays: the batched hand-overs take members only, so those come to the host with their counts)
    pairs = list(zip(_voxels_to_host([s for s, _ in pairs], sws), _voxels_to_host([t for _, t in pairs], ws)))
    big = [k for k, (s, _) in enumerate(pairs) if len(_points(s)) >= BATCH_MAX_POINTS]
    if big:
        # a cloud of >= 400 000 points fills the chip by itself and takes the serial build's four-points-per-thread
        # log-likelihood, which the batched path does not reproduce: those pairs run one by one, the rest as a batch
        out = [None] * len(pairs)
        info = {"build_iters": np.full((len(pairs), tree_level), -1, np.int32), "registration_iters": [None] * len(pairs),
                "status": [None] * len(pairs)}
        if score:
            info["score"] = [None] * len(pairs)
        if starts is not None:
            info.update({k: v for k, v in _multistart_info(len(pairs)).items() if k != "build_iters"})
        for k in big:
            gt = GMMTree(pairs[k][0], tree_level=tree_level, lambda_c=lambda_c, ls=ls, ld=ld, sig2=sig2, init_idx=init_idx, ctx=ctx,
                         solve_on_device=solve_on_device, maha2_gate=gate, source_weights=sws[k])
            if starts is not None:
                tgt = _points(pairs[k][1]) if ws[k] is None else WeightedPoints(_points(pairs[k][1]), ws[k])
                out[k], every = gt.registration_multistart(tgt, starts[k], maxiter, tol, maha2_max, return_all=True)
                info["registration_iters"][k], info["status"][k], info["score"][k] = int(gt.n_iter_), 0, out[k].score
                info["hypothesis_scores"][k] = [e.score for e in every]
                continue
            out[k] = gt.registration(_points(pairs[k][1]), maxiter, tol, weights=ws[k])
            info["registration_iters"][k], info["status"][k] = int(gt.n_iter_), 0
            if score:
                info["score"][k] = gt._score_resident(per_point=False)
        rest = [k for k in range(len(pairs)) if k not in set(big)]
        if rest:
            r, inf = registration_gmmtree_batch([pairs[k] for k in rest], maxiter, tol, ctx, tree_level, lambda_c, ls, ld, sig2,
                                                init_idx, True, pdf_dtype, solve_on_device, score, gate, [ws[k] for k in rest],
                                                source_weights=[sws[k] for k in rest],
                                                starts=None if starts is None else [starts[k] for k in rest], maha2_max=maha2_max)
            for j, k in enumerate(rest):
                out[k] = r[j]
                info["build_iters"][k] = inf["build_iters"][j]
                for key in info:
                    if key != "build_iters":
                        info[key][k] = inf[key][j]
        return (out, info) if return_info else out
    if pdf_dtype is None:
        kinds = [np.dtype(np.float32) if _points(s).dtype == np.float32 else np.dtype(np.float64) for s, _ in pairs]
        if len(set(kinds)) > 1:                                   # one batch per kind, results back in the caller's order
            out, info = [None] * len(pairs), {"build_iters": [None] * len(pairs), "registration_iters": [None] * len(pairs),
                                              "status": [None] * len(pairs)}
            if score:
                info["score"] = [None] * len(pairs)
            if starts is not None:
                info.update(_multistart_info(len(pairs)))
            for kind in sorted(set(kinds), key=str):
                sel = [k for k, v in enumerate(kinds) if v == kind]
                r, inf = registration_gmmtree_batch([pairs[k] for k in sel], maxiter, tol, ctx, tree_level, lambda_c, ls, ld,
                                                    sig2, init_idx, True, kind, solve_on_device, score, gate,
                                                    [ws[k] for k in sel], source_weights=[sws[k] for k in sel],
                                                    starts=None if starts is None else [starts[k] for k in sel],
                                                    maha2_max=maha2_max)
                for j, k in enumerate(sel):
                    out[k] = r[j]
                    for key in info:
                        info[key][k] = inf[key][j]
            info["build_iters"] = np.asarray(info["build_iters"])
            return (out, info) if return_info else out
        pdf_dtype = kinds[0]
    clock = [time.perf_counter()]
    # (float32 clouds are handed over as they are -- the library widens them on the device, exactly -- and only the T rows of
    #  the initial means are widened here)
    srcs = [_points(s) for s, _ in pairs]
    tgts = [_points(t) for _, t in pairs]
    B = len(pairs)
    T = n_total_nodes(tree_level)
    idx = np.asarray(init_idx) if init_idx is not None else np.random.RandomState(72).randint(T, size=T)
    vox_src, vox_tgt = _is_voxels(srcs[0]), _is_voxels(tgts[0])      # (all of a side or none: _voxels_to_host)
    init = dict(init_mu=None, init_rows=idx) if vox_src else dict(init_mu=np.stack([np.asarray(S[idx], dtype=np.float64) for S in srcs]))
    clock.append(time.perf_counter())
    if vox_src:
        ctx.set_points_batch_from_voxels(srcs, weighted=True)
    elif any(w is not None for w in sws):
        ctx.set_points_batch(srcs, weights=sws)
    else:
        ctx.set_points_batch(srcs)
    clock.append(time.perf_counter())
    prev = getattr(ctx, "tree_dtype", np.dtype(np.float64))     # (a precision the caller set on the context survives this call)
    ctx.tree_set_precision(pdf_dtype)
    try:
        _, build_iters, _ = ctx.tree_build_batch([len(S) for S in srcs], tree_level, ls, ld, sig2=sig2, want_tables=False, **init)
    finally:
        ctx.tree_set_precision(prev)
    clock.append(time.perf_counter())
    if vox_tgt:
        ctx.tree_set_targets_batch_from_voxels(tgts, weighted=True)
    elif any(w is not None for w in ws):
        ctx.tree_set_targets_batch(tgts, weights=ws)
    else:
        ctx.tree_set_targets_batch(tgts)
    clock.append(time.perf_counter())
    if starts is not None:
        out, (hyp_iters, hyp_status, hyp_scores) = _register_batch_multistart(
            ctx, starts, starts_scale, tgts, ws, tree_level, lambda_c, ls, ld, sig2, maxiter, tol, solve_on_device, gate,
            maha2_max, clock)
        if not return_info:
            return out
        clock.append(time.perf_counter())
        phases = dict(zip(("prepare", "sources_up", "build", "targets_up", "register", "score", "results"),
                          (1e3 * np.diff(clock)).tolist()))
        return out, {"build_iters": build_iters, "registration_iters": [w.n_iter_ for w in out],
                     "status": [hyp_status[b][w.best_index_] for b, w in enumerate(out)], "phases_ms": phases,
                     "score": [w.score for w in out], "hypothesis_iters": hyp_iters, "hypothesis_status": hyp_status,
                     "hypothesis_scores": hyp_scores}
    rot0 = np.tile(np.identity(3), (B, 1, 1))
    with _reg_gate(ctx, gate):                                   # (the batch AND the pairs finished serially below)
        if solve_on_device:                                          # (per-context option reg_device_solve for this call)
            with ctx.config(reg_device_solve=1):
                rot, t, iters, q, status, _ = ctx.tree_register_batch(rot0, np.zeros((B, 3)), 1.0, lambda_c, maxiter, tol)
        else:
            rot, t, iters, q, status, _ = ctx.tree_register_batch(rot0, np.zeros((B, 3)), 1.0, lambda_c, maxiter, tol)
        clock.append(time.perf_counter())
        # (the batch is scored first: finishing a pair serially below moves the context's serial tree and target, not the forest)
        scores = None
        if score:
            sums = ctx.tree_score_batch(rot, t, 1.0, lambda_c)
            scores = [tree_score_from_summary(sums[b]) for b in range(B)]
        clock.append(time.perf_counter())
        out = []
        reg_iters = [int(v) for v in iters]
        for b in range(B):
            if status[b] == 2:                                        # finish this pair through the serial entries
                gt = GMMTree(tree_level=tree_level, lambda_c=lambda_c, ls=ls, ld=ld, sig2=sig2, ctx=ctx,
                             solve_on_device=solve_on_device, maha2_gate=gate)
                gt.set_nodes(*ctx.tree_get_nodes_batch(b, tree_level))
                gt._tf_result = RigidTransformation(rot[b], t[b])
                ctx.tree_set_nodes(tree_level, gt._mixingCoeff, gt._mean, gt._covar)
                _set_target(ctx, tgts[b], ws[b])
                res = gt._registration_in_library(maxiter, tol, _resume=(int(iters[b]), None if np.isnan(q[b]) else float(q[b]), True))
                reg_iters[b] = int(gt.n_iter_)
                if score:                                                 # (its pose moved on: the serial entry, at the final pose)
                    scores[b] = gt._score_resident(per_point=False)
                out.append(res)
                continue
            tf = RigidTransformation(rot[b].copy(), t[b].copy())
            out.append(MstepResult(tf.inverse(), np.array([q[b]]) if not np.isnan(q[b]) else np.array([])))
    if return_info:
        clock.append(time.perf_counter())
        # wall time of the call's phases, ms: host preparation (type conversion, initial means), upload of the sources, forest
        # build, upload of the targets, batched registration, score (0 unless asked for), result objects
        phases = dict(zip(("prepare", "sources_up", "build", "targets_up", "register", "score", "results"),
                          (1e3 * np.diff(clock)).tolist()))
        info = {"build_iters": build_iters, "registration_iters": reg_iters, "status": [int(v) for v in status],
                "phases_ms": phases}
        if score:
            info["score"] = scores
        return out, info
    return out
