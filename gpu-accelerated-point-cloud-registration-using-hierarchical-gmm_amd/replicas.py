"""Replica fan-out: INDEPENDENT units of work -- scan pairs to register, frames to fit -- spread over the GPUs of one
node with no communication between them ("Independent scan pairs: no communication ('replicas')").

The reference's unit of work is one pair: ``registration_gmmtree(source, target, ...)`` (src/python/hgmm/hgmm_gpu.py:
802-807) or ``registration_gmmreg(source, target, ...)`` (gmmreg_gpu/gmmreg.py:149-157), on one GPU.  Here a pool owns
one engine context per device (or several per device: a 40 k-point pair occupies a chip for a few milliseconds and
leaves most of it idle), each driven by its own thread; the library's calls drop the GIL, every C-ABI entry selects its
context's device itself (csrc/hgmm_ctx.h, HGMM_ENTER), so the threads never touch each other's state.  Jobs are handed
out dynamically (a pair that converges early frees its GPU for the next one); results come back in job order.

    from hgmm_amd.replicas import register_pairs
    results = register_pairs([(src0, tgt0), (src1, tgt1), ...], tree_level=3, maxiter=20)     # all visible GPUs

One process per GPU under an external launcher (torchrun) needs none of this: every rank simply registers its own pairs
on its own context (bench.py --mode pairs does exactly that and only meets the other ranks for the timing barrier).
"""
from __future__ import annotations

import ctypes
import queue
import threading

from ._native import Context, load_library, use_context


def device_count() -> int:
    n = ctypes.c_int(0)
    load_library().hgmm_device_count(ctypes.byref(n))
    return n.value


class ReplicaPool:
    """``contexts_per_device`` engine contexts on each of ``devices`` (default: every visible GPU), one worker thread
    per context.  ``map(fn, jobs)`` calls ``fn(ctx, job)`` for every job and returns the results in job order; the
    first exception of a worker is re-raised after the queue has drained."""

    def __init__(self, devices=None, contexts_per_device: int = 1, context_factory=Context):
        if devices is None:
            devices = list(range(max(device_count(), 1)))
        self.devices = [int(d) for d in devices for _ in range(max(int(contexts_per_device), 1))]
        if not self.devices:
            raise ValueError("ReplicaPool: no devices")
        self._factory = context_factory
        self._ctxs = [None] * len(self.devices)
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _context(self, i):
        if self._ctxs[i] is None:
            self._ctxs[i] = self._factory(self.devices[i])
        return self._ctxs[i]

    def map(self, fn, jobs):
        if self._closed:
            raise RuntimeError("ReplicaPool is closed")
        jobs = list(jobs)
        results = [None] * len(jobs)
        errors = []
        todo = queue.SimpleQueue()
        for item in enumerate(jobs):
            todo.put(item)

        def work(i):
            try:
                ctx = self._context(i)                       # created by the thread that uses it
                with use_context(ctx):                       # module-level mirror functions of this thread run on it
                    while not errors:
                        try:
                            k, job = todo.get_nowait()
                        except queue.Empty:
                            return
                        results[k] = fn(ctx, job)
            except BaseException as e:                       # noqa: BLE001 -- handed to the caller below
                errors.append((i, e))
                c = self._ctxs[i]                            # a context that failed mid-call is not handed out again
                self._ctxs[i] = None
                if c is not None:
                    try:
                        c.close()
                    except Exception:                        # noqa: BLE001 -- the original error is the one to report
                        pass

        threads = [threading.Thread(target=work, args=(i,), name="hgmm-replica-%d" % i, daemon=True)
                   for i in range(min(len(self.devices), max(len(jobs), 1)))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            i, e = errors[0]
            raise RuntimeError("replica %d (device %d) failed: %r" % (i, self.devices[i], e)) from e
        return results

    def close(self):
        self._closed = True
        for i, c in enumerate(self._ctxs):
            if c is not None:
                c.close()
                self._ctxs[i] = None


def register_pairs(pairs, devices=None, contexts_per_device: int = 1, maxiter: int = 20, tol: float = 1.0e-4,
                   method: str = "gmmtree", pool: ReplicaPool | None = None, batch: int = 1, score: bool = False, **kargs):
    """Register every (source, target) pair of ``pairs`` -- arrays [N,3] or objects with ``.points`` -- with
    ``registration_gmmtree`` (``method='gmmtree'``, hgmm/hgmm_gpu.py:802-807; ``kargs`` = GMMTree's: tree_level,
    lambda_c, ls, sig2, ...) or ``registration_gmmreg`` (``method='gmmreg'``, gmmreg_gpu/gmmreg.py:149-157; it has no
    iteration budget or tolerance of its own, so ``maxiter`` / ``tol`` other than the defaults are refused), the pairs
    fanned out over the pool's contexts.  -> the reference's per-pair results, in the order of ``pairs``.
    Per-point weights travel with the pair: a source or target that is a ``WeightedPoints(points, weights)`` brings its own to
    the tree build resp. the registration (``kargs`` go to every pair alike, so the per-pair lists ``source_weights=`` /
    ``target_weights=`` of ``registration_gmmtree_batch`` are not for this function).

    ``batch`` > 1 (gmmtree only): every context takes ``batch`` pairs at a time through the SAME launches
    (``registration_gmmtree_batch``: the trees built as one forest, the targets registered together) -- a 40 k-point pair
    alone is a chain of ~350 small launches that leaves the chip idle; results are bitwise those of ``batch=1``.  Two
    contexts per device let one batch's uploads and 6 x 6 solves overlap the other's kernels.

    ``score=True`` (gmmtree only): every result is a ``ScoredResult(transformation, q, score)`` with the ``TreeScore`` of the
    target at the pose the loop ended at (``registration_gmmtree(..., return_score=True)``; with ``batch`` > 1
    ``registration_gmmtree_batch(..., score=True)``: the same numbers without the per-point arrays).

    ``starts=`` (gmmtree only, among ``kargs``): multi-start for every pair -- one list of start poses for all pairs, or with
    ``batch`` > 1 also one list per pair of ``pairs``.  With ``batch`` > 1 every chunk runs
    ``registration_gmmtree_batch(..., starts=...)`` and every result is its ``MultiStartResult``, which carries the winner's
    score whether ``score`` is set or not."""
    pairs = list(pairs)
    if method == "gmmtree":
        from .hgmm.hgmm_gpu import ScoredResult, registration_gmmtree, registration_gmmtree_batch

        if int(batch) > 1:
            # (starts=: one list for every pair, or one list per pair of ``pairs`` -- those travel with their chunk)
            starts = kargs.pop("starts", None)
            starts_per_pair = starts is not None and len(starts) > 0 and all(isinstance(s, (list, tuple)) for s in starts)
            if starts_per_pair and len(starts) != len(pairs):
                raise ValueError("starts must be one list of start poses, or one such list per pair: %d lists for %d pairs"
                                 % (len(starts), len(pairs)))

            def one(ctx, job):
                first, chunk = job
                if starts is not None:               # every result is a MultiStartResult, which carries its score
                    st = starts[first:first + len(chunk)] if starts_per_pair else starts
                    return registration_gmmtree_batch(chunk, maxiter=maxiter, tol=tol, ctx=ctx, starts=st, **kargs)
                if not score:
                    return registration_gmmtree_batch(chunk, maxiter=maxiter, tol=tol, ctx=ctx, **kargs)
                res, info = registration_gmmtree_batch(chunk, maxiter=maxiter, tol=tol, ctx=ctx, return_info=True, score=True, **kargs)
                return [ScoredResult(r.transformation, r.q, sc) for r, sc in zip(res, info["score"])]
        else:
            def one(ctx, pair):
                if not score:
                    return registration_gmmtree(pair[0], pair[1], maxiter=maxiter, tol=tol, ctx=ctx, **kargs)
                return registration_gmmtree(pair[0], pair[1], maxiter=maxiter, tol=tol, ctx=ctx, return_score=True, **kargs)
    elif method == "gmmreg":
        from .gmmreg_gpu.gmmreg import registration_gmmreg

        if int(batch) > 1:
            raise ValueError("batch > 1 is implemented for method='gmmtree' only")
        if score:
            raise ValueError("score=True is implemented for method='gmmtree' only")
        if maxiter != 20 or tol != 1.0e-4:
            raise ValueError("registration_gmmreg takes neither maxiter nor tol (its optimiser's settings live in "
                             "L2DistRegistration); leave them at their defaults")

        def one(ctx, pair):
            return registration_gmmreg(pair[0], pair[1], ctx=ctx, **kargs)
    else:
        raise ValueError("method must be 'gmmtree' or 'gmmreg', not %r" % (method,))
    own = pool is None
    pool = pool or ReplicaPool(devices, contexts_per_device)
    try:
        if method == "gmmtree" and int(batch) > 1:
            B = int(batch)
            chunks = [(i, pairs[i:i + B]) for i in range(0, len(pairs), B)]
            return [r for rs in pool.map(one, chunks) for r in rs]
        return pool.map(one, pairs)
    finally:
        if own:
            pool.close()


def fit_frames(frames, n_components=100, max_iter=30, tol=1.0e-4, cov_type="diag", devices=None,
               contexts_per_device: int = 1, pool: ReplicaPool | None = None, batch: int = 1, voxel_size=None,
               flavour: str = "W"):
    """One flat GMM per frame (``GMM_GPU_Base(n_components, max_iter, tol, cov_type).fit(frame)``,
    gmm_waymo/src/gmm.py:65-84), the frames fanned out over the pool's contexts.  -> the fitted models in frame order.

    ``batch`` > 1: every context takes ``batch`` frames at a time through the SAME launches (``GMM_GPU_Base.fit_batch``: one
    fused launch per iteration for all of them) -- a scan-sized frame alone is a chain of small launches that leaves the
    chip idle.  The last chunk may be short.  With one context and a seeded RNG the models are bitwise those of
    ``batch=1``: the initial parameters are drawn frame by frame in frame order either way.  (With several contexts the
    worker threads share the host RNG, with or without ``batch``.)

    ``voxel_size``: the reference's pipeline -- every frame is voxel-down-sampled before it is fitted
    (run_gmm_static.py:28).  Each chunk of ``batch`` frames (``batch=1``: a chunk of one) is down-sampled on its context by
    one launch set (``voxel_down_sample_batch(chunk, voxel_size, download=False)``) and fitted COUNT-WEIGHTED through
    ``fit_batch`` where the centroids lie: a voxel counts as the raw points it stands for.  Only the initialiser's copy of
    the centroids comes back to the host.

    ``flavour="G"``: the GMMReg flavour's model instead (``gmmreg_gpu.gmm.GMM_GPU_Base(n_components, max_iter, tol)``: diag,
    KMeans initialisation); with ``batch`` > 1 its ``fit_batch`` runs the KMeans initialiser of the chunk's frames through
    one launch set as well, and the models are bitwise those of ``batch=1``.  It takes neither ``cov_type`` other than
    ``"diag"`` nor ``voxel_size``.

    ``flavour="full"``: the flat FULL-covariance fit (``hgmm.hgmm_gpu.fitFullCovGMM(frame, n_components, ls=tol,
    max_iters=max_iter)``; ``tol`` is its stop rule's ``ls`` on |q - q_prev|, the other parameters its defaults) -> one
    ``(pi, mu, cov)`` per frame.  ``batch`` > 1: ``fitFullCovGMM_batch`` of every chunk, four launches per iteration for
    all its frames, bitwise ``batch=1``.  ``voxel_size``: every chunk is down-sampled on its context and fitted
    count-weighted where the centroids lie (``batch=1``: chunks of one through the same route).  ``cov_type`` is not looked
    at."""
    if flavour == "full":
        return _fit_frames_full(list(frames), n_components, max_iter, tol, devices, contexts_per_device, pool, batch, voxel_size)
    if flavour == "G":
        from .gmmreg_gpu.gmm import GMM_GPU_Base as _G

        if cov_type != "diag" or voxel_size is not None:
            raise ValueError("fit_frames(flavour='G') takes cov_type='diag' and no voxel_size")

        def GMM_GPU_Base(n_components, max_iter, tol, cov_type):
            return _G(n_components, max_iter, tol)
    elif flavour == "W":
        from .gmm_waymo.gmm import GMM_GPU_Base
    else:
        raise ValueError("flavour must be 'W' or 'G' (or 'full'), not %r" % (flavour,))

    frames = list(frames)
    B = int(batch)
    if B < 1:
        raise ValueError("batch must be >= 1, not %r" % (batch,))

    def one(ctx, frame):                                     # (the worker thread runs under use_context(ctx))
        return GMM_GPU_Base(n_components, max_iter, tol, cov_type).fit(frame)

    def chunk(ctx, part):
        return GMM_GPU_Base(n_components, max_iter, tol, cov_type).fit_batch(part)

    def voxel_chunk(ctx, part):
        result = ctx.voxel_down_sample_batch(part, voxel_size, download=False)
        return GMM_GPU_Base(n_components, max_iter, tol, cov_type).fit_batch(result.members())

    own = pool is None
    pool = pool or ReplicaPool(devices, contexts_per_device)
    try:
        if B > 1 or voxel_size is not None:
            chunks = [frames[i:i + B] for i in range(0, len(frames), B)]
            return [m for ms in pool.map(chunk if voxel_size is None else voxel_chunk, chunks) for m in ms]
        return pool.map(one, frames)
    finally:
        if own:
            pool.close()


def _fit_frames_full(frames, n_components, max_iter, tol, devices, contexts_per_device, pool, batch, voxel_size):
    """fit_frames(flavour="full"): fitFullCovGMM per frame, or fitFullCovGMM_batch per chunk of ``batch`` frames"""
    from .hgmm.hgmm_gpu import fitFullCovGMM, fitFullCovGMM_batch
    B = int(batch)
    if B < 1:
        raise ValueError("batch must be >= 1, not %r" % (batch,))
    kw = dict(ls=tol, max_iters=max_iter)

    def one(ctx, frame):                                     # (the worker thread runs under use_context(ctx))
        if voxel_size is None:
            return fitFullCovGMM(frame, n_components, ctx=ctx, **kw)
        vc = ctx.voxel_down_sample_batch([frame], voxel_size, download=False).members()[0]
        return fitFullCovGMM(vc, n_components, ctx=ctx, **kw)

    def chunk(ctx, part):
        if voxel_size is not None:
            part = ctx.voxel_down_sample_batch(part, voxel_size, download=False).members()
        return fitFullCovGMM_batch(part, n_components, ctx=ctx, **kw)

    own = pool is None
    pool = pool or ReplicaPool(devices, contexts_per_device)
    try:
        if B > 1:
            chunks = [frames[i:i + B] for i in range(0, len(frames), B)]
            return [m for ms in pool.map(chunk, chunks) for m in ms]
        return pool.map(one, frames)
    finally:
        if own:
            pool.close()
