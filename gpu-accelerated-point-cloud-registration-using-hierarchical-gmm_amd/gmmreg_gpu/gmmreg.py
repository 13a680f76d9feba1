"""L2-distance GMM registration (GMMReg) -- drop-in for ``src/python/gmmreg_gpu/gmmreg.py``.

Both clouds are summarised by a mixture (fitted on the MI355X engine through ``gmm.GMM_GPU``, or by a
one-class SVM's support vectors for the SVR variant); a 7-parameter rigid transform is then found by BFGS on
the L2 distance between the two mixtures, the kernel width annealed between outer rounds.  The optimiser is
host SciPy as in the reference; the J_s x J_t Gauss transform behind every cost evaluation runs on the
device (``hgmm_gauss_transform``).

Layout of this module: the algorithm is three small functions -- :func:`cloud_scale` (the kernel width the
reference derives from the source covariance, gmmreg.py:48-52), :func:`summarise` (features of one cloud, with
the reference's 1e3 weight scaling, gmmreg.py:71-75, 84-89) and :func:`l2_register` (the annealed BFGS loop,
gmmreg.py:62-121) -- and the classes of the reference's API (``L2DistRegistration``, ``RigidGMMReg``,
``RigidSVR``, ``registration_gmmreg``, ``registration_svr``) are thin state holders over them.

No counterpart in the reference: the multi-start and the batch.  :func:`lockstep_solve` runs one unmodified
:func:`bfgs_round` per hypothesis in lock-step, all cost evaluations of a step served by ONE
``RigidCostFunction.evaluate_many`` over mixtures that stay on the device (``hgmm_l2_set_pairs`` / ``hgmm_l2_cost``);
``L2DistRegistration.optimise_multistart`` / ``registration_multistart``, ``registration_gmmreg(..., starts=)`` and
:func:`registration_gmmreg_batch` are built on it.  ``registration_gmmreg(...)`` without ``starts`` is what it was.
Each of them takes ``solver="device"`` (default "scipy"): the solves then run as ONE ``RigidCostFunction.solve_many`` -- the
whole BFGS loop of every hypothesis on the device (``hgmm_l2_solve``), no Python between two evaluations (:func:`solve_jobs`).
"""
import threading
import time

import numpy as np
from scipy.optimize import minimize

from . import cost_functions as cf
from . import gmm as ft

WEIGHT_SCALE = 1e3          # both mixtures' weights are multiplied by this before the optimiser sees them


def _points(x):
    return np.asarray(x.points if hasattr(x, "points") else x)


def cloud_scale(data):
    """(det of the sample covariance)^(1 / 2d): the initial kernel width."""
    data = np.asarray(data)
    count, dim = data.shape
    centred = data - data.mean(axis=0)
    return np.power(np.linalg.det(centred.T @ centred / (count - 1)), 1.0 / (2.0 * dim))


def summarise(feature_gen, cloud):
    """-> (centres[J,3] float64, weights[J] float64 x WEIGHT_SCALE) of one cloud."""
    centres, weights = feature_gen.compute(cloud)
    return np.asarray(centres, np.float64), np.asarray(weights, np.float64) * WEIGHT_SCALE


def bfgs_round(cost_fn, x0, source_mix, target_mix, sigma, maxiter, tol, on_step=None):
    """One BFGS solve on fixed mixtures at kernel width ``sigma``."""
    return minimize(cost_fn, x0, args=(*source_mix, *target_mix, sigma), method='BFGS', jac=True, tol=tol,
                    options={'maxiter': maxiter}, callback=on_step)


class _Abandoned(Exception):
    """Raised inside a solve whose answer will never come: another solve or the evaluator has failed."""


def lockstep_solve(evaluate_many, jobs, maxiter, tol):
    """Run one unmodified :func:`bfgs_round` per job, all in lock-step.  ``jobs`` is a sequence of ``(x0, pair_id, sigma)``;
    ``evaluate_many(thetas, pair_ids, sigmas) -> (f [R], grad [R, 7])`` is the only thing that evaluates a cost.

    Every solve runs on a thread of its own; its cost function hands theta to the dispatcher -- this thread, the only one
    that calls ``evaluate_many`` -- and waits.  The dispatcher waits until every solve that is still running has asked, then
    serves them all with ONE call, in job order.  So the number of calls is the largest ``nfev`` among the jobs, not the sum,
    and since row r of ``evaluate_many`` does not depend on the other rows each result is bit for bit the solve run alone.
    A solve that finishes simply stops asking.  An exception of the evaluator or of a solve abandons the other solves and is
    raised here, after every thread has been joined.  -> list of ``OptimizeResult``, one per job."""
    jobs = list(jobs)
    if not jobs:
        return []
    # Nobody is woken who has nothing to do: the dispatcher sleeps at `ready`, which the LAST solve to ask (or a solve that
    # ends while all others have asked) releases; solve k sleeps at gates[k], a lock the dispatcher opens when k's answer is
    # there.  (A condition variable shared by all would wake every sleeper at every arrival: R^2 wake-ups per step.)
    lock = threading.Lock()
    ready = threading.Semaphore(0)
    gates = [threading.Lock() for _ in jobs]
    for gate in gates:
        gate.acquire()
    pending, answers, results = {}, {}, [None] * len(jobs)
    state = {"running": len(jobs), "failure": None}

    def open_gate(gate):
        try:
            gate.release()
        except RuntimeError:                                 # (open already)
            pass

    def solve(k, x0, sigma):
        def cost(theta, _sigma):
            with lock:
                if state["failure"] is not None:
                    raise _Abandoned()
                pending[k] = np.array(theta, dtype=np.float64)
                if len(pending) >= state["running"]:
                    ready.release()
            gates[k].acquire()
            with lock:
                if k not in answers:                         # (the gate was opened by a failure, not by an answer)
                    raise _Abandoned()
                return answers.pop(k)
        try:
            results[k] = bfgs_round(cost, x0, (), (), sigma, maxiter, tol)
        except _Abandoned:
            pass
        except BaseException as exc:                         # (the solve's own failure: it reaches the caller)
            with lock:
                if state["failure"] is None:
                    state["failure"] = exc
        finally:
            with lock:
                state["running"] -= 1
                if state["failure"] is not None or len(pending) >= state["running"]:
                    ready.release()

    threads = [threading.Thread(target=solve, args=(k, np.asarray(x0, dtype=np.float64), sigma), daemon=True)
               for k, (x0, _, sigma) in enumerate(jobs)]
    for th in threads:
        th.start()
    try:
        while True:
            ready.acquire()
            with lock:
                if state["failure"] is not None or state["running"] == 0:
                    break
                if len(pending) < state["running"]:          # (a wake-up whose step has been served already)
                    continue
                asked = sorted(pending)
                thetas = [pending.pop(k) for k in asked]
            try:
                f, grad = evaluate_many(thetas, [jobs[k][1] for k in asked], [jobs[k][2] for k in asked])
            except BaseException as exc:
                with lock:
                    state["failure"] = exc
                break
            with lock:
                for r, k in enumerate(asked):
                    answers[k] = (float(f[r]), np.array(grad[r], dtype=np.float64))
            for k in asked:
                open_gate(gates[k])
    finally:
        with lock:
            if state["running"] and state["failure"] is None:    # (this thread itself was interrupted)
                state["failure"] = _Abandoned()
        for gate in gates:                                   # whoever still sleeps finds no answer and gives up
            open_gate(gate)
        for th in threads:
            th.join()
    if state["failure"] is not None:
        raise state["failure"]
    return results


def solve_jobs(cost_fn, jobs, maxiter, tol, solver="scipy"):
    """The solves of ``jobs`` (``(x0, pair_id, sigma)`` on the mixtures of ``cost_fn.set_pairs``) -> list of ``OptimizeResult``.
    ``solver="scipy"``: :func:`lockstep_solve` over ``cost_fn.evaluate_many``, SciPy's own BFGS per job.  ``solver="device"``:
    ONE ``cost_fn.solve_many`` -- the whole solve of every job on the device (``hgmm_l2_solve``), SciPy's BFGS restated there
    with one deliberate difference: a failed dcsrch line search ends the solve at once (status 2) where SciPy would try a
    second one first."""
    jobs = list(jobs)
    if solver == "scipy":
        return lockstep_solve(cost_fn.evaluate_many, jobs, maxiter, tol)
    if solver != "device":
        raise ValueError("solver = %r (expected 'scipy' or 'device')" % (solver,))
    if not jobs:
        return []
    return cost_fn.solve_many([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], maxiter, tol)


def _start_thetas(starts):
    """Start poses -> list of theta: a ``RigidTransformation`` goes through ``theta_from_transformation``, a 7-vector is
    taken as it is.  An empty list is refused."""
    starts = list(starts) if starts is not None else []
    if not starts:
        raise ValueError("multi-start needs at least one start pose (starts is empty)")
    return [cf.theta_from_transformation(s) if hasattr(s, "rot") else np.asarray(s, dtype=np.float64).reshape(7)
            for s in starts]


def _lowest(funs):
    """Index of the lowest final cost; ties go to the lowest index."""
    return min(range(len(funs)), key=lambda k: (funs[k] if funs[k] == funs[k] else np.inf, k))     # (a NaN cost never wins)


def l2_register(state, target, maxiter, tol, opt_maxiter, opt_tol):
    """The outer loop: re-summarise the source, solve, anneal, until the cost stops moving.
    ``state`` is the registration object (it owns sigma, the feature generator and the callbacks)."""
    state._feature_gen.init()
    target_mix = summarise(state._feature_gen, target)
    x = state._cost_fn.initial()
    previous = None
    for _ in range(maxiter):
        source_mix = summarise(state._feature_gen, state._source)
        res = bfgs_round(state._cost_fn, x, source_mix, target_mix, state._sigma, opt_maxiter, opt_tol,
                         state.optimization_cb)
        state._annealing()
        state._feature_gen.annealing()
        x = res.x
        if previous is not None and abs(res.fun - previous) < tol:
            break
        previous = res.fun
    return state._cost_fn.to_transformation(x)


class L2DistRegistration(object):
    """reference gmmreg.py:14-121 (same constructor, attributes and methods)."""

    def __init__(self, source, feature_gen, cost_fn, sigma=1.0, delta=0.9, use_estimated_sigma=True,
                 verbose=False):
        self._feature_gen, self._cost_fn = feature_gen, cost_fn
        self._sigma, self._delta = sigma, delta
        self._use_estimated_sigma = use_estimated_sigma
        self._callbacks = []
        self._verbose = verbose
        self._source = None
        if source is not None:
            self.set_source(source)

    def set_source(self, source):
        self._source = source
        if self._use_estimated_sigma:
            self._estimate_sigma(source)

    def set_callbacks(self, callbacks):
        self._callbacks.extend(callbacks)

    def _estimate_sigma(self, data):
        self._sigma = cloud_scale(data)
        if self._verbose:
            print("Estimated Sigma: ", self._sigma)

    def _annealing(self):
        self._sigma *= self._delta

    def optimization_cb(self, x):
        if self._callbacks:
            tf_result = self._cost_fn.to_transformation(x)
            for c in self._callbacks:
                c(tf_result)

    def optimise(self, mu_source, phi_source, mu_target, phi_target, x_ini, opt_maxiter=10, opt_tol=1.0e-5):
        """One BFGS solve on given mixtures (the inner step of :meth:`registration`)."""
        return bfgs_round(self._cost_fn, x_ini, (mu_source, phi_source), (mu_target, phi_target), self._sigma,
                          opt_maxiter, opt_tol, self.optimization_cb)

    def registration(self, target, maxiter=1, tol=1.0e-3, opt_maxiter=10, opt_tol=1.0e-5):
        t0 = time.time()
        out = l2_register(self, target, maxiter, tol, opt_maxiter, opt_tol)
        if self._verbose:
            print("Overall Time taken: ", time.time() - t0)
        return out

    def optimise_multistart(self, mu_source, phi_source, mu_target, phi_target, starts, opt_maxiter=10, opt_tol=1.0e-5,
                            solver="scipy"):
        """:meth:`optimise` from every pose of ``starts`` (``RigidTransformation`` objects or 7-vectors), all solves in
        lock-step (:func:`lockstep_solve`): one ``evaluate_many`` of the cost function serves every solve that is still
        running.  -> list of ``OptimizeResult``, each the solve from that start run alone.  The per-step callbacks of
        :meth:`optimise` are not called: the solves do not run one after the other.  ``solver="device"``: the solves run on
        the device instead (:func:`solve_jobs`)."""
        thetas = _start_thetas(starts)
        self._cost_fn.set_pairs([(mu_source, phi_source, mu_target, phi_target)])
        res = solve_jobs(self._cost_fn, [(x0, 0, self._sigma) for x0 in thetas], opt_maxiter, opt_tol, solver)
        self.best_index_ = _lowest([float(r.fun) for r in res])
        return res

    def registration_multistart(self, target, starts, maxiter=1, tol=1.0e-3, opt_maxiter=10, opt_tol=1.0e-5,
                                return_all=False, solver="scipy"):
        """:meth:`registration` from every pose of ``starts`` at once.  The outer rounds are those of :func:`l2_register`:
        per round the source is summarised ONCE for all starts and the kernel width is annealed ONCE; a start stops when its
        own cost moved by less than ``tol`` between two rounds.  The winner is the start with the lowest final cost (ties:
        the lowest index); ``best_index_`` names it and its ``RigidTransformation`` is returned -- with ``return_all=True``,
        ``(winner, [transformation of every start], [final cost of every start])``.  ``solver``: :func:`solve_jobs`."""
        thetas = _start_thetas(starts)
        self._feature_gen.init()
        target_mix = summarise(self._feature_gen, target)
        K = len(thetas)
        funs, previous, running = [np.inf] * K, [None] * K, list(range(K))
        for _ in range(maxiter):
            source_mix = summarise(self._feature_gen, self._source)
            self._cost_fn.set_pairs([(*source_mix, *target_mix)])
            res = solve_jobs(self._cost_fn, [(thetas[k], 0, self._sigma) for k in running], opt_maxiter, opt_tol, solver)
            self._annealing()
            self._feature_gen.annealing()
            still = []
            for k, r in zip(running, res):
                thetas[k], funs[k] = r.x, float(r.fun)
                if previous[k] is None or not abs(funs[k] - previous[k]) < tol:
                    still.append(k)
                previous[k] = funs[k]
            running = still
            if not running:
                break
        self.best_index_ = _lowest(funs)
        tfs = [self._cost_fn.to_transformation(x) for x in thetas]
        return (tfs[self.best_index_], tfs, funs) if return_all else tfs[self.best_index_]


def _default_cost(ctx):
    from .._native import default_context
    return cf.RigidCostFunction(ctx=ctx or default_context())


class RigidGMMReg(L2DistRegistration):
    """reference gmmreg.py:138-147: GMM_GPU features (10 EM iterations), at most 0.8 N components."""

    def __init__(self, source, sigma=1.0, delta=0.9, n_gmm_components=50, use_estimated_sigma=True,
                 verbose=False, ctx=None):
        k = min(n_gmm_components, int(source.shape[0] * 0.8))
        super().__init__(source, ft.GMM_GPU(k, max_iter=10), _default_cost(ctx), sigma, delta, use_estimated_sigma,
                         verbose)


class RigidSVR(L2DistRegistration):
    """reference gmmreg.py:123-136: the clouds are summarised by the support vectors of a one-class SVM
    (third-party estimator, scikit-learn on the host) instead of a GMM; cost, gradient and Gauss transform are
    the same device path as RigidGMMReg.  The SVM's RBF width follows the kernel width."""

    def __init__(self, source, sigma=1.0, delta=0.9, gamma=0.5, nu=0.1, use_estimated_sigma=True,
                 verbose=False, ctx=None):
        super().__init__(source, ft.OneClassSVM(source.shape[1], sigma, gamma, nu), _default_cost(ctx), sigma, delta,
                         use_estimated_sigma, verbose)

    def _estimate_sigma(self, data):
        super()._estimate_sigma(data)
        self._feature_gen._sigma = self._sigma
        self._feature_gen._gamma = 1.0 / (2.0 * np.square(self._sigma))


def _run(kind, source, target, tf_type_name, callbacks, reg_args, kargs):
    if tf_type_name != 'rigid':
        raise ValueError('Unknown transform type %s' % tf_type_name)
    reg = kind(_points(source), **kargs)
    reg.set_callbacks(callbacks)
    return reg.registration(_points(target), *reg_args)


def registration_gmmreg(source, target, tf_type_name='rigid', callbacks=[], starts=None, solver="scipy", **kargs):
    """reference gmmreg.py:149-157: returns the RigidTransformation mapping source onto target.

    ``starts`` (no counterpart in the reference; default None: the reference's single solve from the identity): a list
    of start poses -- the result is ``RigidGMMReg.registration_multistart``'s winner.  ``solver`` ("scipy", the default, or
    "device": :func:`solve_jobs`): with "device" the solves run on the device; without ``starts`` that is the one solve from
    the identity.  Without ``starts`` and with the default solver this is the reference's path, as it was."""
    if solver not in ("scipy", "device"):
        raise ValueError("solver = %r (expected 'scipy' or 'device')" % (solver,))
    if starts is None and solver == "scipy":
        return _run(RigidGMMReg, source, target, tf_type_name, callbacks, (), kargs)
    if tf_type_name != 'rigid':
        raise ValueError('Unknown transform type %s' % tf_type_name)
    reg = RigidGMMReg(_points(source), **kargs)
    reg.set_callbacks(callbacks)
    if starts is None:
        starts = [reg._cost_fn.initial()]
    return reg.registration_multistart(_points(target), starts, solver=solver)


def registration_gmmreg_batch(pairs, starts=None, ctx=None, maxiter=1, solver="scipy", **kargs):
    """``registration_gmmreg(source, target, **kargs)`` for every ``(source, target)`` of ``pairs`` through one launch set
    per stage.  The 2B mixtures are fitted by ONE ``fit_batch`` in the order t0, s0, t1, s1, ... -- the order in which a
    loop of ``registration_gmmreg`` draws from NumPy's random stream; if the pairs' component counts differ (a small cloud
    caps its own at 0.8 N) the fits run one by one in that same order.  All pairs' mixtures then become resident with one
    ``set_pairs`` and every pair's solve (with ``starts``: every start of every pair) runs in lock-step
    (:func:`lockstep_solve`), each at its own pair's kernel width -- with ``solver="device"`` in ONE ``solve_many`` on the device
    (:func:`solve_jobs`).

    Only the single outer round ``registration_gmmreg`` uses is offered: ``maxiter`` other than 1 is refused.
    -> list of ``RigidTransformation``; with ``starts``, ``(list, winners' indices)``."""
    if solver not in ("scipy", "device"):
        raise ValueError("solver = %r (expected 'scipy' or 'device')" % (solver,))
    if maxiter != 1:
        raise ValueError("registration_gmmreg_batch: outer maxiter = %r is not supported (only maxiter = 1, which is "
                         "what registration_gmmreg uses); register the pairs one by one" % (maxiter,))
    pairs = [(_points(s), _points(t)) for s, t in pairs]
    thetas = None if starts is None else _start_thetas(starts)
    if not pairs:
        return [] if starts is None else ([], [])
    cost = _default_cost(ctx)
    regs = [RigidGMMReg(s, ctx=ctx, **kargs) for s, _ in pairs]
    for reg in regs:
        reg._cost_fn = cost
        reg._feature_gen.init()
    if len({reg._feature_gen._clf.num_components for reg in regs}) == 1:
        fits = regs[0]._feature_gen._clf.fit_batch([cloud for s, t in pairs for cloud in (t, s)])
        mixes = [(np.asarray(m.means_, np.float64), np.asarray(m.weights_, np.float64) * WEIGHT_SCALE) for m in fits]
    else:
        mixes = [summarise(reg._feature_gen, cloud) for reg, (s, t) in zip(regs, pairs) for cloud in (t, s)]
    cost.set_pairs([(*mixes[2 * b + 1], *mixes[2 * b]) for b in range(len(pairs))])
    if thetas is None:
        thetas = [cost.initial()]
    K = len(thetas)
    # (opt_maxiter = 10, opt_tol = 1e-5: the defaults of L2DistRegistration.registration, which registration_gmmreg runs with)
    res = solve_jobs(cost, [(x0, b, reg._sigma) for b, reg in enumerate(regs) for x0 in thetas], 10, 1.0e-5, solver)
    tfs, winners = [], []
    for b in range(len(regs)):
        mine = res[b * K:(b + 1) * K]
        winners.append(_lowest([float(r.fun) for r in mine]))
        tfs.append(cost.to_transformation(mine[winners[-1]].x))
    return tfs if starts is None else (tfs, winners)


def registration_svr(source, target, tf_type_name='rigid', maxiter=1, tol=1.0e-3, opt_maxiter=50,
                     opt_tol=1.0e-3, callbacks=[], **kargs):
    """reference gmmreg.py:159-169."""
    return _run(RigidSVR, source, target, tf_type_name, callbacks, (maxiter, tol, opt_maxiter, opt_tol), kargs)
