"""L2 distance between two Gaussian mixtures and its rigid (quaternion + translation) cost
(drop-in for ``src/python/gmmreg_gpu/cost_functions.py``: ``compute_l2_dist``, ``RigidCostFunction``).

With both mixtures isotropic of width sigma, the cross term of the L2 distance is a Gauss transform of width
sqrt(2) sigma: f = -sum_s phi_s G(mu_s), G(x) = sum_t (phi_t / z) exp(-|x - mu_t|^2 / 2 sigma^2); its gradient
with respect to the source centres needs the same kernel against the weight rows phi_t mu_t / z.  Both come out
of ONE kernel matrix here (the reference evaluates it 1 + 3 times, cost_functions.py:29-40); with a device
context it is `hgmm_gauss_transform`.  The 7-parameter chain rule stays in NumPy.
``RigidCostFunction.evaluate_many`` evaluates R hypotheses at once over mixtures that stay resident on the device
(`hgmm_l2_set_pairs` / `hgmm_l2_cost`: the fused kernel returns f, the column sums of the gradient and g.T @ mu_source);
``__call__`` is the path it always was.  ``RigidCostFunction.solve_many`` runs the whole BFGS solve of R hypotheses on the
device (`hgmm_l2_solve`): chain rule, line search and inverse-Hessian update included, no Python between two evaluations.
"""
import numpy as np

from . import so
from . import transforms as tf


def compute_l2_dist(mu_source, phi_source, mu_target, phi_target, sigma, ctx=None):
    """-> (f, df/dmu_source [J_s, 3]).  ``ctx``: evaluate the Gauss transform on that device context."""
    dim = mu_source.shape[1]
    z = np.power(2.0 * np.pi * sigma ** 2, dim * 0.5)
    rows = np.vstack([phi_target, phi_target * mu_target.T]) / z           # [1 + dim, J_t]
    sums = tf.GaussTransform(mu_target, np.sqrt(2.0) * sigma, ctx=ctx).compute(mu_source, rows)
    g0, g1 = sums[0], sums[1:]                                             # sum_t w e  and  sum_t w mu_t e
    grad = (phi_source * (g0 * mu_source.T - g1)).T / (2.0 * sigma ** 2)
    return -(phi_source @ g0), grad


def theta_from_transformation(tf_obj):
    """RigidTransformation -> theta = (qw, qx, qy, qz, tx, ty, tz), the inverse of ``RigidCostFunction.to_transformation``
    for a proper rotation.  The quaternion comes from Shepperd's method -- the largest of (trace, R00, R11, R22) decides
    which component is taken from a square root, so nothing is divided by a small number, also at a turn of 180 degrees --
    is of unit length and has w >= 0."""
    r = np.asarray(tf_obj.rot, dtype=np.float64)
    tr = np.trace(r)
    k = int(np.argmax([tr, r[0, 0], r[1, 1], r[2, 2]]))
    if k == 0:                         # s = 4 q_k in every branch; the other three components are off-diagonal sums / s
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [0.25 * s, (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s]
    elif k == 1:
        s = 2.0 * np.sqrt(1.0 + r[0, 0] - r[1, 1] - r[2, 2])
        q = [(r[2, 1] - r[1, 2]) / s, 0.25 * s, (r[0, 1] + r[1, 0]) / s, (r[0, 2] + r[2, 0]) / s]
    elif k == 2:
        s = 2.0 * np.sqrt(1.0 + r[1, 1] - r[0, 0] - r[2, 2])
        q = [(r[0, 2] - r[2, 0]) / s, (r[0, 1] + r[1, 0]) / s, 0.25 * s, (r[1, 2] + r[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + r[2, 2] - r[0, 0] - r[1, 1])
        q = [(r[1, 0] - r[0, 1]) / s, (r[0, 2] + r[2, 0]) / s, (r[1, 2] + r[2, 1]) / s, 0.25 * s]
    q = np.array(q, dtype=np.float64)
    if q[0] < 0.0:
        q = -q
    q[0] = abs(q[0])                   # (-0.0 at a half turn)
    return np.concatenate([q, np.asarray(tf_obj.t, dtype=np.float64).reshape(3)])


class CostFunction(object):
    """Interface BFGS drives: ``initial()`` -> theta0, ``__call__(theta, *mixtures)`` -> (f, grad),
    ``to_transformation(theta)`` (cost_functions.py:11-26)."""

    def __init__(self, tf_type):
        self._tf_type = tf_type

    def to_transformation(self, theta):
        raise NotImplementedError

    def initial(self):
        raise NotImplementedError

    def __call__(self, theta, *args):
        raise NotImplementedError


class RigidCostFunction(CostFunction):
    """theta = (qw, qx, qy, qz, tx, ty, tz)   (cost_functions.py:43-68)."""

    def __init__(self, ctx=None):
        super().__init__(tf.RigidTransformation)
        self._ctx = ctx                     # device context for the Gauss transform (None: host NumPy)
        self._pairs = None                  # set_pairs: the mixtures evaluate_many works on
        self._resident = None               # ... and the token the context carries while THEY are its resident set

    def to_transformation(self, theta):
        return self._tf_type(so.quaternion_matrix(theta[:4])[:3, :3], theta[4:7])

    def initial(self):
        return np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])

    def __call__(self, theta, *args):
        mu_source, phi_source, mu_target, phi_target, sigma = args
        moved = self.to_transformation(theta).transform(mu_source)
        f, g = compute_l2_dist(moved, phi_source, mu_target, phi_target, sigma, ctx=self._ctx)
        # d f / d q_k = sum_{a,b} (g^T mu_source)[a, b] dR[a, b] / d q_k ;  d f / d t = column sums of g
        d_quat = np.einsum('ab,kab->k', g.T @ mu_source, so.diff_rot_from_quaternion(theta[:4]))
        return f, np.concatenate([d_quat, g.sum(axis=0)])

    # ---- many hypotheses over resident mixtures -------------------------------------------------------------------
    def set_pairs(self, pairs):
        """The mixtures :meth:`evaluate_many` works on: a sequence of ``(mu_source, phi_source, mu_target, phi_target)``.
        With a context they become resident on the device (``Context.l2_set_pairs``); a later call replaces them."""
        self._pairs = [tuple(np.asarray(a, dtype=np.float64) for a in p) for p in pairs]
        self._make_resident()

    def _make_resident(self):
        # a context holds ONE resident set: a cost function that finds another's there (two registrations sharing the
        # default context) puts its own back instead of evaluating on the wrong mixtures
        if self._ctx is not None:
            self._ctx.l2_set_pairs(self._pairs)          # (clears the context's token)
            self._resident = self._ctx.l2_owner = object()

    def evaluate_many(self, thetas, pair_ids, sigmas):
        """R hypotheses at once -> (f [R], grad [R, 7]): hypothesis r is theta ``thetas[r]`` on pair ``pair_ids[r]`` of
        :meth:`set_pairs` at kernel width ``sigmas[r]``.  With a context one ``l2_cost`` call evaluates them all (the fused
        kernel returns f, the column sums of g and g.T @ mu_source; the chain rule below is that of ``__call__``); without,
        a loop of ``__call__``.  Row r does not depend on R or on the other rows."""
        thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, 7)
        R = len(thetas)
        pair_ids = np.broadcast_to(np.asarray(pair_ids, dtype=np.int64), (R,))
        sigmas = np.broadcast_to(np.asarray(sigmas, dtype=np.float64), (R,))
        pairs = self._pairs
        if not pairs:
            raise ValueError("evaluate_many: no mixtures (call set_pairs first)")
        f, grad = np.empty(R), np.empty((R, 7))
        if self._ctx is None:
            for r in range(R):
                f[r], grad[r] = self(thetas[r], *pairs[int(pair_ids[r])], float(sigmas[r]))
            return f, grad
        if self._ctx.l2_owner is not self._resident:
            self._make_resident()
        poses = [self.to_transformation(th) for th in thetas]
        out = self._ctx.l2_cost(pair_ids, [p.rot for p in poses], [p.t for p in poses], sigmas)
        f[:] = out[:, 0]
        grad[:, 4:] = out[:, 1:4]
        for r in range(R):
            grad[r, :4] = np.einsum('ab,kab->k', out[r, 4:].reshape(3, 3), so.diff_rot_from_quaternion(thetas[r, :4]))
        return f, grad

    SOLVE_MESSAGES = ("Optimization terminated successfully.", "Maximum number of iterations has been exceeded.",
                      "Desired error not necessarily achieved due to precision loss.", "NaN result encountered.")

    def solve_many(self, thetas, pair_ids, sigmas, maxiter=10, tol=1.0e-5):
        """The whole BFGS solve of R hypotheses on the device, in lock-step (``Context.l2_solve`` / ``hgmm_l2_solve``):
        hypothesis r starts at ``thetas[r]`` on pair ``pair_ids[r]`` of :meth:`set_pairs` at kernel width ``sigmas[r]``;
        ``maxiter`` and ``tol`` are what ``gmmreg.bfgs_round`` hands SciPy.  -> list of ``OptimizeResult`` with ``x, fun, jac,
        nit, nfev, status, success, message``, each the solve of that hypothesis run alone.

        The optimiser is SciPy's BFGS with its first line search (dcsrch), restated on the device.  One deliberate
        difference: where SciPy tries a second line search after dcsrch has failed, the solve ends at once with status 2
        ("precision loss") at the last accepted iterate -- ``nfev`` differs from SciPy's by design, ``x, fun, nit, status`` are
        what compare.  Needs a context: this project has no CPU fallback."""
        from scipy.optimize import OptimizeResult
        thetas = np.asarray(thetas, dtype=np.float64).reshape(-1, 7)
        R = len(thetas)
        pair_ids = np.broadcast_to(np.asarray(pair_ids, dtype=np.int64), (R,))
        sigmas = np.broadcast_to(np.asarray(sigmas, dtype=np.float64), (R,))
        if not self._pairs:
            raise ValueError("solve_many: no mixtures (call set_pairs first)")
        if self._ctx is None:
            raise RuntimeError("solve_many: the device solve needs a context (there is no CPU fallback)")
        if self._ctx.l2_owner is not self._resident:
            self._make_resident()
        x, f, grad, nit, nfev, status = self._ctx.l2_solve(pair_ids, thetas, sigmas, maxiter, tol)
        return [OptimizeResult(x=x[r].copy(), fun=float(f[r]), jac=grad[r].copy(), nit=int(nit[r]), nfev=int(nfev[r]),
                               status=int(status[r]), success=bool(status[r] == 0), message=self.SOLVE_MESSAGES[int(status[r])])
                for r in range(R)]
