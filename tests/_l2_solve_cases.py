"""What the CPU and the GPU tests of the device L2 solve share: the host evaluator the model is given on a CPU, SciPy's own
solve with its cost outputs perturbed by an ulp (the yardstick of ``x`` and ``f``), the 28 solves of the multi-start scenario
and the golden case of tests/test_gmmreg_gpu.py."""
import numpy as np

from conftest import load_golden
import l2_scenario as l2s

X_FLOOR, F_FLOOR = 2e-10, 1e-11          # 10 x the largest SciPy spread among the starts that end with status 2
SEEDS = (1, 2, 3)


def host_evaluator(pairs):
    """evaluate(pose, pair, sigma) -> 13 numbers from the host NumPy cost (``compute_l2_dist`` without a context)."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, transforms as tf

    def evaluate(pose, pair, sigma):
        mu_s, phi_s, mu_t, phi_t = pairs[pair]
        moved = tf.RigidTransformation(np.array(pose[0]).reshape(3, 3), np.array(pose[1])).transform(mu_s)
        f, g = cf.compute_l2_dist(moved, phi_s, mu_t, phi_t, sigma)
        return np.concatenate([[f], g.sum(axis=0), (g.T @ mu_s).ravel()])
    return evaluate


def scipy_solve(x0, pair, sigma, maxiter, tol, seed=None):
    """The reference's optimiser call (``gmmreg.bfgs_round``) on the host cost; ``seed``: every cost output (f and the seven
    of the gradient) multiplied by 1 + 2.2e-16 u, u uniform in [-1, 1]."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, gmmreg
    cost = cf.RigidCostFunction()
    if seed is None:
        fn = cost
    else:
        rs = np.random.RandomState(seed)

        def fn(theta, *args):
            f, g = cost(theta, *args)
            u = rs.uniform(-1.0, 1.0, 8)
            return f * (1.0 + 2.2e-16 * u[0]), g * (1.0 + 2.2e-16 * u[1:])
    return gmmreg.bfgs_round(fn, np.asarray(x0, dtype=np.float64), pair[:2], pair[2:], sigma, maxiter, tol)


def spread(x0, pair, sigma, maxiter, tol, base):
    """-> (largest |x - base.x|, largest |f - base.fun| / |base.fun|) over SciPy's perturbed solves."""
    dx = df = 0.0
    for seed in SEEDS:
        r = scipy_solve(x0, pair, sigma, maxiter, tol, seed)
        dx = max(dx, float(np.abs(r.x - base.x).max()))
        df = max(df, abs(float(r.fun) - float(base.fun)) / abs(float(base.fun)))
    return dx, df


def scenario_jobs():
    """-> (scenario, pair, [theta0] * 28): the 27 starts of rotation_starts((-60, 0, 60)), then the identity."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    sc = l2s.scenario()
    pair = (sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"])
    thetas = [cf.theta_from_transformation(s) for s in sc["starts"]] + [cf.RigidCostFunction().initial()]
    return sc, pair, thetas


def golden_case():
    """-> (golden, pair, sigma): the reference's own mixtures and the kernel width tests/test_gmmreg_gpu.py solves them at."""
    from hgmm_amd.gmmreg_gpu import gmmreg
    g = load_golden("gmmreg_l2.npz")
    pair = (g["reg_mu_source"].astype(np.float64), g["reg_phi_source"] * 1e3,
            g["reg_mu_target"].astype(np.float64), g["reg_phi_target"] * 1e3)
    return g, pair, float(gmmreg.cloud_scale(g["reg_source"]))


def golden_allowance(pair, sigma):
    """The pose tolerance on the golden case: 1e-7 (tests/test_gmmreg_gpu.py:59-60) provided 10 x SciPy's own +-1-ulp spread
    of the pose stays below it; that spread x 10 otherwise.  -> (allowance, 10 x spread)."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    cost = cf.RigidCostFunction()
    base = scipy_solve(cost.initial(), pair, sigma, 10, 1.0e-5)
    tb = cost.to_transformation(base.x)
    worst = 0.0
    for seed in SEEDS:
        tp = cost.to_transformation(scipy_solve(cost.initial(), pair, sigma, 10, 1.0e-5, seed).x)
        worst = max(worst, float(np.abs(tp.rot - tb.rot).max()), float(np.abs(tp.t - tb.t).max()))
    return (1e-7 if 10.0 * worst < 1e-7 else 10.0 * worst), 10.0 * worst
