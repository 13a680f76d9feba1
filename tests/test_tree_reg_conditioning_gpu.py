"""The conditioning verdict of a registration iteration, on the host path and with the solve on the device
(reg_device_solve), against the float64 oracle's eigenvalues.

reg_host_step and reg_device_step (csrc/tree_device.h) hand an iteration to the stacked least squares -- status 2, nothing
updated -- where lambda_min <= 1e-11 lambda_max of the 6 x 6 normal equations; both ask reg_well_conditioned.  The ladder
of tree_reg_conditioning_scene.py (256 points, 8 nodes) has three rungs a decade or more above the rule and three a decade
or more below it (tests/test_tree_reg_conditioning_cpu.py holds them there), and on the rungs delta = 1e-6, 1e-7 and 3e-8
the Cholesky pivots look harmless (pivot ratio 9e-7 to 8e-10): a device step that judged by its pivots went on there,
solved a system of condition 1e12 to 1e15 and composed whatever came out.

The library builds A^T A from 64-bit fixed-point moments (a relative 2^-53 or so at this scale) and the oracle from
float64 sums; a verdict could differ between them only within rounding of the rule, and no rung is within a decade of it."""
import numpy as np
import pytest

from test_tree_multistart_gpu import assert_multi_is_serial
from test_tree_reg_depth_gpu import U, cholesky_gap, ctx  # noqa: F401
from tree_reg_conditioning_scene import (COND_RULE, I3, L, LADDER, LC, Z3, eig_ratio, hands_over, oracle_system, rot_z,
                                         scene)

pytestmark = pytest.mark.gpu

BUDGET = 4


@pytest.fixture(scope="module")
def rungs():
    """delta -> (pi, mu, cov, target, whether the oracle hands the first iteration over), computed once"""
    return {d: scene(d) + (hands_over(d),) for d in LADDER}


def load(ctx, pi, mu, cov, target):
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(target)


@pytest.mark.parametrize("device_solve", [0, 1])
@pytest.mark.parametrize("delta", LADDER)
def test_register_verdict_is_the_oracles(ctx, rungs, delta, device_solve):
    pi, mu, cov, target, over = rungs[delta]
    load(ctx, pi, mu, cov, target)
    q_in = 0.125                                             # (a previous q, to see that a hand-over leaves it alone)
    with ctx.config(reg_device_solve=device_solve):
        rot, t, done, q, status, trace = ctx.tree_register(I3, Z3, 1.0, LC, BUDGET, 0.0, q_in, want_trace=True)
    print("delta %g, reg_device_solve %d: status %d after %d iterations" % (delta, device_solve, status, done))
    if over:
        assert (status, done) == (2, 0)
        assert np.array_equal(rot, I3) and np.array_equal(t, Z3) and q == q_in and trace.shape == (0, 13)
        return
    assert done >= 1 and trace.shape == (done, 13)
    assert np.array_equal(trace[-1, :9].reshape(3, 3), rot) and np.array_equal(trace[-1, 9:12], t) and trace[-1, 12] == q
    if status == 2:
        # a later iteration was handed over: then the oracle's system at that pose is not clearly above the rule
        r = eig_ratio(oracle_system(pi, mu, cov, target, rot, t)[1])
        assert done < BUDGET and r < 10 * COND_RULE, (done, r)
    else:
        assert (status, done) == (0, BUDGET)                 # (tol 0 never stops)


@pytest.mark.parametrize("device_solve", [0, 1])
@pytest.mark.parametrize("delta", LADDER)
def test_multi_verdicts_are_the_serial_calls(ctx, rungs, delta, device_solve):
    """K = 3 start poses (the identity, +-0.5 degrees about z): every hypothesis is its own serial call bit for bit, status
    included; the identity's first verdict is the oracle's."""
    pi, mu, cov, target, over = rungs[delta]
    load(ctx, pi, mu, cov, target)
    rot0 = np.stack([I3, rot_z(0.5), rot_z(-0.5)])
    t0 = np.zeros((3, 3))
    with ctx.config(reg_device_solve=device_solve):
        _, _, iters, _, status, _ = assert_multi_is_serial(ctx, rot0, t0, LC, BUDGET, 0.0,
                                                           "delta %g, reg_device_solve %d" % (delta, device_solve))
    print("delta %g, reg_device_solve %d: status %s after %s iterations" % (delta, device_solve, status.tolist(), iters.tolist()))
    assert ((status[0] == 2 and iters[0] == 0) if over else iters[0] >= 1), (status.tolist(), iters.tolist())
    for k in (1, 2):                                         # the other starts: the oracle's verdict at their own pose
        r = eig_ratio(oracle_system(pi, mu, cov, target, rot0[k], t0[k])[1])
        if r <= COND_RULE / 10:
            assert status[k] == 2 and iters[k] == 0, (k, r)
        elif r >= COND_RULE * 10:
            assert iters[k] >= 1, (k, r)


def gmmtree_result(ctx, pi, mu, cov, target, solve_on_device):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    gt = GMMTree(None, tree_level=L, lambda_c=LC, ctx=ctx, solve_on_device=solve_on_device)
    gt.set_nodes(pi, mu, cov)
    res = gt.registration(target, BUDGET, 0.0)
    return res.transformation.rot, res.transformation.t, np.ravel(res.q), int(gt.n_iter_)


@pytest.mark.parametrize("delta", LADDER)
def test_gmmtree_with_the_solve_on_the_device(ctx, rungs, delta):
    """GMMTree(..., solve_on_device=True).registration against solve_on_device=False.  Where the first iteration is handed
    over, both run the Python stacked least squares on the same E-step from iteration 0: bit for bit.  Where it is not, the
    device's Cholesky solve against the host's elimination on the same normal equations, per iteration within the bound
    the device loop is held to against the oracle in test_tree_reg_depth_gpu.py,

        1e-9 + cond(A^T A) u |x|  (solution_tolerance)  +  8 * 6 * cond(A^T A) * 2^-52 * |x|  (cholesky_gap),

    with cond and x (the twist; |.| the max norm) the oracle's at the start pose.  The later iterations of this scene move
    less -- the first recovers the motion to first order -- so BUDGET times the first bound holds the final pose; the
    translation of the returned inverse, -R^T t, moves by |dR| |t| + |dt|."""
    pi, mu, cov, target, over = rungs[delta]
    dev = gmmtree_result(ctx, pi, mu, cov, target, True)
    host = gmmtree_result(ctx, pi, mu, cov, target, False)
    assert dev[3] == host[3] == BUDGET
    if over:
        for a, b in zip(dev[:3], host[:3]):
            assert np.array_equal(a, b), (delta, a, b)
        return
    _, ata, atb = oracle_system(pi, mu, cov, target)
    x = np.linalg.solve(ata, atb)
    tol = BUDGET * (1e-9 + U * np.abs(x).max() / eig_ratio(ata) + cholesky_gap(ata, x))
    worst = max(np.abs(dev[0] - host[0]).max(), np.abs(dev[1] - host[1]).max())
    print("delta %g: cond %.3g, |x| %.3g, device solve vs host solve %.3g, bound %.3g"
          % (delta, 1 / eig_ratio(ata), np.abs(x).max(), worst, tol))
    np.testing.assert_allclose(dev[0], host[0], rtol=0, atol=tol)
    np.testing.assert_allclose(dev[1], host[1], rtol=0, atol=tol * (1 + np.abs(host[1]).max()))
