"""The written-down arithmetic of the device L2 solve (tests/_l2_solve_model.py) against SciPy itself, on the CPU: the dcsrch
port step for step, the 28 solves of the multi-start scenario and the golden mixtures, with the host NumPy cost as the
model's evaluator.  And the mirrors' refusal without a context: this project has no CPU fallback."""
import numpy as np
import pytest

import _l2_solve_cases as cases
import _l2_solve_model as model
import l2_scenario as l2s


# ---- the dcsrch port -------------------------------------------------------------------------------------------------------
def _quadratic(a):
    return (a - 2.0) * (a - 2.0), 2.0 * (a - 2.0)


def _beyond(a):                       # More and Thuente's first function: the minimum at sqrt(2), far beyond a first step of 1e-3
    return -a / (a * a + 2.0), (a * a - 2.0) / ((a * a + 2.0) * (a * a + 2.0))


def _unbounded(a):                    # fails: the step grows until the 100 evaluations are spent
    return -a, -1.0


def _lying(a):                        # fails: the derivative promises a descent the function never delivers
    return 1.0 + a, -1.0


@pytest.mark.parametrize("fn,alpha1,ends", [(_quadratic, 1.0, "CONV"), (_quadratic, 7.5, "CONV"), (_beyond, 1e-3, "CONV"),
                                             (_beyond, 10.0, "CONV"), (_unbounded, 1.0, "WARN"), (_lying, 1.0, "WARN")])
def test_dcsrch_port_takes_scipys_steps(fn, alpha1, ends):
    from scipy.optimize._dcsrch import DCSRCH
    phi0, derphi0 = fn(0.0)
    theirs = []

    def phi(a):
        theirs.append(float(a))
        return fn(a)[0]
    stp, phi1, _, task = DCSRCH(phi, lambda a: fn(a)[1], model.FTOL, model.GTOL, model.XTOL, model.STPMIN, model.STPMAX)(
        alpha1, phi0=phi0, derphi0=derphi0, maxiter=100)
    my_task, my_stp, my_phi1, mine = model.line_search(fn, alpha1, phi0, derphi0)
    print("%s from %g: %d steps, task %r" % (fn.__name__, alpha1, len(mine), task))
    assert mine == theirs
    assert task[:4].decode() == ends and {model.CONV: "CONV", model.WARN: "WARN", model.ERROR: "ERRO"}[my_task] == ends
    if ends == "CONV":
        assert my_stp == stp and my_phi1 == phi1
    else:
        assert stp is None


def test_dcsrch_port_refuses_what_scipy_refuses():
    from scipy.optimize._dcsrch import DCSRCH
    for alpha1, derphi0 in ((0.0, -1.0), (1.0, 0.5), (1e101, -1.0)):
        stp, _, _, task = DCSRCH(lambda a: a, lambda a: 1.0, model.FTOL, model.GTOL, model.XTOL, model.STPMIN, model.STPMAX)(
            alpha1, phi0=0.0, derphi0=derphi0)
        assert stp is None and task[:5] == b"ERROR"
        assert model.line_search(lambda a: (a, 1.0), alpha1, 0.0, derphi0)[0] == model.ERROR
    # scalar_search_wolfe1's first step
    assert model.first_step(1.0, 1.5, -1.0) == 1.0 and model.first_step(1.0, 1.5, 0.0) == 1.0
    assert model.first_step(1.0, 1.25, -2.0) == min(1.0, 1.01 * 2 * (1.0 - 1.25) / -2.0)
    assert model.first_step(1.0, 0.5, -1.0) == 1.0                       # (negative: 1)


# ---- the 28 solves of the scenario -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    sc, pair, thetas = cases.scenario_jobs()
    evaluate = cases.host_evaluator([pair])
    ours = [model.solve(evaluate, th, 0, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL) for th in thetas]
    scipys = [cases.scipy_solve(th, pair, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL) for th in thetas]
    spreads = [cases.spread(th, pair, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL, base) for th, base in zip(thetas, scipys)]
    return ours, scipys, spreads


def test_nit_and_status_are_scipys_for_every_start(solved):
    ours, scipys, _ = solved
    assert len(ours) == 28
    print("status: %s" % [o["status"] for o in ours])
    print("nfev (model, SciPy): %s" % [(o["nfev"], int(s.nfev)) for o, s in zip(ours, scipys)])
    for k, (o, s) in enumerate(zip(ours, scipys)):
        assert (o["nit"], o["status"]) == (int(s.nit), int(s.status)), k
    # (nfev is not compared: the second line search is not run, and SciPy does not count a point it is asked for twice in a row)


def test_x_and_f_within_scipys_own_spread(solved):
    ours, scipys, spreads = solved
    for k, (o, s, (sx, sf)) in enumerate(zip(ours, scipys, spreads)):
        dx = float(np.abs(np.array(o["x"]) - s.x).max())
        df = abs(o["f"] - float(s.fun)) / abs(float(s.fun))
        print("start %2d status %d: |dx| %.2e (SciPy's spread %.2e)  |df|/|f| %.2e (%.2e)" % (k, o["status"], dx, sx, df, sf))
    for k, (o, s, (sx, sf)) in enumerate(zip(ours, scipys, spreads)):
        assert float(np.abs(np.array(o["x"]) - s.x).max()) <= max(10.0 * sx, cases.X_FLOOR), k
        assert abs(o["f"] - float(s.fun)) / abs(float(s.fun)) <= max(10.0 * sf, cases.F_FLOOR), k


def test_winner_is_start_14(solved):
    from hgmm_amd.gmmreg_gpu import gmmreg
    ours, _, _ = solved
    assert gmmreg._lowest([o["f"] for o in ours[:27]]) == 14


# ---- the reference's own mixtures -------------------------------------------------------------------------------------------
def test_golden_mixtures_land_on_the_reference_pose():
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    g, pair, sigma = cases.golden_case()
    allowance, spread10 = cases.golden_allowance(pair, sigma)
    print("10 x SciPy's +-1-ulp spread of the pose: %.2e -> allowance %.1e" % (spread10, allowance))
    cost = cf.RigidCostFunction()
    res = model.solve(cases.host_evaluator([pair]), cost.initial(), 0, sigma, 10, 1.0e-5)
    tfm = cost.to_transformation(np.array(res["x"]))
    print("|rot - reg_rot| %.2e  |t - reg_t| %.2e" % (np.abs(tfm.rot - g["reg_rot"]).max(), np.abs(tfm.t - g["reg_t"]).max()))
    np.testing.assert_allclose(tfm.rot, g["reg_rot"], rtol=0, atol=allowance)
    np.testing.assert_allclose(tfm.t, g["reg_t"], rtol=0, atol=allowance)


# ---- the model's pose and Jacobian are the host's ---------------------------------------------------------------------------
def test_quaternion_terms_are_the_hosts():
    from hgmm_amd.gmmreg_gpu import so
    rs = np.random.RandomState(3)
    for scale in (1.0, 1.7, 0.3):
        q = rs.randn(4)
        q *= scale / np.linalg.norm(q)
        rot, d = model.quat_terms([float(v) for v in q])
        np.testing.assert_allclose(np.array(rot).reshape(3, 3), so.quaternion_matrix(q)[:3, :3], rtol=0, atol=1e-15)
        np.testing.assert_allclose(np.array(d).reshape(4, 3, 3), so.diff_rot_from_quaternion(q), rtol=0, atol=1e-14)
    rot, d = model.quat_terms([0.0, 0.0, 0.0, 0.0])
    assert rot == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and all(v != v for row in d for v in row)


# ---- the mirrors -----------------------------------------------------------------------------------------------------------
def test_solve_many_without_a_context_raises():
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    sc, pair, thetas = cases.scenario_jobs()
    cost = cf.RigidCostFunction()
    cost.set_pairs([pair])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cost.solve_many(thetas[:2], 0, sc["sigma"], 10, 1.0e-5)
    reg = l2s.registration(cost, sc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.optimise_multistart(*pair, sc["starts"], solver="device")
    with pytest.raises(ValueError, match="solver"):
        reg.optimise_multistart(*pair, sc["starts"], solver="host")
    # the default is SciPy, as it was
    import inspect
    from hgmm_amd.gmmreg_gpu import gmmreg
    for fn in (gmmreg.L2DistRegistration.optimise_multistart, gmmreg.L2DistRegistration.registration_multistart,
               gmmreg.registration_gmmreg, gmmreg.registration_gmmreg_batch):
        assert inspect.signature(fn).parameters["solver"].default == "scipy", fn


@pytest.mark.parametrize("name", ["hgmm_l2_solve", "hgmm_l2_solve_each"])
def test_solve_entries_are_declared_exported_and_bound(name):
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    from test_gmmreg_multistart_cpu import _declared_args
    lib = hgmm_amd.load_library()
    declared = _declared_args(name)
    bound = getattr(lib, name).argtypes
    assert bound is not None and len(bound) == len(declared), (declared, bound)
    for dcl, b in zip(declared, bound):
        if "*" in dcl:
            assert b is ctypes.c_void_p or issubclass(b, ctypes._Pointer), (dcl, b)
        else:
            assert (dcl.split()[0], b) in (("int", ctypes.c_int), ("double", ctypes.c_double)), (dcl, b)
    assert hasattr(hgmm_amd.Context, "l2_solve")
