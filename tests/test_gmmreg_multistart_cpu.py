"""Multi-start L2 GMMReg on the host path (no context): the lock-step driver of gmmreg_gpu/gmmreg.py, the start poses'
quaternions, and the declarations of the resident-cost entries.  CPU only."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

from conftest import ROOT
import l2_scenario as l2s


@pytest.fixture(scope="module")
def solved():
    """The scenario solved once: lock-step from the 27 starts (evaluator calls counted) and serially from each."""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    sc = l2s.scenario()
    cost = cf.RigidCostFunction()
    calls = []
    inner = cost.evaluate_many
    cost.evaluate_many = lambda thetas, pair_ids, sigmas: calls.append(len(thetas)) or inner(thetas, pair_ids, sigmas)
    reg = l2s.registration(cost, sc)
    multi = reg.optimise_multistart(sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"], sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL)
    serial_reg = l2s.registration(cf.RigidCostFunction(), sc)
    serial = [serial_reg.optimise(sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"], cf.theta_from_transformation(s),
                                  l2s.OPT_MAXITER, l2s.OPT_TOL) for s in sc["starts"]]
    identity = serial_reg.optimise(sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"], cost.initial(), l2s.OPT_MAXITER, l2s.OPT_TOL)
    return sc, reg, multi, serial, identity, calls


def test_every_hypothesis_is_the_serial_solve_bit_for_bit(solved):
    _, _, multi, serial, _, _ = solved
    assert len(multi) == len(serial) == 27
    for k, (m, s) in enumerate(zip(multi, serial)):
        assert np.array_equal(m.x, s.x) and m.fun == s.fun and m.nfev == s.nfev, k


def test_evaluator_runs_once_per_lock_step_not_once_per_evaluation(solved):
    _, _, multi, _, _, calls = solved
    nfev = [m.nfev for m in multi]
    print("nfev: sum %d, max %d; evaluator calls %d" % (sum(nfev), max(nfev), len(calls)))
    assert len(calls) == max(nfev) == 85
    assert sum(calls) == sum(nfev) and calls[0] == 27


def test_winner_is_start_14_and_escapes_the_identity_starts_minimum(solved):
    sc, reg, multi, _, identity, _ = solved
    assert reg.best_index_ == 14
    assert all(multi[14].fun <= m.fun for m in multi)
    won = l2s.angle_deg(reg._cost_fn.to_transformation(multi[14].x).rot, sc["truth_rot"])
    stuck = l2s.angle_deg(reg._cost_fn.to_transformation(identity.x).rot, sc["truth_rot"])
    print("winner %.1f deg from the truth (f = %.6e), identity start %.1f deg (f = %.6e)" % (won, multi[14].fun, stuck, identity.fun))
    assert won < 15.0 and stuck > 45.0


def test_theta_from_transformation_round_trips():
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, transforms as tf
    cost = cf.RigidCostFunction()
    poses = list(l2s.scenario()["starts"])
    for axis in range(3):                                     # a half turn about each axis: trace = -1, w = 0
        rot = -np.identity(3)
        rot[axis, axis] = 1.0
        poses.append(tf.RigidTransformation(rot, np.array([0.1, -0.2, 0.3])))
    for k, pose in enumerate(poses):
        theta = cf.theta_from_transformation(pose)
        assert theta.shape == (7,) and theta[0] >= 0.0 and not np.signbit(theta[0]), k
        assert abs(theta[:4] @ theta[:4] - 1.0) < 1e-14, k
        back = cost.to_transformation(theta)
        np.testing.assert_allclose(back.rot, pose.rot, rtol=0, atol=1e-14, err_msg=str(k))
        np.testing.assert_allclose(back.t, pose.t, rtol=0, atol=1e-14, err_msg=str(k))
    assert np.array_equal(cf.theta_from_transformation(tf.RigidTransformation()), cost.initial())


def _quadratic(thetas, pair_ids, sigmas):
    """A synthetic cost: |theta - centre|^2 scaled per hypothesis, so that the solves differ in length."""
    thetas = np.asarray(thetas)
    scale = np.asarray(sigmas, dtype=np.float64)[:, None]
    centre = np.arange(7.0)
    return (scale * (thetas - centre) ** 2).sum(axis=1), 2.0 * scale * (thetas - centre)


def test_evaluator_exception_reaches_the_caller_and_no_thread_survives():
    from hgmm_amd.gmmreg_gpu import gmmreg
    before = threading.active_count()
    calls = []

    def evaluate(thetas, pair_ids, sigmas):
        calls.append(len(thetas))
        if len(calls) == 3:
            raise RuntimeError("evaluator failed on its third call")
        return _quadratic(thetas, pair_ids, sigmas)

    with pytest.raises(RuntimeError, match="third call"):
        gmmreg.lockstep_solve(evaluate, [(np.zeros(7), 0, 1.0 + k) for k in range(5)], 10, 1e-5)
    assert len(calls) == 3 and threading.active_count() == before


def test_solve_exception_reaches_the_caller_and_no_thread_survives():
    from hgmm_amd.gmmreg_gpu import gmmreg
    before = threading.active_count()

    def evaluate(thetas, pair_ids, sigmas):                   # hypothesis 1 gets a gradient of the wrong length: its solve raises
        f, g = _quadratic(thetas, pair_ids, sigmas)
        return f, [row[:3] if pid == 1 else row for row, pid in zip(g, pair_ids)]

    with pytest.raises(Exception):
        gmmreg.lockstep_solve(evaluate, [(np.zeros(7), k, 1.0) for k in range(3)], 10, 1e-5)
    assert threading.active_count() == before


def test_empty_starts_are_refused():
    from hgmm_amd.gmmreg_gpu import cost_functions as cf
    sc = l2s.scenario()
    reg = l2s.registration(cf.RigidCostFunction(), sc)
    with pytest.raises(ValueError, match="starts"):
        reg.optimise_multistart(sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"], [])
    with pytest.raises(ValueError, match="starts"):
        reg.registration_multistart(sc["mu_t"], [])


def test_solves_of_unequal_length_finish():
    """opt_maxiter = 1 on the synthetic cost: the solves stop after different numbers of evaluations (a badly scaled
    hypothesis needs a longer line search); each is the solve run alone and the call count is the longest's."""
    from hgmm_amd.gmmreg_gpu import gmmreg
    before = threading.active_count()
    jobs = [(np.zeros(7), k, s) for k, s in enumerate((1.0, 1e-3, 50.0, 0.5, 7.0))]
    calls = []
    res = gmmreg.lockstep_solve(lambda *a: calls.append(1) or _quadratic(*a), jobs, 1, 1e-5)
    nfev = [r.nfev for r in res]
    assert len(set(nfev)) > 1 and len(calls) == max(nfev), nfev
    for job, r in zip(jobs, res):
        alone = gmmreg.lockstep_solve(_quadratic, [job], 1, 1e-5)[0]
        assert np.array_equal(alone.x, r.x) and alone.fun == r.fun and alone.nfev == r.nfev
    assert threading.active_count() == before


def _declared_args(name):
    txt = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in include/hgmm.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["hgmm_l2_set_pairs", "hgmm_l2_cost"])
def test_resident_cost_entries_are_declared_exported_and_bound(name):
    """The way tests/test_abi_cpu.py checks the other entries, and the binding's argument list against the header's:
    as many arguments, an int where the header has an int, a pointer where it has a pointer."""
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    lib = hgmm_amd.load_library()
    declared = _declared_args(name)
    assert hasattr(lib, name)
    bound = getattr(lib, name).argtypes
    assert bound is not None and len(bound) == len(declared), (declared, bound)
    for d, b in zip(declared, bound):
        if "*" in d:
            assert b is ctypes.c_void_p or issubclass(b, ctypes._Pointer), (d, b)
        else:
            assert d.split()[0] == "int" and b is ctypes.c_int, (d, b)
