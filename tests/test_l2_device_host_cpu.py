"""csrc/l2_device.h -- the text the step kernel of hgmm_l2_solve runs -- built for the host with ROCm's clang++ (contraction
off, as the header's pragmas ask on the device) and held to tests/_l2_solve_model.py bit for bit, driven evaluation by
evaluation the way the step kernel is: the 28 solves of the multi-start scenario and the odd ones (a non-unit, a zero and a
NaN quaternion, max_iter = 1, a huge gtol, a long solve).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _l2_solve_cases as cases
import _l2_solve_model as model
import l2_scenario as l2s

CSRC = os.path.join(ROOT, "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("l2_device_host") / "l2_device_host.so")
    cmd = [CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + CSRC,
           os.path.join(ROOT, "tests", "l2_device_host_shim.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.l2h_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    for fn in (lib.l2h_pose, lib.l2h_step, lib.l2h_get):
        fn.argtypes = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_solve(lib, evaluate, theta0, pair, sigma, max_iter, gtol):
    """the loop of hgmm_l2_solve with the host build of l2_solve_step in the step kernel's place"""
    state = np.zeros(lib.l2h_state_size(), np.uint8)
    cur = np.array(theta0, dtype=np.float64)
    lib.l2h_init(_p(state), _p(cur), int(max_iter), float(gtol))
    x, g, xt, f, ints, rot = np.zeros(7), np.zeros(7), np.zeros(7), np.zeros(1), np.zeros(4, np.int32), np.zeros(9)
    for _ in range(1 + 100 * max_iter):                                # (the entry's budget)
        lib.l2h_pose(_p(cur), _p(rot))
        out = np.ascontiguousarray(evaluate((list(rot), list(cur[4:])), pair, sigma), dtype=np.float64)
        lib.l2h_step(_p(state), _p(out))
        lib.l2h_get(_p(state), _p(x), _p(f), _p(g), _p(ints), _p(xt))
        if ints[3]:
            return {"x": x, "f": float(f[0]), "grad": g, "nit": int(ints[0]), "nfev": int(ints[1]), "status": int(ints[2])}
        cur = xt.copy()
    raise AssertionError("the solve did not leave the loop within its budget")


def _differences(a, b):
    return [k for k in a if not np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64),
                                               equal_nan=True)]


def test_the_state_is_the_size_the_device_copies(host):
    assert host.l2h_state_size() == 808


def test_host_build_of_the_step_is_the_model_bit_for_bit(host):
    sc, pair, thetas = cases.scenario_jobs()
    evaluate = cases.host_evaluator([pair])
    jobs = [(th, l2s.OPT_MAXITER, l2s.OPT_TOL) for th in thetas]
    jobs += [(np.r_[thetas[3][:4] * 1.7, thetas[3][4:]], 10, 1e-5), (np.zeros(7), 10, 1e-5), (thetas[0], 1, 1e-5),
             (thetas[5], 3, 1e30), (np.r_[np.nan, np.zeros(6)], 10, 1e-5), (thetas[14], 40, 1e-5)]
    seen = set()
    for k, (th, max_iter, gtol) in enumerate(jobs):
        want = model.solve(evaluate, th, 0, sc["sigma"], max_iter, gtol)
        got = host_solve(host, evaluate, th, 0, sc["sigma"], max_iter, gtol)
        assert not _differences(want, got), (k, _differences(want, got), want, got)
        seen.add(want["status"])
    assert seen == {0, 1, 2, 3}
