"""flat_boundary_kernel (reduction + M-step + next packed table + stop rule in one launch, over the fused kernel's
component-major partials) against the two launches it replaces (flat_reduce_kernel + flat_finalize_kernel over
stat-major partials): the same fit BIT FOR BIT -- model, log-likelihood trace, iteration count, flags.  No tolerance.

Every case runs the same fit twice in this process: on a context created under HGMM_FLAT_BOUNDARY=1 (the one launch)
and on one created under HGMM_FLAT_BOUNDARY=2 (the two launches; the switch is read once, at context creation).  The
one-launch form measured no faster (profiles/r07/boundary_ab.md), so the two launches are also what a context created
without the variable runs -- which the second test checks.

Shapes: N = 4099 (ragged last wave) and N = 40000; on a 256-CU device both get a fused grid of 512 workgroups -- a
multiple of the reduction's 32 slices -- so N = 1999 is run as well: 500 workgroups, 20 slices of 16 blocks and 12 of
15 (asserted from the device's CU count and launch_fused's grid rule).  J = 1 (a single slot), 33 (ragged slot),
100 (the bunny size, on bun000), 800 (the headline's 13 slots), 1024 (the largest non-chunked).
"""
import os

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

FLAVOURS = [("diag", "W"), ("spherical", "W"), ("diag", "G")]
FIELDS = ("inv_std", "mu", "w", "cov", "lls", "converged")


def _context_under(value):
    import hgmm_amd
    old = os.environ.pop("HGMM_FLAT_BOUNDARY", None)
    try:
        if value is not None:
            os.environ["HGMM_FLAT_BOUNDARY"] = value
        return hgmm_amd.Context(0)
    finally:
        os.environ.pop("HGMM_FLAT_BOUNDARY", None)
        if old is not None:
            os.environ["HGMM_FLAT_BOUNDARY"] = old


@pytest.fixture(scope="module")
def pair():
    one, two = _context_under("1"), _context_under("2")
    yield one, two
    one.close()
    two.close()


@pytest.fixture(scope="module")
def frame():
    return bench.synth_frame(0)


def _cloud(frame, bunny, n, J):
    src = bunny if J == 100 else frame
    return np.ascontiguousarray(src[:n], dtype=np.float32)


def _init(X, J, cov_type):
    mu, w, cov = bench.init_params(X, J)
    return mu, w, (cov if cov_type == "diag" else np.ascontiguousarray(cov[:, 0]))


def _fused_grid(cus, n, J):
    """launch_fused's grid (flat_kernels.hip)."""
    ns = (J + 63) // 64
    bpc = 8 if ns <= 4 else (6 if ns <= 8 else 4)
    floor = max(1, min((n + 3) // 4, cus * 2, 2048))
    return max(floor, min(n // 400, cus * bpc, 2048))


def _same(a, b):
    for name, x, y in zip(FIELDS, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, name
        if x.dtype == np.float32:                             # the bits, so that a NaN equals itself and -0 is not +0
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("cov_type,variant", FLAVOURS)
@pytest.mark.parametrize("J", [1, 33, 100, 800, 1024])
@pytest.mark.parametrize("n", [1999, 4099, 40000])
def test_one_launch_is_bitwise_the_two_launches(pair, frame, bunny, n, J, cov_type, variant):
    one, two = pair
    if n == 1999:
        grid = _fused_grid(one.device_info()["compute_units"], n, J)
        assert grid % 32 != 0 and grid > 32, grid            # some slices get one block fewer
    X = _cloud(frame, bunny, n, J)
    mu, w, cov = _init(X, J, cov_type)
    got = []
    for c in (one, two):
        c.set_points(X)
        got.append(c.flat_train(5, 0.0, mu, cov, w, cov_type, variant))
    assert len(got[0][4]) == 5 and len(got[1][4]) == 5 and not got[0][5]
    _same(got[0], got[1])


def test_the_switch_selects_the_kernel_and_the_default_is_two_launches(pair, frame):
    X = np.ascontiguousarray(frame[:4099])
    mu, w, cov = _init(X, 33, "diag")
    default = _context_under(None)
    try:
        launches = []
        for c in pair + (default,):
            c.set_points(X)
            c.profile_reset()
            c.profile_enable(True)
            c.flat_train(5, 0.0, mu, cov, w, "diag", "W")
            launches.append((c.profile_get("flat_boundary")[1], c.profile_get("flat_fused")[1]))
            c.profile_enable(False)
    finally:
        default.close()
    assert launches == [(5, 5), (0, 5), (0, 5)]


def test_early_stop_stays_stopped(pair, frame):
    """A tolerance that stops the fit at iteration 3 of 10 enqueued, then six more steps: the double-buffered stop
    flag (both parities) and "stays stopped"."""
    one, two = pair
    X = np.ascontiguousarray(frame[:40000])
    mu, w, cov = _init(X, 33, "diag")
    two.set_points(X)
    trace = two.flat_train(10, 0.0, mu, cov, w, "diag", "W")[4].astype(np.float64)
    d1, d2 = abs(trace[1] - trace[0]), abs(trace[2] - trace[1])
    assert d2 < 0.5 * d1                                      # (a tolerance fits between the second and the third change)
    tol = float(np.float32(0.5 * (d1 + d2)))
    results = []
    for c in (one, two):
        c.set_points(X)
        for extra in (0, 6):
            c.flat_train_begin(tol, mu, cov, w, "diag", "W", lls_capacity=16)
            c.flat_train_step(10)
            if extra:
                c.flat_train_step(extra)
            results.append(c.flat_train_end())
    for r in results:
        assert r[6] == 3 and r[5] and len(r[4]) == 3
        _same(results[0][:6], r[:6])
    assert np.array_equal(results[0][4], trace[:3].astype(np.float32))
