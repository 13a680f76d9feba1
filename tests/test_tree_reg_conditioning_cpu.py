"""The conditioning ladder of the registration's 6 x 6 normal equations, with the float64 oracle alone (no GPU).

The library hands an iteration to the stacked least squares (status 2) where lambda_min <= 1e-11 lambda_max of A^T A
(reg_conditioning in csrc/tree_device.h, used by the host step and by the device step).  The ladder
(tree_reg_conditioning_scene.py) brings the eight centroids of a one-level tree within delta of a line; every rung is at
least a decade away from the rule on either side, so that the verdict does not depend on whose rounding built the matrix.
tests/test_tree_reg_conditioning_gpu.py runs the same rungs through the library.

The second half pins which way the cheap tests bound the exact one.  For a symmetric positive definite A = L L^T every
Cholesky pivot L_jj^2 is a Schur complement's leading entry, so L_jj^2 >= lambda_min(A), and every diagonal entry is a
Rayleigh quotient, so A_ii <= lambda_max(A): pivot / diagonal >= lambda_min / lambda_max.  A small pivot ratio therefore
IMPLIES a small eigenvalue ratio, and a harmless pivot ratio says nothing -- the ladder has rungs where the pivots look
six decades better than the eigenvalues are."""
import numpy as np
import pytest

from tree_reg_conditioning_scene import COND_RULE, LADDER, eig_ratio, oracle_system, pivot_ratio, scene
from oracle import hgmm_tree

GO_ON, HAND_OVER = 1e-10, 1e-12          # no rung may fall between the two


@pytest.mark.parametrize("delta", LADDER)
def test_ladder_rung_is_clear_of_the_rule(delta):
    pi, mu, cov, target = scene(delta)
    assert target.shape == (256, 3) and len(pi) == hgmm_tree.n_total(1) == 8
    m0, ata, _ = oracle_system(pi, mu, cov, target)
    assert (~(m0 < hgmm_tree.F32_EPS)).all(), m0
    assert (m0 > 31.9).all(), m0                                  # (every node keeps its own 32 points)
    r, p = eig_ratio(ata), pivot_ratio(ata)
    print("delta %g: lambda_min / lambda_max %.3g, smallest pivot / largest diagonal entry %.3g" % (delta, r, p))
    assert r >= GO_ON or r <= HAND_OVER, r
    assert HAND_OVER < COND_RULE < GO_ON


def test_ladder_has_both_verdicts_and_rungs_the_pivots_do_not_see():
    """Three rungs go on, three hand over, and on at least three of the latter the pivot ratio is far above 1e-11: the rungs
    on which a rule on the pivots goes on where the eigenvalue rule hands over."""
    ratios = [(eig_ratio(a), pivot_ratio(a)) for a in (oracle_system(*scene(d))[1] for d in LADDER)]
    assert [r >= GO_ON for r, _ in ratios] == [True, True, False, False, False, False]
    blind = [d for d, (r, p) in zip(LADDER, ratios) if r <= HAND_OVER and p > 10 * COND_RULE]
    assert blind == [1e-6, 1e-7, 3e-8]


def test_pivot_ratio_never_below_eigenvalue_ratio():
    """Random SPD 6 x 6 matrices Q diag(lam) Q^T with prescribed spectra over 0 to 12 decades: pivot ratio >= eigenvalue
    ratio, up to the rounding of building and factorising the matrix (of order 6 u cond relative to the smallest pivot,
    7e-4 at cond 1e12: the bound carries a factor 1 - 1e-2).  Random rotations rarely open the gap the ladder has; the
    count is printed, not asserted."""
    rs = np.random.RandomState(7)
    n, loose = 4000, 0
    for k in range(n):
        decades = rs.uniform(0.0, 12.0)
        lam = 10.0 ** -np.sort(rs.uniform(0.0, decades, 6))
        lam[0], lam[-1] = 1.0, 10.0 ** -decades                   # the ratio is exactly what was drawn
        lam *= 10.0 ** rs.uniform(-6, 6)
        Q = np.linalg.qr(rs.randn(6, 6))[0]
        A = (Q * lam) @ Q.T
        A = 0.5 * (A + A.T)
        want = lam.min() / lam.max()
        p = pivot_ratio(A)
        assert p >= want * (1.0 - 1e-2), (k, p, want)
        loose += p > 100.0 * want
    print("pivot ratio more than 100 times the eigenvalue ratio in %d of %d matrices" % (loose, n))
