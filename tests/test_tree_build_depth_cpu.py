"""The inputs of tests/test_tree_build_depth_gpu.py are FAIR: conditions on the cases, checked on the float64 oracle alone.

The GPU file compares leaves and per-level iteration counts exactly, on all points and all levels, with no allowance for
flips.  That is only right if no decision of the oracle's run sits within rounding of going the other way, so for every
case the GPU file uses, _tree_helpers.build_fairness runs the oracle once (the same cached run the GPU file compares
against) and this file asserts:
  every stop margin ||dq| - ls| / ls                              >= 1e-6
  every |m0 - ld| / ld, |det - EPS| / EPS, |den - EPS| / EPS      >= 1e-6
  every non-zero gap between a point's two largest gammas         >= 1e-9
  every zero gap lies between children with bitwise-equal pi, mu, cov (duplicated initial means: every arithmetic ties)
and for the deep cases: live, non-singular nodes at EVERY level, more than 30 distinct leaves, and (L = 6, 256 CUs) chunks
of three or more 256-node tiles in the split log-likelihood, the tiles behind tree_loglik_body's LL_WPRE = 2 prefetch.

Margins of the oracle runs (n = 2500, sig2 = 0.5, ld = 1e-4; "+w": integer weights 0 .. 5; ties = (point, E-step) pairs
with an exact tie, forced = pairs with den <= EPS):
  case          iterations                 stop     ld      det     den     gap     ties  forced  live per level             leaves
  L5_budget     6 6 6 6 6                  7e31    2.2e-2  2.7e-1  4.7e-4  1.0e-6    30    2181   8 33 83 120 192             145
  L5_budget+w   6 6 6 6 6                  2e32    2.2e-2  2.6e-2  3.9e-2  9.8e-6    19    2672   8 33 91 129 197             151
  L6_budget     4 4 4 4 4 4                4e31    3.3e-3  3.8e-2  1.0     3.7e-5   461     257   8 27 85 132 168 209         106
  L6_budget+w   4 4 4 4 4 4                1e32    1.7e-2  1.4e-1  9.9e-1  3.9e-6   457     447   8 29 89 122 156 185         116
  L5_stop       14 27 29 31 15             4.2e-2  1.8e-3  1.4e-3  3.9e-1  4.2e-7   175    1732   8 42 111 186 241            279
  L5_stop+w     14 23 39 31 23             1.1e-1  2.2e-3  3.7e-3  4.6e-2  8.9e-6     0    3473   8 44 95 149 196             235
  L6_stop       10 14 17 9 2 2             6.3e-2  7.3e-3  2.5e-2  1.0     4.4e-7    18     733   8 41 116 267 534 569        273
  L6_stop+w     14 14 11 5 2 2             1.5e-2  5.8e-3  5.0e-4  8.1e-1  3.2e-6     6     713   8 45 124 333 398 418        226
(ls: 1e-30 for the budget cases, 2 / 5 for L5_stop / +w, 20 / 80 for L6_stop / +w; the exact ties all lie between siblings
that drew the same initial mean.)  The plan-boundary cases at 256 CUs (40 blobs in the unit cube, sig2 = 0.01, ls = 1e-30,
budget 2: two iterations per level, stop margins above 1e34, no ties):
  case               n       L  ld      det     den     gap     forced  live per level
  estep_one_pass     196863  2  6.2e-1  4.3e2   7.7     1.1e-7     0    8 56
  estep_two_pass     196864  2  2.2e-1  4.4e1   1.1e6   5.1e-6     0    8 54
  estep_one_pass_w   196863  2  3.5e-2  5.8e2   7.2     1.1e-7     0    8 56
  estep_two_pass_w   196864  2  1.1e-1  3.9e3   1.1e6   5.1e-6     0    8 55
  ll_split_last      261632  3  3.1e-2  1.0     5.6e-2  6.5e-7    15    8 54 155
  ll_unsplit_first   261633  3  1.4e-1  1.0     5.7e-2  2.7e-6    30    8 54 146
  ll_two_points      399999  2  6.0e-2  5.4e3   1.6e9   7.1e-6     0    8 47
  ll_four_points     400000  2  4.0e-2  2.5e1   6.6e3   3.0e-7     0    8 48
(a det margin of 1.0: the nearest determinant to the 1e-15 threshold is a singular node's, of order 1e-18 or below.)
An L = 6 oracle run takes 9 to 14 s (the Python M-step visits 262 144 nodes per level-5 iteration, and every E-step
prepares all 299 592 nodes), the L = 5 ones 2 to 10 s; each is computed once per process."""
import numpy as np
import pytest

import _tree_helpers as H
from oracle import hgmm_tree

CUS = 256                                                       # the MI355X; the GPU file asks the device and checks again
DEEP = [(name, weighted) for name in H.DEEP_CASES for weighted in (False, True)]


def assert_fair(f, label):
    print("%s: iterations %s, margins: stop %.3g, ld %.3g, det %.3g, den %.3g, non-zero gamma gap %.3g; %d exact ties "
          "(between bitwise-equal siblings: %s), %d forced; live per level %s; %d leaves"
          % (label, [int(v) for v in f.trace.iters_per_level], f.stop, f.ld, f.det, f.den, f.gap, f.ties, f.ties_bitwise,
             f.forced, f.live, f.leaves))
    assert H.unfair(f) == [], label


@pytest.mark.parametrize("name,weighted", DEEP)
def test_deep_case_is_fair(name, weighted):
    f = H.deep_oracle(name, weighted)
    label = name + ("+w" if weighted else "")
    assert_fair(f, label)
    L, _, ls, ls_w, budget = H.DEEP_CASES[name]
    iters = [int(v) for v in f.trace.iters_per_level]
    if name.endswith("_budget"):
        assert iters == [budget] * L                            # every level runs to the budget
    else:
        assert max(iters) < budget and min(iters) >= 2          # every level is stopped by ls
    assert len(f.live) == L and min(f.live) >= 8, f.live        # live, non-singular nodes at every level, the last included
    assert f.live[-1] > 100
    assert f.leaves > 30


def test_tolerance_table_covers_the_oracles_own_order_spread():
    """_tree_helpers.DEEP_SPREAD was measured with order_spread (the oracle on the points in index order against the oracle
    on the points reversed); here it is measured again on the cheapest case: the two orders take the same decisions, and
    the tolerance the GPU file derives (10 x the recorded spread, or test_tree_gpu.py's where that is more) covers it.  The
    covariance floor assumes coordinates that reach 4: every deep cloud's do."""
    spread, same = H.order_spread("L5_budget")
    tol = H.depth_rtol(("L5_budget", False))
    print("L5_budget: spread between the two orders", spread, "allowed on the device", tol)
    assert same
    assert all(spread[key] <= tol[key] for key in tol)
    assert set(H.DEEP_SPREAD) == set(DEEP)
    for name in H.DEEP_CASES:
        assert 4.0 <= np.abs(H.deep_inputs(name)[0]).max() <= 10.0


def test_duplicated_initial_means_tie_exactly():
    """T is far above n, so sibling groups draw the same initial mean twice; such siblings stay bitwise equal and their
    gammas tie exactly: the first-max arg-max rule is exercised, at both depths."""
    for L in (5, 6):
        assert sum(H.deep_oracle(name, w).ties for name, w in DEEP if H.DEEP_CASES[name][0] == L) > 0


def test_l6_cases_reach_the_tiles_behind_the_weight_prefetch():
    """tree_ll_split at 256 CUs: the last level of an L = 6 build of 2500 points gets chunks of >= 3 tiles of 256 nodes
    (tree_loglik_body prefetches the node weights of a chunk's first LL_WPRE = 2 tiles only); no level of an L <= 4 build
    of such a cloud gets more than one tile per chunk."""
    llblocks = -(-H.DEEP_N // 512)                              # two points per thread below 400 000 points
    per_level = [H.ll_split(llblocks, 8 ** (l + 1), CUS) for l in range(6)]
    print("chunks x nodes per chunk, levels 0 .. 5:", per_level)
    assert per_level[5][1] // 256 >= 3
    assert per_level[5][0] * per_level[5][1] >= 8 ** 6 > (per_level[5][0] - 1) * per_level[5][1]
    assert all(per // 256 <= 1 for _, per in per_level[:4])


def test_ll_split_at_the_plan_boundary():
    """the split is on at 512 (2 cus - 1) points and off one point later (level 2 of an L = 3 build: two tiles)"""
    n = 512 * (2 * CUS - 1)
    assert H.ll_split(-(-n // 512), 512, CUS) == (2, 256)
    assert H.ll_split(-(-(n + 1) // 512), 512, CUS) == (1, 512)
    assert H.ll_split(-(-n // 512), 64, CUS) == (1, 256)        # (a level of one tile is never split: hence L = 3 there)


@pytest.mark.parametrize("weighted", [False, True])
def test_build_fairness_is_the_oracles_build(weighted):
    """build_fairness only watches: its tables and trace are bit for bit hgmm_tree.build_tree's, with the same ll_chunk --
    and ll_chunk itself only regroups q's sum over the points (the default stays the goldens' bits, test_oracle_golden)."""
    P = H.deep_cloud(7, 900)
    L = 3
    idx = H.deep_init(7, len(P), L)
    w = H.integer_weights(len(P)) if weighted else None
    f = H.build_fairness(P, L, 2.0, 1e-4, idx, 0.5, 40, w=w, ll_chunk=128)
    pi, mu, cov, tr = hgmm_tree.build_tree(P, L, 2.0, 1e-4, idx, 0.5, 40, w=w, ll_chunk=128)
    assert H.same_bits((pi, mu, cov, tr.q, tr.iters_per_level), (f.pi, f.mu, f.cov, f.trace.q, f.trace.iters_per_level))
    assert H.same_bits(tr.current_idx_per_level, f.trace.current_idx_per_level)
    d_pi, d_mu, d_cov, d_tr = hgmm_tree.build_tree(P, L, 2.0, 1e-4, idx, 0.5, 40, w=w)
    assert list(d_tr.iters_per_level) == list(tr.iters_per_level)
    assert H.same_bits((d_pi, d_mu, d_cov), (pi, mu, cov))        # (the E- and M-steps do not see the chunk)
    np.testing.assert_allclose(d_tr.q, tr.q, rtol=1e-13)


@pytest.mark.parametrize("tag,n,L,weighted", H.plan_sizes(CUS))
def test_plan_boundary_case_is_fair(tag, n, L, weighted):
    f = H.plan_oracle(n, L, weighted)
    assert_fair(f, "%s (n = %d, L = %d%s)" % (tag, n, L, ", weighted" if weighted else ""))
    assert [int(v) for v in f.trace.iters_per_level] == [H.PLAN_BUDGET] * L
    assert min(f.live) >= 8
