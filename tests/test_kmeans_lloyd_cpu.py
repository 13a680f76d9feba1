"""The inputs of tests/test_kmeans_lloyd_gpu.py are fair ones, proved on the float64 oracle alone (no GPU needed):

* ``_kmeans_helpers.walk`` -- the oracle's Lloyd loop with every iteration's labels, margin, shift, empties and changed
  labels kept -- returns exactly what ``oracle.kmeans.lloyd`` returns on every input used;
* every lattice case holds the exact ties it claims (a point equidistant from two centres of different coordinates;
  a point whose nearest centre is a duplicated one);
* every floating-point trajectory keeps a margin >= 1e-10 between the nearest and the second nearest centre at every
  point of every iteration and (section 2) never empties a cluster, so labels and iteration counts of two float64
  implementations that differ by summation order (~1e-15) must be identical;
* the tolerances of the stop-rule test sit strictly between the shifts they separate; the empty-cluster cases empty
  their first cluster in the iteration they claim.

If a case stops meeting its condition the input is to be changed, never the bound."""
import numpy as np
import pytest

import _kmeans_helpers as H
from oracle import kmeans as okm


def _same_as_lloyd(Xc, init, max_iter, tol_abs, w=None):
    w = w or H.walk(Xc, init, max_iter, tol_abs)
    labels, inertia, centres, n_iter = okm.lloyd(Xc, init, max_iter, tol_abs)
    assert w.n_iter == n_iter
    assert np.array_equal(w.centres, centres)
    assert np.array_equal(w.final_labels, labels)
    assert w.strict == (w.changed[-1] == 0)
    assert len(w.labels) == len(w.margin) == len(w.shift) == len(w.n_empty) == len(w.changed) == n_iter
    # the pieces: every iteration's labels are the oracle's assignment to the centres it started from
    for lab, c in zip(w.labels, w.centres_in):
        assert np.array_equal(lab, okm.assign(Xc, c)[0])
    assert w.changed[0] == len(Xc)
    for i in range(1, n_iter):
        assert w.changed[i] == int((w.labels[i] != w.labels[i - 1]).sum())
    return w


# -- section 1 ---------------------------------------------------------------------------------------
def test_duplicate_positions():
    assert H.duplicate_pairs(1) == []
    assert H.duplicate_pairs(2) == [(0, 1)]
    assert H.duplicate_pairs(3) == [(0, 1), (1, 2)]
    assert H.duplicate_pairs(7) == [(0, 1), (3, 4), (5, 6)]
    assert H.duplicate_pairs(8) == [(0, 1), (2, 7)]
    assert H.duplicate_pairs(63) == [(0, 1), (2, 7), (59, 60), (61, 62)]
    assert H.duplicate_pairs(65) == [(0, 1), (2, 7), (63, 64)]
    assert H.duplicate_pairs(257) == [(0, 1), (2, 7), (255, 256), (63, 64)]
    assert H.duplicate_pairs(1025) == [(0, 1), (2, 7), (1023, 1024), (63, 64), (255, 256)]
    assert H.duplicate_pairs(1024) == [(0, 1), (2, 7), (63, 64), (255, 256)]


@pytest.mark.parametrize("n,k", H.LATTICE_CASES)
def test_lattice_case_holds_the_ties_it_claims(n, k):
    X, A, B, pairs = H.lattice_case(n, k)
    for arr in (X, A, B):
        assert np.array_equal(arr * 2, np.round(arr * 2)) and np.abs(arr).max() <= 8.0
    for a, b in pairs:
        assert np.array_equal(A[a], A[b])
    lab, mind2, counts, sums, inertia, d = H.lattice_expect(X, A)
    # exactness: every distance is a multiple of 1/4, every sum a multiple of 1/2, far below 2^53
    assert np.array_equal(d * 4, np.round(d * 4)) and np.array_equal(sums * 2, np.round(sums * 2))
    assert inertia == float(np.sort(mind2).sum())
    later = [b for _, b in pairs]
    earlier = [a for a, _ in pairs]
    assert (counts[later] == 0).all() and (sums[later] == 0).all()
    if pairs:
        # a point's nearest centre is a duplicated one: the first-index rule decides its label
        assert np.isin(lab, earlier).any()
    distinct = len(np.unique(A, axis=0))
    if distinct >= 2:
        # a point exactly equidistant from its two nearest centres, which differ in their coordinates
        first = np.unique(A, axis=0, return_index=True)[1]          # one position per distinct centre
        two = np.sort(d[:, first], axis=1)[:, :2]
        assert (two[:, 0] == two[:, 1]).any()
    else:
        # (1, 1), (1, 3) and (63, 2): the duplicates leave one distinct centre, so only the duplicate rule is at stake
        assert (n, k) in [(1, 1), (1, 3), (63, 2)]


@pytest.mark.parametrize("n,k", H.LATTICE_SECOND_STEP)
def test_lattice_second_step_changes_some_labels_and_not_all(n, k):
    X, A, B, _ = H.lattice_case(n, k)
    changed = int((H.lattice_expect(X, A)[0] != H.lattice_expect(X, B)[0]).sum())
    assert 0 < changed < n


# -- section 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", H.LOOP_CASES)
def test_loop_case_is_fair_and_walk_is_lloyd(n, k):
    Xc, init = H.loop_case(n, k)
    w = _same_as_lloyd(Xc, init, 60, 0.0, H.loop_walk(n, k))
    H.assert_fair(w)
    assert w.strict and w.n_iter < 60
    print("loop case n=%d k=%d: %d iterations, min margin %.3g" % (n, k, w.n_iter, min(w.margin)))


# -- section 3 ---------------------------------------------------------------------------------------
def _final_assignment_has_a_margin(Xc, centres):
    # the labels reported after a stop that is not strict belong to the final centres: their margin counts too
    d = np.sort(okm._sq_dists(Xc, centres), axis=1)
    assert (d[:, 1] - d[:, 0]).min() >= H.MARGIN_MIN


@pytest.mark.parametrize("name", ["uniform", "blobs"])
def test_golden_trajectory_is_fair_and_walk_is_lloyd(name):
    Xc, init = H.golden_case(name)
    w = _same_as_lloyd(Xc, init, 50, 0.0, H.golden_walk(name))
    H.assert_fair(w)
    assert w.strict and w.n_iter == H.STRICT_AT[name]
    print("%s k=%d: %d iterations, min margin %.3g, shifts %s"
          % (name, len(init), w.n_iter, min(w.margin), " ".join("%.3g" % s for s in w.shift)))


@pytest.mark.parametrize("budget", H.BUDGETS + [a + b for a, b in H.SPLITS])
def test_uniform_budget_walk_is_lloyd(budget):
    Xc, init = H.golden_case("uniform")
    w = _same_as_lloyd(Xc, init, budget, 0.0, H.golden_walk("uniform", budget))
    full = H.golden_walk("uniform")
    assert w.n_iter == min(budget, H.STRICT_AT["uniform"]) and w.strict == (budget >= H.STRICT_AT["uniform"])
    for a, b in zip(w.labels, full.labels):
        assert np.array_equal(a, b)
    if not w.strict:
        _final_assignment_has_a_margin(Xc, w.centres)


@pytest.mark.parametrize("name,m", H.TOL_STOPS)
def test_tolerance_separates_the_shifts(name, m):
    Xc, init = H.golden_case(name)
    shift = H.golden_walk(name).shift
    tol = H.tol_for_stop(name, m)
    assert shift[m - 1] < tol
    assert all(tol < shift[i] for i in range(m - 1))
    # no decision is borderline: percents, not ulps, on either side
    assert shift[m - 1] * 1.01 < tol < min(shift[:m - 1]) / 1.01
    w = _same_as_lloyd(Xc, init, 50, tol, H.golden_walk(name, 50, tol))
    assert w.n_iter == m and not w.strict
    H.assert_fair(w)
    _final_assignment_has_a_margin(Xc, w.centres)


def test_no_tolerance_stops_the_uniform_trajectory_at_iteration_8():
    """Why the stop at the last iteration of a batch is taken from 'blobs': a tolerance stops at iteration m only if
    shift[m] <= tol < every earlier shift, and here iteration 7 moved the centres less than iteration 8."""
    shift = H.golden_walk("uniform").shift
    assert shift[6] < shift[7]
    assert {m for n, m in H.TOL_STOPS if n == "blobs"} == {8, 9, 12}


# -- section 4 ---------------------------------------------------------------------------------------
def _margin_everywhere(w):
    assert min(w.margin) >= H.MARGIN_MIN, min(w.margin)


def _relocation_is_decided(Xc, w):
    # the farthest points, in their order, choose who moves where: none of them within the margin of the next
    assert H.relocation_gap(Xc, w) >= H.MARGIN_MIN, H.relocation_gap(Xc, w)


def _tol_is_not_borderline(w, tol_abs):
    for s in w.shift:
        assert abs(s - tol_abs) > 1e-6 * tol_abs, (s, tol_abs)


def test_reloc8_case_empties_three_clusters_in_iteration_1():
    X, init = H.reloc8_case()
    assert len(np.unique(init, axis=0)) == 5 and len(init) == 8
    Xc, init_c, tol_abs = H.fit_inputs(X, init)
    for i, j in enumerate(H.RELOC8_LAYOUT):
        assert np.array_equal(init_c[i], init_c[H.RELOC8_LAYOUT.index(j)])
    w = _same_as_lloyd(Xc, init_c, 50, tol_abs)
    assert w.n_empty[0] == 3 and H.first_empty(w) == 1
    _tol_is_not_borderline(w, tol_abs)
    _relocation_is_decided(Xc, w)
    # iteration 1 has the exact ties of the copies (margin 0, settled by the first-index rule on both sides);
    # from iteration 2 on no point is near a tie
    assert w.margin[0] == 0.0
    d = okm._sq_dists(Xc, np.unique(init_c, axis=0))
    p = np.partition(d, 1, axis=1)
    assert (p[:, 1] - p[:, 0]).min() >= H.MARGIN_MIN
    assert min(w.margin[1:]) >= H.MARGIN_MIN
    print("reloc8: %d iterations, empties per iteration %s, min margin after it 1 %.3g"
          % (w.n_iter, w.n_empty, min(w.margin[1:])))


@pytest.mark.parametrize("n,k,blobs,spread,seed,at", H.LATE_EMPTY_CASES)
def test_late_empty_case_empties_its_first_cluster_where_it_claims(n, k, blobs, spread, seed, at):
    X, init = H.late_empty_case(n, k, blobs, spread, seed)
    assert X.shape == (n, 3) and init.shape == (k, 3) and at >= 2
    w = _same_as_lloyd(X, init, 50, 0.0)
    assert not any(w.n_empty[:at - 1]) and w.n_empty[at - 1] > 0 and H.first_empty(w) == at
    _margin_everywhere(w)
    _relocation_is_decided(X, w)
    # the same through KMeans.fit's own centring and tolerance (the mean of an already centred cloud is ~1e-17, not 0)
    Xc, init_c, tol_abs = H.fit_inputs(X, init)
    wf = _same_as_lloyd(Xc, init_c, 50, tol_abs)
    assert H.first_empty(wf) == at
    _margin_everywhere(wf)
    _relocation_is_decided(Xc, wf)
    _tol_is_not_borderline(wf, tol_abs)
    print("late empty n=%d k=%d seed %d: %d iterations (fit: %d), empties %s, min margin %.3g"
          % (n, k, seed, w.n_iter, wf.n_iter, w.n_empty, min(w.margin)))
