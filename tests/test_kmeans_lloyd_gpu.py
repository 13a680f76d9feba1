"""The Lloyd half of the KMeans initialiser (csrc/kmeans_kernels.hip: kmeans_assign_kernel, both accumulators,
kmeans_update_kernel and the device-resident loop hgmm_kmeans_lloyd) against the float64 oracle, where the goldens of
tests/test_kmeans_gpu.py do not reach: exact ties, labels beyond the first 64-centre slot in every accumulator layout,
every stop rule at and around the batch of 8 iterations the host enqueues per synchronisation, and the hand-over of an
empty cluster to the host in iteration 1 and after the device has advanced.

tests/_kmeans_helpers.py holds the inputs and ``walk``, the oracle's loop iteration by iteration;
tests/test_kmeans_lloyd_cpu.py proves on the oracle alone that the inputs are fair (ties where claimed, a margin of
1e-10 at every point of every floating-point iteration -- the two sides differ by summation order, ~1e-15); the
conditions a comparison rests on are asserted here once more before the device is compared."""
import contextlib
import os

import numpy as np
import pytest

import _kmeans_helpers as H
from oracle import kmeans as okm

pytestmark = pytest.mark.gpu

ACC = [pytest.param(0, id="default"), pytest.param(1, id="acc_regs")]


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def _acc(ctx, regs):
    """The accumulator under test: the default (LDS tables up to k = 1024) or the register form at every k."""
    return ctx.config(kmeans_acc_regs=1) if regs else contextlib.nullcontext()


# -- 1. one step on a lattice: everything exact, ties included ------------------------------------------
@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("n,k", H.LATTICE_CASES)
def test_lattice_step_is_exact(ctx, n, k, regs):
    """Coordinates are multiples of 1/2 in [-8, 8]: every difference, square, distance, sum and the inertia is an
    exactly representable double whatever the order and whether or not the distance fuses, so nothing has a
    tolerance.  Bitwise duplicate centres sit inside a group of four, across groups, between the last group and the
    scalar tail, inside the tail and across the 64 / 256 / 1024 boundaries of the accumulators: the first index that
    attains the minimum wins, the later copy stays empty."""
    X, A, _, pairs = H.lattice_case(n, k)
    lab, mind2, counts, sums, inertia, _ = H.lattice_expect(X, A)
    if len(np.unique(A, axis=0)) >= 2:
        assert H.has_tie(X, A).any()
    ctx.set_points(X)
    with _acc(ctx, regs):
        g_sums, g_counts, g_inertia, g_changed = ctx.kmeans_step(A, reset_labels=True)
        g_lab, g_mind2 = ctx.kmeans_labels(with_distances=True)
    assert np.array_equal(g_lab, lab)
    assert np.array_equal(g_mind2, mind2)
    assert np.array_equal(g_counts, counts)
    assert np.array_equal(g_sums, sums)
    assert g_inertia == inertia
    assert g_changed == n
    for _, later in pairs:
        assert g_counts[later] == 0 and not g_sums[later].any()


@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("n,k", H.LATTICE_SECOND_STEP)
def test_lattice_second_step_counts_the_changed_labels(ctx, n, k, regs):
    """A step without a reset after a step with other centres: ``changed`` is the number of labels that differ,
    somewhere strictly between none and all."""
    X, A, B, _ = H.lattice_case(n, k)
    lab_a = H.lattice_expect(X, A)[0]
    lab_b, mind2, counts, sums, inertia, _ = H.lattice_expect(X, B)
    expect = int((lab_a != lab_b).sum())
    assert 0 < expect < n
    ctx.set_points(X)
    with _acc(ctx, regs):
        _, _, _, first = ctx.kmeans_step(A, reset_labels=True)
        g_sums, g_counts, g_inertia, g_changed = ctx.kmeans_step(B, reset_labels=False)
        g_lab, g_mind2 = ctx.kmeans_labels(with_distances=True)
    assert first == n and g_changed == expect
    assert np.array_equal(g_lab, lab_b) and np.array_equal(g_mind2, mind2)
    assert np.array_equal(g_counts, counts) and np.array_equal(g_sums, sums) and g_inertia == inertia


# -- 2. the whole loop at every accumulator layout --------------------------------------------------
@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("n,k", H.LOOP_CASES)
def test_whole_loop_vs_oracle(ctx, n, k, regs):
    """k = 65, 200 (slots 1..3 of the four-slot forms), 300 (the 1024-centre table / sixteen register slots) and 1100
    (two passes of the register form, slot0 > 0): the loop runs to strict convergence on the device."""
    Xc, init = H.loop_case(n, k)
    w = H.loop_walk(n, k)
    H.assert_fair(w)
    ctx.set_points(Xc)
    with _acc(ctx, regs):
        centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, max_iter=60, tol_abs=0.0)
        labels = ctx.kmeans_labels()
    assert (n_iter, strict) == (w.n_iter, w.strict)
    assert pending is None
    assert np.array_equal(labels, w.final_labels)
    np.testing.assert_allclose(centres, w.centres, rtol=0, atol=1e-12)


# -- 3. stop rules and the batch of 8 -----------------------------------------------------------------
@pytest.fixture()
def uniform(ctx):
    Xc, init = H.golden_case("uniform")
    ctx.set_points(Xc)
    return Xc, init


@pytest.mark.parametrize("budget", H.BUDGETS)
def test_budget_stop(ctx, uniform, budget):
    """The budget runs out inside a batch (1, 7, 9, 17), on its last iteration (8, 16): n_iter is the budget, the
    centres are the oracle's after as many iterations, and the assignment to them is the oracle's final one."""
    Xc, init = uniform
    w = H.golden_walk("uniform", budget)
    H.assert_fair(w)
    assert w.n_iter == budget and not w.strict
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, budget, 0.0)
    assert (n_iter, strict) == (budget, False) and pending is None
    np.testing.assert_allclose(centres, w.centres, rtol=0, atol=1e-12)
    # the labels on the device are still those of the budget's last assignment
    assert np.array_equal(ctx.kmeans_labels(), w.labels[-1])
    ctx.kmeans_step(centres)
    assert np.array_equal(ctx.kmeans_labels(), w.final_labels)


def test_strict_stop(ctx, uniform):
    Xc, init = uniform
    w = H.golden_walk("uniform")
    H.assert_fair(w)
    assert w.n_iter == H.STRICT_AT["uniform"] and w.strict
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 50, 0.0)
    assert (n_iter, strict) == (19, True) and pending is None
    assert np.array_equal(ctx.kmeans_labels(), w.labels[18])
    np.testing.assert_allclose(centres, w.centres, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name,m", H.TOL_STOPS)
def test_tolerance_stop(ctx, name, m):
    """``shift <= tol`` at the last iteration of a batch (8), the first of the next (9) and inside one (12), with the
    tolerance percents away from the shifts on either side."""
    Xc, init = H.golden_case(name)
    tol = H.tol_for_stop(name, m)
    shift = H.golden_walk(name).shift
    assert shift[m - 1] < tol and all(tol < s for s in shift[:m - 1])
    w = H.golden_walk(name, 50, tol)
    H.assert_fair(w)
    assert w.n_iter == m and not w.strict
    ctx.set_points(Xc)
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 50, tol)
    assert (n_iter, strict) == (m, False) and pending is None
    np.testing.assert_allclose(centres, w.centres, rtol=0, atol=1e-12)
    assert np.array_equal(ctx.kmeans_labels(), w.labels[-1])


@pytest.mark.parametrize("a,b", H.SPLITS)
def test_split_budget_equals_one_call(ctx, uniform, a, b):
    """Two calls, the second resuming on the first one's labels, are bitwise one call with the summed budget; the
    second reports a strict stop that falls into it."""
    Xc, init = uniform
    whole, n_whole, s_whole, p_whole = ctx.kmeans_lloyd(init, a + b, 0.0)
    labels_whole = ctx.kmeans_labels()
    first, n_a, s_a, p_a = ctx.kmeans_lloyd(init, a, 0.0)
    second, n_b, s_b, p_b = ctx.kmeans_lloyd(first, b, 0.0, reset_labels=False)
    assert p_whole is None and p_a is None and p_b is None
    assert (n_a, s_a) == (a, False) and n_a + n_b == n_whole == a + b
    assert s_b == s_whole == (a + b >= H.STRICT_AT["uniform"])
    assert np.array_equal(second, whole)
    assert np.array_equal(ctx.kmeans_labels(), labels_whole)
    w = H.golden_walk("uniform", a + b)
    assert (w.n_iter, w.strict) == (n_whole, s_whole)
    np.testing.assert_allclose(whole, w.centres, rtol=0, atol=1e-12)


def test_no_budget_returns_at_once(ctx, uniform):
    Xc, init = uniform
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 0, 0.0)
    assert np.array_equal(centres, init) and n_iter == 0 and not strict and pending is None


def test_loop_refuses_a_communicator():
    """The device-resident loop is single-rank: a context with a communicator attached, even of one rank, is an error
    (KMeans.fit takes the step-by-step path there)."""
    import hgmm_amd
    Xc, init = H.golden_case("uniform")
    c = hgmm_amd.Context(0)
    try:
        c.set_points(Xc)
        c.comm_init_host(1, 0, "hgmm_km_lloyd_%d" % os.getpid())
        try:
            with pytest.raises(hgmm_amd.HgmmError):
                c.kmeans_lloyd(init, 5, 0.0)
        finally:
            c.comm_destroy()
    finally:
        c.close()


# -- 4. empty clusters handed to the host -------------------------------------------------------------
def _pending_is_the_oracles_step(pending, Xc, labels, k, changed):
    sums, counts, g_changed = pending
    o_sums, o_counts = H.step_sums(Xc, labels, k)
    assert (o_counts == 0).any()
    assert np.array_equal(counts, o_counts)
    np.testing.assert_allclose(sums, o_sums, rtol=0, atol=1e-11)
    assert g_changed == changed


def _fit_is_the_oracles(ctx, X, init):
    from hgmm_amd.kmeans import KMeans
    Xc, init_c, tol_abs = H.fit_inputs(X, init)
    w = H.walk(Xc, init_c, 50, tol_abs)
    assert min(w.margin[1:] if w.margin[0] == 0.0 else w.margin) >= H.MARGIN_MIN
    assert H.relocation_gap(Xc, w) >= H.MARGIN_MIN
    labels, inertia, centres, n_iter = okm.lloyd(Xc, init_c, 50, tol_abs)
    km = KMeans(n_clusters=len(init), init=init, max_iter=50, ctx=ctx).fit(X)
    assert km.n_iter_ == n_iter and np.array_equal(km.labels_, labels)
    np.testing.assert_allclose(km.cluster_centers_, centres + X.mean(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(km.inertia_, inertia, rtol=1e-12)


def test_three_empty_clusters_in_iteration_1(ctx):
    """Three of k = 8 start centres are bitwise copies of others: the first iteration hands its sums, counts and
    changed labels to the host with the centres untouched and no iteration counted."""
    X, init = H.reloc8_case()
    Xc, init_c, tol_abs = H.fit_inputs(X, init)
    w = H.walk(Xc, init_c, 50, tol_abs)
    assert w.n_empty[0] == 3
    ctx.set_points(Xc)
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init_c, 50, tol_abs)
    assert n_iter == 0 and not strict and pending is not None
    assert np.array_equal(centres, init_c)
    _pending_is_the_oracles_step(pending, Xc, w.labels[0], 8, len(Xc))
    assert np.array_equal(ctx.kmeans_labels(), w.labels[0])
    _fit_is_the_oracles(ctx, X, init)


@pytest.mark.parametrize("n,k,blobs,spread,seed,at", H.LATE_EMPTY_CASES)
def test_first_empty_cluster_after_the_device_has_advanced(ctx, n, k, blobs, spread, seed, at):
    """The device has advanced one iteration (three in the last case) when a cluster comes up empty: it returns that
    count, the centres after it, and the sums, counts and changed labels of the iteration that met the empty cluster;
    the fit resumes from there."""
    X, init = H.late_empty_case(n, k, blobs, spread, seed)
    w = H.walk(X, init, 50, 0.0)
    assert H.first_empty(w) == at and min(w.margin) >= H.MARGIN_MIN
    ctx.set_points(X)
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 50, 0.0)
    assert n_iter == at - 1 and not strict and pending is not None
    np.testing.assert_allclose(centres, w.centres_in[at - 1], rtol=0, atol=1e-12)
    _pending_is_the_oracles_step(pending, X, w.labels[at - 1], k, w.changed[at - 1])
    assert np.array_equal(ctx.kmeans_labels(), w.labels[at - 1])
    _fit_is_the_oracles(ctx, X, init)
