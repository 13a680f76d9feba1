"""hgmm_tree_build at the depths it is used at -- L = 5 (the default of GMMTree) and L = 6 -- and on either side of the
sizes at which build_plan / tree_ll_split change form, against the float64 oracle: tables, leaves, per-level iteration
counts and the q trace, of the tree the build itself produces (the deep registration tests run on trees handed in).

What L <= 4 on a small cloud never reaches: log-likelihood chunks of several 256-node tiles (the tiles behind
tree_loglik_body's LL_WPRE = 2 weight prefetch, and tree_ll_estep_kernel's twin), the partition / offsets / chunk table at
4096 and 32 768 parent segments, moments launches of 32 768 workgroups and more that mostly gather nothing, the reach test
and live-node compaction with more than 99.9 % of a level dead, the direct download of tables too large for the ring.

Every case's inputs are vetted on the oracle alone by tests/test_tree_build_depth_cpu.py (no decision within rounding of
going the other way), so leaves and iteration counts are compared exactly, on all points and levels.  q and the tables:
the tolerances of tests/test_tree_gpu.py for this path where a second float64 arithmetic can meet them -- the
plan-boundary cases do -- and ten times the measured spread between two summation orders of the oracle itself on the deep
cases, whose 50 to 140 EM iterations carry last-bit differences along (_tree_helpers.DEEP_SPREAD: the figures, case by
case; profiles/tree_build_depth.md: the device's differences beside them).  Every oracle run is computed once (a cache in
_tree_helpers) and shared."""
import numpy as np
import pytest

import _tree_helpers as H
from oracle import hgmm_tree

pytestmark = pytest.mark.gpu

I3 = np.identity(3)
STOP_CASES = ["L5_stop", "L6_stop"]
ALL_CASES = list(H.DEEP_CASES)


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def gpu_build(ctx, inputs, w=None):
    P, L, ls, ld, idx, sig2, budget = inputs
    P = np.ascontiguousarray(P, dtype=np.float64)
    ctx.set_points(P)
    if w is not None:
        ctx.tree_set_source_weights(w)
    return ctx.tree_build(L, ls, ld, P[idx], sig2, budget)


@pytest.fixture(scope="module")
def built(ctx):
    """the default-form float64 builds of the deep cases, each run once: built(name, weighted) -> (pi, mu, cov, leaf, iters, q)"""
    cache = {}

    def get(name, weighted=False):
        if (name, weighted) not in cache:
            w = H.integer_weights(H.DEEP_N) if weighted else None
            cache[name, weighted] = gpu_build(ctx, H.deep_inputs(name, weighted), w)
        return cache[name, weighted]
    return get


def assert_is_the_oracles_tree(got, f, label, case=None, leaf=True):
    """(pi, mu, cov, leaf, iters, q) of the device against a Fairness of the oracle; prints the figures before it asserts.
    Iterations, leaves (the whole path of every point) and the set of dead nodes exactly; q, pi, mu, cov within
    _tree_helpers.depth_rtol: the tolerances of tests/test_tree_gpu.py, or ten times the spread between two summation
    orders of the oracle itself on that ``case`` where that is more (DEEP_SPREAD holds the measured figures)."""
    tol = H.depth_rtol(case)
    coord2 = 1.0 if case is None else H.DEEP_COORD2             # (the plan-boundary clouds lie in the unit cube)
    pi, mu, cov, lf, iters, q = got
    print("%s: iterations %s / %s" % (label, [int(v) for v in iters], [int(v) for v in f.trace.iters_per_level]))
    assert list(iters) == list(f.trace.iters_per_level), label
    assert len(q) == int(np.sum(iters)) == len(f.trace.q), label
    live = f.pi > 0
    print("%s: largest |dq| / |q| %.3g; |dpi| %.3g, |dmu| %.3g, |dcov| %.3g (over max(|cov|, 1e-3): %.3g); "
          "dead nodes %d / %d"
          % (label, (np.abs(q - f.trace.q) / np.abs(f.trace.q)).max(), np.abs(pi - f.pi).max(), np.abs(mu - f.mu).max(),
             np.abs(cov - f.cov).max(),
             (np.abs(cov - f.cov) / np.maximum(np.abs(f.cov), 1e-3)).max(),
             int((pi == 0).sum()), int((~live).sum())))
    excess = {key: H.depth_excess(a, b, key, tol[key], coord2) for key, a, b in (("q", q, f.trace.q), ("pi", pi, f.pi), ("mu", mu, f.mu),
                                                                         ("cov", cov, f.cov))}
    print("%s: largest |a - b| / (|b| + floor) %s; allowed %s"
          % (label, {k: "%.3g" % (v * tol[k]) for k, v in excess.items()}, {k: "%.3g" % v for k, v in tol.items()}))
    assert excess["q"] <= 1.0, (label, excess)
    if leaf:
        L = len(iters)
        node = lf.astype(np.int64)
        for l in range(L - 1, -1, -1):                          # the leaf determines the path: parent(c) = c // 8 - 1
            wrong = np.nonzero(node != f.trace.current_idx_per_level[l])[0]
            assert len(wrong) == 0, "%s: %d points differ at level %d, the first: %s" % (label, len(wrong), l, wrong[:5])
            node = node // 8 - 1
    # dead nodes: the same set, and exactly (0, 0, I) on both sides
    assert np.array_equal(pi == 0, ~live), label
    for p_, m_, c_ in ((pi, mu, cov), (f.pi, f.mu, f.cov)):
        assert (p_[~live] == 0).all() and (m_[~live] == 0).all() and (c_[~live] == I3).all(), label
    assert excess["pi"] <= 1.0 and excess["mu"] <= 1.0 and excess["cov"] <= 1.0, (label, excess)


# ---- a. the serial build against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_serial_build_is_the_oracles_tree(built, name):
    assert_is_the_oracles_tree(built(name), H.deep_oracle(name), name, (name, False))


# ---- b. weights 0 .. 5: deep nodes die by weight ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_weighted_build_is_the_oracles_tree(ctx, built, name):
    inputs = H.deep_inputs(name, True)
    P, L, ls, ld, idx, sig2, budget = inputs
    assert_is_the_oracles_tree(built(name, True), H.deep_oracle(name, True), name + "+w", (name, True))
    # weights off on the resident cloud: the unweighted build again, bit for bit
    plain = built(name)
    un = H.deep_inputs(name)
    ctx.set_points(P)
    ctx.tree_set_source_weights(H.integer_weights(len(P)))
    ctx.tree_set_source_weights(None)
    again = ctx.tree_build(L, un[2], ld, P[idx], sig2, budget)
    assert H.same_bits(again, plain)


# ---- c. the plan's other forms at depth --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_other_forms_of_the_plan_build_the_same_tree(ctx, built, name):
    """HGMM_TREE_TICKETS=1, HGMM_TREE_AHEAD=0, HGMM_TREE_OVERLAP=0 as in
    test_stop_rule_in_the_next_launch_equals_the_ticketed_tail: tables, leaves and iteration counts bit for bit, q bit for bit
    below level 0 and within 1e-13 at level 0 (the overlapped form takes level 0's q out of the E-step workgroups).  The
    symmetric quadratic form (HGMM_TREE_NO_CHOL=1) is another arithmetic: it is held to the oracle like the default."""
    inputs = H.deep_inputs(name)
    a = built(name)
    n0 = int(a[4][0])
    for option in ("tree_tickets", "tree_ahead", "tree_overlap"):
        with ctx.config(**{option: 1 if option == "tree_tickets" else 0}):
            other = gpu_build(ctx, inputs)
        assert list(other[4]) == list(a[4]), option
        assert H.same_bits(other[:4], a[:4]), option
        assert np.array_equal(other[5][n0:], a[5][n0:]), option
        np.testing.assert_allclose(other[5][:n0], a[5][:n0], rtol=1e-13, atol=0, err_msg=option)
    with ctx.config(tree_no_chol=1):
        sym = gpu_build(ctx, inputs)
        assert ctx.tree_stats()[1] == 1
    assert_is_the_oracles_tree(sym, H.deep_oracle(name), name + " symmetric form", (name, False))


# ---- d. float32 pdfs behind the stop rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STOP_CASES)
def test_float32_pdfs_stop_where_float64_does(ctx, built, name):
    inputs = H.deep_inputs(name)
    ref = built(name)
    ctx.tree_set_precision(np.float32)
    try:
        got = gpu_build(ctx, inputs)
    finally:
        ctx.tree_set_precision(np.float64)
    print("%s: iterations float32 %s / float64 %s" % (name, list(got[4]), list(ref[4])))
    assert list(got[4]) == list(ref[4])
    worst = np.abs(got[5] - ref[5]).max()
    print("%s: largest |q32 - q64| %.3g (ls = %g)" % (name, worst, inputs[2]))
    assert H.same_bits(got[:4], ref[:4])                        # the E-step and the moments stay float64
    assert worst < 0.01 * inputs[2]


# ---- e. a member of a ragged forest ------------------------------------------------------------------------------------
def test_weighted_member_of_a_ragged_forest_is_the_oracles_tree(ctx):
    """three deep clouds of different sizes, L = 6; the middle one is the weighted L6_stop case and goes against the oracle
    (the batched entry returns no leaves: tables, iteration counts and q)"""
    P, L, ls, ld, idx, sig2, budget = H.deep_inputs("L6_stop", True)
    clouds = [H.deep_cloud(71, 1700), P, H.deep_cloud(72, 3100)]
    weights = [None, H.integer_weights(len(P)), None]
    arrs = ctx.set_points_batch(clouds, weights=weights)
    init = np.stack([a[H.deep_init(61 + b, len(a), L)] if b != 1 else a[idx] for b, a in enumerate(arrs)])
    (pi, mu, cov), iters, traces = ctx.tree_build_batch([len(a) for a in arrs], L, ls, ld, init, sig2, budget, want_trace=True)
    print("forest: per-level iterations", iters.tolist())
    assert_is_the_oracles_tree((pi[1], mu[1], cov[1], None, iters[1], traces[1]), H.deep_oracle("L6_stop", True),
                               "forest member", ("L6_stop", True), leaf=False)


# ---- f. the plan's boundaries in n -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [row[0] for row in H.plan_sizes(256)])
def test_plan_boundaries_in_n(ctx, tag):
    """either side of the two-pass E-step, of the last split log-likelihood launch and of the four-point log-likelihood
    (where the overlapped form ends): tables, leaves and q against the oracle, one weighted case on each side of the first.
    The sizes follow the device's CU count."""
    cus = int(ctx.device_info()["compute_units"])
    sizes = {row[0]: row[1:] for row in H.plan_sizes(cus)}
    assert {n for n, _, _ in sizes.values()} == {256 * 3 * cus + 255, 256 * 3 * cus + 256, 512 * (2 * cus - 1),
                                                 512 * (2 * cus - 1) + 1, 399_999, 400_000}
    n, L, weighted = sizes[tag]
    f = H.plan_oracle(n, L, weighted)
    assert H.unfair(f) == [], tag                               # (vetted in the CPU file for 256 CUs; here for this device's)
    inputs = H.plan_inputs(n, L)
    got = gpu_build(ctx, inputs, H.integer_weights(n) if weighted else None)
    assert_is_the_oracles_tree(got, f, "%s (n = %d, L = %d)" % (tag, n, L))         # (test_tree_gpu.py's tolerances as they are)


# ---- g. repeatability --------------------------------------------------------------------------------------------------
def test_deep_build_repeats_bit_for_bit(ctx, built):
    again = gpu_build(ctx, H.deep_inputs("L6_stop"))
    assert H.same_bits(again, built("L6_stop"))
