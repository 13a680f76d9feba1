"""Per-point weights of the SOURCE cloud in the tree build (hgmm_tree_set_source_weights), the parts that need no GPU: the
weighted build the GPU tests compare against (oracle.hgmm_tree.build_tree(w=...)) is the pinned unweighted build of the
cloud with its points repeated when the weights are integers, is the unweighted build bit for bit with unit weights, and
scales exactly with w == 2; the mirrors refuse bad weights before they touch the library, upload the cloud before its weights, and a
WeightedPoints source brings its weights; the two C entries are declared, exported and bound."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import hgmm_tree

LS, LD, SIG2 = 20.0, 1e-4, 0.004
CASES = {700: 2, 3000: 3}           # points -> tree levels


def draw_cases(bunny, seed=5):
    """per case: n bunny points, integer weights 1..4 and T initial means among the points -- ONE seeded generator, the
    cases drawn in the order of their size"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in sorted(CASES):
        X = bunny[rng.choice(len(bunny), n, replace=False)].astype(np.float64)
        c = rng.integers(1, 5, n)
        out[n] = (X, c, rng.integers(0, n, hgmm_tree.n_total(CASES[n])))
    return out


def draw(bunny, n, L):
    return draw_cases(bunny)[n]


def wbuild(X, L, ls, ld, init_mu, w, **kw):
    """the oracle's build as the C entry is called: initial means as coordinates, weights ``w`` (None: none)"""
    return hgmm_tree.build_tree(X, L, ls, ld, None, SIG2, w=w, init_mu=init_mu, **kw)


@pytest.fixture(scope="module")
def builds(bunny):
    """the weighted build of every case, computed once"""
    out = {}
    for n, L in CASES.items():
        X, c, idx = draw(bunny, n, L)
        out[n] = (X, c, idx, wbuild(X, L, LS, LD, X[idx], c.astype(np.float64)))
    return out


@pytest.mark.parametrize("n", sorted(CASES))
def test_restatement_is_the_pinned_oracle_on_the_repeated_cloud(builds, n):
    """integer weights are repetition: the weighted build of (X, c) against oracle.hgmm_tree.build_tree of np.repeat(X, c).
    The two differ in the order of the additions only.  Equal iteration counts, every stop decision of the oracle's build
    further than 1e-3 (relative to ls) from going the other way, q and the tables at rtol 1e-9."""
    L = CASES[n]
    X, c, idx, (pi, mu, cov, tr) = builds[n]
    first = np.cumsum(c) - c                                          # the first copy of point i in the repeated cloud
    o_pi, o_mu, o_cov, o_tr = hgmm_tree.build_tree(np.repeat(X, c, axis=0), L, LS, LD, first[idx], SIG2)
    margin = hgmm_tree.stop_margins(o_tr.q, o_tr.iters_per_level, LS)
    dead = int((o_pi == 0.0).sum())
    print("n=%d L=%d: iterations %s / %s, smallest stop margin %.3g, %d dead nodes" %
          (n, L, list(tr.iters_per_level), list(o_tr.iters_per_level), margin.min(), dead))
    for name, a, b in (("q", tr.q, o_tr.q), ("pi", pi, o_pi), ("mu", mu, o_mu), ("cov", cov, o_cov)):
        if np.shape(a) == np.shape(b):
            print("   %s: largest relative difference %.3g" % (name, (np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max()))
    assert margin.min() > 1e-3
    assert list(tr.iters_per_level) == list(o_tr.iters_per_level)
    np.testing.assert_allclose(tr.q, o_tr.q, rtol=1e-9, atol=0)
    assert np.array_equal(pi == 0.0, o_pi == 0.0)                     # the same nodes died
    np.testing.assert_allclose(pi, o_pi, rtol=1e-9, atol=0)
    # (mu and cov carry the cancellation of m1 / m0 resp. m2 / m0 - mu mu^T: relative to the table's largest entry)
    np.testing.assert_allclose(mu, o_mu, rtol=1e-9, atol=1e-9 * np.abs(o_mu).max())
    np.testing.assert_allclose(cov, o_cov, rtol=1e-9, atol=1e-9 * np.abs(o_cov[o_pi > 0]).max())
    for a, b in zip(tr.current_idx_per_level, o_tr.current_idx_per_level):
        assert np.array_equal(np.repeat(a, c), b)                     # every copy of a point goes where the point went


@pytest.mark.parametrize("n", sorted(CASES))
def test_restatement_without_weights_and_with_unit_weights_is_the_oracle_bit_for_bit(bunny, n):
    """There is one build: ``w = None`` with the means given as indices is the reference.  Against it, bit for bit, the
    means given as coordinates (the other initialisation) and ``w = ones``, which runs the three weighted statements --
    the multiply, W as an index-order sum and the weighted log-likelihood sum."""
    L = CASES[n]
    X, _, idx = draw(bunny, n, L)
    ref = hgmm_tree.build_tree(X, L, LS, LD, idx, SIG2)
    assert hgmm_tree.weight_sum(np.ones(n)) == n
    for w in (None, np.ones(n)):
        got = wbuild(X, L, LS, LD, X[idx], w)
        for a, b in zip(ref[:3], got[:3]):
            assert np.array_equal(a, b)
        assert np.array_equal(ref[3].q, got[3].q) and list(ref[3].iters_per_level) == list(got[3].iters_per_level)
        assert all(np.array_equal(a, b) for a, b in zip(ref[3].current_idx_per_level, got[3].current_idx_per_level))


@pytest.mark.parametrize("n", sorted(CASES))
def test_restatement_scales_exactly_with_a_weight_of_two(bunny, n):
    """w == 2 with ls and ld doubled: the unweighted tables and iteration counts bit for bit, exactly twice the q trace --
    a scale by a power of two commutes with every product, sum, comparison and quotient of the build"""
    L = CASES[n]
    X, _, idx = draw(bunny, n, L)
    ref = wbuild(X, L, LS, LD, X[idx], None)
    got = wbuild(X, L, 2 * LS, 2 * LD, X[idx], np.full(n, 2.0))
    for a, b in zip(ref[:3], got[:3]):
        assert np.array_equal(a, b)
    assert list(ref[3].iters_per_level) == list(got[3].iters_per_level)
    assert np.array_equal(2.0 * ref[3].q, got[3].q)


def test_a_zero_weight_is_an_absent_point_in_the_restatement(bunny):
    X, c, idx = draw(bunny, 700, 2)
    w = c.astype(np.float64)
    extra = np.r_[X[:30] + 1e-3, X[:30] + 10.0]                       # inside the cloud, and where every pdf underflows
    a = wbuild(X, 2, 0.0, LD, X[idx], w, max_iters_per_level=4)
    b = wbuild(np.r_[X, extra], 2, 0.0, LD, X[idx], np.r_[w, np.zeros(60)], max_iters_per_level=4)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_allclose(u, v, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(a[3].q, b[3].q, rtol=1e-12)


# ---- the mirrors, against stand-ins for the context ----------------------------------------------------------------------
class _Untouchable:
    """a context that fails the test if anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the weights were checked" % name)


class _Built(Exception):
    """raised by the recording context where the build would start: everything of interest has been recorded by then"""


class _Rec:
    """a recording stand-in for the context, up to the build"""
    tree_dtype = np.dtype(np.float64)

    def __init__(self):
        self.calls = []

    def set_points(self, P):
        self.calls.append(("points", len(P)))

    def tree_set_source_weights(self, w):
        self.calls.append(("weights", [float(v) for v in w]))

    def set_points_batch(self, clouds, **kw):
        self.calls.append(("points_batch", [len(c) for c in clouds],
                           {k: [None if w is None else [float(v) for v in w] for w in v] for k, v in kw.items()}))

    def tree_set_precision(self, dt):
        pass

    def tree_build(self, *a, **k):
        raise _Built()

    def tree_build_batch(self, *a, **k):
        raise _Built()


BAD = {"length": np.ones(49), "negative": np.r_[np.ones(49), -1e-3], "nan": np.r_[np.ones(49), np.nan],
       "infinite": np.r_[np.ones(49), np.inf], "all zero": np.zeros(50), "shape": np.ones((50, 1))}


@pytest.mark.parametrize("what", sorted(BAD))
def test_mirrors_refuse_bad_source_weights_before_touching_the_library(what):
    from hgmm_amd.hgmm import hgmm_gpu as H
    bad = BAD[what]
    P = np.random.RandomState(0).rand(50, 3)
    ctx = _Untouchable()
    with pytest.raises(ValueError, match="weights"):
        H.buildGMMTree(P, 1, 20, 1e-4, ctx=ctx, weights=bad)
    with pytest.raises(ValueError, match="weights"):
        H.buildGMMTree(H.WeightedPoints(P, bad), 1, 20, 1e-4, ctx=ctx)
    with pytest.raises(ValueError, match="weights"):
        H.GMMTree(P, tree_level=1, ctx=ctx, source_weights=bad)
    with pytest.raises(ValueError, match="weights"):
        H.GMMTree(H.WeightedPoints(P, bad), tree_level=1, ctx=ctx)
    with pytest.raises(ValueError, match="weights"):
        H.GMMTree(None, tree_level=1, ctx=ctx).set_source(P, weights=bad)
    with pytest.raises(ValueError, match="weights"):
        H.registration_gmmtree(P, P, tree_level=1, ctx=ctx, source_weights=bad)
    with pytest.raises(ValueError, match="weights"):
        H.registration_gmmtree_batch([(P, P), (P, P)], tree_level=1, ctx=ctx, source_weights=[None, bad])
    with pytest.raises(ValueError, match="source_weights"):
        H.registration_gmmtree_batch([(P, P), (P, P)], tree_level=1, ctx=ctx, source_weights=[np.ones(50)])
    with pytest.raises(ValueError, match="source_weights"):
        H.GMMTree(None, tree_level=1, ctx=ctx, source_weights=np.ones(50))


def test_source_weight_arguments():
    from hgmm_amd import Context
    from hgmm_amd.hgmm import hgmm_gpu as H
    assert inspect.signature(H.buildGMMTree).parameters["weights"].default is None
    assert inspect.signature(H.GMMTree.__init__).parameters["source_weights"].default is None
    assert list(inspect.signature(H.GMMTree.set_source).parameters) == ["self", "source", "weights"]
    assert inspect.signature(H.registration_gmmtree_batch).parameters["source_weights"].default is None
    assert list(inspect.signature(Context.tree_set_source_weights).parameters) == ["self", "w"]
    assert list(inspect.signature(Context.tree_set_source_weights_batch).parameters) == ["self", "weights"]
    assert list(inspect.signature(Context.set_points_batch).parameters) == ["self", "clouds", "weights"]
    assert inspect.signature(Context.set_points_batch).parameters["weights"].default is None
    assert "SOURCE" in H.WeightedPoints.__doc__ and "dropped" in H.WeightedPoints.__doc__


def _calls_up_to_the_build(fn, rec):
    with pytest.raises(_Built):
        fn()
    return rec.calls


def test_mirrors_upload_the_cloud_before_its_weights():
    """the cloud goes first (a new cloud drops the previous one's weights in the library), its weights after it, and a
    cloud without weights makes no weight call at all; a WeightedPoints source brings its weights, an explicit argument
    takes precedence"""
    from hgmm_amd.hgmm import hgmm_gpu as H
    P = np.random.RandomState(1).rand(20, 3)
    w = np.arange(20.0) + 1
    want = [("points", 20), ("weights", list(w))]
    for fn in (lambda r: H.buildGMMTree(P, 1, 20, 1e-4, ctx=r, weights=w),
               lambda r: H.buildGMMTree(H.WeightedPoints(P, w), 1, 20, 1e-4, ctx=r),
               lambda r: H.buildGMMTree(H.WeightedPoints(P, np.ones(20)), 1, 20, 1e-4, ctx=r, weights=w),
               lambda r: H.GMMTree(P, tree_level=1, ctx=r, source_weights=w),
               lambda r: H.GMMTree(H.WeightedPoints(P, w), tree_level=1, ctx=r),
               lambda r: H.GMMTree(None, tree_level=1, ctx=r).set_source(P, w),
               lambda r: H.GMMTree(None, tree_level=1, ctx=r).set_source(H.WeightedPoints(P, w)),
               lambda r: H.registration_gmmtree(P, P, tree_level=1, ctx=r, source_weights=w),
               lambda r: H.registration_gmmtree(H.WeightedPoints(P, w), H.WeightedPoints(P, np.ones(20)), tree_level=1, ctx=r)):
        rec = _Rec()
        assert _calls_up_to_the_build(lambda: fn(rec), rec) == want
    for fn in (lambda r: H.buildGMMTree(P, 1, 20, 1e-4, ctx=r),
               lambda r: H.GMMTree(P, tree_level=1, ctx=r),
               lambda r: H.registration_gmmtree(P, H.WeightedPoints(P, w), tree_level=1, ctx=r)):
        rec = _Rec()
        assert _calls_up_to_the_build(lambda: fn(rec), rec) == [("points", 20)]


def test_batch_mirror_takes_a_list_of_source_weights():
    from hgmm_amd.hgmm import hgmm_gpu as H
    rs = np.random.RandomState(2)
    A, B_, C_ = rs.rand(20, 3), rs.rand(30, 3), rs.rand(25, 3)
    wa, wc = np.arange(20.0) + 1, np.arange(25.0) + 2
    rec = _Rec()
    _calls_up_to_the_build(lambda: H.registration_gmmtree_batch([(A, A), (B_, B_), (C_, C_)], tree_level=1, ctx=rec,
                                                               source_weights=[wa, None, wc]), rec)
    assert rec.calls == [("points_batch", [20, 30, 25], {"weights": [list(wa), None, list(wc)]})]
    # a WeightedPoints source brings its own; an explicit entry takes precedence
    rec = _Rec()
    _calls_up_to_the_build(lambda: H.registration_gmmtree_batch(
        [(H.WeightedPoints(A, wa), A), (B_, B_), (H.WeightedPoints(C_, np.ones(25)), C_)], tree_level=1, ctx=rec,
        source_weights=[None, None, wc]), rec)
    assert rec.calls == [("points_batch", [20, 30, 25], {"weights": [list(wa), None, list(wc)]})]
    # no weights anywhere: the call every earlier version made
    rec = _Rec()
    _calls_up_to_the_build(lambda: H.registration_gmmtree_batch([(A, A), (B_, H.WeightedPoints(B_, np.ones(30)))], tree_level=1,
                                                               ctx=rec), rec)
    assert rec.calls == [("points_batch", [20, 30], {})]


def test_batch_mirror_builds_a_large_pair_serially_under_its_weights(monkeypatch):
    """pairs of >= BATCH_MAX_POINTS points leave the batch: their GMMTree gets the pair's source weights"""
    from hgmm_amd.hgmm import hgmm_gpu as H
    monkeypatch.setattr(H, "BATCH_MAX_POINTS", 25)
    rs = np.random.RandomState(3)
    A, B_ = rs.rand(20, 3), rs.rand(30, 3)
    wb = np.arange(30.0) + 1
    rec = _Rec()
    _calls_up_to_the_build(lambda: H.registration_gmmtree_batch([(A, A), (B_, B_)], tree_level=1, ctx=rec,
                                                               source_weights=[None, wb]), rec)
    assert rec.calls == [("points", 30), ("weights", list(wb))]


def test_entries_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    lib = hgmm_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    for name in ("hgmm_tree_set_source_weights", "hgmm_tree_set_source_weights_batch"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) >= 3, name
    # the header names the reference statements that change, and who ignores the weights
    doc = header[header.index("Per-point weights of the SOURCE"):header.index("int hgmm_tree_set_source_weights(")]
    for word in ("gmmTreeEStep", "mlEstimator", "logLikelihoodValue", "IGNORED", "hgmm_tree_estep", "flat", "communicator"):
        assert word in doc, word
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hgmm_tree_set_source_weights" in integration and "hgmm_tree_set_source_weights_batch" in integration
