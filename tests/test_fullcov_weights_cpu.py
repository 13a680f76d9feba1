"""Per-point weights of the flat full-covariance fit (hgmm_fullcov_fit_weighted / hgmm_fullcov_estep_weighted), the parts that
need no GPU: the weighted restatement the GPU tests compare against (tests/_fullcov_weight_oracle.py) is the committed oracle
bit for bit without weights and with unit weights, scales exactly with w == 2, is the oracle's fit of the repeated cloud when
the weights are integers and the weighted one-level tree build at J = 8; the mirror refuses bad weights before it touches the
library, makes no weight call for a plain array and the right ones for WeightedPoints / weights= / VoxelCloud; the two C
entries are declared, exported and bound."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import hgmm_tree
from _fullcov_weight_oracle import LD, SIG2, build_flat_fullcov_w, case, e_step_w, init_rows

ITERS = 6
JS = [8, 40, 520]


@pytest.fixture(scope="module")
def cloud(bunny):
    P, w = case(bunny)
    assert len(P) == 1300 and int((w == 0).sum()) == 258 and hgmm_tree.weight_sum(w) == 2541.0
    return P, w


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("J", JS)
def test_restatement_without_weights_and_with_unit_weights_is_the_oracle_bit_for_bit(cloud, J):
    P, _ = cloud
    idx = np.random.RandomState(J).choice(len(P), J, replace=False)
    ref = hgmm_tree.build_flat_fullcov(P, J, 1.0, LD, idx, SIG2, max_iters=ITERS)
    for w in (None, np.ones(len(P))):
        got = build_flat_fullcov_w(P, J, 1.0, LD, idx, SIG2, ITERS, w)
        assert all(np.array_equal(a, b) for a, b in zip(ref, got))


@pytest.mark.parametrize("J", JS)
def test_restatement_scales_exactly_with_a_weight_of_two(cloud, J):
    """w == 2 with ls and ld doubled: tables and labels bit for bit, the q trace exactly doubled"""
    P, _ = cloud
    idx = np.random.RandomState(J).choice(len(P), J, replace=False)
    ref = build_flat_fullcov_w(P, J, 1.0, LD, idx, SIG2, ITERS, None)
    got = build_flat_fullcov_w(P, J, 2.0, 2 * LD, idx, SIG2, ITERS, np.full(len(P), 2.0))
    for a, b in zip(ref[:3], got[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(ref[4], got[4]) and np.array_equal(2.0 * ref[3], got[3])


@pytest.mark.parametrize("J", JS)
def test_integer_weights_are_the_oracle_on_the_repeated_cloud(cloud, J):
    """The fit of (P, w) against oracle.hgmm_tree.build_flat_fullcov of np.repeat(P, w): the two differ in the order of the
    additions only.  Measured: q 3e-14 relative, pi 1e-13 and mu 9e-14 absolute (pi <= 1, |mu| ~ 0.1: a coordinate may be
    near zero), cov 3e-10 relative to |cov| + 1e-14 (the cancellation in m2 / m0 - mu mu^T); asserted with two decimal orders
    of margin over these."""
    P, w = cloud
    c = w.astype(int)
    idx = init_rows(w, J)
    first = np.cumsum(c) - c                                          # the first copy of point i in the repeated cloud
    pi, mu, cov, q, cur = build_flat_fullcov_w(P, J, 1.0, LD, idx, SIG2, ITERS, w)
    o_pi, o_mu, o_cov, o_q, o_cur = hgmm_tree.build_flat_fullcov(np.repeat(P, c, axis=0), J, 1.0, LD, first[idx], SIG2,
                                                                 max_iters=ITERS)
    assert len(q) == len(o_q)
    live = o_pi > 0
    print("J=%d: %d iterations, q %.2g relative, pi %.2g, mu %.2g absolute, cov %.2g relative, %d dead" %
          (J, len(q), _rel(q, o_q), np.abs(pi - o_pi).max(), np.abs(mu - o_mu).max(),
           np.max(np.abs(cov - o_cov) / (np.abs(o_cov) + 1e-14)), int((~live).sum())))
    assert np.array_equal(np.repeat(cur, c), o_cur)                   # every copy of a point is labelled as the point is
    assert np.array_equal(pi == 0.0, o_pi == 0.0)
    np.testing.assert_allclose(q, o_q, rtol=3e-12, atol=0)
    np.testing.assert_allclose(pi, o_pi, rtol=0, atol=1e-11)
    np.testing.assert_allclose(mu, o_mu, rtol=0, atol=9e-12)
    assert float(np.max(np.abs(cov - o_cov) / (np.abs(o_cov) + 1e-14))) < 3e-8


def test_eight_components_are_the_weighted_one_level_tree(cloud):
    """J = 8 is oracle.hgmm_tree.build_tree(P, 1, ..., w=w): labels equal, q to 3e-15 relative measured (asserted at 3e-13)"""
    P, w = cloud
    idx = init_rows(w, 8)
    pi, mu, cov, q, cur = build_flat_fullcov_w(P, 8, 1.0, LD, idx, SIG2, ITERS, w)
    t_pi, t_mu, t_cov, tr = hgmm_tree.build_tree(P, 1, 1.0, LD, idx, SIG2, max_iters_per_level=ITERS, w=w)
    assert list(tr.iters_per_level) == [len(q)]
    assert np.array_equal(tr.current_idx_per_level[0], cur)
    print("q %.2g relative" % _rel(q, tr.q))
    np.testing.assert_allclose(q, tr.q, rtol=3e-13, atol=0)
    np.testing.assert_allclose(pi, t_pi, rtol=1e-12)
    np.testing.assert_allclose(mu, t_mu, rtol=1e-12)
    np.testing.assert_allclose(cov, t_cov, rtol=1e-9)


def test_single_estep_is_the_first_step_of_the_fit(cloud):
    """e_step_w of the initial parameters gives the moments the fit's first M-step takes, and of the fitted parameters
    the last q of the trace"""
    P, w = cloud
    J = 8
    idx = init_rows(w, J)
    m0, m1, m2, cur, _ = e_step_w(P, np.full(J, 1.0 / J), P[idx].copy(), np.tile(np.identity(3) * SIG2, (J, 1, 1)), w)
    pi, mu, cov, q, _ = build_flat_fullcov_w(P, J, 1e-30, LD, idx, SIG2, 1, w)
    assert np.array_equal(pi, m0 / hgmm_tree.weight_sum(w)) and np.array_equal(mu, m1 / m0[:, None])
    assert abs(m0.sum() - 2541.0) < 1e-9
    assert e_step_w(P, pi, mu, cov, w)[4] == pytest.approx(q[-1], rel=1e-13)
    # without weights it is the unweighted E-step, and unit weights change no bit
    a, b = e_step_w(P, pi, mu, cov, None), e_step_w(P, pi, mu, cov, np.ones(len(P)))
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_stop_rule_case_sees_the_weights(cloud):
    """the case of the GPU stop-rule test: under ls = 20 the weighted fit stops after 21 iterations, the unweighted after 17"""
    P, w = cloud
    idx = init_rows(w, 24)
    a = build_flat_fullcov_w(P, 24, 20.0, LD, idx, SIG2, 40, w)
    b = build_flat_fullcov_w(P, 24, 20.0, LD, idx, SIG2, 40, None)
    assert (len(a[3]), len(b[3])) == (21, 17)
    assert hgmm_tree.stop_margins(a[3], [len(a[3])], 20.0).min() >= 0.05


# ---- the mirror, against stand-ins for the context ------------------------------------------------------------------------
class _Untouchable:
    """a context that fails the test if anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the weights were checked" % name)


class _Fitted(Exception):
    """raised by the recording context where the fit would start: everything of interest has been recorded by then"""


class _Rec:
    """a recording stand-in for the context, up to the fit"""
    tree_dtype = np.dtype(np.float64)

    def __init__(self):
        self.calls = []

    def set_points(self, P):
        self.calls.append(("points", len(P)))

    def tree_set_source_weights(self, w):
        self.calls.append(("weights", [float(v) for v in w]))

    def set_points_from_voxels(self, vc, tree_weights=True, flat_weights=False):
        self.calls.append(("voxels", bool(tree_weights), bool(flat_weights)))

    def points_rows(self, rows):
        self.calls.append(("rows", [int(r) for r in rows]))
        return np.zeros((len(rows), 3))

    def tree_set_precision(self, dt):
        pass

    def fullcov_fit(self, *a, **k):
        self.calls.append(("fit", dict(k)))
        raise _Fitted()


def _calls(fn):
    rec = _Rec()
    with pytest.raises(_Fitted):
        fn(rec)
    return rec.calls


BAD = {"length": np.ones(49), "negative": np.r_[np.ones(49), -1e-3], "nan": np.r_[np.ones(49), np.nan],
       "infinite": np.r_[np.ones(49), np.inf], "all zero": np.zeros(50), "shape": np.ones((50, 1))}


@pytest.mark.parametrize("what", sorted(BAD))
def test_mirror_refuses_bad_weights_before_touching_the_library(what):
    from hgmm_amd.hgmm import hgmm_gpu as H
    P = np.random.RandomState(0).rand(50, 3)
    with pytest.raises(ValueError, match="weights"):
        H.fitFullCovGMM(P, 4, ctx=_Untouchable(), weights=BAD[what])
    with pytest.raises(ValueError, match="weights"):
        H.fitFullCovGMM(H.WeightedPoints(P, BAD[what]), 4, ctx=_Untouchable())


def test_mirror_makes_the_weight_calls_the_cloud_asks_for():
    """a plain array: the calls every earlier version made, no weight call and no keyword; WeightedPoints and weights=: the
    cloud, then its weights, then the weighted fit; explicit weights take precedence over the cloud's own"""
    from hgmm_amd.hgmm import hgmm_gpu as H
    P = np.random.RandomState(1).rand(20, 3)
    w = np.arange(20.0) + 1
    assert _calls(lambda r: H.fitFullCovGMM(P, 4, ctx=r)) == [("points", 20), ("fit", {})]
    want = [("points", 20), ("weights", list(w)), ("fit", {"weighted": True})]
    for fn in (lambda r: H.fitFullCovGMM(P, 4, ctx=r, weights=w),
               lambda r: H.fitFullCovGMM(H.WeightedPoints(P, w), 4, ctx=r),
               lambda r: H.fitFullCovGMM(H.WeightedPoints(P, np.ones(20)), 4, ctx=r, weights=w)):
        assert _calls(fn) == want
    # .points gives the unweighted fit
    assert _calls(lambda r: H.fitFullCovGMM(H.WeightedPoints(P, w).points, 4, ctx=r)) == [("points", 20), ("fit", {})]


def test_mirror_hands_a_voxel_cloud_over_on_the_device():
    """a VoxelCloud: handed over with its counts as the source weights, the initial means read back by row number; explicit
    weights next to it are refused before anything is touched"""
    from hgmm_amd import VoxelCloud
    from hgmm_amd.hgmm import hgmm_gpu as H

    class _Result:                                                    # (a member is a name for what lies on the device)
        m, n = [30], [400]

    vc = VoxelCloud(_Result(), 0)
    idx = np.array([3, 1, 4, 1])
    assert len(vc) == 30
    calls = _calls(lambda r: H.fitFullCovGMM(vc, 4, ctx=r, init_idx=idx))
    assert calls == [("voxels", True, False), ("rows", [3, 1, 4, 1]), ("fit", {"weighted": True})]
    with pytest.raises(ValueError, match="VoxelCloud"):
        H.fitFullCovGMM(vc, 4, ctx=_Untouchable(), weights=np.ones(30))


def test_arguments_and_documentation():
    from hgmm_amd import Context
    from hgmm_amd.hgmm import hgmm_gpu as H
    assert inspect.signature(H.fitFullCovGMM).parameters["weights"].default is None
    assert inspect.signature(Context.fullcov_fit).parameters["weighted"].default is False
    assert inspect.signature(Context.fullcov_estep).parameters["weighted"].default is False
    assert list(inspect.signature(Context.fullcov_fit).parameters)[:7] == ["self", "J", "ls", "ld", "init_mu", "sig2", "max_iters"]
    for doc in (H.WeightedPoints.__doc__, H.fitFullCovGMM.__doc__):
        assert "fitFullCovGMM" in doc or "weights" in doc
        assert "dropped" in doc and ".points" in doc


def test_entries_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    lib = hgmm_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    for name, plain in (("hgmm_fullcov_fit_weighted", "hgmm_fullcov_fit"), ("hgmm_fullcov_estep_weighted", "hgmm_fullcov_estep")):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        # the argument list of the unweighted entry
        assert [a for a in getattr(lib, name).argtypes] == [a for a in getattr(lib, plain).argtypes], name
    doc = header[header.index("The same fit and E-step under the SOURCE weights"):header.index("int hgmm_fullcov_fit_weighted(")]
    for word in ("hgmm_tree_set_source_weights", "HGMM_VOXEL_W_TREE", "floor", "arg-max", "m0_j / W", "zero weight",
                 "bit for bit", "HGMM_ERR_STATE", "communicator", "float32", "centroid"):
        assert word in doc, word
    # the sentences that listed the full-covariance entries among those that ignore the source weights
    flat = re.sub(r"\s*\n \*\s*", " ", header)                        # (comment lines joined)
    assert flat.count("the unweighted entries ignore them") == 3 and "`_weighted` honours them" in flat
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hgmm_fullcov_fit_weighted" in integration and "hgmm_fullcov_estep_weighted" in integration
