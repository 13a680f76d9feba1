"""Per-point weights of the registration target (hgmm_tree_set_target_weights), the parts that need no GPU: the
float64 E-step the GPU tests compare against (oracle.hgmm_tree.reg_e_step(w=...)) is the unweighted E-step bit for bit
when every weight is 1 and the E-step of a cloud with its points repeated when the weights are integers;
voxel_down_sample hands out the counts; the mirrors refuse bad weights before they touch the library; the two C entries
are declared, exported and bound."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import hgmm_tree


@pytest.fixture(scope="module")
def records():
    return {2: load_golden("hgmm_reg_L2.npz"), 4: load_golden("hgmm_reg_L4.npz")}


@pytest.mark.parametrize("L", [2, 4])
def test_restatement_with_unit_weights_is_the_oracle_bit_for_bit(records, L):
    """``w = None`` runs the unweighted statements themselves and is the reference; ``w = ones`` runs the multiply and must
    change no bit, in the E-step and along the register loop (the build: tests/test_tree_source_weights_cpu.py)."""
    g = records[L]
    tree = (g["pi"], g["mu"], g["cov"], L, float(g["lambda_c"]))
    for deg in (10, 30):
        X = g["rot%d_target" % deg]
        ref = hgmm_tree.reg_e_step(X, *tree)
        got = hgmm_tree.reg_e_step(X, *tree, np.ones(len(X)))
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)
    # the loop around it
    X = g["rot10_target"]
    o_rot, o_t, o_q, o_tr = hgmm_tree.register(X, *tree, 3, 1e-4)
    rot, t, q, tr = hgmm_tree.register(X, *tree, 3, 1e-4, np.ones(len(X)))
    assert len(tr) == len(o_tr) and np.array_equal(rot, o_rot) and np.array_equal(t, o_t) and np.array_equal(q, o_q)
    for a, b in zip(tr, o_tr):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("L", [2, 4])
def test_integer_weights_are_repeated_points(records, L):
    """w_i = k_i in {0, 1, 2, 3}: the weighted E-step against the unweighted E-step of the cloud with point i present k_i
    times.  The two differ in the order of the additions only: each of m0, m1, m2 within 1e-12 of its array's largest
    magnitude (measured: at most 2.5e-15)."""
    g = records[L]
    lc = float(g["lambda_c"])
    X = g["rot10_target"]
    k = np.random.RandomState(11).randint(0, 4, len(X))
    assert (k == 0).sum() > 400 and (k == 3).sum() > 400
    got = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, k.astype(np.float64))
    ref = hgmm_tree.reg_e_step(np.repeat(X, k, axis=0), g["pi"], g["mu"], g["cov"], L, lc)
    for name, a, b in zip(("m0", "m1", "m2"), got, ref):
        err = np.abs(a - b).max() / np.abs(b).max()
        print("L=%d %s: %d zero weights, largest difference %.3g of the largest magnitude" % (L, name, (k == 0).sum(), err))
        assert err <= 1e-12, name


def test_gate_and_weights_compose_in_the_restatement(records):
    """the gate decides on the pair, the weight scales what passes: a 0/1 weight is a point left out"""
    g = records[2]
    L, lc = 2, float(g["lambda_c"])
    X = g["rot10_target"]
    e = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, gate=16.0, report=True)
    got = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, np.ones(len(X)), 16.0)
    for a, b in zip((e.m0, e.m1, e.m2), got):
        assert np.array_equal(a, b)
    keep = np.random.RandomState(3).uniform(size=len(X)) < 0.7
    sub = hgmm_tree.reg_e_step(X[keep], g["pi"], g["mu"], g["cov"], L, lc, None, 16.0)
    got = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, keep.astype(np.float64), 16.0)
    for a, b in zip(sub, got):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(b).max())


def test_voxel_down_sample_returns_the_counts(bunny):
    from hgmm_amd.pointcloud_io import voxel_down_sample
    P = bunny.astype(np.float64)
    old = voxel_down_sample(P, 0.004)
    assert isinstance(old, np.ndarray) and old.shape[1] == 3          # the default return is what it was
    cen, cnt = voxel_down_sample(P, 0.004, return_counts=True)
    assert np.array_equal(cen, old)                                   # bitwise
    assert cnt.shape == (len(cen),) and cnt.dtype == np.int64 and cnt.min() >= 1 and cnt.sum() == len(P)
    assert np.array_equal(voxel_down_sample(P, 0.004, False), old)
    assert inspect.signature(voxel_down_sample).parameters["return_counts"].default is False
    # the count-weighted mean of the centroids is the cloud's mean
    np.testing.assert_allclose((cen * cnt[:, None]).sum(axis=0) / cnt.sum(), P.mean(axis=0), rtol=1e-12)


class _Untouchable:
    """a context that fails the test if anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the weights were checked" % name)


BAD = {"length": np.ones(49), "negative": np.r_[np.ones(49), -1e-3], "nan": np.r_[np.ones(49), np.nan],
       "infinite": np.r_[np.ones(49), np.inf], "all zero": np.zeros(50), "shape": np.ones((50, 1))}


@pytest.mark.parametrize("what", sorted(BAD))
def test_mirrors_refuse_bad_weights_before_touching_the_library(what):
    from hgmm_amd.hgmm import hgmm_gpu as H
    bad = BAD[what]
    P = np.random.RandomState(0).rand(50, 3)
    ctx = _Untouchable()
    gt = H.GMMTree(None, tree_level=1, ctx=ctx)
    with pytest.raises(ValueError, match="weights"):
        gt.registration(P, weights=bad)
    with pytest.raises(ValueError, match="weights"):
        gt.registration(H.WeightedPoints(P, bad))
    with pytest.raises(ValueError, match="weights"):
        H._set_target(ctx, H.WeightedPoints(P, bad))
    with pytest.raises(ValueError, match="weights"):
        H.registration_gmmtree(P, P, tree_level=1, ctx=ctx, target_weights=bad)
    with pytest.raises(ValueError, match="weights"):
        H.registration_gmmtree(P, P, starts=[H.RigidTransformation()], tree_level=1, ctx=ctx, target_weights=bad)
    with pytest.raises(ValueError, match="weights"):
        H.registration_gmmtree_batch([(P, P), (P, P)], tree_level=1, ctx=ctx, target_weights=[None, bad])
    with pytest.raises(ValueError, match="target_weights"):
        H.registration_gmmtree_batch([(P, P), (P, P)], tree_level=1, ctx=ctx, target_weights=[np.ones(50)])


def test_weight_arguments():
    from hgmm_amd import Context
    from hgmm_amd.hgmm import hgmm_gpu as H
    assert H._weights_arg(None, 7) is None
    w = H._weights_arg([0, 1, 2.5], 3)
    assert w.dtype == np.float64 and w.flags["C_CONTIGUOUS"] and list(w) == [0.0, 1.0, 2.5]
    assert list(H._weights_arg(np.array([3, 0, 1], np.int64), 3)) == [3.0, 0.0, 1.0]        # counts as they come
    with pytest.raises(ValueError, match="weight 1 is -1"):
        H._weights_arg([1, -1, -2], 3)                                 # the first offending index is named
    assert inspect.signature(H.GMMTree.registration).parameters["weights"].default is None
    assert inspect.signature(H.registration_gmmtree_batch).parameters["target_weights"].default is None
    assert list(inspect.signature(Context.tree_set_target_weights).parameters) == ["self", "w"]
    assert list(inspect.signature(Context.tree_set_targets_batch).parameters) == ["self", "targets", "weights"]
    assert inspect.signature(Context.tree_set_targets_batch).parameters["weights"].default is None
    assert H.WeightedPoints._fields == ("points", "weights")
    P = np.zeros((3, 3))
    assert H._points(H.WeightedPoints(P, w)) is P
    assert H._target_weights(H.WeightedPoints(P, [1, 1, 1]), w) is not None and list(H._target_weights(H.WeightedPoints(P, [1, 1, 1]), w)) == [0.0, 1.0, 2.5]


def test_set_target_uploads_the_target_before_its_weights():
    """a recording stand-in for the context: the target goes first (a new target drops the previous one's weights in the
    library), its weights after it, and a target without weights makes no weight call at all"""
    from hgmm_amd.hgmm import hgmm_gpu as H

    class Rec:
        def __init__(self):
            self.calls = []

        def tree_set_target(self, t):
            self.calls.append(("target", len(t)))

        def tree_set_target_weights(self, w):
            self.calls.append(("weights", len(w)))

    P = np.random.RandomState(1).rand(20, 3)
    r = Rec()
    H._set_target(r, P)
    H._set_target(r, P, np.ones(20))
    H._set_target(r, H.WeightedPoints(P[:10], np.arange(10.0) + 1))
    H._set_target(r, P)
    assert r.calls == [("target", 20), ("target", 20), ("weights", 20), ("target", 10), ("weights", 10), ("target", 20)]


def test_entries_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    lib = hgmm_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    for name in ("hgmm_tree_set_target_weights", "hgmm_tree_set_target_weights_batch"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) >= 3, name
    # the header says who ignores the weights
    doc = header[header.index("Per-point WEIGHTS"):header.index("int hgmm_tree_set_target_weights(")]
    assert "NOT honoured by the build" in doc and "flat" in doc
