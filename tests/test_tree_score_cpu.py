"""CPU-only checks of the tree score's surface: the two C entries are declared, exported and bound; the host-side helpers
(node_level, tree_score_from_summary) on hand-made input; the new methods and keyword arguments exist with defaults that
leave the old return shapes.  What the entries compute is tested on the GPU (tests/test_tree_score_gpu.py)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    return hgmm_amd.load_library()


def test_score_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("hgmm_tree_score", 10), ("hgmm_tree_score_batch", 8)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, "%s is not declared in include/hgmm.h" % name
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == n_args
        assert header.count(name) >= 2                             # documented in the comment, not only declared
    assert re.search(r"HGMM_K_TREE_SCORE\s*=\s*13", header)
    from hgmm_amd._native import CHI2_3_99, KERNEL_IDS
    assert KERNEL_IDS["tree_score"] == 13
    assert CHI2_3_99 == 11.344866730144373


def test_node_level():
    from hgmm_amd.hgmm.hgmm_gpu import node_level
    first = [8 * (8 ** l - 1) // 7 for l in range(7)]            # 0, 8, 72, 584, 4680, 37448, 299592
    for l in range(6):
        assert node_level(first[l]) == l and node_level(first[l + 1] - 1) == l
    out = node_level(np.array([0, 7, 8, 71, 72, 583, 584, 4679, 4680, 299591], dtype=np.int32))
    assert out.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 5]


def test_tree_score_from_summary():
    from hgmm_amd.hgmm.hgmm_gpu import TreeScore, tree_score_from_summary
    assert TreeScore._fields == ("fitness", "inlier_rmse", "mahalanobis_rms", "mean_log_density", "n_points", "n_inliers",
                                 "n_dead", "n_above_leaf", "node", "maha2", "logp")
    node = np.arange(4, dtype=np.int32)
    sc = tree_score_from_summary([200.0, 50.0, 450.0, 0.02, -125.0, 7.0, 30.0, 0.0], {"node": node})
    assert sc.fitness == 0.25 and sc.n_points == 200 and sc.n_inliers == 50 and sc.n_dead == 7 and sc.n_above_leaf == 30
    assert sc.mahalanobis_rms == 3.0 and sc.inlier_rmse == 0.02 and sc.mean_log_density == -2.5
    assert sc.node is node and sc.maha2 is None and sc.logp is None
    assert all(isinstance(v, (int, float)) for v in sc[:8])
    # no inlier: nothing to average -- fitness 0 and "infinitely far", never NaN, and no floating-point warning
    with np.errstate(all="raise"):
        none = tree_score_from_summary(np.array([200.0, 0.0, 0.0, 0.0, 0.0, 200.0, 0.0, 0.0]))
    assert none.fitness == 0.0 and none.n_inliers == 0 and none.n_dead == 200
    assert none.inlier_rmse == np.inf and none.mahalanobis_rms == np.inf and none.mean_log_density == -np.inf
    assert not any(np.isnan(v) for v in none[:8])
    assert none.node is None
    assert "inlier" in tree_score_from_summary.__doc__ and "NaN" in tree_score_from_summary.__doc__


def test_new_methods_and_keywords_keep_the_old_defaults():
    from hgmm_amd import Context
    from hgmm_amd._native import CHI2_3_99
    from hgmm_amd.hgmm import hgmm_gpu
    from hgmm_amd import replicas
    sig = inspect.signature(Context.tree_score).parameters
    assert [k for k in sig][1:] == ["rot", "t", "scale", "lambda_c", "maha2_max", "want"]
    assert sig["rot"].default is None and sig["t"].default is None and sig["scale"].default == 1.0
    assert sig["lambda_c"].default == 0.01 and sig["maha2_max"].default == CHI2_3_99
    assert tuple(sig["want"].default) == ("node", "maha2", "logp")
    sig = inspect.signature(Context.tree_score_batch).parameters
    assert [k for k in sig][1:] == ["rot", "t", "scale", "lambda_c", "maha2_max"]
    sig = inspect.signature(hgmm_gpu.GMMTree.score).parameters
    assert [k for k in sig][1:] == ["target", "transformation", "maha2_max", "per_point"]
    assert sig["transformation"].default is None and sig["maha2_max"].default == CHI2_3_99 and sig["per_point"].default is True
    assert "registration" in hgmm_gpu.GMMTree.score.__doc__ and "rounding" in hgmm_gpu.GMMTree.score.__doc__
    assert list(inspect.signature(hgmm_gpu.GMMTree.predict).parameters)[1:] == ["points"]
    assert inspect.signature(hgmm_gpu.GMMTree.registration).parameters["return_score"].default is False
    assert inspect.signature(hgmm_gpu.registration_gmmtree).parameters["return_score"].default is False
    assert inspect.signature(hgmm_gpu.registration_gmmtree_batch).parameters["score"].default is False
    assert inspect.signature(replicas.register_pairs).parameters["score"].default is False
    # the result types: MstepResult stays (transformation, q); the scored one adds a third field
    assert hgmm_gpu.MstepResult._fields == ("transformation", "q")
    assert hgmm_gpu.ScoredResult._fields == ("transformation", "q", "score")
