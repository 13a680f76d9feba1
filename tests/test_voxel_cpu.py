"""The host side of the device voxel down-sample (no GPU): the new arguments default to the old behaviour, the host function
-- the DEFINITION the device path is held to in tests/test_voxel_gpu.py -- returns what it returned before, and the C header
states the semantics the device path implements."""
import inspect
import os
import re

import numpy as np

from conftest import ROOT


def test_new_arguments_default_to_none():
    from hgmm_amd.pointcloud_io import voxel_down_sample
    from hgmm_amd.hgmm.hgmm_gpu import prepare_source_and_target_rigid_3d, registration_gmmtree, registration_gmmtree_batch
    from hgmm_amd.gmm_waymo.run_gmm_stream import run_stream
    assert inspect.signature(voxel_down_sample).parameters["ctx"].default is None
    assert inspect.signature(run_stream).parameters["ctx"].default is None
    assert inspect.signature(prepare_source_and_target_rigid_3d).parameters["ctx"].default is None
    assert inspect.signature(registration_gmmtree_batch).parameters["voxel_size"].default is None
    # registration_gmmtree's parameter list is pinned (tests/test_tree_multistart_cpu.py): like target_weights= and
    # source_weights=, voxel_size= is a keyword it takes out of **kargs, with None as its default
    assert "voxel_size" not in inspect.signature(registration_gmmtree).parameters
    assert 'kargs.pop("voxel_size", None)' in inspect.getsource(registration_gmmtree)
    assert "``voxel_size=``" in registration_gmmtree.__doc__
    assert list(inspect.signature(voxel_down_sample).parameters)[:3] == ["points", "voxel_size", "return_counts"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_host_function_is_what_it_was():
    from hgmm_amd.pointcloud_io import voxel_down_sample
    # 1: three voxels in lexicographic order; rows 0, 1, 3 share a voxel (sums exact: binary fractions)
    P = np.array([[0.375, 0.125, 0.375], [0.375, 0.25, 0.0], [2.5, 0.0, 0.0], [0.0, 0.0, 0.0],
                  [1.25, 1.0, 0.75], [1.25, 1.0, 0.75]])
    cent, cnt = voxel_down_sample(P, 1.0, return_counts=True)
    assert np.array_equal(bits(cent), bits([[0.25, 0.125, 0.125], [1.25, 1.0, 0.75], [2.5, 0.0, 0.0]]))
    assert cnt.dtype == np.int64 and list(cnt) == [3, 2, 1]
    alone = voxel_down_sample(P, 1.0)
    assert isinstance(alone, np.ndarray) and np.array_equal(bits(alone), bits(cent))
    assert np.array_equal(bits(voxel_down_sample(P, 1.0, ctx=None)), bits(cent))
    # 2: a voxel that holds only -0.0 comes out as +0.0 (the sums start from a zeroed array)
    Z = np.array([[-1.0, -1.0, -1.0], [-0.0, -0.0, -0.0], [1.0, 1.0, 1.0]])
    cent, cnt = voxel_down_sample(Z, 0.5, True)
    assert np.array_equal(bits(cent), bits([[-1.0] * 3, [0.0] * 3, [1.0] * 3])) and list(cnt) == [1, 1, 1]
    # 3: float32 input is widened; the origin is 0.25 - 0.25 = 0, so the point ON a voxel face (2.0 = 4 v) belongs to the
    #    voxel above the face and its float32 neighbour below to the one beneath; the mean of rows 0 and 2 is one float64
    #    addition and one division
    below = np.nextafter(np.float32(2.0), np.float32(0.0))
    F = np.array([[0.25, 0.0, 0.0], [2.0, 0.0, 0.0], [0.3, 0.0, 0.0], [below, 0.0, 0.0]], np.float32)
    cent, cnt = voxel_down_sample(F, 0.5, True)
    b = np.float64(np.float32(0.3))
    assert np.array_equal(bits(cent), bits([[(0.25 + b) / 2.0, 0.0, 0.0], [np.float64(below), 0.0, 0.0], [2.0, 0.0, 0.0]]))
    assert list(cnt) == [2, 1, 1]


def test_header_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    m = re.search(r"/\* ---- voxel-grid down-sample.*?\*/", header, flags=re.S)
    assert m, "include/hgmm.h has no voxel-grid down-sample section"
    text = " ".join(m.group(0).split())
    for phrase in ("+0.0", "ASCENDING POINT INDEX", "floor((P - origin) / voxel)", "REFUSALS", "non-finite", "2^63", "2^31",
                   "HGMM_ERR_STATE", "HGMM_K_VOXEL", "hgmm_gpu.py:786", "run_gmm_static.py:28", "waymoutils.py:99",
                   "gmmreg.py:203-204"):
        assert phrase in text, phrase
    assert re.search(r"HGMM_K_VOXEL\s*=\s*15\b", header) and re.search(r"HGMM_K_COUNT\s*=\s*16\b", header)
    for name in ("hgmm_voxel_downsample_f64", "hgmm_voxel_downsample_f32", "hgmm_voxel_downsample_batch_f64",
                 "hgmm_voxel_downsample_batch_f32", "hgmm_voxel_downsample_get"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def test_kernel_id():
    from hgmm_amd._native import KERNEL_IDS
    assert KERNEL_IDS["voxel"] == 15


def test_weights_next_to_a_voxel_size_are_refused_before_any_device_work():
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints, _voxel_pairs
    import pytest
    P = np.zeros((4, 3))
    with pytest.raises(ValueError):
        _voxel_pairs(None, [(P, P)], 0.1, [np.ones(4)])
    with pytest.raises(ValueError):
        _voxel_pairs(None, [(WeightedPoints(P, np.ones(4)), P)], 0.1, [])
