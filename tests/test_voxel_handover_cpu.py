"""The host-side bookkeeping of the voxel hand-over, without a GPU: VoxelResult / VoxelCloud against a stub context (serial
staleness, len, count), the identity de-duplication of ``_voxel_pairs`` and the refusal of explicit weights next to a
VoxelCloud.  (That header, exports and bindings agree on the new entries is test_abi_cpu.py's business.)"""
import numpy as np
import pytest


class StubContext:
    """What VoxelResult / _voxel_pairs ask of a Context: a voxel result described by (m, n, serial)."""

    def __init__(self):
        self.serial = 0
        self.m, self.n = [], []
        self.calls = []

    def voxel_result_info(self):
        return list(self.m), list(self.n), self.serial

    def voxel_down_sample_batch(self, clouds, voxel_size, download=True):
        from hgmm_amd import VoxelResult
        assert download is False
        self.calls.append(list(clouds))
        self.n = [len(c) for c in clouds]
        self.m = [(len(c) + 1) // 2 for c in clouds]
        self.serial += 1
        return VoxelResult(self)

    def voxel_down_sample_get(self):
        M = sum(self.m)
        return np.zeros((M, 3)), np.ones(M, np.int64)


def cloud(n, seed=0):
    return np.random.RandomState(seed).rand(n, 3)


def test_result_and_cloud_bookkeeping():
    from hgmm_amd import HgmmError
    ctx = StubContext()
    res = ctx.voxel_down_sample_batch([cloud(10), cloud(7)], 0.1, download=False)
    assert len(res) == 2 and res.m == [5, 4] and res.n == [10, 7] and res.serial == 1
    a, b = res.member(0), res.member(1)
    assert (len(a), a.count, a.shape, a.index) == (5, 10, (5, 3), 0) and (len(b), b.count) == (4, 7)
    assert a.dtype == np.float64 and a.ctx is ctx
    assert [len(v) for v in res.members()] == [5, 4]
    with pytest.raises(IndexError):
        res.member(2)
    with pytest.raises(IndexError):
        res.member(-1)
    cent, cnt = b.get()
    assert cent.shape == (4, 3) and cnt.shape == (4,)
    a.check(ctx)
    with pytest.raises(HgmmError, match="another context"):
        a.check(StubContext())
    # the next down-sample of the context makes every name of the old result stale
    newer = ctx.voxel_down_sample_batch([cloud(3)], 0.1, download=False)
    for use in (a.check, b.get, res.get, res.check, a.to_host):
        with pytest.raises(HgmmError, match="down-sampled something else since"):
            use()
    newer.member(0).check(ctx)
    assert len(newer.member(0)) == 2


def test_voxel_pairs_merge_by_identity_only():
    from hgmm_amd.hgmm.hgmm_gpu import VoxelCloud, _voxel_pairs
    ctx = StubContext()
    a, b, c = cloud(10, 1), cloud(8, 2), cloud(6, 3)
    pairs = _voxel_pairs(ctx, [(a, b), (b, c)], 0.1, [])
    assert len(ctx.calls) == 1 and len(ctx.calls[0]) == 3
    assert all(x is y for x, y in zip(ctx.calls[0], (a, b, c)))
    assert all(isinstance(v, VoxelCloud) for p in pairs for v in p)
    assert [(s.index, t.index) for s, t in pairs] == [(0, 1), (1, 2)]
    assert [(len(s), t.count) for s, t in pairs] == [(5, 8), (4, 6)]
    # equal but distinct arrays are NOT merged
    pairs = _voxel_pairs(ctx, [(a, b), (b.copy(), c)], 0.1, [])
    assert len(ctx.calls[-1]) == 4 and [(s.index, t.index) for s, t in pairs] == [(0, 1), (2, 3)]
    # a pair of one array with itself is one member
    pairs = _voxel_pairs(ctx, [(a, a)], 0.1, [])
    assert len(ctx.calls[-1]) == 1 and [(s.index, t.index) for s, t in pairs] == [(0, 0)]


def test_mixed_sides_download_each_result_once():
    from hgmm_amd.hgmm.hgmm_gpu import _voxels_to_host
    ctx = StubContext()
    res = ctx.voxel_down_sample_batch([cloud(10), cloud(8), cloud(6)], 0.1, download=False)
    gets = []
    inner = ctx.voxel_down_sample_get
    ctx.voxel_down_sample_get = lambda: gets.append(1) or inner()
    host = cloud(4)
    weights = [None] * 4
    out = _voxels_to_host([res.member(2), host, res.member(0), res.member(2)], weights)
    assert len(gets) == 1 and out[1] is host and weights[1] is None
    assert [len(o) for o in out] == [3, 4, 5, 3] and [None if w is None else (w.dtype, len(w)) for w in weights] == \
        [(np.float64, 3), None, (np.float64, 5), (np.float64, 3)]
    # all members, or none: the list as it is, nothing downloaded
    members = res.members()
    assert _voxels_to_host(members, [None] * 3) is members and _voxels_to_host([host], [None])[0] is host and len(gets) == 1


def test_flat_weight_sum_of_rounded_counts():
    """The argument behind hgmm_voxel_to_points' flat weight sum.  The flat weights are the float32 values (float)count and
    hgmm_flat_set_weights sums them in float64 in index order.  Each is an integer, so the sum is exact in any order and
    equals the integer sum of (uint64)(float)count -- what the hand-over's kernel adds up when a count can reach 2^24 --;
    below 2^24 the conversion is exact and the sum is the raw point count, which needs no device sum at all."""
    rs = np.random.RandomState(11)
    small = rs.randint(1, 1 << 24, size=5000).astype(np.int64)
    assert np.array_equal(small.astype(np.float32).astype(np.int64), small)
    assert float(np.sum(small.astype(np.float32).astype(np.float64))) == float(small.sum())
    big = np.concatenate([small, np.array([(1 << 24) + 1, (1 << 25) + 1, (1 << 30) + 1, (1 << 30) + 129], np.int64)])
    as_f32 = big.astype(np.float32)
    assert not np.array_equal(as_f32.astype(np.int64), big)                     # (these counts DO round: by -1, -1, -1, -1)
    index_order = 0.0
    for v in as_f32.astype(np.float64):                                      # hgmm_flat_set_weights' loop
        index_order += v
    integer_sum = int(as_f32.astype(np.uint64).sum())                        # the kernel's sum, in any order
    assert index_order == float(integer_sum) and integer_sum != int(big.sum())
    assert float(np.sum(rs.permutation(as_f32).astype(np.float64))) == index_order


def test_explicit_weights_next_to_voxels_are_refused():
    from hgmm_amd.hgmm.hgmm_gpu import (WeightedPoints, _target_weights, _voxel_pairs, buildGMMTree, registration_gmmtree,
                                        registration_gmmtree_batch)
    ctx = StubContext()
    res = ctx.voxel_down_sample_batch([cloud(10), cloud(8)], 0.1, download=False)
    s, t = res.member(0), res.member(1)
    calls = len(ctx.calls)
    assert _target_weights(s) is None
    with pytest.raises(ValueError, match="VoxelCloud"):
        _target_weights(s, np.ones(len(s)))
    with pytest.raises(ValueError, match="VoxelCloud"):
        buildGMMTree(s, 1, 20.0, 1.0e-4, ctx=ctx, weights=np.ones(len(s)))
    with pytest.raises(ValueError, match="VoxelCloud"):
        registration_gmmtree(s, t, ctx=ctx, tree_level=1, target_weights=np.ones(len(t)))
    with pytest.raises(ValueError, match="VoxelCloud"):
        registration_gmmtree(s, t, ctx=ctx, tree_level=1, source_weights=np.ones(len(s)))
    with pytest.raises(ValueError, match="VoxelCloud"):
        registration_gmmtree_batch([(s, t)], ctx=ctx, tree_level=1, source_weights=[np.ones(len(s))])
    with pytest.raises(ValueError, match="VoxelCloud"):
        registration_gmmtree_batch([(s, t)], ctx=ctx, tree_level=1, target_weights=[np.ones(len(t))])
    # ... as they are next to voxel_size=, and a cloud that is down-sampled already takes no voxel size
    with pytest.raises(ValueError):
        _voxel_pairs(ctx, [(cloud(5), cloud(5))], 0.1, [np.ones(5)])
    with pytest.raises(ValueError):
        _voxel_pairs(ctx, [(WeightedPoints(cloud(5), np.ones(5)), cloud(5))], 0.1, [])
    with pytest.raises(ValueError, match="down-sampled already"):
        _voxel_pairs(ctx, [(s, cloud(5))], 0.1, [])
    assert len(ctx.calls) == calls                                  # (every refusal came before the context was touched)
