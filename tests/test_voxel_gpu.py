"""Voxel-grid down-sample on the device (hgmm_voxel_downsample_*, Context.voxel_down_sample[_batch]) against its definition,
the host function ``pointcloud_io.voxel_down_sample(P, v, return_counts=True)`` with ``ctx=None``, and against hand-computed
cases: BIT FOR BIT -- centroids compared as uint64, counts as int64 -- since origin (a min), index (one subtraction, one
division, one floor), order (lexicographic) and centroid (float64 sum in ascending point index from +0.0, one division) are
all fixed by the definition.  Expected values never come from the device path.

Shapes: the smallest at which each step can go wrong -- one point; 255 / 256 / 257 points (one workgroup of the key and
centroid kernels, exactly, and one more); 5 000 points in ONE voxel (a segment that spans workgroups of the sort, one long
walk); 5 000 voxels of one point (M = n); 20 000 points far from the origin at a voxel size that is no binary fraction (ten
2 048-row workgroups of the bounding-box pass, quotients that round); the scans at the reference's two voxel sizes; keys of
63 bits; a batch whose members end inside a bounding-box workgroup."""
import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bun045():
    return np.load(GOLDEN + "/bun045_xyz.npy")


_HOST = {}


def host(P, v, key=None):
    """the definition (computed once per named input and never modified)"""
    from hgmm_amd.pointcloud_io import voxel_down_sample
    if key is None:
        return voxel_down_sample(P, v, True)
    if (key, v) not in _HOST:
        cent, cnt = voxel_down_sample(P, v, True)
        cent.setflags(write=False)
        cnt.setflags(write=False)
        _HOST[(key, v)] = (cent, cnt)
    return _HOST[(key, v)]


def same(got, want):
    """(centroids, counts) bit for bit"""
    gc, gn = got
    wc, wn = want
    assert gc.dtype == np.float64 and gn.dtype == np.int64 and gc.shape == (len(gn), 3)
    assert gn.shape == wn.shape and np.array_equal(gn, wn)
    assert np.array_equal(np.ascontiguousarray(gc).view(np.uint64), np.ascontiguousarray(wc).view(np.uint64))
    return True


HAND = np.array([[0.375, 0.125, 0.375], [0.375, 0.25, 0.0], [2.5, 0.0, 0.0], [0.0, 0.0, 0.0],
                 [1.25, 1.0, 0.75], [1.25, 1.0, 0.75]])
# v = 1: origin -0.5; rows 0, 1, 3 fall into voxel (0,0,0), the identical rows 4, 5 into (1,1,1), row 2 into (3,0,0)
HAND_CENT = np.array([[0.25, 0.125, 0.125], [1.25, 1.0, 0.75], [2.5, 0.0, 0.0]])
HAND_CNT = np.array([3, 2, 1], np.int64)


def boundary_cloud():
    """multiples of 0.125 in [-2, 2] at v = 0.25: every quotient is exact and half of them are whole numbers"""
    return np.random.RandomState(3).randint(-16, 17, size=(300, 3)) * 0.125


def test_hand_computed(ctx):
    assert same(ctx.voxel_down_sample(HAND, 1.0), (HAND_CENT, HAND_CNT))
    # every value is a small binary fraction: the shift is exact, so are the sums, the voxels stay what they were
    assert same(ctx.voxel_down_sample(HAND - 7.25, 1.0), (HAND_CENT - 7.25, HAND_CNT))
    assert same(host(HAND, 1.0), (HAND_CENT, HAND_CNT))


def test_points_on_voxel_faces(ctx):
    P = boundary_cloud()
    assert (np.modf((P - (P.min(0) - 0.125)) / 0.25)[0] == 0).mean() > 0.4
    assert same(ctx.voxel_down_sample(P, 0.25), host(P, 0.25))


def test_sign_of_zero(ctx):
    P = np.array([[-1.0, -1.0, -1.0], [-0.0, -0.0, -0.0], [1.0, 1.0, 1.0]])
    cent, cnt = ctx.voxel_down_sample(P, 0.5)
    assert list(cnt) == [1, 1, 1]
    assert (cent[1].view(np.uint64) == 0).all()              # +0.0, not the -0.0 that went in
    assert same((cent, cnt), host(P, 0.5))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_small_sizes(ctx, n):
    P = np.random.RandomState(n).rand(n, 3)
    assert same(ctx.voxel_down_sample(P, 0.1), host(P, 0.1))


def test_one_voxel_holds_everything(ctx):
    P = np.random.RandomState(5).rand(5000, 3) * 0.5
    cent, cnt = ctx.voxel_down_sample(P, 10.0)
    assert list(cnt) == [5000]
    assert same((cent, cnt), host(P, 10.0))


def test_every_point_its_own_voxel(ctx):
    rs = np.random.RandomState(6)
    i = rs.permutation(5000)
    P = np.stack([i % 20, (i // 20) % 20, i // 400], axis=1) + 0.3 * rs.rand(5000, 3)
    cent, cnt = ctx.voxel_down_sample(P, 1.0)
    assert len(cnt) == 5000 and (cnt == 1).all()
    assert same((cent, cnt), host(P, 1.0))


def test_far_from_the_origin(ctx):
    P = 1000.0 + np.random.RandomState(7).rand(20000, 3)
    assert same(ctx.voxel_down_sample(P, 0.013), host(P, 0.013))


@pytest.mark.parametrize("v,M,largest", [(0.004, 2095, 51), (0.002, 7128, 14)])
def test_scan(ctx, bunny, v, M, largest):
    assert bunny.dtype == np.float32
    cent, cnt = ctx.voxel_down_sample(bunny, v)
    assert len(cnt) == M and cnt.max() == largest and cnt.sum() == 40256
    assert same((cent, cnt), host(bunny, v, "bun000"))


def test_wide_keys(ctx):
    import hgmm_amd
    P = np.array([[0.0, 0.0, 0.0], [3e6, 2e6, 1e6], [1.0, 1.0, 1.0]])           # 3 000 001 x 2 000 001 x 1 000 001 cells: 63 bits
    assert same(ctx.voxel_down_sample(P, 1.0), host(P, 1.0))
    with pytest.raises(hgmm_amd.HgmmError, match="grid"):
        ctx.voxel_down_sample(np.array([[0.0, 0.0, 0.0], [1e7, 1e7, 1e7]]), 1e-3)
    assert same(ctx.voxel_down_sample(HAND, 1.0), (HAND_CENT, HAND_CNT))


def test_refusals_leave_the_context_working(ctx):
    import hgmm_amd
    prev = ctx.voxel_down_sample(HAND, 1.0)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(hgmm_amd.HgmmError):
            ctx.voxel_down_sample(HAND, v)
        assert same(ctx.voxel_down_sample_get(), prev)       # the previous result is still there
        assert same(ctx.voxel_down_sample(HAND, 1.0), (HAND_CENT, HAND_CNT))
    P = np.random.RandomState(8).rand(100, 3)
    P[17, 1] = np.nan
    P[40, 0] = np.inf
    with pytest.raises(hgmm_amd.HgmmError, match="17"):
        ctx.voxel_down_sample(P, 0.1)
    assert same(ctx.voxel_down_sample_get(), prev)
    with pytest.raises(hgmm_amd.HgmmError, match="17"):
        ctx.voxel_down_sample(P.astype(np.float32), 0.1)
    assert same(ctx.voxel_down_sample(HAND, 1.0), (HAND_CENT, HAND_CNT))


def test_sizes_refused_on_entry(ctx):
    """n < 1 and n >= 2^31 through the C ABI itself (the Python wrapper refuses an empty array before the library sees it);
    both are refused on the count alone, before a row is read."""
    import ctypes
    HGMM_ERR_ARG = -2                     # include/hgmm.h
    prev = ctx.voxel_down_sample(HAND, 1.0)
    m = (ctypes.c_int64 * 1)()
    for n in (0, -3, 1 << 31):
        assert ctx.lib.hgmm_voxel_downsample_f64(ctx.h, HAND.ctypes.data_as(ctypes.c_void_p), n, 1.0, m) == HGMM_ERR_ARG
        assert ctx.lib.hgmm_last_error(ctx.h)
    ptrs = (ctypes.c_void_p * 2)(HAND.ctypes.data, HAND.ctypes.data)
    counts = (ctypes.c_int64 * 2)(1 << 30, 1 << 30)              # each below 2^31, the total is not
    m2 = (ctypes.c_int64 * 2)()
    assert ctx.lib.hgmm_voxel_downsample_batch_f64(ctx.h, 2, ptrs, counts, 1.0, m2) == HGMM_ERR_ARG
    assert same(ctx.voxel_down_sample_get(), prev)


def test_get_without_a_result():
    import hgmm_amd
    fresh = hgmm_amd.Context(0)
    try:
        with pytest.raises(hgmm_amd.HgmmError):
            fresh.voxel_down_sample_get()
        with pytest.raises(hgmm_amd.HgmmError):               # a refused first call is no result either
            fresh.voxel_down_sample(HAND, 0.0)
        with pytest.raises(hgmm_amd.HgmmError):
            fresh.voxel_down_sample_get()
    finally:
        fresh.close()


def test_large_then_small_and_repeat(ctx, bunny):
    big = ctx.voxel_down_sample(bunny, 0.004)
    assert same(ctx.voxel_down_sample(HAND, 1.0), (HAND_CENT, HAND_CNT))          # no stale segments of the large call
    assert same(ctx.voxel_down_sample(bunny, 0.004), big)


def test_resident_cloud_is_not_disturbed(ctx, bunny):
    rs = np.random.RandomState(9)
    X = bunny[rs.choice(len(bunny), 3001, replace=False)]
    J = 16
    mu = X[rs.choice(len(X), J, replace=False)].astype(np.float32)
    inv = np.full((J, 3), 50.0, np.float32)
    w = np.full(J, 1.0 / J, np.float32)
    ctx.set_points(X)
    ctx.flat_set_weights(rs.uniform(0.5, 2.0, len(X)).astype(np.float32))
    before = ctx.flat_stats(inv, mu, w, "diag", "W")
    ctx.voxel_down_sample(bunny, 0.004)
    ctx.voxel_down_sample(bunny.astype(np.float64), 0.002)
    after = ctx.flat_stats(inv, mu, w, "diag", "W")
    assert ctx.num_points == len(X)
    assert np.array_equal(before[0].view(np.uint64), after[0].view(np.uint64)) and before[1:] == after[1:]
    ctx.flat_set_weights(None)


def batch_members(bunny, bun045):
    return [bunny, np.array([[0.5, -0.25, 3.0]], np.float32), boundary_cloud().astype(np.float32), bun045,
            np.random.RandomState(10).rand(257, 3).astype(np.float32)]


def test_batch_members_are_their_serial_calls(ctx, bunny, bun045):
    clouds = batch_members(bunny, bun045)
    assert all(c.dtype == np.float32 for c in clouds)
    # 4 mm: the scans' voxel size (the boundary cloud's grid is 1 001^3 cells: 30 key bits + 3 cloud bits);
    # 0.25: the boundary cloud's points lie on voxel faces, and a whole scan falls into a handful of voxels
    for v in (0.004, 0.25):
        got = ctx.voxel_down_sample_batch(clouds, v)
        assert len(got) == len(clouds)
        for k, (g, c) in enumerate(zip(got, clouds)):
            assert same(g, ctx.voxel_down_sample(c, v))
            assert same(g, host(c, v, "batch member %d" % k))
        # float32 rows are widened exactly: the float64 entry on the widened arrays gives the same bits
        wide = ctx.voxel_down_sample_batch([c.astype(np.float64) for c in clouds], v)
        for g, h in zip(got, wide):
            assert same(g, h)


def test_pointcloud_io_with_a_context(ctx, bunny):
    from hgmm_amd.pointcloud_io import voxel_down_sample
    want = host(bunny, 0.004, "bun000")
    assert same(voxel_down_sample(bunny, 0.004, True, ctx=ctx), want)
    alone = voxel_down_sample(bunny, 0.004, ctx=ctx)
    assert isinstance(alone, np.ndarray) and same((alone, want[1]), want)


def same_result(a, b):
    ta, tb = a.transformation, b.transformation
    def bits(x):
        return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)
    return all(np.array_equal(bits(x), bits(y)) for x, y in ((ta.rot, tb.rot), (ta.t, tb.t), (ta.scale, tb.scale), (a.q, b.q)))


def test_registration_with_a_voxel_size(ctx, bunny, bun045):
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints, registration_gmmtree
    s, t = WeightedPoints(*host(bunny, 0.004, "bun000")), WeightedPoints(*host(bun045, 0.004, "bun045"))
    want = registration_gmmtree(s, t, tree_level=3, maxiter=10, ctx=ctx)
    got = registration_gmmtree(bunny, bun045, tree_level=3, maxiter=10, voxel_size=0.004, ctx=ctx)
    assert same_result(got, want)
    assert same_result(registration_gmmtree(s, t, tree_level=3, maxiter=10, ctx=ctx, voxel_size=None), want)
    with pytest.raises(ValueError):
        registration_gmmtree(bunny, bun045, tree_level=3, maxiter=10, voxel_size=0.004, ctx=ctx,
                             target_weights=np.ones(len(bun045)))


def test_batch_registration_with_a_voxel_size(ctx, bunny, bun045):
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints, registration_gmmtree_batch
    s, t = WeightedPoints(*host(bunny, 0.004, "bun000")), WeightedPoints(*host(bun045, 0.004, "bun045"))
    want = registration_gmmtree_batch([(s, t), (t, s)], maxiter=10, ctx=ctx, tree_level=3)
    got = registration_gmmtree_batch([(bunny, bun045), (bun045, bunny)], maxiter=10, ctx=ctx, tree_level=3, voxel_size=0.004)
    assert len(got) == 2 and all(same_result(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError):
        registration_gmmtree_batch([(bunny, bun045)], maxiter=10, ctx=ctx, tree_level=3, voxel_size=0.004,
                                   target_weights=[np.ones(len(bun045))])
