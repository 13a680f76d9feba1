"""The voxel result handed to build and registration on the device (hgmm_voxel_to_*, hgmm_points_rows_f64,
hgmm_tree_build_rows / _batch_rows; Context.*_from_voxels, tree_build(init_rows=)) against the sequences of existing entries
that DEFINE them: down-sample, download, upload again through set_points / tree_set_target / set_points_batch /
tree_set_targets_batch and their weight entries -- "the old path" below, on the same context.  Every comparison is on bits
(dtype, shape and bytes): the hand-overs copy, the weight sums are integers, the extent bound is a maximum -- there is
nothing a tolerance would be for.

Shapes: M = 1 / 255 / 256 / 257 voxels (the pad of the resident planes: under, exactly, one over), a hand-computed cloud,
the two scans at 4 mm (2095 / ~2000 voxels: nine workgroups of the hand-over kernel), a batch whose members are permuted,
repeated, one voxel long and end inside a workgroup."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LS, LD, SIG2, LAMBDA_C = 20.0, 1.0e-4, 0.004, 0.01
ERR_ARG, ERR_STATE = -2, -3


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bun045():
    return np.load(GOLDEN + "/bun045_xyz.npy")


def same(a, b):
    """dtype, shape and bytes of two results (arrays, scalars, or tuples / lists / dicts of them)"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        return all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), (len(a), len(b))
        return all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        assert a is None and b is None
        return True
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes()
    return True


def line_cloud(M):
    """M points on a line one unit apart, point i repeated i % 3 + 1 times: at voxel 0.5 M voxels with counts 1, 2, 3, ..."""
    i = np.repeat(np.arange(M), np.arange(M) % 3 + 1).astype(np.float64)
    return np.stack([i, 0.37 * i, -0.11 * i], axis=1)


def init_idx(L):
    T = 8 * (8 ** L - 1) // 7
    return np.random.RandomState(72).randint(T, size=T)


POSE = (np.array([[np.cos(0.1), -np.sin(0.1), 0.0], [np.sin(0.1), np.cos(0.1), 0.0], [0.0, 0.0, 1.0]]), np.array([0.01, -0.02, 0.005]))

HAND = np.array([[0.375, 0.125, 0.375], [0.375, 0.25, 0.0], [2.5, 0.0, 0.0], [0.0, 0.0, 0.0],
                 [1.25, 1.0, 0.75], [1.25, 1.0, 0.75]])
# v = 1: origin -0.5; rows 0, 1, 3 fall into voxel (0,0,0), the identical rows 4, 5 into (1,1,1), row 2 into (3,0,0)
HAND_CENT = np.array([[0.25, 0.125, 0.125], [1.25, 1.0, 0.75], [2.5, 0.0, 0.0]])
HAND_CNT = np.array([3, 2, 1], np.int64)


# ---- 1: what is resident ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_resident_bits(ctx, M):
    from hgmm_amd.pointcloud_io import voxel_down_sample
    P = line_cloud(M)
    cent, cnt = ctx.voxel_down_sample(P, 0.5)
    assert len(cent) == M and same((cent, cnt), voxel_down_sample(P, 0.5, True))
    vc = ctx.voxel_down_sample(P, 0.5, download=False)
    assert len(vc) == M and vc.count == len(P) and vc.dtype == np.float64
    ctx.set_points(np.full((300, 3), 7.0))                        # (what the pad must not keep)
    ctx.set_points_from_voxels(vc)
    assert ctx.num_points == M
    assert same(ctx.points_rows(np.arange(M)), cent)
    assert same(ctx.points_rows([M - 1, 0, M - 1]), cent[[M - 1, 0, M - 1]])
    assert same(ctx.points_download(), cent.astype(np.float32))


def test_resident_bits_hand_computed(ctx):
    vc = ctx.voxel_down_sample(HAND, 1.0, download=False)
    assert (len(vc), vc.count) == (3, 6)
    ctx.set_points_from_voxels(vc, tree_weights=False, flat_weights=True)
    assert ctx.num_points == 3
    assert same(ctx.points_rows(np.arange(3)), HAND_CENT)
    assert same(ctx.points_download(), HAND_CENT.astype(np.float32))
    # the flat weights are the counts: the point count flat_stats divides by is their sum, 6
    mu = HAND_CENT.astype(np.float32)
    n = ctx.flat_stats(np.full((3, 3), 4.0, np.float32), mu, np.full(3, 1 / 3, np.float32))[2]
    assert n == 6.0
    cent, cnt = vc.get()
    assert same((cent, cnt), (HAND_CENT, HAND_CNT))


# ---- 2: the tree build on a handed-over source ---------------------------------------------------------------------------------
def source_cases(bunny):
    return {"bun000": (bunny, 0.004, 3), "line257": (line_cloud(257), 0.5, 2)}


@pytest.mark.parametrize("precision", [np.float64, np.float32])
@pytest.mark.parametrize("case", ["bun000", "line257"])
def test_source_serial(ctx, bunny, case, precision):
    P, v, L = source_cases(bunny)[case]
    idx = init_idx(L)
    cent, cnt = ctx.voxel_down_sample(P, v)
    if case == "bun000":
        assert len(cent) == 2095
    ctx.tree_set_precision(precision)
    try:
        for weighted in (True, False):
            ctx.set_points(cent)
            if weighted:
                ctx.tree_set_source_weights(cnt.astype(np.float64))
            want = ctx.tree_build(L, LS, LD, cent[idx], SIG2, 200)
            vc = ctx.voxel_down_sample(P, v, download=False)
            ctx.set_points_from_voxels(vc, tree_weights=weighted)
            got = ctx.tree_build(L, LS, LD, None, SIG2, 200, init_rows=idx)       # pi, mu, cov, leaf_idx, iters_per_level, q trace
            assert len(want[5]) > 0 and same(got, want), (case, weighted)
            # ... and on a cloud that did not come from a voxel result
            ctx.set_points(cent)
            if weighted:
                ctx.tree_set_source_weights(cnt.astype(np.float64))
            assert same(ctx.tree_build(L, LS, LD, None, SIG2, 200, init_rows=idx), want)
    finally:
        ctx.tree_set_precision(np.float64)
    # weighted and unweighted builds differ (the comparison above is not between two runs that ignore the weights)
    assert len(set(cnt.tolist())) > 1


# ---- 3: the serial target ------------------------------------------------------------------------------------------------------
def registration_outputs(ctx, T):
    """everything the serial registration entries return for the resident tree and target"""
    out = {"estep_identity": ctx.tree_reg_estep(T, lambda_c=LAMBDA_C),
           "estep_pose": ctx.tree_reg_estep(T, POSE[0], POSE[1], 1.0, LAMBDA_C),
           "register": ctx.tree_register(np.identity(3), np.zeros(3), 1.0, LAMBDA_C, 10, 1.0e-4)[:5],
           "score": ctx.tree_score(POSE[0], POSE[1], 1.0, LAMBDA_C, want=())[0]}
    return out


@pytest.mark.parametrize("gate", [np.inf, 16.27])
def test_target_serial(ctx, bunny, bun045, gate):
    L = 3
    T = 8 * (8 ** L - 1) // 7
    res = ctx.voxel_down_sample_batch([bunny, bun045], 0.004, download=False)
    (_, _), (cent45, cnt45) = res.get()
    ctx.set_points_from_voxels(res.member(0))
    ctx.tree_build(L, LS, LD, None, SIG2, 200, init_rows=init_idx(L), want_leaf=False)
    ctx.tree_set_reg_gate(gate)
    try:
        for weighted in (True, False):
            ctx.tree_set_target(cent45)
            if weighted:
                ctx.tree_set_target_weights(cnt45.astype(np.float64))
            want = registration_outputs(ctx, T)
            ctx.tree_set_target(np.full((5, 3), 3.0))              # (a target the hand-over must replace entirely)
            ctx.tree_set_target_from_voxels(res.member(1), weighted=weighted)
            got = registration_outputs(ctx, T)
            assert same(got, want), (gate, weighted)
            assert want["register"][2] > 0 and want["score"][0] == (len(bun045) if weighted else len(cent45))
    finally:
        ctx.tree_set_reg_gate(np.inf)


# ---- 4: the batch --------------------------------------------------------------------------------------------------------------
def batch_outputs(ctx, counts, L, init):
    return ctx.tree_build_batch(counts, L, LS, LD, sig2=SIG2, max_iters_per_level=200, want_trace=True, **init)


def pair_outputs(ctx, B):
    reg = ctx.tree_register_batch(np.tile(np.identity(3), (B, 1, 1)), np.zeros((B, 3)), 1.0, LAMBDA_C, 10, 1.0e-4)[:5]
    return reg, ctx.tree_score_batch(np.tile(POSE[0], (B, 1, 1)), np.tile(POSE[1], (B, 1)), 1.0, LAMBDA_C)


@pytest.mark.parametrize("weighted", [True, False])
def test_batch(ctx, bunny, bun045, weighted):
    L = 2
    idx = init_idx(L)
    clouds = [bunny, np.array([[0.1, 0.2, 0.3]]), np.random.RandomState(5).rand(257, 3), bun045]
    res = ctx.voxel_down_sample_batch(clouds, 0.004, download=False)
    host = res.get()
    assert res.m[1] == 1 and res.m[2] == 257 and res.n == [len(c) for c in clouds]
    src, tgt_sets = [3, 0, 0, 2], ([0, 3, 2, 0], [1, 0, 3, 1])       # (the second set: the one-voxel member as a target)
    wts = lambda members: [host[m][1].astype(np.float64) for m in members] if weighted else None
    # the old path
    arrs = ctx.set_points_batch([host[m][0] for m in src], weights=wts(src))
    counts = [len(a) for a in arrs]
    want_rows = ctx.points_rows(np.arange(sum(counts)))
    want_build = batch_outputs(ctx, counts, L, dict(init_mu=np.stack([a[idx] for a in arrs])))
    want_pairs = []
    for tg in tgt_sets:
        ctx.tree_set_targets_batch([host[m][0] for m in tg], weights=wts(tg))
        want_pairs.append(pair_outputs(ctx, len(src)))
    # the hand-over
    assert ctx.set_points_batch_from_voxels([res.member(m) for m in src], weighted=weighted) == counts
    assert ctx.num_points == sum(counts)
    assert same(ctx.points_rows(np.arange(sum(counts))), want_rows)
    assert same(want_rows, np.concatenate([host[m][0] for m in src]))
    got_build = batch_outputs(ctx, counts, L, dict(init_mu=None, init_rows=idx))
    assert same(got_build, want_build)
    assert same(batch_outputs(ctx, counts, L, dict(init_mu=None, init_rows=np.tile(idx, (4, 1)))), want_build)
    for tg, want in zip(tgt_sets, want_pairs):
        ctx.tree_set_targets_batch_from_voxels([res.member(m) for m in tg], weighted=weighted)
        assert same(pair_outputs(ctx, len(src)), want), tg
    # the score's slot 0 is the targets' weight sums: the raw point counts, or the voxels
    s0 = pair_outputs(ctx, len(src))[1][:, 0]
    assert s0.tolist() == [float(res.n[m] if weighted else res.m[m]) for m in tgt_sets[1]]
    # a node table of the forest still comes out at the depth it was built with
    assert same(ctx.tree_get_nodes_batch(1, L), tuple(t[1] for t in want_build[0]))


# ---- 5: the flat fit -----------------------------------------------------------------------------------------------------------
def test_flat(ctx, bunny):
    J = 16
    P = bunny[np.sort(np.random.RandomState(0).choice(len(bunny), 3001, replace=False))]
    cent, cnt = ctx.voxel_down_sample(P, 0.002)
    assert cnt.max() > 1
    mu = cent[np.random.RandomState(1).choice(len(cent), J, replace=False)].astype(np.float32)
    inv, cov, w = np.full((J, 3), 100.0, np.float32), np.full((J, 3), 1.0e-4, np.float32), np.full(J, 1.0 / J, np.float32)

    def outputs():
        return ctx.flat_stats(inv, mu, w, "diag", "W"), ctx.flat_train(3, 0.0, mu.copy(), cov.copy(), w.copy(), "diag", "W")
    ctx.set_points(cent)
    ctx.flat_set_weights(cnt.astype(np.float32))
    want = outputs()
    assert want[0][2] == float(len(P))
    vc = ctx.voxel_down_sample(P, 0.002, download=False)
    ctx.set_points_from_voxels(vc, tree_weights=False, flat_weights=True)
    assert same(outputs(), want)
    # without the flag the fit is unweighted
    ctx.set_points_from_voxels(vc, tree_weights=True, flat_weights=False)
    assert ctx.flat_stats(inv, mu, w, "diag", "W")[2] == float(len(cent))


# ---- 6: the result is copied, not moved ------------------------------------------------------------------------------------------
def test_the_result_survives(ctx, bunny, bun045):
    L = 2
    T = 8 * (8 ** L - 1) // 7
    res = ctx.voxel_down_sample_batch([bunny, bun045], 0.004, download=False)
    before = ctx.voxel_down_sample_get()
    states = []
    for _ in range(2):
        ctx.set_points_batch_from_voxels([res.member(1), res.member(1)])
        ctx.tree_set_targets_batch_from_voxels(res.members())
        ctx.set_points_from_voxels(res.member(0), flat_weights=True)
        ctx.set_points_from_voxels(res.member(0), flat_weights=True)
        build = ctx.tree_build(L, LS, LD, None, SIG2, 200, init_rows=init_idx(L))
        ctx.tree_set_target_from_voxels(res.member(1))
        ctx.tree_set_target_from_voxels(res.member(1))
        states.append((ctx.points_rows(np.arange(len(res.member(0)))), ctx.points_download(), build, ctx.tree_reg_estep(T)))
        assert same(ctx.voxel_down_sample_get(), before)
        assert same(res.get(), [(before[0][:res.m[0]], before[1][:res.m[0]]), (before[0][res.m[0]:], before[1][res.m[0]:])])
    assert same(states[0], states[1])
    assert ctx.voxel_result_info() == (res.m, res.n, res.serial)


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_in_place(ctx, bunny, bun045):
    import hgmm_amd
    L = 2
    T = 8 * (8 ** L - 1) // 7
    J = 8
    res = ctx.voxel_down_sample_batch([bunny, bun045], 0.004, download=False)
    ctx.set_points_from_voxels(res.member(0), tree_weights=True, flat_weights=True)
    ctx.tree_build(L, LS, LD, None, SIG2, 200, init_rows=init_idx(L), want_leaf=False)
    ctx.tree_set_target_from_voxels(res.member(1))
    mu = ctx.points_download()[:J]
    inv, w = np.full((J, 3), 100.0, np.float32), np.full(J, 1.0 / J, np.float32)
    state = lambda: (ctx.flat_stats(inv, mu, w), ctx.tree_reg_estep(T, POSE[0], POSE[1], 1.0, LAMBDA_C), ctx.num_points,
                     ctx.voxel_down_sample_get(), ctx.voxel_result_info())
    before = state()
    lib, h = ctx.lib, ctx.h
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    out = np.empty((4, 3))

    def rows_call(values, k=None, with_rows=True, with_out=True):
        rows = np.array(values, np.int64)                           # (alive until the call has returned)
        return lib.hgmm_points_rows_f64(h, rows.ctypes.data if with_rows else None, len(rows) if k is None else k,
                                        out.ctypes.data if with_out else None)
    n = ctx.num_points
    rows_T = np.zeros(T, np.int64)
    tb = lambda rows: lib.hgmm_tree_build_rows(h, L, LS, LD, None if rows is None else rows.ctypes.data, SIG2, 200,
                                               None, None, None, None, None, None, 0, None)
    refused = [
        (lib.hgmm_voxel_to_points(h, -1, 1), ERR_ARG, "member -1"),
        (lib.hgmm_voxel_to_points(h, 2, 1), ERR_ARG, "member 2"),
        (lib.hgmm_voxel_to_points(h, 0, 4), ERR_ARG, "bits"),
        (lib.hgmm_voxel_to_points(h, 0, 7), ERR_ARG, "bits"),
        (lib.hgmm_voxel_to_target(h, 2, 1), ERR_ARG, "member 2"),
        (lib.hgmm_voxel_to_target(h, -1, 0), ERR_ARG, "member -1"),
        (lib.hgmm_voxel_to_points_batch(h, 0, i32(0), 1), ERR_ARG, "B = 0"),
        (lib.hgmm_voxel_to_points_batch(h, 2, None, 1), ERR_ARG, "NULL"),
        (lib.hgmm_voxel_to_points_batch(h, 3, i32(0, 1, 2), 1), ERR_ARG, "members[2] = 2"),
        (lib.hgmm_voxel_to_targets_batch(h, 0, i32(0), 1), ERR_ARG, "B = 0"),
        (lib.hgmm_voxel_to_targets_batch(h, 4097, i32(*([0] * 4097)), 1), ERR_ARG, "B = 4097"),
        (lib.hgmm_voxel_to_targets_batch(h, 2, None, 0), ERR_ARG, "NULL"),
        (lib.hgmm_voxel_to_targets_batch(h, 2, i32(0, -1), 0), ERR_ARG, "members[1] = -1"),
        (rows_call([0, 1, n, 2]), ERR_ARG, "rows[2] = %d" % n),
        (rows_call([-1]), ERR_ARG, "rows[0] = -1"),
        (rows_call([0], k=-1), ERR_ARG, "k = -1"),
        (rows_call([0], with_rows=False), ERR_ARG, "NULL"),
        (rows_call([0], with_out=False), ERR_ARG, "NULL"),
        (tb(None), ERR_ARG, "init_rows is NULL"),
        (tb(np.where(np.arange(T) == 5, n, rows_T)), ERR_ARG, "init_rows[5] = %d" % n),
        (tb(np.where(np.arange(T) == T - 1, -3, rows_T)), ERR_ARG, "init_rows[%d] = -3" % (T - 1)),
    ]
    for rc, code, what in refused:
        assert rc == code, what
    # (hgmm_last_error answers for the last call: the texts that name a position and a value are read after a call of their own)
    assert lib.hgmm_voxel_to_points(h, 2, 1) == ERR_ARG and b"member 2" in lib.hgmm_last_error(h)
    assert rows_call([0, 1, n, 2]) == ERR_ARG and ("rows[2] = %d" % n).encode() in lib.hgmm_last_error(h)
    assert tb(np.where(np.arange(T) == 5, n, rows_T)) == ERR_ARG and ("init_rows[5] = %d" % n).encode() in lib.hgmm_last_error(h)
    assert lib.hgmm_voxel_to_points(h, 0, 4) == ERR_ARG and b"bits" in lib.hgmm_last_error(h)
    with pytest.raises(hgmm_amd.HgmmError):
        ctx.set_points_from_voxels(hgmm_amd.VoxelCloud(res, 5))
    assert same(state(), before)

    # the forest: a refused hand-over / a refused row table leaves cloud, weights, targets and trees what they were
    counts = ctx.set_points_batch_from_voxels([res.member(0), res.member(1)])
    ctx.tree_build_batch(counts, L, LS, LD, None, SIG2, 200, want_tables=False, init_rows=init_idx(L))
    ctx.tree_set_targets_batch_from_voxels([res.member(1), res.member(0)])
    forest = lambda: (ctx.tree_score_batch(), ctx.points_rows(np.arange(sum(counts))),
                      ctx.tree_register_batch(np.tile(np.identity(3), (2, 1, 1)), np.zeros((2, 3)), 1.0, LAMBDA_C, 5, 1.0e-4)[:5])
    f_before = forest()
    bad = np.tile(np.zeros(T, np.int64), (2, 1))
    bad[1, 3] = counts[1]
    with pytest.raises(hgmm_amd.HgmmError, match=r"init_rows\[1\]\[3\] = %d" % counts[1]):
        ctx.tree_build_batch(counts, L, LS, LD, None, SIG2, 200, want_tables=False, init_rows=bad)
    assert lib.hgmm_voxel_to_points_batch(h, 2, i32(0, 2), 1) == ERR_ARG
    assert lib.hgmm_voxel_to_targets_batch(h, 2, i32(2, 0), 1) == ERR_ARG
    # ... and the Context's own bookkeeping of the forest cloud and its targets
    book = lambda: (list(ctx._batch_counts), ctx._tgt_B, list(ctx._tgt_counts), ctx.n)
    b_before = book()
    beyond = hgmm_amd.VoxelCloud(res, 5)
    for refused_call in (lambda: ctx.set_points_batch_from_voxels([res.member(0), beyond]),
                         lambda: ctx.tree_set_targets_batch_from_voxels([beyond, res.member(0)]),
                         lambda: ctx.set_points_from_voxels(beyond)):
        with pytest.raises(hgmm_amd.HgmmError):
            refused_call()
    assert book() == b_before
    ctx.tree_set_source_weights_batch([None, None])                 # (a None entry takes its count from that bookkeeping)
    ctx.tree_set_source_weights_batch(None)
    assert same(forest(), f_before)


def test_without_a_result_and_stale_clouds(bunny):
    import hgmm_amd
    c = hgmm_amd.Context(0)
    try:
        lib, h = c.lib, c.h
        m = (C.c_int32 * 1)(0)
        assert lib.hgmm_voxel_result_info(h, None, None, None, None) == ERR_STATE
        assert lib.hgmm_voxel_to_points(h, 0, 1) == ERR_STATE
        assert lib.hgmm_voxel_to_target(h, 0, 1) == ERR_STATE
        assert lib.hgmm_voxel_to_points_batch(h, 1, m, 1) == ERR_STATE
        assert lib.hgmm_voxel_to_targets_batch(h, 1, m, 1) == ERR_STATE and b"no voxel result" in lib.hgmm_last_error(h)
        rows, out = np.zeros(1, np.int64), np.empty((1, 3))
        assert lib.hgmm_points_rows_f64(h, rows.ctypes.data, 1, out.ctypes.data) == ERR_STATE
        with pytest.raises(hgmm_amd.HgmmError):
            c.voxel_result_info()
        first = c.voxel_down_sample(bunny[:500], 0.004, download=False)
        c.set_points_from_voxels(first)
        assert c.voxel_result_info()[2] == 1
        # a refused down-sample keeps the result and its serial number
        with pytest.raises(hgmm_amd.HgmmError):
            c.voxel_down_sample(bunny[:500], -1.0)
        c.set_points_from_voxels(first)
        second = c.voxel_down_sample(bunny[:400], 0.004, download=False)
        assert c.voxel_result_info()[2] == 2
        for use in (lambda: c.set_points_from_voxels(first), lambda: c.tree_set_target_from_voxels(first),
                    lambda: c.set_points_batch_from_voxels([second, first]), lambda: c.tree_set_targets_batch_from_voxels([first]),
                    first.get):
            with pytest.raises(hgmm_amd.HgmmError, match="down-sampled something else since"):
                use()
        c.set_points_from_voxels(second)
        assert c.num_points == len(second)
        # a member of another context's result is refused by name, not handed over
        other = hgmm_amd.Context(0)
        try:
            with pytest.raises(hgmm_amd.HgmmError, match="another context"):
                other.set_points_from_voxels(second)
        finally:
            other.close()
    finally:
        c.close()


# ---- 8: the round trip is gone -------------------------------------------------------------------------------------------------
def same_result(a, b):
    ta, tb = a.transformation, b.transformation
    return same((ta.rot, ta.t, np.float64(ta.scale), a.q), (tb.rot, tb.t, np.float64(tb.scale), b.q))


def host_weighted(P, v):
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    from hgmm_amd.pointcloud_io import voxel_down_sample
    return WeightedPoints(*voxel_down_sample(P, v, True))


def test_no_host_round_trip(ctx, bunny, bun045, monkeypatch):
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import registration_gmmtree, registration_gmmtree_batch
    s, t = host_weighted(bunny, 0.004), host_weighted(bun045, 0.004)
    want = registration_gmmtree(s, t, tree_level=3, maxiter=10, ctx=ctx)
    want_batch = registration_gmmtree_batch([(s, t), (t, s)], maxiter=10, ctx=ctx, tree_level=3)

    def no_download(self):
        raise AssertionError("the voxel result was downloaded")
    monkeypatch.setattr(hgmm_amd.Context, "voxel_down_sample_get", no_download)
    got = registration_gmmtree(bunny, bun045, voxel_size=0.004, tree_level=3, maxiter=10, ctx=ctx)
    assert same_result(got, want)
    got_batch = registration_gmmtree_batch([(bunny, bun045), (bun045, bunny)], maxiter=10, ctx=ctx, tree_level=3, voxel_size=0.004)
    assert len(got_batch) == 2 and all(same_result(g, w) for g, w in zip(got_batch, want_batch))
    # VoxelClouds from the start
    res = ctx.voxel_down_sample_batch([bunny, bun045], 0.004, download=False)
    assert same_result(registration_gmmtree(res.member(0), res.member(1), tree_level=3, maxiter=10, ctx=ctx), want)
    with pytest.raises(ValueError):
        registration_gmmtree(res.member(0), res.member(1), tree_level=3, maxiter=10, ctx=ctx, target_weights=np.ones(len(res.member(1))))


def test_voxel_clouds_among_host_clouds(ctx, bunny, bun045, monkeypatch):
    """the batched hand-overs take members only: a batch that mixes VoxelClouds and host clouds on a side brings the members
    to the host with their counts, and returns what the all-host call returns"""
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import registration_gmmtree_batch
    s, t = host_weighted(bunny, 0.004), host_weighted(bun045, 0.004)
    want = registration_gmmtree_batch([(s, t), (s, t)], maxiter=10, ctx=ctx, tree_level=3)
    res = ctx.voxel_down_sample_batch([bunny, bun045], 0.004, download=False)
    got = registration_gmmtree_batch([(res.member(0), t), (s, res.member(1))], maxiter=10, ctx=ctx, tree_level=3)
    assert all(same_result(g, w) for g, w in zip(got, want))
    # one side members, the other host arrays: no conversion on the members' side
    got = registration_gmmtree_batch([(res.member(0), t), (res.member(0), t)], maxiter=10, ctx=ctx, tree_level=3)
    assert all(same_result(g, w) for g, w in zip(got, want))
    # several members of one result among host clouds: the result comes to the host once
    downloads = []
    inner = hgmm_amd.Context.voxel_down_sample_get
    monkeypatch.setattr(hgmm_amd.Context, "voxel_down_sample_get", lambda self: downloads.append(1) or inner(self))
    got = registration_gmmtree_batch([(res.member(0), t), (res.member(0), t), (s, t)], maxiter=10, ctx=ctx, tree_level=3)
    assert len(downloads) == 1 and all(same_result(g, want[0]) for g in got)


def test_a_chain_down_samples_each_scan_once(ctx, bunny, bun045, monkeypatch):
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import registration_gmmtree_batch
    th = 0.05
    rz = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    a, b, c = bunny, bun045, np.asarray(bunny, np.float64) @ rz.T
    kw = dict(maxiter=10, ctx=ctx, tree_level=3, voxel_size=0.004)
    want = registration_gmmtree_batch([(a, b)], **kw) + registration_gmmtree_batch([(b, c)], **kw)
    seen = []
    inner = hgmm_amd.Context.voxel_down_sample_batch

    def counting(self, clouds, *args, **kwargs):
        seen.append(len(clouds))
        return inner(self, clouds, *args, **kwargs)
    monkeypatch.setattr(hgmm_amd.Context, "voxel_down_sample_batch", counting)
    got = registration_gmmtree_batch([(a, b), (b, c)], **kw)
    assert seen == [3] and len(ctx.voxel_result_info()[0]) == 3
    assert len(got) == 2 and all(same_result(g, w) for g, w in zip(got, want))
    # equal arrays that are different objects are not merged
    del seen[:]
    registration_gmmtree_batch([(a, b), (b.copy(), c)], **kw)
    assert seen == [4]
