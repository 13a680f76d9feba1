"""Batched multi-start (hgmm_tree_register_batch_multi / hgmm_tree_score_batch_multi, registration_gmmtree_batch(starts=)):
R start poses over the resident FOREST in the launches of one, hypothesis r on the tree and the target of pair[r].

The registration moments are 64-bit fixed-point integer sums and the score's shares are added in a fixed order, so the bar
for every hypothesis is ``np.array_equal`` with the serial sequence  tree_set_nodes(tree_get_nodes_batch(pair[r])),
tree_set_target(target pair[r]) (+ its weights), tree_register / tree_score from / at that pose:  pose, iteration count,
status, q and the whole per-iteration trace, resp. all eight summary words -- whatever R is, wherever r sits and whoever its
neighbours are.  What the serial entry itself is held to is in tests/test_tree_gpu.py and tests/test_tree_reg_depth_gpu.py.

The recovery numbers of test 11 are the float64 oracle's on tests/golden/hgmm_reg_L4.npz (docstring of
tests/test_tree_multistart_gpu.py): from the identity the 30-degree record ends at fitness 0.549, from 5 of the 27 grid
starts at 0.937."""
import ctypes

import numpy as np
import pytest

from _tree_helpers import weights_for
from conftest import load_golden
from oracle import hgmm_tree
from test_tree_multistart_gpu import HGMM_ERR_ARG, I3, Z3, five_starts, grid_starts
from test_tree_reg_depth_gpu import ctx, moved, rot_about  # noqa: F401
from test_tree_score_gpu import CHI2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record4():
    return load_golden("hgmm_reg_L4.npz")


def build_forest(ctx, clouds, targets, L, weights=None):
    """the forest of ``clouds`` with ``targets`` resident (the library's default constants) -> the B node tables"""
    T = hgmm_tree.n_total(L)
    rs = np.random.RandomState(72)
    arrs = ctx.set_points_batch(clouds)
    init = np.stack([np.asarray(a[rs.randint(len(a), size=T)], dtype=np.float64) for a in arrs])
    ctx.tree_build_batch([len(a) for a in arrs], L, 20.0, 1e-4, init, 0.004, want_tables=False)
    ctx.tree_set_targets_batch(targets, weights=weights)
    return [ctx.tree_get_nodes_batch(b, L) for b in range(len(clouds))]


def serial_pair(ctx, L, nodes, target, w=None):
    ctx.tree_set_nodes(L, *nodes)
    ctx.tree_set_target(target)
    if w is not None:
        ctx.tree_set_target_weights(w)


def serial_register(ctx, rot0, t0, lc, maxiter, tol):
    return ctx.tree_register(rot0, t0, 1.0, lc, maxiter, tol, None, want_trace=True)


def assert_hypothesis(multi, r, serial, what):
    m_rot, m_t, m_it, m_q, m_st, m_tr = multi
    s_rot, s_t, s_it, s_q, s_st, s_tr = serial
    assert (int(m_it[r]), int(m_st[r])) == (s_it, s_st), what
    assert np.array_equal(m_rot[r], s_rot) and np.array_equal(m_t[r], s_t), what
    assert (np.isnan(m_q[r]) and s_q is None) or m_q[r] == s_q, what
    assert m_tr[r].shape == (s_it, 13) and np.array_equal(m_tr[r], s_tr), what


def assert_multi_is_serial(ctx, L, nodes, targets, pair, rot0, t0, lc, maxiter, tol, label, weights=None, score_at=None):
    """One batch_multi call == the serial sequence per hypothesis, bit for bit; with ``score_at`` (rot, t) also the scores at
    those poses.  The serial entries leave the forest alone, so they run after the call.  -> the call's results"""
    pair = np.asarray(pair)
    R = len(pair)
    multi = ctx.tree_register_batch_multi(pair, rot0, t0, 1.0, lc, maxiter, tol, want_trace=True)
    assert multi[0].shape == (R, 3, 3) and multi[1].shape == (R, 3) and len(multi[5]) == R
    sums = None if score_at is None else ctx.tree_score_batch_multi(pair, score_at[0], score_at[1], 1.0, lc, CHI2)
    for b in sorted(set(pair.tolist())):
        serial_pair(ctx, L, nodes[b], targets[b], None if weights is None else weights[b])
        for r in np.nonzero(pair == b)[0]:
            what = "%s, hypothesis %d of pair %d" % (label, r, b)
            assert_hypothesis(multi, r, serial_register(ctx, rot0[r], t0[r], lc, maxiter, tol), what)
            if sums is not None:
                alone = ctx.tree_score(score_at[0][r], score_at[1][r], 1.0, lc, CHI2, want=())[0]
                assert np.array_equal(sums[r], alone), what
    return multi + (sums,)


def hypotheses(targets, pair):
    """row r: the (r mod 5)-th of five_starts about the centroid of target pair[r]"""
    per = [five_starts(t.mean(axis=0)) for t in targets]
    count = {}
    rot, t = [], []
    for b in pair:
        k = count.get(b, 0)
        count[b] = k + 1
        rot.append(per[b][0][k % 5])
        t.append(per[b][1][k % 5])
    return np.stack(rot), np.stack(t)


@pytest.fixture(scope="module")
def small_forest(ctx, bunny):
    """B = 3 trees at L = 2; targets of 100, 256 and 257 points: a partial chunk, an exact chunk, one over"""
    b = bunny.astype(np.float64)
    clouds = [b[::40], b[5::50], b[7::45]]
    targets = [moved(c, 5.0, [0, 0, 1], [0.002, 0.0, 0.001])[:n] for c, n in zip(clouds, (100, 256, 257))]
    return clouds, targets


# ---------------------------------------------------------------------------------------------------------------------
# 1. a ragged set in scrambled order   2. a pair without a hypothesis, R = 1
# ---------------------------------------------------------------------------------------------------------------------
def test_ragged_set_in_scrambled_order(ctx, small_forest):
    clouds, targets = small_forest
    nodes = build_forest(ctx, clouds, targets, 2)
    pair = [2, 1, 0, 1, 2, 1, 1, 2, 1]                          # K = (1, 5, 3)
    rot0, t0 = hypotheses(targets, pair)
    out = assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "ragged", score_at=(rot0, t0))
    assert (out[2] > 0).all()
    assert out[6][:, 0].tolist() == [len(targets[b]) for b in pair]
    # ... and at the poses the loops ended at
    sums = ctx.tree_score_batch_multi(pair, out[0], out[1], 1.0, 0.01, CHI2)
    for b in range(3):
        serial_pair(ctx, 2, nodes[b], targets[b])
        for r in np.nonzero(np.asarray(pair) == b)[0]:
            assert np.array_equal(sums[r], ctx.tree_score(out[0][r], out[1][r], 1.0, 0.01, CHI2, want=())[0]), r


def test_a_pair_without_a_hypothesis_and_a_single_one(ctx, small_forest):
    clouds, targets = small_forest
    nodes = build_forest(ctx, clouds, targets, 2)
    pair = [2, 0, 2, 0]                                         # pair 1 takes no part
    rot0, t0 = hypotheses(targets, pair)
    assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "no hypothesis for pair 1", score_at=(rot0, t0))
    rot1, t1 = hypotheses(targets, [1, 1, 1])
    assert_multi_is_serial(ctx, 2, nodes, targets, [1], rot1[2:], t1[2:], 0.01, 6, 1e-6, "R = 1", score_at=(rot1[2:], t1[2:]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. pair = 0..B-1 from the identity is the forest's own registration and score
# ---------------------------------------------------------------------------------------------------------------------
def test_one_identity_hypothesis_per_pair_is_register_batch(ctx, small_forest):
    clouds, targets = small_forest
    build_forest(ctx, clouds, targets, 2)
    rot0, t0 = np.tile(I3, (3, 1, 1)), np.zeros((3, 3))
    forest = ctx.tree_register_batch(rot0, t0, 1.0, 0.01, 8, 1e-6, want_trace=True)
    multi = ctx.tree_register_batch_multi(np.arange(3), rot0, t0, 1.0, 0.01, 8, 1e-6, want_trace=True)
    for x, y in zip(forest[:5], multi[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(forest[5], multi[5]))
    assert np.array_equal(ctx.tree_score_batch(forest[0], forest[1], 1.0, 0.01),
                          ctx.tree_score_batch_multi(np.arange(3), forest[0], forest[1], 1.0, 0.01))


# ---------------------------------------------------------------------------------------------------------------------
# 4. different stop iterations in one call: two pairs at L = 4, the 27-start grid each
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record_forest(record4):
    points = np.asarray(record4["points"], dtype=np.float64)
    assert len(record4["rot30_target"]) == 5032
    return [points, points], [np.asarray(record4["rot30_target"]), np.asarray(record4["rot10_target"])]


def test_different_stop_iterations_in_one_call(ctx, record4, record_forest):
    clouds, targets = record_forest
    nodes = build_forest(ctx, clouds, targets, 4)
    g_rot, g_t = grid_starts()
    pair = np.repeat([0, 1], 27)
    rot0, t0 = np.concatenate([g_rot, g_rot]), np.concatenate([g_t, g_t])
    lc = float(record4["lambda_c"])
    _, _, iters, _, status, _, _ = assert_multi_is_serial(ctx, 4, nodes, targets, pair, rot0, t0, lc, 30, 1e-4, "two grids")
    print("iterations:", iters.tolist(), "status:", status.tolist())
    stops = [set(iters[(pair == b) & (status == 1)].tolist()) for b in (0, 1)]
    assert max(len(s) for s in stops) >= 2


# ---------------------------------------------------------------------------------------------------------------------
# 5. the reference's default depth
# ---------------------------------------------------------------------------------------------------------------------
def test_depth_5(ctx, bunny):
    b = bunny.astype(np.float64)
    clouds = [b[::40], b[5::50]]
    targets = [moved(c, 3.0, [0.2, 1.0, 0.4], [0.002, 0.0, 0.001]) for c in clouds]
    nodes = build_forest(ctx, clouds, targets, 5)
    pair = [0, 1, 1, 0, 0, 1]
    rot0, t0 = hypotheses(targets, pair)
    out = assert_multi_is_serial(ctx, 5, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "L = 5", score_at=(rot0, t0))
    assert out[2].max() > 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. the gate; weights on one pair only   7. the loop on the device alone
# ---------------------------------------------------------------------------------------------------------------------
def test_gate_and_weights(ctx, small_forest):
    clouds, targets = small_forest
    clouds, targets = clouds[:2], targets[1:]                   # targets of 256 and 257 points
    pair = [1, 0, 1, 0, 1, 0]
    rot0, t0 = hypotheses(targets, pair)
    nodes = build_forest(ctx, clouds, targets, 2)
    plain = assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "plain", score_at=(rot0, t0))
    ctx.tree_set_reg_gate(11.34)
    try:
        gated = assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "gated", score_at=(rot0, t0))
    finally:
        ctx.tree_set_reg_gate(np.inf)
    assert not np.array_equal(gated[0], plain[0])                # (the gate took part)
    weights = [weights_for(len(targets[0])), None]
    nodes_w = build_forest(ctx, clouds, targets, 2, weights=weights)
    assert all(np.array_equal(x, y) for a, b in zip(nodes, nodes_w) for x, y in zip(a, b))
    weighted = assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "weights on pair 0",
                                      weights=weights, score_at=(rot0, t0))
    one = np.asarray(pair) == 1                                  # the unweighted pair: its unweighted bits
    for k in (0, 1, 2, 3, 4, 6):
        assert np.array_equal(np.asarray(weighted[k])[one], np.asarray(plain[k])[one]), k
    assert all(np.array_equal(weighted[5][r], plain[5][r]) for r in np.nonzero(one)[0])
    assert not np.array_equal(weighted[0][~one], plain[0][~one])
    assert weighted[6][~one, 0] == pytest.approx(weights[0].sum(), rel=1e-12)     # (the library's sum: in index order)
    ctx.tree_set_reg_gate(11.34)
    try:
        assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "gated and weighted", weights=weights)
    finally:
        ctx.tree_set_reg_gate(np.inf)


def test_with_the_solve_on_the_device(ctx, small_forest):
    clouds, targets = small_forest
    nodes = build_forest(ctx, clouds, targets, 2)
    pair = [2, 1, 0, 1, 2, 1, 1, 2, 1]
    rot0, t0 = hypotheses(targets, pair)
    with ctx.config(reg_device_solve=1):
        out = assert_multi_is_serial(ctx, 2, nodes, targets, pair, rot0, t0, 0.01, 12, 1e-4, "device solve")
    print("device solve, iterations:", out[2].tolist(), "status:", out[4].tolist())
    assert (out[2] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. one singular hypothesis of one pair leaves (status 2); nobody else notices; the mirror finishes it serially
# ---------------------------------------------------------------------------------------------------------------------
def test_ill_conditioned_hypothesis_leaves_alone_and_is_finished_serially(ctx, bunny):
    from hgmm_amd.hgmm.hgmm_gpu import RigidTransformation, registration_gmmtree, registration_gmmtree_batch
    b = bunny.astype(np.float64)
    clouds = [b[::10], b[3::12]]
    targets = [moved(clouds[0], 4.0, [0, 1, 0], [0.001, 0.001, 0.0]), moved(clouds[1], 3.0, [1, 0, 0], [0.0, 0.001, 0.001])]
    nodes = build_forest(ctx, clouds, targets, 1)
    R1 = rot_about([0, 0, 1], 5)
    c = [t.mean(axis=0) for t in targets]
    # rows: pair 0 from the identity, pair 1 turned, pair 0 SINGULAR (R = 0 moves every point onto one), pair 1 identity, pair 0 turned
    pair = [0, 1, 0, 1, 0]
    rot0 = np.stack([I3, R1, np.zeros((3, 3)), I3, R1])
    t0 = np.stack([Z3, c[1] - R1 @ c[1], clouds[0][0] + 0.001, Z3, c[0] - R1 @ c[0]])
    _, _, iters, _, status, _, _ = assert_multi_is_serial(ctx, 1, nodes, targets, pair, rot0, t0, 0.01, 6, 1e-6, "one singular")
    assert status[2] == 2 and iters[2] == 0
    assert (np.delete(status, 2) != 2).all() and (np.delete(iters, 2) > 0).all()
    # the others keep the bits they have without it
    rest = [0, 1, 3, 4]
    alone = ctx.tree_register_batch_multi(np.asarray(pair)[rest], rot0[rest], t0[rest], 1.0, 0.01, 6, 1e-6)
    both = ctx.tree_register_batch_multi(pair, rot0, t0, 1.0, 0.01, 6, 1e-6)
    for x, y in zip(alone[:5], both[:5]):
        assert np.array_equal(x, y[rest])
    # through the mirror: finished like the serial mirror finishes it
    starts = [[RigidTransformation(rot0[r], t0[r]) for r in (0, 2, 4)], [RigidTransformation(rot0[r], t0[r]) for r in (1, 3)]]
    kw = dict(tree_level=1, lambda_c=0.01, ls=20, sig2=0.004, ctx=ctx)
    res, info = registration_gmmtree_batch(list(zip(clouds, targets)), maxiter=6, tol=1e-6, starts=starts, return_info=True, **kw)
    assert info["hypothesis_status"][0][1] == 2 and 2 not in info["hypothesis_status"][1]
    for k in range(2):
        one = registration_gmmtree(clouds[k], targets[k], 6, 1e-6, starts=starts[k], **kw)
        assert_same_winner(res[k], one, "pair %d" % k)
    only = registration_gmmtree_batch([(clouds[0], targets[0])], maxiter=6, tol=1e-6, starts=[starts[0][1:2]], **kw)[0]
    assert only.best_index_ == 0 and np.isfinite(only.transformation.t).all() and np.isfinite(only.transformation.rot).all()
    one = registration_gmmtree(clouds[0], targets[0], 6, 1e-6, starts=starts[0][1:2], **kw)
    assert_same_winner(only, one, "the singular start alone")


def assert_same_winner(batch, serial, what):
    """a pair's MultiStartResult of the batch against registration_gmmtree(starts=): bit for bit"""
    from hgmm_amd.hgmm.hgmm_gpu import MultiStartResult
    assert isinstance(batch, MultiStartResult), what
    assert np.array_equal(batch.transformation.rot, serial.transformation.rot), what
    assert np.array_equal(batch.transformation.t, serial.transformation.t), what
    assert batch.transformation.scale == serial.transformation.scale, what
    assert np.array_equal(np.ravel(batch.q), np.ravel(serial.q)), what
    assert (batch.best_index_, batch.n_iter_) == (serial.best_index_, serial.n_iter_), what
    assert batch.score[:8] == serial.score[:8], (what, batch.score[:8], serial.score[:8])
    assert batch.score.node is None and batch.score.maha2 is None and batch.score.logp is None, what


# ---------------------------------------------------------------------------------------------------------------------
# 9. the forest's own calls, the serial entries and the serial multi-start are left alone
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_multi_leaves_everything_else_alone(ctx, small_forest):
    g = load_golden("hgmm_reg_L2.npz")
    lc = float(g["lambda_c"])
    T = hgmm_tree.n_total(2)
    clouds, targets = small_forest
    build_forest(ctx, clouds, targets, 2)
    forest = lambda: ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, 0.01, 8, 1e-6, want_trace=True)
    f_before = forest()
    fs_before = ctx.tree_score_batch(f_before[0], f_before[1], 1.0, 0.01)
    ctx.tree_set_nodes(2, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(g["rot10_target"])
    serial = lambda: ctx.tree_register(I3, Z3, 1.0, lc, 8, 1e-6, None, want_trace=True)
    s_before = serial()
    s_rot, s_t = five_starts(np.asarray(g["rot10_target"]).mean(axis=0))
    sm = lambda: ctx.tree_register_multi(s_rot, s_t, 1.0, lc, 8, 1e-6, want_trace=True)
    sm_before = sm()
    sms_before = ctx.tree_score_multi(sm_before[0], sm_before[1], 1.0, lc, CHI2)
    m_before = ctx.tree_reg_estep(T, I3, Z3, 1.0, lc)         # (leaves its [T][10] sums behind in the serial buffer)

    pair = [2, 1, 0, 1, 2, 1, 1, 2, 1]
    rot0, t0 = hypotheses(targets, pair)
    first = ctx.tree_register_batch_multi(pair, rot0, t0, 1.0, 0.01, 8, 1e-6, want_trace=True)
    fsum = ctx.tree_score_batch_multi(pair, first[0], first[1], 1.0, 0.01, CHI2)

    for x, y in zip(m_before, ctx.tree_reg_estep(T, I3, Z3, 1.0, lc)):
        assert np.array_equal(x, y)
    for x, y in zip(s_before, serial()):
        assert np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    sm_after = sm()
    for x, y in zip(sm_before[:5], sm_after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(sm_before[5], sm_after[5]))
    assert np.array_equal(sms_before, ctx.tree_score_multi(sm_before[0], sm_before[1], 1.0, lc, CHI2))
    # a second call, of fewer hypotheses, after all the others: the first call's bits for those
    second = ctx.tree_register_batch_multi(pair[:4], rot0[:4], t0[:4], 1.0, 0.01, 8, 1e-6, want_trace=True)
    for x, y in zip(first[:5], second[:5]):
        assert np.array_equal(x[:4], y)
    assert all(np.array_equal(x, y) for x, y in zip(first[5][:4], second[5]))
    assert np.array_equal(fsum[:4], ctx.tree_score_batch_multi(pair[:4], second[0], second[1], 1.0, 0.01, CHI2))
    # the forest registers and scores as before
    f_after = forest()
    for x, y in zip(f_before[:5], f_after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(f_before[5], f_after[5]))
    assert np.array_equal(fs_before, ctx.tree_score_batch(f_before[0], f_before[1], 1.0, 0.01))


# ---------------------------------------------------------------------------------------------------------------------
# 10. rounds: the mirror under a cap that makes it take three
# ---------------------------------------------------------------------------------------------------------------------
def test_three_rounds_give_the_bits_of_one(ctx, small_forest, monkeypatch):
    from hgmm_amd import _native
    from hgmm_amd.hgmm.hgmm_gpu import RigidTransformation, registration_gmmtree_batch
    clouds, targets = small_forest
    counts = (1, 5, 3)
    starts = []
    for tg, k in zip(targets, counts):
        rot, t = five_starts(tg.mean(axis=0))
        starts.append([RigidTransformation(rot[j], t[j]) for j in range(k)])
    kw = dict(tree_level=2, maxiter=6, tol=1e-6, starts=starts, return_info=True, ctx=ctx)
    one, info1 = registration_gmmtree_batch(list(zip(clouds, targets)), **kw)
    T = hgmm_tree.n_total(2)
    calls = []
    real = ctx.tree_register_batch_multi
    monkeypatch.setattr(ctx, "tree_register_batch_multi", lambda pair, *a, **k: calls.append(len(pair)) or real(pair, *a, **k))
    monkeypatch.setattr(_native, "BATCH_MULTI_MAX_BYTES", 4 * 32 * T)           # four hypotheses a round: 4 + 4 + 1
    three, info3 = registration_gmmtree_batch(list(zip(clouds, targets)), **kw)
    assert calls == [4, 4, 1]
    for a, b in zip(one, three):
        assert np.array_equal(a.transformation.rot, b.transformation.rot) and np.array_equal(a.transformation.t, b.transformation.t)
        assert np.array_equal(a.q, b.q) and (a.best_index_, a.n_iter_) == (b.best_index_, b.n_iter_) and a.score[:8] == b.score[:8]
    for key in ("hypothesis_iters", "hypothesis_status"):
        assert info1[key] == info3[key]
    assert [[s[:8] for s in p] for p in info1["hypothesis_scores"]] == [[s[:8] for s in p] for p in info3["hypothesis_scores"]]
    assert [len(p) for p in info1["hypothesis_iters"]] == list(counts)


# ---------------------------------------------------------------------------------------------------------------------
# 11. the mirror: bitwise registration_gmmtree(starts=) per pair, and the 30-degree record recovered inside a batch
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_is_bitwise_the_serial_mirror_and_recovers_the_30_degree_record(ctx, record4, bunny):
    from hgmm_amd.hgmm.hgmm_gpu import registration_gmmtree, registration_gmmtree_batch, rotation_starts
    points = np.asarray(record4["points"], dtype=np.float64)
    bun = bunny.astype(np.float64)[3::8]
    pairs = [(points, np.asarray(record4["rot30_target"])), (bun, moved(bun, 5.0, [0, 0, 1], [0.002, 0.0, 0.001]))]
    # (the constants and the initial rows the record's own tree was built with: tools/gen_golden.py)
    kw = dict(tree_level=4, lambda_c=float(record4["lambda_c"]), ls=float(record4["ls"]), ld=float(record4["ld"]),
              sig2=float(record4["sig2"]), init_idx=np.asarray(record4["init_idx"]), ctx=ctx)
    starts = rotation_starts()
    serial = [registration_gmmtree(s, t, 30, 1e-4, starts=starts, **kw) for s, t in pairs]
    alone = registration_gmmtree(pairs[0][0], pairs[0][1], 30, 1e-4, return_score=True, **kw)
    print("serial mirror, pair 0: fitness %.4f from the identity, %.4f from start %d of the grid"
          % (alone.score.fitness, serial[0].score.fitness, serial[0].best_index_))
    assert alone.score.fitness < 0.6 and serial[0].score.fitness > 0.9       # the gap on the tree built here
    res, info = registration_gmmtree_batch(pairs, maxiter=30, tol=1e-4, starts=starts, return_info=True, **kw)
    for k in range(2):
        assert_same_winner(res[k], serial[k], "pair %d" % k)
        assert info["score"][k] is res[k].score and info["registration_iters"][k] == res[k].n_iter_
        assert len(info["hypothesis_iters"][k]) == len(info["hypothesis_status"][k]) == len(info["hypothesis_scores"][k]) == 27
        assert info["hypothesis_scores"][k][res[k].best_index_][:8] == res[k].score[:8]
    plain, plain_info = registration_gmmtree_batch(pairs, maxiter=30, tol=1e-4, score=True, return_info=True, **kw)
    print("batch, pair 0: fitness %.4f without starts, %.4f with" % (plain_info["score"][0].fitness, res[0].score.fitness))
    assert plain_info["score"][0].fitness < 0.6 and res[0].score.fitness > 0.9
    assert "hypothesis_iters" not in plain_info


def test_mirror_ragged_starts_voxels_and_register_pairs(ctx, bunny):
    from hgmm_amd.hgmm.hgmm_gpu import MultiStartResult, registration_gmmtree, registration_gmmtree_batch, rotation_starts
    from hgmm_amd.replicas import register_pairs
    b = bunny.astype(np.float64)
    clouds = [b[::6], b[3::7], bunny[1::9]]                      # (the last one float32: the two kinds of a call)
    pairs = [(c, moved(np.asarray(c, dtype=np.float64), 6.0, [0, 0, 1], [0.002, 0.0, 0.001])) for c in clouds]
    kw = dict(tree_level=3, ctx=ctx)
    grid = rotation_starts((-10, 10))
    starts = [grid[:3], grid[2:7], grid[5:6]]
    res = registration_gmmtree_batch(pairs, maxiter=8, tol=1e-5, starts=starts, **kw)
    for k, (s, t) in enumerate(pairs):
        assert_same_winner(res[k], registration_gmmtree(s, t, 8, 1e-5, starts=starts[k], **kw), "ragged, pair %d" % k)
    # voxel_size with starts; a gate and the solve on the device
    for extra in (dict(voxel_size=0.004), dict(maha2_gate=16.27, solve_on_device=True)):
        res = registration_gmmtree_batch(pairs[:2], maxiter=8, tol=1e-5, starts=grid[:4], **extra, **kw)
        for k, (s, t) in enumerate(pairs[:2]):
            assert_same_winner(res[k], registration_gmmtree(s, t, 8, 1e-5, starts=grid[:4], **extra, **kw), "%s, pair %d" % (extra, k))
    # register_pairs(batch=2) on one context: one list for all pairs, and one list per pair
    del kw["ctx"]
    for st in (grid[:4], starts):
        out = register_pairs(pairs, devices=[0], batch=2, maxiter=8, tol=1e-5, starts=st, score=True, **kw)
        assert len(out) == 3 and all(isinstance(r, MultiStartResult) for r in out)
        for k, (s, t) in enumerate(pairs):
            mine = st[k] if st is starts else st
            assert_same_winner(out[k], registration_gmmtree(s, t, 8, 1e-5, starts=mine, ctx=ctx, **kw), "register_pairs, pair %d" % k)


# ---------------------------------------------------------------------------------------------------------------------
# 12. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_multi_errors_name_their_cause(bunny):
    import hgmm_amd
    c = hgmm_amd.Context(0)
    try:
        b = bunny.astype(np.float64)
        clouds = [b[::40], b[5::50]]
        targets = [moved(x, 5.0, [0, 0, 1], [0.002, 0.0, 0.001]) for x in clouds]
        R, t = np.tile(I3, (2, 1, 1)), np.zeros((2, 3))
        calls = (c.tree_register_batch_multi, c.tree_score_batch_multi)
        for call in calls:
            with pytest.raises(hgmm_amd.HgmmError, match="(?i)no forest"):
                call([0, 1], R, t)
        T = hgmm_tree.n_total(2)
        idx = np.random.RandomState(72).randint(T, size=T)
        arrs = c.set_points_batch(clouds)
        c.tree_build_batch([len(a) for a in arrs], 2, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
        for call in calls:
            with pytest.raises(hgmm_amd.HgmmError, match="(?i)no targets"):
                call([0, 1], R, t)
        c.tree_set_targets_batch(targets)
        for call in calls:
            with pytest.raises(hgmm_amd.HgmmError, match="R = 0"):
                call([], np.zeros((0, 3, 3)), np.zeros((0, 3)))
            with pytest.raises(hgmm_amd.HgmmError, match=r"pair\[1\] = 2"):
                call([0, 2], R, t)
            with pytest.raises(hgmm_amd.HgmmError, match=r"pair\[0\] = -1"):
                call([-1, 1], R, t)
            with pytest.raises(ValueError):
                call([0], R, t)
        with pytest.raises(hgmm_amd.HgmmError, match="NaN"):
            c.tree_score_batch_multi([0, 1], R, t, maha2_max=float("nan"))
        # NULL pair / rot / outputs, straight through the C ABI: the code and the text
        q, it, st, out = np.full(2, np.nan), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros((2, 8))
        pair = np.array([0, 1], np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        lib = c.lib
        rc = lib.hgmm_tree_register_batch_multi(c.h, 2, None, p(R), p(t), 1.0, 0.01, 5, 1e-4, p(q), p(it), p(st), None)
        assert rc == HGMM_ERR_ARG and b"pair" in lib.hgmm_last_error(c.h)
        rc = lib.hgmm_tree_score_batch_multi(c.h, 2, None, p(R), p(t), 1.0, 0.01, CHI2, p(out))
        assert rc == HGMM_ERR_ARG and b"pair" in lib.hgmm_last_error(c.h)
        rc = lib.hgmm_tree_register_batch_multi(c.h, 2, p(pair), None, p(t), 1.0, 0.01, 5, 1e-4, p(q), p(it), p(st), None)
        assert rc == HGMM_ERR_ARG and b"rot" in lib.hgmm_last_error(c.h)
        rc = lib.hgmm_tree_score_batch_multi(c.h, 2, p(pair), None, p(t), 1.0, 0.01, CHI2, p(out))
        assert rc == HGMM_ERR_ARG and b"rot" in lib.hgmm_last_error(c.h)
        rc = lib.hgmm_tree_register_batch_multi(c.h, 2, p(pair), p(R), p(t), 1.0, 0.01, 5, 1e-4, p(q), None, p(st), None)
        assert rc == HGMM_ERR_ARG and b"NULL" in lib.hgmm_last_error(c.h)
        rc = lib.hgmm_tree_score_batch_multi(c.h, 2, p(pair), p(R), p(t), 1.0, 0.01, CHI2, None)
        assert rc == HGMM_ERR_ARG and b"summary_out" in lib.hgmm_last_error(c.h)
        # and the context still works
        rot, tt, iters, _, status, _ = c.tree_register_batch_multi([1, 0], R, t, 1.0, 0.01, 3, 1e-6)
        assert (iters > 0).all()
        assert c.tree_score_batch_multi([1, 0], rot, tt)[:, 0].tolist() == [len(targets[1]), len(targets[0])]
        # the cap: 32 T bytes of sums per hypothesis, 4 GiB in all -- at L = 5 (T = 37448) 3584 hypotheses fit
        cloud = b[::16]
        arrs = c.set_points_batch([cloud])
        T5 = hgmm_tree.n_total(5)
        assert (4 << 30) // (32 * T5) == 3584
        c.tree_build_batch([len(cloud)], 5, 20.0, 1e-4, cloud[np.random.RandomState(72).randint(len(cloud), size=T5)][None], 0.004,
                           want_tables=False)
        c.tree_set_targets_batch([cloud[:100]])
        many = 3585
        for call in calls:
            with pytest.raises(hgmm_amd.HgmmError, match="at most R = 3584 "):
                call(np.zeros(many, np.int32), np.tile(I3, (many, 1, 1)), np.zeros((many, 3)))
        assert c.tree_score_batch_multi([0, 0], R, t)[:, 0].tolist() == [100, 100]
    finally:
        c.close()
