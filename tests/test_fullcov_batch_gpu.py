"""GPU tests of the batched flat full-covariance fit (hgmm_fullcov_fit_batch / _rows, Context.fullcov_fit_batch,
fitFullCovGMM_batch, fit_frames(flavour="full")): every member of a batch bit for bit the serial fit of that cloud alone on
the same context -- tables, labels, q trace, iteration count --, whatever its neighbours are; the members against the float64
oracle at the tolerances of tests/test_fullcov_gpu.py and tests/test_fullcov_weights_gpu.py; the refusals by name."""
import functools
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import hgmm_tree
from _fullcov_weight_oracle import build_flat_fullcov_w, init_rows
from test_fullcov_batch_cpu import RAGGED_ITERS, RAGGED_N, LD, SIG2, ragged_case, sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


_BUNNY = {}


@pytest.fixture(autouse=True)
def _share_bunny(bunny):
    _BUNNY["xyz"] = bunny


def _idx(P, J, N):
    return np.random.RandomState(J + N).choice(len(P), J, replace=len(P) < J)


@functools.lru_cache(maxsize=None)
def _oracle(N, J, ls, budget):
    """the oracle's fit of the N-point subsample, computed once per case"""
    P = sub(_BUNNY["xyz"], N)
    return hgmm_tree.build_flat_fullcov(P, J, ls, LD, _idx(P, J, N), SIG2, max_iters=budget)


def _serial(ctx, P, J, ls, budget, idx, w=None, weighted=False, ld=LD, sig2=SIG2):
    ctx.set_points(P)
    if w is not None:
        ctx.tree_set_source_weights(w)
    return ctx.fullcov_fit(J, ls, ld, P[idx], sig2, budget, weighted=weighted)


def _batch(ctx, Ps, J, ls, budget, idxs, ws=None, weighted=False, ld=LD, sig2=SIG2):
    """-> one (pi, mu, cov, labels, q) per member"""
    ctx.set_points_batch(Ps, weights=ws)
    pi, mu, cov, labels, q = ctx.fullcov_fit_batch([len(P) for P in Ps], J, ls, ld, init_mu=np.stack([P[i] for P, i in zip(Ps, idxs)]),
                                                   sig2=sig2, max_iters=budget, weighted=weighted)
    return [(pi[b], mu[b], cov[b], labels[b], q[b]) for b in range(len(Ps))]


def _same_bits(a, b):
    """bit for bit, NaNs included"""
    return len(a) == len(b) and all(np.asarray(u).shape == np.asarray(v).shape and
                                    np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes() for u, v in zip(a, b))


def _assert_oracle(got, ref):
    """the tolerances of tests/test_fullcov_gpu.py (test_fullcov_vs_oracle)"""
    pi, mu, cov, labels, q = got
    o_pi, o_mu, o_cov, o_q, o_cur = ref
    assert len(q) == len(o_q)
    np.testing.assert_allclose(q, o_q, rtol=1e-9, atol=1e-6)
    assert np.array_equal(labels, o_cur)
    np.testing.assert_allclose(pi, o_pi, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(mu, o_mu, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(cov, o_cov, rtol=1e-6, atol=1e-14)


# ---- 1. a ragged batch whose members stop on their own -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(ctx, bunny):
    """J = 16, ls = 1.0, budget 40, members of 1 .. 5032 points in ONE call, and the serial fit of each on the same context"""
    Ps, idxs = ragged_case(bunny)
    got = _batch(ctx, Ps, 16, 1.0, 40, idxs)
    serial = [_serial(ctx, P, 16, 1.0, 40, i) for P, i in zip(Ps, idxs)]
    return Ps, idxs, got, serial


def test_ragged_batch_members_stop_on_their_own(ctx, ragged):
    """Sizes on either side of the 16-point tile, 5032 points = more tiles than CUs (the grid is capped for that member
    only); the oracle's iteration counts 2 .. 40 (tests/test_fullcov_batch_cpu.py holds them and their margins >= 0.11)."""
    Ps, idxs, got, serial = ragged
    print("iterations", [len(g[4]) for g in got], "serial", [len(s[4]) for s in serial])
    assert [len(g[4]) for g in got] == RAGGED_ITERS
    for b, N in enumerate(RAGGED_N):
        assert _same_bits(got[b], serial[b]), "member %d (N = %d) differs from its serial fit" % (b, N)
        _assert_oracle(got[b], _oracle(N, 16, 1.0, 40))


# ---- 2. neighbours do not matter ----------------------------------------------------------------------------------------------
def test_neighbours_do_not_matter(ctx, ragged):
    """the same members in reversed order, each as a batch of one, and a batch of twice the same member"""
    Ps, idxs, got, _ = ragged
    rev = _batch(ctx, Ps[::-1], 16, 1.0, 40, idxs[::-1])[::-1]
    for b in range(len(Ps)):
        assert _same_bits(rev[b], got[b]), "member %d depends on its place" % b
        one = _batch(ctx, [Ps[b]], 16, 1.0, 40, [idxs[b]])
        assert _same_bits(one[0], got[b]), "member %d differs as a batch of one" % b
    for b in (2, 6):
        twice = _batch(ctx, [Ps[b], Ps[b]], 16, 1.0, 40, [idxs[b], idxs[b]])
        assert _same_bits(twice[0], got[b]) and _same_bits(twice[1], got[b])


# ---- 3. the reference golden inside a batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [8, 32])
def test_reference_golden_inside_a_batch(ctx, bunny, J):
    """fullcov_flat.npz as member 1 of 3 next to bunny subsamples: test_fullcov_matches_reference_golden's tolerances"""
    g = load_golden("fullcov_flat.npz")
    P = np.ascontiguousarray(g["points"], dtype=np.float64)
    tag = "J%d_" % J
    A, C = sub(bunny, 777), sub(bunny, 1300)
    got = _batch(ctx, [A, P, C], J, 80.0, 1000, [_idx(A, J, 777), g[tag + "init_idx"], _idx(C, J, 1300)], sig2=0.00034)
    pi, mu, cov, labels, q = got[1]
    np.testing.assert_allclose(q, g[tag + "q_trace"], rtol=1e-9, atol=1e-6)
    assert np.array_equal(labels, g[tag + "current_idx"])
    np.testing.assert_allclose(pi, g[tag + "pi"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(mu, g[tag + "mu"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cov, g[tag + "cov"], rtol=1e-7, atol=1e-14)
    assert _same_bits(got[1], _serial(ctx, P, J, 80.0, 1000, g[tag + "init_idx"], sig2=0.00034))


# ---- 4. component layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [17, 100, 513, 540, 1024])
def test_component_layouts(ctx, bunny, J):
    """one and two components per lane, a tail block, a partly filled last wave: members of 1300 and 40 points, three
    iterations, against the serial call bitwise and against the oracle"""
    Ps = [sub(bunny, 1300), sub(bunny, 40)]
    idxs = [_idx(P, J, len(P)) for P in Ps]
    got = _batch(ctx, Ps, J, 1e-30, 3, idxs)
    for b, P in enumerate(Ps):
        assert _same_bits(got[b], _serial(ctx, P, J, 1e-30, 3, idxs[b]))
        _assert_oracle(got[b], _oracle(len(P), J, 1e-30, 3))


# ---- 5. the budget boundaries of the host loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [1, 4, 5, 9])
def test_budget_boundaries(ctx, bunny, budget):
    """ls = 1e-30 never stops a member: every one runs to the budget, whichever way the host's look-ahead falls on it"""
    J = 24
    Ps = [sub(bunny, N) for N in (31, 1300, 2095)]
    idxs = [_idx(P, J, len(P)) for P in Ps]
    got = _batch(ctx, Ps, J, 1e-30, budget, idxs)
    for b, P in enumerate(Ps):
        assert len(got[b][4]) == budget
        assert _same_bits(got[b], _serial(ctx, P, J, 1e-30, budget, idxs[b]))


# ---- 6. weights ------------------------------------------------------------------------------------------------------------------
def _weight_members(bunny):
    """integer weights 0..4, w == 1, None, and integer weights with row 0 at weight zero.  (No NaN coordinates: the serial
    weighted entry does not cover non-finite coordinates -- include/hgmm.h -- so the zero-weight row keeps its own.)"""
    Ps = [sub(bunny, N) for N in (1300, 777, 601, 333)]
    ws = [np.random.RandomState(5).randint(0, 5, 1300).astype(np.float64), np.ones(777), None,
          np.random.RandomState(7).randint(1, 4, 333).astype(np.float64)]
    ws[3][0] = 0.0
    return Ps, ws


def test_weights(ctx, bunny):
    J, ls, budget = 24, 1e-30, 6                                        # (no stop decision for rounding to change)
    Ps, ws = _weight_members(bunny)
    idxs = [init_rows(np.ones(len(P)) if w is None else w, J) for P, w in zip(Ps, ws)]
    got = _batch(ctx, Ps, J, ls, budget, idxs, ws=ws, weighted=True)
    for b, (P, w) in enumerate(zip(Ps, ws)):
        if w is None:          # a member without weights: its unweighted serial fit
            assert _same_bits(got[b], _serial(ctx, P, J, ls, budget, idxs[b]))
        else:
            assert _same_bits(got[b], _serial(ctx, P, J, ls, budget, idxs[b], w=w, weighted=True))
        # tests/_fullcov_weight_oracle.py at the tolerances of tests/test_fullcov_weights_gpu.py (_assert_f64)
        _assert_oracle(got[b], build_flat_fullcov_w(P, J, ls, LD, idxs[b], SIG2, budget, w))
    assert _same_bits(got[1], _serial(ctx, Ps[1], J, ls, budget, idxs[1]))      # w == 1: the unweighted bits
    # weighted = 0 ignores the resident weights
    ctx.set_points_batch(Ps, weights=ws)
    pi, mu, cov, labels, q = ctx.fullcov_fit_batch([len(P) for P in Ps], J, ls, LD, init_mu=np.stack([P[i] for P, i in zip(Ps, idxs)]),
                                                   sig2=SIG2, max_iters=budget)
    assert _same_bits((pi[0], mu[0], cov[0], labels[0], q[0]), _serial(ctx, Ps[0], J, ls, budget, idxs[0]))


def test_weight_two_scales_exactly_per_member(ctx, bunny):
    """w == 2 with ls and ld doubled: every member's tables, labels and iteration count bitwise those of the unweighted batch,
    exactly twice its q trace"""
    J = 24
    Ps = [sub(bunny, N) for N in (1300, 333, 64)]
    idxs = [_idx(P, J, len(P)) for P in Ps]
    a = _batch(ctx, Ps, J, 20.0, 30, idxs)
    b = _batch(ctx, Ps, J, 40.0, 30, idxs, ws=[np.full(len(P), 2.0) for P in Ps], weighted=True, ld=2 * LD)
    print("iterations", [len(m[4]) for m in a])
    assert len({len(m[4]) for m in a}) > 1                             # (the stop rule decided, member by member)
    for u, v in zip(a, b):
        assert _same_bits(u[:4], v[:4]) and np.array_equal(2.0 * u[4], v[4])


# ---- 7. voxels -------------------------------------------------------------------------------------------------------------------
def test_voxel_batch_is_the_serial_voxel_fit(ctx, bunny):
    from hgmm_amd.hgmm.hgmm_gpu import fitFullCovGMM, fitFullCovGMM_batch
    full = bunny.astype(np.float64)
    vcs = ctx.voxel_down_sample_batch([full, full[::2], full[1::3]], 0.004, download=False).members()
    kw = dict(ctx=ctx, return_trace=True)                              # (the functions' own ls, ld, sig2, draw and budget)
    got = fitFullCovGMM_batch(vcs, 16, **kw)
    print("iterations", [len(g[3]["q_trace"]) for g in got])
    for b, vc in enumerate(vcs):
        ref = fitFullCovGMM(vc, 16, **kw)
        assert _same_bits(got[b][:3], ref[:3])
        assert np.array_equal(got[b][3]["labels"], ref[3]["labels"]) and np.array_equal(got[b][3]["q_trace"], ref[3]["q_trace"])
    # init_rows and init_mu give the same bits
    counts = ctx.set_points_batch_from_voxels(vcs, weighted=True)
    rows = np.stack([np.random.RandomState(b).choice(n, 16, replace=False) for b, n in enumerate(counts)])
    first = np.concatenate(([0], np.cumsum(counts)[:-1]))
    mu0 = ctx.points_rows((rows + first[:, None]).reshape(-1)).reshape(len(counts), 16, 3)
    by_rows = ctx.fullcov_fit_batch(counts, 16, 20.0, 1e-4, init_rows=rows, max_iters=10, weighted=True)
    by_mu = ctx.fullcov_fit_batch(counts, 16, 20.0, 1e-4, init_mu=mu0, max_iters=10, weighted=True)
    assert _same_bits(by_rows[:3], by_mu[:3])
    assert all(np.array_equal(u, v) for u, v in zip(by_rows[3], by_mu[3])) and all(np.array_equal(u, v) for u, v in zip(by_rows[4], by_mu[4]))


# ---- 8. the Cholesky flag is a member's own ----------------------------------------------------------------------------------------
def test_cholesky_flag_is_per_member(ctx, bunny):
    """A member on a straight line far from the origin (x = the bunny's, y = 1e6, z = -7e5): its y and z (co)variances are
    rounding noise of either sign around 1e-4, so among 64 components some have det >= 1e-15 with two negative eigenvalues --
    Sigma^-1 fails the Cholesky test and the serial fit of that cloud takes the symmetric form (hgmm_tree_stats' flag; found
    with the oracle's covariances: ~3 of 16 components in the first M-step).  Its well-conditioned neighbour keeps the
    triangular form: bit for bit its serial fit, before or behind the flagged member."""
    J = 64
    line = sub(bunny, 600).copy()
    line[:, 1], line[:, 2] = 1.0e6, -0.7e6
    good = sub(bunny, 777)
    i_line, i_good = _idx(line, J, 600), _idx(good, J, 777)
    s_line = _serial(ctx, line, J, 1e-30, 3, i_line)
    assert ctx.tree_stats()[1] & 1, "the line cloud did not fail the Cholesky test: the case does not test what it should"
    s_good = _serial(ctx, good, J, 1e-30, 3, i_good)
    assert not ctx.tree_stats()[1] & 1
    for order in ((0, 1), (1, 0)):
        Ps, idxs, ser = [(line, good)[o] for o in order], [(i_line, i_good)[o] for o in order], [(s_line, s_good)[o] for o in order]
        got = _batch(ctx, Ps, J, 1e-30, 3, idxs)
        for b in range(2):
            assert _same_bits(got[b], ser[b]), "order %s member %d" % (order, b)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(ctx, bunny):
    import hgmm_amd
    J = 24
    Ps = [sub(bunny, 333), sub(bunny, 64)]
    idxs = [_idx(P, J, len(P)) for P in Ps]
    counts = [len(P) for P in Ps]
    mu0 = np.stack([P[i] for P, i in zip(Ps, idxs)])
    ref = _serial(ctx, Ps[0], J, 1e-30, 3, idxs[0])

    def refused(match, counts=counts, J=J, **kw):
        args = dict(init_mu=mu0, sig2=SIG2, max_iters=3)
        args.update(kw)
        with pytest.raises(hgmm_amd.HgmmError, match=match):
            ctx.fullcov_fit_batch(counts, J, 1e-30, LD, **args)

    def serial_still_gives_its_bits():
        assert _same_bits(_serial(ctx, Ps[0], J, 1e-30, 3, idxs[0]), ref)

    ctx.set_points(Ps[0])
    refused("no batch cloud is resident")                               # a serial cloud is no forest cloud
    serial_still_gives_its_bits()
    ctx.set_points_batch(Ps)
    refused("B = 3, but 2 clouds are resident", counts=counts + [5], init_mu=np.zeros((3, J, 3)))
    refused(r"counts\[1\] = 63", counts=[333, 63])
    refused("B = 0 outside 1..4096", counts=[], init_mu=np.zeros((0, J, 3)))
    refused("B = 4097 outside 1..4096", counts=[1] * 4097, init_mu=np.zeros((4097, J, 3)))
    refused("one-pass float64 kernel only", J=1025, init_mu=np.zeros((2, 1025, 3)))
    with ctx.config(fullcov_two_pass=1):
        refused("fullcov_two_pass")
    ctx.tree_set_precision(np.float32)
    try:
        refused("F32_PDF")
    finally:
        ctx.tree_set_precision(np.float64)
    refused("no source weights of the batch cloud", weighted=True)
    refused(r"init_rows\[1\]\[0\] = 64, but member 1 has 64 points", init_mu=None,
            init_rows=np.concatenate((np.zeros((1, J), np.int64), np.full((1, J), 64, np.int64))))
    refused(r"init_rows\[0\]\[0\] = -1", init_mu=None, init_rows=np.full((2, J), -1, np.int64))
    # NULL init_mu / init_rows: below the binding, which never passes one
    import ctypes as C
    cnt = (C.c_int64 * 2)(*counts)
    out = [np.empty((2, J)), np.empty((2, J, 3)), np.empty((2, J, 3, 3))]
    qlen = np.zeros(2, np.int32)
    for entry, name in ((ctx.lib.hgmm_fullcov_fit_batch, "init_mu is NULL"), (ctx.lib.hgmm_fullcov_fit_batch_rows, "init_rows is NULL")):
        rc = entry(ctx.h, 2, cnt, J, 1e-30, LD, None, SIG2, 3, 0, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None,
                   None, 0, qlen.ctypes.data)
        assert rc != 0 and name in ctx.lib.hgmm_last_error(ctx.h).decode()
    # after all of them the batch still runs on the resident cloud, and a serial fit gives its bits
    assert _same_bits(_batch(ctx, Ps, J, 1e-30, 3, idxs)[0], ref)
    # a communicator (host backend, world of one)
    ctx.set_points_batch(Ps)
    ctx.comm_init_host(1, 0, "hgmm_fullcov_b1_%d" % os.getpid())
    try:
        refused("communicator")
    finally:
        ctx.comm_destroy()
    serial_still_gives_its_bits()


# ---- 10. the mirrors ----------------------------------------------------------------------------------------------------------------
def test_mirrors(ctx, bunny):
    from hgmm_amd import replicas
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints, fitFullCovGMM, fitFullCovGMM_batch
    kw = dict(ls=20.0, max_iters=12, ctx=ctx, return_trace=True)
    Ps = [sub(bunny, N) for N in (1300, 333, 64)]
    w1 = np.random.RandomState(3).randint(1, 4, 333).astype(np.float64)

    def same(a, b):
        return _same_bits(a[:3], b[:3]) and np.array_equal(a[3]["labels"], b[3]["labels"]) and np.array_equal(a[3]["q_trace"], b[3]["q_trace"])

    clouds = [Ps[0], WeightedPoints(Ps[1], w1), Ps[2]]
    got = fitFullCovGMM_batch(clouds, 16, **kw)
    assert all(same(g, fitFullCovGMM(c, 16, **kw)) for g, c in zip(got, clouds))
    assert not _same_bits(got[1][:1], fitFullCovGMM(Ps[1], 16, **kw)[:1])               # (the member's weights count)
    got = fitFullCovGMM_batch(Ps, 16, weights=[None, w1, None], **kw)                 # ... and as an explicit list
    assert all(same(g, fitFullCovGMM(c, 16, **kw)) for g, c in zip(got, clouds))
    plain = fitFullCovGMM_batch(Ps, 16, ls=20.0, max_iters=12, ctx=ctx)
    assert all(_same_bits(g, fitFullCovGMM(P, 16, ls=20.0, max_iters=12, ctx=ctx)) for g, P in zip(plain, Ps))
    # more components than the batched kernel takes: the members go through the serial function one by one
    big = fitFullCovGMM_batch(Ps[:1], 1040, ls=1e-30, max_iters=2, ctx=ctx)
    assert _same_bits(big[0], fitFullCovGMM(Ps[0], 1040, ls=1e-30, max_iters=2, ctx=ctx))
    vcs = ctx.voxel_down_sample_batch([bunny.astype(np.float64)], 0.004, download=False).members()
    with pytest.raises(ValueError, match="cannot be mixed"):
        fitFullCovGMM_batch([vcs[0], Ps[0]], 16, ctx=ctx)
    # fit_frames(flavour="full"): batch = 4 against batch = 1, from arrays and through the voxel result
    frames = [sub(bunny, N) for N in (1300, 777, 333, 2095, 601)]
    a = replicas.fit_frames(frames, 16, max_iter=12, tol=20.0, flavour="full", devices=[0], batch=1)
    b = replicas.fit_frames(frames, 16, max_iter=12, tol=20.0, flavour="full", devices=[0], batch=4)
    assert len(a) == len(b) == 5 and all(_same_bits(u, v) for u, v in zip(a, b))
    scans = [bunny.astype(np.float64), bunny[::2].astype(np.float64), bunny[1::3].astype(np.float64)]
    a = replicas.fit_frames(scans, 16, max_iter=12, tol=20.0, flavour="full", devices=[0], batch=1, voxel_size=0.004)
    b = replicas.fit_frames(scans, 16, max_iter=12, tol=20.0, flavour="full", devices=[0], batch=4, voxel_size=0.004)
    assert len(a) == len(b) == 3 and all(_same_bits(u, v) for u, v in zip(a, b))
