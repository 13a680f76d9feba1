"""The batched KMeans initialiser (hgmm_kmeans_fit_batch, csrc/kmeans_batch.h; KMeans.fit_batch; the GMMReg flavour's
fit_batch): B clouds through the same launches, each bit for bit the serial fit of that cloud alone -- the serial entries
hgmm_kmeans_plusplus / _lloyd / _step on the member by itself are the reference of sections 1, 2, 4, 5 and 7, the float64
oracle (oracle/kmeans.py through tests/_kmeans_helpers.py) and the reference's recorded seeds that of section 3.

The members of one batch share k (the entry's contract), so wherever two inputs of the helpers differ in k -- the golden
'uniform' (k = 16) and 'blobs' (k = 20) clouds -- each gets a batch at its own k with the other cloud as its neighbour."""
import contextlib
import os

import numpy as np
import pytest

import _kmeans_helpers as H
from conftest import load_golden

pytestmark = pytest.mark.gpu

ACC = [pytest.param(0, id="default"), pytest.param(1, id="acc_regs")]
ERR_ARG, ERR_STATE = -2, -3          # include/hgmm.h


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def _acc(ctx, regs):
    return ctx.config(kmeans_acc_regs=1) if regs else contextlib.nullcontext()


def _centred(X):
    from hgmm_amd.kmeans import column_mean_var
    mean, var, Xc = column_mean_var(np.asarray(X, dtype=np.float64))
    return Xc, float(np.mean(var) * 1e-4)


def _draws(seed, n, k):
    """A first seed and the uniforms of the k - 1 later centres, as KMeans draws them (2 + int(log k) trials)."""
    rs = np.random.RandomState(seed)
    return int(rs.randint(n)), rs.uniform(size=(max(k - 1, 0), 2 + int(np.log(k))))


def serial(ctx, Xc, k, max_iter, tol_abs, first=None, rand=None, init=None):
    """The sequence the batch's member has to equal: set_points, kmeans_plusplus (or the explicit start), kmeans_lloyd with a
    label reset, one more kmeans_step when the loop stopped neither strictly nor for an empty cluster."""
    ctx.set_points(Xc)
    ids = None
    if init is None:
        ids, start = ctx.kmeans_plusplus(k, first, rand)
    else:
        start = np.array(init, dtype=np.float64)
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(start, max_iter, tol_abs, reset_labels=True)
    inertia = 0.0
    if pending is None and not strict:
        inertia = ctx.kmeans_step(centres)[2]
    return {"ids": ids, "seeds": start, "centres": centres, "n_iter": n_iter, "strict": int(strict),
            "status": int(pending is not None), "inertia": inertia, "labels": ctx.kmeans_labels()}


def batch(ctx, clouds, k, max_iter, tols, draws=None, inits=None):
    ctx.set_points_batch(clouds)
    counts = [len(c) for c in clouds]
    if inits is not None:
        return ctx.kmeans_fit_batch(counts, k, max_iter, tols, init_centres=np.stack(inits))
    return ctx.kmeans_fit_batch(counts, k, max_iter, tols, first_ids=[d[0] for d in draws],
                                rand_vals=np.stack([d[1] for d in draws]) if k > 1 else None)


def assert_member(res, b, ref, what=""):
    """Member b of a batch's raw outputs against the serial sequence's, bit for bit."""
    assert res["status"][b] == ref["status"], what
    if ref["ids"] is not None:
        assert np.array_equal(res["ids"][b], ref["ids"]), what
    assert np.array_equal(res["seeds"][b], ref["seeds"]), what
    if ref["status"]:
        return
    assert (res["n_iter"][b], res["strict"][b]) == (ref["n_iter"], ref["strict"]), what
    assert np.array_equal(res["centres"][b], ref["centres"]), what
    assert np.array_equal(res["labels"][b], ref["labels"]), what
    assert res["inertia"][b] == ref["inertia"], what


def assert_fit(a, b, what=""):
    """Everything KMeans.fit leaves behind."""
    assert np.array_equal(a.cluster_centers_, b.cluster_centers_), what
    assert np.array_equal(a.labels_, b.labels_), what
    assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_, what
    if b.init_indices_ is None:
        assert a.init_indices_ is None, what
    else:
        assert np.array_equal(a.init_indices_, b.init_indices_), what


# -- 1. the batch is the serial fit, bitwise ----------------------------------------------------------------------------
EDGE_SIZES = [255, 256, 257, 511, 512, 513, 4095, 4096, 4097]     # blocks of 256, assignment workgroups of 512, one seeding
KS = [1, 2, 3, 65, 100, 300, 1100]                                # workgroup (4096) against two
BATCHES = [1, 2, 5, 33]


@pytest.fixture(scope="module")
def members(bunny):
    """Ragged clouds by size: rows of the bunny drawn without replacement, the whole scan last."""
    rs = np.random.RandomState(20)
    def take(n):
        return np.asarray(bunny[rs.choice(len(bunny), n, replace=False)], dtype=np.float64)
    return take, {n: take(n) for n in EDGE_SIZES}, np.asarray(bunny, dtype=np.float64)


@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("k", KS)
def test_batch_is_the_serial_fit(ctx, members, k, regs):
    """n_b = k, the sizes around every grid's edge and the ~40 000-point scan, k over the scalar tail of the assignment
    (3), the 64-centre slots (65, 100), nslot 16 (300) and the two-pass register accumulator (1100), in batches of 1, 2, 5
    and 33: the C entry's raw outputs and everything KMeans.fit leaves equal the serial calls on each member alone."""
    from hgmm_amd.kmeans import KMeans
    take, by_size, scan = members
    raw = [take(k)] + [by_size[n] for n in EDGE_SIZES if n >= k] + [scan]
    max_iter = 50 if k < 1000 else 12
    with _acc(ctx, regs):
        cent = [_centred(X) for X in raw]
        draws = [_draws(100 + i, len(X), k) for i, X in enumerate(raw)]
        refs = [serial(ctx, Xc, k, max_iter, tol, *d) for (Xc, tol), d in zip(cent, draws)]
        assert refs[-1]["status"] == 0                                    # (empty clusters are section 5's)
        for B in BATCHES:
            pick = [(3 * B + 7 * i) % len(raw) for i in range(B)]            # (B = 33 repeats members, the scan among them)
            if B == 5:
                pick[2] = len(raw) - 1                                       # the scan in the middle
            res = batch(ctx, [cent[i][0] for i in pick], k, max_iter, [cent[i][1] for i in pick], [draws[i] for i in pick])
            for b, i in enumerate(pick):
                assert_member(res, b, refs[i], "B=%d member %d (n=%d)" % (B, b, len(raw[i])))
        # the Python mirror: an int seed gives every member a fresh RandomState, as a loop of fit does
        some = raw[1:4] + raw[-1:]
        km = KMeans(k, random_state=1, max_iter=max_iter, ctx=ctx)
        loop = [KMeans(k, random_state=1, max_iter=max_iter, ctx=ctx).fit(X) for X in some]
        for b, (f, g) in enumerate(zip(km.fit_batch(some), loop)):
            assert_fit(f, g, "fit_batch member %d" % b)


# -- 2. neighbours do not matter ------------------------------------------------------------------------------------------
def test_neighbours_do_not_matter(ctx, members):
    """One member first, last and in the middle of batches of other neighbours, twice in one batch, and alone: the same
    bits every time, the serial fit's."""
    take, by_size, scan = members
    k = 65
    me, others = by_size[4097], [by_size[513], scan[:9000], by_size[255], by_size[4096]]
    (Xc, tol), d = _centred(me), _draws(5, 4097, k)
    ref = serial(ctx, Xc, k, 50, tol, *d)
    oc = [_centred(X) for X in others]
    od = [_draws(60 + i, len(X), k) for i, X in enumerate(others)]
    def run(order):
        """order: indices into `others`, -1 for the member under test -> its positions' results"""
        cl = [Xc if i < 0 else oc[i][0] for i in order]
        res = batch(ctx, cl, k, 50, [tol if i < 0 else oc[i][1] for i in order], [d if i < 0 else od[i] for i in order])
        return res, [b for b, i in enumerate(order) if i < 0]
    for order in ([-1, 0, 1], [2, 3, -1], [1, -1, 0, 2], [-1, 3, -1], [-1]):
        res, at = run(order)
        for b in at:
            assert_member(res, b, ref, "order %s position %d" % (order, b))


# -- 3. against the oracle and the reference's seeds ---------------------------------------------------------------------
LOOP_PARTNER = {3000: 4000, 4000: 5000, 5000: 6000, 6000: 4000}


@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("n,k", H.LOOP_CASES)
def test_batch_vs_oracle(ctx, n, k, regs):
    """Two H.loop_case clouds of one k from explicit starts in one batch, to strict convergence: labels and iteration
    counts are the oracle's (both inputs are fair: asserted first), the centres agree to the 1e-12 of the Lloyd tests."""
    cases = [(n, k), (LOOP_PARTNER[n], k)]
    walks = [H.loop_walk(*c) for c in cases]
    for w in walks:
        H.assert_fair(w)
    clouds, inits = zip(*[H.loop_case(*c) for c in cases])
    with _acc(ctx, regs):
        res = batch(ctx, list(clouds), k, 60, [0.0, 0.0], inits=list(inits))
    for b, w in enumerate(walks):
        assert res["status"][b] == 0
        assert (res["n_iter"][b], bool(res["strict"][b])) == (w.n_iter, w.strict)
        assert np.array_equal(res["labels"][b], w.final_labels)
        np.testing.assert_allclose(res["centres"][b], w.centres, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["uniform", "blobs"])
def test_batch_seeding_picks_the_references_seeds(ctx, name):
    """The golden clouds seeded in a batch -- each at its own k, the other cloud its neighbour -- pick the point indices
    scikit-learn's k-means++ picked (tests/golden/kmeans_init.npz)."""
    from hgmm_amd.kmeans import KMeans
    g = load_golden("kmeans_init.npz")
    clouds = [g["uniform_X"], g["blobs_X"]]
    fits = KMeans(int(g[name + "_k"]), random_state=1, max_iter=50, ctx=ctx).fit_batch(clouds)
    me = fits[["uniform", "blobs"].index(name)]
    assert np.array_equal(me.init_indices_, g[name + "_init_indices"])
    assert me.n_iter_ == int(g[name + "_n_iter"])
    assert np.array_equal(me.labels_, g[name + "_labels"])


# -- 4. members stop on their own -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", H.BUDGETS + [50])
@pytest.mark.parametrize("name", ["uniform", "blobs"])
def test_members_stop_on_their_own(ctx, name, budget):
    """One cloud several times in one batch under tolerances of its own: tol 0 (strict at iteration 19 resp. 16) next to the
    tolerance stops of H.TOL_STOPS (the last iteration of a host batch of eight, the first of the next, one inside),
    under every budget of H.BUDGETS: each member has n_iter, strict and centres of its own serial run -- the oracle's count."""
    Xc, init = H.golden_case(name)
    stops = [m for nm, m in H.TOL_STOPS if nm == name]
    tols = [0.0] + [H.tol_for_stop(name, m) for m in stops]
    expect = [H.STRICT_AT[name]] + stops
    res = batch(ctx, [Xc] * len(tols), len(init), budget, tols, inits=[init] * len(tols))
    for b, (tol, m) in enumerate(zip(tols, expect)):
        ref = serial(ctx, Xc, len(init), budget, tol, init=init)
        assert_member(res, b, ref, "tol %g" % tol)
        assert res["n_iter"][b] == min(m, budget)
        assert bool(res["strict"][b]) == (b == 0 and budget >= m)


# -- 5. empty clusters ----------------------------------------------------------------------------------------------------
def _empty_cluster_batch(ctx, triples, empties):
    """triples: (X, init) in the cloud's own frame.  The C entry on the centred members, then KMeans.fit_batch."""
    from hgmm_amd.kmeans import KMeans
    k = len(triples[0][1])
    fi = [H.fit_inputs(X, init) for X, init in triples]
    res = batch(ctx, [f[0] for f in fi], k, 50, [f[2] for f in fi], inits=[f[1] for f in fi])
    assert [int(s) for s in res["status"]] == [int(b in empties) for b in range(len(triples))]
    for b, (Xc, init_c, tol) in enumerate(fi):
        assert_member(res, b, serial(ctx, Xc, k, 50, tol, init=init_c), "member %d" % b)     # (status 1: its start is valid)
    fits = KMeans(k, init=[init for _, init in triples], max_iter=50, ctx=ctx).fit_batch([X for X, _ in triples])
    for b, (X, init) in enumerate(triples):
        assert_fit(fits[b], KMeans(k, init=init, max_iter=50, ctx=ctx).fit(X), "member %d" % b)


def test_empty_cluster_in_iteration_1_between_fair_neighbours(ctx):
    _empty_cluster_batch(ctx, [H.loop_case(700, 8), H.reloc8_case(), H.loop_case(2000, 8)], {1})


def test_late_empty_clusters_next_to_a_fair_member(ctx):
    cases = [H.late_empty_case(*c[:5]) for c in H.LATE_EMPTY_CASES[:3]]
    assert all(len(init) == 20 for _, init in cases)
    _empty_cluster_batch(ctx, cases[:2] + [H.loop_case(1500, 20)] + cases[2:], {0, 1, 3})


def test_seeded_member_with_an_empty_cluster_reports_its_seeds(ctx):
    """A seeded member that meets an empty cluster (bitwise duplicate points make duplicate seeds likely: here forced, every
    point of the cloud is one of three sites and k = 5) leaves with status 1 and the serial seeds; fit_batch finishes it."""
    from hgmm_amd.kmeans import KMeans
    rs = np.random.RandomState(3)
    sites = rs.rand(3, 3)
    X = sites[rs.randint(3, size=300)]
    fair = np.asarray(H.loop_case(700, 8)[0])
    fits = KMeans(5, random_state=1, max_iter=50, ctx=ctx).fit_batch([fair, X, fair])
    for f, Y in zip(fits, [fair, X, fair]):
        assert_fit(f, KMeans(5, random_state=1, max_iter=50, ctx=ctx).fit(Y))
    (Xc, tol), d = _centred(X), _draws(1, 300, 5)
    res = batch(ctx, [Xc], 5, 50, [tol], [d])
    ref = serial(ctx, Xc, 5, 50, tol, *d)
    assert ref["status"] == 1
    assert_member(res, 0, ref)


# -- 6. refusals and state ------------------------------------------------------------------------------------------------
def _refused(ctx, code, needle, fn):
    import hgmm_amd
    with pytest.raises(hgmm_amd.HgmmError) as e:
        fn()
    assert "(%d)" % code in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_and_state():
    import hgmm_amd
    from hgmm_amd.kmeans import KMeans
    from oracle import hgmm_tree
    ctx = hgmm_amd.Context(0)
    try:
        rs = np.random.RandomState(0)
        P = rs.rand(8, 3)[rs.randint(8, size=3000)] + 0.03 * rs.randn(3000, 3)
        clouds = [_centred(P[:1500])[0], _centred(P[1500:2700])[0], _centred(P[2700:])[0]]          # 1500, 1200, 300
        counts, k = [1500, 1200, 300], 10
        draws = [_draws(i, n, k) for i, n in enumerate(counts)]
        first, rand = [d[0] for d in draws], np.stack([d[1] for d in draws])
        call = lambda **kw: ctx.kmeans_fit_batch(**{**dict(counts=counts, k=k, max_iter=5, tol_abs=0.0, first_ids=first,
                                                           rand_vals=rand), **kw})
        _refused(ctx, ERR_STATE, "no batch cloud", call)                                            # nothing resident
        ctx.set_points(P)
        _refused(ctx, ERR_STATE, "no batch cloud", call)                                            # a serial cloud
        # what has to survive: a voxel result, a forest on the batch cloud, a serial fit's result
        vox = ctx.voxel_down_sample(P, 0.05)
        ctx.set_points_batch(clouds)
        L, T = 2, hgmm_tree.n_total(2)
        idx = np.random.RandomState(72).randint(300, size=T)
        ctx.tree_build_batch(counts, L, 20.0, 1e-4, np.stack([c[idx] for c in clouds]), 0.004, 50)
        nodes = [ctx.tree_get_nodes_batch(b, L) for b in range(3)]

        def state_is_unchanged():
            for b in range(3):
                for a, c in zip(ctx.tree_get_nodes_batch(b, L), nodes[b]):
                    assert np.array_equal(a, c)
            for a, c in zip(ctx.voxel_down_sample_get(), vox):
                assert np.array_equal(a, c)

        bad_first = list(first)
        bad_first[1] = 1200
        for code, needle, kw in [
                (ERR_STATE, "3 clouds are resident", dict(counts=counts[:2], first_ids=first[:2], rand_vals=rand[:2])),
                (ERR_STATE, "member 2", dict(counts=[1500, 1200, 299])),
                (ERR_ARG, "k = 0", dict(k=0, rand_vals=None)),
                (ERR_ARG, "k = 16385", dict(k=16385, rand_vals=np.zeros((3, 16384, 1)))),
                (ERR_ARG, "member 2", dict(k=301, rand_vals=np.zeros((3, 300, 7)))),                 # k > counts[2]
                (ERR_ARG, "n_trials = 17", dict(rand_vals=np.zeros((3, k - 1, 17)))),
                (ERR_ARG, "member 1", dict(first_ids=bad_first)),
                (ERR_ARG, "max_iter", dict(max_iter=-1))]:
            _refused(ctx, code, needle, lambda: call(**kw))
            state_is_unchanged()
        # the argument combinations the binding refuses itself reach the library through the raw entry
        import ctypes as C
        cnt = np.array(counts, np.int64)
        out = dict(c=np.empty((3, k, 3)), i=np.empty((3, k), np.int64), s=np.empty((3, k, 3)), n=np.zeros(3, np.int32),
                   st=np.zeros(3, np.int32), x=np.zeros(3, np.int32), e=np.zeros(3), tol=np.zeros(3),
                   f=np.array(first, np.int64), init=np.zeros((3, k, 3)))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        def raw(first_ids, rand_vals, init, tol=out["tol"], centres=out["c"], B=3):
            return ctx.lib.hgmm_kmeans_fit_batch(ctx.h, B, p(cnt), k, p(first_ids), p(rand_vals), 7, p(init), 5, p(tol),
                                                 p(out["i"]), p(out["s"]), p(centres), p(out["n"]), p(out["st"]), p(out["x"]),
                                                 p(out["e"]), None)
        assert raw(out["f"], rand, out["init"]) == ERR_ARG and b"both" in ctx.lib.hgmm_last_error(ctx.h)
        assert raw(None, None, None) == ERR_ARG and b"neither" in ctx.lib.hgmm_last_error(ctx.h)
        assert raw(out["f"], None, None) == ERR_ARG and b"rand_vals" in ctx.lib.hgmm_last_error(ctx.h)
        assert raw(out["f"], rand, None, tol=None) == ERR_ARG and b"NULL" in ctx.lib.hgmm_last_error(ctx.h)
        assert raw(out["f"], rand, None, centres=None) == ERR_ARG and b"NULL" in ctx.lib.hgmm_last_error(ctx.h)
        for B in (0, 4097):
            assert raw(out["f"], rand, None, B=B) == ERR_ARG and b"B = %d" % B in ctx.lib.hgmm_last_error(ctx.h)
        state_is_unchanged()
        # a successful call leaves the same things alone, and a serial step without a reset still counts its changes
        # against the serial labels, not the batch's
        res = call()
        assert not res["status"].any()
        state_is_unchanged()
        c0, c1 = clouds[0][:k], clouds[0][k:2 * k]
        ctx.kmeans_step(c0, reset_labels=True)                             # (serial, on the packed cloud of 3000 rows)
        serial_labels = ctx.kmeans_labels()
        ctx.kmeans_step(c1, reset_labels=True)
        expect = int((ctx.kmeans_labels() != serial_labels).sum())
        assert 0 < expect < 3000
        ctx.kmeans_step(c0, reset_labels=True)
        call()
        assert np.array_equal(ctx.kmeans_labels(), serial_labels)
        assert ctx.kmeans_step(c1, reset_labels=False)[3] == expect
        before = KMeans(k, random_state=1, max_iter=20, ctx=ctx).fit(P)
        ctx.set_points_batch(clouds)
        _refused(ctx, ERR_ARG, "max_iter", lambda: call(max_iter=-1))
        call()
        assert_fit(KMeans(k, random_state=1, max_iter=20, ctx=ctx).fit(P), before)
        # under a communicator
        ctx.set_points_batch(clouds)
        ctx.comm_init_host(1, 0, "hgmm_km_batch_%d" % os.getpid())
        try:
            _refused(ctx, ERR_STATE, "communicator", call)
            with pytest.raises(ValueError, match="communicator"):
                KMeans(k, random_state=1, ctx=ctx).fit_batch(clouds)
        finally:
            ctx.comm_destroy()
    finally:
        ctx.close()


def test_resident_source_weights_are_ignored(ctx):
    """Weights on the batch cloud do not enter, as the unweighted serial entries ignore them."""
    clouds = [H.loop_case(700, 8)[0], H.loop_case(2000, 8)[0]]
    draws = [_draws(i, len(c), 8) for i, c in enumerate(clouds)]
    plain = batch(ctx, clouds, 8, 20, [0.0, 0.0], draws)
    ctx.set_points_batch(clouds, weights=[np.random.RandomState(b).rand(len(c)) + 0.5 for b, c in enumerate(clouds)])
    res = ctx.kmeans_fit_batch([len(c) for c in clouds], 8, 20, [0.0, 0.0], first_ids=[d[0] for d in draws],
                               rand_vals=np.stack([d[1] for d in draws]))
    for key in ("ids", "seeds", "centres", "n_iter", "strict", "inertia"):
        assert np.array_equal(res[key], plain[key]), key
    for a, b in zip(res["labels"], plain["labels"]):
        assert np.array_equal(a, b)


# -- 7. the consumer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(bunny):
    rs = np.random.RandomState(4)
    return [np.asarray(bunny[np.sort(rs.choice(len(bunny), n, replace=False))], dtype=np.float64)
            for n in (9000, 12345, 7001, 10240)]


def test_flavour_g_fit_batch_is_the_loop_of_fit(frames, capsys):
    from hgmm_amd.gmmreg_gpu.gmm import GMM_GPU_Base
    models = GMM_GPU_Base(100, max_iter=10).fit_batch(frames)
    for b, X in enumerate(frames):
        one = GMM_GPU_Base(100, max_iter=10).fit(X)
        for field in ("means_", "covariances_", "weights_", "lls"):
            assert np.array_equal(np.asarray(getattr(models[b], field)), np.asarray(getattr(one, field))), (b, field)


def test_fit_frames_flavour_g_batch_equals_serial(frames, capsys):
    from hgmm_amd import replicas
    with replicas.ReplicaPool([0]) as pool:
        a = replicas.fit_frames(frames, 100, 10, flavour="G", batch=4, pool=pool)
        b = replicas.fit_frames(frames, 100, 10, flavour="G", batch=1, pool=pool)
    for x, y in zip(a, b):
        for field in ("means_", "covariances_", "weights_", "lls"):
            assert np.array_equal(np.asarray(getattr(x, field)), np.asarray(getattr(y, field))), field
    with pytest.raises(ValueError, match="flavour"):
        replicas.fit_frames(frames, flavour="X")
