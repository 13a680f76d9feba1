"""Per-point weights for the KMeans initialiser on the device (csrc/kmeans_kernels.hip: the ``_w`` kernels behind
hgmm_kmeans_plusplus_weighted / _step_weighted / _lloyd_weighted) against the weighted restatement of
tests/_kmeans_weight_oracle.py, and the public layers above them.

tests/test_kmeans_weights_cpu.py pins the restatement to live scikit-learn and proves, on the restatement alone, that
every input used here is a fair one (every seeding decision 1e-10 of the potential away from flipping, every label
1e-10 away from a tie); the conditions a comparison rests on are asserted here once more where they are cheap."""
import contextlib
import os

import numpy as np
import pytest

import _kmeans_helpers as H
import _kmeans_weight_oracle as W
from oracle import kmeans as okm

pytestmark = pytest.mark.gpu

ACC = [pytest.param(0, id="default"), pytest.param(1, id="acc_regs")]


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def _acc(ctx, regs):
    return ctx.config(kmeans_acc_regs=1) if regs else contextlib.nullcontext()


def _load(ctx, X, w):
    ctx.set_points(X)
    ctx.tree_set_source_weights(w)


# -- 1. seeding and one step vs the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("n,k", W.SEED_CASES)
def test_seeding_and_one_step_vs_oracle(ctx, n, k):
    """Ragged blocks, the 4096-point group boundary, the 64-centre slot, the 256-centre allocation, the 1024-centre
    pass; the LDS accumulator up to k = 1024 and the register accumulator at k = 1100."""
    Xc, w, first, uniforms = W.seed_case(n, k)
    centres, ids, trace, lab, mind2, margin = W.seed_expect(n, k)
    if k > 1:
        assert min(trace.thr_margin) >= W.SEED_MARGIN_MIN and min(trace.pot_gap) >= W.SEED_MARGIN_MIN
        assert margin >= H.MARGIN_MIN
    _load(ctx, Xc, w)
    g_ids, g_centres = ctx.kmeans_plusplus(k, first, uniforms, weighted=True)
    assert np.array_equal(g_ids, ids)
    assert np.array_equal(g_centres, centres)
    g_sums, g_w, g_inertia, g_changed = ctx.kmeans_step(g_centres, reset_labels=True, weighted=True)
    g_lab, g_d2 = ctx.kmeans_labels(with_distances=True)
    assert np.array_equal(g_lab, lab)
    assert g_changed == n
    np.testing.assert_allclose(g_d2, mind2, rtol=1e-13, atol=0)
    assert np.array_equal(g_w, np.bincount(lab, weights=w, minlength=k))        # integer weights: exact
    sums, _ = W.step_sums_w(Xc, w, lab, k)
    np.testing.assert_allclose(g_sums, sums, rtol=0, atol=1e-11 * w.max())
    np.testing.assert_allclose(g_inertia, float((w * mind2).sum()), rtol=1e-12)
    s2, w2, i2, c2 = ctx.kmeans_step(g_centres, reset_labels=False, weighted=True)
    assert c2 == 0 and np.array_equal(s2, g_sums) and np.array_equal(w2, g_w) and i2 == g_inertia
    assert np.array_equal(ctx.kmeans_labels(), lab)


# -- 2. exact arithmetic -------------------------------------------------------------------------------
@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("n,k", W.LATTICE_W_CASES)
def test_lattice_step_is_exact(ctx, n, k, regs):
    """Lattice coordinates and weights in {0, 1, 2, 4}: every product and sum is an exactly representable double in any
    order, so labels (ties included), weights, sums and inertia are the oracle's exactly."""
    X, A, _, _ = H.lattice_case(n, k)
    w = W.lattice_weights(n, k)
    lab, mind2, _, _, _, _ = H.lattice_expect(X, A)
    sums, wsum = W.step_sums_w(X, w, lab, k)
    _load(ctx, X, w)
    with _acc(ctx, regs):
        g_sums, g_w, g_inertia, g_changed = ctx.kmeans_step(A, reset_labels=True, weighted=True)
        g_lab, g_d2 = ctx.kmeans_labels(with_distances=True)
    assert np.array_equal(g_lab, lab) and np.array_equal(g_d2, mind2)
    assert np.array_equal(g_w, wsum)
    assert np.array_equal(g_sums, sums)
    assert g_inertia == float((w * mind2).sum())
    assert g_changed == n


# -- 3. invariants on the device -------------------------------------------------------------------------
def _all_three(ctx, k, first, uniforms, init, weighted):
    ids, seeds = ctx.kmeans_plusplus(k, first, uniforms, weighted=weighted)
    sums, cnt, inertia, changed = ctx.kmeans_step(seeds, reset_labels=True, weighted=weighted)
    step_lab = ctx.kmeans_labels()
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 60, 0.0, weighted=weighted)
    return dict(ids=ids, seeds=seeds, sums=sums, cnt=cnt, inertia=inertia, changed=changed, step_lab=step_lab,
                centres=centres, n_iter=n_iter, strict=strict, pending=pending, labels=ctx.kmeans_labels())


def _same_bits(a, b, keys):
    for key in keys:
        x, y = a[key], b[key]
        assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), key


ALL_KEYS = ["ids", "seeds", "sums", "cnt", "inertia", "changed", "step_lab", "centres", "n_iter", "strict", "pending",
            "labels"]


@pytest.mark.parametrize("n,k", [(3000, 65), (6000, 1100)])
def test_unit_and_double_weights(ctx, n, k):
    """w = 1 through the weighted entries is the unweighted entries bit for bit; w = 2 leaves seeds, labels, centres and
    n_iter bit for bit and doubles sums, weights and inertia exactly; the unweighted entries return their bits with
    weights resident."""
    Xc, init = H.loop_case(n, k)
    ru = np.random.RandomState(5)
    first = int(ru.randint(n))
    uniforms = ru.uniform(size=(k - 1, okm.n_local_trials(k)))
    ctx.set_points(Xc)
    plain = _all_three(ctx, k, first, uniforms, init, False)
    assert plain["pending"] is None and plain["n_iter"] > 2
    ctx.tree_set_source_weights(np.ones(n))
    _same_bits(_all_three(ctx, k, first, uniforms, init, True), plain, ALL_KEYS)
    _same_bits(_all_three(ctx, k, first, uniforms, init, False), plain, ALL_KEYS)
    ctx.tree_set_source_weights(np.full(n, 2.0))
    twice = _all_three(ctx, k, first, uniforms, init, True)
    _same_bits(twice, plain, ["ids", "seeds", "changed", "step_lab", "centres", "n_iter", "strict", "pending", "labels"])
    assert np.array_equal(twice["sums"], 2.0 * plain["sums"])
    assert np.array_equal(twice["cnt"], 2.0 * plain["cnt"])
    assert twice["inertia"] == 2.0 * plain["inertia"]
    _same_bits(_all_three(ctx, k, first, uniforms, init, False), plain, ALL_KEYS)


# -- 4. the whole loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("regs", ACC)
@pytest.mark.parametrize("n,k", H.LOOP_CASES)
def test_whole_loop_vs_oracle(ctx, n, k, regs):
    Xc, init = H.loop_case(n, k)
    wk = W.loop_walk_w(n, k)
    W.assert_fair_w(wk)
    _load(ctx, Xc, W.count_weights(n, n + k + 1))
    with _acc(ctx, regs):
        centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, max_iter=60, tol_abs=0.0, weighted=True)
        labels = ctx.kmeans_labels()
    assert (n_iter, strict) == (wk.n_iter, wk.strict)
    assert pending is None
    assert np.array_equal(labels, wk.final_labels)
    np.testing.assert_allclose(centres, wk.centres, rtol=0, atol=1e-12)


# -- 5. stop rules and the batch of 8 -------------------------------------------------------------------
@pytest.fixture()
def uniform(ctx):
    Xc, init = H.golden_case("uniform")
    _load(ctx, Xc, W.count_weights(len(Xc), W.STOP_WEIGHT_SEED))
    return Xc, init


def _final_labels(ctx, centres, strict):
    if not strict:
        ctx.kmeans_step(centres, weighted=True)
    return ctx.kmeans_labels()


@pytest.mark.parametrize("budget", H.BUDGETS)
def test_budget_stop(ctx, uniform, budget):
    Xc, init = uniform
    wk = W.golden_walk_w("uniform", budget)
    W.assert_fair_w(wk)
    assert wk.n_iter == budget and not wk.strict
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, budget, 0.0, weighted=True)
    assert (n_iter, strict, pending) == (budget, False, None)
    np.testing.assert_allclose(centres, wk.centres, rtol=0, atol=1e-12)
    assert np.array_equal(_final_labels(ctx, centres, strict), wk.final_labels)


@pytest.mark.parametrize("which", [0, 1], ids=["inside_a_batch", "in_a_later_batch"])
def test_tolerance_stop(ctx, uniform, which):
    Xc, init = uniform
    m = W.tol_stops_w("uniform")[which]
    tol = W.tol_for_stop_w("uniform", m)
    wk = W.golden_walk_w("uniform", 50, tol)
    assert wk.n_iter == m and not wk.strict and (m < 8 if which == 0 else m > 8)
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 50, tol, weighted=True)
    assert (n_iter, strict, pending) == (m, False, None)
    np.testing.assert_allclose(centres, wk.centres, rtol=0, atol=1e-12)
    assert np.array_equal(_final_labels(ctx, centres, strict), wk.final_labels)


def test_strict_stop(ctx, uniform):
    Xc, init = uniform
    wk = W.golden_walk_w("uniform")
    assert wk.strict
    centres, n_iter, strict, pending = ctx.kmeans_lloyd(init, 50, 0.0, weighted=True)
    assert (n_iter, strict, pending) == (wk.n_iter, True, None)
    np.testing.assert_allclose(centres, wk.centres, rtol=0, atol=1e-12)
    assert np.array_equal(ctx.kmeans_labels(), wk.final_labels)


# -- 6. relocation handed to the host -------------------------------------------------------------------
@pytest.mark.parametrize("zeros", [False, True], ids=["positive_weights", "zero_weights"])
def test_relocation_in_iteration_one(ctx, zeros):
    """Three clusters of weight 0 in iteration 1; with zero weights the farthest point has weight 0 and the cluster it is
    given takes the heaviest cluster's row (both pinned to scikit-learn in the CPU file)."""
    from hgmm_amd.kmeans import KMeans
    X, init = H.reloc8_case()
    w = W.reloc8_weights(zeros)
    exp = W.fit_w(X, w, len(init), max_iter=50, tol=1e-4, init=init)
    assert exp["walk"].n_empty[0] == 3
    km = KMeans(n_clusters=len(init), init=init, max_iter=50, tol=1e-4, ctx=ctx).fit(X, sample_weight=w)
    assert km.n_iter_ == exp["n_iter_"]
    assert np.array_equal(km.labels_, exp["labels_"])
    np.testing.assert_allclose(km.cluster_centers_, exp["cluster_centers_"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(km.inertia_, exp["inertia_"], rtol=1e-12)


def test_relocation_after_the_device_has_advanced(ctx):
    """The ``LATE_EMPTY_CASES`` cloud whose trajectory under count weights still meets a cluster of weight 0 after
    iteration 1 (tests/test_kmeans_weights_cpu.py shows that one does, and that it is fair)."""
    from hgmm_amd.kmeans import KMeans
    n, k, blobs, spread, seed, hit = W.late_empty_pick()
    Xl, il = H.late_empty_case(n, k, blobs, spread, seed)
    w = W.count_weights(n, seed)
    exp = W.fit_w(Xl, w, k, max_iter=50, tol=0, init=il)
    assert H.first_empty(exp["walk"]) == hit > 1
    km = KMeans(n_clusters=k, init=il, max_iter=50, tol=0, ctx=ctx).fit(Xl, sample_weight=w)
    assert km.n_iter_ == exp["n_iter_"]
    assert np.array_equal(km.labels_, exp["labels_"])
    np.testing.assert_allclose(km.cluster_centers_, exp["cluster_centers_"], rtol=0, atol=1e-12)


# -- 7. many groups ------------------------------------------------------------------------------------
def test_many_groups(ctx):
    """n = 4.3 M: more than 1024 groups of 4096 points, so a thread of the seeding tail owns two group sums."""
    Xc, w, first, uniforms, ids, trace = W.many_groups_case()
    assert min(trace.thr_margin) >= W.MANY_MARGIN_MIN and min(trace.pot_gap) >= W.MANY_MARGIN_MIN
    _load(ctx, Xc, w)
    g_ids, g_centres = ctx.kmeans_plusplus(W.MANY_K, first, uniforms, weighted=True)
    assert np.array_equal(g_ids, ids)
    assert np.array_equal(g_centres, Xc[ids])


# -- 8. through the public layers -----------------------------------------------------------------------
def test_fit_on_the_bunny_centroids(ctx):
    from hgmm_amd.kmeans import KMeans
    C, cnt, exp = W.bunny_case()
    km = KMeans(n_clusters=W.BUNNY_K, random_state=1, max_iter=50, n_init=1, ctx=ctx).fit(C, sample_weight=cnt)
    assert np.array_equal(km.init_indices_, exp["init_indices"])
    assert km.n_iter_ == exp["n_iter_"]
    assert np.array_equal(km.labels_, exp["labels_"])
    np.testing.assert_allclose(km.cluster_centers_, exp["cluster_centers_"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(km.inertia_, exp["inertia_"], rtol=1e-12)
    plain = KMeans(n_clusters=W.BUNNY_K, random_state=1, max_iter=50, n_init=1, ctx=ctx).fit(C)
    assert not np.array_equal(plain.init_indices_, km.init_indices_)          # the weights are not a no-op here


def test_fit_on_the_bunny_centroids_vs_live_sklearn(ctx):
    cluster = pytest.importorskip("sklearn.cluster")
    from hgmm_amd.kmeans import KMeans
    C, cnt, _ = W.bunny_case()
    ref = cluster.KMeans(n_clusters=W.BUNNY_K, random_state=1, max_iter=50, n_init=1).fit(C, sample_weight=cnt)
    km = KMeans(n_clusters=W.BUNNY_K, random_state=1, max_iter=50, n_init=1, ctx=ctx).fit(C, sample_weight=cnt)
    assert km.n_iter_ == ref.n_iter_ and np.array_equal(km.labels_, ref.labels_)
    np.testing.assert_allclose(km.cluster_centers_, ref.cluster_centers_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(km.inertia_, ref.inertia_, rtol=1e-12)


def _fit_bits(km):
    return km.init_indices_, km.labels_, km.cluster_centers_, km.inertia_, km.n_iter_


def _assert_fit_bits(a, b):
    for x, y in zip(_fit_bits(a), _fit_bits(b)):
        assert np.array_equal(x, y)


def test_own_weights_and_the_default(ctx):
    """``"own"`` on a WeightedPoints or a VoxelCloud is the explicit array bit for bit; the default on a WeightedPoints
    keeps reading its points only; ``init_gmm_params`` hands the weights through."""
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    from hgmm_amd.kmeans import KMeans, kmeans_centres
    from hgmm_amd.gmmreg_gpu.gmm_impl import init_gmm_params
    C, cnt, _ = W.bunny_case()

    def km():
        return KMeans(n_clusters=W.BUNNY_K, random_state=1, max_iter=50, n_init=1, ctx=ctx)
    explicit = km().fit(C, sample_weight=cnt)
    _assert_fit_bits(km().fit(WeightedPoints(C, cnt), sample_weight="own"), explicit)
    _assert_fit_bits(km().fit(WeightedPoints(C, cnt)), km().fit(C))
    assert np.array_equal(km().fit_predict(C, sample_weight=cnt), explicit.labels_)
    assert np.array_equal(kmeans_centres(C, W.BUNNY_K, ctx=ctx, sample_weight=cnt), explicit.cluster_centers_)
    with hgmm_amd.use_context(ctx):
        means, pis = init_gmm_params(C, W.BUNNY_K, sample_weight=cnt)
        plain_means, _ = init_gmm_params(C, W.BUNNY_K)
    assert np.array_equal(means, explicit.cluster_centers_) and np.array_equal(pis, np.ones(W.BUNNY_K) / W.BUNNY_K)
    assert np.array_equal(plain_means, km().fit(C).cluster_centers_)
    # a VoxelCloud: the centroids and counts of the device's own down-sample
    bunny = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bun000_xyz.npy"))
    vc = ctx.voxel_down_sample(bunny.astype(np.float64), 0.004, download=False)
    pts, counts = vc.get()
    from_vc = km().fit(vc, sample_weight="own")
    _assert_fit_bits(from_vc, km().fit(pts, sample_weight=counts))


def test_weighted_init_of_the_estimator(ctx):
    """``GMM_GPU(..., weighted_init=True).compute(data, weights=w)`` seeds its EM from the weighted clustering; the default
    keeps the unweighted seeding."""
    import hgmm_amd
    from hgmm_amd.gmmreg_gpu.gmm import GMM_GPU
    C, cnt, _ = W.bunny_case()
    out = []
    with hgmm_amd.use_context(ctx):
        for kwargs in ({}, {"weighted_init": False}, {"weighted_init": True}):
            f = GMM_GPU(n_gmm_components=20, max_iter=5, **kwargs)
            f.init()
            out.append(f.compute(C, weights=cnt))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.isfinite(out[2][0]).all() and np.isfinite(out[2][1]).all()
    assert not np.array_equal(out[2][0], out[0][0])


# -- 9. refusals ---------------------------------------------------------------------------------------
def _weighted_calls(ctx, k, first, uniforms, init):
    return [("hgmm_kmeans_plusplus_weighted", lambda: ctx.kmeans_plusplus(k, first, uniforms, weighted=True)),
            ("hgmm_kmeans_step_weighted", lambda: ctx.kmeans_step(init, reset_labels=True, weighted=True)),
            ("hgmm_kmeans_lloyd_weighted", lambda: ctx.kmeans_lloyd(init, 5, 0.0, weighted=True))]


def test_refusals_leave_the_resident_state_alone():
    import hgmm_amd
    from hgmm_amd._native import HgmmError
    n, k = 3000, 65
    Xc, init = H.loop_case(n, k)
    ru = np.random.RandomState(5)
    first, uniforms = int(ru.randint(n)), ru.uniform(size=(k - 1, okm.n_local_trials(k)))
    c = hgmm_amd.Context(0)
    try:
        c.set_points(Xc)
        plain = _all_three(c, k, first, uniforms, init, False)
        # no weights resident
        for name, call in _weighted_calls(c, k, first, uniforms, init):
            with pytest.raises(HgmmError, match=name + ".*no source weights are resident"):
                call()
        _same_bits(_all_three(c, k, first, uniforms, init, False), plain, ALL_KEYS)
        # set_points dropped them
        c.tree_set_source_weights(W.count_weights(n, 3))
        c.kmeans_step(init, reset_labels=True, weighted=True)
        c.set_points(Xc)
        for name, call in _weighted_calls(c, k, first, uniforms, init):
            with pytest.raises(HgmmError, match=name + ".*no source weights are resident"):
                call()
        _same_bits(_all_three(c, k, first, uniforms, init, False), plain, ALL_KEYS)
        # a communicator of one rank
        c.tree_set_source_weights(W.count_weights(n, 3))
        c.comm_init_host(1, 0, "hgmm_km_weights_%d" % os.getpid())
        try:
            for name, call in _weighted_calls(c, k, first, uniforms, init):
                with pytest.raises(HgmmError, match=name + ".*communicator.*sharded weighted fits are not supported"):
                    call()
            from hgmm_amd.kmeans import KMeans
            with pytest.raises(ValueError, match="communicator"):
                KMeans(n_clusters=k, random_state=1, ctx=c).fit(Xc, sample_weight=W.count_weights(n, 3))
        finally:
            c.comm_destroy()
        _same_bits(_all_three(c, k, first, uniforms, init, False), plain, ALL_KEYS)
    finally:
        c.close()
