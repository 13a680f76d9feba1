"""Per-point weights for the KMeans initialiser, on the host: the weighted restatement
(tests/_kmeans_weight_oracle.py) is pinned to live scikit-learn, every input of tests/test_kmeans_weights_gpu.py is
shown to be a fair one on the restatement alone, and the host-side refusals of the public layers are held without a
device."""
import numpy as np
import pytest

import _kmeans_helpers as H
import _kmeans_weight_oracle as W
from oracle import kmeans as okm


# -- 1. the restatement against live scikit-learn ---------------------------------------------------------
def _cloud(n, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(n, 3) * [1.0, 2.0, 0.5] + [3.0, -1.0, 0.25]


def _weights(kind, n, seed):
    rs = np.random.RandomState(seed + 1)
    if kind == "counts":
        return rs.randint(1, 40, n).astype(np.float64)
    if kind == "real":
        return rs.rand(n) * 3.0 + 0.01
    if kind == "zeros":
        w = rs.randint(1, 40, n).astype(np.float64)
        w[rs.rand(n) < 0.3] = 0.0
        return w
    if kind == "counts_1e6":
        return rs.randint(1, 40, n).astype(np.float64) * 1e6
    raise KeyError(kind)


@pytest.mark.parametrize("n,k", [(3000, 65), (1500, 200)])
@pytest.mark.parametrize("kind", ["counts", "real", "zeros", "counts_1e6"])
def test_oracle_matches_live_sklearn(kind, n, k):
    """Seeds, labels and n_iter identical, centres to 1e-12, inertia to rtol 1e-12 -- and the unweighted clustering of
    the same cloud picks other seeds, so the weights are not a no-op here."""
    cluster = pytest.importorskip("sklearn.cluster")
    X, w = _cloud(n, 11 * n + k), _weights(kind, n, n + k)
    ref = cluster.KMeans(n_clusters=k, random_state=1, max_iter=50, n_init=1, tol=1e-4).fit(X, sample_weight=w)
    got = W.fit_w(X, w, k, random_state=1, max_iter=50, tol=1e-4)
    print("label margin", min(got["walk"].margin), "seed margins", min(got["seed_trace"].thr_margin),
          min(got["seed_trace"].pot_gap))
    W.assert_fair_w(got["walk"])
    # (scikit-learn keeps no seed indices: the seeds are compared through a fit that stops after one iteration)
    np.testing.assert_array_equal(got["labels_"], ref.labels_)
    assert got["n_iter_"] == ref.n_iter_
    np.testing.assert_allclose(got["cluster_centers_"], ref.cluster_centers_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["inertia_"], ref.inertia_, rtol=1e-12)
    seeds_ref = cluster.kmeans_plusplus(X - X.mean(axis=0), k, sample_weight=w,
                                        random_state=np.random.RandomState(1))[1]
    np.testing.assert_array_equal(got["init_indices"], seeds_ref)
    assert not np.array_equal(got["init_indices"], okm.fit(X, k, random_state=1, max_iter=1)["init_indices"])


def test_relocation_matches_live_sklearn():
    """``reloc8_case`` with strictly positive count weights: three clusters are empty in iteration 1."""
    cluster = pytest.importorskip("sklearn.cluster")
    X, init = H.reloc8_case()
    w = W.reloc8_weights()
    assert (w > 0).all()
    got = W.fit_w(X, w, len(init), max_iter=50, tol=1e-4, init=init)
    assert got["walk"].n_empty[0] == 3
    ref = cluster.KMeans(n_clusters=len(init), init=init, max_iter=50, n_init=1, tol=1e-4).fit(X, sample_weight=w)
    np.testing.assert_array_equal(got["labels_"], ref.labels_)
    assert got["n_iter_"] == ref.n_iter_
    np.testing.assert_allclose(got["cluster_centers_"], ref.cluster_centers_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["inertia_"], ref.inertia_, rtol=1e-12)


def test_zero_weight_relocation_matches_live_sklearn():
    """The same cloud with 30 % zero weights: the farthest point of iteration 1 has weight 0, so a relocated cluster
    stays at weight 0 and takes the heaviest cluster's row (statement 5 of the restatement)."""
    cluster = pytest.importorskip("sklearn.cluster")
    X, init = H.reloc8_case()
    w = W.reloc8_weights(True)
    got = W.fit_w(X, w, len(init), max_iter=50, tol=1e-4, init=init)
    wk = got["walk"]
    assert wk.n_empty[0] == 3
    lab0 = wk.labels[0]
    far = np.argmax((((X - X.mean(axis=0)) - wk.centres_in[0][lab0]) ** 2).sum(axis=1))
    assert w[far] == 0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = cluster.KMeans(n_clusters=len(init), init=init, max_iter=50, n_init=1, tol=1e-4).fit(X, sample_weight=w)
    assert got["n_iter_"] == ref.n_iter_
    np.testing.assert_array_equal(got["labels_"], ref.labels_)
    np.testing.assert_allclose(got["cluster_centers_"], ref.cluster_centers_, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["inertia_"], ref.inertia_, rtol=1e-12)


# -- 2. fairness of every GPU input ---------------------------------------------------------------------
@pytest.mark.parametrize("n,k", W.SEED_CASES)
def test_seed_cases_are_fair(n, k):
    """Every seeding decision (threshold against the running sum, best against second-best candidate) has a margin of
    1e-10 of the potential, all k seeds are distinct, and the step from the seeds has MARGIN_MIN at every point."""
    Xc, w, first, uniforms = W.seed_case(n, k)
    centres, ids, trace, lab, mind2, margin = W.seed_expect(n, k)
    assert w[first] > 0
    assert len(set(ids.tolist())) == k
    assert (w[ids] > 0).all()                       # the threshold search never lands on a zero weight
    if n >= 255:
        assert (w == 0).any()
    if k > 1:
        print("(%d, %d): threshold margin %.3g, potential gap %.3g, label margin %.3g"
              % (n, k, min(trace.thr_margin), min(trace.pot_gap), margin))
        assert min(trace.thr_margin) >= W.SEED_MARGIN_MIN
        assert min(trace.pot_gap) >= W.SEED_MARGIN_MIN
        assert margin >= H.MARGIN_MIN


@pytest.mark.parametrize("n,k", W.LATTICE_W_CASES)
def test_lattice_cases_have_ties_and_every_weight(n, k):
    X, A, _, _ = H.lattice_case(n, k)
    w = W.lattice_weights(n, k)
    assert H.has_tie(X, A).any()
    assert set(np.unique(w).tolist()) == {0.0, 1.0, 2.0, 4.0}


@pytest.mark.parametrize("n,k", H.LOOP_CASES)
def test_loop_cases_are_fair(n, k):
    wk = W.loop_walk_w(n, k)
    W.assert_fair_w(wk)
    assert wk.strict and 2 < wk.n_iter < 60


def test_stop_rule_inputs_are_fair():
    """The weighted 'uniform' trajectory: long enough for every budget, fair at every iteration, and with one tolerance
    stop inside the first batch of 8 and one in a later batch."""
    wk = W.golden_walk_w("uniform")
    W.assert_fair_w(wk)
    assert wk.n_iter > max(H.BUDGETS), wk.n_iter
    inside, across = W.tol_stops_w("uniform")
    assert 2 <= inside < 8 < across
    for m in (inside, across):
        t = W.tol_for_stop_w("uniform", m)
        stopped = W.golden_walk_w("uniform", 50, t)
        assert stopped.n_iter == m and not stopped.strict
        assert wk.shift[m - 1] < t < min(wk.shift[:m - 1])


def test_relocation_inputs():
    """``reloc8_case`` under positive count weights relocates in iteration 1 with a clear order of the farthest points;
    which LATE_EMPTY clouds still meet an empty cluster under count weights is printed -- the GPU file uses the first."""
    X, init = H.reloc8_case()
    Xc, start, tol_abs = H.fit_inputs(X, init)
    wk = W.lloyd_w(Xc, W.reloc8_weights(), start, 50, tol_abs)
    assert wk.n_empty[0] == 3
    assert min(wk.margin[1:]) >= H.MARGIN_MIN
    late = []
    for n, k, blobs, spread, seed, _ in H.LATE_EMPTY_CASES:
        Xl, il = H.late_empty_case(n, k, blobs, spread, seed)
        wl = W.lloyd_w(Xl, W.count_weights(n, seed), il, 50, 0.0)
        late.append((n, k, seed, H.first_empty(wl)))
    print("weighted LATE_EMPTY trajectories (n, k, seed, first empty iteration):", late)
    pick = W.late_empty_pick()
    assert pick is not None, "no LATE_EMPTY cloud meets an empty cluster under count weights: drop the GPU case"
    n, k, blobs, spread, seed, hit = pick
    Xl, il = H.late_empty_case(n, k, blobs, spread, seed)
    wl = W.lloyd_w(Xl, W.count_weights(n, seed), il, 50, 0.0)
    assert hit == H.first_empty(wl) and hit > 1
    W.assert_fair_w(wl, allow_empty=True)
    assert H.relocation_gap(Xl, wl) >= H.MARGIN_MIN


def test_many_groups_case_is_fair():
    """n = 4.3 M: two summation orders differ by at most n * 2^-53 ~ 4.8e-10 of the potential; every decision keeps ten
    times that."""
    assert (W.MANY_N + 4095) // 4096 > 1024
    *_, ids, trace = W.many_groups_case()
    print("many groups: threshold margin %.3g, potential gap %.3g" % (min(trace.thr_margin), min(trace.pot_gap)))
    assert len(set(ids.tolist())) == W.MANY_K
    assert min(trace.thr_margin) >= W.MANY_MARGIN_MIN and min(trace.pot_gap) >= W.MANY_MARGIN_MIN


def test_bunny_case_is_fair():
    C, cnt, fit = W.bunny_case()
    assert 1500 < len(C) < 3000 and cnt.sum() == 40256 and cnt.max() > 1
    W.assert_fair_w(fit["walk"])
    print("bunny: %d centroids, label margin %.3g, seed margins %.3g / %.3g"
          % (len(C), min(fit["walk"].margin), min(fit["seed_trace"].thr_margin), min(fit["seed_trace"].pot_gap)))
    assert min(fit["seed_trace"].thr_margin) >= W.SEED_MARGIN_MIN and min(fit["seed_trace"].pot_gap) >= W.SEED_MARGIN_MIN
    assert len(set(fit["init_indices"].tolist())) == W.BUNNY_K


# -- 3. invariants on the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(3000, 65), (1500, 200)])
def test_unit_weights_reproduce_the_unweighted_oracle(n, k):
    X = _cloud(n, n + k)
    a = okm.fit(X, k, random_state=1, max_iter=50)
    b = W.fit_w(X, np.ones(n), k, random_state=1, max_iter=50)
    np.testing.assert_array_equal(a["init_indices"], b["init_indices"])
    np.testing.assert_array_equal(a["labels_"], b["labels_"])
    assert a["n_iter_"] == b["n_iter_"]
    np.testing.assert_array_equal(a["cluster_centers_"], b["cluster_centers_"])
    assert a["inertia_"] == b["inertia_"]


def test_integer_weights_are_repetition():
    """An explicit start, tol = 0: the weighted fit of (X, c) and the unweighted fit of X with row i repeated c_i times
    agree in n_iter and, to 1e-12, in centres (they differ by the order of summation alone)."""
    n, k = 1200, 40
    X = _cloud(n, 5)
    c = np.random.RandomState(6).randint(0, 5, n)
    Xc = X - X.mean(axis=0)
    init = Xc[np.random.RandomState(7).choice(np.flatnonzero(c > 0), k, replace=False)]
    a = W.lloyd_w(Xc, c.astype(np.float64), init, 60, 0.0)
    rep = np.repeat(Xc, c, axis=0)
    lab, inertia, centres, n_iter = okm.lloyd(rep, init, 60, 0.0)
    W.assert_fair_w(a)
    assert a.n_iter == n_iter
    np.testing.assert_allclose(a.centres, centres, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.inertia, inertia, rtol=1e-12)
    np.testing.assert_array_equal(np.repeat(a.final_labels, c), lab)


# -- 4. host logic without a device ---------------------------------------------------------------------
def _kmeans_module():
    try:
        from hgmm_amd import kmeans
        from hgmm_amd._native import load_library
        load_library()
    except (ImportError, OSError) as e:
        pytest.skip("library not built: %s" % e)
    return kmeans


@pytest.mark.parametrize("bad,what", [(np.ones(9), "length"), (np.r_[-1.0, np.ones(9)], "negative"),
                                      (np.r_[np.nan, np.ones(9)], "nan"), (np.r_[np.inf, np.ones(9)], "infinite"),
                                      (np.zeros(10), "all zero")])
def test_fit_refuses_bad_weights(bad, what):
    km = _kmeans_module()
    X = np.random.RandomState(0).rand(10, 3)
    with pytest.raises(ValueError):
        km.KMeans(n_clusters=2, random_state=1).fit(X, sample_weight=bad)


def test_own_on_a_plain_array_is_refused():
    km = _kmeans_module()
    with pytest.raises(ValueError, match="own"):
        km.KMeans(n_clusters=2, random_state=1).fit(np.random.RandomState(0).rand(10, 3), sample_weight="own")


def test_weighted_init_without_weights_is_refused():
    """(The opt-in is an option of the estimator: ``fit`` and ``compute`` keep the argument lists
    tests/test_flat_weights_cpu.py holds them to.)"""
    _kmeans_module()
    from hgmm_amd.gmmreg_gpu.gmm import GMM_GPU, GMM_GPU_Base
    X = np.random.RandomState(0).rand(50, 3)
    with pytest.raises(ValueError, match="weighted_init"):
        GMM_GPU_Base(4, weighted_init=True).fit(X)
    f = GMM_GPU(n_gmm_components=4, weighted_init=True)
    f.init()
    with pytest.raises(ValueError, match="weighted_init"):
        f.compute(X)
    assert GMM_GPU_Base(4).weighted_init is False and GMM_GPU().weighted_init is False
