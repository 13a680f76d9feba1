"""GPU tests of the flat full-covariance fit under per-point weights (hgmm_fullcov_fit_weighted / hgmm_fullcov_estep_weighted):
all three kernel paths -- one-pass float64, float32 tile, two-pass -- against the weighted restatement of the oracle
(tests/_fullcov_weight_oracle.py, pinned to the committed oracle by tests/test_fullcov_weights_cpu.py) at the tolerances of the
corresponding unweighted tests in tests/test_fullcov_gpu.py; the identities (w == 1, w == 2, zero weights, reruns) bitwise;
the voxel route; what the weighted entries leave alone; their refusals."""
import functools
import os

import numpy as np
import pytest

from oracle import hgmm_tree
from _fullcov_weight_oracle import LD, SIG2, build_flat_fullcov_w, case, e_step_w, init_rows, label_gaps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cloud(bunny):
    return case(bunny)


_CLOUD = {}


@functools.lru_cache(maxsize=None)
def _oracle(N, J, ls, iters, weighted=True, shift=0.0):
    """the weighted restatement's fit of the first N points of THE cloud, computed once per case"""
    P, w = _CLOUD["P"][:N] + shift, _CLOUD["w"][:N]
    idx = init_rows(w, J)
    return idx, build_flat_fullcov_w(P, J, ls, LD, idx, SIG2, iters, w if weighted else None)


@pytest.fixture(autouse=True)
def _share_cloud(cloud):
    _CLOUD["P"], _CLOUD["w"] = cloud


def _resident(ctx, P, w):
    ctx.set_points(P)
    if w is not None:
        ctx.tree_set_source_weights(w)


def _fit(ctx, P, w, J, ls, iters, idx, ld=LD, weighted=True):
    _resident(ctx, P, w)
    return ctx.fullcov_fit(J, ls, ld, P[idx], SIG2, iters, weighted=weighted)


def _same_bits(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _assert_f64(got, ref):
    """the float64 tolerances of tests/test_fullcov_gpu.py (test_fullcov_vs_oracle)"""
    pi, mu, cov, labels, q = got
    o_pi, o_mu, o_cov, o_q, o_cur = ref
    assert len(q) == len(o_q)
    np.testing.assert_allclose(q, o_q, rtol=1e-9, atol=1e-6)
    assert np.array_equal(labels, o_cur)
    np.testing.assert_allclose(pi, o_pi, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(mu, o_mu, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(cov, o_cov, rtol=1e-6, atol=1e-14)


# ---- float64 one-pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J", [(1300, 8), (1300, 40), (1300, 520), (1300, 1024), (777, 17), (15, 4), (1, 3)])
def test_weighted_fit_vs_oracle(ctx, cloud, N, J):
    """N not a multiple of 16 or 64, one and two components per lane, a tail block, fewer points than a tile"""
    P, w = cloud[0][:N], cloud[1][:N]
    iters = 6 if (N, J) == (1300, 40) else 3
    idx, ref = _oracle(N, J, 1e-30, iters)
    _assert_f64(_fit(ctx, P, w, J, 1e-30, iters, idx), ref)


def test_stop_rule_sees_the_weights(ctx, cloud):
    """J = 24, ls = 20, budget 40: the weighted oracle stops after 21 iterations and the unweighted after 17 -- a fit that
    ignores the weights cannot pass.  The oracle's own stop decisions are at least 0.05 ls from going the other way."""
    P, w = cloud
    idx, ref = _oracle(1300, 24, 20.0, 40)
    _, unweighted = _oracle(1300, 24, 20.0, 40, weighted=False)
    margin = hgmm_tree.stop_margins(ref[3], [len(ref[3])], 20.0).min()
    print("oracle: %d iterations weighted, %d unweighted, smallest stop margin %.3g" % (len(ref[3]), len(unweighted[3]), margin))
    assert margin >= 0.05 and len(ref[3]) != len(unweighted[3])
    got = _fit(ctx, P, w, 24, 20.0, 40, idx)
    assert len(got[4]) == len(ref[3])
    _assert_f64(got, ref)
    # the host stop rule (two-pass loop) decides the same
    with ctx.config(fullcov_two_pass=1):
        two = _fit(ctx, P, w, 24, 20.0, 40, idx)
    assert len(two[4]) == len(ref[3])
    _assert_f64(two, ref)


def test_two_pass_path(ctx, cloud):
    """full_pass_kernel + full_moments_kernel under the weights: the J = 40 case forced onto them, and J = 1040 (> 1024)"""
    P, w = cloud
    idx, ref = _oracle(1300, 40, 1e-30, 6)
    with ctx.config(fullcov_two_pass=1):
        got = _fit(ctx, P, w, 40, 1e-30, 6, idx)
    _assert_f64(got, ref)
    idx, ref = _oracle(1300, 1040, 1e-30, 2)
    _assert_f64(_fit(ctx, P, w, 1040, 1e-30, 2, idx), ref)


def test_symmetric_form_fallback(ctx, cloud):
    P, w = cloud
    idx, ref = _oracle(1300, 40, 1e-30, 6)
    with ctx.config(tree_no_chol=1):
        got = _fit(ctx, P, w, 40, 1e-30, 6, idx)
    _assert_f64(got, ref)


# ---- identities, bitwise -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["float64", "float32", "two_pass"])
def test_unit_weights_are_the_unweighted_entry_bit_for_bit(ctx, cloud, path):
    P, _ = cloud
    J = 40
    idx = np.random.RandomState(J).choice(len(P), J, replace=False)
    ctx.tree_set_precision(np.float32 if path == "float32" else np.float64)
    try:
        with ctx.config(fullcov_two_pass=1 if path == "two_pass" else 0):
            a = _fit(ctx, P, None, J, 1.0, 6, idx, weighted=False)
            b = _fit(ctx, P, np.ones(len(P)), J, 1.0, 6, idx)
            e_a = ctx.fullcov_estep(a[0], a[1], a[2])
            e_b = ctx.fullcov_estep(a[0], a[1], a[2], weighted=True)
    finally:
        ctx.tree_set_precision(np.float64)
    assert _same_bits(a, b) and _same_bits(e_a, e_b)


def test_weight_two_scales_exactly(ctx, cloud):
    """w == 2 with ls and ld doubled: tables, labels and iteration count bitwise, exactly twice the q trace; the E-step
    entry returns exactly twice the unweighted moments"""
    P, _ = cloud
    J = 40
    idx = np.random.RandomState(J).choice(len(P), J, replace=False)
    a = _fit(ctx, P, None, J, 20.0, 30, idx, weighted=False)
    b = _fit(ctx, P, np.full(len(P), 2.0), J, 40.0, 30, idx, ld=2 * LD)
    print("iterations", len(a[4]), len(b[4]))
    assert 1 < len(a[4]) < 30 and len(a[4]) == len(b[4])                 # (the stop rule decided)
    assert _same_bits(a[:4], b[:4]) and np.array_equal(2.0 * a[4], b[4])
    e_b = ctx.fullcov_estep(a[0], a[1], a[2], weighted=True)
    e_a = ctx.fullcov_estep(a[0], a[1], a[2])
    for u, v in zip(e_a[:3], e_b[:3]):
        assert np.array_equal(2.0 * u, v)
    assert np.array_equal(e_a[3], e_b[3]) and 2.0 * e_a[4] == e_b[4]


def test_two_weighted_calls_return_the_same_bits(ctx, cloud):
    P, w = cloud
    idx = init_rows(w, 40)
    assert _same_bits(_fit(ctx, P, w, 40, 1e-30, 6, idx), _fit(ctx, P, w, 40, 1e-30, 6, idx))


def test_zero_weight_is_absence(ctx, cloud):
    """the fit of (P, w) against the fit of the rows with w > 0: the same parameters, and the same labels on the kept rows
    (the partials group other points, so not bitwise: q rtol 1e-12, tables rtol 1e-9)"""
    P, w = cloud
    keep = w > 0
    idx = init_rows(w, 40)
    a = _fit(ctx, P, w, 40, 1e-30, 4, idx)
    _resident(ctx, P[keep], w[keep])
    b = ctx.fullcov_fit(40, 1e-30, LD, P[idx], SIG2, 4, weighted=True)
    assert len(a[3]) == len(P) and a[3].min() >= 0 and a[3].max() < 40   # a zero-weight point is still labelled
    assert np.array_equal(a[3][keep], b[3])
    np.testing.assert_allclose(a[4], b[4], rtol=1e-12, atol=0)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_allclose(u, v, rtol=1e-9, atol=0)


def test_fit_is_the_one_level_tree_build_on_the_device(ctx, cloud):
    """J = 8: tree_build(L = 1) under the source weights, then the weighted fit on the same context (src_w is still in
    level-0 order after a build)"""
    P, w = cloud
    idx = init_rows(w, 8)
    _resident(ctx, P, w)
    t_pi, t_mu, t_cov, leaf, iters, t_q = ctx.tree_build(1, 1.0, LD, P[idx], SIG2, 6)
    pi, mu, cov, labels, q = ctx.fullcov_fit(8, 1.0, LD, P[idx], SIG2, 6, weighted=True)
    assert list(iters) == [len(q)]
    assert np.array_equal(labels, leaf)
    np.testing.assert_allclose(q, t_q, rtol=1e-9, atol=0)
    for u, v in ((pi, t_pi), (mu, t_mu), (cov, t_cov)):
        np.testing.assert_allclose(u, v, rtol=1e-9, atol=0)


def test_estep_entry(ctx, cloud):
    """m0 / m1 / m2 / q of given parameters, with the asymmetric covariance of test_fullcov_estep_moments_layout"""
    P, w = cloud
    J = 24
    idx = np.random.RandomState(1).choice(len(P), J, replace=False)
    pi = np.full(J, 1.0 / J)
    mu = P[idx].copy()
    cov = np.tile(np.identity(3) * 0.0004, (J, 1, 1))
    cov[:, 0, 1] = cov[:, 1, 0] = 0.0001
    _resident(ctx, P, w)
    m0, m1, m2, labels, q = ctx.fullcov_estep(pi, mu, cov, weighted=True)
    o0, o1, o2, o_cur, o_q = e_step_w(P, pi, mu, cov, w)
    np.testing.assert_allclose(m0, o0, rtol=1e-10)
    np.testing.assert_allclose(m1, o1, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(m2, o2, rtol=1e-10, atol=1e-15)
    assert np.array_equal(labels, o_cur)
    np.testing.assert_allclose(q, o_q, rtol=1e-10)
    assert abs(m0.sum() - hgmm_tree.weight_sum(w)) < 1e-9 * w.sum()
    # ... and through the two kernels of the two-pass path
    with ctx.config(fullcov_two_pass=1):
        t0, t1, t2, t_lab, t_q = ctx.fullcov_estep(pi, mu, cov, weighted=True)
    np.testing.assert_allclose(t0, o0, rtol=1e-10)
    np.testing.assert_allclose(t1, o1, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(t2, o2, rtol=1e-10, atol=1e-15)
    assert np.array_equal(t_lab, o_cur)
    np.testing.assert_allclose(t_q, o_q, rtol=1e-10)


# ---- float32 tile --------------------------------------------------------------------------------------------------------
def _cov_err(cov, ref):
    """largest |d Sigma_ab| over a component's mean variance (tests/test_fullcov_gpu.py)"""
    scale = np.abs(np.einsum("jii->j", ref)) / 3.0
    return float(np.max(np.abs(cov - ref).reshape(len(ref), -1).max(1) / np.maximum(scale, 1e-300)))


@pytest.mark.parametrize("N,J,shift", [(1300, 17, 0.0), (1300, 17, 50.0), (1300, 540, 0.0), (15, 4, 0.0)])
def test_weighted_float32_tile_vs_oracle(ctx, cloud, N, J, shift):
    """the unweighted float32 tests' bounds: at most max(2, N // 2000) labels off, q rtol 1e-5 / atol 1e-2, pi rtol 1e-3,
    mu atol 1e-5, covariances to 1e-3 of a variance on live components.  The label allowance presumes that the float64
    oracle has no more near-ties than that among these rows: counted here first, on the parameters the labels come from."""
    P, w = cloud[0][:N] + shift, cloud[1][:N]
    iters = 3
    idx, ref = _oracle(N, J, 1e-30, iters, True, shift)
    o_pi, o_mu, o_cov, o_q, o_cur = ref
    allowed = max(2, N // 2000)
    before = _oracle(N, J, 1e-30, iters - 1, True, shift)[1]            # the parameters of the E-step that labelled
    near = int((label_gaps(P, *before[:3]) < 1e-5).sum())
    print("N=%d J=%d shift=%g: %d rows of the oracle within 1e-5 of a label tie" % (N, J, shift, near))
    assert near <= allowed
    _resident(ctx, P, w)
    ctx.tree_set_precision(np.float32)
    try:
        pi, mu, cov, labels, q = ctx.fullcov_fit(J, 1e-30, LD, P[idx], SIG2, iters, weighted=True)
    finally:
        ctx.tree_set_precision(np.float64)
    print("   labels off %d, |dq| %.3g, |d mu| %.3g" % ((labels != o_cur).sum(), np.abs(q - o_q).max(), np.abs(mu - o_mu).max()))
    assert len(q) == len(o_q)
    assert (labels != o_cur).sum() <= allowed
    np.testing.assert_allclose(q, o_q, rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(pi, o_pi, rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(mu, o_mu, rtol=0, atol=1e-5)
    live = o_pi > 1e-6
    if live.any():
        assert _cov_err(cov[live], o_cov[live]) < 1e-3
    else:
        # (15 points under 4 components of sig2 = 0.0005: every component dies in the oracle -- the dead-component rule)
        assert (N, J) == (15, 4) and np.array_equal(pi, o_pi) and np.array_equal(cov, o_cov)


# ---- the voxel route and the mirror -----------------------------------------------------------------------------------------
def test_voxel_route_is_the_host_route_bit_for_bit(ctx, bunny):
    """voxel_down_sample(bun000, 4 mm, download=False) -> fitFullCovGMM(vc, 16): the fit of the centroids under their counts
    without a host trip, against the same fit from host arrays"""
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints, fitFullCovGMM
    vc = ctx.voxel_down_sample(bunny.astype(np.float64), 0.004, download=False)
    cent, cnt = vc.get()
    assert cnt.sum() == len(bunny) and len(cent) == len(vc)
    idx = np.random.RandomState(16).choice(len(vc), 16, replace=False)
    a = fitFullCovGMM(vc, 16, ls=1e-30, init_idx=idx, max_iters=5, ctx=ctx, return_trace=True)
    b = fitFullCovGMM(WeightedPoints(cent, cnt), 16, ls=1e-30, init_idx=idx, max_iters=5, ctx=ctx, return_trace=True)
    c = fitFullCovGMM(cent, 16, ls=1e-30, init_idx=idx, max_iters=5, ctx=ctx, return_trace=True)
    assert _same_bits(a[:3], b[:3]) and np.array_equal(a[3]["labels"], b[3]["labels"]) and np.array_equal(a[3]["q_trace"], b[3]["q_trace"])
    assert not np.array_equal(a[0], c[0])                              # the counts count
    # ... and they are the restatement's weights
    o = build_flat_fullcov_w(cent, 16, 1e-30, 1e-4, idx, 0.00034, 5, cnt.astype(np.float64))
    np.testing.assert_allclose(a[3]["q_trace"], o[3], rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(a[0], o[0], rtol=1e-9, atol=1e-13)


# ---- what the weighted entries leave alone ---------------------------------------------------------------------------------
def test_unweighted_entry_ignores_resident_weights(ctx, cloud):
    P, w = cloud
    idx = init_rows(w, 40)
    a = _fit(ctx, P, None, 40, 1e-30, 4, idx, weighted=False)
    b = _fit(ctx, P, w, 40, 1e-30, 4, idx, weighted=False)
    e_b = ctx.fullcov_estep(a[0], a[1], a[2])
    ctx.set_points(P)
    e_a = ctx.fullcov_estep(a[0], a[1], a[2])
    assert _same_bits(a, b) and _same_bits(e_a, e_b)


def test_weighted_fit_leaves_the_weighted_tree_build_alone(ctx, cloud):
    P, w = cloud
    T = hgmm_tree.n_total(2)
    tdx = init_rows(w, T, seed=72)
    _resident(ctx, P, w)
    a = ctx.tree_build(2, 20.0, LD, P[tdx], 0.004, 30)
    _resident(ctx, P, w)
    ctx.fullcov_fit(40, 1e-30, LD, P[init_rows(w, 40)], SIG2, 3, weighted=True)
    b = ctx.tree_build(2, 20.0, LD, P[tdx], 0.004, 30)
    assert _same_bits(a, b)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(ctx, cloud):
    import hgmm_amd
    P, w = cloud
    J = 24
    idx = init_rows(w, J)
    ref = _fit(ctx, P, None, J, 1e-30, 3, idx, weighted=False)
    pi, mu, cov = ref[:3]

    def refused(match):
        with pytest.raises(hgmm_amd.HgmmError, match=match):
            ctx.fullcov_fit(J, 1e-30, LD, P[idx], SIG2, 3, weighted=True)
        with pytest.raises(hgmm_amd.HgmmError, match=match):
            ctx.fullcov_estep(pi, mu, cov, weighted=True)
        assert _same_bits(ctx.fullcov_fit(J, 1e-30, LD, P[idx], SIG2, 3), ref)      # the unweighted fit still gives its bits

    ctx.set_points(P)
    refused("no source weights")                                        # none resident
    _resident(ctx, P, w)
    ctx.set_points(P)
    refused("no source weights")                                        # dropped by a new cloud
    ctx.set_points_batch([P[:600], P[600:]], weights=[w[:600], w[600:]])
    refused("no source weights")                                        # a forest cloud's weights are not these
    # under a communicator (host backend, world of one): sharded weighted fits are not supported
    _resident(ctx, P, w)
    ctx.comm_init_host(1, 0, "hgmm_fullcov_w1_%d" % os.getpid())
    try:
        refused("communicator")
    finally:
        ctx.comm_destroy()
    # the weights are still resident, and in force again without the communicator
    got = ctx.fullcov_fit(J, 1e-30, LD, P[idx], SIG2, 3, weighted=True)
    _assert_f64(got, _oracle(1300, J, 1e-30, 3)[1])
    # every argument error of the unweighted entry
    with pytest.raises(hgmm_amd.HgmmError, match="outside 1..4096"):
        ctx.fullcov_fit(5000, 1e-30, LD, np.zeros((5000, 3)), SIG2, 3, weighted=True)
