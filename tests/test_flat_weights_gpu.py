"""Per-point weights of the flat (diag / spherical) GMM fit (hgmm_flat_set_weights) on the GPU.

Point i counts as s_i >= 0 points: the M-step sums take s_i resp_ij, the mixing weights are nk / S (S = sum s), the
log-likelihood behind the stop rule is sum s_i lpn_i / S, hgmm_flat_stats returns the weighted sums and S.  The yard-stick
is the float64 restatement tests/_flat_weight_oracle.py (oracle.flat_em with those three statements changed), and the
bounds are the ones tests/test_flat_gpu.py holds the UNWEIGHTED calls to on the same kind of cloud -- weights act
relatively, no wider bound is needed: test_ragged_sizes (statistics, mean), test_every_lane_layout (M-step from a
materialised matrix, two iterations of training), test_train_small (training on the golden cloud),
test_large_component_counts_chunked_path (J > 1024).  Every case prints its largest differences before it asserts.

Standard weights: uniform in [0.25, 4), one in ten exactly zero (those of tests/test_tree_source_weights_gpu.py).
"""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

import _flat_weight_oracle as fw
from conftest import load_golden
from oracle import flat_em

pytestmark = pytest.mark.gpu

HGMM_ERR_ARG, HGMM_ERR_STATE = -2, -3
FLAVOURS = [("W", "diag"), ("W", "spherical"), ("G", "diag")]
SHAPES = [(1, 1), (63, 5), (65, 37), (1000, 64), (777, 257), (300, 1023), (500, 1024)]
CHUNKED = [(3000, 1025), (1500, 4096)]
f64 = lambda a: np.asarray(a, dtype=np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def weights_for(n, seed=11):
    s = fw.standard_weights(n, seed)
    if not s.any():
        s[0] = 1.0                                   # (n = 1: the one row must count)
    return s


def ragged(N, J):
    """test_ragged_sizes' cloud and model (J <= 1024), test_large_component_counts_chunked_path's (J > 1024)"""
    rs = np.random.RandomState(N * 1000 + J if J <= 1024 else J)
    X = rs.rand(N, 3).astype(np.float32)
    mu = rs.rand(J, 3).astype(np.float32)
    inv = (1.0 / np.sqrt((0.01 + 0.1 * rs.rand(J, 3)) if J <= 1024 else (0.003 + 0.02 * rs.rand(J, 3)))).astype(np.float32)
    w = rs.rand(J).astype(np.float32) + 0.01
    w /= w.sum()
    return X, mu, inv, w, weights_for(N)


def golden_small(variant, cov_type):
    g = load_golden("flat_small_%s_%s.npz" % (variant, cov_type))
    return g["X"], g["mu0"], g["cov0"], g["w0"]


def dmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max())


def check_stats(ctx, X, s, inv, mu, w, chunked, label):
    stats, sum_lpn, n = ctx.flat_stats(inv, mu, w, "diag", "W")
    o_stats, o_sum, o_S = fw.stats(f64(X), s, f64(inv), f64(mu), f64(w), "diag", "W")
    print("%s stats: S %.17g vs %.17g, sum_lpn %.10g vs %.10g, max |d s0| %.3g, |d a| %.3g, |d b| %.3g"
          % (label, n, fw.weight_sum(s), sum_lpn, o_sum, dmax(stats[:, 0], o_stats[:, 0]), dmax(stats[:, 1:4], o_stats[:, 1:4]),
             dmax(stats[:, 4:7], o_stats[:, 4:7])))
    assert n == fw.weight_sum(s)
    np.testing.assert_allclose(sum_lpn, o_sum, rtol=1e-5, atol=1e-4)
    if chunked:
        np.testing.assert_allclose(stats[:, 0], o_stats[:, 0], rtol=1e-4, atol=1e-6)
    else:
        np.testing.assert_allclose(stats[:, 0], o_stats[:, 0], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(stats[:, 1:4], o_stats[:, 1:4], rtol=1e-3, atol=2e-5)
        np.testing.assert_allclose(stats[:, 4:7], o_stats[:, 4:7], rtol=1e-3, atol=2e-5)
    return stats, sum_lpn, n


def check_mean(ctx, X, s, inv, mu, w, label):
    """the mean of all three E-step entries (host, asynchronous, device parameters), with and without a caller's lpn array"""
    o_mean, _, o_lpn = fw.e_step(f64(X), s, f64(inv), f64(mu), f64(w), "diag", "W")
    got = []
    for kw in (dict(), dict(want_lpn=True), dict(lazy_mean=True), dict(want_log_resp=False), dict(want_lpn=True, want_argmax=True)):
        mean, lr, lpn, _ = ctx.flat_estep(inv, mu, w, "diag", "W", **kw)
        got.append(float(mean))
        if lpn is not None:                                   # the per-point normaliser does not see the weights
            live = s > 0
            assert np.abs(lpn.get()[live] - o_lpn[live]).max() <= 2e-5 * max(1.0, np.abs(o_lpn[live]).max())
    d_mean, *_ = ctx.flat_estep(ctx.to_device(inv), ctx.to_device(mu), ctx.to_device(w), "diag", "W", want_log_resp=False)
    got.append(float(d_mean))
    print("%s mean: %s vs %.10g" % (label, ["%.10g" % v for v in got], o_mean))
    for v in got:
        assert abs(v - o_mean) <= 1e-5 * max(1.0, abs(o_mean))
    # (the same kernel, the same rows per wave, the workgroups' sums added by the host: the same bits whether the rows' lpn
    #  go to the caller's array or to the context's)
    assert got[0] == got[1]
    return got[0], lr


def check_mstep(ctx, X, s, lr, mu, label):
    """host and device results, log and plain responsibilities (test_every_lane_layout's bounds)"""
    o_w, o_mu, o_cov = fw.m_step(f64(X), s, np.exp(f64(lr)), "diag", "W")
    live = o_w > 1e-6
    lr_dev = ctx.to_device(lr)
    outs = {"log, host": ctx.flat_mstep(lr_dev.exp(), "diag", "W", centre_hint=mu),
            "plain, host": ctx.flat_mstep(np.exp(lr), "diag", "W", centre_hint=mu),
            "log, device": tuple(a.get() for a in ctx.flat_mstep(lr_dev.exp(), "diag", "W", centre_hint=mu, device_out=True)),
            "plain, device": tuple(a.get() for a in ctx.flat_mstep(ctx.to_device(np.exp(lr)), "diag", "W", centre_hint=mu,
                                                                     device_out=True))}
    for name, (w_m, mu_m, cov_m) in outs.items():
        print("%s m_step (%s): max |dw| %.3g rel %.3g, |dmu| %.3g, rel dcov %.3g"
              % (label, name, dmax(w_m, o_w), float(np.abs(w_m / o_w - 1).max()), dmax(mu_m[live], o_mu[live]),
                 float(np.abs(cov_m[live] / o_cov[live] - 1).max())))
        np.testing.assert_allclose(w_m, o_w, rtol=1e-4, atol=1e-8)
        np.testing.assert_allclose(mu_m[live], o_mu[live], rtol=0, atol=1e-5)
        np.testing.assert_allclose(cov_m[live], o_cov[live], rtol=1e-3, atol=1e-8)
    assert all(same_bits(a, b) for a, b in zip(outs["log, host"], outs["log, device"]))
    assert all(same_bits(a, b) for a, b in zip(outs["plain, host"], outs["plain, device"]))
    return outs["log, host"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the restatement: statistics, M-step, E-step mean, two iterations of training, every shape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J", SHAPES)
def test_ragged_sizes_against_the_restatement(ctx, N, J):
    X, mu, inv, w, s = ragged(N, J)
    label = "weighted %dx%d" % (N, J)
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    check_stats(ctx, X, s, inv, mu, w, False, label)
    _, lr = check_mean(ctx, X, s, inv, mu, w, label)
    check_mstep(ctx, X, s, lr.get(), mu, label)
    # two iterations of training (test_every_lane_layout's run and bounds)
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    inv_t, mu_t, w_t, cov_t, lls, _ = ctx.flat_train(2, 0.0, mu, cov0, w0, "diag", "W")
    o = fw.train(f64(X), s, 2, 0.0, f64(mu), f64(cov0), f64(w0), "diag", "W")
    print("%s train: max |dlls| %.3g, |dmu| %.3g, |dw| %.3g" % (label, dmax(lls, o[4]), dmax(mu_t, o[1]), dmax(w_t, o[2])))
    # A cloud of ONE point collapses on the covariance floor in its first M-step: the variance that is left is the 2e-6 of
    # the two regularisers, and the float32 statistics' rounding, 2^-24 d^2 = 1.5e-8 for d = 0.5, is a percent of it --
    # weights or none.  test_every_lane_layout's bound is for clouds that keep a variance of their own (N = 1500 + J there):
    # the one-point cloud is held to it before that M-step (lls[0]) and in its means, not in lls[1].
    k = 1 if N == 1 else 2
    np.testing.assert_allclose(lls[:k], o[4][:k], rtol=0, atol=3e-5)
    assert np.isfinite(lls).all()
    np.testing.assert_allclose(mu_t, o[1], rtol=0, atol=2e-5)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("J", [64, 65])
def test_mstep_every_instantiation_flag(ctx, J, weighted):
    """flat_mstep_kernel's three flags in one place: log / plain responsibilities (check_mstep runs both), rows that are whole
    16-byte pieces or not (J % 4), weights or none (unit weights in the restatement: its sums are then the unweighted ones)"""
    X, mu, inv, w, s = ragged(300, J)
    ctx.set_points(X)
    ctx.flat_set_weights(s if weighted else None)
    lr = ctx.flat_estep(inv, mu, w, "diag", "W")[1].get()
    check_mstep(ctx, X, s if weighted else np.ones(len(X), np.float32), lr, mu, "flags %dx%d %s" % (300, J, weighted))


@pytest.mark.parametrize("N,J", CHUNKED)
def test_chunked_path_against_the_restatement(ctx, N, J):
    """J > 1024 (test_large_component_counts_chunked_path's cloud, runs and bounds), the early stop included"""
    X, mu, inv, w, s = ragged(N, J)
    label = "weighted chunked %dx%d" % (N, J)
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    check_stats(ctx, X, s, inv, mu, w, True, label)
    _, lr = check_mean(ctx, X, s, inv, mu, w, label)
    check_mstep(ctx, X, s, lr.get(), mu, label)
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    inv_t, mu_t, w_t, cov_t, lls, conv = ctx.flat_train(3, 0.0, mu, cov0, w0, "diag", "W")
    o = fw.train(f64(X), s, 3, 0.0, f64(mu), f64(cov0), f64(w0), "diag", "W")
    live = o[2] > 1e-5
    print("%s train: max |dlls| %.3g, |dmu| %.3g, rel dw %.3g, rel dcov %.3g"
          % (label, dmax(lls, o[4]), dmax(mu_t[live], o[1][live]), float(np.abs(w_t / o[2] - 1).max()),
             float(np.abs(cov_t[live] / o[3][live] - 1).max())))
    np.testing.assert_allclose(lls, o[4], rtol=0, atol=3e-5)
    np.testing.assert_allclose(mu_t[live], o[1][live], rtol=0, atol=2e-5)
    np.testing.assert_allclose(w_t, o[2], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(cov_t[live], o[3][live], rtol=2e-3, atol=1e-7)
    r = ctx.flat_train(25, 0.05, mu, cov0, w0, "diag", "W")
    o2 = fw.train(f64(X), s, 25, 0.05, f64(mu), f64(cov0), f64(w0), "diag", "W")
    print("%s early stop: %d iterations (restatement %d), converged %s (%s)" % (label, len(r[4]), len(o2[4]), r[5], o2[5]))
    assert len(r[4]) == len(o2[4]) and r[5] == o2[5]


@pytest.mark.parametrize("variant,cov_type", FLAVOURS)
def test_train_small_against_the_restatement(ctx, variant, cov_type):
    """test_train_small's cloud, runs (2 and 5 iterations here) and bounds, all three flavour / covariance pairs"""
    X, mu0, cov0, w0 = golden_small(variant, cov_type)
    s = weights_for(len(X))
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    for iters in (2, 5):
        inv, mu, w, cov, lls, conv = ctx.flat_train(iters, 0.0, mu0, cov0, w0, cov_type, variant)
        o_inv, o_mu, o_w, o_cov, o_lls, _ = fw.train(f64(X), s, iters, 0.0, f64(mu0), f64(cov0), f64(w0), cov_type, variant)
        print("weighted train %s/%s %d iterations: max |dlls| %.3g, |dmu| %.3g, rel dw %.3g, rel dcov %.3g, rel dinv %.3g"
              % (variant, cov_type, iters, dmax(lls, o_lls), dmax(mu, o_mu), float(np.abs(w / o_w - 1).max()),
                 float(np.abs(cov / o_cov - 1).max()), float(np.abs(inv / o_inv - 1).max())))
        assert len(lls) == iters and not conv
        np.testing.assert_allclose(lls, o_lls, rtol=0, atol=2e-5)
        np.testing.assert_allclose(mu, o_mu, rtol=0, atol=5e-6)
        np.testing.assert_allclose(w, o_w, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(cov, o_cov, rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(inv, o_inv, rtol=1e-4)


def test_early_stop_follows_the_weighted_log_likelihood(ctx):
    """tol 0.05: the iteration count and the converged flag are the restatement's -- and not the unweighted fit's trace"""
    X, mu0, cov0, w0 = golden_small("W", "diag")
    s = weights_for(len(X))
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    inv, mu, w, cov, lls, conv = ctx.flat_train(30, 0.05, mu0, cov0, w0, "diag", "W")
    o = fw.train(f64(X), s, 30, 0.05, f64(mu0), f64(cov0), f64(w0), "diag", "W")
    print("early stop: %d iterations (restatement %d), converged %s (%s), max |dlls| %.3g" % (len(lls), len(o[4]), conv, o[5],
                                                                                             dmax(lls, o[4])))
    assert len(lls) == len(o[4]) and conv == o[5] and conv and len(lls) < 30
    np.testing.assert_allclose(lls, o[4], rtol=0, atol=2e-5)
    # the split form of the same loop
    ctx.flat_train_begin(0.05, mu0, cov0, w0, "diag", "W", lls_capacity=30)
    ctx.flat_train_step(30)
    r = ctx.flat_train_end()
    assert all(same_bits(a, b) for a, b in zip(r[:5], (inv, mu, w, cov, lls))) and r[5] == conv and r[6] == len(lls)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the one-launch boundary against the two launches, bit for bit, with weights
# ---------------------------------------------------------------------------------------------------------------------
def _context_under(value):
    import hgmm_amd
    old = os.environ.pop("HGMM_FLAT_BOUNDARY", None)
    try:
        os.environ["HGMM_FLAT_BOUNDARY"] = value
        return hgmm_amd.Context(0)
    finally:
        os.environ.pop("HGMM_FLAT_BOUNDARY", None)
        if old is not None:
            os.environ["HGMM_FLAT_BOUNDARY"] = old


def test_boundary_form_is_the_two_launches_bit_for_bit(bunny):
    one, two = _context_under("1"), _context_under("2")
    try:
        for (N, J), (variant, cov_type) in zip([(1999, 33), (4099, 100), (4099, 800)], FLAVOURS):
            X = np.ascontiguousarray(bunny[:N])
            s = weights_for(N)
            mu0, w0, cov0 = flat_em.seeded_init(X, J, 2, cov_type)
            cov0 = cov0 * np.float32(1e-3)
            res = []
            for c in (one, two):
                c.set_points(X)
                c.flat_set_weights(s)
                res.append(c.flat_train(6, 1e-4, mu0, cov0, w0, cov_type, variant))
            assert all(same_bits(a, b) for a, b in zip(res[0][:5], res[1][:5])) and res[0][5] == res[1][5], (N, J)
            assert np.isfinite(res[0][4]).all()
    finally:
        one.close()
        two.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. bitwise properties
# ---------------------------------------------------------------------------------------------------------------------
def _everything(ctx, inv, mu, w, cov0, w0, lr, cov_type="diag", variant="W"):
    """train, stats, M-step (log and plain) and the E-step mean under whatever weights are in force"""
    out = list(ctx.flat_train(4, 0.0, mu, cov0, w0, cov_type, variant)[:5])
    st = ctx.flat_stats(inv, mu, w, cov_type, variant)
    out += [st[0], np.float64(st[1]), np.float64(st[2])]
    out += list(ctx.flat_mstep(ctx.to_device(lr).exp(), cov_type, variant, centre_hint=mu))
    out += list(ctx.flat_mstep(np.exp(lr), cov_type, variant, centre_hint=mu))
    out.append(np.float64(ctx.flat_estep(inv, mu, w, cov_type, variant, want_log_resp=False)[0]))
    # (... and of the other two entries: asynchronous with the table written, device-resident parameters)
    out.append(np.float64(float(ctx.flat_estep(inv, mu, w, cov_type, variant, lazy_mean=True)[0])))
    out.append(np.float64(float(ctx.flat_estep(ctx.to_device(inv), ctx.to_device(mu), ctx.to_device(w), cov_type, variant,
                                               want_log_resp=False)[0])))
    return out


@pytest.mark.parametrize("N,J", [(777, 257), (1000, 64), (3000, 1025)])
def test_unit_weights_null_and_a_new_cloud_give_the_unweighted_bits(ctx, N, J):
    X, mu, inv, w, s = ragged(N, J)
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    ctx.set_points(X)
    lr = ctx.flat_estep(inv, mu, w, "diag", "W")[1].get()
    plain = _everything(ctx, inv, mu, w, cov0, w0, lr)
    assert plain[7] == N
    ctx.flat_set_weights(np.ones(N, np.float32))
    ones = _everything(ctx, inv, mu, w, cov0, w0, lr)
    assert all(same_bits(a, b) for a, b in zip(plain, ones)), [i for i, (a, b) in enumerate(zip(plain, ones)) if not same_bits(a, b)]
    ctx.flat_set_weights(s)
    weighted = _everything(ctx, inv, mu, w, cov0, w0, lr)
    assert not same_bits(weighted[1], plain[1]) and weighted[7] == fw.weight_sum(s)
    again = _everything(ctx, inv, mu, w, cov0, w0, lr)                       # two runs: the same bits
    assert all(same_bits(a, b) for a, b in zip(weighted, again))
    ctx.flat_set_weights(None)                                              # NULL takes the weights off
    assert all(same_bits(a, b) for a, b in zip(plain, _everything(ctx, inv, mu, w, cov0, w0, lr)))
    ctx.flat_set_weights(s)
    ctx.set_points(X)                                                       # a new cloud drops them
    assert all(same_bits(a, b) for a, b in zip(plain, _everything(ctx, inv, mu, w, cov0, w0, lr)))
    hd = ctx.points_create(X)                                               # ... and so does binding another one
    ctx.flat_set_weights(s)
    ctx.points_bind(hd)
    assert ctx.flat_stats(inv, mu, w, "diag", "W")[2] == N
    ctx.flat_set_weights(s)                                                 # weights on the bound handle's rows
    st = ctx.flat_stats(inv, mu, w, "diag", "W")
    assert same_bits(weighted[5], st[0]) and weighted[6] == st[1] and weighted[7] == st[2]
    ctx.points_destroy(hd)


@pytest.mark.parametrize("N,J", [(777, 257), (1000, 64), (500, 1024), (3000, 1025)])
def test_weights_of_two_double_the_statistics_exactly(ctx, N, J):
    X, mu, inv, w, s = ragged(N, J)
    ctx.set_points(X)
    st1, sl1, n1 = ctx.flat_stats(inv, mu, w, "diag", "W")
    ctx.flat_set_weights(np.full(N, 2.0, np.float32))
    st2, sl2, n2 = ctx.flat_stats(inv, mu, w, "diag", "W")
    assert n1 == N and n2 == 2 * N
    assert same_bits(st2, 2.0 * st1) and sl2 == 2.0 * sl1
    # ... and with the standard weights doubled (a power of two is exact in every product and sum)
    ctx.flat_set_weights(s)
    a = ctx.flat_stats(inv, mu, w, "diag", "W")
    ctx.flat_set_weights(2.0 * s)
    b = ctx.flat_stats(inv, mu, w, "diag", "W")
    assert same_bits(b[0], 2.0 * a[0]) and b[1] == 2.0 * a[1] and b[2] == 2.0 * a[2]


# ---------------------------------------------------------------------------------------------------------------------
# 4. a zero weight makes the row absent, whatever its coordinates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,J", [(777, 257), (1000, 64), (3000, 1025)])
def test_zero_weight_rows_are_absent_even_when_their_coordinates_are_nan(ctx, N, J):
    X, mu, inv, w, s = ragged(N, J)
    keep = s > 0
    assert 0 < (~keep).sum() < N
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    ctx.set_points(X)
    lr = ctx.flat_estep(inv, mu, w, "diag", "W")[1].get()
    ctx.flat_set_weights(s)
    full = _everything(ctx, inv, mu, w, cov0, w0, lr)
    # the same cloud without the rows: within the bounds of the shape's own test (the sums differ in their order only)
    ctx.set_points(X[keep])
    ctx.flat_set_weights(s[keep])
    cut = _everything(ctx, inv, mu, w, cov0, w0, lr[keep])
    print("zero rows %dx%d: max |dlls| %.3g, |dmu| %.3g, rel dw %.3g, rel d s0 %.3g, |d sum_lpn| %.3g, |d mean| %.3g"
          % (N, J, dmax(full[4], cut[4]), dmax(full[1], cut[1]), float(np.abs(full[2] / cut[2] - 1).max()),
             float(np.abs(full[5][:, 0] / cut[5][:, 0] - 1).max()), abs(full[6] - cut[6]), abs(full[14] - cut[14])))
    np.testing.assert_allclose(full[4], cut[4], rtol=0, atol=3e-5)
    np.testing.assert_allclose(full[1], cut[1], rtol=0, atol=2e-5)
    np.testing.assert_allclose(full[5][:, 0], cut[5][:, 0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(full[6], cut[6], rtol=1e-5, atol=1e-4)
    assert full[7] == cut[7] and all(abs(full[i] - cut[i]) <= 1e-5 * max(1.0, abs(cut[i])) for i in (14, 15, 16))
    live = f64(cut[8]) > 1e-6
    np.testing.assert_allclose(full[8], cut[8], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(full[9][live], cut[9][live], rtol=0, atol=1e-5)
    # NaN coordinates (and NaN responsibilities) in the rows of weight zero: every output finite and unchanged bit for bit
    Xn, lrn = X.copy(), lr.copy()
    Xn[~keep] = np.nan
    lrn[~keep] = np.nan
    ctx.set_points(Xn)
    ctx.flat_set_weights(s)
    nan = _everything(ctx, inv, mu, w, cov0, w0, lrn)
    assert all(np.isfinite(f64(a)).all() for a in nan)
    assert all(same_bits(a, b) for a, b in zip(full, nan)), [i for i, (a, b) in enumerate(zip(full, nan)) if not same_bits(a, b)]
    if J <= 1024:                                    # (without the weights the NaN rows do reach the fused kernel's sums)
        ctx.flat_set_weights(None)
        assert not np.isfinite(ctx.flat_stats(inv, mu, w, "diag", "W")[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. what weights buy: a count-weighted fit of the 4 mm voxel centroids of bun000 is the full scan's model
# ---------------------------------------------------------------------------------------------------------------------
def test_count_weighted_centroids_give_the_full_scans_model(ctx, bunny):
    """bun000 (40 256 points), its 4 mm voxel centroids (2 095), J = 16 means drawn with RandomState(1).choice among the
    centroids, cov0 1e-4, w0 1/J, flavour W, diag, 20 iterations at tol 0.  Mean log-normaliser of the FULL scan under the
    three models; the float64 restatement gives 7.9810 (full scan), 7.7962 (centroids), 7.9822 (centroids with counts)."""
    from hgmm_amd.pointcloud_io import voxel_down_sample
    cen, cnt = voxel_down_sample(bunny, 0.004, return_counts=True)
    cen = cen.astype(np.float32)
    assert len(bunny) == 40256 and len(cen) == 2095 and cnt.sum() == 40256
    J = 16
    mu0 = cen[np.random.RandomState(1).choice(len(cen), J, replace=False)]
    cov0, w0 = np.full((J, 3), 1e-4, np.float32), (np.ones(J) / J).astype(np.float32)
    models = {}
    ctx.set_points(bunny)
    models["full"] = ctx.flat_train(20, 0.0, mu0, cov0, w0, "diag", "W")
    ctx.set_points(cen)
    models["centroids"] = ctx.flat_train(20, 0.0, mu0, cov0, w0, "diag", "W")
    ctx.flat_set_weights(cnt)
    models["weighted"] = ctx.flat_train(20, 0.0, mu0, cov0, w0, "diag", "W")
    ctx.set_points(bunny)
    ll = {k: ctx.flat_estep(m[0], m[1], m[2], "diag", "W", want_log_resp=False)[0] for k, m in models.items()}
    for k in ("centroids", "weighted"):
        print("%-9s mean log-normaliser of the full scan %.4f (full fit %.4f), max pi error %.2g, max mu error %.3g mm"
              % (k, ll[k], ll["full"], dmax(models[k][2], models["full"][2]), 1e3 * dmax(models[k][1], models["full"][1])))
    assert ll["weighted"] >= ll["full"] - 0.01
    assert ll["centroids"] <= ll["full"] - 0.1


# ---------------------------------------------------------------------------------------------------------------------
# 6. two ranks on one GPU (host communicator): each holds its shard's weights, the count slot carries the rank's S
# ---------------------------------------------------------------------------------------------------------------------
N_RANKS, J_RANKS, CUT = 3001, 24, 1300


def _rank_inputs():
    rs = np.random.RandomState(21)
    X = (rs.rand(8, 3)[rs.randint(8, size=N_RANKS)] + 0.05 * rs.randn(N_RANKS, 3)).astype(np.float32)
    mu0, w0, cov0 = flat_em.seeded_init(X, J_RANKS, 4)
    return X, weights_for(N_RANKS, 23), mu0, w0, cov0


def _rank_run(ctx, lo, hi):
    X, s, mu0, w0, cov0 = _rank_inputs()
    ctx.set_points(X[lo:hi])
    ctx.flat_set_weights(s[lo:hi])
    out = {}
    for variant in ("W", "G"):
        inv, mu, w, cov, lls, _ = ctx.flat_train(6, 0.0, mu0, cov0, w0, "diag", variant)
        out[variant] = (mu, w, cov, np.asarray(lls))
    inv0 = (1.0 / np.sqrt(cov0)).astype(np.float32)
    out["stats"] = ctx.flat_stats(inv0, mu0, w0, "diag", "W")
    return out


def _rank_worker(rank, name, q):
    try:
        import hgmm_amd
        ctx = hgmm_amd.Context(0)
        ctx.comm_init_host(2, rank, name)
        lo, hi = (0, CUT) if rank == 0 else (CUT, N_RANKS)
        res = _rank_run(ctx, lo, hi)
        ctx.close()
        q.put((rank, res))
    except BaseException as e:                              # the parent must not wait out its timeout for a dead rank
        import traceback
        q.put((rank, "rank %d failed: %r\n%s" % (rank, e, traceback.format_exc())))
        raise


def test_two_ranks_on_one_gpu_match_the_single_context_weighted_fit():
    import hgmm_amd
    name = "hgmm_test_flatw_%d" % os.getpid()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_rank_worker, args=(r, name, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in procs:
        rank, res = q.get(timeout=300)
        assert not isinstance(res, str), res
        got[rank] = res
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    ctx = hgmm_amd.Context(0)
    ref = _rank_run(ctx, 0, N_RANKS)
    ctx.close()
    S = fw.weight_sum(_rank_inputs()[1])
    for variant in ("W", "G"):
        assert all(same_bits(a, b) for a, b in zip(got[0][variant], got[1][variant])), variant     # both ranks: the same bits
        mu, w, cov, lls = got[0][variant]
        rmu, rw, rcov, rlls = ref[variant]
        print("two ranks, flavour %s: max |dlls| %.3g, |dmu| %.3g, rel dw %.3g, rel dcov %.3g"
              % (variant, dmax(lls, rlls), dmax(mu, rmu), float(np.abs(w / rw - 1).max()), float(np.abs(cov / rcov - 1).max())))
        np.testing.assert_allclose(lls, rlls, rtol=0, atol=2e-6)                    # (tests/test_multirank_gpu.py's bounds)
        np.testing.assert_allclose(mu, rmu, rtol=0, atol=2e-6)
        np.testing.assert_allclose(w, rw, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(cov, rcov, rtol=1e-4, atol=1e-9)
    for r in range(2):
        st, sl, n = got[r]["stats"]
        assert abs(n - S) <= 1e-12 * S and abs(ref["stats"][2] - S) == 0          # the count slot carried both ranks' S
        print("two ranks, rank %d statistics: max rel d s0 %.3g, sum_lpn %.12g vs %.12g" % (r, float(np.abs(st[:, 0] / ref["stats"][0][:, 0] - 1).max()), sl, ref["stats"][1]))
        np.testing.assert_allclose(st[:, 0], ref["stats"][0][:, 0], rtol=1e-4, atol=1e-5)      # (test_ragged_sizes' bounds)
        np.testing.assert_allclose(sl, ref["stats"][1], rtol=1e-5, atol=1e-4)
    assert same_bits(got[0]["stats"][0], got[1]["stats"][0])


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors and state
# ---------------------------------------------------------------------------------------------------------------------
def _fptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_errors_and_state():
    import hgmm_amd
    from hgmm_amd import HgmmError
    X, mu, inv, w, s = ragged(1000, 64)
    n = len(X)
    c = hgmm_amd.Context(0)
    try:
        lib, h = c.lib, c.h
        ones = np.ones(n, np.float32)
        # no cloud: HGMM_ERR_STATE, also for NULL
        assert lib.hgmm_flat_set_weights(h, _fptr(ones), n) == HGMM_ERR_STATE
        assert lib.hgmm_flat_set_weights(h, None, 0) == HGMM_ERR_STATE
        with pytest.raises(HgmmError, match="no cloud"):
            c.flat_set_weights(ones)
        # a forest cloud resident: no float32 rows to weight
        c.set_points_batch([f64(X[:400]), f64(X[400:])])
        assert lib.hgmm_flat_set_weights(h, _fptr(ones), n) == HGMM_ERR_STATE
        assert b"hgmm_flat_set_weights" in lib.hgmm_last_error(h)
        c.set_points(X)
        c.flat_set_weights(s)
        ref = c.flat_stats(inv, mu, w, "diag", "W")
        assert ref[2] == fw.weight_sum(s)
        bad = {"length": (ones[:-1], b"1000"), "negative": (np.r_[ones[:-1], np.float32(-1e-3)], b" 999 "),
               "nan": (np.r_[np.float32(np.nan), ones[1:]], b" 0 "), "infinite": (np.r_[ones[:5], np.float32(np.inf), ones[6:]], b" 5 "),
               "all zero": (np.zeros(n, np.float32), b"zero")}
        for name, (v, word) in bad.items():
            v = np.ascontiguousarray(v, dtype=np.float32)
            assert lib.hgmm_flat_set_weights(h, _fptr(v), len(v)) == HGMM_ERR_ARG, name
            msg = lib.hgmm_last_error(h)
            assert b"hgmm_flat_set_weights" in msg and word in msg, (name, msg)
            with pytest.raises(HgmmError):
                c.flat_set_weights(v)
            # the previous weights survived the refused upload
            again = c.flat_stats(inv, mu, w, "diag", "W")
            assert same_bits(ref[0], again[0]) and ref[1:] == again[1:], name
        with pytest.raises(ValueError):
            c.flat_set_weights(np.ones((n, 1)))
        # float64 input is taken as the float32 values the device holds; a negative zero is a zero
        c.flat_set_weights(s.astype(np.float64))
        assert c.flat_stats(inv, mu, w, "diag", "W")[2] == ref[2]
        sz = s.copy()
        sz[s == 0] = -0.0
        c.flat_set_weights(sz)
        again = c.flat_stats(inv, mu, w, "diag", "W")
        assert same_bits(ref[0], again[0]) and ref[1:] == again[1:]
        # the handle the weights were on is destroyed: no cloud again
        hd = c.points_create(X)
        c.points_bind(hd)
        c.flat_set_weights(s)
        c.points_destroy(hd)
        with pytest.raises(HgmmError):
            c.flat_set_weights(s)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the Python mirrors
# ---------------------------------------------------------------------------------------------------------------------
def test_mirrors_agree(bunny):
    import hgmm_amd
    from hgmm_amd.gmm_waymo import gmm as Wg, gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm as Gg
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    from hgmm_amd.pointcloud_io import voxel_down_sample
    cen, cnt = voxel_down_sample(bunny[::4], 0.006, return_counts=True)
    cen = cen.astype(np.float32)
    J = 12
    mu0, w0, cov0 = flat_em.seeded_init(cen, J, 3)
    cov0 = cov0 * np.float32(1e-2)

    def fitted(f):
        return [np.asarray(a) for a in (f.means_, f.weights_, f.covariances_, f.inv_covs, f.lls)]

    ref = fitted(Wg.GMM_GPU_Base(J, max_iter=5, tol=0.0).fit(cen, init=(mu0, w0, cov0), sample_weight=cnt))
    plain = fitted(Wg.GMM_GPU_Base(J, max_iter=5, tol=0.0).fit(cen, init=(mu0, w0, cov0)))
    assert not same_bits(ref[0], plain[0])
    o = fw.train(f64(cen), cnt.astype(np.float32), 5, 0.0, f64(mu0), f64(cov0), f64(w0), "diag", "W")
    np.testing.assert_allclose(ref[4], o[4], rtol=0, atol=2e-5)
    np.testing.assert_allclose(ref[0], o[1], rtol=0, atol=5e-6)
    for X in (WeightedPoints(cen, cnt), hgmm_amd.DevicePoints(cen, weights=cnt), hgmm_amd.asarray(cen, weights=cnt)):
        got = fitted(Wg.GMM_GPU_Base(J, max_iter=5, tol=0.0).fit(X, init=(mu0, w0, cov0)))
        assert all(same_bits(a, b) for a, b in zip(ref, got)), type(X)
    # the module functions: sample_weight=, and a resident cloud that brings its own
    dp = hgmm_amd.DevicePoints(cen, weights=cnt)
    for r in (W.train_gmm(cen, 5, 0.0, mu0, cov0, w0, sample_weight=cnt), W.train_gmm(dp, 5, 0.0, mu0, cov0, w0)):
        assert same_bits(r[1], ref[0]) and same_bits(r[2], ref[1])
    assert same_bits(W.train_gmm(dp, 5, 0.0, mu0, cov0, w0, sample_weight=np.ones(len(cen)))[1], plain[0])
    assert same_bits(W.train_gmm(hgmm_amd.asarray(cen), 5, 0.0, mu0, cov0, w0)[1], plain[0])       # nothing lingers
    lr = W.e_step(cen, ref[3], ref[0], ref[1])[1]
    m_w = W.m_step(cen, lr.exp(), sample_weight=cnt)
    m_dp = W.m_step(dp, lr.exp())
    assert all(same_bits(np.asarray(_get(a)), np.asarray(_get(b))) for a, b in zip(m_w, m_dp))
    e_w, e_dp, e_plain = float(W.e_step(cen, ref[3], ref[0], ref[1], sample_weight=cnt)[0]), float(W.e_step(dp, ref[3], ref[0], ref[1])[0]), \
        float(W.e_step(cen, ref[3], ref[0], ref[1])[0])
    assert e_w == e_dp and e_w != e_plain
    dp.free()
    # GMM_GPU.compute of both flavours: a WeightedPoints brings its weights, weights= is fit(..., sample_weight=)
    for mod, kw in ((Wg, dict(cov_type="diag")), (Gg, dict())):
        res = []
        for call in (lambda f: f.compute(WeightedPoints(cen, cnt)), lambda f: f.compute(cen, weights=cnt),
                     lambda f: (f._clf.fit(cen, sample_weight=cnt), (f._clf.means_, f._clf.weights_))[1], lambda f: f.compute(cen)):
            np.random.seed(5)                                   # (flavour W draws its initial means with the host RNG)
            f = mod.GMM_GPU(n_gmm_components=J, max_iter=4, tol=0.0, **kw)
            f.init()
            res.append(call(f))
        assert all(same_bits(a, b) for a, b in zip(res[0][:2], res[1][:2])) and all(same_bits(a, b) for a, b in zip(res[0][:2], res[2][:2]))
        assert not same_bits(res[0][0], res[3][0])


def _get(a):
    return a.get() if hasattr(a, "get") else a
