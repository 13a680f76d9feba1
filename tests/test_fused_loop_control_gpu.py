"""The fused EM kernel's loop bounds, set-up and epilogue (flat_fused_pk_kernel) at the shapes where they can go wrong.

The kernel keeps a wave's first row and row count in scalar registers, counts its rows from zero (prefetch clamp, the
8-row flush of the log-normalisers, the exit test) and combines the four waves of a workgroup over three LDS copies.  Every
case is held to the float64 oracle (oracle.flat_em; tests/_flat_weight_oracle.py with per-point weights) at the bounds
tests/test_flat_gpu.py and tests/test_flat_weights_gpu.py hold small clouds to -- test_ragged_sizes for the statistics,
test_every_lane_layout for two iterations of training -- and every case runs twice and asks for the same bits.
Every case prints its largest differences before it asserts.
"""
import warnings

import numpy as np
import pytest

import _flat_weight_oracle as fw
from oracle import flat_em

pytestmark = pytest.mark.gpu

f64 = lambda a: np.asarray(a, dtype=np.float64)
WAVES_PER_BLOCK, FLAT_MAX_BLOCKS = 4, 2048


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max())


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def model(J, seed, N=None):
    """test_every_lane_layout's kind of cloud and model"""
    N = 1500 + J if N is None else N
    rs = np.random.RandomState(seed)
    X = rs.rand(N, 3).astype(np.float32)
    mu = rs.rand(J, 3).astype(np.float32)
    inv = (1.0 / np.sqrt(0.005 + 0.05 * rs.rand(J, 3))).astype(np.float32)
    w = rs.rand(J).astype(np.float32) + 0.01
    w /= w.sum()
    return X, mu, inv, w


def oracle_stats(X, inv, mu, w, variant="W"):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # (log(0) of a dead component)
        with np.errstate(all="ignore"):
            _, lr, lpn, _ = flat_em.e_step_full(f64(X), f64(inv), f64(mu), f64(w), "diag", variant)
    r = np.exp(lr)
    d = f64(X)[:, None, :] - f64(mu)[None]
    return np.concatenate([r.sum(0)[:, None], (r[:, :, None] * d).sum(0), (r[:, :, None] * d * d).sum(0)], axis=1), lpn.sum()


def assert_stats(label, got, want, live=None):
    """test_ragged_sizes' bounds"""
    (stats, sum_lpn, _), (o_stats, o_sum) = got, want
    live = slice(None) if live is None else live
    print("%s: sum_lpn %.10g vs %.10g, max |d s0| %.3g, |d a| %.3g, |d b| %.3g"
          % (label, sum_lpn, o_sum, dmax(stats[live, 0], o_stats[live, 0]), dmax(stats[live, 1:4], o_stats[live, 1:4]),
             dmax(stats[live, 4:7], o_stats[live, 4:7])))
    np.testing.assert_allclose(sum_lpn, o_sum, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(stats[live, 0], o_stats[live, 0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(stats[live, 1:4], o_stats[live, 1:4], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(stats[live, 4:7], o_stats[live, 4:7], rtol=1e-3, atol=2e-5)


def stats_twice(ctx, inv, mu, w, variant="W"):
    a = ctx.flat_stats(inv, mu, w, "diag", variant)
    b = ctx.flat_stats(inv, mu, w, "diag", variant)
    assert same_bits(a[0], b[0]) and same_bits(np.float64(a[1]), np.float64(b[1])) and a[2] == b[2]
    return a


def train_twice(ctx, iters, mu, cov0, w0):
    a = ctx.flat_train(iters, 0.0, mu, cov0, w0, "diag", "W")
    b = ctx.flat_train(iters, 0.0, mu, cov0, w0, "diag", "W")
    assert all(same_bits(x, y) for x, y in zip(a[:5], b[:5]))
    return a


def assert_train(label, got, o, k=None):
    """test_every_lane_layout's bounds"""
    inv_t, mu_t, w_t, cov_t, lls, _ = got
    k = len(lls) if k is None else k
    print("%s train: max |dlls| %.3g, |dmu| %.3g" % (label, dmax(lls[:k], np.array(o[4])[:k]), dmax(mu_t, o[1])))
    assert np.isfinite(lls).all()
    np.testing.assert_allclose(lls[:k], np.array(o[4])[:k], rtol=0, atol=3e-5)
    np.testing.assert_allclose(mu_t, o[1], rtol=0, atol=2e-5)


def fused_rows_per_wave(N, J, cus):
    """launch_fused's grid rule and wave_row_range's split: the set of row counts the fused kernel's waves own"""
    ns = (J + 63) // 64
    bpc_max = 8 if ns <= 4 else (6 if ns <= 8 else 4)
    big = min(N // (WAVES_PER_BLOCK * 100), cus * bpc_max, FLAT_MAX_BLOCKS)
    floor2 = max(1, min((N + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK, min(cus * 2, FLAT_MAX_BLOCKS)))
    nw = max(floor2, big) * WAVES_PER_BLOCK
    per = (N + nw - 1) // nw
    full, rest = divmod(N, per)                               # waves with `per` rows, then one with the rest, then none
    return ({per} if full else set()) | ({rest} if rest else set()) | ({0} if full + (rest > 0) < nw else set())


def cloud_with_waves_of(want, J, cus):
    for N in range(1, 60000):
        if set(want) <= fused_rows_per_wave(N, J, cus):
            return N
    raise AssertionError("no cloud size gives waves of %s rows" % (want,))


# ---------------------------------------------------------------------------------------------------------------------
# loop bounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65])
def test_small_clouds_waves_without_rows_and_the_last_rows_prefetch(ctx, N):
    J = 800
    X, mu, inv, w = model(J, 100 + N, N)
    ctx.set_points(X)
    assert_stats("N=%d J=%d" % (N, J), stats_twice(ctx, inv, mu, w), oracle_stats(X, inv, mu, w))
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    # ONE iteration: a few points among 800 components collapse on the covariance floor in their first M-step (the oracle's
    # smallest variance after it is the 1e-6 floor for N = 1 and 3), and from there on the float32 statistics' rounding is
    # a percent of the variance that is left (tests/test_flat_weights_gpu.py on its one-point cloud)
    o = flat_em.train(f64(X), 1, 0.0, f64(mu), f64(cov0), f64(w0), "diag", "W")
    assert_train("N=%d J=%d" % (N, J), train_twice(ctx, 1, mu, cov0, w0), o)


@pytest.mark.parametrize("want", [(7, 9), (7, 8)])
def test_waves_of_seven_eight_and_nine_rows_round_the_flush(ctx, want):
    J = 800
    N = cloud_with_waves_of(want, J, ctx.device_info()["compute_units"])
    X, mu, inv, w = model(J, 7, N)
    ctx.set_points(X)
    assert_stats("waves of %s rows (N=%d)" % (want, N), stats_twice(ctx, inv, mu, w), oracle_stats(X, inv, mu, w))


@pytest.mark.parametrize("J", [64, 100, 769, 800, 832])
def test_slot_counts_full_half_empty_and_one_wide_tail(ctx, J):
    X, mu, inv, w = model(J, J)
    ctx.set_points(X)
    assert_stats("J=%d" % J, stats_twice(ctx, inv, mu, w), oracle_stats(X, inv, mu, w))
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    o = flat_em.train(f64(X), 2, 0.0, f64(mu), f64(cov0), f64(w0), "diag", "W")
    assert_train("J=%d" % J, train_twice(ctx, 2, mu, cov0, w0), o)


# ---------------------------------------------------------------------------------------------------------------------
# set-up: the table's largest constant and the origin of the first moments
# ---------------------------------------------------------------------------------------------------------------------
def test_a_needle_component_takes_the_row_maximum_loop(ctx):
    """One component with sigma = 1e-8 on every axis: its constant, log2(e) (3 log 1e8 - 1.5 log 2 pi + log w) = 66 with
    w = 1/800, is above CS_MAX_SHIFT = 60, so the whole launch runs the row-maximum loop.  The needle sits on the cloud's
    first point, both at the coordinate origin, where the oracle's expanded quadratic form cancels nothing."""
    J = 800
    X, mu, inv, w = model(J, 31)
    X[0] = 0.0
    mu[17] = 0.0
    inv[17] = 1e8
    w[:] = 1.0 / J
    assert np.log2(np.e) * (3 * np.log(1e8) - 1.5 * np.log(2 * np.pi) + np.log(1.0 / J)) > 65.0
    ctx.set_points(X)
    got = stats_twice(ctx, inv, mu, w)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1])
    assert_stats("needle", got, oracle_stats(X, inv, mu, w))
    assert abs(got[0][17, 0] - 1.0) < 1e-5                     # the needle owns its point and nothing else


def test_dead_and_nan_components_and_all_weights_zero(ctx):
    J = 800
    X, mu, inv, w = model(J, 41)
    ctx.set_points(X)
    # flavour G takes log(w) as it is: a weight of zero is a dead component (constant -inf), a NaN weight is packed as one
    # too; neither counts towards the origin.  The oracle gets both as zero.
    w_dead = w.copy()
    w_dead[5] = 0.0
    w_nan = w_dead.copy()
    w_nan[700] = np.nan
    w_dead[700] = 0.0
    got = stats_twice(ctx, inv, mu, w_nan, "G")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1])
    assert not got[0][[5, 700]].any()
    assert_stats("dead and NaN", got, oracle_stats(X, inv, mu, w_dead, "G"))
    # flavour W takes log(w + eps): all weights zero are 800 equal components, and an origin with nothing to average
    w_zero = np.zeros(J, np.float32)
    assert_stats("all weights zero", stats_twice(ctx, inv, mu, w_zero), oracle_stats(X, inv, mu, w_zero))


# ---------------------------------------------------------------------------------------------------------------------
# per-point weights
# ---------------------------------------------------------------------------------------------------------------------
def test_unit_weights_are_the_unweighted_bits_and_nan_rows_of_weight_zero_are_absent(ctx):
    J = 800
    X, mu, inv, w = model(J, 51)
    N = len(X)
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    ctx.set_points(X)
    plain = list(stats_twice(ctx, inv, mu, w)) + list(train_twice(ctx, 2, mu, cov0, w0)[:5])
    ctx.flat_set_weights(np.ones(N, np.float32))
    ones = list(stats_twice(ctx, inv, mu, w)) + list(train_twice(ctx, 2, mu, cov0, w0)[:5])
    assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(plain, ones))
    s = fw.standard_weights(N)
    assert 0 < (s == 0).sum() < N
    Xn = X.copy()
    Xn[s == 0] = np.nan
    ctx.set_points(Xn)
    ctx.flat_set_weights(s)
    got = stats_twice(ctx, inv, mu, w)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]) and got[2] == fw.weight_sum(s)
    o_stats, o_sum, _ = fw.stats(f64(X), s, f64(inv), f64(mu), f64(w), "diag", "W")
    assert_stats("weighted, NaN rows of weight zero", got, (o_stats, o_sum))
    assert_train("weighted", train_twice(ctx, 2, mu, cov0, w0),
                 fw.train(f64(X), s, 2, 0.0, f64(mu), f64(cov0), f64(w0), "diag", "W"))
    ctx.flat_set_weights(None)


# ---------------------------------------------------------------------------------------------------------------------
# the split training loop
# ---------------------------------------------------------------------------------------------------------------------
def test_split_training_loop_is_the_one_call_bit_for_bit(ctx):
    J = 800
    X, mu, inv, w = model(J, 61)
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    ctx.set_points(X)
    whole = train_twice(ctx, 3, mu, cov0, w0)
    assert_train("three iterations", whole, flat_em.train(f64(X), 3, 0.0, f64(mu), f64(cov0), f64(w0), "diag", "W"))
    for steps in ((1, 1, 1), (3,)):
        ctx.flat_train_begin(0.0, mu, cov0, w0, "diag", "W", lls_capacity=3)
        for k in steps:
            ctx.flat_train_step(k)
        r = ctx.flat_train_end()
        assert all(same_bits(a, b) for a, b in zip(r[:5], whole[:5])) and r[6] == 3, steps
