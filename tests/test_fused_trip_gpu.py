"""The fused EM kernel's eight-row trip (csrc/flat_fused_body.h) at the row counts where a trip loop can go wrong.

The constant-shift loop runs full trips of eight rows while eight are left -- no per-row clamp, exit test or flush test, the
coordinates and weights fetched half a trip at a time, one float64 flush of the log-normalisers per trip -- and hands the
last ``nrows % 8`` rows to a loop of one row per trip.  The clouds here give their waves 0, 1, 7, 8, 9, 15, 16 and 17 rows
(sizes found from the grid rule for the device's CU count, row counts computed and asserted in the test), at J = 800 (13
slots per lane), 100 and 64.  Plain fits, fits with per-point weights whose zeros sit on rows 7 and 8 of every wave (the
last row of a trip and the first of the next), and one batched launch that mixes them.

Every fit runs 3 iterations from ``seeded_init`` and is held to the float64 oracle (oracle.flat_em.train;
tests/_flat_weight_oracle.train with weights) at the bounds tests/test_flat_gpu.py holds the fused path to (lls 3e-5, mu
2e-5: test_every_lane_layout).  Every cloud's statistics are also compared with the kernel's other loop, the row-maximum
variant, which keeps one row per trip: the same table with one component -- six units away from the unit cube, so that it
owns nothing in either loop -- narrowed to sigma = 1e-8, which puts the largest constant above the constant-shift range
(test_a_needle_component_takes_the_row_maximum_loop).  The two loops are held to each other at the bounds at which the
existing tests hold each of them to the oracle (test_ragged_sizes).  Oracles are computed once per (cloud, J, weights).
Every case prints its largest differences before it asserts.
"""
import numpy as np
import pytest

import _flat_weight_oracle as fw
from oracle import flat_em

pytestmark = pytest.mark.gpu

f64 = lambda a: np.asarray(a, dtype=np.float64)
WAVES_PER_BLOCK, FLAT_MAX_BLOCKS = 4, 2048
ITERS = 3
# the row counts a cloud's waves must have, one cloud each
WANTED = {"0_1": (0, 1), "7_8": (7, 8), "9_16": (9, 16), "15_17": (15, 17)}


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


def dmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max())


def wave_rows(N, J, cus):
    """launch_fused's grid rule (fused_grid) and wave_row_range's split: (rows per full wave, full waves, rows of the wave
    after them, waves in all)"""
    ns = (J + 63) // 64
    bpc_max = 8 if ns <= 4 else (6 if ns <= 8 else 4)
    big = min(N // (WAVES_PER_BLOCK * 100), cus * bpc_max, FLAT_MAX_BLOCKS)
    floor2 = max(1, min((N + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK, min(cus * 2, FLAT_MAX_BLOCKS)))
    nw = max(floor2, big) * WAVES_PER_BLOCK
    per = (N + nw - 1) // nw
    full, rest = divmod(N, per)
    return per, full, rest, nw


def row_counts(N, J, cus):
    per, full, rest, nw = wave_rows(N, J, cus)
    return ({per} if full else set()) | ({rest} if rest else set()) | ({0} if full + (rest > 0) < nw else set())


_sizes = {}


def cloud_size(name, cus):
    """The smallest cloud of at least 800 points (seeded_init draws J distinct points) whose waves have the wanted row counts
    at every J of this file"""
    if (name, cus) not in _sizes:
        want = set(WANTED[name])
        _sizes[name, cus] = next(N for N in range(800, 80000) if all(want <= row_counts(N, J, cus) for J in (64, 100, 800)))
    return _sizes[name, cus]


def cloud(name, cus):
    N = cloud_size(name, cus)
    return np.random.RandomState(N).rand(N, 3).astype(np.float32)


def trip_weights(N, J, cus):
    """1 + (i % 3), and zero on rows 7 and 8 of every wave that has them"""
    per, full, rest, nw = wave_rows(N, J, cus)
    s = (1 + np.arange(N) % 3).astype(np.float32)
    for r in (7, 8):
        at = np.arange(nw, dtype=np.int64) * per + r
        s[at[(at < N) & (r < per)]] = 0
    assert 0 < (s == 0).sum() < N or per <= 7
    return s


_oracles = {}


def oracle(name, J, weighted, cus):
    key = (name, J, weighted, cus)
    if key not in _oracles:
        X = cloud(name, cus)
        mu0, w0, cov0 = flat_em.seeded_init(X, J, 1)
        if weighted:
            o = fw.train(f64(X), trip_weights(len(X), J, cus), ITERS, 0.0, f64(mu0), f64(cov0), f64(w0), "diag", "W")
        else:
            o = flat_em.train(f64(X), ITERS, 0.0, f64(mu0), f64(cov0), f64(w0), "diag", "W")
        _oracles[key] = (np.array(o[4]), np.array(o[1]))
    return _oracles[key]


def assert_fit(label, got, want):
    """test_every_lane_layout's bounds"""
    lls, mu = got[4], got[1]
    print("%s: max |dlls| %.3g, |dmu| %.3g" % (label, dmax(lls, want[0]), dmax(mu, want[1])))
    assert len(lls) == ITERS and np.isfinite(lls).all()
    np.testing.assert_allclose(lls, want[0], rtol=0, atol=3e-5)
    np.testing.assert_allclose(mu, want[1], rtol=0, atol=2e-5)


def assert_other_loop(ctx, label, X, J):
    """flat_stats of one table through the constant-shift loop and through the row-maximum loop (test_ragged_sizes' bounds)"""
    mu0, w0, cov0 = flat_em.seeded_init(X, J, 1)
    inv = flat_em.inv_std_from_cov(cov0, "W", initial=True).astype(np.float32)
    mu0 = mu0.copy()
    mu0[J // 2] = 6.0                                          # owns nothing: 2^-(3 * 25 / 0.2 * log2 e) is zero in float32
    needle = inv.copy()
    needle[J // 2] = 1e8
    assert np.log2(np.e) * (3 * np.log(1e8) - 1.5 * np.log(2 * np.pi) + np.log(1.0 / J)) > 65.0
    (cs, cs_lpn, cs_sw), (rm, rm_lpn, rm_sw) = ctx.flat_stats(inv, mu0, w0, "diag", "W"), ctx.flat_stats(needle, mu0, w0, "diag", "W")
    print("%s, constant shift against row maximum: sum_lpn %.10g vs %.10g, max |d s0| %.3g, |d a| %.3g, |d b| %.3g"
          % (label, cs_lpn, rm_lpn, dmax(cs[:, 0], rm[:, 0]), dmax(cs[:, 1:4], rm[:, 1:4]), dmax(cs[:, 4:7], rm[:, 4:7])))
    assert np.isfinite(cs).all() and np.isfinite(rm).all() and cs_sw == rm_sw
    assert not cs[J // 2].any() and not rm[J // 2].any()
    np.testing.assert_allclose(cs_lpn, rm_lpn, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(cs[:, 0], rm[:, 0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(cs[:, 1:4], rm[:, 1:4], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(cs[:, 4:7], rm[:, 4:7], rtol=1e-3, atol=2e-5)


def fit(ctx, X, J, s=None):
    mu0, w0, cov0 = flat_em.seeded_init(X, J, 1)
    ctx.set_points(X)
    ctx.flat_set_weights(s)
    return ctx.flat_train(ITERS, 0.0, mu0, cov0, w0, "diag", "W")


@pytest.mark.parametrize("J", [800, 100, 64])
@pytest.mark.parametrize("name", list(WANTED))
def test_plain_fits(ctx, name, J):
    cus = ctx.device_info()["compute_units"]
    X = cloud(name, cus)
    counts = row_counts(len(X), J, cus)
    assert set(WANTED[name]) <= counts, (len(X), counts)
    label = "plain J=%d N=%d, waves of %s rows" % (J, len(X), sorted(counts))
    assert_fit(label, fit(ctx, X, J), oracle(name, J, False, cus))
    assert_other_loop(ctx, label, X, J)


@pytest.mark.parametrize("name,J", [("9_16", 800), ("7_8", 800), ("15_17", 100), ("7_8", 64), ("15_17", 64)])
def test_weighted_fits_with_zero_weights_on_rows_7_and_8(ctx, name, J):
    cus = ctx.device_info()["compute_units"]
    X = cloud(name, cus)
    s = trip_weights(len(X), J, cus)
    counts = row_counts(len(X), J, cus)
    assert set(WANTED[name]) <= counts and (s == 0).any(), (len(X), counts)
    label = "weighted J=%d N=%d, waves of %s rows, %d rows of weight zero" % (J, len(X), sorted(counts), int((s == 0).sum()))
    try:
        assert_fit(label, fit(ctx, X, J, s), oracle(name, J, True, cus))
        assert_other_loop(ctx, label, X, J)                    # (the weights are still in force)
    finally:
        ctx.flat_set_weights(None)


def test_one_batched_launch_mixes_plain_and_weighted_members(ctx):
    """Members: plain with waves of 7 and 8 rows, weighted with waves of 9 and 16, plain with waves of 0 and 1, weighted with
    waves of 7 and 8 -- an unweighted and a weighted fused launch per iteration.  Each member is the serial fit bit for bit
    (tests/test_flat_batch_weights_gpu.py) and is held to the oracle."""
    J = 800
    cus = ctx.device_info()["compute_units"]
    names = ["7_8", "9_16", "0_1", "7_8"]
    weighted = [False, True, False, True]
    clouds = [cloud(n, cus) for n in names]
    ws = [trip_weights(len(X), J, cus) if wt else None for X, wt in zip(clouds, weighted)]
    inits = [flat_em.seeded_init(X, J, 1) for X in clouds]
    hs = [ctx.points_create(X) for X in clouds]
    try:
        got = ctx.flat_train_batch(hs, ITERS, 0.0, [i[0] for i in inits], [i[2] for i in inits], [i[1] for i in inits],
                                   "diag", "W", weights=ws)
    finally:
        for h in hs:
            ctx.points_destroy(h)
    try:
        for b, (name, wt, X, s) in enumerate(zip(names, weighted, clouds, ws)):
            label = "batch member %d (%s, %s)" % (b, name, "weighted" if wt else "plain")
            assert_fit(label, got[b], oracle(name, J, wt, cus))
            alone = fit(ctx, X, J, s)
            for what, x, y in zip(("inv", "mu", "w", "cov", "lls"), got[b], alone):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "%s: %s is not the serial fit's" % (label, what)
    finally:
        ctx.flat_set_weights(None)
