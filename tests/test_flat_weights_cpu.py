"""Per-point weights of the flat (diag / spherical) GMM fit (hgmm_flat_set_weights), the parts that need no GPU: the
float64 restatement the GPU tests compare against (tests/_flat_weight_oracle.py) is oracle.flat_em with unit weights and
oracle.flat_em on a repeated cloud with integer weights; the Python mirrors check their arguments, upload the cloud before
its weights and take a WeightedPoints apart; the C entry is declared, exported, bound and documented."""
import inspect
import os
import re

import numpy as np
import pytest

import _flat_weight_oracle as fw
from conftest import ROOT
from oracle import flat_em

FLAVOURS = [("W", "diag"), ("W", "spherical"), ("G", "diag")]


def _cloud(bunny, n=700, J=8, seed=3):
    rng = np.random.default_rng(seed)
    X = bunny[rng.choice(len(bunny), n, replace=False)].astype(np.float64)
    mu0 = X[rng.choice(n, J, replace=False)].copy()
    return X, mu0, np.ones(J) / J, rng


def _cov0(J, cov_type):
    return np.full((J, 3) if cov_type == "diag" else (J,), 1e-4)


@pytest.mark.parametrize("variant,cov_type", FLAVOURS)
def test_unit_weights_are_the_unweighted_oracle(bunny, variant, cov_type):
    X, mu0, w0, _ = _cloud(bunny)
    a = fw.train(X, np.ones(len(X), np.float32), 5, 0.0, mu0, _cov0(8, cov_type), w0, cov_type, variant)
    b = flat_em.train(X, 5, 0.0, mu0, _cov0(8, cov_type), w0, cov_type, variant)
    for x, y in zip(a[:5], b[:5]):
        np.testing.assert_allclose(x, y, rtol=1e-13, atol=0)
    assert a[5] == b[5]
    inv, mu, w = b[0], b[1], b[2]
    s = np.ones(len(X), np.float32)
    st, sl, S = fw.stats(X, s, inv, mu, w, cov_type, variant)
    mean, lr, lpn = fw.e_step(X, s, inv, mu, w, cov_type, variant)
    o_mean, o_lr = flat_em.e_step(X, inv, mu, w, cov_type, variant)
    assert S == len(X) and abs(mean - o_mean) <= 1e-13 * abs(o_mean) and abs(sl - lpn.sum()) <= 1e-12 * abs(sl)
    np.testing.assert_array_equal(lr, o_lr)
    np.testing.assert_allclose(st[:, 0], np.exp(o_lr).sum(0), rtol=1e-13)
    for x, y in zip(fw.m_step(X, s, np.exp(o_lr), cov_type, variant), flat_em.m_step(X, np.exp(o_lr), cov_type, variant)):
        np.testing.assert_allclose(x, y, rtol=1e-13, atol=0)


@pytest.mark.parametrize("variant", ["W", "G"])
def test_integer_weights_are_repetition(bunny, variant):
    """700 bunny points, J = 8, 5 iterations, both flavours: the weighted restatement is flat_em.train on np.repeat, to 1e-8
    on inv and 1e-12 elsewhere (the order of summation differs, nothing else)."""
    X, mu0, w0, rng = _cloud(bunny)
    c = rng.integers(0, 5, len(X))
    c[:3] = (0, 1, 4)
    a = fw.train(X, c.astype(np.float32), 5, 0.0, mu0, _cov0(8, "diag"), w0, "diag", variant)
    b = flat_em.train(np.repeat(X, c, axis=0), 5, 0.0, mu0, _cov0(8, "diag"), w0, "diag", variant)
    d = [np.abs(np.asarray(x) - np.asarray(y)).max() for x, y in zip(a[:5], b[:5])]
    rel_inv = np.abs(a[0] / b[0] - 1).max()
    print("flavour %s: max |inv, mu, w, cov, lls difference| %s, inv relative %.3g" % (variant, d, rel_inv))
    assert rel_inv <= 1e-8
    for x, y in zip(a[1:5], b[1:5]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12)
    assert a[5] == b[5]
    st_a = fw.stats(X, c.astype(np.float32), b[0], b[1], b[2], "diag", variant)
    st_b = fw.stats(np.repeat(X, c, axis=0), np.ones(int(c.sum()), np.float32), b[0], b[1], b[2], "diag", variant)
    np.testing.assert_allclose(st_a[0], st_b[0], rtol=1e-10, atol=1e-12)
    assert abs(st_a[1] - st_b[1]) <= 1e-10 * abs(st_b[1]) and st_a[2] == st_b[2] == c.sum()


def test_zero_weight_rows_are_absent_whatever_their_coordinates(bunny):
    X, mu0, w0, _ = _cloud(bunny)
    s = fw.standard_weights(len(X))
    assert (s == 0).sum() > 20 and s.dtype == np.float32
    Xn = X.copy()
    Xn[s == 0] = np.nan
    a = fw.train(X, s, 4, 0.0, mu0, _cov0(8, "diag"), w0)
    b = fw.train(Xn, s, 4, 0.0, mu0, _cov0(8, "diag"), w0)
    c = fw.train(X[s > 0], s[s > 0], 4, 0.0, mu0, _cov0(8, "diag"), w0)
    for x, y, z in zip(a[:5], b[:5], c[:5]):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
        assert np.isfinite(np.asarray(x)).all()
    assert fw.weight_sum(s) == pytest.approx(float(s.astype(np.float64).sum()), rel=1e-15)


# ---- the Python mirrors -------------------------------------------------------------------------------------------------
class _Rec:
    """a recording stand-in for the context"""

    def __init__(self):
        self.calls = []

    def set_points(self, X):
        self.calls.append(("points", len(X)))
        return self

    def points_create(self, X):
        self.calls.append(("create", len(X)))
        return object()

    def points_bind(self, h):
        self.calls.append(("bind",))

    def points_destroy(self, h):
        pass

    def flat_set_weights(self, s):
        self.calls.append(("weights", None if s is None else [float(v) for v in s]))
        return self

    def synchronize(self):
        pass

    def flat_train(self, max_iter, tol, mu, cov, w, cov_type="diag", variant="W"):
        self.calls.append(("train", variant))
        return np.ones_like(cov), mu, w, cov, np.zeros(1, np.float32), True

    def flat_mstep(self, resp, cov_type, variant, centre_hint, device_out=False):
        self.calls.append(("mstep", variant))
        return None, None, None

    def flat_estep(self, inv, mu, w, cov_type, variant, lazy_mean=False):
        self.calls.append(("estep", variant))
        return 0.0, None, None, None


@pytest.fixture
def rec(monkeypatch):
    from hgmm_amd import _flat
    r = _Rec()
    monkeypatch.setattr(_flat, "default_context", lambda: r)
    return r


P20 = np.random.RandomState(1).rand(20, 3).astype(np.float32)
S20 = (np.arange(20.0) % 4).astype(np.float32)
MODEL = (P20[:3].copy(), np.full((3, 3), 0.1, np.float32), np.ones(3, np.float32) / 3)

BAD = {"length": np.ones(19), "negative": np.r_[np.ones(19), -1e-3], "nan": np.r_[np.ones(19), np.nan],
       "infinite": np.r_[np.ones(19), np.inf], "all zero": np.zeros(20), "shape": np.ones((20, 1))}


@pytest.mark.parametrize("what", sorted(BAD))
def test_mirrors_refuse_bad_sample_weights_before_touching_the_library(rec, what):
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm as Wg, gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    bad = BAD[what]
    mu, cov, w = MODEL
    for fn in (lambda: W.train_gmm(P20, 3, 0.0, mu, cov, w, sample_weight=bad),
               lambda: G.train_gmm(P20, 3, 0.0, mu, cov, w, sample_weight=bad),
               lambda: W.m_step(P20, np.ones((20, 3), np.float32), sample_weight=bad),
               lambda: W.e_step(P20, cov, mu, w, sample_weight=bad),
               lambda: _flat.DevicePoints(P20, weights=bad),
               lambda: _flat.asarray(P20, weights=bad),
               lambda: Wg.GMM_GPU_Base(3).fit(P20, init=(mu, w, cov), sample_weight=bad),
               lambda: Wg.GMM_GPU_Base(3).fit(WeightedPoints(P20, bad), init=(mu, w, cov))):
        rec.calls.clear()
        with pytest.raises(ValueError, match="sample_weight"):
            fn()
        assert rec.calls == [], rec.calls


def test_sample_weight_arguments():
    from hgmm_amd import Context, _flat
    from hgmm_amd.gmm_waymo import gmm as Wg, gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm as Gg, gmm_impl as G
    assert list(inspect.signature(Context.flat_set_weights).parameters) == ["self", "s"]
    for mod in (W, G):
        for name in ("train_gmm", "m_step", "e_step"):
            assert inspect.signature(getattr(mod, name)).parameters["sample_weight"].default is None, (mod, name)
    for name in ("train_gmm", "m_step", "e_step"):
        assert inspect.signature(getattr(_flat, name)).parameters["sample_weight"].default is None
    assert inspect.signature(_flat.DevicePoints.__init__).parameters["weights"].default is None
    assert inspect.signature(_flat.asarray).parameters["weights"].default is None
    for mod in (Wg, Gg):
        assert list(inspect.signature(mod.GMM_GPU_Base.fit).parameters) == ["self", "X", "init", "sample_weight"]
        assert list(inspect.signature(mod.GMM_GPU.compute).parameters) == ["self", "data", "weights"]
        assert inspect.signature(mod.GMM_GPU.compute).parameters["weights"].default is None


def test_mirrors_upload_the_cloud_before_its_weights(rec):
    """a host array: the cloud, then its weights (a new cloud drops the previous one's in the library), no weight call at all
    without weights; a resident cloud: bind, then the weights it carries (None takes a predecessor's off), an explicit
    sample_weight after them"""
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    mu, cov, w = MODEL
    s = list(map(float, S20))
    W.train_gmm(P20, 3, 0.0, mu, cov, w, sample_weight=S20)
    assert rec.calls == [("points", 20), ("weights", s), ("train", "W")]
    rec.calls.clear()
    G.train_gmm(P20, 3, 0.0, mu, cov, sample_weight=S20)
    assert rec.calls == [("points", 20), ("weights", s), ("train", "G")]
    rec.calls.clear()
    W.train_gmm(P20, 3, 0.0, mu, cov, w)
    assert rec.calls == [("points", 20), ("train", "W")]
    rec.calls.clear()
    W.m_step(P20, np.ones((20, 3), np.float32), sample_weight=S20)
    W.e_step(P20, cov, mu, w, sample_weight=S20)
    assert rec.calls == [("points", 20), ("weights", s), ("mstep", "W"), ("points", 20), ("weights", s), ("estep", "W")]
    rec.calls.clear()
    dp = _flat.DevicePoints(P20, weights=S20)
    assert _flat.asarray(dp) is dp and list(dp.weights) == s
    W.train_gmm(dp, 3, 0.0, mu, cov, w)
    assert rec.calls == [("create", 20), ("bind",), ("weights", s), ("train", "W")]
    rec.calls.clear()
    W.train_gmm(dp, 3, 0.0, mu, cov, w, sample_weight=np.ones(20))
    assert rec.calls == [("bind",), ("weights", s), ("weights", [1.0] * 20), ("train", "W")]
    rec.calls.clear()
    W.train_gmm(_flat.asarray(P20), 3, 0.0, mu, cov, w)
    assert rec.calls == [("create", 20), ("bind",), ("weights", None), ("train", "W")]
    assert list(_flat.asarray(dp, weights=np.ones(20)).weights) == [1.0] * 20


def test_weighted_points_bring_their_weights_to_fit_and_compute(rec, monkeypatch):
    from hgmm_amd.gmm_waymo import gmm as Wg
    from hgmm_amd.gmmreg_gpu import gmm as Gg
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    mu, cov, w = MODEL
    s = list(map(float, S20))
    monkeypatch.setattr(Gg, "init_gmm_params", lambda X, k: (mu, w))
    monkeypatch.setattr(Wg, "init_gmm_params", lambda X, k, cov_type="diag": (mu, w, cov))
    want = [("create", 20), ("bind",), ("weights", s), ("train", None)]
    for mod, variant in ((Wg, "W"), (Gg, "G")):
        want[-1] = ("train", variant)
        for fn in (lambda f: f.compute(WeightedPoints(P20, S20)),
                   lambda f: f.compute(P20, weights=S20),
                   lambda f: f.compute(WeightedPoints(P20, np.ones(20)), weights=S20),
                   lambda f: f._clf.fit(P20, sample_weight=S20),
                   lambda f: f._clf.fit(WeightedPoints(P20, S20))):
            rec.calls.clear()
            f = mod.GMM_GPU(n_gmm_components=3, max_iter=2)
            f.init()
            fn(f)
            assert rec.calls == want, (mod, rec.calls)
        rec.calls.clear()
        f = mod.GMM_GPU(n_gmm_components=3, max_iter=2)
        f.init()
        f.compute(P20)                                           # every earlier call: no weights
        assert rec.calls == [("create", 20), ("bind",), ("weights", None), ("train", variant)]


def test_entry_is_declared_exported_bound_and_documented():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    lib = hgmm_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    assert re.search(r"\bint hgmm_flat_set_weights\s*\(", header)
    assert len(lib.hgmm_flat_set_weights.argtypes) == 3
    doc = header[header.index("Per-point weights for the flat"):header.index("int hgmm_flat_set_weights(")]
    for word in ("M-step", "stop rule", "hgmm_flat_stats", "ZERO WEIGHT", "NaN", "bit for bit", "HGMM_ERR_STATE", "forest",
                 "per-handle ownership is out of scope", "KMeans", "communicator", "IGNORED"):
        assert word in doc, word
    assert "hgmm_flat_set_weights" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the two tree weight sections no longer claim that every flat entry is without weights of its own
    assert header.count("the flat fit") >= 2 and header.count("hgmm_flat_set_weights") >= 3
