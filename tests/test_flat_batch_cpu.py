"""The host side of the batched flat fit, without a GPU and without a library call that needs one: what
``Context.flat_train_batch`` and ``train_gmm_batch`` refuse before the library is reached, how ``fit_frames(batch=)`` cuts the
frames into chunks, and the order in which ``fit_batch`` draws its initial parameters."""
import ctypes as C

import numpy as np
import pytest


class _Untouchable:
    """Stands where the library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s)" % name)


def _context():
    from hgmm_amd._native import Context
    c = Context.__new__(Context)              # no device, no library: only the host-side checks can run
    c.lib = _Untouchable()
    c.h = None
    return c


class _Points:
    """What the checks look at in a DevicePoints."""

    def __init__(self, ctx, weights=None, n=10):
        self.ctx, self.weights, self._h, self.shape = ctx, weights, C.c_void_p(0x1000), (n, 3)


def _model(J, B=1, cov_type="diag"):
    mu = [np.zeros((J, 3), np.float32) for _ in range(B)]
    cov = [np.ones((J, 3) if cov_type == "diag" else (J,), np.float32) for _ in range(B)]
    w = [np.full(J, 1.0 / J, np.float32) for _ in range(B)]
    return mu, cov, w


def test_flat_train_batch_refuses_before_the_library():
    c, other = _context(), _context()
    good = [_Points(c), C.c_void_p(0x2000)]
    mu, cov, w = _model(4, 2)
    with pytest.raises(ValueError, match="2 clouds, but 3 arrays in mu"):
        c.flat_train_batch(good, 3, 0.0, mu + mu[:1], cov, w)
    with pytest.raises(ValueError, match="2 clouds, but 1 arrays in w"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w[:1])
    with pytest.raises(ValueError, match=r"member 1: means must be \[J,3\]"):
        c.flat_train_batch(good, 3, 0.0, [mu[0], np.zeros((4, 2), np.float32)], cov, w)
    with pytest.raises(ValueError, match="member 1 has J = 5, member 0 has J = 4"):
        c.flat_train_batch(good, 3, 0.0, [mu[0], np.zeros((5, 3), np.float32)], cov, w)
    with pytest.raises(ValueError, match="member 0: expected shape"):
        c.flat_train_batch(good, 3, 0.0, mu, [np.ones(4, np.float32), cov[1]], w)          # spherical cov, diag fit
    with pytest.raises(ValueError, match="member 1 is a cloud of another context"):
        c.flat_train_batch([_Points(c), _Points(other)], 3, 0.0, mu, cov, w)
    with pytest.raises(ValueError, match="member 1 brings per-point weights"):
        c.flat_train_batch([_Points(c), _Points(c, np.ones(10, np.float32))], 3, 0.0, mu, cov, w)
    with pytest.raises(ValueError, match="member 0 is neither"):
        c.flat_train_batch([object(), _Points(c)], 3, 0.0, mu, cov, w)
    with pytest.raises(ValueError, match="no clouds"):
        c.flat_train_batch([], 3, 0.0, [], [], [])
    with pytest.raises(ValueError, match="cov_type"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, cov_type="full")
    # stacked arrays are sequences too; what passes the checks comes out stacked, member-major
    hs, J, m, cv, ww = c._flat_batch_args(good, np.stack(mu), np.stack(cov), np.stack(w), "diag")
    assert J == 4 and m.shape == (2, 4, 3) and cv.shape == (2, 4, 3) and ww.shape == (2, 4) and len(hs) == 2
    assert m.dtype == cv.dtype == ww.dtype == np.float32 and hs[0].value == 0x1000 and hs[1].value == 0x2000


class _Rec:
    """A recording stand-in for the context behind the mirrors."""

    def __init__(self):
        self.calls = []

    def points_create(self, X):
        self.calls.append(("create", len(X)))
        return C.c_void_p(0x3000 + len(self.calls))

    def points_destroy(self, h):
        self.calls.append(("destroy",))

    def flat_train(self, *a, **k):
        raise AssertionError("the serial fit was reached")

    def flat_train_batch(self, clouds, max_iter, tol, mu, cov, w, cov_type="diag", variant="W"):
        self.calls.append(("batch", len(clouds), variant, cov_type))
        return [(np.ones_like(c), m, ww, c, np.zeros(1, np.float32), True) for m, c, ww in zip(mu, cov, w)]


@pytest.fixture
def rec(monkeypatch):
    from hgmm_amd import _flat
    r = _Rec()
    monkeypatch.setattr(_flat, "default_context", lambda: r)
    return r


P = [np.random.RandomState(i).rand(20 + i, 3).astype(np.float32) for i in range(3)]


def test_train_gmm_batch_refuses_before_the_context(rec):
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    mu, cov, w = _model(4, 3)
    for mod in (W, G):
        with pytest.raises(ValueError, match="3 clouds, but 2 arrays in means"):
            mod.train_gmm_batch(P, 3, 0.0, mu[:2], cov, w)
        with pytest.raises(ValueError, match=r"member 2: means must be \[J,3\]"):
            mod.train_gmm_batch(P, 3, 0.0, [mu[0], mu[1], np.zeros(4, np.float32)], cov, w)
        with pytest.raises(ValueError, match="member 1 has J = 6, member 0 has J = 4"):
            mod.train_gmm_batch(P, 3, 0.0, [mu[0], np.zeros((6, 3), np.float32), mu[2]], cov, w)
        with pytest.raises(ValueError, match="member 2 brings per-point weights"):
            mod.train_gmm_batch([P[0], P[1], WeightedPoints(P[2], np.ones(len(P[2]), np.float32))], 3, 0.0, mu, cov, w)
        with pytest.raises(ValueError, match=r"member 1: points must have shape \[N,3\]"):
            mod.train_gmm_batch([P[0], np.zeros((5, 2), np.float32), P[2]], 3, 0.0, mu, cov, w)
    a = _flat.DevicePoints(P[0], rec)
    other = _Rec()
    b = _flat.DevicePoints(P[1], other)
    with pytest.raises(ValueError, match="member 1 is a cloud of another context"):
        W.train_gmm_batch([a, b, P[2]], 3, 0.0, mu, cov, w)
    weighted = _flat.DevicePoints(P[1], rec, weights=np.ones(len(P[1]), np.float32))
    with pytest.raises(ValueError, match="member 1 brings per-point weights"):
        W.train_gmm_batch([a, weighted, P[2]], 3, 0.0, mu, cov, w)
    assert not [c for c in rec.calls if c[0] == "batch"]            # nothing of the above reached the context's fit


def test_train_gmm_batch_uploads_host_members_and_frees_them(rec):
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    mu, cov, w = _model(4, 3)
    resident = _flat.DevicePoints(P[1], rec)
    rec.calls.clear()
    out = W.train_gmm_batch([P[0], resident, P[2]], 3, 0.0, mu, cov, w, cov_type="diag")
    assert rec.calls == [("create", 20), ("create", 22), ("batch", 3, "W", "diag"), ("destroy",), ("destroy",)]
    assert len(out) == 3 and all(len(t) == 5 and isinstance(t[4], list) for t in out)       # train_gmm's tuples
    assert resident._h is not None                                                         # used where it is, not freed
    rec.calls.clear()
    out = G.train_gmm_batch([P[0]], 3, 0.0, mu[:1], cov[:1])                                # weights=None: uniform
    assert rec.calls[1] == ("batch", 1, "G", "diag") and np.allclose(out[0][2], 0.25)
    assert W.train_gmm_batch([], 3, 0.0, [], [], []) == []


def test_above_1024_components_the_mirror_loops_over_train_gmm(rec, monkeypatch):
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm_impl as W
    seen = []
    monkeypatch.setattr(_flat, "train_gmm", lambda X, *a: seen.append(len(X)) or "fit%d" % len(seen))
    mu, cov, w = _model(1025, 2)
    assert W.train_gmm_batch(P[:2], 2, 0.0, mu, cov, w) == ["fit1", "fit2"] and seen == [20, 21]
    assert not rec.calls


class _Pool:
    """A stand-in pool that hands the jobs out in REVERSE and returns the results in job order, like ReplicaPool.map."""

    def __init__(self):
        self.jobs = None

    def map(self, fn, jobs):
        self.jobs = list(jobs)
        done = {k: fn(None, job) for k, job in reversed(list(enumerate(self.jobs)))}
        return [done[k] for k in range(len(self.jobs))]

    def close(self):
        raise AssertionError("a pool the caller brought is the caller's to close")


def test_fit_frames_chunks_keep_the_frame_order(monkeypatch):
    from hgmm_amd import replicas
    from hgmm_amd.gmm_waymo.gmm import GMM_GPU_Base
    monkeypatch.setattr(GMM_GPU_Base, "fit_batch", lambda self, frames, inits=None: ["model%d" % f for f in frames])
    monkeypatch.setattr(GMM_GPU_Base, "fit", lambda self, frame, **k: "model%d" % frame)
    pool = _Pool()
    want = ["model%d" % f for f in range(9)]
    assert replicas.fit_frames(range(9), pool=pool, batch=4) == want
    assert pool.jobs == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]                    # a short last chunk
    assert replicas.fit_frames(range(9), pool=pool, batch=1) == want and pool.jobs == list(range(9))
    assert replicas.fit_frames(range(9), pool=pool) == want and pool.jobs == list(range(9))
    assert replicas.fit_frames(range(3), pool=pool, batch=16) == want[:3] and pool.jobs == [[0, 1, 2]]
    assert replicas.fit_frames([], pool=pool, batch=4) == [] and pool.jobs == []
    with pytest.raises(ValueError, match="batch must be >= 1"):
        replicas.fit_frames(range(3), pool=pool, batch=0)


def test_fit_batch_draws_its_initial_parameters_frame_by_frame(monkeypatch):
    """A loop of ``.fit`` draws frame 0's parameters, fits (the fit draws nothing), draws frame 1's ...: fit_batch must consume
    the host RNG in exactly that order, before the one batched fit."""
    from hgmm_amd.gmm_waymo import gmm as Wg
    from hgmm_amd.gmm_waymo.gmm_impl import init_gmm_params
    frames = [np.random.RandomState(50 + i).rand(30 + i, 3) for i in range(5)]          # float64 host frames, like a reader's
    np.random.seed(11)
    want = [init_gmm_params(X, 6, cov_type="spherical") for X in frames]
    passed = {}

    def fake(Xs, max_iter, tol, means, covariances, weights, cov_type="diag"):
        passed.update(Xs=Xs, means=means, covs=covariances, weights=weights, cov_type=cov_type, args=(max_iter, tol))
        return [(np.ones_like(c), m, w, c, [np.float32(0)]) for m, c, w in zip(means, covariances, weights)]

    monkeypatch.setattr(Wg, "train_gmm_batch", fake)
    monkeypatch.setattr(Wg, "timer", lambda *a, **k: __import__("contextlib").nullcontext())
    class Quiet(Wg.GMM_GPU_Base):                                         # (a subclass: the models are of the caller's type)
        _verbose = False

    est = Quiet(6, max_iter=7, tol=1e-3, cov_type="spherical")
    np.random.seed(11)
    models = est.fit_batch(frames)
    assert passed["cov_type"] == "spherical" and passed["args"] == (7, 1e-3) and len(models) == 5
    for b, (mu, w, cov) in enumerate(want):
        assert passed["means"][b].tobytes() == mu.tobytes() and passed["means"][b].dtype == np.float32
        assert passed["weights"][b].tobytes() == w.tobytes() and passed["covs"][b].tobytes() == cov.tobytes()
        assert passed["Xs"][b].dtype == np.float32 and passed["Xs"][b].tobytes() == frames[b].astype(np.float32).tobytes()
        m = models[b]
        assert type(m) is Quiet and m is not est and m.means_.tobytes() == mu.tobytes()
        assert (m.num_components, m.max_iter, m.tol, m.cov_type) == (6, 7, 1e-3, "spherical") and len(m.lls) == 1
    assert not hasattr(est, "means_")                                     # the estimator the batch was called on stays as it is
    # explicit initialisations draw nothing
    state = np.random.get_state()[1].copy()
    est.fit_batch(frames[:2], inits=want[:2])
    assert (np.random.get_state()[1] == state).all()
    with pytest.raises(ValueError, match="2 frames, but 1 initialisations"):
        est.fit_batch(frames[:2], inits=want[:1])
