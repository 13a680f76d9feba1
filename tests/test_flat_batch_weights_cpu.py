"""The host side of the weighted batched flat fit, without a GPU: the ``weights=`` / ``sample_weight=`` conventions of
``Context.flat_train_batch``, ``train_gmm_batch`` and ``fit_batch``, the precedence of explicit weights over a member's own,
the ``VoxelCloud`` rules, that nothing reaches the context when a check fails -- and the precondition of the GPU test on
members that stop at different iterations, against the float64 restatement it was chosen with."""
import ctypes as C

import numpy as np
import pytest

import _flat_weight_oracle as fw
from test_flat_batch_weights_gpu import STOPPERS, STOPPER_OFF, stopper


class _Untouchable:
    """Stands where the library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s)" % name)


class _Lib:
    """Records the entries a test reaches and returns HGMM_OK.  ``during``: called with the arguments while the call is in
    progress (the arrays behind its pointers live no longer than that); what it returns is kept in ``seen``."""

    def __init__(self, during=None):
        self.calls, self.seen, self.during = [], [], during

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if self.during:
                self.seen.append(self.during(*args))
            return 0
        return entry


def _context(lib=None):
    from hgmm_amd._native import Context
    c = Context.__new__(Context)              # no device: only the host-side checks and the marshalling can run
    c.lib = lib or _Untouchable()
    c.h = None
    return c


class _Points:
    """What the checks look at in a DevicePoints."""

    def __init__(self, ctx, weights=None, n=10):
        self.ctx, self.weights, self._h, self.shape = ctx, weights, C.c_void_p(0x1000), (n, 3)


def _model(J, B=1):
    return ([np.zeros((J, 3), np.float32) for _ in range(B)], [np.ones((J, 3), np.float32) for _ in range(B)],
            [np.full(J, 1.0 / J, np.float32) for _ in range(B)])


def _floats(address, n):
    return np.ctypeslib.as_array(C.cast(address, C.POINTER(C.c_float)), (n,)).copy()


def test_flat_train_batch_weights_keyword():
    lens = (10, 10, 0, 7)
    lib = _Lib(lambda *args: [None if args[3][b] is None else _floats(args[3][b], n).tolist() for b, n in enumerate(lens)])
    c = _context(lib)
    own = np.arange(1, 11, dtype=np.float32)
    explicit = np.full(10, 2.0)                                   # (float64: converted)
    clouds = [_Points(c, own), _Points(c, own), _Points(c), C.c_void_p(0x2000)]
    mu, cov, w = _model(4, 4)
    c.flat_train_batch(clouds, 3, 0.0, mu, cov, w, weights=[None, explicit, None, np.ones(7, np.float32)])
    (name, args), = lib.calls
    assert name == "hgmm_flat_train_batch_weighted" and args[1] == 4
    s, = lib.seen
    assert s[0] == own.tolist()                                   # None: the member's own
    assert s[1] == [2.0] * 10                                     # an explicit array takes precedence
    assert s[2] is None                                           # a member that brings none, None: unweighted
    assert s[3] == [1.0] * 7                                      # a bare handle: the array as it is
    # weights=None is today's entry, and today's refusal
    lib.calls.clear()
    lib.during = None
    c.flat_train_batch([_Points(c), C.c_void_p(0x2000)], 3, 0.0, mu[:2], cov[:2], w[:2])
    assert [n for n, _ in lib.calls] == ["hgmm_flat_train_batch"]
    with pytest.raises(ValueError, match="member 0 brings per-point weights"):
        c.flat_train_batch(clouds[:1], 3, 0.0, mu[:1], cov[:1], w[:1])


def test_flat_train_batch_weights_refusals_before_the_library():
    c = _context()
    mu, cov, w = _model(4, 2)
    good = [_Points(c), _Points(c)]
    with pytest.raises(ValueError, match="2 clouds, but 1 entries in weights"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, weights=[None])
    with pytest.raises(ValueError, match=r"member 1: weights must have shape \[10\], got \(9,\)"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, weights=[None, np.ones(9)])
    with pytest.raises(ValueError, match=r"member 0: weights must have shape"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, weights=[np.ones((10, 1)), None])
    bad = np.ones(10, np.float32)
    bad[7] = np.nan
    with pytest.raises(ValueError, match="member 1: weight 7 is nan"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, weights=[None, bad])
    bad[7] = -1
    with pytest.raises(ValueError, match="member 1: weight 7 is -1"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, weights=[None, bad])
    with pytest.raises(ValueError, match="member 0: all 10 weights are zero"):
        c.flat_train_batch(good, 3, 0.0, mu, cov, w, weights=[np.zeros(10), None])
    with pytest.raises(ValueError, match="member 1 has J = 5"):                 # the existing checks still run
        c.flat_train_batch(good, 3, 0.0, [mu[0], np.zeros((5, 3), np.float32)], cov, w, weights=[None, None])


class _Rec:
    """A recording stand-in for the context behind the mirrors."""

    def __init__(self):
        self.calls = []

    def points_create(self, X):
        self.calls.append(("create", len(X)))
        return C.c_void_p(0x3000 + len(self.calls))

    def points_destroy(self, h):
        self.calls.append(("destroy",))

    def flat_train_batch(self, clouds, max_iter, tol, mu, cov, w, cov_type="diag", variant="W", **kw):
        self.calls.append(("batch", [None if s is None else np.asarray(s).tolist() for s in kw["weights"]] if kw else None))
        return [(np.ones_like(c), m, ww, c, np.zeros(1, np.float32), True) for m, c, ww in zip(mu, cov, w)]

    def flat_train_batch_voxels(self, vcs, max_iter, tol, mu, cov, w, cov_type="diag", variant="W", weighted=True):
        self.calls.append(("voxels", [vc.index for vc in vcs], weighted, variant))
        return [(np.ones_like(c), m, ww, c, np.zeros(1, np.float32), True) for m, c, ww in zip(mu, cov, w)]

    def set_points_from_voxels(self, vc, tree_weights=True, flat_weights=False):
        self.calls.append(("from_voxels", vc.index, tree_weights, flat_weights))

    def flat_train(self, max_iter, tol, mu, cov, w, cov_type="diag", variant="W"):
        self.calls.append(("train", len(mu)))
        return np.ones_like(cov), mu, w, cov, np.zeros(1, np.float32), True


@pytest.fixture
def rec(monkeypatch):
    from hgmm_amd import _flat
    r = _Rec()
    monkeypatch.setattr(_flat, "default_context", lambda: r)
    return r


P = [np.random.RandomState(i).rand(20 + i, 3).astype(np.float32) for i in range(3)]
S = [np.arange(1, len(X) + 1, dtype=np.float32) for X in P]


def test_train_gmm_batch_sample_weight_conventions(rec):
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    mu, cov, w = _model(4, 3)
    dev = _flat.DevicePoints(P[0], rec, weights=S[0])
    members = [dev, WeightedPoints(P[1], S[1]), P[2]]
    for mod, args in ((W, (mu, cov, w)), (G, (mu, cov))):
        rec.calls.clear()
        out = mod.train_gmm_batch(members, 3, 0.0, *args, sample_weight="own")
        assert rec.calls == [("create", 21), ("create", 22), ("batch", [S[0].tolist(), S[1].tolist(), None]),
                             ("destroy",), ("destroy",)]
        assert len(out) == 3 and all(len(t) == 5 for t in out)
    # a sequence: the explicit array takes precedence, None is the member's own
    rec.calls.clear()
    W.train_gmm_batch(members, 3, 0.0, mu, cov, w, sample_weight=[2 * S[0], None, S[2]])
    assert rec.calls[2] == ("batch", [(2 * S[0]).tolist(), S[1].tolist(), S[2].tolist()])
    # the default: today's call (no keyword reaches the context) and today's refusal
    rec.calls.clear()
    W.train_gmm_batch(P, 3, 0.0, mu, cov, w)
    assert ("batch", None) in rec.calls
    rec.calls.clear()
    with pytest.raises(ValueError, match="member 0 brings per-point weights"):
        W.train_gmm_batch(members, 3, 0.0, mu, cov, w)
    # what fails a check reaches nothing
    with pytest.raises(ValueError, match="3 clouds, but 2 entries in sample_weight"):
        W.train_gmm_batch(members, 3, 0.0, mu, cov, w, sample_weight=[None, None])
    with pytest.raises(ValueError, match=r"member 2: sample_weight must have shape \[22\]"):
        W.train_gmm_batch(members, 3, 0.0, mu, cov, w, sample_weight=[None, None, np.ones(21)])
    with pytest.raises(ValueError, match=r"member 1: sample_weight\[3\] is -1"):
        W.train_gmm_batch(members, 3, 0.0, mu, cov, w, sample_weight=[None, np.where(np.arange(21) == 3, -1.0, 1.0), None])
    with pytest.raises(ValueError, match="must be None, 'own' or a sequence"):
        W.train_gmm_batch(members, 3, 0.0, mu, cov, w, sample_weight="counts")
    assert not rec.calls


def test_above_1024_components_the_weighted_mirror_loops_over_train_gmm(rec, monkeypatch):
    from hgmm_amd import _flat
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    seen = []
    monkeypatch.setattr(_flat, "train_gmm", lambda X, *a, sample_weight="absent": seen.append((len(X), sample_weight)) or "fit")
    mu, cov, w = _model(1025, 2)
    assert W.train_gmm_batch([WeightedPoints(P[0], S[0]), P[1]], 2, 0.0, mu, cov, w, sample_weight="own") == ["fit", "fit"]
    assert seen[0][0] == 20 and seen[0][1].tolist() == S[0].tolist() and seen[1] == (21, None)
    assert not rec.calls


class _Result:
    def __init__(self, ctx, m):
        self.ctx, self.m, self.n = ctx, m, [10 * v for v in m]
        self.downloads = 0

    def check(self, ctx=None):
        pass

    def get(self):
        self.downloads += 1
        return [(np.random.RandomState(k).rand(m, 3), np.full(m, 10, np.int64)) for k, m in enumerate(self.m)]


def _voxel_clouds(ctx, m=(30, 40, 50)):
    from hgmm_amd._native import VoxelCloud
    result = _Result(ctx, list(m))
    return result, [VoxelCloud(result, k) for k in range(len(m))]


def test_voxel_clouds_go_to_the_voxel_entry(rec):
    from hgmm_amd.gmm_waymo import gmm_impl as W
    from hgmm_amd.gmmreg_gpu import gmm_impl as G
    _, vcs = _voxel_clouds(rec)
    mu, cov, w = _model(4, 3)
    for sample_weight in (None, "own", [None, None, None]):
        rec.calls.clear()
        out = W.train_gmm_batch([vcs[2], vcs[0], vcs[0]], 3, 0.0, mu, cov, w, sample_weight=sample_weight)
        assert rec.calls == [("voxels", [2, 0, 0], True, "W")] and len(out) == 3           # count-weighted, whatever it says
    rec.calls.clear()
    G.train_gmm_batch(vcs, 3, 0.0, mu, cov)
    assert rec.calls == [("voxels", [0, 1, 2], True, "G")]
    rec.calls.clear()
    with pytest.raises(ValueError, match="member 1 is a VoxelCloud.*no explicit sample_weight"):
        W.train_gmm_batch(vcs, 3, 0.0, mu, cov, w, sample_weight=[None, np.ones(40), None])
    with pytest.raises(ValueError, match=r"VoxelClouds and other members in one batch \(2 of 3"):
        W.train_gmm_batch([vcs[0], P[0], vcs[1]], 3, 0.0, mu, cov, w)
    with pytest.raises(ValueError, match=r"VoxelClouds and other members"):
        W.train_gmm_batch([vcs[0], P[0], vcs[1]], 3, 0.0, mu, cov, w, sample_weight="own")
    _, foreign = _voxel_clouds(_Rec())
    with pytest.raises(ValueError, match="member 1 is a cloud of another context"):
        W.train_gmm_batch([vcs[0], foreign[0], vcs[1]], 3, 0.0, mu, cov, w)
    assert not rec.calls
    # J = 1025: set_points_from_voxels with the counts as flat weights, then the serial fit, member by member
    mu, cov, w = _model(1025, 2)
    W.train_gmm_batch(vcs[:2], 2, 0.0, mu, cov, w)
    assert rec.calls == [("from_voxels", 0, False, True), ("train", 1025), ("from_voxels", 1, False, True), ("train", 1025)]


def test_flat_train_batch_voxels_checks_before_the_library():
    from hgmm_amd._native import HgmmError
    lib = _Lib()
    c = _context(lib)
    _, vcs = _voxel_clouds(c)
    mu, cov, w = _model(4, 2)
    c.flat_train_batch_voxels([vcs[2], vcs[0]], 3, 0.0, mu, cov, w, weighted=False)
    (name, args), = lib.calls
    assert name == "hgmm_flat_train_batch_voxels" and args[1] == 2 and list(args[2]) == [2, 0] and args[3] == 0
    lib.calls.clear()
    with pytest.raises(TypeError, match="takes VoxelClouds"):
        c.flat_train_batch_voxels([vcs[0], P[0]], 3, 0.0, mu, cov, w)
    with pytest.raises(ValueError, match="no clouds"):
        c.flat_train_batch_voxels([], 3, 0.0, [], [], [])
    with pytest.raises(ValueError, match="2 clouds, but 1 arrays in mu"):
        c.flat_train_batch_voxels(vcs[:2], 3, 0.0, mu[:1], cov, w)
    vcs[1].result.check = lambda ctx=None: (_ for _ in ()).throw(HgmmError("stale voxel result"))
    with pytest.raises(HgmmError, match="stale"):
        c.flat_train_batch_voxels(vcs[:2], 3, 0.0, mu, cov, w)
    assert not lib.calls


def test_fit_batch_conventions(monkeypatch):
    from hgmm_amd.gmm_waymo import gmm as Wg
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints
    passed = {}

    def fake(Xs, max_iter, tol, means, covariances, weights, cov_type="diag", **kw):
        passed.update(Xs=Xs, kw=kw)
        return [(np.ones_like(c), m, w, c, [np.float32(0)]) for m, c, w in zip(means, covariances, weights)]

    monkeypatch.setattr(Wg, "train_gmm_batch", fake)
    monkeypatch.setattr(Wg, "timer", lambda *a, **k: __import__("contextlib").nullcontext())

    class Quiet(Wg.GMM_GPU_Base):
        _verbose = False

    est = Quiet(6, max_iter=7, tol=1e-3)
    frames = [WeightedPoints(P[0].astype(np.float64), S[0]), P[1]]
    with pytest.raises(ValueError, match="frame 0 brings per-point weights"):
        est.fit_batch(frames)                                                  # the default still refuses
    est.fit_batch(frames, sample_weight="own")
    assert passed["kw"] == {"sample_weight": "own"}
    assert passed["Xs"][0].weights is S[0] and passed["Xs"][0].points.dtype == np.float32      # the weights travel on
    assert passed["Xs"][1].weights is None and passed["Xs"][1].points.tobytes() == P[1].tobytes()
    est.fit_batch([P[0], P[1]])
    assert passed["kw"] == {} and passed["Xs"][1].tobytes() == P[1].tobytes()   # no keyword where none was given
    # VoxelClouds: without inits ONE download, the initialiser samples the host centroids frame by frame; with inits none
    result, vcs = _voxel_clouds(object())
    np.random.seed(5)
    want = [Wg.init_gmm_params(cent, 6, cov_type="diag") for cent, _ in result.get()]
    result.downloads = 0
    np.random.seed(5)
    models = est.fit_batch(vcs)
    assert result.downloads == 1 and passed["Xs"] == vcs and passed["kw"] == {}
    for m, (mu, _, _) in zip(models, want):
        assert m.means_.tobytes() == np.asarray(mu, np.float32).tobytes()
    result.downloads = 0
    est.fit_batch(vcs, inits=want)
    assert result.downloads == 0
    with pytest.raises(ValueError, match="frame 2 is a VoxelCloud"):
        est.fit_batch(vcs, sample_weight=[None, None, np.ones(50)])
    with pytest.raises(ValueError, match=r"VoxelClouds and other frames in one batch \(1 of 2"):
        est.fit_batch([vcs[0], P[0]])


class _Pool:
    """A stand-in pool: every job on one recording context, results in job order."""

    def __init__(self, ctx):
        self.ctx, self.jobs = ctx, None

    def map(self, fn, jobs):
        self.jobs = list(jobs)
        return [fn(self.ctx, job) for job in self.jobs]


class _VoxelCtx:
    def __init__(self):
        self.calls = []

    def voxel_down_sample_batch(self, clouds, voxel_size, download=True):
        self.calls.append((list(clouds), voxel_size, download))

        class R:
            def members(_):
                return ["vc%d" % f for f in clouds]
        return R()


def test_fit_frames_down_samples_every_chunk_on_its_context(monkeypatch):
    from hgmm_amd import replicas
    from hgmm_amd.gmm_waymo.gmm import GMM_GPU_Base
    monkeypatch.setattr(GMM_GPU_Base, "fit_batch", lambda self, frames, inits=None: ["model:" + f for f in frames])
    monkeypatch.setattr(GMM_GPU_Base, "fit", lambda self, frame, **k: "plain%d" % frame)
    c = _VoxelCtx()
    pool = _Pool(c)
    want = ["model:vc%d" % f for f in range(9)]
    assert replicas.fit_frames(range(9), pool=pool, batch=4, voxel_size=0.25) == want
    assert c.calls == [([0, 1, 2, 3], 0.25, False), ([4, 5, 6, 7], 0.25, False), ([8], 0.25, False)]
    c.calls.clear()
    assert replicas.fit_frames(range(3), pool=pool, voxel_size=0.25) == want[:3]              # batch=1: chunks of one
    assert c.calls == [([0], 0.25, False), ([1], 0.25, False), ([2], 0.25, False)]
    c.calls.clear()
    assert replicas.fit_frames(range(2), pool=pool) == ["plain0", "plain1"] and not c.calls   # no voxel_size: as before


def test_the_weighted_stopper_clouds_stop_where_they_were_chosen_to():
    """The recipe of test_flat_batch_weights_gpu.py::test_members_that_stop_at_different_iterations against the float64
    restatement it was chosen with: 5, 9, 13 and 16 iterations, every deciding change clear of tol on either side."""
    f64 = lambda a: np.asarray(a, np.float64)
    its, last, before = [], [], []
    for spec, off in zip(STOPPERS, STOPPER_OFF):
        X, s, p = stopper(*spec, off=off)
        o = fw.train(f64(X), s, 40, 1e-3, f64(p[0]), f64(p[1]), f64(p[2]), "diag", "W")
        assert o[5]
        lls = np.asarray(o[4], np.float64)
        its.append(len(lls))
        d = np.abs(np.diff(lls)) / 1e-3
        last.append(d[-1])
        before.append(d[-2])
    print("iterations", its, "deciding change / tol", last, "the one before / tol", before)
    assert its == [5, 9, 13, 16]
    assert max(last) < 0.85 and min(before) > 1.25
