"""Multi-start registration, the parts that need no GPU: the two C entries are declared, exported and bound; the grid of
start poses; the winner rule; the public signatures."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    return hgmm_amd.load_library()


def declared_arguments(name):
    txt = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, "%s is not declared in include/hgmm.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("hgmm_tree_register_multi", 12), ("hgmm_tree_score_multi", 8)])
def test_entries_are_declared_exported_and_bound(lib, name, n_args):
    args = declared_arguments(name)
    assert len(args) == n_args, args
    assert args[0].startswith("hgmm_ctx*") and args[1] == "int K"
    fn = getattr(lib, name)                                  # exported
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    comments = "".join(re.findall(r"/\*.*?\*/", header, flags=re.S))
    assert name in comments, "%s has no entry in the header comment" % name
    from hgmm_amd import Context
    assert callable(getattr(Context, name[len("hgmm_"):]))


def test_rotation_starts_default_grid():
    from hgmm_amd.hgmm.hgmm_gpu import RigidTransformation, euler_matrix_xyz, rotation_starts
    starts = rotation_starts()
    assert len(starts) == 27 and all(isinstance(s, RigidTransformation) for s in starts)
    assert np.array_equal(starts[13].rot, np.identity(3)) and np.array_equal(starts[13].t, np.zeros(3))
    assert starts[13].scale == 1.0
    for s, (ax, ay, az) in zip(starts, itertools.product((-15, 0, 15), repeat=3)):
        assert np.abs(s.rot @ s.rot.T - np.identity(3)).max() <= 1e-15
        assert abs(np.linalg.det(s.rot) - 1.0) <= 1e-15
        assert np.array_equal(s.t, np.zeros(3))             # about the origin
        # Rz(az) Ry(ay) Rx(ax), itertools.product order over (ax, ay, az)
        assert np.array_equal(s.rot, euler_matrix_xyz(*np.deg2rad([float(ax), float(ay), float(az)])))
    # the last index turns fastest about z: index 14 = (0, 0, +15) is a pure rotation about z
    th = np.deg2rad(15.0)
    np.testing.assert_allclose(starts[14].rot, [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], atol=1e-16)


def test_rotation_starts_about_a_centre_leave_it_fixed():
    from hgmm_amd.hgmm.hgmm_gpu import rotation_starts
    c = np.array([0.3, -1.25, 40.0])
    starts = rotation_starts((-20, 5), centre=c)
    assert len(starts) == 8
    origin = rotation_starts((-20, 5))
    for s, o in zip(starts, origin):
        assert np.array_equal(s.rot, o.rot)
        # |c| = 40: one rounding of R c and one of c - R c, each below 2^-53 * 64
        assert np.abs(s.transform(c[None])[0] - c).max() <= 64 * 2.0 ** -52
    assert rotation_starts((0,), centre=c)[0].t.tolist() == [0.0, 0.0, 0.0]


def summary(n_in, maha, n=100.0):
    return [n, n_in, maha, 0.1, -3.0, 0.0, 0.0, 0.0]


def test_winner_rule():
    from hgmm_amd.hgmm.hgmm_gpu import best_hypothesis
    I, z = np.identity(3), np.zeros(3)
    rot, t = np.tile(I, (4, 1, 1)), np.tile(z, (4, 1))
    # most inliers
    assert best_hypothesis([summary(50, 9.0), summary(70, 99.0), summary(60, 1.0), summary(10, 0.1)], rot, t) == 1
    # the inlier tie: the smaller sum of squared Mahalanobis distances
    assert best_hypothesis([summary(70, 9.0), summary(70, 8.5), summary(60, 1.0), summary(70, 8.75)], rot, t) == 1
    # the summary[2] tie: the lower index
    assert best_hypothesis([summary(60, 1.0), summary(70, 8.5), summary(70, 8.5), summary(70, 8.5)], rot, t) == 1
    # a NaN pose loses, whatever its summary says -- in the rotation or in the translation
    bad = rot.copy()
    bad[1, 2, 2] = np.nan
    assert best_hypothesis([summary(50, 9.0), summary(99, 0.0), summary(60, 1.0), summary(10, 0.1)], bad, t) == 2
    bad_t = t.copy()
    bad_t[2, 0] = np.inf
    assert best_hypothesis([summary(50, 9.0), summary(99, 0.0), summary(60, 1.0), summary(10, 0.1)], bad, bad_t) == 0
    # no inliers anywhere: still an index, the lowest
    assert best_hypothesis([summary(0, 0.0)] * 4, rot, t) == 0
    assert best_hypothesis([summary(5, 2.0)], I[None], z[None]) == 0
    with pytest.raises(ValueError):
        best_hypothesis(np.zeros((0, 8)), np.zeros((0, 3, 3)), np.zeros((0, 3)))


def test_public_signatures():
    from hgmm_amd import Context
    from hgmm_amd.hgmm import hgmm_gpu
    p = inspect.signature(hgmm_gpu.registration_gmmtree).parameters
    assert list(p) == ["source", "target", "maxiter", "tol", "callbacks", "return_score", "starts", "kargs"]
    assert p["starts"].default is None and p["kargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert (p["maxiter"].default, p["tol"].default, p["return_score"].default) == (20, 1.0e-4, False)
    m = inspect.signature(hgmm_gpu.GMMTree.registration_multistart).parameters
    assert list(m) == ["self", "target", "starts", "maxiter", "tol", "maha2_max", "return_all"]
    assert (m["maxiter"].default, m["tol"].default, m["return_all"].default) == (20, 1.0e-4, False)
    assert m["maha2_max"].default == hgmm_gpu.CHI2_3_99
    r = inspect.signature(hgmm_gpu.rotation_starts).parameters
    assert r["angles_deg"].default == (-15, 0, 15) and r["centre"].default is None
    assert list(inspect.signature(Context.tree_register_multi).parameters)[1:] == \
        list(inspect.signature(Context.tree_register_batch).parameters)[1:]
    assert issubclass(hgmm_gpu.MultiStartResult, hgmm_gpu.ScoredResult)


def test_registration_multistart_host_logic_with_a_recording_context():
    """GMMTree.registration_multistart (host logic only, a recording stand-in for the context): ONE tree_register_multi and
    ONE tree_score_multi for all starts, a status-2 hypothesis finished through the serial entries BEFORE the scoring, the
    winner by the rule, per-point arrays from one serial tree_score at the winner's pose."""
    import contextlib
    from hgmm_amd.hgmm import hgmm_gpu as H

    class Recorder:
        def __init__(self):
            self.calls = []

        def tree_set_nodes(self, L, pi, mu, cov):
            self.calls.append(("nodes", L))

        def tree_set_target(self, target):
            self.n = len(target)
            self.calls.append(("target", len(target)))

        def config(self, **kw):
            self.calls.append(("config", kw))
            return contextlib.nullcontext()

        def tree_register_multi(self, rot, t, scale, lambda_c, maxiter, tol):
            K = len(rot)
            self.calls.append(("register_multi", K, maxiter))
            # hypothesis k "moves" by k along x in k + 1 iterations; hypothesis 2 leaves after one iteration at status 2
            t = t + np.arange(K)[:, None] * np.array([1.0, 0.0, 0.0])
            status = np.where(np.arange(K) == 2, 2, 1).astype(np.int32)
            iters = np.where(status == 2, 1, np.arange(K) + 1).astype(np.int32)
            return rot.copy(), t, iters, np.arange(K) + 0.5, status, None

        def tree_register(self, rot, t, scale, lambda_c, max_iter, tol, q_prev):
            self.calls.append(("register", max_iter, q_prev))
            return rot, t + np.array([0.0, 7.0, 0.0]), 2, 0.25, 1, None

        def tree_reg_estep(self, T, rot, t, scale, lambda_c):
            self.calls.append(("reg_estep", tuple(t)))
            m0 = np.full(T, 2.0)                      # every node has mass, its points a little off its mean: well-conditioned
            return m0, m0[:, None] * (MU + 0.01 * np.random.RandomState(4).randn(T, 3)), np.zeros((T, 3, 3))

        def tree_score_multi(self, rot, t, scale, lambda_c, maha2_max):
            self.calls.append(("score_multi", len(rot), t.copy()))
            s = np.zeros((len(rot), 8))
            s[:, 0] = self.n
            s[:, 1] = [10, 40, 40, 5][:len(rot)]
            s[:, 2] = [1.0, 9.0, 3.0, 1.0][:len(rot)]
            return s

        def tree_score(self, rot, t, scale, lambda_c, maha2_max, want):
            self.calls.append(("score", tuple(want), tuple(t)))
            s = np.array([self.n, 40, 3.0, 0.4, -80.0, 0, 0, 0], dtype=np.float64)
            return s, {w: np.zeros(self.n) for w in want}

    T = 8
    rs = np.random.RandomState(3)
    cov = np.tile(np.identity(3), (T, 1, 1)) * 0.01
    MU = rs.rand(T, 3)
    ctx = Recorder()
    gt = H.GMMTree(None, tree_level=1, ctx=ctx)
    gt.set_nodes(np.full(T, 1.0 / T), MU, cov)
    starts = [H.RigidTransformation(np.identity(3), np.array([0.0, 0.0, float(k)])) for k in range(4)]
    win, every = gt.registration_multistart(rs.rand(50, 3), starts, maxiter=9, tol=1e-3, return_all=True)
    names = [c[0] for c in ctx.calls]
    assert names.count("register_multi") == 1 and names.count("score_multi") == 1 and names.count("score") == 1
    assert names.index("register_multi") < names.index("reg_estep") < names.index("register") < names.index("score_multi")
    assert ("register_multi", 4, 9) in ctx.calls and not any(c[0] == "config" for c in ctx.calls)
    # hypothesis 2: one iteration in the multi call, one on the host (stacked least squares), then the serial entry with the
    # rest of the budget and the host step's q; what is scored is the pose it ended at
    reg = [c for c in ctx.calls if c[0] == "register"]
    assert len(reg) == 1 and reg[0][1] == 9 - 2 and reg[0][2] is not None
    scored_t = [c for c in ctx.calls if c[0] == "score_multi"][0][2]
    assert scored_t[1].tolist() == [1.0, 0.0, 1.0] and scored_t[2][1] > 6.0
    # 40 inliers twice: the smaller summary[2] wins -- hypothesis 2, which took 1 + 1 + 2 iterations
    assert win.best_index_ == 2 and win.n_iter_ == 4 and gt.best_index_ == 2 and gt.n_iter_ == 4
    assert every[2] is win and len(every) == 4
    assert win.score.node is not None and all(e.score.node is None for k, e in enumerate(every) if k != 2)
    assert [e.score.n_inliers for e in every] == [10, 40, 40, 5]
    assert [c for c in ctx.calls if c[0] == "score"][0][2] == tuple(scored_t[2])
    # what comes back is the inverse of the loop's pose, as registration() returns it
    assert np.allclose(every[1].transformation.t, -np.array([1.0, 0.0, 1.0])) and float(every[1].q[0]) == 1.5
    # solve_on_device: the per-context option for the multi call
    ctx2 = Recorder()
    gt2 = H.GMMTree(None, tree_level=1, ctx=ctx2, solve_on_device=True)
    gt2.set_nodes(np.full(T, 1.0 / T), rs.rand(T, 3), cov)
    assert gt2.registration_multistart(rs.rand(50, 3), starts[:2]).best_index_ == 1
    assert ("config", {"reg_device_solve": 1}) in ctx2.calls
    with pytest.raises(ValueError):
        gt.registration_multistart(rs.rand(50, 3), [])
    with pytest.raises(ValueError):
        gt.registration_multistart(rs.rand(50, 3), [starts[0], H.RigidTransformation(np.identity(3), np.zeros(3), 2.0)])
