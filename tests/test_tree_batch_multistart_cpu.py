"""Batched multi-start, the parts that need no GPU: the two C entries are declared, exported and bound; the round planner;
what registration_gmmtree_batch(starts=) refuses before it reaches the device; the per-pair winner selection over stubbed
native calls; starts=None reaches none of the new calls."""
import contextlib
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_tree_multistart_cpu import declared_arguments, summary


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import hgmm_amd
    return hgmm_amd.load_library()


@pytest.mark.parametrize("name,n_args", [("hgmm_tree_register_batch_multi", 13), ("hgmm_tree_score_batch_multi", 9)])
def test_entries_are_declared_exported_and_bound(lib, name, n_args):
    args = declared_arguments(name)
    assert len(args) == n_args, args
    assert args[0].startswith("hgmm_ctx*") and args[1] == "int R" and args[2] == "const int32_t* pair"
    assert args[3] == ("double* rot" if "register" in name else "const double* rot")
    fn = getattr(lib, name)                                  # exported
    assert fn.argtypes is not None and len(fn.argtypes) == n_args
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    comments = "".join(re.findall(r"/\*.*?\*/", header, flags=re.S))
    assert name in comments, "%s has no entry in the header comment" % name
    # ... which says what the entry replaces
    at = comments.index(name + " <-")
    assert "replacing" in comments[at:at + 400]
    from hgmm_amd import Context
    assert callable(getattr(Context, name[len("hgmm_"):]))


def test_the_cap_is_the_header_s():
    from hgmm_amd import _native
    header = open(os.path.join(ROOT, "include", "hgmm.h")).read()
    m = re.search(r"#define\s+HGMM_TREE_BATCH_MULTI_MAX_BYTES\s+(\d+)ull", header)
    assert m and int(m.group(1)) == _native.BATCH_MULTI_MAX_BYTES == 4 << 30


def test_public_signatures():
    from hgmm_amd import Context
    from hgmm_amd.hgmm import hgmm_gpu
    p = inspect.signature(hgmm_gpu.registration_gmmtree_batch).parameters
    assert list(p) == ["pairs", "maxiter", "tol", "ctx", "tree_level", "lambda_c", "ls", "ld", "sig2", "init_idx", "return_info",
                       "pdf_dtype", "solve_on_device", "score", "maha2_gate", "target_weights", "source_weights", "voxel_size",
                       "starts", "maha2_max"]
    assert p["starts"].default is None and p["maha2_max"].default == hgmm_gpu.CHI2_3_99
    r = list(inspect.signature(Context.tree_register_batch_multi).parameters)
    assert r[1] == "pair" and r[2:] == list(inspect.signature(Context.tree_register_multi).parameters)[1:]
    s = list(inspect.signature(Context.tree_score_batch_multi).parameters)
    assert s[1] == "pair" and s[2:] == list(inspect.signature(Context.tree_score_multi).parameters)[1:]


# ---- the round planner ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,owners,cap", [(72, [2, 1, 0, 1, 2, 1, 1, 2, 1], 4 * 32 * 72), (72, [0] * 9, 9 * 32 * 72),
                                          (72, [0] * 9, 9 * 32 * 72 - 1), (37448, list(range(32)) * 27, None),
                                          (299592, list(range(32)) * 27, None), (8, [], None), (72, [5], 32 * 72)])
def test_round_planner(T, owners, cap):
    from hgmm_amd._native import BATCH_MULTI_MAX_BYTES, plan_batch_multi_rounds
    rounds = plan_batch_multi_rounds(T, owners, cap)
    cap = BATCH_MULTI_MAX_BYTES if cap is None else cap
    # every hypothesis exactly once, order kept, consecutive
    assert [r for a, e in rounds for r in range(a, e)] == list(range(len(owners)))
    assert all(a < e for a, e in rounds)
    # no round above the cap, and none that could have taken the next hypothesis as well (but the last)
    assert all(32 * T * (e - a) <= cap for a, e in rounds)
    assert all(32 * T * (e - a + 1) > cap for a, e in rounds[:-1])


def test_round_planner_figures_and_refusal():
    from hgmm_amd._native import plan_batch_multi_rounds
    # 32 pairs x 27 starts: one round at L = 5 (1.2 MB a hypothesis), two at L = 6 (9.6 MB: 448 fit)
    assert plan_batch_multi_rounds(37448, [0] * 864) == [(0, 864)]
    assert plan_batch_multi_rounds(299592, [0] * 864) == [(0, 448), (448, 864)]
    assert plan_batch_multi_rounds(72, [0] * 9, 4 * 32 * 72) == [(0, 4), (4, 8), (8, 9)]
    with pytest.raises(ValueError, match=r"hypothesis 0 \(pair 3\)"):
        plan_batch_multi_rounds(72, [3, 1], 32 * 72 - 1)


# ---- registration_gmmtree_batch(starts=): refusals before the device, winner selection, starts=None ----------------------
class Dead:
    """a context that must not be reached"""
    def __getattr__(self, name):
        raise AssertionError("the device was reached: %s" % name)


def test_starts_are_validated_before_the_device_is_reached():
    from hgmm_amd.hgmm.hgmm_gpu import RigidTransformation, registration_gmmtree_batch
    rs = np.random.RandomState(0)
    pairs = [(rs.rand(100, 3), rs.rand(90, 3)) for _ in range(3)]
    s1, s2 = RigidTransformation(np.identity(3), np.zeros(3)), RigidTransformation(np.identity(3), np.zeros(3), 2.0)
    with pytest.raises(ValueError, match="2 lists for 3 pairs"):
        registration_gmmtree_batch(pairs, ctx=Dead(), starts=[[s1], [s1]])
    with pytest.raises(ValueError, match="pair 1 has no start"):
        registration_gmmtree_batch(pairs, ctx=Dead(), starts=[[s1], [], [s1, s1]])
    with pytest.raises(ValueError, match="pair 0 has no start"):
        registration_gmmtree_batch(pairs, ctx=Dead(), starts=[])
    with pytest.raises(ValueError, match=r"share one scale \(pair 2"):
        registration_gmmtree_batch(pairs, ctx=Dead(), starts=[[s1], [s1, s1], [s1, s2]])
    with pytest.raises(ValueError, match="share one scale"):
        registration_gmmtree_batch(pairs, ctx=Dead(), starts=[s1, s2])
    with pytest.raises(ValueError, match="voxel_size"):            # (voxel_size next to weights: still refused first)
        registration_gmmtree_batch(pairs, ctx=Dead(), starts=[s1], voxel_size=0.1, target_weights=[np.ones(90)] * 3)


class Recorder:
    """stands in for the context: records the calls, hands out what the test planted"""
    tree_dtype = np.dtype(np.float64)

    def __init__(self, sums=None, status=None):
        self.calls, self.sums, self.status = [], sums, status

    def set_points_batch(self, srcs, weights=None):
        self.calls.append(("points", len(srcs)))

    def tree_set_precision(self, dtype):
        pass

    def tree_build_batch(self, counts, L, ls, ld, sig2, want_tables, init_mu):
        self.calls.append(("build", len(counts), L))
        return None, np.ones((len(counts), L), np.int32), None

    def tree_set_targets_batch(self, tgts, weights=None):
        self.counts = [len(t) for t in tgts]
        self.calls.append(("targets", len(tgts)))

    def tree_get_reg_gate(self):
        return np.inf

    def tree_set_reg_gate(self, gate):
        self.calls.append(("gate", gate))

    def config(self, **kw):
        self.calls.append(("config", kw))
        return contextlib.nullcontext()

    def tree_register_batch(self, rot, t, scale, lambda_c, maxiter, tol):
        B = len(rot)
        self.calls.append(("register_batch", B))
        return rot.copy(), t.copy(), np.full(B, 3, np.int32), np.full(B, 0.5), np.ones(B, np.int32), None

    def tree_register_batch_multi(self, pair, rot, t, scale, lambda_c, maxiter, tol):
        R = len(pair)
        self.calls.append(("register_batch_multi", np.asarray(pair).tolist(), maxiter))
        # hypothesis r "moves" by r along x in r + 1 iterations
        t = t + np.arange(R)[:, None] * np.array([1.0, 0.0, 0.0])
        status = np.ones(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        return rot.copy(), t, (np.arange(R) + 1).astype(np.int32), np.arange(R) + 0.5, status, None

    def tree_score_batch_multi(self, pair, rot, t, scale, lambda_c, maha2_max):
        self.calls.append(("score_batch_multi", np.asarray(pair).tolist(), maha2_max))
        return np.array(self.sums, dtype=np.float64)


def test_winner_per_pair_over_stubbed_native_calls():
    from hgmm_amd.hgmm import hgmm_gpu as H
    rs = np.random.RandomState(1)
    pairs = [(rs.rand(80, 3), rs.rand(60, 3)) for _ in range(3)]
    mk = lambda z: H.RigidTransformation(np.identity(3), np.array([0.0, 0.0, float(z)]))
    starts = [[mk(0), mk(1)], [mk(2), mk(3), mk(4)], [mk(5)]]
    # pair 0: the second has more inliers.  pair 1: a three-way inlier tie, two of them tie in summary[2] as well: the lower
    # index of ITS group (1) wins -- although row 0 of the whole set, in another group, would beat all of them.
    sums = [summary(99, 0.5), summary(100, 9.0),
            summary(70, 8.5), summary(70, 8.0), summary(70, 8.0),
            summary(1, 0.0)]
    ctx = Recorder(sums)
    res, info = H.registration_gmmtree_batch(pairs, maxiter=9, tol=1e-3, ctx=ctx, tree_level=1, starts=starts, return_info=True,
                                             maha2_max=7.0)
    names = [c[0] for c in ctx.calls]
    assert names.count("register_batch_multi") == 1 and names.count("score_batch_multi") == 1 and "register_batch" not in names
    assert names.index("build") < names.index("targets") < names.index("register_batch_multi") < names.index("score_batch_multi")
    assert ("register_batch_multi", [0, 0, 1, 1, 1, 2], 9) in ctx.calls and ("score_batch_multi", [0, 0, 1, 1, 1, 2], 7.0) in ctx.calls
    assert not any(c[0] == "config" for c in ctx.calls)
    assert [r.best_index_ for r in res] == [1, 1, 0]
    assert [r.n_iter_ for r in res] == [2, 4, 6]                 # rows 1, 3, 5 of the set: r + 1 iterations
    assert all(isinstance(r, H.MultiStartResult) for r in res)
    assert [float(r.q[0]) for r in res] == [1.5, 3.5, 5.5]
    # what comes back is the inverse of the loop's pose: start z, moved by the row number along x
    assert np.allclose(res[1].transformation.t, -np.array([3.0, 0.0, 3.0]))
    assert [r.score.n_inliers for r in res] == [100, 70, 1] and all(r.score.node is None for r in res)
    assert info["hypothesis_iters"] == [[1, 2], [3, 4, 5], [6]] and info["hypothesis_status"] == [[1, 1], [1, 1, 1], [1]]
    assert [[s.n_inliers for s in p] for p in info["hypothesis_scores"]] == [[99, 100], [70, 70, 70], [1]]
    assert info["score"] == [r.score for r in res] and info["registration_iters"] == [2, 4, 6] and info["status"] == [1, 1, 1]
    # one list for every pair; the solve on the device is the per-context option around the multi call
    ctx2 = Recorder([summary(5, 1.0), summary(6, 1.0)] * 3)
    res2 = H.registration_gmmtree_batch(pairs, ctx=ctx2, tree_level=1, starts=starts[0], solve_on_device=True)
    assert [r.best_index_ for r in res2] == [1, 1, 1]
    assert ("register_batch_multi", [0, 0, 1, 1, 2, 2], 20) in ctx2.calls and ("config", {"reg_device_solve": 1}) in ctx2.calls


def test_rounds_in_the_mirror_keep_the_order(monkeypatch):
    from hgmm_amd import _native
    from hgmm_amd.hgmm import hgmm_gpu as H
    rs = np.random.RandomState(2)
    pairs = [(rs.rand(80, 3), rs.rand(60, 3)) for _ in range(2)]
    starts = [H.RigidTransformation(np.identity(3), np.zeros(3))] * 3

    class Rounds(Recorder):
        def tree_score_batch_multi(self, pair, rot, t, scale, lambda_c, maha2_max):
            self.calls.append(("score_batch_multi", np.asarray(pair).tolist(), maha2_max))
            return np.array([summary(10 + p, 1.0) for p in pair], dtype=np.float64)
    ctx = Rounds()
    monkeypatch.setattr(_native, "BATCH_MULTI_MAX_BYTES", 4 * 32 * 8)            # T = 8 at L = 1: four hypotheses a round
    res = H.registration_gmmtree_batch(pairs, ctx=ctx, tree_level=1, starts=starts)
    assert [c[1] for c in ctx.calls if c[0] == "register_batch_multi"] == [[0, 0, 0, 1], [1, 1]]
    assert [c[1] for c in ctx.calls if c[0] == "score_batch_multi"] == [[0, 0, 0, 1], [1, 1]]
    # (the stub numbers the iterations within a call: rows 0 and 3 of round one)
    assert [r.best_index_ for r in res] == [0, 0] and [r.n_iter_ for r in res] == [1, 4]


def test_without_starts_none_of_the_new_calls_is_reached():
    from hgmm_amd.hgmm import hgmm_gpu as H
    rs = np.random.RandomState(3)
    pairs = [(rs.rand(80, 3), rs.rand(60, 3)) for _ in range(2)]
    ctx = Recorder()
    res = H.registration_gmmtree_batch(pairs, ctx=ctx, tree_level=1)
    names = [c[0] for c in ctx.calls]
    assert names.count("register_batch") == 1 and not any("multi" in n for n in names)
    assert len(res) == 2 and not any(isinstance(r, H.MultiStartResult) for r in res)
