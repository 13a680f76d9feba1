"""The host side of the batched full-covariance fit, without a GPU: the member plan of hgmm_fullcov_fit_batch
(csrc/fullcov_batch_plan.h) as a host program under sanitizers, what ``Context.fullcov_fit_batch``, ``fitFullCovGMM_batch`` and
``fit_frames(flavour="full")`` refuse before the device is reached, and the oracle's side of the ragged GPU case
(tests/test_fullcov_batch_gpu.py): its iteration counts and the distance of every stop decision from ``ls``."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import hgmm_tree

LD, SIG2 = 1.0e-4, 0.0005
# the ragged batch of the GPU test: J = 16, ls = 1.0, budget 40
RAGGED_N = [1, 15, 16, 17, 33, 64, 777, 1300, 5032]
RAGGED_ITERS = [2, 9, 9, 7, 3, 13, 29, 33, 40]


def sub(bunny, N):
    return bunny[::max(1, len(bunny) // N)][:N].astype(np.float64)


def ragged_case(bunny, J=16):
    Ps = [sub(bunny, N) for N in RAGGED_N]
    idxs = [np.random.RandomState(J + N).choice(len(P), J, replace=len(P) < J) for N, P in zip(RAGGED_N, Ps)]
    return Ps, idxs


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd", "csrc")


# -- the member and workgroup tables of the C entry, on the host under sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """tests/fullcov_batch_plan_main.cpp over csrc/fullcov_batch_plan.h: a program of its own, built with the host compiler
    and -fsanitize=address,undefined."""
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", rocm_clang) if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("fcplan") / "fullcov_batch_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "fullcov_batch_plan_main.cpp"), "-o", exe],
                   check=True)

    def run(J, cus, counts):
        r = subprocess.run([exe, str(J), str(cus)] + [str(int(n)) for n in counts], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, (r.stdout, r.stderr)
        return r.stdout
    return run


@pytest.mark.parametrize("J", [1, 16, 17, 100, 1024])
def test_member_plan(plan, J):
    """Every member gets the serial grid min(tiles, CUs) and the serial tile-to-workgroup map, pieces of the buffers that
    follow each other without overlap, and the fused launch's table lists member after member."""
    cus = 256
    around = [16 * cus + d for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17)]         # counts around 16 * CUs
    out = plan(J, cus, [1, 15, 16, 17, 31, 32, 33] + around + [2095, 40256, 1000000])
    assert out.startswith("ok B=19 ") and out.rstrip().endswith("J16=%d" % ((J + 15) // 16 * 16))
    assert plan(J, cus, [2095]).startswith("ok B=1 rows=2095 wgs=131 ")            # B = 1: the voxel-sized cloud's 131 tiles
    assert plan(J, cus, [1] * 4096).startswith("ok B=4096 rows=4096 wgs=4096 ")
    plan(J, cus, [16 * cus + 1] * 4096)                                            # every member capped: 4096 * 256 workgroups
    plan(J, 8, [1000000, 3, 129])                                                  # a small chip
    # zero-tile edge cases: a member without points has no tile, no workgroup and no division (the entry refuses it)
    assert plan(J, cus, [0]).startswith("ok B=1 rows=0 wgs=0 ")
    assert plan(J, cus, [5, 0, 17]).startswith("ok B=3 rows=22 wgs=3 ")
    plan(J, cus, np.random.RandomState(J).randint(0, 20000, size=200))


def test_plan_header_needs_no_hip():
    with open(os.path.join(CSRC, "fullcov_batch_plan.h")) as f:
        includes = [line.split()[1] for line in f if line.lstrip().startswith("#include")]
    assert includes and all(i[0] == "<" and i[-1] == ">" and i[1:-1].isalnum() for i in includes)


# -- the Python argument checks that need no device ---------------------------------------------------------------------------
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


def test_binding_refuses_before_the_library():
    c, J = _context(), 5
    counts = [40, 25, 33]
    with pytest.raises(ValueError, match="one of the two"):
        c.fullcov_fit_batch(counts, J, 1.0, LD)
    with pytest.raises(ValueError, match="one of the two"):
        c.fullcov_fit_batch(counts, J, 1.0, LD, init_mu=np.zeros((3, J, 3)), init_rows=np.zeros((3, J), np.int64))
    with pytest.raises(ValueError, match=r"init_mu must be \[3,5,3\]"):
        c.fullcov_fit_batch(counts, J, 1.0, LD, init_mu=np.zeros((2, J, 3)))
    with pytest.raises(ValueError, match=r"init_rows must be \[3,5\]"):
        c.fullcov_fit_batch(counts, J, 1.0, LD, init_rows=np.zeros((3, J + 1), np.int64))
    with pytest.raises(ValueError, match="max_iters must be >= 1"):
        c.fullcov_fit_batch(counts, J, 1.0, LD, init_rows=np.zeros(J, np.int64), max_iters=0)


def test_mirror_refusals_need_no_device():
    from hgmm_amd import replicas
    from hgmm_amd.hgmm.hgmm_gpu import WeightedPoints, fitFullCovGMM_batch
    dead = _context()
    rs = np.random.RandomState(9)
    Xs = [rs.rand(n, 3) for n in (40, 25, 33)]
    assert fitFullCovGMM_batch([], 4, ctx=dead) == []
    with pytest.raises(ValueError, match="3 clouds, but 2 weights entries"):
        fitFullCovGMM_batch(Xs, 4, weights=[None, None], ctx=dead)
    with pytest.raises(ValueError, match=r"expected shape \(25,\)"):
        fitFullCovGMM_batch(Xs, 4, weights=[None, np.ones(24), None], ctx=dead)
    with pytest.raises(ValueError, match="finite and >= 0"):
        fitFullCovGMM_batch([Xs[0], WeightedPoints(Xs[1], -np.ones(25))], 4, ctx=dead)
    with pytest.raises(ValueError, match=r"init_idx must be \[4\] or \[3,4\]"):
        fitFullCovGMM_batch(Xs, 4, init_idx=np.zeros((2, 4), np.int64), ctx=dead)
    with pytest.raises(ValueError, match="batch must be >= 1"):
        replicas.fit_frames(Xs, 4, flavour="full", batch=0)
    with pytest.raises(ValueError, match="flavour must be 'W' or 'G'"):
        replicas.fit_frames(Xs, 4, flavour="fullcov")


def test_fit_frames_full_cuts_chunks_like_the_other_flavours(monkeypatch):
    """flavour="full": batch = 1 -> fitFullCovGMM per frame, batch > 1 -> fitFullCovGMM_batch per chunk (the last one short),
    tol handed over as ls and max_iter as the budget"""
    from hgmm_amd import replicas
    from hgmm_amd.hgmm import hgmm_gpu
    seen = []
    monkeypatch.setattr(hgmm_gpu, "fitFullCovGMM", lambda frame, J, ctx=None, **kw: seen.append(("one", frame, J, kw)) or frame)
    monkeypatch.setattr(hgmm_gpu, "fitFullCovGMM_batch", lambda part, J, ctx=None, **kw: seen.append(("chunk", list(part), J, kw)) or list(part))

    class Pool:
        def map(self, fn, jobs):
            return [fn(None, j) for j in jobs]

    kw = dict(ls=0.5, max_iters=7)
    assert replicas.fit_frames(range(5), 6, max_iter=7, tol=0.5, flavour="full", pool=Pool(), batch=2) == list(range(5))
    assert seen == [("chunk", [0, 1], 6, kw), ("chunk", [2, 3], 6, kw), ("chunk", [4], 6, kw)]
    del seen[:]
    assert replicas.fit_frames(range(3), 6, max_iter=7, tol=0.5, flavour="full", pool=Pool()) == [0, 1, 2]
    assert seen == [("one", f, 6, kw) for f in range(3)]


# -- the oracle's side of the ragged GPU case -----------------------------------------------------------------------------------
def test_ragged_case_on_the_oracle(bunny):
    """J = 16, ls = 1.0, budget 40: the members stop after 2 .. 33 iterations or run into the budget, no stop decision is
    closer than 0.11 ls to going the other way (rounding cannot change a count), and the dead-component rule m0 < ld fires in
    most members.  If an input drifts, the GPU test fails here first."""
    Ps, idxs = ragged_case(bunny)
    iters, margins, dead = [], [], []
    for P, idx in zip(Ps, idxs):
        pi, mu, cov, q, cur = hgmm_tree.build_flat_fullcov(P, 16, 1.0, LD, idx, SIG2, max_iters=40)
        iters.append(len(q))
        margins.append(hgmm_tree.stop_margins(q, [len(q)], 1.0).min())
        dead.append(int((pi == 0.0).sum()))
    print("iterations", iters, "margins", ["%.3g" % m for m in margins], "dead components", dead)
    assert [len(P) for P in Ps] == RAGGED_N
    assert iters == RAGGED_ITERS
    assert min(margins) >= 0.11
    assert sum(d > 0 for d in dead) > len(dead) // 2
    assert -(-5032 // 16) > 256 and -(-1300 // 16) < 256      # more tiles than CUs for the largest member only
