"""The host side of the batched KMeans initialiser, without a GPU: what ``Context.kmeans_fit_batch``, ``KMeans.fit_batch``, the
GMMReg flavour's ``fit_batch`` and ``fit_frames(flavour=)`` refuse before the device is reached, and the order in which
``fit_batch`` consumes the random stream against a loop of ``fit`` (the native calls stubbed; the one library call that
runs is the host helper hgmm_kmeans_center_f64)."""
import collections

import numpy as np
import pytest


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


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


class _Stub:
    """A context that records what the mirrors hand to the device and answers with something of the right shape."""
    nranks, comm_attached = 1, False

    def __init__(self):
        self.seeding = []                     # (first_id, rand_vals) per cloud, in the order the device would see them
        self.batches = 0

    # the serial path
    def set_points(self, Xc):
        self.Xc = np.asarray(Xc)

    def kmeans_plusplus(self, k, first_id, rand_vals):
        self.seeding.append((int(first_id), np.array(rand_vals)))
        return np.arange(k, dtype=np.int64), self.Xc[:k].copy()

    def kmeans_lloyd(self, centres, max_iter, tol_abs, reset_labels=True):
        return np.array(centres), 1, True, None

    def kmeans_labels(self):
        return np.zeros(len(self.Xc), np.int32)

    # the batched path
    def set_points_batch(self, clouds):
        self.clouds = [np.asarray(c) for c in clouds]

    def kmeans_fit_batch(self, counts, k, max_iter, tol_abs, first_ids=None, rand_vals=None, init_centres=None):
        assert list(counts) == [len(c) for c in self.clouds]
        self.batches += 1
        B = len(counts)
        if first_ids is not None:
            self.seeding += [(int(f), np.array(r)) for f, r in zip(first_ids, rand_vals)]
        start = np.stack([c[:k] for c in self.clouds]) if init_centres is None else np.array(init_centres)
        return {"ids": None if first_ids is None else np.tile(np.arange(k, dtype=np.int64), (B, 1)), "seeds": start,
                "centres": start.copy(), "n_iter": np.ones(B, np.int32), "strict": np.ones(B, np.int32),
                "status": np.zeros(B, np.int32), "inertia": np.zeros(B), "labels": [np.zeros(n, np.int32) for n in counts]}


def _clouds(sizes=(40, 25, 33)):
    rs = np.random.RandomState(9)
    return [rs.rand(n, 3) for n in sizes]


def _same_seeding(a, b):
    assert len(a) == len(b)
    for (fa, ra), (fb, rb) in zip(a, b):
        assert fa == fb and np.array_equal(ra, rb)


@pytest.mark.parametrize("seed", ["shared", 1])
def test_fit_batch_consumes_the_random_stream_as_a_loop_of_fit(seed):
    """Cloud by cloud in order: one random_sample, then uniform(size=(k - 1, trials)).  A shared RandomState is drawn from
    in the loop's order and left where the loop leaves it; an int seed gives every cloud a fresh RandomState(seed)."""
    from hgmm_amd.kmeans import KMeans
    Xs, k = _clouds(), 7
    state = lambda: np.random.RandomState(5) if seed == "shared" else seed
    loop_ctx, rs_loop = _Stub(), state()
    loop = [KMeans(k, random_state=rs_loop, max_iter=3, ctx=loop_ctx).fit(X) for X in Xs]
    batch_ctx, rs_batch = _Stub(), state()
    fits = KMeans(k, random_state=rs_batch, max_iter=3, ctx=batch_ctx).fit_batch(Xs)
    assert batch_ctx.batches == 1 and len(fits) == 3
    _same_seeding(batch_ctx.seeding, loop_ctx.seeding)
    assert all(r.shape == (k - 1, 2 + int(np.log(k))) for _, r in batch_ctx.seeding)
    if seed == "shared":
        assert rs_batch.random_sample() == rs_loop.random_sample()
        assert len({r.tobytes() for _, r in batch_ctx.seeding}) == 3          # (the stream moves on from cloud to cloud)
    else:
        assert all(np.array_equal(r, batch_ctx.seeding[0][1]) for _, r in batch_ctx.seeding)
    for f, g in zip(fits, loop):                             # the estimators come back in the state fit leaves
        assert np.array_equal(f.cluster_centers_, g.cluster_centers_) and np.array_equal(f.init_indices_, g.init_indices_)
        assert np.array_equal(f.labels_, g.labels_) and f.inertia_ == g.inertia_ and f.n_iter_ == g.n_iter_ == 1


def test_fit_batch_with_a_list_of_starts_draws_nothing():
    from hgmm_amd.kmeans import KMeans
    Xs, k = _clouds(), 4
    rs = np.random.RandomState(3)
    ctx = _Stub()
    fits = KMeans(k, random_state=rs, init=[X[:k] for X in Xs], max_iter=3, ctx=ctx).fit_batch(Xs)
    assert not ctx.seeding and all(f.init_indices_ is None for f in fits)
    assert rs.random_sample() == np.random.RandomState(3).random_sample()


def test_fit_batch_refusals_need_no_device():
    from hgmm_amd.kmeans import KMeans
    Xs = _clouds()
    dead = _context()
    with pytest.raises(ValueError, match=r"cloud 1: n_samples=25 should be >= n_clusters=30"):
        KMeans(30, ctx=dead).fit_batch(Xs)
    with pytest.raises(ValueError, match=r"cloud 2: expected an \[N,3\] array"):
        KMeans(3, ctx=dead).fit_batch(Xs[:2] + [np.zeros((5, 2))])
    with pytest.raises(ValueError, match="3 clouds, but init has 2 entries"):
        KMeans(3, init=[X[:3] for X in Xs[:2]], ctx=dead).fit_batch(Xs)
    with pytest.raises(ValueError, match="unweighted"):
        KMeans(3, ctx=dead).fit_batch(Xs, sample_weight=[np.ones(len(X)) for X in Xs])
    assert KMeans(3, ctx=dead).fit_batch([]) == []


def test_binding_refuses_length_mismatches_before_the_library():
    c, k = _context(), 5
    counts = [40, 25, 33]
    rand = np.zeros((3, k - 1, 3))
    with pytest.raises(ValueError, match=r"first_ids must be \[3\]"):
        c.kmeans_fit_batch(counts, k, 10, 0.0, first_ids=[0, 1], rand_vals=rand)
    with pytest.raises(ValueError, match=r"rand_vals must be \[3,4,n_trials\]"):
        c.kmeans_fit_batch(counts, k, 10, 0.0, first_ids=[0, 1, 2], rand_vals=rand[:2])
    with pytest.raises(ValueError, match=r"rand_vals must be \[3,4,n_trials\]"):
        c.kmeans_fit_batch(counts, k, 10, 0.0, first_ids=[0, 1, 2], rand_vals=np.zeros((3, k, 3)))
    with pytest.raises(ValueError, match=r"init_centres must be \[3,5,3\]"):
        c.kmeans_fit_batch(counts, k, 10, 0.0, init_centres=np.zeros((2, k, 3)))
    with pytest.raises(ValueError, match="one of the two"):
        c.kmeans_fit_batch(counts, k, 10, 0.0)
    with pytest.raises(ValueError, match="one of the two"):
        c.kmeans_fit_batch(counts, k, 10, 0.0, first_ids=[0, 1, 2], init_centres=np.zeros((3, k, 3)))
    with pytest.raises(ValueError):
        c.kmeans_fit_batch(counts, k, 10, [0.0, 0.0], first_ids=[0, 1, 2], rand_vals=rand)      # tol_abs [2] for 3 members


WeightedPoints = collections.namedtuple("WeightedPoints", ["points", "weights"])


def test_flavour_g_fit_batch_refusals_need_no_device():
    from hgmm_amd.gmmreg_gpu.gmm import GMM_GPU_Base
    Xs = _clouds()
    with pytest.raises(ValueError, match="weighted_init=True is not supported"):
        GMM_GPU_Base(4, weighted_init=True).fit_batch(Xs)
    with pytest.raises(ValueError, match="3 frames, but 2 initialisations"):
        GMM_GPU_Base(4).fit_batch(Xs, inits=[(X[:4], np.ones(4) / 4) for X in Xs[:2]])
    with pytest.raises(ValueError, match="3 frames, but 1 sample_weight entries"):
        GMM_GPU_Base(4).fit_batch(Xs, sample_weight=[np.ones(40)])
    with pytest.raises(ValueError, match="frame 1 brings per-point weights"):
        GMM_GPU_Base(4).fit_batch([Xs[0], WeightedPoints(Xs[1], np.ones(25)), Xs[2]])
    assert GMM_GPU_Base(4).fit_batch([]) == []


def test_fit_frames_flavour_refusals_need_no_device():
    from hgmm_amd import replicas
    with pytest.raises(ValueError, match="flavour must be 'W' or 'G'"):
        replicas.fit_frames(_clouds(), flavour="X")
    with pytest.raises(ValueError, match="flavour='G'"):
        replicas.fit_frames(_clouds(), flavour="G", cov_type="spherical")
    with pytest.raises(ValueError, match="flavour='G'"):
        replicas.fit_frames(_clouds(), flavour="G", voxel_size=0.1)


def test_init_gmm_params_batch_is_the_serial_call_per_member(monkeypatch):
    """(centres, uniform weights) per member, from ONE batched KMeans of the reference's settings."""
    from hgmm_amd import kmeans
    from hgmm_amd.gmmreg_gpu import gmm_impl
    seen = {}

    def fake(Xs, k, random_state=1, max_iter=50, ctx=None):
        seen.update(k=k, random_state=random_state, max_iter=max_iter, B=len(Xs))
        return [np.full((k, 3), float(b)) for b in range(len(Xs))]

    monkeypatch.setattr(kmeans, "kmeans_centres_batch", fake)
    out = gmm_impl.init_gmm_params_batch(_clouds(), 6)
    assert seen == dict(k=6, random_state=1, max_iter=50, B=3)
    for b, (c, w) in enumerate(out):
        assert np.array_equal(c, np.full((6, 3), float(b))) and np.array_equal(w, np.ones(6) / 6)


# -- the member and workgroup tables of the C entry, on the host under sanitizers -----------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """tests/kmeans_batch_plan_main.cpp over csrc/kmeans_batch_plan.h: a program of its own, built with the host compiler
    and -fsanitize=address,undefined."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd", "csrc")
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", rocm_clang) if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("kmplan") / "kmeans_batch_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", csrc, os.path.join(root, "tests", "kmeans_batch_plan_main.cpp"), "-o", exe],
                   check=True)

    def run(k_alloc, acc_lds, cus, counts):
        r = subprocess.run([exe, str(k_alloc), str(int(acc_lds)), str(cus)] + [str(n) for n in counts], capture_output=True,
                           text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, (r.stdout, r.stderr)
        return r.stdout
    return run


@pytest.mark.parametrize("k_alloc,acc_lds", [(256, True), (1024, True), (2048, False)])
def test_member_and_workgroup_tables(plan, k_alloc, acc_lds):
    """Every member gets the serial grids of a cloud of its size and pieces of the buffers that follow each other without
    overlap, each starting at a multiple of 4096 rows; every sized launch's table lists member after member."""
    edges = [1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8192, 8193, 40256, 65536, 65537, 131073]
    out = plan(k_alloc, acc_lds, 256, edges)
    assert out.startswith("ok B=%d " % len(edges))
    plan(k_alloc, acc_lds, 256, [40256] * 64)
    plan(k_alloc, acc_lds, 8, [1000000, 3])                  # the accumulator capped by the CUs
    plan(k_alloc, acc_lds, 256, [16777216])                  # the largest member: 4096 seeding workgroups
    plan(k_alloc, acc_lds, 256, [1] * 4096)
    rs = np.random.RandomState(k_alloc)
    plan(k_alloc, acc_lds, 256, rs.randint(1, 20000, size=200))


def test_plan_header_needs_no_hip():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd", "csrc", "kmeans_batch_plan.h")
    with open(path) as f:
        includes = [line.split()[1] for line in f if line.lstrip().startswith("#include")]
    assert includes and all(i[0] == "<" and i[-1] == ">" and i[1:-1].isalnum() for i in includes)
