"""The operation table of the context-history tests (test_context_history_gpu.py / _cpu.py): every numerical family of
include/hgmm.h as a self-contained call sequence, each at a LARGE and a SMALL shape (a helper, not a conftest and not an
oracle).

    OPS[name] = Op(fn, family, size, dims)       fn(ctx) -> tuple of NumPy arrays: EVERY output of the entries it calls

An op uploads everything it reads -- points, targets, weights, nodes, pairs -- and takes every seed explicitly, so its result
is a function of the op alone: whatever differs between two runs of it comes from what the context held before.  ``dims``
names what sizes a buffer (n, J / T / k, B, R / K ...); the large shape exceeds the small one in every one of them
(test_context_history_cpu.py), so that after a large op the small one works in buffers whose tails hold the large one's data
and, in the batches, inside a hand-over block laid out for the larger B.

Shapes (the smallest that still separate the buffer sizes):
    clouds     bunny[::13] (3097 points) / bunny[::130] (310); the batches of the large shape hold a member of ONE point
               where the entry takes one (KMeans wants k <= n, a registration wants a tree: there the third member has 415)
    flat EM    J = 100 / 8          KMeans  k = 50 / 3          full covariance  J = 40 / 3
    tree       L = 3 / 2 (T = 584 / 72); registration on the reference's own L = 3 / L = 2 node tables (tests/golden)
    forest     B = 3, L = 3, R = 7 / B = 1, L = 2, R = 1
    voxel      bunny[::13] at 10 mm (a few hundred voxels) / a 3-point cloud
    L2         the ragged pairs of test_gmmreg_resident_gpu.py, (70, 300) among them, B = 4, R = 40 / (1, 1), B = 1, R = 1
"""
import functools
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hgmm.h")

Op = namedtuple("Op", ["fn", "family", "size", "dims"])
Shape = namedtuple("Shape", ["size", "stride", "J", "k", "Jf", "L", "B", "R", "voxel", "l2", "l2_R"])

SHAPES = {
    "large": Shape("large", 13, 100, 50, 40, 3, 3, 7, 0.01, ((30, 25), (70, 300), (5, 129), (200, 64)), 40),
    "small": Shape("small", 130, 8, 3, 3, 2, 1, 1, 0.5, ((1, 1),), 1),
}
SIZES = ("large", "small")
FAMILIES = ("flat", "kmeans", "fullcov", "tree", "forest", "voxel", "l2", "handles")

# the tree builds' parameters (the bunny's 0.1 m scale: those of __graft_entry__.smoke) and iteration budgets
LS, LD, SIG2, TREE_BUDGET = 20.0, 1e-4, 0.004, 8
LAMBDA_C, REG_BUDGET, REG_TOL = 0.01, 6, 1e-4
FLAT_ITERS, FULL_ITERS, FULL_LS, FULL_SIG2, KM_ITERS = 5, 10, 1.0, 0.0005, 10
CHI2_3_999 = 16.27
I3, Z3 = np.identity(3), np.zeros(3)

OPS = {}


def n_total(L):
    return 8 * (8 ** L - 1) // 7


def flat(x):
    """a result -- arrays, numbers, device arrays, None, nested in tuples / lists / dicts -- as a flat tuple of arrays"""
    if x is None:
        return ()
    if isinstance(x, (tuple, list)):
        return tuple(a for y in x for a in flat(y))
    if isinstance(x, dict):
        return tuple(a for key in sorted(x) for a in flat(x[key]))
    if not isinstance(x, np.ndarray) and hasattr(x, "get"):
        return (np.asarray(x.get()),)
    return (np.asarray(x),)


def same_bits(a, b):
    """two flat results agree in count, shape, type and every bit (NaN payloads and the sign of zero included)"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
                                    for x, y in zip(a, b))


def first_difference(a, b):
    if len(a) != len(b):
        return "%d outputs against %d" % (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype:
            return "output %d: %s %s against %s %s" % (i, x.dtype, x.shape, y.dtype, y.shape)
        if x.tobytes() != y.tobytes():
            xb = np.ascontiguousarray(x).reshape(-1).view(np.uint8).reshape(x.size, x.dtype.itemsize)
            yb = np.ascontiguousarray(y).reshape(-1).view(np.uint8).reshape(y.size, y.dtype.itemsize)
            bad = np.flatnonzero((xb != yb).any(axis=1))
            at = int(bad[0])
            return "output %d %s %s: %d of %d entries differ, first at %d: %r against %r" % (
                i, x.dtype, x.shape, len(bad), x.size, at, x.reshape(-1)[at], y.reshape(-1)[at])
    return None


class Recorder:
    """A forwarding proxy for ``Context.lib`` that notes which hgmm_* entries were asked for (the wrapper fetches an entry
    from ``self.lib`` right before it calls it)."""

    def __init__(self, lib, reached):
        self._lib, self._reached = lib, reached

    def __getattr__(self, name):
        if name.startswith("hgmm_"):
            self._reached.add(name)
        return getattr(self._lib, name)


REACHED = set()


def recording_context():
    """a fresh ``Context(0)`` whose library calls are noted in REACHED"""
    import hgmm_amd
    c = hgmm_amd.Context(0)
    c.lib = Recorder(c.lib, REACHED)
    return c


def run_fresh(name):
    """the op on a context of its own, closed straight afterwards"""
    c = recording_context()
    try:
        return OPS[name].fn(c)
    finally:
        c.close()


def register(name, family, dims):
    """decorator: fn(ctx, shape) becomes OPS[name + '_large'] and OPS[name + '_small']; dims(shape) -> {dimension: size}"""
    def wrap(fn):
        for size in SIZES:
            s = SHAPES[size]
            OPS["%s_%s" % (name, size)] = Op(functools.partial(fn, s=s), family, size, dims(s))
        return fn
    return wrap


# ---- data: seeded, computed once per process, never modified ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bunny():
    b = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def cloud(size, dtype="float64"):
    """the family's cloud: bunny[::13] / bunny[::130]"""
    a = np.ascontiguousarray(bunny()[::SHAPES[size].stride], dtype=dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def members(size, dtype="float64", one_point=True):
    """the batches' clouds: B = 3 (3097, 1388 and 1 point -- or 415 where the entry cannot take one point) / B = 1 (310)"""
    b = bunny()
    if size == "small":
        raw = [b[::130]]
    else:
        raw = [b[::13], b[5::29], b[7:8] if one_point else b[3::97]]
    out = tuple(np.ascontiguousarray(a, dtype=dtype) for a in raw)
    for a in out:
        a.setflags(write=False)
    return out


def n_of(size, one_point=True):
    return sum(len(a) for a in members(size, "float64", one_point))


@functools.lru_cache(maxsize=None)
def weights(n, seed=11):
    """uniform in [0.25, 4), one in ten exactly zero (tests/_tree_helpers.weights_for); a single point weighs 1.5"""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.25, 4.0, n)
    w[rs.uniform(size=n) < 0.1] = 0.0
    if not (w > 0).any():
        w[:] = 1.5
    w.setflags(write=False)
    return w


def rows_of(n, count, seed):
    """``count`` row numbers of a cloud of n points (with repetition: T may exceed n)"""
    return np.random.RandomState(seed).randint(n, size=count)


def flat_init(X, J, seed=1, cov_type="diag", cov0=0.1):
    """means = J rows of X (distinct where X has J), cov = cov0, w = 1 / J, float32 (oracle/flat_em.seeded_init)"""
    rs = np.random.RandomState(seed)
    idx = rs.choice(len(X), J, replace=len(X) < J)
    mu = np.ascontiguousarray(X[idx], dtype=np.float32)
    cov = np.full((J, 3) if cov_type == "diag" else (J,), cov0, np.float32)
    return mu, np.full(J, 1.0 / J, np.float32), cov


def moved(P, deg, axis, shift):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    return np.ascontiguousarray(np.asarray(P, dtype=np.float64) @ R.T + np.asarray(shift))


def poses(count, seed=5):
    """start poses: rotations of up to a few degrees about seeded axes, shifts of millimetres; the first is the identity"""
    rs = np.random.RandomState(seed)
    rot, t = [I3], [Z3]
    for _ in range(count - 1):
        rot.append(moved(I3, rs.uniform(-4, 4), rs.randn(3), Z3).T.copy())
        t.append(rs.uniform(-0.003, 0.003, 3))
    return np.stack(rot), np.stack(t)


RegCase = namedtuple("RegCase", ["L", "T", "pi", "mu", "cov", "points", "target"])


@functools.lru_cache(maxsize=None)
def reg_case(size):
    """the reference's own node tables (tests/golden: its L = 3 build of 1007 points, its L = 2 build of 2013) and a moved
    copy of the cloud they were built on as the target: 1007 / 288 points"""
    if size == "large":
        g = np.load(os.path.join(GOLDEN, "hgmm_build_L3.npz"))
        P = g["points"]
    else:
        g = np.load(os.path.join(GOLDEN, "hgmm_build_L2.npz"))
        P = g["points"][::7]
    L = int(g["L"])
    return RegCase(L, n_total(L), g["pi"], g["mu"], g["cov"], np.ascontiguousarray(P),
                   moved(P, 6.0, [0.2, 1.0, 0.1], [0.003, -0.002, 0.001]))


def tree_init(P, L, seed=72):
    return np.ascontiguousarray(P[rows_of(len(P), n_total(L), seed)])


# ---- flat EM (diag / spherical, float32) ---------------------------------------------------------------------------------------

def _flat_dims(s):
    return {"n": len(cloud(s.size)), "J": s.J}


@register("flat_fit_diag", "flat", _flat_dims)
def flat_fit_diag(c, s):
    X = cloud(s.size, "float32")
    mu, w, cov = flat_init(X, s.J)
    c.set_points(X)
    return flat(c.flat_train(FLAT_ITERS, 0.0, mu, cov, w, "diag", "W"))


@register("flat_fit_spherical_and_G", "flat", _flat_dims)
def flat_fit_spherical_and_G(c, s):
    X = cloud(s.size, "float32")
    c.set_points(X)
    mu, w, cov = flat_init(X, s.J, 2, "spherical")
    sph = c.flat_train(FLAT_ITERS, 1e-7, mu, cov, w, "spherical", "W")
    mu, w, cov = flat_init(X, s.J, 3)
    return flat((sph, c.flat_train(FLAT_ITERS, 0.0, mu, cov, w, "diag", "G")))


@register("flat_fit_weighted", "flat", _flat_dims)
def flat_fit_weighted(c, s):
    """flat_set_weights + flat_train + flat_stats; the weights stay in force when the op ends: whatever comes next drops them"""
    X = cloud(s.size, "float32")
    mu, w, cov = flat_init(X, s.J, 4)
    c.set_points(X)
    c.flat_set_weights(weights(len(X), 21))
    fit = c.flat_train(FLAT_ITERS, 0.0, mu, cov, w, "diag", "W")
    return flat((fit, c.flat_stats(fit[0], fit[1], fit[2], "diag", "W")))


@register("flat_split_loop", "flat", _flat_dims)
def flat_split_loop(c, s):
    """flat_train_begin / _step / _end, uninterrupted: two steps of one iteration and one of three"""
    X = cloud(s.size, "float32")
    mu, w, cov = flat_init(X, s.J, 5)
    c.set_points(X)
    c.flat_train_begin(0.0, mu, cov, w, "diag", "W", lls_capacity=16)
    for iters in (1, 1, 3):
        c.flat_train_step(iters)
    return flat(c.flat_train_end())


def _flat_batch_dims(s):
    return {"n": n_of(s.size), "J": s.J, "B": s.B}


def _batch_inits(clouds, J, seed):
    inits = [flat_init(X, J, seed + b) for b, X in enumerate(clouds)]
    return [i[0] for i in inits], [i[2] for i in inits], [i[1] for i in inits]


@register("flat_batch", "flat", _flat_batch_dims)
def flat_batch(c, s):
    """flat_train_batch over points_create handles, plain and with per-slot weights (a None slot beside weighted ones)"""
    clouds = members(s.size, "float32")
    mu, cov, w = _batch_inits(clouds, s.J, 30)
    handles = [c.points_create(X) for X in clouds]
    try:
        plain = c.flat_train_batch(handles, FLAT_ITERS, 0.0, mu, cov, w, "diag", "W")
        sw = [weights(len(X), 40 + b).astype(np.float32) if b != 1 else None for b, X in enumerate(clouds)]
        weighted = c.flat_train_batch(handles, FLAT_ITERS, 0.0, mu, cov, w, "diag", "W", weights=sw)
    finally:
        for h in handles:
            c.points_destroy(h)
    return flat((plain, weighted))


def _voxel_clouds(size, dtype="float64"):
    """the voxel family's raw clouds: the batch members / one cloud of 3 points, two of them in one voxel"""
    if size == "large":
        return members("large", dtype)
    a = np.ascontiguousarray([[0.0, 0.0, 0.0], [0.125, 0.125, 0.0], [1.0, 1.0, 1.0]], dtype=dtype)
    a.setflags(write=False)
    return (a,)


def _voxel_dims(s):
    return {"n": sum(len(a) for a in _voxel_clouds(s.size)), "B": s.B, "J": s.J, "T": n_total(s.L)}


@register("flat_batch_voxels", "flat", _voxel_dims)
def flat_batch_voxels(c, s):
    """flat_train_batch_voxels over the members of a resident voxel result, counts as weights and without"""
    clouds = _voxel_clouds(s.size, "float32")
    mu, cov, w = _batch_inits(clouds, s.J, 50)
    vcs = c.voxel_down_sample_batch(clouds, s.voxel, download=False).members()
    counted = c.flat_train_batch_voxels(vcs, FLAT_ITERS, 0.0, mu, cov, w, "diag", "W", weighted=True)
    plain = c.flat_train_batch_voxels(vcs[::-1], FLAT_ITERS, 0.0, mu[::-1], cov[::-1], w[::-1], "diag", "W", weighted=False)
    return flat((counted, plain))


def _estep_params(X, J, seed):
    mu, w, _ = flat_init(X, J, seed)
    rs = np.random.RandomState(seed)
    inv = (1.0 / np.sqrt(0.0002 + 0.001 * rs.rand(J, 3))).astype(np.float32)
    return inv, mu, w


@register("flat_estep", "flat", _flat_dims)
def flat_estep(c, s):
    """the materialising E-step with the arg-max (row-maximum loop) and without (constant-shift loop), predict,
    estimate_log_prob, the M-step from responsibilities and from log-responsibilities"""
    X = cloud(s.size, "float32")
    inv, mu, w = _estep_params(X, s.J, 6)
    c.set_points(X)
    with_am = c.flat_estep(inv, mu, w, "diag", "W", want_lpn=True, want_argmax=True)
    without = c.flat_estep(inv, mu, w, "diag", "W", want_lpn=True, want_argmax=False)
    labels = c.flat_predict(inv, mu, w, "diag", "W")
    log_prob = c.flat_log_prob(inv, mu, "diag")
    m_log = c.flat_mstep(with_am[1].exp(), "diag", "W", centre_hint=mu)
    m_resp = c.flat_mstep(np.exp(with_am[1].get()), "diag", "W")
    return flat((with_am, without, labels, log_prob, m_log, m_resp))


@register("flat_device_arrays", "flat", _flat_dims)
def flat_device_arrays(c, s):
    """the parameters as device arrays: E-step, predict and M-step without a host trip, the caller's own elementwise
    update of inv_std between them, and the asynchronous E-step with its lazy mean"""
    X = cloud(s.size, "float32")
    inv, mu, w = _estep_params(X, s.J, 7)
    c.set_points(X)
    d_inv, d_mu, d_w = c.to_device(inv), c.to_device(mu), c.to_device(w)
    mean, lr, lpn, am = c.flat_estep(d_inv, d_mu, d_w, "diag", "W", want_lpn=True, want_argmax=True)
    labels = c.flat_predict(d_inv, d_mu, d_w, "diag", "W")
    w2, mu2, cov2 = c.flat_mstep(lr.exp(), "diag", "W", centre_hint=d_mu, device_out=True)
    inv2 = 1.0 / (np.sqrt(cov2 + 1e-6) + 1e-6)
    mean2, lr2, _, _ = c.flat_estep(inv2, mu2, w2, "diag", "W")
    lazy, lr3, lpn3, _ = c.flat_estep(inv, mu, w, "diag", "W", want_lpn=True, lazy_mean=True)
    return flat((mean, lr, lpn, am, labels, w2, mu2, cov2, inv2, mean2, lr2, float(lazy), lr3, lpn3))


# ---- KMeans initialiser (float64) ---------------------------------------------------------------------------------------------

KM_SEED = 8


def _km_inputs(n, k, seed):
    """the first seed and the uniforms of the later steps, drawn as oracle/kmeans.kmeans_plusplus draws them from
    RandomState(seed): the oracle seeded alike picks the same candidates"""
    rs = np.random.RandomState(seed)
    first = int(rs.choice(n, p=np.ones(n) / n))
    return first, rs.uniform(size=(k - 1, 2 + int(np.log(k))))


def _centred(P):
    return np.ascontiguousarray(P - P.mean(axis=0))


def _km_dims(s):
    return {"n": len(cloud(s.size)), "k": s.k}


def _kmeans(c, s, weighted):
    Xc = _centred(cloud(s.size))
    first, rand = _km_inputs(len(Xc), s.k, KM_SEED + weighted)
    c.set_points(Xc)
    if weighted:
        c.tree_set_source_weights(weights(len(Xc), 22))
    seeds = c.kmeans_plusplus(s.k, first, rand, weighted=weighted)
    loop = c.kmeans_lloyd(seeds[1], KM_ITERS, 0.0, weighted=weighted)
    step = c.kmeans_step(loop[0], weighted=weighted)
    return flat((seeds, loop, step, c.kmeans_labels(with_distances=True)))


@register("kmeans", "kmeans", _km_dims)
def kmeans(c, s):
    """k-means++ seeding, the device-resident Lloyd loop, one more assignment, labels and distances"""
    return _kmeans(c, s, False)


@register("kmeans_weighted", "kmeans", _km_dims)
def kmeans_weighted(c, s):
    return _kmeans(c, s, True)


@register("kmeans_batch", "kmeans", lambda s: {"n": n_of(s.size, False), "k": s.k, "B": s.B})
def kmeans_batch(c, s):
    clouds = [_centred(P) for P in members(s.size, "float64", one_point=False)]
    ins = [_km_inputs(len(P), s.k, 60 + b) for b, P in enumerate(clouds)]
    arrs = c.set_points_batch(clouds)
    fit = c.kmeans_fit_batch([len(a) for a in arrs], s.k, KM_ITERS, 0.0, first_ids=[i[0] for i in ins],
                             rand_vals=np.stack([i[1] for i in ins]))
    assert not fit["status"].any(), "a member met an empty cluster: its outputs are unspecified, choose other seeds"
    return flat(fit)


# ---- flat full-covariance EM (float64) -----------------------------------------------------------------------------------------

def _full_dims(s):
    return {"n": len(cloud(s.size)), "J": s.Jf}


def _fullcov(c, s, weighted, seed):
    P = cloud(s.size)
    c.set_points(P)
    if weighted:
        c.tree_set_source_weights(weights(len(P), 23))
    fit = c.fullcov_fit(s.Jf, FULL_LS, LD, P[rows_of(len(P), s.Jf, seed)], FULL_SIG2, FULL_ITERS, weighted=weighted)
    return flat((fit, c.fullcov_estep(fit[0], fit[1], fit[2], weighted=weighted)))


@register("fullcov_fit", "fullcov", _full_dims)
def fullcov_fit(c, s):
    return _fullcov(c, s, False, 9)


@register("fullcov_weighted", "fullcov", _full_dims)
def fullcov_weighted(c, s):
    return _fullcov(c, s, True, 10)


@register("fullcov_f32_tile", "fullcov", _full_dims)
def fullcov_f32_tile(c, s):
    """the float32-tile kernel: the fit and the E-step under tree_set_precision(float32), which the op takes back"""
    c.tree_set_precision(np.float32)
    try:
        return _fullcov(c, s, False, 11)
    finally:
        c.tree_set_precision(np.float64)


@register("fullcov_two_pass", "fullcov", _full_dims)
def fullcov_two_pass(c, s):
    with c.config(fullcov_two_pass=1):
        return _fullcov(c, s, False, 12)


@register("fullcov_batch", "fullcov", lambda s: {"n": n_of(s.size), "J": s.Jf, "B": s.B})
def fullcov_batch(c, s):
    """fullcov_fit_batch from explicit means, and from row numbers under the members' weights (one member unweighted)"""
    clouds = members(s.size)
    arrs = c.set_points_batch(clouds, weights=[weights(len(P), 70 + b) if b != 1 else None for b, P in enumerate(clouds)])
    counts = [len(a) for a in arrs]
    rows = np.stack([rows_of(n, s.Jf, 80 + b) for b, n in enumerate(counts)])
    plain = c.fullcov_fit_batch(counts, s.Jf, FULL_LS, LD, init_mu=np.stack([P[r] for P, r in zip(clouds, rows)]),
                                sig2=FULL_SIG2, max_iters=FULL_ITERS)
    weighted = c.fullcov_fit_batch(counts, s.Jf, FULL_LS, LD, init_rows=rows, sig2=FULL_SIG2, max_iters=FULL_ITERS, weighted=True)
    return flat((plain, weighted))


# ---- the tree: build --------------------------------------------------------------------------------------------------------

def _tree_dims(s):
    return {"n": len(cloud(s.size)), "T": n_total(s.L)}


@register("tree_build", "tree", _tree_dims)
def tree_build(c, s):
    P = cloud(s.size)
    c.set_points(P)
    built = c.tree_build(s.L, LS, LD, tree_init(P, s.L), SIG2, TREE_BUDGET)
    return flat((built, c.tree_node_complexity(n_total(s.L)), c.tree_stats()))


@register("tree_build_weighted", "tree", _tree_dims)
def tree_build_weighted(c, s):
    """under source weights, which stay in force when the op ends"""
    P = cloud(s.size)
    c.set_points(P)
    c.tree_set_source_weights(weights(len(P), 24))
    return flat(c.tree_build(s.L, LS, LD, tree_init(P, s.L, 73), SIG2, TREE_BUDGET))


@register("tree_build_rows", "tree", _tree_dims)
def tree_build_rows(c, s):
    """initial means gathered on the device from row numbers, a float32 upload, and the rows read back"""
    P = cloud(s.size, "float32")
    rows = rows_of(len(P), n_total(s.L), 74)
    c.set_points(P)
    return flat((c.tree_build(s.L, LS, LD, None, SIG2, TREE_BUDGET, init_rows=rows), c.points_rows(rows[:40])))


@register("tree_build_f32_pdfs", "tree", _tree_dims)
def tree_build_f32_pdfs(c, s):
    P = cloud(s.size)
    c.set_points(P)
    c.tree_set_precision(np.float32)
    try:
        return flat(c.tree_build(s.L, LS, LD, tree_init(P, s.L, 75), SIG2, TREE_BUDGET, want_leaf=False))
    finally:
        c.tree_set_precision(np.float64)


# ---- the tree: registration against uploaded node tables -------------------------------------------------------------------------

def _reg_dims(s):
    g = reg_case(s.size)
    return {"n": len(g.target), "T": g.T}


def _resident(c, size, w=None):
    g = reg_case(size)
    c.tree_set_nodes(g.L, g.pi, g.mu, g.cov)
    c.tree_set_target(g.target)
    if w is not None:
        c.tree_set_target_weights(w)
    return g


def _registration(c, g):
    estep = c.tree_reg_estep(g.T, None, None, 1.0, LAMBDA_C)
    normal = c.tree_reg_normal(I3, Z3, 1.0, LAMBDA_C)
    reg = c.tree_register(I3, Z3, 1.0, LAMBDA_C, REG_BUDGET, REG_TOL, want_trace=True)
    score = c.tree_score(reg[0], reg[1], 1.0, LAMBDA_C)
    return estep, normal, reg, score


@register("tree_register", "tree", _reg_dims)
def tree_register(c, s):
    """set_nodes + set_target, the registration E-step, the normal equations, the library's loop (host solve), the score"""
    return flat(_registration(c, _resident(c, s.size)))


@register("tree_register_device_solve", "tree", _reg_dims)
def tree_register_device_solve(c, s):
    _resident(c, s.size)
    with c.config(reg_device_solve=1):
        return flat(c.tree_register(I3, Z3, 1.0, LAMBDA_C, REG_BUDGET, REG_TOL, want_trace=True))


@register("tree_register_gated", "tree", _reg_dims)
def tree_register_gated(c, s):
    """under a Mahalanobis gate, which the op takes off again"""
    g = _resident(c, s.size)
    c.tree_set_reg_gate(CHI2_3_999)
    try:
        return flat((_registration(c, g), c.tree_get_reg_gate()))
    finally:
        c.tree_set_reg_gate(np.inf)


@register("tree_register_weighted", "tree", _reg_dims)
def tree_register_weighted(c, s):
    """under target weights, which stay in force when the op ends"""
    g = reg_case(s.size)
    return flat(_registration(c, _resident(c, s.size, weights(len(g.target), 25))))


@register("tree_multistart", "tree", lambda s: dict(_reg_dims(s), K=s.R))
def tree_multistart(c, s):
    _resident(c, s.size)
    rot, t = poses(s.R)
    reg = c.tree_register_multi(rot, t, 1.0, LAMBDA_C, REG_BUDGET, REG_TOL, want_trace=True)
    return flat((reg, c.tree_score_multi(reg[0], reg[1], 1.0, LAMBDA_C)))


@register("tree_steps", "tree", lambda s: {"n": len(reg_case(s.size).points), "T": reg_case(s.size).T})
def tree_steps(c, s):
    """the stand-alone E-step, M-step and log-likelihood of level 1 on the uploaded node tables (they drop the resident tree)"""
    g = reg_case(s.size)
    c.set_points(g.points)
    parent = np.random.RandomState(1).randint(-1, g.T // 8 - 1, size=len(g.points)).astype(np.int32)
    m0, m1, m2, cur = c.tree_estep(g.pi, g.mu, g.cov, parent)
    nodes = c.tree_mstep(m0, m1, m2, 8, 72, len(g.points), LD, g.pi, g.mu, g.cov)
    return flat((m0, m1, m2, cur, nodes, c.tree_loglik(nodes[0], nodes[1], nodes[2], 8, 72)))


# ---- the forest: B clouds / pairs per launch set ----------------------------------------------------------------------------------

def _forest_dims(s, one_point=True):
    return {"n": n_of(s.size, one_point), "T": n_total(s.L), "B": s.B}


@register("forest_build", "forest", _forest_dims)
def forest_build(c, s):
    """set_points_batch from float32 rows with source weights (one member unweighted, one of one point), the build from row
    numbers with its q traces, and a member's tables read back"""
    clouds = members(s.size, "float32")
    arrs = c.set_points_batch(clouds)
    c.tree_set_source_weights_batch([weights(len(P), 90 + b) if b != 1 else None for b, P in enumerate(clouds)])
    counts = [len(a) for a in arrs]
    rows = np.stack([rows_of(n, n_total(s.L), 100 + b) for b, n in enumerate(counts)])
    built = c.tree_build_batch(counts, s.L, LS, LD, None, SIG2, TREE_BUDGET, want_trace=True, init_rows=rows)
    return flat((built, c.tree_get_nodes_batch(s.B - 1, s.L)))


FOREST_INIT_SEED = 110


def forest_targets(size):
    """every second point of each source, moved by a few degrees and millimetres (another motion per pair)"""
    return [moved(P[::2], 3.0 + 2.0 * b, [0.2, 1.0, 0.1 * b], [0.003, -0.002, 0.001 * b])
            for b, P in enumerate(members(size, "float64", one_point=False))]


def _forest_pairs(c, s, f32_targets=False, target_weights=False):
    clouds = members(s.size, "float64", one_point=False)
    arrs = c.set_points_batch(clouds)
    built = c.tree_build_batch([len(a) for a in arrs], s.L, LS, LD,
                               np.stack([tree_init(P, s.L, FOREST_INIT_SEED + b) for b, P in enumerate(clouds)]), SIG2, TREE_BUDGET)
    targets = forest_targets(s.size)
    if f32_targets:
        targets = [a.astype(np.float32) for a in targets]
    c.tree_set_targets_batch(targets)
    if target_weights:
        c.tree_set_target_weights_batch([weights(len(a), 120 + b) if b != 1 else None for b, a in enumerate(targets)])
    return built


@register("forest_register", "forest", lambda s: dict(_forest_dims(s, False), R=s.R))
def forest_register(c, s):
    """build_batch from explicit means, float64 targets, the batched registration and score, R hypotheses over the pairs"""
    built = _forest_pairs(c, s)
    reg = c.tree_register_batch(np.tile(I3, (s.B, 1, 1)), np.zeros((s.B, 3)), 1.0, LAMBDA_C, REG_BUDGET, REG_TOL, want_trace=True)
    score = c.tree_score_batch(reg[0], reg[1], 1.0, LAMBDA_C)
    pair = np.random.RandomState(6).randint(s.B, size=s.R)
    rot, t = poses(s.R, 7)
    multi = c.tree_register_batch_multi(pair, rot, t, 1.0, LAMBDA_C, REG_BUDGET, REG_TOL, want_trace=True)
    score_multi = c.tree_score_batch_multi(pair, multi[0], multi[1], 1.0, LAMBDA_C)
    return flat((built, reg, score, multi, score_multi, c.tree_get_nodes_batch(0, s.L)))


@register("forest_register_weighted", "forest", lambda s: _forest_dims(s, False))
def forest_register_weighted(c, s):
    """float32 targets under weights (one pair unweighted), the 6 x 6 solves on the device"""
    _forest_pairs(c, s, f32_targets=True, target_weights=True)
    with c.config(reg_device_solve=1):
        reg = c.tree_register_batch(np.tile(I3, (s.B, 1, 1)), np.zeros((s.B, 3)), 1.0, LAMBDA_C, REG_BUDGET, REG_TOL, want_trace=True)
    return flat((reg, c.tree_score_batch(None, None, 1.0, LAMBDA_C)))


# ---- voxel-grid down-sample and its hand-overs ---------------------------------------------------------------------------------

@register("voxel_down_sample", "voxel", _voxel_dims)
def voxel_down_sample(c, s):
    """one cloud from float64 and from float32 rows, the batch from both, the result fetched once more, its description"""
    c64, c32 = _voxel_clouds(s.size), _voxel_clouds(s.size, "float32")
    one64 = c.voxel_down_sample(c64[0], s.voxel)
    one32 = c.voxel_down_sample(c32[0], s.voxel)
    batch32 = c.voxel_down_sample_batch(c32, s.voxel)
    batch64 = c.voxel_down_sample_batch(c64, s.voxel)
    m, n, _ = c.voxel_result_info()                       # (the serial number counts the context's down-samples: history)
    return flat((one64, one32, batch32, batch64, c.voxel_down_sample_get(), m, n))


@register("voxel_hand_over", "voxel", _voxel_dims)
def voxel_hand_over(c, s):
    """the four hand-overs, each followed by a consumer of what it made resident: a weighted build and the flat statistics,
    the normal equations against that tree, the forest build, the batched score"""
    vcs = c.voxel_down_sample_batch(_voxel_clouds(s.size), s.voxel, download=False).members()
    T = n_total(s.L)
    c.set_points_from_voxels(vcs[0], tree_weights=True, flat_weights=True)
    built = c.tree_build(s.L, LS, LD, None, SIG2, TREE_BUDGET, init_rows=rows_of(len(vcs[0]), T, 130))
    X = c.points_download()
    inv, mu, w = _estep_params(X, s.J, 8)
    stats = c.flat_stats(inv, mu, w, "diag", "W")
    c.tree_set_target_from_voxels(vcs[-1], weighted=True)
    normal = c.tree_reg_normal(None, None, 1.0, LAMBDA_C)
    counts = c.set_points_batch_from_voxels(vcs, weighted=True)
    rows = np.stack([rows_of(n, T, 140 + b) for b, n in enumerate(counts)])
    forest = c.tree_build_batch(counts, s.L, LS, LD, None, SIG2, TREE_BUDGET, init_rows=rows)
    c.tree_set_targets_batch_from_voxels(vcs[::-1], weighted=True)
    return flat((built, X, stats, normal, forest, c.tree_score_batch(None, None, 1.0, LAMBDA_C)))


# ---- L2 GMMReg ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def l2_case(size):
    """(pairs, pair ids [R], rotations [R,3,3], translations [R,3], sigmas [R]): random centres in the unit cube, positive
    weights (the mixtures of test_gmmreg_resident_gpu.py)"""
    s = SHAPES[size]
    rs = np.random.RandomState(7)
    pairs = tuple((rs.rand(js, 3), 0.1 + rs.rand(js), rs.rand(jt, 3), 0.1 + rs.rand(jt)) for js, jt in s.l2)
    ids = rs.randint(len(pairs), size=s.l2_R).astype(np.int32)
    rot, t = poses(s.l2_R, 8)
    t = t + 0.5 - rot @ np.full(3, 0.5)                   # (rotations about the cube's centre: the mixtures overlap)
    return pairs, ids, rot, t, rs.uniform(0.1, 0.4, s.l2_R)


@register("l2", "l2", lambda s: {"Js": max(p[0] for p in s.l2), "Jt": max(p[1] for p in s.l2), "B": len(s.l2), "R": s.l2_R})
def l2(c, s):
    """l2_set_pairs + l2_cost, and the Gauss transform of the largest pair (value and gradient rows)"""
    pairs, ids, rot, t, sigma = l2_case(s.size)
    c.l2_set_pairs(pairs)
    cost = c.l2_cost(ids, rot, t, sigma)
    mu_s, _, mu_t, phi_t = pairs[min(1, len(pairs) - 1)]
    gt = c.gauss_transform(mu_t, mu_s, np.vstack([phi_t[None, :], (phi_t[:, None] * mu_t).T]), np.sqrt(2.0) * 0.2)
    return flat((cost, gt))


# ---- resident handles -------------------------------------------------------------------------------------------------------------

def handles(c):
    """points_create / points_bind of two clouds of different size, a tree build and a flat fit on each, the smaller first
    and once more after the larger; the handles are destroyed when the op ends (nothing is bound afterwards)"""
    big, small = cloud("large"), cloud("small", "float32")
    h_big, h_small = c.points_create(big), c.points_create(small)
    out = []
    try:
        for h, P, L, J in ((h_small, small, 2, 8), (h_big, big, 3, 100), (h_small, small, 2, 8)):
            c.points_bind(h)
            out.append(c.tree_build(L, LS, LD, tree_init(np.asarray(P, dtype=np.float64), L, 76), SIG2, TREE_BUDGET))
            mu, w, cov = flat_init(P, J, 9)
            out.append(c.flat_train(FLAT_ITERS, 0.0, mu, cov, w, "diag", "W"))
        out.append(c.points_download(h_small))
        out.append(c.points_download())
    finally:
        c.points_destroy(h_big)
        c.points_destroy(h_small)
    return flat(out)


OPS["handles"] = Op(handles, "handles", "mixed", {})


# ---- the orders of test_context_history_gpu.py ------------------------------------------------------------------------------------

SHUFFLE_SEEDS = (20261, 20262, 20263)


def of_size(size):
    """the ops of one size in table order; the mixed op (handles) closes each list"""
    return [name for name, op in OPS.items() if op.size in (size, "mixed")]


def grow_shrink_grow():
    return of_size("large") + of_size("small") + of_size("large")


def shuffled(seed):
    names = sorted(OPS)
    np.random.RandomState(seed).shuffle(names)
    return names


# ---- the entries of include/hgmm.h, and those no op has to reach --------------------------------------------------------------------

def declared_entries():
    """every function include/hgmm.h declares"""
    import re
    with open(HEADER) as f:
        text = f.read()
    return sorted(set(re.findall(r"^(?:const\s+)?\w+\s*\*?\s*(hgmm_\w+)\s*\(", text, re.M)))


EXCLUDED = {
    # the life of a context and of the library: what the tests stand on, not what they compare
    "hgmm_version": "library constant, no context",
    "hgmm_device_count": "device enumeration, no context",
    "hgmm_create": "creates the contexts the module runs on; it is reached outside any op",
    "hgmm_destroy": "ends a context; there is no later call whose bits it could change",
    "hgmm_last_error": "text of the last failure, read by the wrapper on a refusal only",
    "hgmm_device_info": "device description, no numerical state",
    "hgmm_synchronize": "drains the stream; every op ends on a call that synchronises",
    # raw memory: the ops reach these through the device arrays; none is an entry with a result of its own
    "hgmm_alloc": "raw allocation (the wrapper's device arrays)",
    "hgmm_free": "raw allocation (the wrapper's device arrays)",
    "hgmm_h2d": "raw copy", "hgmm_d2h": "raw copy", "hgmm_d2d": "raw copy",
    "hgmm_event_record": "stream events: ordering, no numerical result",
    "hgmm_event_wait": "stream events: ordering, no numerical result",
    # communicators: out of scope (multi-rank entries), tests/test_multirank_gpu.py
    "hgmm_comm_unique_id": "communicator", "hgmm_comm_init_rank": "communicator", "hgmm_comm_destroy": "communicator",
    "hgmm_comm_init_host": "communicator", "hgmm_comm_init_ipc": "communicator", "hgmm_comm_allreduce_f64": "communicator",
    "hgmm_comm_stats": "communicator counters",
    # measurement aids
    "hgmm_profile_enable": "profiling", "hgmm_profile_reset": "profiling", "hgmm_profile_get": "profiling",
    "hgmm_fullcov_phase_clocks": "profiling (cycle counters of one workgroup)",
    "hgmm_util_fill_f32": "bandwidth probe into a caller's buffer",
    "hgmm_pace_info": "the store pacer's learnt rate: timing-dependent by design, changes no result",
    "hgmm_pace_reset": "the store pacer's learnt rate: timing-dependent by design, changes no result",
    # configuration: set / get are reached by the ops that select a path; the enumeration has no state
    "hgmm_config_count": "config enumeration", "hgmm_config_name": "config enumeration",
    "hgmm_kmeans_center_f64": "host-only arithmetic, takes no context",
}
