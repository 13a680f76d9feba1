"""Every entry is held to a FRESH context's bits after any call history on ONE long-lived context.

In production ``default_context()`` lives for the whole process: one hgmm_ctx carries the node tables, the shared ``t_parent`` /
``t_current`` / ``scratch`` buffers, the fixed-point moment sums (zero only by the MomqScope invariant), the arrival counters
and flags ("every launch leaves its counters at zero"), a pinned hand-over block that only grows, buffers that ``ensure()``
only grows (a small call after a large one works in a buffer whose tail holds the large call's data) and sticky host words.
Every other module of the suite makes a context of its own and runs its own family on it; here all families share one.

The reference of every comparison is the op (tests/_history_ops.py) on a fresh ``Context(0)``, closed straight afterwards.
It runs twice: where the two runs agree bit for bit the op is BITWISE and every later result must be those bits
(``same_bits``: shape, type and every byte).  An op that is not must be listed in ORDER_DEPENDENT with the sentence of
include/hgmm.h that allows it and the tolerance of the existing test of that entry; the list is empty -- the header promises
fixed orders of summation everywhere ("no floating-point atomics", "two calls return the same bits").

    (a) grow, shrink, grow: all large ops, all small ops, all large ops again
    (b) three seeded shuffles of the whole table
    (c) after the last shuffle one op per family and size against the float64 oracle, at the tolerances of the existing
        tests named beside each check: the module is not a comparison of the code with itself
    (d) split loops (flat_train_begin / _step / _end, a registration budget in two calls, l2_cost on resident pairs) with
        foreign-family work between the pieces == the uninterrupted loop
    (e) the documented invalidations ("X drops Y's state"): Y's consumer after X refuses by name or returns fresh bits
    (f) sticky settings (tree precision, registration gate, every path option) leave no trace once taken back
    (g) a refused call of every family between two ops of other families changes neither neighbour
    (h) the entries the ops reached plus EXCLUDED (entry -> reason) are exactly the entries include/hgmm.h declares

The tests run in file order on the module's context; each also runs alone.  profiles/context_history.md has the op list,
the invalidation table and the outcome of breaking the MomqScope invariant on purpose.
"""
import re

import numpy as np
import pytest

import _history_ops as H
from oracle import flat_em, hgmm_tree, kmeans as okm

pytestmark = pytest.mark.gpu

# op -> (sentence of include/hgmm.h that makes it order-dependent, existing test whose tolerance it is held to).
# Nothing is listed: every op of the table returns the same bits on two fresh contexts.
ORDER_DEPENDENT = {}

LAST = {}                 # op -> its latest result on the long-lived context (what (c) compares with the oracle)


@pytest.fixture(scope="module")
def refs():
    """op -> (result on a fresh context, whether a second fresh context returned the same bits, their first difference)"""
    out = {}
    for name in H.OPS:
        a, b = H.run_fresh(name), H.run_fresh(name)
        for x in a:
            x.setflags(write=False)
        out[name] = (a, H.same_bits(a, b), H.first_difference(b, a))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = H.recording_context()
    yield c
    c.close()


def fresh(fn):
    """fn(context) on a context of its own"""
    c = H.recording_context()
    try:
        return fn(c)
    finally:
        c.close()


def check(name, out, refs, where=""):
    want, bitwise, _ = refs[name]
    assert bitwise or name in ORDER_DEPENDENT, "%s is not bitwise on fresh contexts and names no tolerance" % name
    diff = H.first_difference(out, want)
    assert diff is None, "%s%s differs from its fresh context: %s" % (name, where, diff)


def run_order(ctx, refs, order, tag):
    prev = "(the state the test found)"
    for at, name in enumerate(order):
        out = H.OPS[name].fn(ctx)
        LAST[name] = out
        check(name, out, refs, " (%s, op %d, after %s)\norder: %s" % (tag, at, prev, " ".join(order)))
        prev = name


def test_fresh_contexts_agree_bit_for_bit(refs):
    """the classification: bitwise, or documented as order-dependent"""
    loose = {name: r[2] for name, r in refs.items() if not r[1]}
    assert set(loose) <= set(ORDER_DEPENDENT), "two fresh contexts disagree, and the header does not say they may: %s" % loose
    assert all(len(r[0]) > 0 for r in refs.values())


# ---- (a), (b) ----------------------------------------------------------------------------------------------------------------

def test_grow_shrink_grow(ctx, refs):
    run_order(ctx, refs, H.grow_shrink_grow(), "grow, shrink, grow")


@pytest.mark.parametrize("seed", H.SHUFFLE_SEEDS)
def test_seeded_shuffle(ctx, refs, seed):
    run_order(ctx, refs, H.shuffled(seed), "shuffle %d" % seed)


# ---- (c) held to the oracle --------------------------------------------------------------------------------------------------

def oracle_flat(size, out):
    """test_flat_gpu.test_train_bunny_20_iterations, flavour W: lls within 2e-5, live means within 2e-5, live weights 1e-5"""
    s = H.SHAPES[size]
    X = H.cloud(size, "float32")
    mu0, w0, cov0 = H.flat_init(X, s.J)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    inv, mu, w, cov, lls, conv = out
    o_inv, o_mu, o_w, o_cov, o_lls, _ = flat_em.train(f64(X), H.FLAT_ITERS, 0.0, f64(mu0), f64(cov0), f64(w0), "diag", "W")
    live = o_w > 1e-4
    d_ll, d_mu = np.abs(lls - np.array(o_lls)).max(), np.abs(mu - o_mu)[live].max()
    print("flat %s: |lls - oracle| %.3g, live means %.3g" % (size, d_ll, d_mu))
    assert len(lls) == H.FLAT_ITERS and d_ll <= 2e-5 and d_mu <= 2e-5
    np.testing.assert_allclose(w[live], o_w[live], rtol=0, atol=1e-5)


def oracle_kmeans(size, out):
    """test_kmeans_gpu.test_seeding_and_step_vs_oracle: seeds identical, one assignment identical in labels and counts,
    distances rtol 1e-13, sums atol 1e-11, inertia rtol 1e-12; test_kmeans_lloyd_gpu.test_whole_loop_vs_oracle: the loop's
    iteration count, centres atol 1e-12"""
    s = H.SHAPES[size]
    Xc = H._centred(H.cloud(size))
    ids, seeds, centres, n_iter, strict, sums, counts, inertia, changed, labels, d2 = out
    o_seeds, o_ids = okm.kmeans_plusplus(Xc, s.k, np.random.RandomState(H.KM_SEED))
    assert np.array_equal(ids, o_ids) and np.array_equal(seeds, o_seeds)
    o_labels, _, o_centres, o_iter = okm.lloyd(Xc, o_seeds, H.KM_ITERS, 0.0)
    assert int(n_iter) == o_iter
    np.testing.assert_allclose(centres, o_centres, rtol=0, atol=1e-12)
    lab, dist = okm.assign(Xc, centres)
    assert np.array_equal(labels, lab) and np.array_equal(counts, np.bincount(lab, minlength=s.k))
    np.testing.assert_allclose(d2, dist, rtol=1e-13, atol=1e-30)
    o_sums = np.zeros((s.k, 3))
    np.add.at(o_sums, lab, Xc)
    np.testing.assert_allclose(sums, o_sums, rtol=0, atol=1e-11)
    np.testing.assert_allclose(inertia, dist.sum(), rtol=1e-12)


def oracle_fullcov(size, out):
    """test_fullcov_gpu.test_fullcov_vs_oracle: q rtol 1e-9 atol 1e-6, labels identical, pi 1e-9 / 1e-13, mu 1e-8 / 1e-11,
    cov 1e-6 / 1e-14"""
    s = H.SHAPES[size]
    P = H.cloud(size)
    pi, mu, cov, labels, q = out[:5]
    o_pi, o_mu, o_cov, o_q, o_cur = hgmm_tree.build_flat_fullcov(P, s.Jf, H.FULL_LS, H.LD, H.rows_of(len(P), s.Jf, 9),
                                                                 H.FULL_SIG2, max_iters=H.FULL_ITERS)
    assert len(q) == len(o_q)
    np.testing.assert_allclose(q, o_q, rtol=1e-9, atol=1e-6)
    assert np.array_equal(labels, o_cur)
    np.testing.assert_allclose(pi, o_pi, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(mu, o_mu, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(cov, o_cov, rtol=1e-6, atol=1e-14)


def built_against_oracle(tables, iters, q, leaf, P, L, init_seed):
    """test_tree_gpu.test_build_bunny_subsample_L4_vs_oracle: iterations identical, q rtol 1e-9 atol 1e-6, leaves identical,
    pi 1e-9 / 1e-13, mu 1e-9 / 1e-12, cov 1e-6 / 1e-14"""
    pi, mu, cov = tables
    o_pi, o_mu, o_cov, tr = hgmm_tree.build_tree(P, L, H.LS, H.LD, H.rows_of(len(P), H.n_total(L), init_seed), H.SIG2, H.TREE_BUDGET)
    assert list(iters) == list(tr.iters_per_level)
    if q is not None:
        np.testing.assert_allclose(q, tr.q, rtol=1e-9, atol=1e-6)
    if leaf is not None:
        assert np.array_equal(leaf, tr.current_idx_per_level[-1])
    np.testing.assert_allclose(pi, o_pi, rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(mu, o_mu, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cov, o_cov, rtol=1e-6, atol=1e-14)


def registered_against_oracle(rot, t, done, status, target, pi, mu, cov, L):
    """test_tree_gpu.test_registration_loop_inside_the_library (and __graft_entry__.smoke): the library's loop stops where the
    oracle's does and ends on its transformation to 1e-8 (the oracle returns the inverse, the entry the forward one)"""
    o_rot, o_t, _, trace = hgmm_tree.register(target, pi, mu, cov, L, H.LAMBDA_C, H.REG_BUDGET, H.REG_TOL)
    print("registration: %d iterations (oracle %d), status %d, |rot - oracle| %.3g, |t - oracle| %.3g"
          % (done, len(trace), status, np.abs(rot.T - o_rot).max(), np.abs(-rot.T @ t - o_t).max()))
    assert int(status) in (0, 1) and int(done) == len(trace)
    np.testing.assert_allclose(rot.T, o_rot, rtol=0, atol=1e-8)
    np.testing.assert_allclose(-rot.T @ t, o_t, rtol=0, atol=1e-8)


def oracle_tree(size, out):
    """the build (tree_build_<size>) and the registration (tree_register_<size>); the registration E-step's moments as
    test_tree_gpu.test_registration_estep_and_loop_match_reference holds them: rtol 1e-9, atol 1e-12"""
    build, reg = out
    s = H.SHAPES[size]
    pi, mu, cov, leaf, iters, q = build[:6]
    built_against_oracle((pi, mu, cov), iters, q, leaf, H.cloud(size), s.L, 72)
    g = H.reg_case(size)
    for x, y in zip(reg[:3], hgmm_tree.reg_e_step(g.target, g.pi, g.mu, g.cov, g.L, H.LAMBDA_C)):
        np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-12)
    rot, t, done, _, status = reg[6:11]
    registered_against_oracle(rot, t, done, status, g.target, g.pi, g.mu, g.cov, g.L)


def oracle_forest(size, out):
    """a member of the forest is its serial build (test_tree_batch_gpu.test_build_batch_is_bitwise_the_serial_build) and is
    held to the oracle as that is; its pair's registration against the tables the device built, as smoke() does"""
    s = H.SHAPES[size]
    b = min(1, s.B - 1)
    P = H.members(size, "float64", one_point=False)[b]
    pi, mu, cov, iters = out[:4]
    built_against_oracle((pi[b], mu[b], cov[b]), iters[b], None, None, P, s.L, H.FOREST_INIT_SEED + b)
    rot, t, done, _, status = out[4:9]
    registered_against_oracle(rot[b], t[b], done[b], status[b], H.forest_targets(size)[b], pi[b], mu[b], cov[b], s.L)


def oracle_voxel(size, out):
    """test_voxel_gpu.test_scan / test_batch_members_are_their_serial_calls: pointcloud_io.voxel_down_sample is the
    definition and the device has its bits"""
    from hgmm_amd.pointcloud_io import voxel_down_sample
    s = H.SHAPES[size]
    clouds = H._voxel_clouds(size)
    B = len(clouds)
    want = [voxel_down_sample(P, s.voxel, True) for P in clouds]
    got = [(out[0], out[1])] + [(out[4 + 2 * B + 2 * b], out[5 + 2 * B + 2 * b]) for b in range(B)]
    for (cent, cnt), (o_cent, o_cnt) in zip(got, [want[0]] + want):
        assert cnt.dtype == np.int64 and np.array_equal(cnt, o_cnt)
        assert cent.shape == o_cent.shape and cent.tobytes() == np.ascontiguousarray(o_cent).tobytes()
    if size == "large":
        assert 200 <= len(want[0][1]) <= 999, len(want[0][1])


def oracle_l2(size, out):
    """test_gmmreg_resident_gpu.test_tile_edges_within_the_summation_bound: each of the 13 outputs within
    (Js + Jt + 16) 2^-52 sum |terms| of the host's RigidCostFunction arithmetic (compute_l2_dist, g.T @ mu_source)"""
    from hgmm_amd.gmmreg_gpu import cost_functions as cf, transforms as tf
    pairs, ids, rots, ts, sigmas = H.l2_case(size)
    worst = 0.0
    for r in range(len(ids)):
        mu_s, phi_s, mu_t, phi_t = pairs[ids[r]]
        sigma = sigmas[r]
        y = mu_s @ rots[r].T + ts[r]
        f, g = cf.compute_l2_dist(y, phi_s, mu_t, phi_t, sigma)
        value = np.concatenate([[f], g.sum(axis=0), (g.T @ mu_s).ravel()])
        e = tf.kernel_matrix(mu_t, y, np.sqrt(2.0) * sigma)
        t0 = phi_s[:, None] * (phi_t / np.power(2.0 * np.pi * sigma ** 2, 1.5))[None, :] * e
        ga = np.stack([t0 * (np.abs(y[:, a, None]) + np.abs(mu_t[None, :, a])) for a in range(3)]) / (2.0 * sigma ** 2)
        terms = np.concatenate([[t0.sum()], ga.sum(axis=(1, 2)), np.einsum('aij,ib->ab', ga, np.abs(mu_s)).ravel()])
        bound = (len(mu_s) + len(mu_t) + 16) * 2.0 ** -52 * terms
        worst = max(worst, float((np.abs(out[0][r] - value) / bound).max()))
        assert (np.abs(out[0][r] - value) <= bound).all(), (r, out[0][r], value)
    print("l2 %s: largest |device - host| / bound = %.3f" % (size, worst))


ORACLES = {"flat": (oracle_flat, "flat_fit_diag"), "kmeans": (oracle_kmeans, "kmeans"), "fullcov": (oracle_fullcov, "fullcov_fit"),
           "tree": (oracle_tree, ("tree_build", "tree_register")), "forest": (oracle_forest, "forest_register"),
           "voxel": (oracle_voxel, "voxel_down_sample"), "l2": (oracle_l2, "l2")}


def test_every_numerical_family_has_an_oracle():
    assert set(ORACLES) == set(H.FAMILIES) - {"handles"}            # (handles: how a cloud is named, no arithmetic of its own)


@pytest.mark.parametrize("size", H.SIZES)
@pytest.mark.parametrize("family", sorted(ORACLES))
def test_held_to_the_oracle_after_the_histories(ctx, family, size):
    """what the long-lived context returned LAST -- after the third shuffle when the module runs as a whole"""
    fn, ops = ORACLES[family]

    def last(base):
        name = "%s_%s" % (base, size)
        return LAST[name] if name in LAST else H.OPS[name].fn(ctx)
    fn(size, last(ops) if isinstance(ops, str) else tuple(last(o) for o in ops))


# ---- (d) split loops with foreign work in between --------------------------------------------------------------------------------

# flat_train_batch[_weighted / _voxels] "LEFT ALONE ... the serial train loop (a hgmm_flat_train_begin ... _end in progress
# included)", hgmm_l2_set_pairs "Nothing else of the context is touched", the voxel down-sample "works in buffers of its own":
# none of these binds a cloud (a new resident cloud ends the loop and drops the tree: see (e))
KEEPS_THE_CLOUD = ["flat_batch_large", "l2_large", "voxel_down_sample_large", "flat_batch_voxels_small", "flat_batch_small",
                   "l2_small", "voxel_down_sample_small", "flat_batch_voxels_large"]


def foreign(ctx, refs, names, at):
    name = names[at % len(names)]
    check(name, H.OPS[name].fn(ctx), refs, " (as foreign work inside a split loop)")


@pytest.mark.parametrize("size", H.SIZES)
def test_split_flat_loop_with_foreign_work_between_the_steps(ctx, refs, size):
    s = H.SHAPES[size]
    X = H.cloud(size, "float32")
    mu, w, cov = H.flat_init(X, s.J, 5)
    ctx.set_points(X)
    ctx.flat_train_begin(0.0, mu, cov, w, "diag", "W", lls_capacity=16)
    for at, iters in enumerate((1, 1, 3)):
        foreign(ctx, refs, KEEPS_THE_CLOUD, 3 * at + (size == "small"))
        ctx.flat_train_step(iters)
        foreign(ctx, refs, KEEPS_THE_CLOUD, 3 * at + 4)
    check("flat_split_loop_%s" % size, H.flat(ctx.flat_train_end()), refs, " with foreign work between its steps")


def split_registration(c, size, device_solve, between=lambda at: None):
    """budgets 3 + 3 with the pose and q handed on (test_tree_reg_depth_gpu.test_split_budget_is_one_call... is the
    uninterrupted form) -> what ONE call with budget 6 returns: pose, iterations, q, status, trace"""
    H._resident(c, size)
    with c.config(reg_device_solve=device_solve):
        between(0)
        r1, t1, d1, q1, s1, tr1 = c.tree_register(H.I3, H.Z3, 1.0, H.LAMBDA_C, 3, 0.0, want_trace=True)
        between(1)
        r2, t2, d2, q2, s2, tr2 = c.tree_register(r1, t1, 1.0, H.LAMBDA_C, 3, 0.0, q_prev=q1, want_trace=True)
    return H.flat((r2, t2, d1 + d2, q2, s2, np.concatenate([tr1, tr2])))


@pytest.mark.parametrize("device_solve", [0, 1])
@pytest.mark.parametrize("size", H.SIZES)
def test_split_registration_budget_with_foreign_work_between_the_calls(ctx, refs, size, device_solve):
    def whole(c):
        H._resident(c, size)
        with c.config(reg_device_solve=device_solve):
            return H.flat(c.tree_register(H.I3, H.Z3, 1.0, H.LAMBDA_C, 6, 0.0, want_trace=True))
    one_call = fresh(whole)
    assert int(one_call[2]) == 6 and int(one_call[4]) == 0
    split = split_registration(ctx, size, device_solve, lambda at: foreign(ctx, refs, KEEPS_THE_CLOUD, 2 * at + device_solve))
    assert H.first_difference(split, one_call) is None, H.first_difference(split, one_call)


# every family may run between two l2_cost calls: the resident pairs are replaced by hgmm_l2_set_pairs alone
ANY_FAMILY = ["tree_register_large", "flat_fit_diag_large", "fullcov_fit_large", "forest_register_large", "kmeans_batch_large",
              "voxel_hand_over_large", "tree_steps_small", "flat_estep_small"]


@pytest.mark.parametrize("size", H.SIZES)
def test_l2_cost_calls_with_other_families_between_them(ctx, refs, size):
    pairs, ids, rot, t, sigma = H.l2_case(size)
    want = refs["l2_%s" % size][0][0]
    ctx.l2_set_pairs(pairs)
    for at in range(len(ANY_FAMILY)):
        cost = ctx.l2_cost(ids, rot, t, sigma)
        assert cost.tobytes() == want.tobytes(), "l2_cost after %s" % (ANY_FAMILY[at - 1] if at else "l2_set_pairs")
        foreign(ctx, refs, ANY_FAMILY, at)
    assert ctx.l2_cost(ids, rot, t, sigma).tobytes() == want.tobytes()


# ---- (e) documented invalidations: the named refusal or fresh bits, never a third thing -----------------------------------------

STATE = r"^hgmm call failed \(-3\): "
NO_TREE = STATE + r"registration( E-step)?: no tree"


def _tree_and_target(c):
    H._resident(c, "large")


def _normal(c):
    return H.flat(c.tree_reg_normal(None, None, 1.0, H.LAMBDA_C))


def _forest(c):
    clouds = H.members("large")
    return [len(a) for a in c.set_points_batch(clouds, weights=[H.weights(len(P), 70 + b) for b, P in enumerate(clouds)])]


def _weighted_cloud(c):
    P = H.cloud("small", "float32")
    c.set_points(P)
    c.flat_set_weights(H.weights(len(P), 21))
    c.tree_set_source_weights(H.weights(len(P), 22))
    c.kmeans_step(np.asarray(P[:3], dtype=np.float64), reset_labels=True)


def _flat_stats(c):
    inv, mu, w = H._estep_params(H.cloud("small", "float32"), 8, 6)
    return H.flat(c.flat_stats(inv, mu, w, "diag", "W"))


def _same_cloud_again(c):
    c.set_points(H.cloud("small", "float32"))


def _weighted_target(c):
    H._resident(c, "small", H.weights(len(H.reg_case("small").target), 25))


def _loop_in_progress(c):
    X = H.cloud("small", "float32")
    mu, w, cov = H.flat_init(X, 8, 5)
    c.set_points(X)
    c.flat_train_begin(0.0, mu, cov, w, "diag", "W", lls_capacity=16)
    c.flat_train_step(1)


def _voxel_member(c):
    c._kept = c.voxel_down_sample_batch(H._voxel_clouds("large"), H.SHAPES["large"].voxel, download=False).member(0)


def _bound_handle(c):
    c._kept = c.points_create(H.cloud("small", "float32"))
    c.points_bind(c._kept)


def _fit_small(c):
    mu, w, cov = H.flat_init(H.cloud("small", "float32"), 8)
    return H.flat(c.flat_train(2, 0.0, mu, cov, w, "diag", "W"))


def _fullcov_batch(c):
    counts = [len(P) for P in H.members("large")]
    rows = np.stack([H.rows_of(n, 3, 80 + b) for b, n in enumerate(counts)])
    return H.flat(c.fullcov_fit_batch(counts, 3, H.FULL_LS, H.LD, init_rows=rows, sig2=H.FULL_SIG2, max_iters=3))


# name -> (Y's state, X, Y's consumer, the refusal's text, or None where the consumer must work: then its bits are those of
#          `X alone` -- the last column -- on a fresh context)
INVALIDATIONS = {
    # hgmm_fullcov_fit and the stand-alone steps write the node tables: "tables no longer describe a complete L-level tree"
    "a full-covariance fit drops the resident tree":
        (_tree_and_target, lambda c: H.OPS["fullcov_fit_small"].fn(c), _normal, NO_TREE, None),
    "tree_estep / mstep / loglik drop the resident tree":
        (_tree_and_target, lambda c: H.OPS["tree_steps_small"].fn(c), _normal, NO_TREE, None),
    # hgmm.h, hgmm_flat_set_weights / hgmm_tree_set_source_weights: "Whatever changes the resident cloud drops them"
    "a new cloud drops the flat weights": (_weighted_cloud, _same_cloud_again, _flat_stats, None, _same_cloud_again),
    "a new cloud drops the source weights":
        (_weighted_cloud, _same_cloud_again, lambda c: c.fullcov_fit(3, 1.0, 1e-4, np.zeros((3, 3)), 0.001, 2, weighted=True),
         STATE + r"\w+: no source weights are resident", None),
    "a new cloud drops the KMeans labels":
        (_weighted_cloud, _same_cloud_again, lambda c: c.kmeans_labels(), STATE + "kmeans: no assignment on the device", None),
    "a new cloud drops the resident tree":
        (_tree_and_target, _same_cloud_again, _normal, NO_TREE, None),
    "a new cloud ends a flat_train_begin in progress":
        (_loop_in_progress, _same_cloud_again, lambda c: c.flat_train_step(1),
         STATE + "hgmm_flat_train_step before hgmm_flat_train_begin", None),
    # hgmm_tree_set_target_weights: "uploading a new target drops them"
    "a new target drops the target weights":
        (_weighted_target, lambda c: c.tree_set_target(H.reg_case("small").target), _normal, None,
         lambda c: H._resident(c, "small")),
    # "It stays resident until the next successful down-sample": a remembered member is refused by its serial number
    "a new down-sample makes a voxel member stale":
        (_voxel_member, lambda c: c.voxel_down_sample(H._voxel_clouds("small")[0], 0.5),
         lambda c: c.set_points_from_voxels(c._kept), r"^stale voxel result: ", None),
    # hgmm_set_points_* replaces the forest cloud: the batched entries want hgmm_set_points_batch_* again
    "set_points drops the forest's members (full covariance)":
        (_forest, _same_cloud_again, _fullcov_batch, STATE + r"\w+: no batch cloud is resident", None),
    "set_points drops the forest's members (KMeans)":
        (_forest, _same_cloud_again,
         lambda c: c.kmeans_fit_batch([len(P) for P in H.members("large")], 1, 2, 0.0, first_ids=[0, 0, 0]),
         STATE + r"\w+: no batch cloud is resident", None),
    # "the forest cloud of hgmm_set_points_batch_* ... has no float32 rows"
    "a forest cloud takes the float32 rows away from the flat entries":
        (_same_cloud_again, _forest, _fit_small, STATE + r".*(float32 rows|hgmm_set_points_f32)", None),
    "a forest cloud refuses flat weights":
        (_same_cloud_again, _forest, lambda c: c.flat_set_weights(np.ones(H.n_of("large"))),
         STATE + r"\w+: no cloud with float32 rows", None),
    # "Destroying the bound handle leaves nothing bound."
    "destroying the bound handle leaves nothing bound":
        (_bound_handle, lambda c: c.points_destroy(c._kept), _fit_small, STATE + r".*(float32 rows|hgmm_set_points_f32)", None),
    # hgmm_fullcov_fit_batch: refused "with hgmm_tree_set_precision(HGMM_PRECISION_F32_PDF) in force", "with the
    # fullcov_two_pass option set"
    "the float32 setting refuses the batched full-covariance fit":
        (_forest, lambda c: c.tree_set_precision(np.float32), _fullcov_batch,
         STATE + r"\w+: hgmm_tree_set_precision\(HGMM_PRECISION_F32_PDF\) is in force", None),
    "the two-pass option refuses the batched full-covariance fit":
        (_forest, lambda c: c.config_set("fullcov_two_pass", 1), _fullcov_batch,
         STATE + r"\w+: the fullcov_two_pass option is set", None),
}


@pytest.mark.parametrize("case", sorted(INVALIDATIONS))
def test_documented_invalidation_refuses_by_name_or_returns_fresh_bits(ctx, case):
    import hgmm_amd
    state, x, consumer, refusal, alone = INVALIDATIONS[case]
    state(ctx)
    try:
        x(ctx)
        if refusal is not None:
            with pytest.raises(hgmm_amd.HgmmError) as e:
                consumer(ctx)
            assert re.search(refusal, str(e.value)), str(e.value)
        else:
            def fresh_bits(c):
                alone(c)
                return consumer(c)
            want = fresh(fresh_bits)
            got = consumer(ctx)
            assert H.first_difference(got, want) is None, H.first_difference(got, want)
    finally:
        ctx.tree_set_precision(np.float64)
        ctx.config_set("fullcov_two_pass", 0)


# ---- (f) sticky settings return --------------------------------------------------------------------------------------------------

# option -> (a value that selects its other path, the op whose family it concerns): every option of hgmm_config_name but
# ipc_timeout_s (communicators are out of scope)
OPTIONS = {
    "estep_target_gbs": (0, "flat_estep"), "pace_start": (5800, "flat_estep"), "pace_forget": (1, "flat_estep"),
    "predict_single_row": (1, "flat_estep"),
    "tree_no_chol": (1, "tree_build"), "tree_rel": (1, "tree_build"), "tree_ahead": (0, "tree_build"),
    "tree_tickets": (1, "tree_build"), "tree_overlap": (0, "tree_build"),
    "fullcov_two_pass": (1, "fullcov_fit"), "kmpp_two_launches": (1, "kmeans"), "kmeans_acc_regs": (1, "kmeans"),
    "reg_device_solve": (1, "tree_register"),
}


def test_every_path_option_is_listed(ctx):
    assert sorted(OPTIONS) == sorted(set(ctx.config_names()) - {"ipc_timeout_s"})


@pytest.mark.parametrize("size", H.SIZES)
@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_an_option_leaves_no_trace_once_taken_back(ctx, refs, option, size):
    value, base = OPTIONS[option]
    name = "%s_%s" % (base, size)
    with ctx.config(**{option: value}):
        inside = H.OPS[name].fn(ctx)
    assert len(inside) == len(refs[name][0])
    check(name, H.OPS[name].fn(ctx), refs, " after %s = %d was taken back" % (option, value))


@pytest.mark.parametrize("size", H.SIZES)
def test_tree_precision_returns_and_reaches_the_full_covariance_fit_meanwhile(ctx, refs, size):
    """Documented: the float32 setting also selects the full-covariance fit's float32-tile kernel.  Inside it the fit is
    the float32-tile op's bits (which differ from the float64 fit's); once float64 is back, both are their defaults."""
    s = H.SHAPES[size]
    ctx.tree_set_precision(np.float32)
    try:
        f32_build = H.OPS["tree_build_%s" % size].fn(ctx)
        tile = H._fullcov(ctx, s, False, 11)
    finally:
        ctx.tree_set_precision(np.float64)
    check("fullcov_f32_tile_%s" % size, tile, refs, " under tree_set_precision(float32)")
    f64 = H._fullcov(ctx, s, False, 11)
    assert not H.same_bits(f64, tile)
    assert len(f32_build) == len(refs["tree_build_%s" % size][0])
    check("tree_build_%s" % size, H.OPS["tree_build_%s" % size].fn(ctx), refs, " after float32 pdfs were taken back")
    check("fullcov_fit_%s" % size, H.OPS["fullcov_fit_%s" % size].fn(ctx), refs, " after float32 pdfs were taken back")


@pytest.mark.parametrize("size", H.SIZES)
def test_registration_gate_returns(ctx, refs, size):
    ctx.tree_set_reg_gate(H.CHI2_3_999)
    try:
        gated = H.OPS["tree_register_%s" % size].fn(ctx)
        forest = H.OPS["forest_register_%s" % size].fn(ctx)
    finally:
        ctx.tree_set_reg_gate(np.inf)
    check("tree_register_gated_%s" % size, H.flat((gated, H.CHI2_3_999)), refs, " under a gate set outside the op")
    assert len(forest) == len(refs["forest_register_%s" % size][0])
    for base in ("tree_register", "forest_register", "tree_multistart"):
        check("%s_%s" % (base, size), H.OPS["%s_%s" % (base, size)].fn(ctx), refs, " after the gate was taken off")


# ---- (g) refusals in the middle ------------------------------------------------------------------------------------------------

def _nan_weights(c):
    P = H.cloud("small", "float32")
    c.set_points(P)
    w = np.array(H.weights(len(P), 21))
    w[len(w) // 2] = np.nan
    c.flat_set_weights(w)                                   # test_weight_state_gpu.test_a_refused_upload_keeps_the_weights


def _k_above_n(c):
    arrs = c.set_points_batch([H._centred(H.cloud("small"))])
    c.kmeans_fit_batch([len(arrs[0])], len(arrs[0]) + 1, 2, 0.0, first_ids=[0],            # test_kmeans_batch_gpu: k > counts[b]
                       rand_vals=np.zeros((1, len(arrs[0]), 2)))


def _weighted_fit_without_weights(c):
    P = H.cloud("small")
    c.set_points(P)
    c.fullcov_fit(3, 1.0, 1e-4, P[:3], 0.001, 2, weighted=True)          # test_fullcov_weights_gpu: no source weights resident


# family -> (the refused call, the text hgmm_last_error gives)
REFUSALS = {
    "flat": (_nan_weights, r"\(-2\): hgmm_flat_set_weights: weight 155 is nan"),
    "kmeans": (_k_above_n, r"\(-2\): "),
    "fullcov": (_weighted_fit_without_weights, r"\(-3\): \w+: no source weights are resident"),
    "tree": (lambda c: c.tree_set_reg_gate(-1.0), r"\(-2\): "),                                  # test_tree_gate_gpu: a gate <= 0
    "forest": (lambda c: c.tree_register_batch_multi([9], [H.I3], [H.Z3], 1.0, H.LAMBDA_C, 2, 0.0), r"\(-[23]\): "),
    "voxel": (lambda c: c.voxel_down_sample(H.cloud("small"), -1.0), r"\(-2\): "),              # test_voxel_gpu: voxel size <= 0
    "l2": (lambda c: c.l2_cost([0], [H.I3], [H.Z3], -1.0), r"\(-[23]\): "),                      # test_gmmreg_resident_gpu: sigma <= 0
}
# the neighbours: one op per family, so that a refusal always stands between two OTHER families
NEIGHBOURS = ["tree_register_large", "flat_fit_weighted_small", "forest_register_large", "fullcov_batch_small", "l2_large",
              "kmeans_weighted_small", "voxel_hand_over_large", "tree_build_weighted_small", "flat_batch_large"]


@pytest.mark.parametrize("family", sorted(REFUSALS))
def test_a_refusal_changes_neither_neighbour(ctx, refs, family):
    import hgmm_amd
    refused, text = REFUSALS[family]
    others = [n for n in NEIGHBOURS if H.OPS[n].family != family]
    at = sorted(REFUSALS).index(family)
    before, after = others[at % len(others)], others[(at + 1) % len(others)]
    check(before, H.OPS[before].fn(ctx), refs, " before the refused %s call" % family)
    with pytest.raises(hgmm_amd.HgmmError) as e:
        refused(ctx)
    assert re.search(text, str(e.value)), str(e.value)
    check(after, H.OPS[after].fn(ctx), refs, " after the refused %s call (which followed %s)" % (family, before))
    check(before, H.OPS[before].fn(ctx), refs, " once more after the refused %s call" % family)


# ---- (h) nothing left out -------------------------------------------------------------------------------------------------------

def test_every_declared_entry_is_reached_or_excluded_with_a_reason(ctx, refs):
    """A new entry of include/hgmm.h fails here until an op calls it or EXCLUDED says why none has to."""
    for name, op in H.OPS.items():                       # (alone, this test still sees every op once)
        if name not in LAST:
            LAST[name] = op.fn(ctx)
    declared = set(H.declared_entries())
    missing = declared - H.REACHED - set(H.EXCLUDED)
    assert not missing, "neither reached by an op nor excluded with a reason: %s" % sorted(missing)
    assert set(H.EXCLUDED) <= declared and H.REACHED <= declared, sorted((set(H.EXCLUDED) | H.REACHED) - declared)
