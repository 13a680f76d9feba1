"""Target weights of any scale (hgmm_tree_set_target_weights[_batch]): the registration E-step's fixed-point sums on the GPU.

The E-step adds every term w gamma (1, u, u u^T) as an integer in units of 2^-F, D 2^-F and D^2 2^-F (tree_reg_estep_body,
reg_extent / reg_encoding in csrc/tree_device.h).  F is set by the sum of the weights: sum < 2^e gives F = 62 - e, in both
directions, so that weights in [0, 1] whose sum is far below 1 (range or incidence weights, M-estimator weights) keep the
resolution that counts have.  The other weighted tests (tests/test_tree_weights_gpu.py) use one weight vector with a sum
between 2^11 and 2^14; here the same vector is scaled.

 a. w 2^k gives exactly 2^k times the moments of w, k from -80 to +50 (F from 130 down to -2); the moments of w itself are
    the bits recorded before F followed the sum below 1.
 b. arbitrary scales c against the NumPy restatement at the weighted tests' bound carried along (the problem is linear in c).
 c. the index-order sum of the weights exactly 2^m and one ulp below it, m = 0 and 12: the two sides of a step of F.
 d. one node takes every point with gamma exactly 1: m0 is the exact sum, up to the largest sums the encoding admits.
 e. the loops under scaled weights against the restatement's loop; batch (one sum per member, re-derived every iteration by
    reg_pair_fill / reg_device_step) and multi-start bitwise the serial call.
 f. the score summaries under w 2^k are exactly 2^k times those under w.
(g., two ranks with an all-reduced sum below 1, is a case of tests/test_tree_weights_gpu.py's two-rank test.)

Fixtures: hgmm_reg_L2.npz (2 013 points, T = 72: every node in the LDS table) and hgmm_reg_L4 (5 032 points, nodes beyond
584 take the global atomics); neither point count is a multiple of the 256-point workgroup."""
import hashlib
import math

import numpy as np
import pytest

from conftest import load_golden
from oracle import hgmm_tree

from _tree_helpers import I3, loop5, resident, weights_for

pytestmark = pytest.mark.gpu

LC = 0.01
TINY = np.finfo(np.float64).tiny


@pytest.fixture(scope="module")
def ctx():
    import hgmm_amd
    c = hgmm_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    return {2: load_golden("hgmm_reg_L2.npz"), 4: load_golden("hgmm_reg_L4.npz")}


@pytest.fixture()
def gated(ctx):
    """set the context's gate for a test, +inf afterwards"""
    def set_gate(gate):
        ctx.tree_set_reg_gate(gate)
    yield set_gate
    ctx.tree_set_reg_gate(np.inf)


@pytest.fixture(scope="module")
def preconditions(records):
    """What a comparison of moments with the restatement presupposes (tests/test_tree_weights_gpu.py): no descent decision of
    the target is a near-tie, and no contributing pair lies within 1e-9 of the gate.  Neither sees the weights; computed once
    per (L, gate)."""
    seen = {}

    def check(L, gate):
        g = records[L]
        X = g["rot10_target"]
        lc = float(g["lambda_c"])
        if L not in seen:
            seen[L] = bool(hgmm_tree.reg_near_ties(hgmm_tree.reg_descent(X, g["pi"], g["mu"], g["cov"], L, lc)).any())
        assert not seen[L]
        if np.isfinite(gate):
            if (L, gate) not in seen:
                seen[L, gate] = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, gate=gate, report=True).margin
            assert seen[L, gate] > 1e-9
    return check


def index_sum(w):
    """the float64 sum of w in index order: what hgmm_tree_set_target_weights computes and the encoding reads"""
    return float(np.cumsum(w)[-1])


def frac_bits(wsum):
    """F of the documented rule: wsum < 2^e -> 62 - e (62 - bits(n) for a count n)"""
    return 62 - int(np.frexp(wsum)[1])


def assert_moments_at_scale(m, o, c, label):
    """rtol 1e-10 / atol 1e-12 c: the weighted tests' bound with its absolute part carried along with the scale"""
    for name, a, b in zip(("m0", "m1", "m2"), m, o):
        print("%s %s: largest |difference| / c %.3g" % (label, name, np.abs(a - b).max() / c))
    for name, a, b in zip(("m0", "m1", "m2"), m, o):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12 * c, err_msg="%s %s" % (label, name))


# ---------------------------------------------------------------------------------------------------------------------
# a. exact covariance of the E-step under power-of-two scales
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("gate", [np.inf, 16.0])
@pytest.mark.parametrize("k", [-80, -40, -13, -1, 1, 20, 50])
def test_power_of_two_scale_of_the_weights_scales_the_moments_exactly(ctx, records, gated, L, gate, k):
    """The integer a term rounds to is rint(gamma w 2^k 2^(F - k) u ...): the same integer for every k, and unpacking and the
    expansion about mu multiply by powers of two only.  So m(w 2^k) == 2^k m(w), bit for bit.  k = +50 takes the sum to about
    1e19, where F <= 0."""
    g = records[L]
    X = g["rot10_target"]
    w = weights_for(len(X))
    _, lc, T = resident(ctx, g, X, w)
    gated(gate)
    base = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    s = 2.0 ** k
    assert (base[0] > 0).sum() > 8
    for b in base:                               # (no product below leaves the normal range: the scaling of `base` is exact)
        assert np.abs(b[b != 0]).min() * min(s, 1.0) > TINY and np.abs(b).max() * max(s, 1.0) < 1e300
    F = frac_bits(index_sum(w * s))
    assert F == frac_bits(index_sum(w)) - k
    if k == 50:
        assert F <= 0
    ctx.tree_set_target_weights(w * s)
    m = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    differ = []
    for name, a, b in zip(("m0", "m1", "m2"), m, base):
        n_bad = int((a != b * s).sum())
        print("L=%d gate %g k=%+d (F = %d) %s: %d of %d entries differ from 2^k times the unscaled ones, largest |difference| / 2^k "
              "%.3g" % (L, gate, k, F, name, n_bad, a.size, np.abs(a / s - b).max()))
        if n_bad:
            differ.append(name)
    assert not differ, differ


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("gate", [np.inf, 16.0])
def test_unscaled_weights_give_the_bits_from_before_f_followed_small_sums(ctx, records, gated, L, gate):
    """For a sum >= 1 the rule is the earlier one (1 <= 2^(e-1) <= sum < 2^e: e is the bit length the earlier loop counted), so
    weights_for(n) must give the bits it gave.  tests/golden/tree_weight_scale_prechange.npz holds what hgmm_tree_reg_estep
    returned for these four cases on an MI355X from the library as it was before the rule changed: m0 in full, m1 and m2 as
    SHA-256 of their bytes.  The sums are integer sums, so the bits do not depend on the order of the atomics; a change that
    moves them on purpose (another exponential, another expansion) records them anew."""
    g = records[L]
    X = g["rot10_target"]
    _, lc, T = resident(ctx, g, X, weights_for(len(X)))
    gated(gate)
    m = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    gold = load_golden("tree_weight_scale_prechange.npz")
    key = "L%d_gate%s" % (L, "inf" if np.isinf(gate) else "%g" % gate)
    print("%s: largest m0 difference to the recorded bits %.3g" % (key, np.abs(m[0] - gold[key + "_m0"]).max()))
    assert np.array_equal(m[0], gold[key + "_m0"])
    for name, a in (("m1", m[1]), ("m2", m[2])):
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest() == gold[key + "_" + name + "_sha256"].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------------
# b. arbitrary scales against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def named_scale(name, w):
    W = index_sum(w)
    return {"1e-9": 1e-9, "3e-5": 3e-5, "0.37/W": 0.37 / W, "1/W": 1.0 / W, "7e11": 7e11}[name]


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("gate", [np.inf, 16.0])
@pytest.mark.parametrize("scale", ["1e-9", "3e-5", "0.37/W", "1/W", "7e11"])
def test_scaled_weights_match_the_restatement(ctx, records, gated, preconditions, L, gate, scale):
    """w c against the restatement under w c at rtol 1e-10 / atol 1e-12 c.  1 / W is the normalised-weights case: its sum sits
    on the 2^0 step of F."""
    g = records[L]
    X = g["rot10_target"]
    w = weights_for(len(X))
    c = named_scale(scale, w)
    wc = w * c
    preconditions(L, gate)
    _, lc, T = resident(ctx, g, X, wc)
    gated(gate)
    m = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    o = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, wc, gate)
    label = "L=%d gate %g c = %s (sum %.17g, F = %d)" % (L, gate, scale, index_sum(wc), frac_bits(index_sum(wc)))
    assert_moments_at_scale(m, o, c, label)


# ---------------------------------------------------------------------------------------------------------------------
# c. the sum exactly on a step of F
# ---------------------------------------------------------------------------------------------------------------------
def weights_summing_to(n, total):
    """weights_for(n) scaled so that the first n - 1 sum (in index order) to about 0.75 total, the last one the exact
    remainder: total / 2 <= S <= 2 total, so total - S is exact (Sterbenz) and S + (total - S) is total.  -> (w, scale)"""
    w0 = weights_for(n)
    c = 0.75 * total / index_sum(w0[:-1])
    w = w0 * c
    S = index_sum(w[:-1])
    assert 0.5 * total <= S < total
    w[-1] = total - S
    assert w[-1] > 0 and index_sum(w) == total
    return w, c


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("m", [0, 12])
@pytest.mark.parametrize("side", ["2^m", "2^m - ulp"])
def test_sum_of_the_weights_on_a_step_of_f(ctx, records, preconditions, L, m, side):
    """sum == 2^m: F = 61 - m; sum == 2^m - ulp: F = 62 - m, and the sums come within an ulp of the 2^62 they may not reach."""
    g = records[L]
    X = g["rot10_target"]
    total = 2.0 ** m if side == "2^m" else float(np.nextafter(2.0 ** m, 0.0))
    w, c = weights_summing_to(len(X), total)
    assert frac_bits(total) == (61 - m if side == "2^m" else 62 - m)
    preconditions(L, np.inf)
    _, lc, T = resident(ctx, g, X, w)
    assert ctx.tree_score(None, None, 1.0, lc, want=())[0][0] == total          # (the library's own sum: slot 0)
    mom = ctx.tree_reg_estep(T, None, None, 1.0, lc)
    o = hgmm_tree.reg_e_step(X, g["pi"], g["mu"], g["cov"], L, lc, w)
    assert_moments_at_scale(mom, o, c, "L=%d sum %s, m = %d (F = %d)" % (L, side, m, frac_bits(total)))


# ---------------------------------------------------------------------------------------------------------------------
# d. one node takes everything: exact saturation of the sums
# ---------------------------------------------------------------------------------------------------------------------
U_FLOAT = 2.0 ** -49                            # sixteen roundings of 2^-53 (check_one_node)


def check_one_node(ctx, X, w, total, label):
    """L = 1, node 0 with pi = 1, mu = (0.5, 0.5, 0.5), cov = 0.1 I (complexity 1/3 > lambda_c: it never stops a point), nodes
    1..7 with pi = 0: gamma = g_0 / g_0 is exactly 1 for every point of [0, 1]^3, so every m0 term is the integer w 2^F.

    m0[0] is the exact sum.  m1[0] and m2[0] against math.fsum: the fixed-point roundings move them by at most
    k 2^-(F+1) (D + |mu|)^p, p = 1 / 2, after k contributions (test_tree_reg_depth_gpu.m2_quantum_bound; for m1 = c1 + m0 mu
    only c1 is rounded, in units of D 2^-F).  That counts the roundings to integers only, and with F = 61 (one point) it is
    1.8e-18 for an m2 entry of about 0.25, which float64 resolves to 5.6e-17: a bound no float64 result can be held to.  So
    the float64 roundings are counted next to it.  Every number on the way is at most S (dmax + |mu|)^p in size, S the sum
    of the weights and dmax the largest |x - mu|, and it is rounded to 2^-53 relative at most sixteen times: per C2 term the
    two differences x - mu and the two products gamma w 2^F u_a u_b; on the totals the conversion of the integer sum, four
    products and three sums of the expansion about mu; and the reference's own products w x_a x_b before math.fsum (m1: fewer
    of each).  That is 2^-49 S (dmax + |mu|)^p, and the bound is the sum of the two.  From F = 47 down the quantum is the
    larger part."""
    T = hgmm_tree.n_total(1)
    pi, mu, cov = np.zeros(T), np.zeros((T, 3)), np.tile(np.eye(3), (T, 1, 1))
    pi[0], mu[0], cov[0] = 1.0, 0.5, 0.1 * np.eye(3)
    assert hgmm_tree.complexity(cov)[0] > LC
    ctx.tree_set_nodes(1, pi, mu, cov)
    ctx.tree_set_target(X)
    if w is not None:
        ctx.tree_set_target_weights(w)
    m0, m1, m2 = ctx.tree_reg_estep(T, None, None, 1.0, LC)
    ww = np.ones(len(X)) if w is None else w
    k = int((ww > 0).sum())
    # (D, F) from the documented rule: extent = |R|_F max|x| + |t| + max|mu| at the identity, rounded up to a power of two
    ext = np.sqrt(3.0) * np.sqrt((X * X).sum(axis=1)).max() + np.sqrt((mu * mu).sum(axis=1)).max()
    D, F = 2.0 ** np.frexp(ext)[1], frac_bits(total)
    r = D + np.linalg.norm(mu[0])
    ref1 = np.array([math.fsum(ww * X[:, a]) for a in range(3)])
    ref2 = np.array([[math.fsum(ww * X[:, a] * X[:, b]) for b in range(3)] for a in range(3)])
    size = float(np.sqrt(((X - mu[0]) ** 2).sum(axis=1)).max()) + np.linalg.norm(mu[0])
    q1, q2 = k * r * 2.0 ** -(F + 1), k * r * r * 2.0 ** -(F + 1)
    tol1, tol2 = q1 + U_FLOAT * total * size, q2 + U_FLOAT * total * size * size
    print("%s: D = %g, F = %d, k = %d; m0[0] - sum = %.3g; largest m1 difference %.3g (bound %.3g, of it the quantum %.3g), "
          "m2 %.3g (bound %.3g, quantum %.3g)" % (label, D, F, k, m0[0] - total, np.abs(m1[0] - ref1).max(), tol1, q1,
                                                  np.abs(m2[0] - ref2).max(), tol2, q2))
    assert m0[0] == total
    assert not m0[1:].any() and not m1[1:].any() and not m2[1:].any()
    assert (np.abs(m1[0] - ref1) <= tol1).all()
    assert (np.abs(m2[0] - ref2) <= tol2).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 65536])
def test_one_node_takes_every_point_unweighted(ctx, n):
    """n on both sides of a workgroup (256) and of two steps of F (4096: 62 - 12 -> 62 - 13; 65536: 45)"""
    X = np.random.RandomState(1000 + n).uniform(size=(n, 3))
    check_one_node(ctx, X, None, float(n), "n = %d" % n)


@pytest.mark.parametrize("short", [False, True])
def test_one_node_takes_every_point_weights_fill_the_sums(ctx, short):
    """Weights that are multiples of 2^-8 in [0, 4] with the exact sum 2^12 (F = 49: m0's integer is 2^61) and 2^12 - 2^-8
    (F = 50: 2^62 - 2^42, as close to the 2^62 the encoding keeps free as these weights come)."""
    n = 2100
    rs = np.random.RandomState(12)
    X = rs.uniform(size=(n, 3))
    q = rs.randint(0, 1025, n).astype(np.int64)
    left = 2 ** 20 - int(short) - int(q.sum())
    for i in range(n):                           # (spend the difference on the first entries, each kept inside [0, 1024])
        step = min(max(left, -int(q[i])), 1024 - int(q[i]))
        q[i] += step
        left -= step
    assert left == 0 and q.min() == 0 and 1000 < q.max() <= 1024
    w = q / 256.0
    total = (2 ** 20 - int(short)) / 256.0
    assert index_sum(w) == math.fsum(w) == total
    assert frac_bits(total) == (50 if short else 49)
    check_one_node(ctx, X, w, total, "sum 2^12%s" % (" - 2^-8" if short else ""))


# ---------------------------------------------------------------------------------------------------------------------
# e. the loops under scaled weights
# ---------------------------------------------------------------------------------------------------------------------
def loop_scale(name, w):
    return {"2^-10": 2.0 ** -10, "2^10": 2.0 ** 10, "1/W": 1.0 / index_sum(w), "2^-20": 2.0 ** -20}[name]


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("deg", [10, 30])
@pytest.mark.parametrize("scale", ["2^-10", "2^10", "1/W", "2^-20"])
def test_loop_under_scaled_weights_matches_the_restatement(ctx, records, L, deg, scale):
    """Five iterations, tol 0, every pose against the restatement's loop under the same weights at atol 1e-8, the loop tests'
    bound.  The M-step leaves out nodes with m0 < float32 eps -- it reads weights as point counts -- so the scales are those
    at which the restatement's live set is not trivial, and no m0 of its trace may lie within 1e-6 (relative) of that
    threshold, where the device could decide the other way."""
    g = records[L]
    X = g["rot%d_target" % deg]
    w = weights_for(len(X))
    wc = w * loop_scale(scale, w)
    _, lc, T = resident(ctx, g, X, wc)
    rot, t, done, q, status, trace = loop5(ctx, lc)
    assert done == 5 and status == 0
    o_tr = hgmm_tree.register(X, g["pi"], g["mu"], g["cov"], L, lc, 5, 0.0, wc)[3]
    assert len(o_tr) == 5
    eps32 = hgmm_tree.F32_EPS
    live = [int((~(it[3] < eps32)).sum()) for it in o_tr]
    nearest = min(float(np.abs(it[3] - eps32).min()) / eps32 for it in o_tr)
    print("L=%d rot%d c = %s: live nodes per iteration %s, nearest m0 to the threshold %.3g (relative)" % (L, deg, scale, live, nearest))
    assert nearest > 1e-6 and min(live) >= 6
    worst = 0.0
    for k in range(5):
        r_k, t_k = trace[k, :9].reshape(3, 3), trace[k, 9:12]
        worst = max(worst, np.abs(r_k - o_tr[k][0]).max(), np.abs(t_k - o_tr[k][1]).max())
    print("L=%d rot%d c = %s: largest pose difference over five iterations %.3g" % (L, deg, scale, worst))
    for k in range(5):
        np.testing.assert_allclose(trace[k, :9].reshape(3, 3), o_tr[k][0], rtol=0, atol=1e-8, err_msg="iteration %d" % k)
        np.testing.assert_allclose(trace[k, 9:12], o_tr[k][1], rtol=0, atol=1e-8, err_msg="iteration %d" % k)
    np.testing.assert_allclose(rot, o_tr[4][0], rtol=0, atol=1e-8)
    np.testing.assert_allclose(t, o_tr[4][1], rtol=0, atol=1e-8)


def rot_about(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def starts_for(X):
    c = X.mean(axis=0)
    rots = [I3, rot_about([0, 0, 1], 10), rot_about([0, 0, 1], -10)]
    return np.stack(rots), np.stack([c - R @ c for R in rots])


@pytest.mark.parametrize("device_solve", [0, 1])
def test_scaled_multi_and_batch_are_bitwise_the_serial_call(ctx, records, device_solve):
    """tests/test_tree_weights_gpu.py's B = 3 ragged pairs of the L = 4 target, with w 2^-20 on the first, none on the second
    and w 2^10 on the third: one weight sum per member, from which reg_pair_fill (host) and reg_device_step
    (reg_device_solve) derive D and F again at every iteration.  Every member is the serial call under its own weights, bit
    for bit; so are K = 3 start poses under w 2^-20 and under w 2^10."""
    g = records[4]
    P, X = g["points"], g["rot10_target"]
    L, lc = int(g["L"]), float(g["lambda_c"])
    T = hgmm_tree.n_total(L)
    rot0, t0 = starts_for(X)
    targets = [X, X[1000:4001], X[3255:]]
    assert [len(tg) for tg in targets] == [5032, 3001, 1777]
    ws = [weights_for(len(targets[0])) * 2.0 ** -20, None, weights_for(len(targets[2])) * 2.0 ** 10]
    assert index_sum(ws[0]) < 2.0 ** -6 and index_sum(ws[2]) > 2.0 ** 21
    idx = np.random.RandomState(72).randint(T, size=T)
    with ctx.config(reg_device_solve=device_solve):
        # the forest first: the serial calls below replace the context's resident cloud
        arrs = ctx.set_points_batch([P] * 3)
        ctx.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
        ctx.tree_set_targets_batch(targets, weights=ws)
        b_rot, b_t, b_it, b_q, b_st, b_tr = ctx.tree_register_batch(np.tile(I3, (3, 1, 1)), np.zeros((3, 3)), 1.0, lc, 5, 0.0,
                                                                    want_trace=True)
        b_sum = ctx.tree_score_batch(b_rot, b_t, 1.0, lc)
        ctx.set_points(P)
        pi, mu, cov = ctx.tree_build(L, 20.0, 1e-4, P[idx], 0.004)[:3]
        for b, tg in enumerate(targets):
            ctx.tree_set_nodes(L, pi, mu, cov)
            ctx.tree_set_target(tg)
            if ws[b] is not None:
                ctx.tree_set_target_weights(ws[b])
            s_rot, s_t, s_it, s_q, s_st, s_tr = loop5(ctx, lc)
            print("device_solve %d pair %d: %d iterations, status %d, q %r" % (device_solve, b, s_it, s_st, s_q))
            assert (int(b_it[b]), int(b_st[b])) == (s_it, s_st) and s_it == 5, b
            assert np.array_equal(b_rot[b], s_rot) and np.array_equal(b_t[b], s_t), b
            assert (b_q[b] == s_q) or (np.isnan(b_q[b]) and s_q is None), b
            assert np.array_equal(b_tr[b], s_tr), b
            s_sum = ctx.tree_score(s_rot, s_t, 1.0, lc, want=())[0]
            assert np.array_equal(b_sum[b], s_sum), b
            assert s_sum[0] == (len(tg) if ws[b] is None else index_sum(ws[b])), b
        # multi-start on the record's own tree: the K hypotheses share the one weight array
        for wk in (ws[0], weights_for(len(X)) * 2.0 ** 10):
            resident(ctx, g, X, wk)
            m_rot, m_t, m_it, m_q, m_st, m_tr = ctx.tree_register_multi(rot0, t0, 1.0, lc, 5, 0.0, want_trace=True)
            m_sum = ctx.tree_score_multi(m_rot, m_t, 1.0, lc)
            for k in range(3):
                s_rot, s_t, s_it, s_q, s_st, s_tr = ctx.tree_register(rot0[k], t0[k], 1.0, lc, 5, 0.0, None, want_trace=True)
                assert (int(m_it[k]), int(m_st[k])) == (s_it, s_st) and s_it > 0, k
                assert np.array_equal(m_rot[k], s_rot) and np.array_equal(m_t[k], s_t) and m_q[k] == s_q, k
                assert np.array_equal(m_tr[k], s_tr), k
                assert np.array_equal(m_sum[k], ctx.tree_score(s_rot, s_t, 1.0, lc, want=())[0]), k


# ---------------------------------------------------------------------------------------------------------------------
# f. score summaries
# ---------------------------------------------------------------------------------------------------------------------
def assert_summary_scaled(s_scaled, s_base, s, label):
    print("%s: slots 0..6 %s\n    2^k times the unscaled ones %s" % (label, s_scaled[:7], s_base[:7] * s))
    assert np.array_equal(s_scaled[:7], s_base[:7] * s, equal_nan=True), label
    assert np.array_equal(s_scaled[7:], s_base[7:], equal_nan=True), label


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("k", [-40, 20])
def test_score_summary_scales_exactly_serial_and_multi(ctx, records, L, k):
    """Slots 0..6 are sums of w x in a fixed order: w 2^k gives exactly 2^k times each; the per-point arrays do not see the
    weights."""
    g = records[L]
    X = g["rot10_target"]
    w = weights_for(len(X))
    s = 2.0 ** k
    rot0, t0 = starts_for(X)
    _, lc, T = resident(ctx, g, X, w)
    base, arr = ctx.tree_score(None, None, 1.0, lc)
    base_multi = ctx.tree_score_multi(rot0, t0, 1.0, lc)
    assert base[0] == index_sum(w) and base[1] > 0 and (base[:7] != 0).sum() >= 5
    ctx.tree_set_target_weights(w * s)
    scaled, arr_s = ctx.tree_score(None, None, 1.0, lc)
    for name in ("node", "maha2", "logp"):
        assert np.array_equal(arr_s[name], arr[name], equal_nan=True), name
    assert_summary_scaled(scaled, base, s, "L=%d k=%+d serial" % (L, k))
    scaled_multi = ctx.tree_score_multi(rot0, t0, 1.0, lc)
    for j in range(3):
        assert_summary_scaled(scaled_multi[j], base_multi[j], s, "L=%d k=%+d start %d" % (L, k, j))


@pytest.mark.parametrize("k", [-40, 20])
def test_score_summary_scales_exactly_batch(ctx, records, k):
    """B = 3 pairs on a forest of the L = 2 record's points; the first pair's weights are scaled, the second has none, the
    third keeps its own: the first summary scales, the others keep their bits."""
    g = records[2]
    P, X = g["points"], g["rot10_target"]
    L, lc = int(g["L"]), float(g["lambda_c"])
    T = hgmm_tree.n_total(L)
    s = 2.0 ** k
    rot0, t0 = starts_for(X)
    targets = [X, X[:1500], X[:700]]
    ws = [weights_for(len(tg)) for tg in targets]
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch([P] * 3)
    ctx.tree_build_batch([len(P)] * 3, L, 20.0, 1e-4, np.stack([a[idx] for a in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch(targets, weights=[ws[0], None, ws[2]])
    base = ctx.tree_score_batch(rot0, t0, 1.0, lc)
    assert base[0][0] == index_sum(ws[0]) and base[1][0] == len(targets[1])
    ctx.tree_set_target_weights_batch([ws[0] * s, None, ws[2]])
    scaled = ctx.tree_score_batch(rot0, t0, 1.0, lc)
    assert_summary_scaled(scaled[0], base[0], s, "k=%+d pair 0" % k)
    assert np.array_equal(scaled[1:], base[1:], equal_nan=True)
