"""The lifetime rules of the five resident weight sets (csrc/hgmm_ctx.h: WeightSet, MemberWeights), one table.

    set            weights of                       uploaded by                              read by (the test's "result")
    src            resident cloud, tree             tree_set_source_weights                  a tree_build of 2 iterations a level
    flat           resident cloud, flat EM          flat_set_weights                         flat_stats
    tgt            serial target                    tree_set_target_weights                  tree_reg_normal
    forest_src     forest cloud, per member         tree_set_source_weights_batch            a tree_build_batch of 2 iterations
    forest_tg      forest targets, per member       tree_set_target_weights_batch            tree_score_batch

Every set obeys the same three rules, bit for bit:
    (a) a refused upload (a NaN at a middle index) keeps the weights that were in force, with the entry's code and message;
    (b) whatever replaces the cloud / the target by a same-sized one -- an upload, a voxel hand-over -- drops them: the next
        result is that of a context that never saw a weight;
    (c) None takes them off likewise.
The forest sets also with one member's entry None: that member keeps its unweighted bits next to a weighted one.

Shapes: clouds and targets of 300 - 700 points (their sizes are the voxel members', so that a hand-over replaces a cloud by a
same-sized one: a weight buffer left in force would fit), L = 2 trees, J = 8 flat components, B = 2 members.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, T, J = 2, 72, 8
LS, LD, SIG2, LAMBDA_C = 20.0, 1e-4, 0.004, 0.01
NAN_MSG = "hgmm call failed (-2): %s: weight %d is nan (weights must be finite and >= 0)"


class Data:
    """what both contexts work on: raw clouds for the voxel members, and clouds / targets of the members' sizes"""

    def __init__(self, sizes):
        rng = np.random.default_rng(20)
        self.sizes = sizes
        self.clouds = [rng.uniform(0.0, 1.0, (m, 3)) for m in sizes]                  # the weighted ones
        self.others = [rng.uniform(0.0, 1.0, (m, 3)) for m in sizes]                  # what replaces them by upload
        self.w = [np.where(rng.uniform(size=m) < 0.1, 0.0, rng.uniform(0.25, 4.0, m)) for m in sizes]
        self.init_mu = rng.uniform(0.1, 0.9, (2, T, 3))
        self.flat = (rng.uniform(2.0, 6.0, (J, 3)).astype(np.float32), rng.uniform(0.0, 1.0, (J, 3)).astype(np.float32),
                     np.full(J, 1.0 / J, np.float32))                                # inv_std, mu, w


RAW = [np.random.default_rng(7 + k).uniform(0.0, 1.0, (1500 + 200 * k, 3)) for k in range(2)]


def voxels(ctx):
    return ctx.voxel_down_sample_batch(RAW, 0.125, download=False).members()


@pytest.fixture(scope="module")
def world():
    """(the context under test, a context that never sees a weight, their voxel members, the data)"""
    import hgmm_amd
    ctx, plain = hgmm_amd.Context(0), hgmm_amd.Context(0)
    vx, vx_plain = voxels(ctx), voxels(plain)
    sizes = [len(v) for v in vx]
    assert sizes == [len(v) for v in vx_plain] and all(300 <= m <= 700 for m in sizes), sizes
    d = Data(sizes)
    # the nodes the serial target is registered against: built without weights
    d.nodes = plain.set_points(d.clouds[0]).tree_build(L, LS, LD, d.init_mu[0], SIG2, 2, want_leaf=False)[:3]
    yield ctx, plain, {id(ctx): vx, id(plain): vx_plain}, d
    ctx.close()
    plain.close()


def bits(result):
    """a result -- an array, or tuples of arrays and numbers, nested -- as a flat list of arrays"""
    if not isinstance(result, (tuple, list)):
        return [np.asarray(result)]
    return [a for r in result for a in bits(r)]


def same(a, b):
    a, b = bits(a), bits(b)
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def with_nan(w):
    v = np.array(w, dtype=np.float64)
    v[len(v) // 2] = np.nan
    return v


class Src:
    """the resident cloud's weights for the tree build"""
    entry = "hgmm_tree_set_source_weights"

    def upload(self, c, d, clouds): c.set_points(clouds[0])
    def hand_over(self, c, vx): c.set_points_from_voxels(vx[0], tree_weights=False, flat_weights=False)
    def weigh(self, c, d): c.tree_set_source_weights(d.w[0])
    def off(self, c): c.tree_set_source_weights(None)
    def refused(self, c, d): c.tree_set_source_weights(with_nan(d.w[0]))
    def message(self, d): return NAN_MSG % (self.entry, d.sizes[0] // 2)
    def result(self, c, d): return c.tree_build(L, LS, LD, d.init_mu[0], SIG2, 2, want_leaf=False)[:3]


class Flat(Src):
    """the resident cloud's weights for the flat EM (float32)"""
    entry = "hgmm_flat_set_weights"

    def weigh(self, c, d): c.flat_set_weights(d.w[0])
    def off(self, c): c.flat_set_weights(None)
    def refused(self, c, d): c.flat_set_weights(with_nan(d.w[0]))
    def result(self, c, d): return c.flat_stats(*d.flat, "diag", "W")


class Tgt(Src):
    """the serial target's weights"""
    entry = "hgmm_tree_set_target_weights"

    def upload(self, c, d, clouds):
        c.tree_set_nodes(L, *d.nodes)
        c.tree_set_target(clouds[0])

    def hand_over(self, c, vx): c.tree_set_target_from_voxels(vx[0], weighted=False)
    def weigh(self, c, d): c.tree_set_target_weights(d.w[0])
    def off(self, c): c.tree_set_target_weights(None)
    def refused(self, c, d): c.tree_set_target_weights(with_nan(d.w[0]))
    def result(self, c, d): return c.tree_reg_normal(None, None, 1.0, LAMBDA_C)


class ForestSrc:
    """the forest cloud's weights, member by member; `entries`: which members bring weights"""
    entry, noun = "hgmm_tree_set_source_weights_batch", "cloud"

    def __init__(self, entries): self.entries = entries
    def weights(self, d): return [d.w[b] if on else None for b, on in enumerate(self.entries)]
    def upload(self, c, d, clouds): c.set_points_batch(clouds)
    def hand_over(self, c, vx): c.set_points_batch_from_voxels(vx, weighted=False)
    def weigh(self, c, d): c.tree_set_source_weights_batch(self.weights(d))
    def off(self, c): c.tree_set_source_weights_batch(None)
    def refused(self, c, d): c.tree_set_source_weights_batch([d.w[0], with_nan(d.w[1])])
    def message(self, d): return NAN_MSG % ("%s (%s 1)" % (self.entry, self.noun), d.sizes[1] // 2)
    def result(self, c, d): return c.tree_build_batch(d.sizes, L, LS, LD, d.init_mu, SIG2, 2)[:2]
    def member(self, result, b): return [a[b] for a in bits(result)]


class ForestTg(ForestSrc):
    """the forest targets' weights, member by member"""
    entry, noun = "hgmm_tree_set_target_weights_batch", "target"

    def upload(self, c, d, clouds):
        c.set_points_batch(d.clouds)                # (the forest they are scored against: built without weights)
        c.tree_build_batch(d.sizes, L, LS, LD, d.init_mu, SIG2, 2)
        c.tree_set_targets_batch(clouds)

    def hand_over(self, c, vx): c.tree_set_targets_batch_from_voxels(vx, weighted=False)
    def weigh(self, c, d): c.tree_set_target_weights_batch(self.weights(d))
    def off(self, c): c.tree_set_target_weights_batch(None)
    def refused(self, c, d): c.tree_set_target_weights_batch([d.w[0], with_nan(d.w[1])])
    def result(self, c, d): return c.tree_score_batch(None, None, 1.0, LAMBDA_C)


SETS = {"src": Src(), "flat": Flat(), "tgt": Tgt(), "forest_src": ForestSrc([True, True]),
        "forest_src_one_none": ForestSrc([True, False]), "forest_tg": ForestTg([True, True]),
        "forest_tg_one_none": ForestTg([True, False])}


@pytest.fixture(params=sorted(SETS))
def case(request, world):
    """the set under test with its weights in force on `ctx` -> (set, ctx, plain, voxel members, data, the weighted and the
    never-weighted result of the same cloud)"""
    import hgmm_amd
    s = SETS[request.param]
    ctx, plain, vx, d = world
    s.upload(plain, d, d.clouds)
    unweighted = s.result(plain, d)
    s.upload(ctx, d, d.clouds)
    s.weigh(ctx, d)
    weighted = s.result(ctx, d)
    assert not same(weighted, unweighted)
    if isinstance(s, ForestSrc):                    # a None member keeps its unweighted bits next to a weighted one
        for b, on in enumerate(s.entries):
            assert same(s.member(weighted, b), s.member(unweighted, b)) == (not on), b
    return s, ctx, plain, vx, d, weighted, unweighted, hgmm_amd.HgmmError


def test_a_refused_upload_keeps_the_weights(case):                                              # (a)
    s, ctx, _, _, d, weighted, _, HgmmError = case
    with pytest.raises(HgmmError) as e:
        s.refused(ctx, d)
    assert str(e.value) == s.message(d)
    assert same(s.result(ctx, d), weighted)


@pytest.mark.parametrize("route", ["upload", "hand_over"])
def test_a_replaced_cloud_drops_the_weights(case, route):                                       # (b)
    s, ctx, plain, vx, d = case[:5]
    for c in (plain, ctx):
        if route == "upload":
            s.upload(c, d, d.others)
        else:
            s.hand_over(c, vx[id(c)])
    assert same(s.result(ctx, d), s.result(plain, d))


def test_none_takes_the_weights_off(case):                                                      # (c)
    s, ctx, _, _, d, _, unweighted, _ = case
    s.off(ctx)
    assert same(s.result(ctx, d), unweighted)
