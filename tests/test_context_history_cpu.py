"""The op table of the context-history tests (tests/_history_ops.py), checked without a device: the shapes separate the
buffer sizes, the exclusions name real entries and give reasons, the names and the orders are what the GPU module assumes."""
import numpy as np

import _history_ops as H


def by_base():
    pairs = {}
    for name, op in H.OPS.items():
        if op.size in H.SIZES:
            assert name.endswith("_" + op.size), name
            pairs.setdefault(name[:-len(op.size) - 1], {})[op.size] = op
    return pairs


def test_every_family_has_both_sizes_and_the_table_covers_every_family():
    pairs = by_base()
    assert all(set(p) == set(H.SIZES) for p in pairs.values()), {b: sorted(p) for b, p in pairs.items()}
    assert {op.family for op in H.OPS.values()} == set(H.FAMILIES)
    for base, p in pairs.items():
        assert p["large"].family == p["small"].family, base
    assert [op.size for op in H.OPS.values()].count("mixed") == 1 and H.OPS["handles"].family == "handles"


def test_large_exceeds_small_in_every_sizing_dimension():
    for base, p in by_base().items():
        large, small = p["large"].dims, p["small"].dims
        assert large and set(large) == set(small), base
        for dim in large:
            assert large[dim] > small[dim] >= 1, (base, dim, large[dim], small[dim])


def test_the_data_is_what_the_shapes_say():
    assert [len(a) for a in H.members("large")] == [3097, 1388, 1] and [len(a) for a in H.members("small")] == [310]
    assert [len(a) for a in H.members("large", "float64", False)] == [3097, 1388, 415]
    assert len(H.cloud("large")) == 3097 and len(H.cloud("small")) == 310
    for size in H.SIZES:
        s, g = H.SHAPES[size], H.reg_case(size)
        assert (g.L, g.T) == (s.L, H.n_total(s.L)) and g.pi.shape == (g.T,) and g.target.shape == g.points.shape
        pairs, ids, rot, t, sigma = H.l2_case(size)
        assert [(len(p[0]), len(p[2])) for p in pairs] == list(s.l2) and len(ids) == len(rot) == len(t) == len(sigma) == s.l2_R
        assert (sigma > 0).all() and ids.max() < len(pairs)
        assert len(H._voxel_clouds(size)) == s.B
    assert (70, 300) in H.SHAPES["large"].l2 and len(H._voxel_clouds("small")[0]) == 3
    # seeded: a second draw is the first one
    assert np.array_equal(H.rows_of(310, 72, 5), H.rows_of(310, 72, 5)) and np.array_equal(H.poses(7)[0], H.poses(7)[0])
    w = H.weights(310, 21)
    assert (w >= 0).all() and (w == 0).any() and (w > 0).any() and not w.flags.writeable


def test_op_names_are_unique_and_the_orders_cover_the_table():
    with open(H.__file__) as f:
        text = f.read()
    import re
    registered = re.findall(r'^@register\("(\w+)"', text, re.M)
    assert len(registered) == len(set(registered)) and len(H.OPS) == 2 * len(registered) + 1
    gsg = H.grow_shrink_grow()
    large, small = H.of_size("large"), H.of_size("small")
    assert gsg == large + small + large and set(large) | set(small) == set(H.OPS)
    assert all(H.OPS[n].size != "small" for n in large) and all(H.OPS[n].size != "large" for n in small)


def test_the_shuffle_seeds_give_three_different_orders():
    orders = [tuple(H.shuffled(seed)) for seed in H.SHUFFLE_SEEDS]
    assert len(H.SHUFFLE_SEEDS) == 3 and len(set(orders)) == 3
    assert all(sorted(o) == sorted(H.OPS) for o in orders)
    assert tuple(H.shuffled(H.SHUFFLE_SEEDS[0])) == orders[0]


def test_exclusions_name_declared_entries_and_give_reasons():
    declared = H.declared_entries()
    assert len(declared) == len(set(declared)) > 100
    for probe in ("hgmm_create", "hgmm_last_error", "hgmm_num_points", "hgmm_points_count", "hgmm_tree_build_batch_rows",
                  "hgmm_util_fill_f32", "hgmm_kmeans_center_f64", "hgmm_l2_cost"):
        assert probe in declared, probe
    for name, reason in H.EXCLUDED.items():
        assert name in declared, name
        assert isinstance(reason, str) and len(reason.strip()) >= 8, name


def test_the_result_comparison_sees_single_bits():
    a = (np.array([1.0, 2.0, np.nan]), np.array([3, 4], np.int32))
    assert H.same_bits(a, (a[0].copy(), a[1].copy())) and H.first_difference(a, a) is None
    assert not H.same_bits(a, (a[0], a[1].astype(np.int64))) and not H.same_bits(a, a[:1])
    b = (np.array([1.0, np.nextafter(2.0, 3.0), np.nan]), a[1])
    assert not H.same_bits(a, b) and "first at 1" in H.first_difference(a, b)
    assert not H.same_bits((np.array([0.0]),), (np.array([-0.0]),))
    assert [x.tolist() for x in H.flat(((1, None), {"b": [2.0], "a": np.arange(2)}))] == [1, [0, 1], 2.0]
