"""The device L2 solve (hgmm_l2_solve, hgmm_l2_solve_each) held to a fresh context's bits after other work on the context,
the way tests/test_context_history_gpu.py holds the ops of tests/_history_ops.py: at the LARGE and the SMALL shape of that
table's L2 case, on recording contexts, with ops of other families -- the device-loop registration of a forest of B = 3
pairs among them, whose hand-over block the solve's progress words share -- and solves of the other size in between.

The solves run on ``_history_ops.recording_context()``, so the entries they call are noted in ``_history_ops.REACHED`` like
those of the table's own ops."""
import numpy as np
import pytest

import _history_ops as H

pytestmark = pytest.mark.gpu

SIZES = H.SIZES
BETWEEN = ("forest_register_large", "tree_register_large", "flat_fit_diag_large", "l2_large", "kmeans_batch_large")


def solve(c, size):
    """l2_set_pairs + the device BFGS solve of the table's L2 hypotheses from random (non-unit) quaternions: with one limit for
    all (hgmm_l2_solve) and with each hypothesis' own (hgmm_l2_solve_each) -> flat tuple of every output"""
    pairs, ids, _, t, sigma = H.l2_case(size)
    R = len(ids)
    thetas = np.concatenate([np.random.RandomState(9).randn(R, 4), t], axis=1)
    c.l2_set_pairs(pairs)
    one = c.l2_solve(ids, thetas, sigma, 4, 1e-5)
    each = c.l2_solve(ids, thetas, sigma, 1 + np.arange(R) % 3, np.where(np.arange(R) % 2, 1e-2, 1e-6))
    return H.flat((one, each))


def fresh(size):
    c = H.recording_context()
    try:
        return solve(c, size)
    finally:
        c.close()


@pytest.fixture(scope="module")
def refs():
    out = {}
    for size in SIZES:
        a, b = fresh(size), fresh(size)
        for x in a:
            x.setflags(write=False)
        out[size] = (a, H.first_difference(b, a))
    return out


def test_fresh_contexts_agree_bit_for_bit(refs):
    for size in SIZES:
        assert refs[size][1] is None, (size, refs[size][1])
        assert len(refs[size][0]) == 12
    nit = refs["large"][0][3]
    assert nit.max() >= 1 and (refs["large"][0][9] <= 3).all()               # (steps were taken; the own limits hold)


def test_solve_after_other_families_and_the_other_size(refs):
    c = H.recording_context()
    try:
        order = ["large"]
        for name in BETWEEN:
            order += [name, "small", "large"]
        prev = "(a fresh context)"
        for at, what in enumerate(order):
            if what in SIZES:
                diff = H.first_difference(solve(c, what), refs[what][0])
                assert diff is None, "the %s solve (step %d, after %s) differs from its fresh context: %s" % (what, at, prev, diff)
            elif what == "forest_register_large":
                with c.config(reg_device_solve=1):                         # B = 3 registrations through the device loop
                    H.OPS[what].fn(c)
            else:
                H.OPS[what].fn(c)
            prev = what
    finally:
        c.close()


def test_solves_inside_a_seeded_shuffle_of_the_whole_table(refs):
    """the first order of test_context_history_gpu.py's seeded shuffles -- every op of the table, both sizes -- with a solve
    after every third op, the sizes alternating; the solves and the ops of the L2 family are compared with fresh contexts"""
    order = H.shuffled(H.SHUFFLE_SEEDS[0])
    l2_fresh = {name: H.run_fresh(name) for name in order if H.OPS[name].family == "l2"}
    c = H.recording_context()
    try:
        for at, name in enumerate(order):
            out = H.OPS[name].fn(c)
            if name in l2_fresh:
                diff = H.first_difference(out, l2_fresh[name])
                assert diff is None, "%s (op %d) differs from its fresh context with solves in the order: %s" % (name, at, diff)
            if at % 3 == 2:
                size = SIZES[(at // 3) % 2]
                diff = H.first_difference(solve(c, size), refs[size][0])
                assert diff is None, "the %s solve after %s (op %d) differs from its fresh context: %s" % (size, name, at, diff)
    finally:
        c.close()


def test_a_refused_solve_changes_no_neighbour(refs):
    import hgmm_amd
    c = H.recording_context()
    try:
        before = H.OPS["l2_large"].fn(c)
        pairs, ids, _, t, sigma = H.l2_case("large")
        thetas = np.concatenate([np.random.RandomState(9).randn(len(ids), 4), t], axis=1)
        with pytest.raises(hgmm_amd.HgmmError, match="max_iter < 1"):
            c.l2_solve(ids, thetas, sigma, 0, 1e-5)
        with pytest.raises(hgmm_amd.HgmmError, match="sigma not positive"):
            c.l2_solve(ids, thetas, -sigma, 4, 1e-5)
        assert H.first_difference(solve(c, "large"), refs["large"][0]) is None
        assert H.first_difference(H.OPS["l2_large"].fn(c), before) is None
    finally:
        c.close()


def test_the_solve_entries_are_reached_on_recording_contexts(refs):
    assert {"hgmm_l2_solve", "hgmm_l2_solve_each"} <= H.REACHED
    assert {"hgmm_l2_solve", "hgmm_l2_solve_each"} <= set(H.declared_entries())
