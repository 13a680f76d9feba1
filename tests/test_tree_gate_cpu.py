"""The Mahalanobis gate of the registration E-step (hgmm_tree_set_reg_gate), the parts that need no GPU: in the float64
E-step the GPU tests compare against (oracle.hgmm_tree.reg_e_step(gate=...)) a gate that every pair passes changes no bit,
and the mirrors refuse a gate that is not a positive number before they touch the library."""
import inspect

import numpy as np
import pytest

from conftest import load_golden
from oracle import hgmm_tree


def test_restatement_with_the_gate_off_is_the_oracle_bit_for_bit():
    """The gated and the ungated E-step are one function, so "off is the oracle" would compare it with itself.  What still
    runs distinct code: a finite gate that every pair passes (1e300) evaluates every quadratic form and makes every
    comparison, and must give the ungated moments and the ungated register trajectory bit for bit, leave no pair out, and
    count as pairs exactly the contributions of reg_descent.  On both records (2 912 and 10 957 pairs at rot10)."""
    for L, record in ((2, "hgmm_reg_L2.npz"), (4, "hgmm_reg_L4.npz")):
        g = load_golden(record)
        assert L == int(g["L"])
        tree = (g["pi"], g["mu"], g["cov"], L, float(g["lambda_c"]))
        for deg in (10, 30):
            X = g["rot%d_target" % deg]
            ref = hgmm_tree.reg_e_step(X, *tree)
            off = hgmm_tree.reg_e_step(X, *tree, report=True)
            e = hgmm_tree.reg_e_step(X, *tree, gate=1e300, report=True)
            print("L=%d rot%d: %d pairs" % (L, deg, e.pairs))
            for a, b, c in zip(ref, e[:3], off[:3]):
                assert np.array_equal(a, b) and np.array_equal(a, c)
            assert e.gated == 0 and e.pairs > 0 and e.pairs == hgmm_tree.reg_descent(X, *tree).contrib.sum()
            assert off.gated == 0 and off.pairs == e.pairs and off.margin == np.inf
            # and a finite gate leaves pairs out, each of them a pair the ungated step counts
            e16 = hgmm_tree.reg_e_step(X, *tree, gate=16.0, report=True)
            assert e16.pairs == e.pairs and 0 < e16.gated < e.pairs
            assert (e16.m0 <= e.m0).all() and e16.m0.sum() < e.m0.sum()
        # the loop around it: with the gate that everything passes, the ungated trajectory
        X = g["rot10_target"]
        o_rot, o_t, o_q, o_tr = hgmm_tree.register(X, *tree, 5, 1e-4)
        rot, t, q, tr = hgmm_tree.register(X, *tree, 5, 1e-4, gate=1e300)
        assert len(tr) == len(o_tr)
        for a, b in zip(tr, o_tr):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        assert np.array_equal(rot, o_rot) and np.array_equal(t, o_t) and np.array_equal(q, o_q)


class _Untouchable:
    """a context that fails the test if anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the gate was checked" % name)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), -np.inf])
def test_mirrors_refuse_a_bad_gate_before_touching_the_library(bad):
    from hgmm_amd.hgmm import hgmm_gpu as H
    P = np.random.RandomState(0).rand(50, 3)
    ctx = _Untouchable()
    with pytest.raises(ValueError, match="maha2_gate"):
        H.GMMTree(P, tree_level=1, ctx=ctx, maha2_gate=bad)
    gt = H.GMMTree(None, tree_level=1, ctx=ctx)
    with pytest.raises(ValueError, match="maha2_gate"):
        gt.registration(P, maha2_gate=bad)
    with pytest.raises(ValueError, match="maha2_gate"):
        H.registration_gmmtree(P, P, tree_level=1, ctx=ctx, maha2_gate=bad)
    with pytest.raises(ValueError, match="maha2_gate"):
        H.registration_gmmtree(P, P, starts=[H.RigidTransformation()], tree_level=1, ctx=ctx, maha2_gate=bad)
    with pytest.raises(ValueError, match="maha2_gate"):
        H.registration_gmmtree_batch([(P, P)], tree_level=1, ctx=ctx, maha2_gate=bad)


def test_gate_arguments_and_constants():
    from hgmm_amd import Context
    from hgmm_amd._native import CHI2_3_99, CHI2_3_999
    from hgmm_amd.hgmm import hgmm_gpu as H
    assert CHI2_3_999 == 16.27 and H.CHI2_3_999 == CHI2_3_999 and CHI2_3_99 < CHI2_3_999
    assert inspect.signature(H.GMMTree.__init__).parameters["maha2_gate"].default is None
    assert inspect.signature(H.GMMTree.registration).parameters["maha2_gate"].default is None
    assert inspect.signature(H.registration_gmmtree_batch).parameters["maha2_gate"].default is None
    assert list(inspect.signature(Context.tree_set_reg_gate).parameters) == ["self", "maha2_gate"]
    assert list(inspect.signature(Context.tree_get_reg_gate).parameters) == ["self"]
    # None leaves the context alone; inf is a value (off for the call); numbers come back as floats
    assert H._gate_arg(None) is None and H._gate_arg(np.inf) == np.inf and H._gate_arg(9) == 9.0


def test_gate_scope_restores_the_contexts_gate_when_the_call_raises():
    """_reg_gate (what every mirror wraps its library calls in) against a recording stand-in: set for the calls inside, the
    previous value back afterwards -- also when they raise -- and nothing touched for None."""
    from hgmm_amd.hgmm import hgmm_gpu as H

    class Recorder:
        def __init__(self):
            self.gate, self.calls = 25.0, []

        def tree_get_reg_gate(self):
            return self.gate

        def tree_set_reg_gate(self, g):
            self.gate = g
            self.calls.append(g)

    ctx = Recorder()
    with pytest.raises(RuntimeError):
        with H._reg_gate(ctx, 9.0):
            assert ctx.gate == 9.0
            raise RuntimeError("midway")
    assert ctx.gate == 25.0 and ctx.calls == [9.0, 25.0]
    with H._reg_gate(ctx, None):
        pass
    assert ctx.calls == [9.0, 25.0]
