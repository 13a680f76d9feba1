"""What the tree tests of the gate and of the per-point weights share (a helper, not a conftest and not an oracle: the
float64 arithmetic they compare against is oracle/hgmm_tree.py alone): ``weights_for``, ``resident``, ``loop5``,
``same_bits``."""
import numpy as np

from oracle import hgmm_tree

I3 = np.identity(3)


def weights_for(n, seed=11):
    """the tests' weights unless stated otherwise: uniform in [0.25, 4), one in ten exactly zero"""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.25, 4.0, n)
    w[rs.uniform(size=n) < 0.1] = 0.0
    return w


def resident(ctx, g, target, w=None):
    L = int(g["L"])
    ctx.tree_set_nodes(L, g["pi"], g["mu"], g["cov"])
    ctx.tree_set_target(target)
    if w is not None:
        ctx.tree_set_target_weights(w)
    return L, float(g["lambda_c"]), hgmm_tree.n_total(L)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def loop5(ctx, lc):
    """five iterations from the identity, no stop rule -> (rot, t, iterations, q, status, trace [5, 13])"""
    return ctx.tree_register(I3, np.zeros(3), 1.0, lc, 5, 0.0, None, want_trace=True)
