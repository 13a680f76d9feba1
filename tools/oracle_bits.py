#!/usr/bin/env python3
"""SHA-256 of every output of the float64 tree oracle, for comparing two checkouts bit for bit (CPU only):

    python tools/oracle_bits.py --root PATH > bits.txt        (once per checkout, one process each; then diff)

A one-off for the fold of the oracle's copies into oracle/hgmm_tree.py (profiles/oracle_descent.md); not part of the suite.
A checkout that still has tests/_gate_oracle.py is read through its old names (``reg_e_step``, ``gated_*``, ``weighted_*``),
any other through ``reg_e_step / register / build_tree`` with ``w=``, ``gate=``, ``report=``.  A line is labelled by the
old function that covered the case (via plain / gated / weighted), so that every old copy is held against the one function.

Registration: records hgmm_reg_L2 and hgmm_reg_L4, targets rot10 and rot30, w in {None, ones, weights_for}, gate in
{inf, 25, 16, 9}: the moments, the gate's diagnostics (finite gates), a five-iteration register trace (tol 0) and every
field of reg_descent.  ``gate = inf`` through the old gated path is left out: it compared every form against inf and so
dropped a NaN form, the one intended difference.
Build: 700 bunny points at L = 2 and 3 000 at L = 3 (tests/test_tree_source_weights_cpu.py), w in {None, ones, integer
counts}: the tables, the q trace, the iterations, the per-level assignments."""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True, help="the checkout whose oracle is hashed")
root = os.path.abspath(ap.parse_args().root)
sys.path[:0] = [root, os.path.join(root, "tests")]
from conftest import GOLDEN, load_golden                              # noqa: E402
from oracle import hgmm_tree as H                                     # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(H.__file__))) == root

if os.path.exists(os.path.join(root, "tests", "_gate_oracle.py")):   # ---- the old names
    import _gate_oracle as G
    import _source_weight_oracle as S
    import _weight_oracle as W
    weights_for = W.weights_for

    def estep(via, X, tree, w, gate):
        if via == "gated":
            return G.gated_reg_e_step(X, *tree, gate)[:3]
        return H.reg_e_step(X, *tree) if via == "plain" else W.weighted_reg_e_step(X, *tree, w, gate)

    def diagnostics(X, tree, w, gate):
        return G.gated_reg_e_step(X, *tree, gate)[3:]

    def register(via, X, tree, w, gate):
        """-> (the trace's arrays, what the loop returns besides the trace)"""
        if via == "gated":
            out = G.gated_register(X, *tree, gate, 5, 0.0)
            return [a for it in out[2] for a in it[:3] + tuple(it[3][:3])], ()
        out = H.register(X, *tree, 5, 0.0) if via == "plain" else W.weighted_register(X, *tree, 5, 0.0, w, gate)
        return [a for it in out[3] for a in it], out[:3]

    def build(via, X, L, idx, w):
        return H.build_tree(X, L, LS, LD, idx, SIG2) if via == "plain" else S.weighted_build_tree(X, L, LS, LD, X[idx], SIG2, w)
else:                                                                 # ---- the one function each
    from _tree_helpers import weights_for

    def estep(via, X, tree, w, gate):
        return H.reg_e_step(X, *tree, w, gate)

    def diagnostics(X, tree, w, gate):
        return H.reg_e_step(X, *tree, w, gate, report=True)[3:]

    def register(via, X, tree, w, gate):
        out = H.register(X, *tree, 5, 0.0, w, gate)
        return [a for it in out[3] for a in it], () if via == "gated" else out[:3]

    def build(via, X, L, idx, w):
        return H.build_tree(X, L, LS, LD, idx, SIG2) if via == "plain" else H.build_tree(X, L, LS, LD, None, SIG2, w=w, init_mu=X[idx])

LS, LD, SIG2 = 20.0, 1e-4, 0.004


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(np.asarray(a))
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes())
    return h.hexdigest()[:32]


def vias(w, gate):
    """the old functions that covered a case"""
    return (["plain"] if w is None and np.isinf(gate) else []) + (["gated"] if w is None and np.isfinite(gate) else []) + ["weighted"]


for record in ("hgmm_reg_L2", "hgmm_reg_L4"):
    g = load_golden(record + ".npz")
    tree = (g["pi"], g["mu"], g["cov"], int(g["L"]), float(g["lambda_c"]))
    for deg in (10, 30):
        X = g["rot%d_target" % deg]
        where = "%s rot%d" % (record, deg)
        d = H.reg_descent(X, *tree)
        for field in d._fields:
            print("%s reg_descent.%-12s %s" % (where, field, sha([getattr(d, field)])), flush=True)
        for wname, w in (("none", None), ("ones", np.ones(len(X))), ("weights_for", weights_for(len(X)))):
            for gate in (np.inf, 25.0, 16.0, 9.0):
                case = "%s w=%-11s gate=%-4g" % (where, wname, gate)
                for via in vias(w, gate):
                    print("%s via %-8s estep    %s" % (case, via, sha(estep(via, X, tree, w, gate))), flush=True)
                    trace, ret = register(via, X, tree, w, gate)
                    print("%s via %-8s register %s %s" % (case, via, sha(trace), sha(ret)), flush=True)
                if np.isfinite(gate):
                    margin, pairs, gated = diagnostics(X, tree, w, gate)
                    print("%s margin %r pairs %d gated %d" % (case, float(margin), pairs, gated), flush=True)

bunny = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
rng = np.random.default_rng(5)                                        # (the draws of tests/test_tree_source_weights_cpu.py)
for n, L in ((700, 2), (3000, 3)):
    X = bunny[rng.choice(len(bunny), n, replace=False)].astype(np.float64)
    c = rng.integers(1, 5, n)
    idx = rng.integers(0, n, H.n_total(L))
    for wname, w in (("none", None), ("ones", np.ones(n)), ("counts", c.astype(np.float64))):
        for via in (["plain"] if w is None else []) + ["weighted"]:
            pi, mu, cov, tr = build(via, X, L, idx, w)
            print("build n=%-4d L=%d w=%-6s via %-8s tables %s q %s iterations %s assignments %s"
                  % (n, L, wname, via, sha([pi, mu, cov]), sha([tr.q]), [int(i) for i in tr.iters_per_level], sha(tr.current_idx_per_level)),
                  flush=True)
