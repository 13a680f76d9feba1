#!/usr/bin/env python3
"""SHA-256 of every output of the flat EM entry points, for comparing two builds of the library bit for bit:

    python tools/flat_bits.py --lib PATH > bits.txt        (once per library, one process each; then diff)

E-step (constant-shift and row-maximum loop: table, lpn, arg-max, mean), predict, log_prob, stats, M-step (log and plain
responsibilities) and a 2-iteration train, at J = 63, 64, 800, 1025 on N = 3000 points, without and with per-point
weights.  A one-off for host-side refactorings (profiles/flat_host_refactor.md); not part of the suite."""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hgmm_amd
from hgmm_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True, help="the libhgmm_hip.so to load")
args = ap.parse_args()
_native.load_library(os.path.abspath(args.lib))
ctx = hgmm_amd.Context(0)
N = 3000


def sha(a):
    a = a.get() if hasattr(a, "get") else a
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a)).tobytes()).hexdigest()[:32]


def line(J, weighted, name, *arrays):
    print("J=%-4d %s %-22s %s" % (J, "weighted" if weighted else "plain   ", name, " ".join(sha(a) for a in arrays)), flush=True)


for J in (63, 64, 800, 1025):
    rs = np.random.RandomState(J)
    X = rs.rand(N, 3).astype(np.float32)
    mu = rs.rand(J, 3).astype(np.float32)
    inv = (1.0 / np.sqrt(0.005 + 0.05 * rs.rand(J, 3))).astype(np.float32)
    w = rs.rand(J).astype(np.float32) + 0.01
    w /= w.sum()
    s = (0.25 + 3.75 * rs.rand(N)).astype(np.float32)
    s[::10] = 0.0
    cov0, w0 = np.full((J, 3), 0.05, np.float32), (np.ones(J) / J).astype(np.float32)
    for weighted in (False, True):
        ctx.set_points(X)
        ctx.flat_set_weights(s if weighted else None)
        mean, lr, lpn, _ = ctx.flat_estep(inv, mu, w, "diag", "W", want_lpn=True)
        line(J, weighted, "estep constant-shift", lr, lpn, np.float64(mean))
        mean, lr2, lpn, am = ctx.flat_estep(inv, mu, w, "diag", "W", want_lpn=True, want_argmax=True)
        line(J, weighted, "estep row-maximum", lr2, lpn, am, np.float64(mean))
        mean = ctx.flat_estep(inv, mu, w, "diag", "W", want_log_resp=False)[0]
        line(J, weighted, "estep mean only", np.float64(mean))
        d_mean = ctx.flat_estep(ctx.to_device(inv), ctx.to_device(mu), ctx.to_device(w), "diag", "W", want_log_resp=False)[0]
        line(J, weighted, "estep device params", np.float64(float(d_mean)))
        line(J, weighted, "predict", ctx.flat_predict(inv, mu, w, "diag", "W"))
        line(J, weighted, "log_prob", ctx.flat_log_prob(inv, mu, "diag"))
        st = ctx.flat_stats(inv, mu, w, "diag", "W")
        line(J, weighted, "stats", st[0], np.float64(st[1]), np.float64(st[2]))
        line(J, weighted, "mstep log", *ctx.flat_mstep(lr.exp(), "diag", "W", centre_hint=mu))
        line(J, weighted, "mstep plain", *ctx.flat_mstep(np.exp(lr.get()), "diag", "W", centre_hint=mu))
        line(J, weighted, "mstep log, device out", *ctx.flat_mstep(lr.exp(), "diag", "W", centre_hint=mu, device_out=True))
        line(J, weighted, "train 2 iterations", *ctx.flat_train(2, 0.0, mu, cov0, w0, "diag", "W")[:5])
ctx.close()
