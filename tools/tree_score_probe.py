#!/usr/bin/env python3
"""What the tree score costs (profiles/tree_score.md): hipEvent time per launch (hgmm_profile_*) of the registration
E-step kernel tree_reg_estep_kernel<4> (through hgmm_tree_reg_normal) and of tree_score_kernel on the same tree, target
and pose -- bun000 at L = 5 (40 256 points) and a 10^6-point cloud at L = 4 -- and the wall time score=True adds to a
32-pair registration_gmmtree_batch.
    python tools/tree_score_probe.py [--skip-pairs]
On a checkout without hgmm_tree_score (the parent commit) only the E-step kernel is timed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hgmm_amd         # noqa: E402
from hgmm_amd.hgmm.hgmm_gpu import buildGMMTree, registration_gmmtree_batch   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LC = 0.01
REPS = 50


def rot_about(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def per_launch(ctx, name, call):
    for _ in range(5):
        call()
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(REPS):
        call()
    ctx.synchronize()
    ctx.profile_enable(False)
    ms, n = ctx.profile_get(name)
    return 1e3 * ms / max(n, 1), n


def kernels(ctx, P, L, label):
    pi, mu, cov = buildGMMTree(P, L, 20, 1e-4, sig2=0.004, ctx=ctx)
    c = P.mean(axis=0)
    R = rot_about([0.2, 1.0, 0.1], 4.0)
    t = c - R @ c + np.array([0.002, -0.001, 0.0015])
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(P)
    us, n = per_launch(ctx, "tree_reg", lambda: ctx.tree_reg_normal(R, t, 1.0, LC))
    print("%s: tree_reg_estep_kernel<4>  %8.2f us per launch (%d launches)" % (label, us, n))
    if not hasattr(ctx, "tree_score"):
        return
    for want in ((), ("node", "maha2", "logp")):
        us_s, n = per_launch(ctx, "tree_score", lambda: ctx.tree_score(R, t, 1.0, LC, want=want))
        t0 = time.perf_counter()
        for _ in range(REPS):
            s, _ = ctx.tree_score(R, t, 1.0, LC, want=want)
        wall = 1e6 * (time.perf_counter() - t0) / REPS
        print("%s: tree_score_kernel %-14s %8.2f us per launch (%d launches), %.2f x the E-step kernel; the call: %.1f us wall; "
              "fitness %.4f" % (label, "(summary only)" if not want else "(+ 3 arrays)", us_s, n, us_s / us, wall, s[1] / s[0]))


def pairs_32(ctx):
    a = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
    b = np.load(os.path.join(GOLDEN, "bun045_xyz.npy"))
    pairs = []
    for k in range(32):
        src = (a if k % 2 == 0 else b).astype(np.float64)
        c = src.mean(axis=0)
        R = rot_about([0.2 + 0.01 * k, 1.0, 0.1], 3.0 + 0.2 * k)
        pairs.append((src, (src[k % 3::3] - c) @ R.T + c + np.array([0.002, -0.001, 0.0015])))
    rows = {False: [], True: []}
    for rep in range(7):
        for flag in (False, True):
            t0 = time.perf_counter()
            res, info = registration_gmmtree_batch(pairs, ctx=ctx, return_info=True, score=flag)
            rows[flag].append((time.perf_counter() - t0, info["phases_ms"].get("score", 0.0)))
    off, on = np.median([r[0] for r in rows[False][1:]]), np.median([r[0] for r in rows[True][1:]])
    print("32 pairs (full scans, L = 5), registration_gmmtree_batch, median of 6 calls: %.2f ms without, %.2f ms with score=True "
          "(+%.2f ms, %.2f %%); the score phase itself: %.3f ms; fitness %.3f .. %.3f"
          % (1e3 * off, 1e3 * on, 1e3 * (on - off), 100 * (on - off) / off, np.median([r[1] for r in rows[True][1:]]),
             min(s.fitness for s in info["score"]), max(s.fitness for s in info["score"])))


def main():
    ctx = hgmm_amd.Context(0)
    P = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    kernels(ctx, P, 5, "bun000, L = 5, N = 40256 ")
    rs = np.random.RandomState(5)
    big = P[rs.randint(len(P), size=1000000)] + 0.0005 * rs.randn(1000000, 3)
    kernels(ctx, big, 4, "resampled bunny, L = 4, N = 10^6")
    if "--skip-pairs" not in sys.argv and hasattr(ctx, "tree_score"):
        pairs_32(ctx)
    ctx.close()


if __name__ == "__main__":
    main()
