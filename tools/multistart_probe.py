#!/usr/bin/env python3
"""What K start poses cost in one launch set (profiles/tree_multistart.md): a bun000 tree at L = 5 with the bun045 scan as
target, K in {1, 8, 27, 64} start poses, 20 iterations each (tol = 0: no hypothesis stops early, so both sides do the same
work).  One tree_register_multi + tree_score_multi against K serial tree_register + tree_score calls on the same context:
wall time (median of REPS repeats after a warm-up) and, in a profiled pass of their own, the kernel times of the library's
profiler (hgmm_profile_*, kernel ids tree_reg and tree_score: the E-step and score launches).
    python tools/multistart_probe.py [--markdown]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hgmm_amd         # noqa: E402
from hgmm_amd.hgmm.hgmm_gpu import buildGMMTree, rotation_starts   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LC, L, ITERS, REPS = 0.01, 5, 20, 7


def starts(K, centre):
    """K poses about ``centre``: the identity first, then a widening grid of rotations"""
    if K == 1:
        s = rotation_starts((0,), centre)
    elif K == 8:
        s = rotation_starts((-10, 10), centre)
    elif K == 27:
        s = rotation_starts((-15, 0, 15), centre)
    else:
        s = rotation_starts((-15, -5, 5, 15), centre)
    assert len(s) == K
    return np.stack([p.rot for p in s]), np.stack([p.t for p in s])


def multi(ctx, rot0, t0):
    rot, t, iters, _, _, _ = ctx.tree_register_multi(rot0, t0, 1.0, LC, ITERS, 0.0)
    return rot, t, iters, ctx.tree_score_multi(rot, t, 1.0, LC)


def serial(ctx, rot0, t0):
    rots, ts, its, sums = [], [], [], []
    for k in range(len(rot0)):
        rot, t, done, _, _, _ = ctx.tree_register(rot0[k], t0[k], 1.0, LC, ITERS, 0.0)
        rots.append(rot), ts.append(t), its.append(done)
        sums.append(ctx.tree_score(rot, t, 1.0, LC, want=())[0])
    return np.stack(rots), np.stack(ts), np.array(its), np.stack(sums)


def wall_ms(ctx, call):
    call()
    ctx.synchronize()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def kernel_ms(ctx, call):
    """-> (ms in the registration E-step launches, their number, ms in the score launches, their number) of ONE call"""
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile_enable(True)
    call()
    ctx.synchronize()
    ctx.profile_enable(False)
    reg, n_reg = ctx.profile_get("tree_reg")
    sc, n_sc = ctx.profile_get("tree_score")
    return reg, n_reg, sc, n_sc


def main():
    ctx = hgmm_amd.Context(0)
    P = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    target = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    pi, mu, cov = buildGMMTree(P, L, 20, 1e-4, sig2=0.004, ctx=ctx)
    ctx.tree_set_nodes(L, pi, mu, cov)
    ctx.tree_set_target(target)
    md = "--markdown" in sys.argv
    print("bun000 tree, L = %d; target bun045, %d points; %d iterations per start, tol = 0; median of %d repeats"
          % (L, len(target), ITERS, REPS))
    if md:
        print("| K | multi: wall | K serial calls: wall | ratio | multi: E-step kernels (launches) | serial: E-step kernels (launches) "
              "| multi: score kernel | serial: score kernels | best fitness |")
        print("|---|---|---|---|---|---|---|---|---|")
    for K in (1, 8, 27, 64):
        rot0, t0 = starts(K, target.mean(axis=0))
        a, b = multi(ctx, rot0, t0), serial(ctx, rot0, t0)
        same = all(np.array_equal(x, y) for x, y in zip(a, b))
        wm, ws = wall_ms(ctx, lambda: multi(ctx, rot0, t0)), wall_ms(ctx, lambda: serial(ctx, rot0, t0))
        km, ks = kernel_ms(ctx, lambda: multi(ctx, rot0, t0)), kernel_ms(ctx, lambda: serial(ctx, rot0, t0))
        fit = (a[3][:, 1] / a[3][:, 0]).max()
        if md:
            print("| %d | %.2f ms | %.2f ms | %.2f | %.3f ms (%d) | %.3f ms (%d) | %.3f ms | %.3f ms | %.3f |"
                  % (K, wm, ws, wm / ws, km[0], km[1], ks[0], ks[1], km[2], ks[2], fit))
        else:
            print("K = %2d: multi %.2f ms wall, %d serial calls %.2f ms wall (ratio %.2f); E-step kernels %.3f ms in %d launches vs "
                  "%.3f ms in %d; score kernels %.3f ms vs %.3f ms; best fitness %.3f; bitwise the serial calls: %s"
                  % (K, wm, K, ws, wm / ws, km[0], km[1], ks[0], ks[1], km[2], ks[2], fit, same))
        assert same, "K = %d: the multi call and the serial calls differ" % K
    ctx.close()


if __name__ == "__main__":
    main()
