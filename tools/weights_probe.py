#!/usr/bin/env python3
"""What per-point weights of the registration target (hgmm_tree_set_target_weights) buy and cost (profiles/tree_weights.md).

    python tools/weights_probe.py [--oracle] [--skip-gpu] [--skip-cost]

Accuracy: bun000's tree (L = 3, product defaults) <- bun045 placed by bun_conf.npz and moved by 8 deg / 5 mm (the scan pair
of tools/gate_probe.py); maxiter 30, tol 1e-6.  The target is reduced three ways -- voxel centroids at 4 mm and at 2 mm
(pointcloud_io.voxel_down_sample), and the half of the scan below its median x thinned to every eighth point -- and
registered without weights and with them (the voxel counts; 8 for a kept point of the thinned half, 1 elsewhere).  The
figure is the mean distance (mm) between the full scan at the pose the reduced target gives and at the pose the full
40 097-point target gives.  ``--oracle`` adds the NumPy column (oracle.hgmm_tree.register(w=) on oracle.build_tree's tree;
minutes of CPU time).
Cost: hipEvent time per launch (hgmm_profile_*, kernel id tree_reg) of the E-step kernel through hgmm_tree_reg_normal without
and with weights (uniform in [0.25, 4): no point is skipped) on the same context, tree, target and pose -- the 40 097-point
scan, L = 3 and L = 5: median of 7 samples of 10 launches after a warm-up, each setting twice, interleaved -- of the batched
E-step of 32 pairs (L = 5, 10 iterations, tol 0), and of the E-step on the 1 986 weighted centroids beside the full scan."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gate_probe import GOLDEN, LC, launch_us, rot_about, scan_pair       # noqa: E402


def reduced_targets(moved):
    """-> [(name, points, weights)] : the three reductions of the moved scan"""
    from hgmm_amd.pointcloud_io import voxel_down_sample
    out = []
    for mm in (4, 2):
        cen, cnt = voxel_down_sample(moved, 1e-3 * mm, return_counts=True)
        out.append(("voxel centroids %d mm" % mm, cen, cnt.astype(np.float64)))
    low = moved[:, 0] < np.median(moved[:, 0])
    kept = np.concatenate([np.nonzero(low)[0][::8], np.nonzero(~low)[0]])
    w = np.where(low[kept], 8.0, 1.0)
    out.append(("half of the scan thinned 8x", moved[kept], w))
    return out


def distance_mm(moved, pose, full_pose):
    a = moved @ pose[0].T + pose[1]
    b = moved @ full_pose[0].T + full_pose[1]
    return 1e3 * np.linalg.norm(a - b, axis=1).mean()


def accuracy_gpu(ctx):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    a, world, moved = scan_pair()
    built = GMMTree(a, tree_level=3, lambda_c=LC, ls=20, sig2=0.004, ctx=ctx)

    def run(target, w=None):
        gt = GMMTree(None, tree_level=3, lambda_c=LC, ctx=ctx)         # (a GMMTree resumes from its last pose: a new one per run)
        gt.set_nodes(built._mixingCoeff, built._mean, built._covar)
        tf = gt.registration(target, 30, 1e-6, weights=w).transformation.inverse()
        return (np.asarray(tf.rot), np.asarray(tf.t)), int(gt.n_iter_)

    full, it_full = run(moved)
    rows = []
    for name, pts, w in reduced_targets(moved):
        pu, iu = run(pts)
        pw, iw = run(pts, w)
        rows.append((name, len(pts), distance_mm(moved, pu, full), iu, distance_mm(moved, pw, full), iw))
    return rows, it_full


def accuracy_oracle():
    from oracle import hgmm_tree
    a, world, moved = scan_pair()
    T = hgmm_tree.n_total(3)
    idx = np.random.RandomState(72).randint(T, size=T)
    pi, mu, cov, _ = hgmm_tree.build_tree(a, 3, 20, 1e-4, idx, 0.004)

    def run(target, w=None):
        tr = hgmm_tree.register(target, pi, mu, cov, 3, LC, 30, 1e-6, w)[3]
        return (tr[-1][0], tr[-1][1]), len(tr)

    full, it_full = run(moved)
    rows = []
    for name, pts, w in reduced_targets(moved):
        pu, iu = run(pts)
        pw, iw = run(pts, w)
        rows.append((name, len(pts), distance_mm(moved, pu, full), iu, distance_mm(moved, pw, full), iw))
        print("   oracle: %s (%d points): %.2f mm (%d it.) unweighted, %.2f mm (%d it.) weighted" % rows[-1], flush=True)
    return rows, it_full


def print_table(rows, it_full, title):
    print("%s  (the full 40 097-point target took %d iterations)" % (title, it_full))
    print("| target | points | unweighted | weighted |")
    print("|---|---|---|---|")
    for name, n, du, iu, dw, iw in rows:
        print("| %s | %d | %.2f mm (%d it.) | %.2f mm (%d it.) |" % (name, n, du, iu, dw, iw))


def report(label, off, on):
    print("%s: unweighted %s us, weighted %s us per launch: %+.2f us (%+.1f %%)"
          % (label, ["%.2f" % v for v in off], ["%.2f" % v for v in on], np.mean(on) - np.mean(off),
             100 * (np.mean(on) - np.mean(off)) / np.mean(off)))


def cost_serial(ctx):
    from hgmm_amd.hgmm.hgmm_gpu import buildGMMTree
    from hgmm_amd.pointcloud_io import voxel_down_sample
    a, world, moved = scan_pair()
    w = np.random.RandomState(11).uniform(0.25, 4.0, len(world))
    cen, cnt = voxel_down_sample(world, 0.004, return_counts=True)
    for L in (3, 5):
        pi, mu, cov = buildGMMTree(a, L, 20, 1e-4, sig2=0.004, ctx=ctx)
        ctx.tree_set_nodes(L, pi, mu, cov)
        ctx.tree_set_target(world)                 # the aligned scan: the accumulation is at its fullest
        call = lambda: ctx.tree_reg_normal(None, None, 1.0, LC)
        res = {False: [], True: []}
        for weighted in (False, True, False, True):        # (each twice, interleaved: drift shows as a difference between the passes)
            ctx.tree_set_target_weights(w if weighted else None)
            res[weighted].append(launch_us(ctx, call)[0])
        ctx.tree_set_target_weights(None)
        report("serial, L = %d, N = %d: tree_reg_estep_kernel<4>" % (L, len(world)), res[False], res[True])
        full_us = np.mean(res[False])
        ctx.tree_set_target(cen)
        ctx.tree_set_target_weights(cnt)
        small = [launch_us(ctx, call)[0] for _ in range(2)]
        print("serial, L = %d: the %d count-weighted 4 mm centroids %s us per launch against %.2f us for the full %d points "
              "(%.1fx)" % (L, len(cen), ["%.2f" % v for v in small], full_us, len(world), full_us / np.mean(small)))


def cost_batch(ctx, B=32, L=5, iters=10):
    a = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    b = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    srcs, tgts = [], []
    for k in range(B):
        src = a if k % 2 == 0 else b
        c = src.mean(axis=0)
        R = rot_about([0.2 + 0.01 * k, 1.0, 0.1], 3.0 + 0.2 * k)
        srcs.append(src)
        tgts.append((src[k % 3::3] - c) @ R.T + c + np.array([0.002, -0.001, 0.0015]))
    ws = [np.random.RandomState(11 + k).uniform(0.25, 4.0, len(t)) for k, t in enumerate(tgts)]
    T = 8 * (8 ** L - 1) // 7
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch(srcs)
    ctx.tree_build_batch([len(s) for s in arrs], L, 20, 1e-4, np.stack([s[idx] for s in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch(tgts)
    rot0, t0 = np.tile(np.eye(3), (B, 1, 1)), np.zeros((B, 3))
    res = {False: [], True: []}
    for weighted in (False, True, False, True):
        ctx.tree_set_target_weights_batch(ws if weighted else None)
        us, _ = launch_us(ctx, lambda: ctx.tree_register_batch(rot0, t0, 1.0, LC, iters, 0.0), launches=1)
        res[weighted].append(us)
    ctx.tree_set_target_weights_batch(None)
    report("batch of %d pairs, L = %d, %d iterations: forest_reg_estep_kernel<4>" % (B, L, iters), res[False], res[True])


def main():
    if "--skip-gpu" not in sys.argv:
        import hgmm_amd
        ctx = hgmm_amd.Context(0)
        print_table(*accuracy_gpu(ctx), "GPU (GMMTree.registration(weights=...)):")
        if "--skip-cost" not in sys.argv:
            cost_serial(ctx)
            cost_batch(ctx)
        ctx.close()
    if "--oracle" in sys.argv:
        print_table(*accuracy_oracle(), "oracle (oracle.hgmm_tree.register(w=)):")


if __name__ == "__main__":
    main()
