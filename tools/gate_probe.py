#!/usr/bin/env python3
"""What the registration E-step's Mahalanobis gate (hgmm_tree_set_reg_gate) buys and costs (profiles/tree_gate.md).

    python tools/gate_probe.py [--oracle] [--skip-gpu] [--skip-cost]

Accuracy: bun000's tree (L = 3, product defaults) <- bun045 placed by bun_conf.npz and moved by 8 deg / 5 mm (the scan pair
of tests/test_tree_gpu.py), as it is and with 10 % / 30 % uniform clutter in its bounding box; maxiter 30, tol 1e-6; gates
inf, 25, 16, 9.  The figure is the mean distance of the registered scan (clutter left out) from its ground-truth placement.
``--oracle`` adds the NumPy column (oracle.hgmm_tree.register(gate=) on oracle.build_tree's tree; minutes of CPU time).
Cost: hipEvent time per launch (hgmm_profile_*, kernel id tree_reg) of the E-step kernel through hgmm_tree_reg_normal with the
gate off and at 16 on the same context, tree, target and pose -- bun045-sized target, L = 3 and L = 5: median of 7 samples
of 10 launches after a warm-up -- and of the batched E-step of 32 pairs (L = 5, 10 iterations, tol 0)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
LC = 0.01
GATES = (np.inf, 25.0, 16.0, 9.0)
CLUTTER = (0.0, 0.1, 0.3)


def rot_about(axis, deg):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scan_pair():
    """-> (bun000, bun045 at its ground-truth placement, the same moved by 8 deg about (0.3, 1, 0.2) and 5 mm)"""
    a = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    b = np.load(os.path.join(GOLDEN, "bun045_xyz.npy")).astype(np.float64)
    conf = np.load(os.path.join(GOLDEN, "bun_conf.npz"), allow_pickle=False)
    pose = conf["poses"][list(conf["names"]).index("bun045.ply")]
    t, (qx, qy, qz, qw) = pose[:3], pose[3:]
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    world = b @ R + t                      # bun.conf convention: p_world = R(q)^T p + t
    moved = world @ rot_about([0.3, 1.0, 0.2], 8.0).T + np.array([0.005, -0.00375, 0.00625])
    return a, world, moved


def with_clutter(target, frac):
    if not frac:
        return target
    lo, hi = target.min(axis=0), target.max(axis=0)
    return np.concatenate([target, np.random.RandomState(5).uniform(lo, hi, (int(frac * len(target)), 3))])


def error_mm(moved, world, rot, t):
    """mean distance (mm) of the scan at the loop's final pose y = rot x + t from its ground-truth placement"""
    return 1e3 * np.linalg.norm(moved @ rot.T + t - world, axis=1).mean()


def accuracy_gpu(ctx):
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    a, world, moved = scan_pair()
    built = GMMTree(a, tree_level=3, lambda_c=LC, ls=20, sig2=0.004, ctx=ctx)
    rows = {}
    for frac in CLUTTER:
        target = with_clutter(moved, frac)
        for gate in GATES:
            gt = GMMTree(None, tree_level=3, lambda_c=LC, ctx=ctx)         # (a GMMTree resumes from its last pose: a new one per run)
            gt.set_nodes(built._mixingCoeff, built._mean, built._covar)
            res = gt.registration(target, 30, 1e-6, maha2_gate=gate)
            pose = res.transformation.inverse()
            rows[frac, gate] = (error_mm(moved, world, pose.rot, pose.t), int(gt.n_iter_))
    return rows


def accuracy_oracle():
    from oracle import hgmm_tree
    a, world, moved = scan_pair()
    T = hgmm_tree.n_total(3)
    idx = np.random.RandomState(72).randint(T, size=T)
    pi, mu, cov, _ = hgmm_tree.build_tree(a, 3, 20, 1e-4, idx, 0.004)
    rows = {}
    for frac in CLUTTER:
        target = with_clutter(moved, frac)
        for gate in GATES:
            trace = hgmm_tree.register(target, pi, mu, cov, 3, LC, 30, 1e-6, gate=gate)[3]
            rows[frac, gate] = (error_mm(moved, world, *trace[-1][:2]), len(trace))
            print("   oracle: clutter %3.0f %%, gate %4g: %.2f mm after %d iterations" % (100 * frac, gate, *rows[frac, gate]),
                  flush=True)
    return rows


def print_table(rows, title):
    print(title)
    print("| target | " + " | ".join("no gate" if np.isinf(g) else "gate %g" % g for g in GATES) + " |")
    print("|---|" + "---|" * len(GATES))
    for frac in CLUTTER:
        name = "bun045 as is" if not frac else "+ %d %% clutter" % round(100 * frac)
        print("| %s | " % name + " | ".join("%.2f mm (%d it.)" % rows[frac, g] for g in GATES) + " |")


def launch_us(ctx, call, samples=7, launches=10):
    """median over ``samples`` of the mean hipEvent time (us) of ``launches`` tree_reg launches, after a warm-up"""
    for _ in range(5):
        call()
    out = []
    for _ in range(samples):
        ctx.synchronize()
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(launches):
            call()
        ctx.synchronize()
        ctx.profile_enable(False)
        ms, n = ctx.profile_get("tree_reg")
        out.append(1e3 * ms / max(n, 1))
    return float(np.median(out)), out


def cost_serial(ctx):
    from hgmm_amd.hgmm.hgmm_gpu import buildGMMTree
    a, world, moved = scan_pair()
    for L in (3, 5):
        pi, mu, cov = buildGMMTree(a, L, 20, 1e-4, sig2=0.004, ctx=ctx)
        ctx.tree_set_nodes(L, pi, mu, cov)
        ctx.tree_set_target(world)                 # the aligned scan: most pairs pass the gate, the accumulation is at its fullest
        res = {}
        for gate in (np.inf, 16.0, np.inf, 16.0):  # (each twice, interleaved: drift shows as a difference between the passes)
            ctx.tree_set_reg_gate(gate)
            res.setdefault(gate, []).append(launch_us(ctx, lambda: ctx.tree_reg_normal(None, None, 1.0, LC))[0])
        ctx.tree_set_reg_gate(np.inf)
        off, on = res[np.inf], res[16.0]
        print("serial, L = %d, N = %d: tree_reg_estep_kernel<4> off %s us, gate 16 %s us per launch: %+.2f us (%+.1f %%)"
              % (L, len(world), ["%.2f" % v for v in off], ["%.2f" % v for v in on], np.mean(on) - np.mean(off),
                 100 * (np.mean(on) - np.mean(off)) / np.mean(off)))


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
    T = 8 * (8 ** L - 1) // 7
    idx = np.random.RandomState(72).randint(T, size=T)
    arrs = ctx.set_points_batch(srcs)
    ctx.tree_build_batch([len(s) for s in arrs], L, 20, 1e-4, np.stack([s[idx] for s in arrs]), 0.004, want_tables=False)
    ctx.tree_set_targets_batch(tgts)
    rot0, t0 = np.tile(np.eye(3), (B, 1, 1)), np.zeros((B, 3))
    res = {}
    for gate in (np.inf, 16.0, np.inf, 16.0):
        ctx.tree_set_reg_gate(gate)
        us, _ = launch_us(ctx, lambda: ctx.tree_register_batch(rot0, t0, 1.0, LC, iters, 0.0), launches=1)
        res.setdefault(gate, []).append(us)
    ctx.tree_set_reg_gate(np.inf)
    off, on = res[np.inf], res[16.0]
    print("batch of %d pairs, L = %d, %d iterations: forest_reg_estep_kernel<4> off %s us, gate 16 %s us per launch: %+.2f us "
          "(%+.1f %%)" % (B, L, iters, ["%.2f" % v for v in off], ["%.2f" % v for v in on], np.mean(on) - np.mean(off),
                          100 * (np.mean(on) - np.mean(off)) / np.mean(off)))


def main():
    if "--skip-gpu" not in sys.argv:
        import hgmm_amd
        ctx = hgmm_amd.Context(0)
        print_table(accuracy_gpu(ctx), "GPU (GMMTree.registration(maha2_gate=...)):")
        if "--skip-cost" not in sys.argv:
            cost_serial(ctx)
            cost_batch(ctx)
        ctx.close()
    if "--oracle" in sys.argv:
        print_table(accuracy_oracle(), "oracle (oracle.hgmm_tree.register(gate=)):")


if __name__ == "__main__":
    main()
