#!/usr/bin/env python3
"""What the voxel-grid down-sample costs on the device beside the host function -> profiles/voxel_downsample.md.

    python tools/voxelbench.py [--out FILE] [--reps 20] [--host-reps 3] [--bench-parent FILE --bench-pr FILE]

Per case: the wall time of ``Context.voxel_down_sample`` (``_batch`` for the batch row) -- upload, launch set, download,
the median of --reps calls after two warm-up calls --, the profiler's ``voxel`` entry per call (hipEvent pair around the
launch set: bounding box, keys, sort, segment heads, centroids, with the two host round trips in between), and the host
function ``pointcloud_io.voxel_down_sample(..., return_counts=True)`` on the same box (median of --host-reps).  Every device
result is compared with the host's bit for bit before it is timed.
Cases: bun000 (40 256 float32 points) at 4 mm and 2 mm; 10^6 uniform float64 points in the unit cube at 0.02; a batch of 64
clouds (bun000 and bun045 alternating) at 4 mm, beside 64 host calls.
--bench-parent / --bench-pr: files of bench.py result lines (one JSON object per line) of the parent commit and of this
tree, taken in one session; their medians are written below the table.

The voxel result handed to build and registration on the device -> profiles/voxel_handover.md:

    python tools/voxelbench.py --handover [--root TREE] [--reps 10]        one run on one tree: ONE JSON line
    python tools/voxelbench.py --handover-report --parent-runs FILE --pr-runs FILE [--bench-parent FILE --bench-pr FILE] [--out FILE]

``--handover`` times three calls that both the parent commit and this tree offer (``voxel_size=`` of the registration
mirrors), bun000 / bun045 at 4 mm, L = 3, 20 iterations, wall clock from host arrays to results, median of --reps calls after
two warm-up calls: (1) one ``registration_gmmtree``; (2) ``registration_gmmtree_batch`` on 32 pairs, every cloud an array
object of its own (64 down-samples on either tree); (3) a chain of 33 scans -- bun000 under 33 small rotations -- registered
as 32 consecutive pairs, the inner scans the same object in two pairs.  ``--root`` names the tree whose package is imported
(a checkout of the parent commit with its library built); the line carries a digest of every result, which the report
compares between the trees.  ``--handover-report`` reads the lines of the alternating runs and writes the table: every run,
the medians, the parent's spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def median_s(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def same(got, want):
    return (np.array_equal(got[1], want[1]) and got[0].shape == want[0].shape
            and np.array_equal(np.ascontiguousarray(got[0]).view(np.uint64), np.ascontiguousarray(want[0]).view(np.uint64)))


def bench_lines(path):
    vals = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            vals.append(float(json.loads(line)["value"]))
    return vals


def handover_run(args):
    """one run on the tree --root names: a JSON line {"rows": {name: median ms}, "digest": {name: sha1 of the results}}"""
    import hashlib
    root = os.path.abspath(args.root or ROOT)
    sys.path.insert(0, root)
    import hgmm_amd
    from hgmm_amd.hgmm.hgmm_gpu import registration_gmmtree, registration_gmmtree_batch
    assert os.path.abspath(hgmm_amd.__file__).startswith(root + os.sep), (hgmm_amd.__file__, root)
    golden = os.path.join(root, "tests", "golden")
    bun000 = np.load(os.path.join(golden, "bun000_xyz.npy"))
    bun045 = np.load(os.path.join(golden, "bun045_xyz.npy"))
    ctx = hgmm_amd.Context(0)
    kw = dict(maxiter=20, ctx=ctx, tree_level=3, voxel_size=0.004)
    pairs32 = [(bun000.copy(), bun045.copy()) for _ in range(32)]
    scans = []
    for k in range(33):
        th = 0.01 * k
        rz = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
        scans.append(np.ascontiguousarray((bun000.astype(np.float64) @ rz.T).astype(np.float32)))
    chain = [(scans[k], scans[k + 1]) for k in range(32)]
    cases = [("one registration_gmmtree", lambda: [registration_gmmtree(bun000, bun045, **kw)]),
             ("registration_gmmtree_batch, 32 pairs", lambda: registration_gmmtree_batch(pairs32, **kw)),
             ("chain of 33 scans, 32 consecutive pairs", lambda: registration_gmmtree_batch(chain, **kw))]
    rows, digest = {}, {}
    for name, run in cases:
        res = run()
        h = hashlib.sha1()
        for r in res:
            tf = r.transformation
            for a in (tf.rot, tf.t, r.q):
                h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        digest[name] = h.hexdigest()
        run()
        rows[name] = 1e3 * median_s(run, args.reps)
    ctx.close()
    print(json.dumps({"root": root, "reps": args.reps, "rows": rows, "digest": digest}), flush=True)
    return 0


def handover_report(args):
    def lines(path):
        return [json.loads(l) for l in open(path) if l.strip().startswith("{")]
    par, pr = lines(args.parent_runs), lines(args.pr_runs)
    names = list(par[0]["rows"])
    out = ["# Voxel centroids straight to build and registration: this tree beside the parent commit", "",
           "`python tools/voxelbench.py --handover --reps %d`, %d runs on a checkout of the parent commit and %d on this tree in one "
           "session, alternating (parent first).  bun000 / bun045 at 4 mm, L = 3, 20 iterations; wall clock of the call from host "
           "arrays to results, per run the median of its calls after two warm-up calls.  Rows 2 and 3: 32 pairs in one "
           "`registration_gmmtree_batch(..., voxel_size=0.004)`; in row 2 every cloud is an array object of its own (64 "
           "down-samples on either tree), in row 3 the 33 scans of a chain are shared between consecutive pairs (64 "
           "down-samples on the parent, 33 here)." % (par[0]["reps"], len(par), len(pr)), "",
           "| call | parent runs, ms | parent median | parent spread | this tree runs, ms | this tree median | this tree / parent | same results |",
           "|---|---|---|---|---|---|---|---|"]
    slower = []
    for name in names:
        a, b = [r["rows"][name] for r in par], [r["rows"][name] for r in pr]
        ma, mb = float(np.median(a)), float(np.median(b))
        same_bits = len({r["digest"][name] for r in par + pr}) == 1
        if mb > max(a):
            slower.append(name)
        out.append("| %s | %s | %.3f | %.3f .. %.3f | %s | %.3f | %.2f | %s |"
                   % (name, ", ".join("%.3f" % x for x in a), ma, min(a), max(a), ", ".join("%.3f" % x for x in b), mb, mb / ma,
                      "yes" if same_bits else "NO"))
    out += ["", "No row's median is above the parent's slowest run." if not slower else
            "SLOWER THAN EVERY RUN OF THE PARENT on: %s." % "; ".join(slower)]
    if args.bench_parent and args.bench_pr:
        bp, bq = bench_lines(args.bench_parent), bench_lines(args.bench_pr)
        out += ["", "## `bench.py --gpus 1 --steps 20 --warmup 5`, parent and this tree in the same session, alternating", "",
                "| tree | runs (`value`, EM it/s) | median |", "|---|---|---|",
                "| parent | %s | %.1f |" % (", ".join("%.1f" % x for x in bp), np.median(bp)),
                "| this tree | %s | %.1f |" % (", ".join("%.1f" % x for x in bq), np.median(bq)), "",
                "This tree's median is %+.2f %% of the parent's." % (100.0 * (np.median(bq) / np.median(bp) - 1.0))]
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--handover", action="store_true")
    ap.add_argument("--handover-report", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--parent-runs", default=None)
    ap.add_argument("--pr-runs", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-pr", default=None)
    args = ap.parse_args()
    args.reps = args.reps or (10 if args.handover else 20)
    if args.handover:
        return handover_run(args)
    if args.handover_report:
        return handover_report(args)

    import hgmm_amd
    from hgmm_amd.pointcloud_io import voxel_down_sample
    ctx = hgmm_amd.Context(0)
    bun000 = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
    bun045 = np.load(os.path.join(GOLDEN, "bun045_xyz.npy"))
    uniform = np.random.RandomState(0).rand(1000000, 3)
    batch = [bun000 if k % 2 == 0 else bun045 for k in range(64)]
    cases = [("bun000 (40 256 points, float32), 4 mm", [bun000], 0.004),
             ("bun000, 2 mm", [bun000], 0.002),
             ("10^6 uniform points (float64), 0.02", [uniform], 0.02),
             ("batch of 64 bun000 / bun045 (2 571 296 points), 4 mm", batch, 0.004)]
    rows = []
    for name, clouds, v in cases:
        serial = len(clouds) == 1
        run = (lambda: [ctx.voxel_down_sample(clouds[0], v)]) if serial else (lambda: ctx.voxel_down_sample_batch(clouds, v))
        distinct = {id(c): c for c in clouds}
        want = {k: voxel_down_sample(c, v, True) for k, c in distinct.items()}
        got = run()
        bitwise = all(same(g, want[id(c)]) for g, c in zip(got, clouds))
        run()
        ctx.profile_enable(True)
        ctx.profile_reset()
        wall = median_s(run, args.reps)
        ms, launches = ctx.profile_get("voxel")
        ctx.profile_enable(False)
        host = median_s(lambda: [voxel_down_sample(c, v, True) for c in clouds], args.host_reps)
        rows.append((name, sum(len(g[1]) for g in got), max(int(g[1].max()) for g in got), wall * 1e3, ms / max(launches, 1),
                     host * 1e3, bitwise))
        print("%-58s M %8d  wall %9.3f ms  voxel entry %9.3f ms  host %10.3f ms  bitwise %s"
              % (name, rows[-1][1], rows[-1][3], rows[-1][4], rows[-1][5], bitwise), flush=True)
    info = ctx.device_info()
    info = "%s, %d compute units" % (info["name"].strip(), info["compute_units"])
    ctx.close()

    out = ["# Voxel-grid down-sample: device call beside the host function", "",
           "`python tools/voxelbench.py --reps %d --host-reps %d` on %s.  Wall: `Context.voxel_down_sample` (`_batch` in the last "
           "row) from host array to host arrays, median.  `voxel` entry: the profiler's time of the launch set per call (with "
           "its two host round trips).  Host: `pointcloud_io.voxel_down_sample(..., return_counts=True)` with `ctx=None` on "
           "the same box, median; the batch row is 64 host calls." % (args.reps, args.host_reps, info), "",
           "| case | M | largest count | device wall ms | `voxel` entry ms | host ms | host / device | bitwise equal |",
           "|---|---|---|---|---|---|---|---|"]
    for name, M, big, wall, ev, host, bitwise in rows:
        out.append("| %s | %d | %d | %.3f | %.3f | %.1f | %.0f x | %s |" % (name, M, big, wall, ev, host, host / wall, "yes" if bitwise else "NO"))
    slower = [r[0] for r in rows if r[3] >= r[5]]
    out += ["", "The device call is below the host function on every row." if not slower else
            "SLOWER THAN THE HOST FUNCTION on: %s." % "; ".join(slower)]
    if args.bench_parent and args.bench_pr:
        par, pr = bench_lines(args.bench_parent), bench_lines(args.bench_pr)
        out += ["", "## `bench.py --gpus 1 --steps 20 --warmup 5`, parent and this tree in one session, alternating", "",
                "| tree | runs (`value`, EM it/s) | median |", "|---|---|---|",
                "| parent | %s | %.1f |" % (", ".join("%.1f" % x for x in par), np.median(par)),
                "| this tree | %s | %.1f |" % (", ".join("%.1f" % x for x in pr), np.median(pr)), "",
                "This tree's median is %+.2f %% of the parent's." % (100.0 * (np.median(pr) / np.median(par) - 1.0))]
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)
    return 0 if all(r[-1] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
