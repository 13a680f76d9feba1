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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-pr", default=None)
    args = ap.parse_args()

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
