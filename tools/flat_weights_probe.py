#!/usr/bin/env python3
"""What per-point weights of the flat (diag / spherical) fit (hgmm_flat_set_weights) cost and buy -> profiles/flat_weights.md.

    python tools/flat_weights_probe.py [--out FILE] [--reps 5] [--skip-gpu] [--bench-parent FILE --bench-pr FILE]

Three things are recorded:
  * what they buy: bun000 (40 256 points) against its 4 mm voxel centroids (2 095), J = 16, 20 iterations -- the mean
    log-normaliser of the full scan under the full-scan fit, the unweighted centroid fit and the count-weighted centroid fit;
  * what they cost: the fused EM iteration with and without weights at N = 10^6, J = 800 and on bun000 at J = 100, the median
    of --reps timed fits of 20 iterations each (weights of one everywhere: the weighted kernel's own cost; the suites'
    standard weights, one in ten zero: with the rows it skips);
  * the resource table of the weighted instantiations beside the unweighted ones, read from the gfx950 code object, and the
    loop profile of the J = 800 kernel (tools/isa_count.py).
--bench-parent / --bench-pr: files of bench.py result lines (one JSON object per line) of the parent commit and of this
tree, taken in one session; their medians are written below the tables.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_count                                                     # noqa: E402
from source_weights_probe import LIB, code_object_notes              # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
KERNELS = re.compile(r"flat_fused_pk_kernel|flat_chunk_fused_kernel|flat_chunk_combine_kernel|flat_weighted_lpn_partials_kernel|"
                     r"flat_mstep_kernelILi3ELi1E")


def standard_weights(n, seed=11):
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.25, 4.0, n)
    w[rs.uniform(size=n) < 0.1] = 0.0
    return w.astype(np.float32)


def resource_table():
    notes = code_object_notes(LIB)
    names = [k for k in notes if KERNELS.search(k)]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = {}
    for k, d in zip(names, dem):
        rows[re.sub(r"\(.*", "", d).replace("hgmm::", "").replace("void ", "")] = notes[k]

    def key(s):
        return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)]
    lines = ["| kernel | VGPR + AGPR | SGPR | LDS B | scratch B | waves per SIMD |", "|---|---|---|---|---|---|"]
    for s in sorted(rows, key=key):
        n = rows[s]
        total, a = n.get("vgpr_count", 0), n.get("agpr_count", 0)        # (the note's vgpr_count is the unified total)
        waves = min(8, 512 // max(8, (total + 7) // 8 * 8))             # (512 registers per lane of a SIMD, allocated in eights)
        lines.append("| `%s` | %d + %d | %d | %d | %d | %d |" % (s, total - a, a, n.get("sgpr_count", 0), n.get("group_segment_fixed_size", 0),
                                                               n.get("private_segment_fixed_size", 0), waves))
    prof = []
    for k, instrs in sorted(isa_count.disassemble(LIB).items()):
        if "flat_fused_pk_kernelILi13E" in k:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_count.py"), k], capture_output=True, text=True).stdout
            loops = [l.strip() for l in out.split("\n") if "loop @instr" in l][:2]
            prof.append("`%s`:\n\n```\n%s\n```" % ("<13, true>" if "Lb1" in k else "<13, false>", "\n".join(loops)))
    return "\n".join(lines), "\n\n".join(prof)


def buys_section(ctx):
    from hgmm_amd.pointcloud_io import voxel_down_sample
    X = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
    cen, cnt = voxel_down_sample(X, 0.004, return_counts=True)
    cen = cen.astype(np.float32)
    J = 16
    mu0 = cen[np.random.RandomState(1).choice(len(cen), J, replace=False)]
    cov0, w0 = np.full((J, 3), 1e-4, np.float32), (np.ones(J) / J).astype(np.float32)
    fits = {}
    ctx.set_points(X)
    fits["full scan (%d points)" % len(X)] = ctx.flat_train(20, 0.0, mu0, cov0, w0, "diag", "W")
    ctx.set_points(cen)
    fits["centroids (%d), unweighted" % len(cen)] = ctx.flat_train(20, 0.0, mu0, cov0, w0, "diag", "W")
    ctx.flat_set_weights(cnt)
    fits["centroids, count-weighted"] = ctx.flat_train(20, 0.0, mu0, cov0, w0, "diag", "W")
    ctx.set_points(X)
    full = next(iter(fits.values()))
    lines = ["| fit | mean log-normaliser of the full scan under the model | max `pi` error vs full-scan fit | max `mu` error vs full-scan fit |",
             "|---|---|---|---|"]
    for name, m in fits.items():
        ll = ctx.flat_estep(m[0], m[1], m[2], "diag", "W", want_log_resp=False)[0]
        lines.append("| %s | %.4f | %s | %s |" % (name, ll, "--" if m is full else "%.2g" % np.abs(m[2] - full[2]).max(),
                                                 "--" if m is full else "%.2g mm" % (1e3 * np.abs(m[1] - full[1]).max())))
    return "\n".join(lines)


def cost_section(ctx, reps):
    import bench
    bunny = np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
    lines = ["| workload | unweighted | weights of one | standard weights (one in ten zero) |", "|---|---|---|---|"]
    for name, X, J in (("N = 10^6, J = 800", bench.synth_frame(0), 800), ("bun000 (40 256), J = 100", bunny, 100)):
        mu, w, cov = bench.init_params(X, J)
        ctx.set_points(X)
        cells = []
        for s in (None, np.ones(len(X), np.float32), standard_weights(len(X))):
            ctx.flat_set_weights(s)
            t = []
            for _ in range(reps + 3):
                ctx.flat_train_begin(0.0, mu, cov, w, "diag", "W", lls_capacity=20)
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.flat_train_step(20)
                ctx.synchronize()
                t.append((time.perf_counter() - t0) / 20)
                ctx.flat_train_end()
            t = np.array(t[3:]) * 1e3                                  # (the first three fits warm the clocks up)
            cells.append("%.4f ms (%.4f - %.4f)" % (np.median(t), t.min(), t.max()))
        lines.append("| %s | %s |" % (name, " | ".join(cells)))
    return "\n".join(lines)


def bench_section(parent_file, pr_file):
    def values(fn):
        return [json.loads(l)["value"] for l in open(fn) if l.strip().startswith("{")]
    p, r = values(parent_file), values(pr_file)
    mp, mr = float(np.median(p)), float(np.median(r))
    return ("| tree | runs (`value`, EM it/s) | median |\n|---|---|---|\n| parent | %s | %.1f |\n| this tree | %s | %.1f |\n\n"
            "This tree's median is %+.2f %% of the parent's." % (", ".join("%.1f" % v for v in p), mp,
                                                               ", ".join("%.1f" % v for v in r), mr, 100.0 * (mr / mp - 1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_weights.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-pr")
    a = ap.parse_args()
    parts = ["# What per-point weights of the flat fit cost and buy (`hgmm_flat_set_weights`)", "",
             "Written by `tools/flat_weights_probe.py`."]
    if not a.skip_gpu:
        import hgmm_amd
        ctx = hgmm_amd.Context(0)
        parts += ["", "## What they buy: bun000 against its 4 mm voxel centroids", "",
                  "J = 16 means drawn with `RandomState(1).choice` among the centroids, cov0 1e-4, w0 1/J, flavour W, diag, "
                  "20 iterations at tol 0, on the GPU.", "", buys_section(ctx)]
        parts += ["", "## What they cost: one fused EM iteration", "",
                  "Median (min - max) of %d timed fits of 20 iterations each, per iteration." % a.reps, "", cost_section(ctx, a.reps)]
        ctx.close()
    table, prof = resource_table()
    parts += ["", "## Resources of the weighted instantiations (gfx950 code object)", "", table, "",
              "Loop profile of the J = 800 kernel (row-maximum loop, constant-shift loop):", "", prof]
    if a.bench_parent and a.bench_pr:
        parts += ["", "## `bench.py --gpus 1 --steps 20 --warmup 5`, parent and this tree in one session", "",
                  bench_section(a.bench_parent, a.bench_pr)]
    with open(a.out, "w") as f:
        f.write("\n".join(parts) + "\n")
    print("\n".join(parts))


if __name__ == "__main__":
    main()
