#!/usr/bin/env python3
"""Wall time per frame of the batched KMeans initialiser (hgmm_kmeans_fit_batch / KMeans.fit_batch) next to the same frames
fitted one by one:

    python tools/kmeans_batch_probe.py                    this tree: batched and serial figures, bun000 sweep
    python tools/kmeans_batch_probe.py --consumer         the G flavour's fit_batch of 32 frames against the loop of fit
    python tools/kmeans_batch_probe.py --big              N = 1e6, k = 800, B = 2 against two serial fits
    python tools/kmeans_batch_probe.py --lib PATH         another checkout's library and package (the parent's: serial figures)

Frames: the project's bun000 scan (tests/golden/bun000_xyz.npy) shifted by a millimetre per frame, so that the members
differ; KMeans(100, random_state=1, max_iter=50), the reference's initialiser.  One context, warmed-up calls, the median of
--reps calls.  The times are those of the Python calls a user makes -- centring, upload and download included on both sides.
The seeding / Lloyd split: the batch with max_iter = 0 (copy launch, seeding, one assignment) against the whole call; the
serial side's is ``seeding_ms_`` (the k-means++ call) against the whole ``fit``.  ``resident_*``: the library call alone on a
batch cloud that is resident already (``Context.kmeans_fit_batch``: no centring, no upload of the clouds), whole and with
max_iter = 0, against the serial ``kmeans_plusplus`` and ``kmeans_lloyd`` calls on a resident cloud.  One JSON line per row."""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="the libhgmm_hip.so to load (default: this tree's)")
ap.add_argument("--B", default="1,8,32,64")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--big", action="store_true")
ap.add_argument("--consumer", action="store_true")
args = ap.parse_args()
root = os.path.dirname(HERE)
if args.lib:                                      # the package of the checkout the library lies in: a parent through its own binding
    lib_root = os.path.dirname(os.path.dirname(os.path.abspath(args.lib)))
    if os.path.exists(os.path.join(lib_root, "hgmm_amd", "__init__.py")):
        root = lib_root
sys.path.insert(0, root)
import hgmm_amd                                   # noqa: E402
from hgmm_amd import _native                      # noqa: E402
from hgmm_amd.kmeans import KMeans                # noqa: E402

if args.lib:
    _native.load_library(os.path.abspath(args.lib))
ctx = hgmm_amd.Context(0)
have_batch = hasattr(ctx, "kmeans_fit_batch")


def median_ms(fn, reps):
    fn()
    fn()                                          # warm: buffers grown, code objects loaded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def frames_of(base, B):
    return [base + 1e-3 * b for b in range(B)]


if args.consumer:
    from hgmm_amd import use_context
    from hgmm_amd.gmmreg_gpu.gmm import GMM_GPU_Base
    base = np.load(os.path.join(HERE, "..", "tests", "golden", "bun000_xyz.npy")).astype(np.float64)
    fr = frames_of(base, 32)
    quiet = io.StringIO()
    with use_context(ctx), redirect_stdout(quiet):
        loop = median_ms(lambda: [GMM_GPU_Base(100, max_iter=10).fit(X) for X in fr], args.reps)
        row = {"what": "G flavour, 32 bun000 frames, k = 100, 10 EM iterations", "loop_ms_per_frame": [v / 32 for v in loop]}
        if have_batch:
            row["fit_batch_ms_per_frame"] = [v / 32 for v in median_ms(lambda: GMM_GPU_Base(100, max_iter=10).fit_batch(fr), args.reps)]
    print(json.dumps(row))
    sys.exit(0)

if args.big:
    rs = np.random.RandomState(0)
    base, k, Bs, max_iter = rs.rand(1000000, 3), 800, [2], 10
else:
    base = np.load(os.path.join(HERE, "..", "tests", "golden", "bun000_xyz.npy")).astype(np.float64)
    k, Bs, max_iter = 100, [int(b) for b in args.B.split(",")], 50

for B in Bs:
    fr = frames_of(base, B)
    seed_ms = []

    def loop():
        seed_ms.clear()
        for X in fr:
            seed_ms.append(KMeans(k, random_state=1, max_iter=max_iter, ctx=ctx).fit(X).seeding_ms_)

    serial = median_ms(loop, args.reps)
    row = {"N": len(base), "k": k, "B": B, "max_iter": max_iter, "loop_of_fit_ms_per_frame": [v / B for v in serial],
           "loop_seeding_ms_per_frame": float(np.mean(seed_ms))}
    if have_batch:
        whole = median_ms(lambda: KMeans(k, random_state=1, max_iter=max_iter, ctx=ctx).fit_batch(fr), args.reps)
        seeding = median_ms(lambda: KMeans(k, random_state=1, max_iter=0, ctx=ctx).fit_batch(fr), args.reps)
        row["fit_batch_ms_per_frame"] = [v / B for v in whole]
        row["fit_batch_max_iter0_ms_per_frame"] = [v / B for v in seeding]
        from hgmm_amd.kmeans import column_mean_var
        cen = [column_mean_var(X) for X in fr]
        tols = [float(np.mean(v) * 1e-4) for _, v, _ in cen]
        rs = np.random.RandomState(1)
        first, rand = [int(rs.randint(len(base))) for _ in fr], rs.uniform(size=(B, k - 1, 2 + int(np.log(k))))
        counts = [len(X) for X in fr]
        ctx.set_points_batch([c[2] for c in cen])
        row["resident_batch_ms_per_frame"] = [v / B for v in median_ms(
            lambda: ctx.kmeans_fit_batch(counts, k, max_iter, tols, first_ids=first, rand_vals=rand), args.reps)]
        row["resident_batch_max_iter0_ms_per_frame"] = [v / B for v in median_ms(
            lambda: ctx.kmeans_fit_batch(counts, k, 0, tols, first_ids=first, rand_vals=rand), args.reps)]
        ctx.set_points(cen[0][2])
        row["resident_serial_plusplus_ms"] = list(median_ms(lambda: ctx.kmeans_plusplus(k, first[0], rand[0]), args.reps))
        seeds = ctx.kmeans_plusplus(k, first[0], rand[0])[1]
        row["resident_serial_lloyd_ms"] = list(median_ms(lambda: ctx.kmeans_lloyd(seeds, max_iter, tols[0]), args.reps))
        n_iter = [f.n_iter_ for f in KMeans(k, random_state=1, max_iter=max_iter, ctx=ctx).fit_batch(fr)]
        row["n_iter"] = [int(min(n_iter)), int(max(n_iter))]
    print(json.dumps(row), flush=True)
ctx.close()
