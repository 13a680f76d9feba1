#!/usr/bin/env python3
"""Wall time per frame of the count-weighted batched flat fit (hgmm_flat_train_batch_voxels, hgmm_flat_train_batch_weighted)
next to the same frames down-sampled, downloaded and fitted one by one:

    python tools/flat_batch_weights_probe.py                      this tree: every figure
    python tools/flat_batch_weights_probe.py --lib PATH           the frame-by-frame figure through another build (the parent's)

The workload: the project's bun000 scan (tests/golden/bun000_xyz.npy, shifted by a millimetre per frame so that the members
differ) voxel-down-sampled at 4 mm, J = 100, 20 iterations, tol = 0, one context, B = 1, 8, 32, 64 frames.  Per B, the median
of --reps warmed-up calls, per frame:
  voxel_ms      voxel_down_sample_batch(download=False) + flat_train_batch_voxels: the down-sample included, no host trip
  host_ms       flat_train_batch(handles of the centroids, weights=counts): the host-array entry on resident handles
                (the down-sample is not in this figure)
  serial_ms     voxel_down_sample_batch with download, then set_points, flat_set_weights and flat_train per frame: what a
                count-weighted frame cost before the batched entries
  serial_fit_ms the same without the down-sample, for comparison with host_ms
and, with the in-library profiler on, the fused launches alone (HGMM_K_FLAT_FUSED) of the weighted batch against the
unweighted batch over the same handles.

--lib PATH: the library to load.  The Python package that is imported is the one of the checkout the library lies in
(<root>/<package>/libhgmm_hip.so -> <root>), so that a parent checkout is measured through its own binding; a build without
the weighted entries reports serial_ms and serial_fit_ms only.  One JSON line per B.  Alternate the two builds, a fresh
process each."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="the libhgmm_hip.so to load (default: this tree's)")
ap.add_argument("--B", default="1,8,32,64")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--voxel", type=float, default=0.004)
args = ap.parse_args()
root = os.path.dirname(HERE)
if args.lib:
    lib_root = os.path.dirname(os.path.dirname(os.path.abspath(args.lib)))
    if os.path.exists(os.path.join(lib_root, "hgmm_amd", "__init__.py")):
        root = lib_root
sys.path.insert(0, root)
import hgmm_amd                                   # noqa: E402
from hgmm_amd import _native                      # noqa: E402
from oracle import flat_em                        # noqa: E402

if args.lib:
    _native.load_library(os.path.abspath(args.lib))
ctx = hgmm_amd.Context(0)
have = hasattr(ctx, "flat_train_batch_voxels")
ITERS, J = 20, 100
base = np.load(os.path.join(HERE, "..", "tests", "golden", "bun000_xyz.npy")).astype(np.float64)
cent0 = ctx.voxel_down_sample(base, args.voxel)[0]
mu0, w0, cov0 = flat_em.seeded_init(cent0.astype(np.float32), J, 1)


def median_ms(fn, reps):
    fn()
    fn()                                          # warm: buffers grown, code objects loaded
    t = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def fused_ms(fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    fn()
    ms, n = ctx.profile_get("flat_fused")
    ctx.profile_enable(False)
    return ms, n


for B in [int(b) for b in args.B.split(",")]:
    frames = [base + 0.001 * k for k in range(B)]
    mus = [mu0 + np.float32(0.001 * k) for k in range(B)]
    down = ctx.voxel_down_sample_batch(frames, args.voxel)
    cents = [c.astype(np.float32) for c, _ in down]
    counts = [n.astype(np.float32) for _, n in down]

    def serial_fit(cc=cents, nn=counts):
        for X, s, m in zip(cc, nn, mus):
            ctx.set_points(X)
            ctx.flat_set_weights(s)
            ctx.flat_train(ITERS, 0.0, m, cov0, w0, "diag", "W")

    def serial():
        out = ctx.voxel_down_sample_batch(frames, args.voxel)
        serial_fit([c for c, _ in out], [n for _, n in out])

    out = {"lib": os.path.abspath(args.lib) if args.lib else "this tree", "N": int(len(base)), "voxel": args.voxel,
           "M": int(np.mean([len(c) for c in cents])), "J": J, "B": B, "iters": ITERS}
    out.update(serial_ms=round(median_ms(serial, args.reps) / B, 4), serial_fit_ms=round(median_ms(serial_fit, args.reps) / B, 4))
    if have:
        handles = [ctx.points_create(X) for X in cents]

        def voxel():
            res = ctx.voxel_down_sample_batch(frames, args.voxel, download=False)
            ctx.flat_train_batch_voxels(res.members(), ITERS, 0.0, mus, [cov0] * B, [w0] * B, "diag", "W")

        def host():
            ctx.flat_train_batch(handles, ITERS, 0.0, mus, [cov0] * B, [w0] * B, "diag", "W", weights=counts)

        def unweighted():
            ctx.flat_train_batch(handles, ITERS, 0.0, mus, [cov0] * B, [w0] * B, "diag", "W")

        v, h = median_ms(voxel, args.reps) / B, median_ms(host, args.reps) / B
        fw_ms, fw_n = fused_ms(host)
        fu_ms, fu_n = fused_ms(unweighted)
        out.update(voxel_ms=round(v, 4), host_ms=round(h, 4), unweighted_batch_ms=round(median_ms(unweighted, args.reps) / B, 4),
                   fused_weighted_ms_per_launch=round(fw_ms / max(fw_n, 1), 5), fused_unweighted_ms_per_launch=round(fu_ms / max(fu_n, 1), 5),
                   fused_launches=[fw_n, fu_n], speedup_voxel=round(out["serial_ms"] / v, 3),
                   speedup_host=round(out["serial_fit_ms"] / h, 3))
        for hd in handles:
            ctx.points_destroy(hd)
    print(json.dumps(out), flush=True)
ctx.close()
