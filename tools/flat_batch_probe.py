#!/usr/bin/env python3
"""Wall time per frame of the batched flat fit (hgmm_flat_train_batch) next to the same frames fitted one by one:

    python tools/flat_batch_probe.py                      this tree: batched and serial figures
    python tools/flat_batch_probe.py --lib PATH           the serial figures through another build (the parent's)

Small frames: the project's bun000 scan (tests/golden/bun000_xyz.npy), J = 100, 20 iterations, tol = 0, for B = 1, 2, 4, 8,
16, 32, 64 frames (the scan shifted by a millimetre per frame, so that the members differ).  The other end: N = 10^6,
J = 800, B = 2 (--big), where one fit fills the chip already and no gain is expected.  One context, warmed-up calls, the
median of --reps calls; the serial side is B `flat_train` calls on bound handles.  A third pass with the in-library profiler
on gives the time of the fused launches alone (HGMM_K_FLAT_FUSED: B x 20 launches of one frame, or 20 launches of B frames).

--lib PATH: the library to load.  The Python package that is imported is the one of the checkout the library lies in
(<root>/<package>/libhgmm_hip.so -> <root>), so that a parent checkout is measured through its own binding; a build without
the batched entry reports the serial figures only.  One JSON line per B.  Alternate the two builds, a fresh process each."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="the libhgmm_hip.so to load (default: this tree's)")
ap.add_argument("--B", default="1,2,4,8,16,32,64")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--big", action="store_true", help="N = 1e6, J = 800, B = 2 instead of the bun000 sweep")
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
have_batch = hasattr(ctx, "flat_train_batch")
ITERS = 20

if args.big:
    rs = np.random.RandomState(0)
    base = rs.rand(1000000, 3).astype(np.float32)
    J, Bs = 800, [2]
else:
    base = np.load(os.path.join(HERE, "..", "tests", "golden", "bun000_xyz.npy")).astype(np.float32)
    J, Bs = 100, [int(b) for b in args.B.split(",")]
mu0, w0, cov0 = flat_em.seeded_init(base, J, 1)


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


for B in Bs:
    frames = [base + np.float32(0.001 * k) for k in range(B)]
    handles = [ctx.points_create(X) for X in frames]
    mus = [mu0 + np.float32(0.001 * k) for k in range(B)]

    def serial():
        for h, m in zip(handles, mus):
            ctx.points_bind(h)
            ctx.flat_train(ITERS, 0.0, m, cov0, w0, "diag", "W")

    def batched():
        ctx.flat_train_batch(handles, ITERS, 0.0, mus, [cov0] * B, [w0] * B, "diag", "W")

    out = {"lib": os.path.abspath(args.lib) if args.lib else "this tree", "N": int(len(base)), "J": J, "B": B, "iters": ITERS}
    ms = median_ms(serial, args.reps)
    f_ms, f_n = fused_ms(serial)
    out.update(serial_ms_per_frame=round(ms / B, 4), serial_fused_ms_per_frame=round(f_ms / B, 4), serial_fused_launches=f_n)
    if have_batch:
        ms = median_ms(batched, args.reps)
        f_ms, f_n = fused_ms(batched)
        out.update(batch_ms_per_frame=round(ms / B, 4), batch_fused_ms_per_frame=round(f_ms / B, 4), batch_fused_launches=f_n,
                   speedup=round(out["serial_ms_per_frame"] / (ms / B), 3))
    print(json.dumps(out), flush=True)
    for h in handles:
        ctx.points_destroy(h)
ctx.close()
