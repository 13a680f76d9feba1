#!/usr/bin/env python3
"""Wall time per frame of the batched flat full-covariance fit (hgmm_fullcov_fit_batch / fitFullCovGMM_batch) next to the same
frames fitted one by one on the same context:

    python tools/fullcov_batch_probe.py                   this tree: batched and serial figures, voxel-sized clouds and bun000
    python tools/fullcov_batch_probe.py --big             N = 1e6, J = 800, B = 2 against two serial fits
    python tools/fullcov_batch_probe.py --lib PATH        another checkout's library and package (the parent's: serial figures)

Frames: the project's bun000 scan (tests/golden/bun000_xyz.npy) shifted by a millimetre per frame, so that the members
differ; the voxel-sized clouds are its 4 mm voxel centroids (2095 points).  20 iterations (ls = 1e-30: no member stops
early), initial means = J distinct rows drawn once.  One context, warmed-up calls, the median of --reps calls.
  host     the Python calls a user makes from host arrays: set_points_batch + fullcov_fit_batch against the loop of
           set_points + fullcov_fit -- upload and download included on both sides
  resident the library call alone on a cloud that is resident already (fullcov_fit_batch; serial: fullcov_fit per frame with
           the frame's upload outside the clock)
  voxel    fitFullCovGMM_batch(VoxelClouds) against the loop of fitFullCovGMM(VoxelCloud) on a resident voxel result
           (count-weighted, hand-over on the device included, down-sampling outside the clock)
One JSON line per row."""
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
ap.add_argument("--J", default="16,100")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--big", action="store_true")
args = ap.parse_args()
root = os.path.dirname(HERE)
if args.lib:                                      # the package of the checkout the library lies in: a parent through its own binding
    lib_root = os.path.dirname(os.path.dirname(os.path.abspath(args.lib)))
    if os.path.exists(os.path.join(lib_root, "hgmm_amd", "__init__.py")):
        root = lib_root
sys.path.insert(0, root)
import hgmm_amd                                   # noqa: E402
from hgmm_amd import _native                      # noqa: E402
from hgmm_amd.hgmm.hgmm_gpu import fitFullCovGMM  # noqa: E402

if args.lib:
    _native.load_library(os.path.abspath(args.lib))
ctx = hgmm_amd.Context(0)
have_batch = hasattr(ctx, "fullcov_fit_batch")
if have_batch:
    from hgmm_amd.hgmm.hgmm_gpu import fitFullCovGMM_batch  # noqa: E402
LS, LD, SIG2 = 1e-30, 1e-4, 0.0005


def median_ms(fn, reps):
    fn()
    fn()                                          # warm: buffers grown, code objects loaded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def row(**kw):
    print(json.dumps(kw), flush=True)


def sweep(name, cloud, Bs, Js, iters):
    n = len(cloud)
    for J in Js:
        idx = np.random.RandomState(J).choice(n, J, replace=False)
        for B in Bs:
            frames = [cloud + 0.001 * b for b in range(B)]
            init = np.stack([f[idx] for f in frames])

            def serial_host():
                for f in frames:
                    ctx.set_points(f)
                    ctx.fullcov_fit(J, LS, LD, f[idx], SIG2, iters)

            def serial_resident():                 # the fit alone: one frame resident, B calls
                for _ in frames:
                    ctx.fullcov_fit(J, LS, LD, init[0], SIG2, iters)

            s_host = median_ms(serial_host, args.reps)
            ctx.set_points(frames[0])
            s_res = median_ms(serial_resident, args.reps)
            out = dict(case=name, N=n, J=J, B=B, iters=iters, serial_host_ms_per_frame=s_host[0] / B,
                       serial_resident_ms_per_frame=s_res[0] / B, serial_host_min_max=[s_host[1] / B, s_host[2] / B])
            if have_batch:
                counts = [n] * B

                def batch_host():
                    ctx.set_points_batch(frames)
                    ctx.fullcov_fit_batch(counts, J, LS, LD, init_mu=init, sig2=SIG2, max_iters=iters)

                def batch_resident():
                    ctx.fullcov_fit_batch(counts, J, LS, LD, init_mu=init, sig2=SIG2, max_iters=iters, want_labels=False)

                b_host = median_ms(batch_host, args.reps)
                ctx.set_points_batch(frames)
                b_res = median_ms(batch_resident, args.reps)
                out.update(batch_host_ms_per_frame=b_host[0] / B, batch_resident_ms_per_frame=b_res[0] / B,
                           batch_host_min_max=[b_host[1] / B, b_host[2] / B],
                           host_speedup=s_host[0] / b_host[0], resident_speedup=s_res[0] / b_res[0])
            row(**out)


def voxel_sweep(scan, Bs, Js, iters):
    for J in Js:
        for B in Bs:
            vcs = ctx.voxel_down_sample_batch([scan + 0.001 * b for b in range(B)], 0.004, download=False).members()
            m = min(len(vc) for vc in vcs)
            idx = np.random.RandomState(J).choice(m, J, replace=False)
            kw = dict(ls=LS, ld=LD, sig2=SIG2, init_idx=idx, max_iters=iters, ctx=ctx)

            def serial():
                for vc in vcs:
                    fitFullCovGMM(vc, J, **kw)

            s = median_ms(serial, args.reps)
            out = dict(case="voxel entry (4 mm)", N=m, J=J, B=B, iters=iters, serial_ms_per_frame=s[0] / B)
            if have_batch:
                b = median_ms(lambda: fitFullCovGMM_batch(vcs, J, **kw), args.reps)
                out.update(batch_ms_per_frame=b[0] / B, speedup=s[0] / b[0])
            row(**out)


bunny = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "bun000_xyz.npy")).astype(np.float64)
Bs = [int(v) for v in args.B.split(",")]
Js = [int(v) for v in args.J.split(",")]
row(lib=os.path.abspath(args.lib) if args.lib else "this tree", have_batch=have_batch)
if args.big:
    big = np.random.RandomState(0).rand(1000000, 3)
    sweep("uniform cube", big, [2], [800], args.iters)
else:
    cent, _ = ctx.voxel_down_sample(bunny, 0.004)
    sweep("bun000 4 mm voxel centroids", np.ascontiguousarray(cent), Bs, Js, args.iters)
    if hasattr(ctx, "voxel_down_sample_batch"):
        voxel_sweep(bunny, Bs, Js, args.iters)
    sweep("bun000", bunny, [b for b in Bs if b <= 8], [100], args.iters)
ctx.close()
