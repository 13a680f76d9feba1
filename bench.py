#!/usr/bin/env python3
"""Headline benchmark of the EM hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

N = 1 runs in this process.  N > 1 needs one process per GPU: either the caller provides them
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P
bench.py --gpus N ...` -- only RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* are read, PyTorch is not imported),
or, when WORLD_SIZE is not set, this script launches the N ranks itself.  The ranks meet over a plain TCP
exchange of the 128-byte RCCL unique id; everything after that is RCCL over xGMI inside the library.

Workload (BASELINE.json configs[2] / configs[4]): per GPU one synthetic frame of
N = 1,000,000 uniform [0,1)^3 points (seed = rank), flat diag GMM with J = 800 components (flavour "W" =
src/python/gmm_waymo/src/gmm_impl.py), float32.  One *step* = one full EM iteration (E-step responsibilities
for all N x J pairs + M-step update of all parameters), device-resident, inputs already in HBM.  With N > 1
the frames are shards of ONE joint fit: every iteration all-reduces the (7 J + 2) float64 sufficient
statistics over RCCL before the (redundant, identical) M-step -- weak scaling, `value` = frames x iterations
/ second.

Timing: a fixed internal clock warm-up (CLOCK_WARMUP_STEPS fused iterations on a scratch fit), W untimed
warm-up steps, then ONE block of exactly K timed steps, bracketed by a barrier + stream synchronisation on
both sides and reduced with MAX over the ranks; `ms_per_step` = block / K.  `--min-time S` repeats K-step
blocks until at least S seconds of timed work (and three blocks) have accumulated and reports the MEDIAN
block, the first (un-settled) block and the spread next to it.

--dump-outputs DIR: after the timed steps, what the timed path returns to its caller after its last step --
the fitted model (mu, cov, w, inv_std) and the log-likelihood of every iteration of the timed fit -- as
DIR/<name>.npy (float32 / float64).  The inputs are fixed by the seeds, so two builds can be compared output
for output.

A plain run prints the headline alone.  --full adds (behind the same headline)
  fused_kernel / roofline_fused / allreduce_us   one more K-step block under the hipEvent profiler -- a fit of its
                  own from the initial parameters; the legs below get the model of the timed steps (W + K x blocks
                  iterations; up to round 6 the profiled block continued the timed fit, one block more)
  roofline        the materialising E-step kernel (the API's e_step(): writes log_resp[N,J]): HBM bound,
                  achieved = algorithmic bytes (12N + 4NJ + 4N + 28J) / mean hipEvent time
  roofline_fused  the kernel the timed step spends its time in (VALU bound): fp32 FLOP/s against the vector
                  peak and VALU instructions per cycle per SIMD, instruction counts read from the code object
  fullcov / tree_1M / hgmm / kmeans_init / registration / bunny    the other hot kernels at their configs
  cpu_baseline    the NumPy oracle (same op sequence as the reference's CPU path) on this box's host cores
  N > 1           the sharded HGMM build and the same joint fit over the one-shot peer exchange (`peer_exchange`)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_POINTS = 1_000_000
J_COMP = 800
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
FP32_VECTOR_PEAK_TF = 157.3  # MI355X_MICROARCH.md: peak FP32 vector (spec)
FP64_VECTOR_PEAK_TF = 78.6   # half the fp32 rate (valubench: v_fma_f64 issues at the v_pk_fma_f32 rate)
SPEC_CLOCK_HZ = 2.4e9
MAX_BLOCKS = 400             # --min-time: at most this many timed blocks
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: at most this much in all
CLOCK_WARMUP_STEPS = int(os.environ.get("HGMM_BENCH_CLOCK_WARMUP", "250"))   # untimed fused iterations before the W + K x blocks
RCCL_INIT_FAILED = 17        # exit code of a rank whose RCCL communicator could not be created

# fused EM kernel, fp32 flops per (point, component) pair (fma = 2), DESIGN.md section 3:
#   E: 3 sub + 3 mul (squares) + 3 fma = 12, exp 1, row sum 1;  M: r = e/S 1, s0 1, first moments 3 fma, second moments 3 fma
#   = 14  -> 28.  (Round 4's formulation executes exactly these; rounds 2-3 spent 3 mul + 3 add + 3 fma on the moments --
#   the same 28 -- plus 3 re-computed subtractions.)
FUSED_FLOP_PER_PAIR = 28
FUSED_RECOMPUTED_FLOP_PER_PAIR = 0


def synth_frame(seed, n=None):
    return np.random.RandomState(seed).rand(n or N_POINTS, 3).astype(np.float32)


def init_params(frame0, J=None, seed=100):
    J = J or J_COMP
    idx = np.random.RandomState(seed).choice(len(frame0), J, replace=False)
    mu = frame0[idx].copy()
    w = (np.ones(J) / J).astype(np.float32)
    cov = (0.1 * np.ones((J, 3))).astype(np.float32)
    return mu, w, cov


# ------------------------------------------------------------------------------------------------
# launcher: N ranks of this script on the N GPUs of this node (used when WORLD_SIZE is not set)
# ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n, argv, script=None, extra_env=None, timeout=None):
    """Start `n` ranks (RANK = LOCAL_RANK = 0..n-1, WORLD_SIZE = n, MASTER_ADDR = 127.0.0.1) of `script`
    and wait for them.  Rank 0 inherits stdout (it prints the JSON line), the other ranks' stdout goes to
    stderr.  Returns the first non-zero exit code, or 0."""
    script = script or os.path.abspath(__file__)
    timeout = timeout or float(os.environ.get("HGMM_BENCH_LAUNCH_TIMEOUT", "1500"))
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, script] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr))
    deadline = time.time() + timeout
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is not None:
                alive.remove(p)
                if code != 0 and rc == 0:
                    rc = code
        if rc != 0 or time.time() > deadline:
            # one rank failed (or the group hangs): the others would wait in a collective for ever
            grace = time.time() + (20 if rc != 0 else 0)
            while alive and time.time() < grace:
                alive = [p for p in alive if p.poll() is None]
                time.sleep(0.1)
            for p in alive:
                p.kill()
            for p in alive:
                p.wait()
            if rc == 0:
                rc = 124
            break
        time.sleep(0.05)
    return rc


def self_launch(args, argv):
    # (a backend that cannot be set up on every rank is replaced IN PLACE by the next one, collectively -- rank_main /
    #  choose_collective; rounds 1-3 restarted the ranks instead, which an external launcher cannot do)
    return launch_ranks(args.gpus, argv, extra_env={"HGMM_BENCH_LAUNCHER": "self"})


# ------------------------------------------------------------------------------------------------
# legs that run on rank 0 at N = 1
# ------------------------------------------------------------------------------------------------
def cpu_baseline_main(sample_n=200_000, sample_iters=5, full_iters=3):
    """NumPy oracle (fp32, reference op sequence) on this box's host cores: the FULL 1M x 800 frame, `full_iters`
    iterations in one piece like the reference (train_gmm materialises its N x J temporaries, ~20 GB at this size) --
    when the host has the memory; beside it (and instead of it on a small host) a 200 k-point sample scaled linearly."""
    from oracle import flat_em
    frame = synth_frame(0)
    mu, w, cov = init_params(frame)
    flat_em.train(frame[:2000], 1, 0.0, mu, cov, w, "diag", "W")          # warm BLAS / pages
    X = frame[:sample_n]
    t0 = time.perf_counter()
    flat_em.train(X, sample_iters, 0.0, mu, cov, w, "diag", "W")
    dt_s = time.perf_counter() - t0
    it_per_s_sample = sample_iters / dt_s
    blas_threads = None
    try:                                   # threads the GEMMs actually ran on (elementwise passes are 1 thread)
        from threadpoolctl import threadpool_info
        pools = [p for p in threadpool_info() if p.get("user_api") == "blas"] or threadpool_info()
        blas_threads = max([p.get("num_threads", 1) for p in pools] or [1])
    except Exception:
        pass
    extrapolated = it_per_s_sample * sample_n / N_POINTS
    out = {
        "unit": "EM it/s per 1M-pt x 800-comp frame",
        "cores": blas_threads or os.cpu_count(),
        "host_cpu_count": os.cpu_count(),
        "kind": "port",
        "extrapolated_from_sample": {"value": extrapolated, "it_per_s_on_sample": it_per_s_sample,
                                     "sample": "N=%d of the frame, %d iterations, %.1f s; scaled linearly in N"
                                               % (sample_n, sample_iters, dt_s)},
    }
    avail_gb = None
    try:
        import psutil
        avail_gb = psutil.virtual_memory().available / 2 ** 30
    except Exception:
        pass
    need_gb = 10 * 4.0 * len(frame) * J_COMP / 2 ** 30              # ~10 live N x J float32 temporaries at the peak
    # (the budget: a few iterations of (sample time per iteration x N / sample_n) must stay within ~40 s)
    est_full_s = full_iters * dt_s / sample_iters * len(frame) / sample_n
    if avail_gb is not None and avail_gb > need_gb + 8 and est_full_s < 60 and not os.environ.get("HGMM_BENCH_CPU_SAMPLE_ONLY"):
        t0 = time.perf_counter()
        flat_em.train(frame, full_iters, 0.0, mu, cov, w, "diag", "W")
        dt = time.perf_counter() - t0
        out["value"] = full_iters / dt
        out["sample"] = ("oracle/flat_em.train (NumPy fp32, same op sequence as reference train_gmm) on the WHOLE 1M-point "
                         "frame, J=800, %d iterations in one piece, %.1f s" % (full_iters, dt))
    else:
        out["value"] = extrapolated
        out["unit"] += " (extrapolated linearly in N from the sample)"
        out["sample"] = ("oracle/flat_em.train (NumPy fp32, same op sequence as reference train_gmm), N=%d of the 1M-point "
                         "frame, J=800, %d iterations, %.1f s -- the whole frame was not timed: %s"
                         % (sample_n, sample_iters, dt_s,
                            "host memory %.0f GB available, ~%.0f GB needed" % (avail_gb or -1, need_gb + 8)
                            if not (avail_gb is not None and avail_gb > need_gb + 8) else
                            "estimated %.0f s exceed the bench's CPU budget" % est_full_s))
    return out


def bunny_leg(ctx):
    """BASELINE configs[0]: bun000.ply, J = 100, 20 iterations, tol = 0: GPU vs CPU oracle."""
    from oracle import flat_em
    path = os.path.join(ROOT, "tests", "golden", "bun000_xyz.npy")
    if not os.path.exists(path):
        return None
    X = np.load(path)
    mu, w, cov = flat_em.seeded_init(X, 100, 0)
    ctx.set_points(X)
    ctx.flat_train(20, 0.0, mu, cov, w, "diag", "W")                   # warm-up
    gpu = []
    for _ in range(5):
        t0 = time.perf_counter()
        ctx.flat_train(20, 0.0, mu, cov, w, "diag", "W")
        gpu.append(20 / (time.perf_counter() - t0))
    flat_em.train(X, 2, 0.0, mu, cov, w, "diag", "W")
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        flat_em.train(X, 20, 0.0, mu, cov, w, "diag", "W")
        cpu.append(20 / (time.perf_counter() - t0))
    g, c = float(np.median(gpu)), float(np.median(cpu))
    return {"workload": "bun000.ply N=40256 J=100 diag, 20 iterations tol=0 (incl. H2D params + D2H results)",
            "gpu_it_per_s": g, "cpu_it_per_s": c, "cpu_cores": os.cpu_count(), "speedup": g / c}


def registration_leg(ctx):
    """End to end through the drop-in API (hgmm_gpu.py:802-807): GMM tree (L = 3, 584 nodes) on the
    full bun000 scan, then GMMTree.registration of a copy rotated 10 deg about z and shifted by a
    few millimetres (20 iterations max, tol 1e-4); the reference's CPU twin needs minutes for this."""
    path = os.path.join(ROOT, "tests", "golden", "bun000_xyz.npy")
    if not os.path.exists(path):
        return None
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    P = np.load(path).astype(np.float64)
    th = np.deg2rad(10.0)
    rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    target = P @ rz.T + np.array([0.005, -0.003, 0.002])
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        gt = GMMTree(P, tree_level=3, lambda_c=0.01, ls=80, sig2=0.00034, ctx=ctx)
        t1 = time.perf_counter()
        res = gt.registration(target, maxiter=20, tol=1e-4)          # no callbacks: the loop runs inside the library
        t2 = time.perf_counter()
        if best is None or t2 - t0 < best[0]:
            err = float(np.linalg.norm(res.transformation.transform(P) - target, axis=1).mean())
            best = (t2 - t0, t1 - t0, t2 - t1, int(gt.n_iter_), err)
    # the same registration with a callback per iteration (the reference's visualisation hook): Python per iteration
    seen = []
    gt.set_callbacks([lambda tf: seen.append(1)])
    t0 = time.perf_counter()
    gt.registration(target, maxiter=20, tol=1e-4)
    with_cb = time.perf_counter() - t0
    return {"workload": "bun000.ply (40256 pts) vs copy rotated 10 deg + shifted, registration_gmmtree L=3",
            "total_ms": best[0] * 1e3, "build_ms": best[1] * 1e3, "registration_ms": best[2] * 1e3,
            "registration_iterations": best[3], "ms_per_registration_iteration": best[2] * 1e3 / max(best[3], 1),
            "registration_ms_with_per_iteration_callbacks": with_cb * 1e3, "callback_iterations": len(seen),
            "mean_residual_m": best[4]}


def kmeans_leg(ctx):
    """KMeans initialiser of the GMMReg flavour (gmmreg_gpu/gmm_impl.py:18-24) at C3 size on the
    device, and on bun000 (k = 100) next to scikit-learn (the reference's own call) when installed."""
    from hgmm_amd.kmeans import KMeans
    X = synth_frame(0).astype(np.float64)
    KMeans(n_clusters=J_COMP, random_state=1, max_iter=2, ctx=ctx).fit(X[:20000])      # warm-up
    t0 = time.perf_counter()
    km = KMeans(n_clusters=J_COMP, random_state=1, max_iter=50, ctx=ctx).fit(X)
    out = {"workload": "KMeans(k=800, random_state=1, max_iter=50, n_init=1) on the C3 frame, float64",
           "fit_ms": (time.perf_counter() - t0) * 1e3, "lloyd_iterations": int(km.n_iter_),
           "seeding_ms": getattr(km, "seeding_ms_", None),
           "fit_ms_note": "first call on this context: includes the device buffers' allocation",
           "sklearn_k800_1M": {"ms": 78395, "source": "profiles/r01/kmbench.log (round-1 box, NOT re-timed in this "
                                                      "run: 78 s of host time; k = 100 on bun000 is re-timed below)"}}
    t0 = time.perf_counter()
    km = KMeans(n_clusters=J_COMP, random_state=1, max_iter=50, ctx=ctx).fit(X)
    out["fit_ms_warm"] = (time.perf_counter() - t0) * 1e3
    out["seeding_ms_warm"] = getattr(km, "seeding_ms_", None)
    path = os.path.join(ROOT, "tests", "golden", "bun000_xyz.npy")
    if os.path.exists(path):
        P = np.load(path).astype(np.float64)
        KMeans(n_clusters=100, random_state=1, max_iter=50, ctx=ctx).fit(P)
        t0 = time.perf_counter()
        km = KMeans(n_clusters=100, random_state=1, max_iter=50, ctx=ctx).fit(P)
        out["bun000_k100_fit_ms"] = (time.perf_counter() - t0) * 1e3
        try:
            from sklearn.cluster import KMeans as SK
            t0 = time.perf_counter()
            ref = SK(n_clusters=100, random_state=1, max_iter=50, n_init=1).fit(P)
            out["bun000_k100_sklearn_ms"] = (time.perf_counter() - t0) * 1e3
            out["bun000_k100_labels_identical"] = bool(np.array_equal(ref.labels_, km.labels_))
        except ImportError:
            pass
    return out


def hgmm_leg(ctx):
    """BASELINE configs[3]: 4-level GMM tree (8 + 64 + 512 + 4096 = 4680 nodes) on bun000.ply,
    CPU-twin constants (ls = 80, ld = 1e-4, sig2 = 0.00034, seed-72 initial means)."""
    path = os.path.join(ROOT, "tests", "golden", "bun000_xyz.npy")
    if not os.path.exists(path):
        return None
    P = np.load(path).astype(np.float64)
    L, T = 4, 4680
    idx = np.random.RandomState(72).randint(T, size=T)
    ctx.set_points(P)
    ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.00034, 1000)               # warm-up
    # what the reference's buildGMMTree returns: the node tables (hgmm_gpu.py:466-548; currentIdx stays on the device)
    ts, ts_leaf = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        pi, mu, cov, leaf, iters, q = ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.00034, 1000, want_leaf=False)
        ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.00034, 1000)
        ts_leaf.append(time.perf_counter() - t0)
    dt = float(np.median(ts))
    return {"workload": "bun000.ply N=40256, HGMM L=4 (4680 nodes), float64, ls=80 ld=1e-4 sig2=0.00034",
            "build_ms": dt * 1e3, "build_with_leaf_assignment_download_ms": float(np.median(ts_leaf)) * 1e3,
            "level_iterations": [int(v) for v in iters],
            "level_iterations_per_s": float(iters.sum() / dt), "q_final": float(q[-1])}


def tree_1m_leg(ctx):
    """HGMM build at Waymo scale: the C3 frame (N = 1e6, float64), L = 4.  The level log-likelihood over ALL
    8^(l+1) nodes of the level (the reference's stop rule, hgmm_gpu.py:107-115, 532) dominates: N x 8^(l+1)
    Gaussian evaluations of ~25 fp64 flops per level-iteration."""
    P = synth_frame(0).astype(np.float64)
    L, T = 4, 4680
    idx = np.random.RandomState(72).randint(len(P), size=T)
    ctx.set_points(P)
    ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.01, 4)                     # warm-up
    # median of five builds each way, alternating (the first builds after the warm-up still run at ramping clocks); the
    # kernel times and the executed-pair count are those of the last node-tables-only build
    ts, ts_leaf = [], []
    for rep in range(5):
        last = rep == 4
        if last:
            ctx.profile_reset()
            ctx.profile_enable(True)
        t0 = time.perf_counter()
        pi, mu, cov, leaf, iters, q = ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.01, 4, want_leaf=False)  # 4 iterations per level
        ts.append(time.perf_counter() - t0)
        if last:
            ctx.profile_enable(False)
            ll_ms, ll_n = ctx.profile_get("tree_loglik")
            es_ms, es_n = ctx.profile_get("tree_estep")
            executed, flags = ctx.tree_stats()                  # pdf evaluations the log-likelihood kernels really did
        t0 = time.perf_counter()
        ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.01, 4)
        ts_leaf.append(time.perf_counter() - t0)
    dt, dt_leaf = float(np.median(ts)), float(np.median(ts_leaf))
    # the same build with the stop rule's pdfs in float32 (hgmm_tree_set_precision: the reference GPU file's type)
    f32 = None
    if hasattr(ctx, "tree_set_precision"):
        ctx.tree_set_precision(np.float32)
        try:
            ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.01, 4, want_leaf=False)
            t32 = []
            for rep in range(5):
                last = rep == 4
                if last:
                    ctx.profile_reset()
                    ctx.profile_enable(True)
                t0 = time.perf_counter()
                r32 = ctx.tree_build(L, 80.0, 1e-4, P[idx], 0.01, 4, want_leaf=False)
                t32.append(time.perf_counter() - t0)
                if last:
                    ctx.profile_enable(False)
            ll32_ms, ll32_n = ctx.profile_get("tree_loglik")
            ex32, _ = ctx.tree_stats()
            f32 = {"build_ms": float(np.median(t32)) * 1e3, "loglik_kernel_ms_total": ll32_ms, "loglik_launches": ll32_n,
                   "executed_pairs": ex32, "level_iterations": [int(v) for v in r32[4]],
                   "node_tables_bitwise_equal_to_the_float64_build": bool(all(np.array_equal(a, b) for a, b in zip(r32[:3], (pi, mu, cov)))),
                   "max_relative_dq_vs_float64": float(np.abs(np.asarray(r32[5]) / np.asarray(q) - 1.0).max()),
                   # 20 packed + 6 plain + 4 transcendental VALU instructions per node for the thread's FOUR points
                   "valu_instr_per_executed_pair": 7.5,
                   "note": "level log-likelihood in packed float32 on workgroup-local coordinates, log() and the sum over "
                           "the points in float64; E-step, moments and M-step float64 (tree identical while the levels "
                           "stop after the same iterations)"}
        finally:
            ctx.tree_set_precision(np.float64)
    pairs = sum(int(it) * len(P) * 8 ** (l + 1) for l, it in enumerate(iters))
    # fp64 VALU instructions per EVALUATED pair (tree_loglik_kernel<4>, local-origin triangular form): 9 quadratic
    # form + compare 1 + exp 16 + accumulate 1 = 27 (all full-rate v_fma/v_mul/v_add_f64: one per 4 cycles per SIMD)
    instr_per_pair = 27
    flop = 25.0 * pairs                     # reference-equivalent work: 3 sub + 6-term quadratic form + scale + exp + accumulate
    dead = [int((pi[8 * (8 ** l - 1) // 7: 8 * (8 ** (l + 1) - 1) // 7] == 0).sum()) for l in range(L)]
    lane_rate = info_cus(ctx) * 4 * 16 * SPEC_CLOCK_HZ      # fp64 lane-instructions per second at the spec clock
    return {"workload": "uniform cloud N=1,000,000 (float64), HGMM L=4 (4680 nodes), 4 iterations per level",
            "build_ms": dt * 1e3, "build_with_leaf_assignment_download_ms": dt_leaf * 1e3,
            "build_ms_note": "node tables only, what the reference's buildGMMTree returns (hgmm_gpu.py:466-548); the second "
                             "figure also un-sorts and downloads the N-long leaf assignment (4 MB through pageable memory)",
            "level_iterations": [int(v) for v in iters],
            "ms_per_level_iteration": dt * 1e3 / max(int(iters.sum()), 1),
            "loglik_kernel_ms_total": ll_ms, "estep_kernel_ms_total": es_ms,
            "float32_pdfs": f32,
            "dead_nodes_per_level_at_the_end": dead,
            "roofline": {"kernel": "tree_loglik_kernel<4>", "bound": "valu (fp64)",
                         "reference_pairs": pairs, "executed_pairs": executed,
                         "executed_fraction": executed / pairs if pairs else None,
                         "valu_instr_per_executed_pair": instr_per_pair,
                         "unit": "fraction of the fp64 VALU issue rate at 2.4 GHz",
                         "achieved": executed * instr_per_pair / (ll_ms * 1e-3) if ll_ms else None,
                         "peak": lane_rate,
                         "frac": executed * instr_per_pair / (ll_ms * 1e-3) / lane_rate if ll_ms else None,
                         "algorithmic_TFLOPs": flop / (ll_ms * 1e-3) / 1e12 if ll_ms else None,
                         "algorithmic_frac_of_fp64_peak": flop / (ll_ms * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TF if ll_ms else None,
                         "note": "frac counts only pdfs that were evaluated (nodes with pi < eps and nodes whose pdf is "
                                 "exactly 0 in float64 for a whole workgroup are skipped: q is bitwise the full sum's); "
                                 "algorithmic_* prices all N x 8^(l+1) pairs "
                                 "of the reference's loop at 25 flops and is NOT a utilisation figure",
                         "flags": flags}}


def sharded_tree_leg(ctx, rank, world):
    """N > 1, every rank takes part (the communicator of the joint fit is still attached): ONE HGMM over all ranks' frames
    -- points stay on their GPU, the 10 8^(l+1) moments + q are all-reduced per level-iteration.  Reports what
    keeping the host ahead of the device-side stop rule costs under a communicator: every rank tops its queue up to
    min(iterations + 2, budget) per level, so the surplus is 2 level-iterations (4 all-reduces on unchanged operands) per
    level; round 5 ran up to 15 blind iterations per level."""
    P = synth_frame(rank).astype(np.float64)
    L, T, budget = 4, 4680, 40
    ls = 1.0e-3 * N_POINTS * world                   # (a uniform cloud converges slowly: stop at 1e-3 per point, so that
    init = synth_frame(0).astype(np.float64)[np.random.RandomState(72).randint(N_POINTS, size=T)]       # levels end by the rule)
    ctx.set_points(P)
    ctx.tree_build(L, ls, 1e-4, init, 0.01, budget, want_leaf=False)                 # warm-up
    c0, s0 = ctx.comm_stats()
    ctx.synchronize()
    t0 = time.perf_counter()
    pi, mu, cov, _, iters, q = ctx.tree_build(L, ls, 1e-4, init, 0.01, budget, want_leaf=False)
    dt = time.perf_counter() - t0
    c1, s1 = ctx.comm_stats()
    digest = float(np.abs(mu).sum() + np.abs(cov).sum())
    lo, hi = ctx.allreduce([-digest, digest], op="max")
    return {"workload": "one HGMM (L = 4, ls = %g, <= %d iterations per level) over %d frames of 10^6 points, one per GPU"
                        % (ls, budget, world),
            "ms": dt * 1e3, "level_iterations": [int(v) for v in iters], "collectives": int(c1 - c0),
            "surplus_collectives": int(2 * (s1 - s0)), "surplus_level_iterations": int(s1 - s0),
            "identical_tree_on_all_ranks": bool(-lo == hi),
            "rule": "collectives = 1 (point count) + 2 per enqueued level-iteration (moments, q); enqueued = "
                    "min(iterations + 2, budget) per level on every rank"}


def info_cus(ctx):
    return int(ctx.device_info()["compute_units"])


def fullcov_leg(ctx):
    """Flat FULL-covariance EM (what north_star's kernel description names: (mu, Sigma^-1, logdet, pi) per
    component, 10-float sufficient statistics) at C3 size, float64 like the reference's CPU twin."""
    P = synth_frame(0).astype(np.float64)
    J = J_COMP
    idx = np.random.RandomState(100).choice(len(P), J, replace=False)
    ctx.set_points(P)
    ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, 2)                   # warm-up
    ctx.profile_reset()
    ctx.profile_enable(True)
    iters = 20
    t0 = time.perf_counter()
    ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, iters)
    dt = time.perf_counter() - t0
    ctx.profile_enable(False)
    # (a fit of k iterations is k + 1 launches of the one-pass kernel: the E-step of the initial parameters comes first;
    #  the marginal cost of an iteration = the difference of a 30- and a 10-iteration fit)
    t1 = time.perf_counter()
    ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, 10)
    t2 = time.perf_counter()
    ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, 30)
    t3 = time.perf_counter()
    out = {"workload": "uniform cloud N=1,000,000 (float64), flat full-covariance GMM J=800, %d iterations" % iters,
           "ms_per_iteration": dt * 1e3 / iters,
           "ms_per_iteration_note": "whole fit / iterations: includes the initial parameters' E-step launch, the "
                                    "uploads and the 4 MB label download",
           "marginal_ms_per_iteration": ((t3 - t2) - (t2 - t1)) * 1e3 / 20.0}
    kern = {}
    for k in ("full_pass", "full_moments", "full_fused"):
        try:
            ms, n = ctx.profile_get(k)
        except KeyError:
            continue
        if n:
            kern[k] = {"avg_ms": ms / n, "launches": n}
    out["kernels"] = kern
    # fp64 flops per pair: pdf 3 sub + 9 (quadratic form) + 2 + exp; statistics 2 x 10 (fma) on the matrix cores
    flop = 36.0 * len(P) * J
    out["roofline"] = {"bound": "valu+mfma (fp64)", "unit": "TFLOP/s", "achieved": flop / (dt / iters) / 1e12,
                       "peak": FP64_VECTOR_PEAK_TF, "frac": flop / (dt / iters) / 1e12 / FP64_VECTOR_PEAK_TF,
                       "flop_per_pair": 36}
    # the same fit with the FLOAT32 TILE (Context.tree_set_precision(np.float32): the reference GPU file's type; opt-in):
    # time, and how far its result is from the float64 fit's after the same 20 iterations
    try:
        ref = ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, iters)
        ctx.tree_set_precision(np.float32)
        ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, 2)
        ctx.profile_reset()
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        got = ctx.fullcov_fit(J, 1e-30, 1e-4, P[idx], 0.01, iters)
        dt32 = time.perf_counter() - t0
        ctx.profile_enable(False)
        ms, nl = ctx.profile_get("full_fused")
        var = np.abs(np.einsum("jii->j", ref[2])) / 3.0
        out["float32_tile"] = {
            "ms_per_iteration": dt32 * 1e3 / iters, "kernel_avg_ms": ms / nl if nl else None, "launches": nl,
            "vs_float64_after_%d_iterations" % iters: {
                "labels_differing": int((ref[3] != got[3]).sum()), "points": int(len(ref[3])),
                "max_abs_dq": float(np.abs(ref[4] - got[4]).max()),
                "max_rel_dpi": float(np.max(np.abs(ref[0] - got[0]) / np.maximum(ref[0], 1e-300))),
                "max_abs_dmu": float(np.abs(ref[1] - got[1]).max()),
                "max_dcov_over_variance": float(np.max(np.abs(ref[2] - got[2]).reshape(J, -1).max(1) / var))},
            "note": "pdfs, tile, gamma and the statistics' products in float32 (v_mfma_f32_16x16x4_f32 about the cloud's "
                    "centroid, float partials per 256 points added in float64); row sums, 1 / den, log and the M-step float64"}
    except Exception as e:                                            # noqa: BLE001 -- a side figure must not take the leg down
        out["float32_tile"] = {"error": repr(e)}
    finally:
        ctx.tree_set_precision(np.float64)
    return out


def estep_roofline_leg(ctx, lr, init, fitted, args):
    """`roofline` of the JSON line: the materialising E-step kernel (the API's e_step(): log_resp[N,J] written once).
    STEADY figure: mean hipEvent time of `--estep-reps` launches after 40 warm-up launches.  COLD figures: what a
    caller of e_step() gets right after a fit -- the first launches behind the VALU-heavy fused loop run at other
    clocks (up to 25 % slower): a 50-iteration fit, then 15 launches timed one by one."""
    inv, mu, w = fitted
    mu0, cov0, w0 = init
    ctx.flat_train(50, 0.0, mu0, cov0, w0, "diag", "W")
    cold = []
    for _ in range(15):
        ctx.profile_reset()
        ctx.profile_enable(True)
        ctx.flat_estep(inv, mu, w, "diag", "W", out=lr)
        ctx.profile_enable(False)
        cold.append(ctx.profile_get("flat_estep")[0])
    for _ in range(25):
        ctx.flat_estep(inv, mu, w, "diag", "W", out=lr)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(args.estep_reps):
        ctx.flat_estep(inv, mu, w, "diag", "W", out=lr)
    ctx.profile_enable(False)
    e_ms, e_n = ctx.profile_get("flat_estep")
    avg_s = e_ms / e_n * 1e-3
    # the same launches as a STREAM nobody waits for (hgmm_flat_estep_async): no idle moment between two launches
    for timed in (False, True):
        ctx.profile_reset()
        ctx.profile_enable(timed)
        for _ in range(args.estep_reps):
            ctx.flat_estep(inv, mu, w, "diag", "W", out=lr, lazy_mean=True)
        ctx.synchronize()
    ctx.profile_enable(False)
    s_ms, s_n = ctx.profile_get("flat_estep")
    stream_s = s_ms / max(s_n, 1) * 1e-3
    alg_bytes = 12 * N_POINTS + 4 * N_POINTS * J_COMP + 4 * N_POINTS + 28 * J_COMP
    achieved = alg_bytes / avg_s / 1e9
    traffic, traffic_source, rocprof_mean_us = None, None, None
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc):
        try:
            rec = json.load(open(pmc))
            traffic = rec.get("flat_estep_bytes_per_launch")
            rocprof_mean_us = rec.get("flat_estep_rocprof_mean_us")
            traffic_source = ("profiles/pmc_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                              "kernel (separate runs of this bench command, measured %s on commit %s; counters cannot be "
                              "collected inside a timed run)" % (rec.get("measured_on", "in an earlier round"),
                                                                rec.get("commit", "unrecorded")))
        except Exception:
            traffic = None
    cold_avg = float(np.mean(cold))
    pace = getattr(ctx, "pace_info", lambda: (None, None, None))()
    # headline: the mean over the three call patterns the kernel was timed in (equal weights) -- blocking calls, an
    # unwaited-for stream, the launches right behind a fit; each pattern's own figure stays beside it
    pattern_ms = [avg_s * 1e3, stream_s * 1e3, cold_avg] if stream_s else [avg_s * 1e3, cold_avg]
    mean_s = float(np.mean(pattern_ms)) * 1e-3
    blocking = achieved
    achieved = alg_bytes / mean_s / 1e9
    return {"kernel": "materialising E-step (flat_estep kernel, log_resp[N,J] written once)",
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
            "rocprof_mean_us": rocprof_mean_us,
            "rocprof_mean_note": "mean launch duration of this kernel in the committed rocprofv3 --kernel-trace --stats of this "
                                 "bench command (profiles/pmc_traffic.json, same lease as `traffic`); `avg_launch_ms` is this "
                                 "run's own hipEvent figure",
            "rule": "achieved = algorithmic bytes / mean launch duration over the call patterns below (hipEvents), equal weights",
            "patterns_ms": {"blocking_calls": avg_s * 1e3, "unsynchronised_stream": stream_s * 1e3,
                            "right_behind_a_fit": cold_avg},
            "blocking_calls_frac": blocking / HBM_PEAK_GBS,
            "store_pacer": {"offered_GBs": pace[0], "controller_steps_down": pace[1], "controller_probes_held": pace[2],
                            "rule": "rows offered at this rate (wall-clock schedule per wave); starts at 6600, backs off 2 % after "
                                    "three launches in a row that ran > 6 % longer than the rate explains, probes 2 % upwards "
                                    "after 24 clean launches (one long launch takes a probe back and caps the rate)"},
            "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": mean_s * 1e3, "launches": e_n + s_n + len(cold),
            "steady_state_rule": "40 untimed launches (15 of them the cold ones below) precede the timed ones; every "
                                 "launch is a blocking hgmm_flat_estep call (the host reads the mean, ~25 us idle)",
            "unsynchronised_stream_avg_ms": stream_s * 1e3,
            "unsynchronised_stream_frac": alg_bytes / stream_s / 1e9 / HBM_PEAK_GBS if stream_s else None,
            "unsynchronised_stream_rule": "the same launches enqueued back to back (hgmm_flat_estep_async), nothing "
                                          "waits in between: the chip runs at its sustained clocks",
            "first_launch_ms": cold[0], "cold_avg_ms": cold_avg, "cold_max_ms": float(np.max(cold)),
            "cold_frac": alg_bytes / (cold_avg * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "cold_rule": "15 launches timed one by one (hipEvents) straight after a 50-iteration fused fit"}


def materialised_iteration_leg(ctx, lr, inv, mu, w):
    """API-faithful iteration, the way a caller of the reference's module functions runs its own loop
    (gmm_impl.py:125-138): log_ll, log_resp = e_step(X, inv_cov, means, weights); weights, means, cov = m_step(X,
    exp(log_resp)); inv_cov = 1 / (sqrt(cov + 1e-6) + eps); stop test on log_ll.  Timed in the two array modules the
    reference's functions accept:
      device arrays  (the reference under CuPy, `it_per_s`): the M-step's results stay in HBM (DeviceArray), the
                     inverse standard deviations are formed there by elementwise kernels, the E-step packs its table
                     from them; the only thing the host reads per iteration is the mean log-normaliser -- a pinned
                     scalar behind an event, so the M-step keeps running while the loop looks at it;
      host arrays    (`host_array_loop`): parameters as NumPy arrays -- every iteration downloads the M-step's results
                     (its one synchronisation), forms inv_cov on the host and uploads it with the next E-step.
    Both start from the fit's initial parameters (two untimed iterations, then eight timed ones): the state a caller's
    loop is in when it starts."""
    reps = 8
    eps6, eps8 = np.float32(1e-6), np.float32(1e-8)

    def run(device_arrays, n_it):
        if device_arrays:
            inv_k, mu_k, w_k = ctx.to_device(inv), ctx.to_device(mu), ctx.to_device(w)
        else:
            inv_k, mu_k, w_k = inv, mu, w
        prev, mean = -np.inf, None
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_it):
            mean, _, _, _ = ctx.flat_estep(inv_k, mu_k, w_k, "diag", "W", out=lr, lazy_mean=True)
            w_k, mu_k, cov_k = ctx.flat_mstep(lr.exp(), "diag", "W", centre_hint=mu_k, device_out=device_arrays)
            if device_arrays:
                inv_k = 1.0 / (np.sqrt(cov_k + eps6) + eps8)                  # four small kernels, nothing waits
                m = float(mean)                                                # (waits for the E-step's event only)
                change, prev = m - prev, m                                     # the stop test's operands (not applied)
            else:
                inv_k = (1.0 / (np.sqrt(cov_k + eps6) + eps8)).astype(np.float32)
        ctx.synchronize()
        return (time.perf_counter() - t0) / n_it, float(mean), np.asarray(mu_k, dtype=np.float32)

    legs = {}
    for device_arrays in (False, True):
        run(device_arrays, 2)
        ctx.profile_reset()
        ctx.profile_enable(True)
        dt, last_mean, mu_end = run(device_arrays, reps)
        ctx.profile_enable(False)
        m_ms, m_n = ctx.profile_get("flat_mstep")
        e_ms, e_n = ctx.profile_get("flat_estep")
        k_ms = (m_ms + e_ms) / max(m_n, 1)
        legs[device_arrays] = {"it_per_s": 1.0 / dt, "ms_per_iteration": dt * 1e3, "kernel_ms_per_iteration": k_ms,
                               "outside_the_two_kernels_ms_per_iteration": dt * 1e3 - k_ms,
                               "last_mean_log_normaliser": last_mean, "mstep_avg_ms": m_ms / max(m_n, 1),
                               "_mu": mu_end}
    dev, host = legs[True], legs[False]
    # the two loops run the same kernels on the same numbers: elementwise float32 on the device == NumPy's
    agree = bool(np.array_equal(dev.pop("_mu"), host.pop("_mu"))) and dev["last_mean_log_normaliser"] == host["last_mean_log_normaliser"]
    m_avg_s = dev["mstep_avg_ms"] * 1e-3
    m_bytes = 4 * N_POINTS * J_COMP + 12 * N_POINTS
    out = dict(dev)
    out.update({"arrays": "device (DeviceArray parameters, pinned scalar for the stop test)",
                "host_overhead_ms_per_iteration": dev["outside_the_two_kernels_ms_per_iteration"],
                "host_array_loop": host, "device_and_host_array_loops_bitwise_equal": agree,
                "mstep_GBs": m_bytes / m_avg_s / 1e9,
                "roofline": {"kernel": "flat_mstep_kernel<3,1>", "bound": "hbm", "unit": "GB/s",
                             "achieved": m_bytes / m_avg_s / 1e9, "peak": HBM_PEAK_GBS,
                             "frac": m_bytes / m_avg_s / 1e9 / HBM_PEAK_GBS}})
    return out


def log_prob_leg(ctx, fitted):
    """estimate_log_prob(X, inv_cov, means) (gmm_impl.py:53-78) on the C3 frame: the un-normalised N x J table.  The same
    bytes as e_step's output, no exponential, no reduction: the kernel is as close to a pure store stream as this path
    gets (four rows in flight per wave, 16-byte non-temporal stores)."""
    inv, mu, w = fitted
    out = None
    for _ in range(5):
        out = None
        out = ctx.flat_log_prob(inv, mu, "diag")
    ctx.profile_reset()
    ctx.profile_enable(True)
    reps = 20
    for _ in range(reps):
        out = None                                      # (the dead table's memory is handed to the next one)
        out = ctx.flat_log_prob(inv, mu, "diag")
    ctx.profile_enable(False)
    k_ms, k_n = ctx.profile_get("flat_estep")
    del out
    k_s = k_ms / max(k_n, 1) * 1e-3
    alg = 12 * N_POINTS + 4 * N_POINTS * J_COMP + 28 * J_COMP
    return {"workload": "estimate_log_prob() on the 1M-point frame, J=800 (log N(x_i; mu_j, diag) for all pairs)",
            "kernel_ms": k_s * 1e3, "launches": k_n,
            "roofline": {"kernel": "flat_logprob_rows_pk_kernel<3,1>", "bound": "hbm", "unit": "GB/s",
                         "algorithmic_bytes_per_launch": alg, "achieved": alg / k_s / 1e9, "peak": HBM_PEAK_GBS,
                         "frac": alg / k_s / 1e9 / HBM_PEAK_GBS}}


def predict_leg(ctx, fitted):
    """predict(X, inv_cov, means, weights) (gmm_impl.py:147-155) on the C3 frame: labels[N] only, parameters in device
    arrays, one call per frame the way run_gmm_waymo_gpu.py:32-61 predicts every frame."""
    inv, mu, w = fitted
    p = (ctx.to_device(inv), ctx.to_device(mu), ctx.to_device(w))
    for _ in range(3):
        lab = ctx.flat_predict(*p)
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile_enable(True)
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        lab = ctx.flat_predict(*p)
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / reps
    ctx.profile_enable(False)
    k_ms, k_n = ctx.profile_get("flat_estep")
    k_s = k_ms / max(k_n, 1) * 1e-3
    flop = 12.0 * N_POINTS * J_COMP                 # per pair and axis: x - mu, (x - mu) g, c -= ((x - mu) g)(x - mu)
    del lab
    return {"workload": "predict() on the 1M-point frame, J=800 (labels only; parameters in device arrays)",
            "ms_per_frame": dt * 1e3, "kernel_ms": k_s * 1e3, "points_per_s": N_POINTS / dt,
            "roofline": {"kernel": "flat_predict_rows_kernel<3,1>", "bound": "valu", "unit": "TFLOP/s",
                         "flop_per_pair": 12, "achieved": flop / k_s / 1e12, "peak": FP32_VECTOR_PEAK_TF,
                         "frac": flop / k_s / 1e12 / FP32_VECTOR_PEAK_TF,
                         "note": "the arg-max (row maximum, index search, two wave reductions) is as many issue slots "
                                 "again as the quadratic forms and is not counted as flops"}}


def published_charts_leg(ctx):
    """The only numbers the reference publishes (bar charts, /root/reference/README.md:214-251, read off in BASELINE.md
    section 1; hardware and inputs unstated) -- the same workloads through the drop-in API on this box:
      gmm_perf1    flat GMM fit, 100 components, 10 k / 50 k / 100 k / 250 k points, a fixed number of iterations
                   (30 = GMM_GPU's default max_iter, gmm.py:46; tol = 0 so that all run), host array in, parameters
                   out; next to it the HGMM at level 2 (72 components) to convergence, as the chart has it;
      hgmm_perf_lvls  buildGMMTree on bun000.ply at tree levels 2 - 5 (72 / 584 / 4680 / 37448 nodes) with the
                   constants of the reference's GPU file (ls = 20, sig2 = 0.004, seed 72: hgmm_gpu.py:469-477, 687);
      gmm_perf3    the streaming loop of run_gmm_waymo_gpu.py:32-61 without the viewer (50 components, spherical,
                   max_iter 50, refit every 10 frames, predict + label download every frame) for 1 k ... 100 k points.
    The chart values are the reference authors' own hardware: context, not a like-for-like baseline."""
    import contextlib
    import io
    import warnings
    from hgmm_amd.gmm_waymo.gmm import GMM_GPU
    from hgmm_amd.gmm_waymo.run_gmm_stream import run_stream
    from hgmm_amd.hgmm.hgmm_gpu import buildGMMTree, n_total_nodes
    import hgmm_amd
    hgmm_amd.set_default_context(ctx)
    frame = synth_frame(0)
    quiet = io.StringIO()
    out = {"source": "reference README.md:214-251 (charts read off to +-5 %, BASELINE.md section 1); reference hardware unstated",
           "data": "uniform [0,1)^3 subsets of the C3 frame (fit / stream), bun000.ply (tree levels)"}
    # ---- gmm_perf1 ---------------------------------------------------------------------------------------------
    chart1 = {10_000: (5.0, 1.0, 0.2), 50_000: (23.0, 2.5, 1.0), 100_000: (32.5, 13.0, 2.5), 250_000: (87.0, 40.0, 13.0)}
    rows = []
    with contextlib.redirect_stdout(quiet), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n, (ref_cpu, ref_gpu, ref_hgmm) in chart1.items():
            X = frame[:n]
            g = GMM_GPU(n_gmm_components=100, max_iter=30, tol=0.0, cov_type="diag")
            g.init()
            np.random.seed(0)
            g.compute(X)                                                  # warm-up (buffers of this size)
            ts = []
            for _ in range(3):
                np.random.seed(0)
                t0 = time.perf_counter()
                g.compute(X)
                ts.append(time.perf_counter() - t0)
            P = X.astype(np.float64)
            buildGMMTree(P, 2, 20, 1e-4, ctx=ctx)
            th = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, _, _, tr = buildGMMTree(P, 2, 20, 1e-4, ctx=ctx, return_trace=True)
                th.append(time.perf_counter() - t0)
            rows.append({"points": n, "flat_100_components_30_iterations_s": float(np.median(ts)),
                         "hgmm_level2_72_components_to_convergence_s": float(np.median(th)),
                         "hgmm_level_iterations": [int(v) for v in tr["iters_per_level"]],
                         "reference_chart_s": {"gmm_cpu": ref_cpu, "gmm_gpu": ref_gpu, "hgmm_gpu_level2": ref_hgmm}})
    out["gmm_perf1_fit_seconds"] = rows
    # ---- hgmm_perf_lvls ----------------------------------------------------------------------------------------
    path = os.path.join(ROOT, "tests", "golden", "bun000_xyz.npy")
    if os.path.exists(path):
        P = np.load(path).astype(np.float64)
        chart2 = {2: 1.0, 3: 3.0, 4: 20.0, 5: 149.0}
        rows = []
        for L, ref_s in chart2.items():
            buildGMMTree(P, L, 20, 1e-4, ctx=ctx)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, _, _, tr = buildGMMTree(P, L, 20, 1e-4, ctx=ctx, return_trace=True)
                ts.append(time.perf_counter() - t0)
            rows.append({"tree_level": L, "nodes": n_total_nodes(L), "build_s": float(np.median(ts)),
                         "level_iterations": [int(v) for v in tr["iters_per_level"]],
                         "reference_chart_s": ref_s})
        out["hgmm_perf_lvls_build_seconds"] = {"cloud": "bun000.ply, 40256 points (the chart's N is unstated)", "rows": rows}
    # ---- gmm_perf3 ---------------------------------------------------------------------------------------------
    chart3 = {1_000: (2.0, 14.3), 10_000: (0.5, 3.1), 25_000: (0.1, 1.3), 50_000: (0.05, 0.7), 100_000: (None, 0.15)}
    rows = []
    with contextlib.redirect_stdout(quiet), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n, (ref_cpu, ref_gpu) in chart3.items():
            # 30 "frames": the same n points jittered per frame (a LIDAR stream's frames differ; the loop's cost does not
            # depend on how), refit every 10
            rs = np.random.RandomState(n)
            frames = [frame[:n] + np.float32(0.002) * rs.randn(n, 3).astype(np.float32) for _ in range(30)]
            run_stream(frames[:10], n_components=50, max_iter=50, cov_type="spherical", fit_every=10)      # warm-up
            res = run_stream(frames, n_components=50, max_iter=50, cov_type="spherical", fit_every=10)
            rows.append({"points": n, "fps": float(res["fps"]), "mean_refit_s": float(np.mean(res["fit_s"])),
                         "frames": int(res["frames"]),
                         "reference_chart_fps": {"cpu": ref_cpu, "gpu": ref_gpu}})
    out["gmm_perf3_stream_fps"] = {"loop": "50 components, spherical, max_iter 50 / tol 1e-4, refit every 10 frames, predict + "
                                           "label download every frame, H2D of every frame; no viewer (the reference's FPS "
                                           "includes Open3D rendering, README.md:250)", "rows": rows}
    return out


def replica_pairs_leg(ctx):
    """The replica mode (`bench.py --mode pairs`, hgmm_amd.replicas) as a side leg of the default line: independent scan
    pairs, eight contexts x 32 pairs per launch set on this GPU (the mode's defaults), no communicator -- run as a process
    of its own (it creates its own contexts and threads)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", "pairs", "--steps", "20", "--warmup", "2", "--min-time", "3.0",
           "--no-cpu-baseline", "--full"]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    env["LOCAL_RANK"] = str(getattr(ctx, "device_id", 0))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": "rc %d: %s" % (r.returncode, r.stderr[-400:])}
    d = json.loads(lines[-1])
    return {"workload": d["config"]["workload"], "pairs_per_s": d["value"], "contexts_per_gpu": d["config"]["contexts_per_gpu"],
            "batch": d["config"].get("batch"), "scan_dtype": d.get("scan_dtype"), "other_scan_dtype": d.get("other_scan_dtype"),
            "ms_per_step": d["ms_per_step"], "registration_iterations_per_pair": d["registration_iterations_per_pair"],
            "accuracy": d["accuracy"], "kernels_ms_per_pair": d.get("kernels_ms_per_pair"), "blocks": d["timing"]["blocks"]}


def fused_roofline(avg_launch_s, cus):
    """VALU accounting of flat_fused_pk_kernel<13> from the code object (tools/isa_count.py)."""
    out = {"kernel": "flat_fused_pk_kernel<13> (constant-shift loop)", "bound": "valu", "unit": "TFLOP/s",
           "peak": FP32_VECTOR_PEAK_TF, "flop_per_pair": FUSED_FLOP_PER_PAIR, "avg_launch_ms": avg_launch_s * 1e3}
    flop = float(FUSED_FLOP_PER_PAIR) * N_POINTS * J_COMP
    out["achieved"] = flop / avg_launch_s / 1e12
    out["frac"] = out["achieved"] / FP32_VECTOR_PEAK_TF
    out["recomputed_flop_per_pair"] = FUSED_RECOMPUTED_FLOP_PER_PAIR
    out["frac_counting_recomputed"] = (out["achieved"] * (FUSED_FLOP_PER_PAIR + FUSED_RECOMPUTED_FLOP_PER_PAIR)
                                       / FUSED_FLOP_PER_PAIR / FP32_VECTOR_PEAK_TF)
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import isa_count
        # the constant-shift row loop is the loop with exactly one wave reduction (6 DPP steps)
        lp = isa_count.loop_profile("flat_fused_pk_kernelILi13", want=lambda l: l.get("valu_dpp", 0) == 6)
        simds = cus * 4
        instr_per_simd = lp["valu"] * N_POINTS / simds
        out.update({"valu_instr_per_row": lp["valu"], "packed_fp32_instr_per_row": lp.get("valu_pk", 0),
                    "transcendental_instr_per_row": lp.get("valu_trans", 0),
                    "lane_components_per_row": 13 * 64,
                    "valu_instr_per_cycle_per_simd_at_2.4GHz": instr_per_simd / (avg_launch_s * SPEC_CLOCK_HZ),
                    "cycles_per_valu_instr_at_2.4GHz": avg_launch_s * SPEC_CLOCK_HZ / instr_per_simd,
                    "source": "code object in libhgmm_hip.so (tools/isa_count.py); per-class issue cost measured by "
                              "tools/valubench.hip -> profiles/r02/valubench.log"})
    except Exception as e:                                   # llvm-objdump missing: keep the flop figures
        out["isa_count_error"] = repr(e)
    return out


# ------------------------------------------------------------------------------------------------
COLLECTIVES = {
    "rccl": "RCCL ncclAllReduce(sum, float64) on the kernel stream",
    "ipc": "one-shot peer exchange over mapped peer memory (hipIpc, xGMI): one kernel per all-reduce, every rank "
           "writes its slice into every peer's buffer, slices summed in rank order",
    "host": "host shared memory (device -> shm -> device)",
}
# what a rank moves on to when a backend cannot be set up on every rank (decided collectively, see choose_collective)
# (the host backend comes BEFORE the peer exchange: the exchange has run with up to eight ranks on ONE GPU but never across
#  two -- until a multi-GPU node has validated it, the headline must not depend on it; `--collective auto` still times it
#  as the side leg `peer_exchange`, wrapped so that its failure cannot lose the line -- ADVICE r4)
FALLBACK_ORDER = {"auto": ["rccl", "host", "ipc"], "rccl": ["rccl", "host", "ipc"], "ipc": ["ipc", "host"], "host": ["host"]}
ATTACH_TIMEOUT_S = float(os.environ.get("HGMM_BENCH_ATTACH_TIMEOUT", "180"))


def _run_with_timeout(fn, seconds):
    """fn() in a daemon thread -> None, or the exception / a TimeoutError.  (A collective set-up call can block for ever
    when a peer rank failed in it: the thread is then abandoned and the backend counts as unavailable.)"""
    import threading
    box = {}

    def work():
        try:
            fn()
        except BaseException as e:          # noqa: BLE001 -- reported, not swallowed
            box["err"] = e
        box["done"] = True
    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(seconds)
    if not box.get("done"):
        return TimeoutError("no answer within %.0f s" % seconds)
    return box.get("err")


def attach_collective(ctx, kind, rank, world, token):
    from hgmm_amd import parallel
    if kind == "rccl":
        return _run_with_timeout(lambda: parallel.attach_communicator(ctx, rank, world, transport="tcp"), ATTACH_TIMEOUT_S)
    if kind == "ipc":
        return _run_with_timeout(lambda: ctx.comm_init_ipc(world, rank, "hgmm_bench_ipc_%s" % token), ATTACH_TIMEOUT_S)
    return _run_with_timeout(lambda: ctx.comm_init_host(world, rank, "hgmm_bench_host_%s" % token), ATTACH_TIMEOUT_S)


def choose_collective(ctx, rank, world, order, token, hosts, round0=1):
    """Attach the first backend of `order` that EVERY rank can set up: after each attempt the ranks all-gather their ok
    flags over plain TCP, so a failure on some ranks only cannot leave the ranks on different backends.
    -> (kind or None, [(kind, error text), ...] of the attempts that failed somewhere)."""
    from hgmm_amd import parallel
    import hgmm_amd
    failed = []
    for i, kind in enumerate(order):
        if kind != "rccl" and len(hosts) > 1:
            failed.append((kind, "the ranks span %s: this backend needs one host" % hosts))
            continue
        err = attach_collective(ctx, kind, rank, world, token)
        if err is not None:
            sys.stderr.write("rank %d: %s backend could not be set up: %r\n" % (rank, kind, err))
        # (a rank that failed at once waits here for one that sits out its whole attach timeout: the agreement's own
        #  deadline must outlast ATTACH_TIMEOUT_S, or the fast rank gives up before rank 0 even listens -- ADVICE r4)
        flags = parallel.allgather_bytes_tcp(rank, world, b"0" if err is not None else b"1",
                                             port_offset=137 + 10 * (round0 + i), timeout=ATTACH_TIMEOUT_S + 60.0)
        if all(f == b"1" for f in flags):
            return kind, failed, ctx
        failed.append((kind, repr(err) if err is not None else "failed on another rank"))
        if err is None:
            # this rank's communicator is useless without the others (the call may wait for peers that are gone)
            _run_with_timeout(ctx.comm_destroy, 30.0)
        elif isinstance(err, TimeoutError):
            # the abandoned attach thread may still be inside the library with this context: the next backend gets a
            # context of its own (the old one is left to the daemon thread and never touched again)
            ctx = hgmm_amd.Context(ctx.device_id)
    return None, failed, ctx


def enough_blocks(blocks, min_time, share=1.0):
    """One timed block by default; with --min-time S, blocks repeat until share x S seconds and three blocks."""
    if min_time is None:
        return True
    return (sum(blocks) >= share * min_time and len(blocks) >= 3) or len(blocks) >= MAX_BLOCKS


def dump_outputs(path, arrays):
    """--dump-outputs: every array as path/<name>.npy, float64 kept float64 (integers too), everything else float32."""
    os.makedirs(path, exist_ok=True)
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        out[name] = a.astype(np.float64 if a.dtype == np.float64 or a.dtype.kind in "iu" else np.float32)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError("--dump-outputs: %d bytes, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def timed_fit(ctx, args, world, init, profile=False):
    """The timed region: W warm-up steps, then one block of exactly K fused EM iterations (--min-time: blocks of K until
    enough_blocks), bracketed by barrier + stream synchronisation, MAX over ranks; the fitted model after the last timed
    step.  profile: one more K-step fit from the same start under the hipEvent profiler (not part of the timing)."""
    mu0, cov0, w0 = init

    def barrier():
        ctx.synchronize()
        ctx.allreduce([0.0])

    K, W = args.steps, args.warmup
    cap = W + K * (MAX_BLOCKS + 1) + 8
    # the chip's clocks need tens of milliseconds of load to settle and the driver's --warmup (5 steps = 1.7 ms) does not
    # provide them: a fixed internal warm-up of CLOCK_WARMUP_STEPS fused iterations on a scratch fit (not part of any count,
    # the timed fit below starts from the initial parameters again) makes `value` independent of --warmup
    if CLOCK_WARMUP_STEPS > 0:
        ctx.flat_train_begin(0.0, mu0, cov0, w0, "diag", "W", lls_capacity=CLOCK_WARMUP_STEPS + 8)
        ctx.flat_train_step(CLOCK_WARMUP_STEPS)
        ctx.flat_train_end()
    ctx.flat_train_begin(0.0, mu0, cov0, w0, "diag", "W", lls_capacity=cap)
    ctx.flat_train_step(W)
    blocks = []
    while True:
        barrier()
        t0 = time.perf_counter()
        ctx.flat_train_step(K)
        barrier()
        dt_local = time.perf_counter() - t0
        blocks.append(float(ctx.allreduce([dt_local], op="max")[0]))        # identical on every rank
        if enough_blocks(blocks, args.min_time):
            break
    inv, mu, w, cov, lls, conv, n_it = ctx.flat_train_end()
    assert n_it == W + K * len(blocks), (n_it, W, K, len(blocks))
    assert np.isfinite(lls).all()
    fused_ms = fused_n = ar_ms = ar_n = None
    if profile:
        # one more block under the hipEvent profiler (not part of the timing): kernel and all-reduce durations
        ctx.flat_train_begin(0.0, mu0, cov0, w0, "diag", "W", lls_capacity=K + 8)
        barrier()
        ctx.profile_reset()
        ctx.profile_enable(True)
        ctx.flat_train_step(K)
        barrier()
        ctx.profile_enable(False)
        fused_ms, fused_n = ctx.profile_get("flat_fused")
        ar_ms, ar_n = ctx.profile_get("allreduce") if (world > 1 or args._world1_comm) else (0.0, 0)
        ctx.flat_train_end()
    # every rank must hold the same model after the joint fit: checksum of (mu, cov, w, inv) as raw 32-bit words
    # (exact in float64), all-reduced with max and with min -- equal on all ranks iff max == min
    words = np.concatenate([np.ascontiguousarray(a).view(np.uint32).ravel() for a in (mu, cov, w, inv)]).astype(np.float64)
    sums = np.array([words.sum(), (words * (1.0 + np.arange(len(words)) % 1021)).sum()])
    hi = ctx.allreduce(sums, op="max")
    lo = -ctx.allreduce(-sums, op="max")
    consistent = bool(np.array_equal(hi, lo))
    barrier()
    return {"blocks": blocks, "fused_ms": fused_ms, "fused_n": fused_n, "ar_ms": ar_ms, "ar_n": ar_n,
            "model": (inv, mu, w, cov), "lls": lls, "consistent": consistent, "checksum": [float(v) for v in hi],
            "checksum_lo": [float(v) for v in lo]}


def collective_world1_leg(ctx, args, init, base_it_per_s):
    """What the all-reduce call itself costs on the stream, before any link is crossed: the fused loop with a
    communicator of ONE rank attached -- RCCL (ncclAllReduce of 57 KB in place) and the one-shot peer exchange (its
    kernel writes the slice into this rank's own slot and reads it back).  `allreduce_us` = hipEvent time around the
    call per iteration; `it_per_s` against `it_per_s_no_communicator` also shows what the enqueue costs the host."""
    out = {"payload_bytes": 8 * (7 * 1024 + 2), "it_per_s_no_communicator": base_it_per_s}
    a2 = argparse.Namespace(**vars(args))
    a2.min_time = 0.3 if args.min_time is None else min(args.min_time, 0.3)
    a2._world1_comm = True
    for kind in ("rccl", "ipc"):
        try:
            if kind == "rccl":
                ctx.comm_init(1, 0, type(ctx).comm_unique_id())
            else:
                ctx.comm_init_ipc(1, 0, "hgmm_bench_w1_%d" % os.getpid())
            try:
                r = timed_fit(ctx, a2, 1, init, profile=True)
            finally:
                ctx.comm_destroy()
            med = float(np.median(r["blocks"]))
            out[kind] = {"allreduce_us": 1e3 * r["ar_ms"] / max(r["ar_n"], 1), "launches": r["ar_n"],
                         "it_per_s": args.steps / med, "ms_per_step": 1e3 * med / args.steps,
                         "fused_kernel_avg_ms": r["fused_ms"] / max(r["fused_n"], 1)}
        except Exception as e:                                  # a side leg must not lose the headline line
            out[kind] = {"error": repr(e)}
    return out


LEG_KEYS = ("bunny", "hgmm", "tree_1M", "fullcov", "kmeans_init", "registration", "published_charts", "replica_pairs",
            "materialised_iteration", "predict", "estimate_log_prob", "collective_world1")


def _pick(d, *path):
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return round(d, 4) if isinstance(d, float) else d


def split_legs(out, args):
    """The side legs in full go to a file next to the line (`legs.file`; gpurun_out/ travels back from a GPU box), the
    line keeps the contract's keys, `roofline`, `cpu_baseline` and -- LAST, so that a reader who only keeps the tail of
    the line still has them -- one figure per leg in `summary`."""
    legs = {k: out.pop(k) for k in LEG_KEYS if k in out}
    path = os.environ.get("HGMM_BENCH_LEGS_FILE") or os.path.join(ROOT, "gpurun_out", "bench_legs_n%d.json" % out["n_gpus"])
    written = None
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(legs, f, indent=1)
        written = os.path.relpath(path, ROOT)
    except OSError as e:
        written = "not written: %r" % (e,)
    out["legs"] = {"file": written, "keys": sorted(legs)}
    pc = legs.get("published_charts") or {}
    summary = {
        "it_per_s": _pick(out, "value"), "estep_frac_of_8TBs": _pick(out, "roofline", "frac"),
        "estep_GBs": _pick(out, "roofline", "achieved"), "fused_kernel_ms": _pick(out, "fused_kernel", "avg_ms"),
        "fused_frac_fp32_peak": _pick(out, "roofline_fused", "frac"),
        "cpu_it_per_s": _pick(out, "cpu_baseline", "value"),
        "bunny_J100_gpu_cpu_it_per_s": [_pick(legs, "bunny", "gpu_it_per_s"), _pick(legs, "bunny", "cpu_it_per_s")],
        "c4_build_ms": _pick(legs, "hgmm", "build_ms"),
        "tree_1M_build_ms_f64_f32pdf": [_pick(legs, "tree_1M", "build_ms"), _pick(legs, "tree_1M", "float32_pdfs", "build_ms")],
        "fullcov_ms_per_it": _pick(legs, "fullcov", "ms_per_iteration"),
        "fullcov_f32_tile_ms_per_it": _pick(legs, "fullcov", "float32_tile", "ms_per_iteration"),
        "predict_ms": _pick(legs, "predict", "kernel_ms"), "mstep_frac": _pick(legs, "materialised_iteration", "roofline", "frac"),
        "kmeans_k800_1M_ms": [_pick(legs, "kmeans_init", "fit_ms_warm"), _pick(legs, "kmeans_init", "seeding_ms_warm")],
        "registration_ms": _pick(legs, "registration", "total_ms"),
        "replica_pairs_per_s": _pick(legs, "replica_pairs", "pairs_per_s"),
        "allreduce_us_world1_rccl_ipc": [_pick(legs, "collective_world1", "rccl", "allreduce_us"),
                                         _pick(legs, "collective_world1", "ipc", "allreduce_us")],
        "chart_fit_100comp_s": {str(r["points"]): round(r["flat_100_components_30_iterations_s"], 4)
                                for r in pc.get("gmm_perf1_fit_seconds", [])},
        "chart_tree_build_s": {str(r["tree_level"]): round(r["build_s"], 4)
                               for r in (pc.get("hgmm_perf_lvls_build_seconds") or {}).get("rows", [])},
        "chart_stream_fps": {str(r["points"]): round(r["fps"], 1)
                             for r in (pc.get("gmm_perf3_stream_fps") or {}).get("rows", [])},
    }
    out["summary"] = {k: v for k, v in summary.items() if v not in (None, {}, [None, None])}
    return out


# ------------------------------------------------------------------------------------------------
class _StdoutGuard:
    """stdout must carry ONE JSON line and nothing else -- and libraries print there (RCCL's version banner at the first
    communicator, five lines through C stdio that surface when the process exits, i.e. BEHIND the JSON line).  While
    the bench runs, file descriptor 1 points at stderr; restore() flushes C stdio into it and puts the real stdout back
    for the one line."""

    def __init__(self):
        self.saved = None
        try:
            if sys.stdout.fileno() == 1:
                sys.stdout.flush()
                self.saved = os.dup(1)
                os.dup2(2, 1)
        except (OSError, ValueError, AttributeError):        # stdout replaced by an in-memory stream (tests)
            self.saved = None

    def restore(self):
        if self.saved is None:
            return
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.saved = None


def rank_main(args):
    guard = _StdoutGuard()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args.gpus = world
    args._world1_comm = False

    import hgmm_amd
    # HGMM_BENCH_DEVICE=<id>: rehearsal of the N > 1 flow on a single-GPU box -- all ranks on one device, joined by the
    #   host shared-memory backend (HGMM_BENCH_HOSTCOMM=<name>, or --collective host) or by the peer exchange
    #   (--collective ipc; RCCL does not accept two ranks on one device).  A flow check, not a measurement.
    hostcomm = os.environ.get("HGMM_BENCH_HOSTCOMM")
    requested = "host" if hostcomm else args.collective
    rehearsal = "HGMM_BENCH_DEVICE" in os.environ and world > 1
    device = int(os.environ["HGMM_BENCH_DEVICE"]) if rehearsal else local_rank
    if not rehearsal:
        # a launcher that narrows every rank's view to its own GPU (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES per rank)
        # leaves LOCAL_RANK beyond the device count: the rank's GPU is then the one it sees
        for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            vis = [v for v in os.environ.get(var, "").split(",") if v.strip()]
            if vis and len(vis) <= local_rank:
                device = local_rank % len(vis)
                break
    ctx = hgmm_amd.Context(device)
    info = ctx.device_info()
    kind, failed_kinds, token, hosts = None, [], "", [socket.gethostname()]
    if world > 1:
        from hgmm_amd import parallel
        # round 0: everybody is there; a job-unique token (names of the shared-memory objects) and the hosts
        mine = ("%s|%s" % (socket.gethostname(), ("%08x" % int.from_bytes(os.urandom(4), "little")) if rank == 0 else "")).encode()
        reports = [r.decode().split("|") for r in parallel.allgather_bytes_tcp(rank, world, mine)]
        token = hostcomm or reports[0][1]
        hosts = sorted(set(r[0] for r in reports))
        order = FALLBACK_ORDER[requested]
        if rehearsal:
            order = [k for k in order if k != "rccl"]
        kind, failed_kinds, ctx = choose_collective(ctx, rank, world, order, token, hosts)
        if kind is None:
            sys.stderr.write("rank %d: no all-reduce backend could be set up on all ranks: %s\n" % (rank, failed_kinds))
            sys.exit(RCCL_INIT_FAILED)
    fallback = bool(failed_kinds) and not rehearsal
    rehearsal_host_only = bool(hostcomm)                  # HGMM_BENCH_HOSTCOMM: the caller asked for the host backend alone

    frame = synth_frame(rank)
    mu0, w0, cov0 = init_params(synth_frame(0) if rank else frame)
    ctx.set_points(frame)

    K, W = args.steps, args.warmup
    full = args.full
    fit = timed_fit(ctx, args, world, (mu0, cov0, w0), profile=full)
    blocks, consistent = fit["blocks"], fit["consistent"]
    inv, mu, w, cov = fit["model"]
    lls = fit["lls"]
    fused_ms, fused_n, ar_ms, ar_n = fit["fused_ms"], fit["fused_n"], fit["ar_ms"], fit["ar_n"]
    if not consistent:
        sys.stderr.write("rank %d: model checksums differ across ranks: max %s min %s\n" % (rank, fit["checksum"], fit["checksum_lo"]))
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"mu": mu, "cov": cov, "w": w, "inv_std": inv, "lls": lls})
    sharded_tree = None
    if full and world > 1 and "sharded_tree" not in args.skip:
        try:                                        # every rank calls it or none does (args.skip is the same everywhere)
            sharded_tree = sharded_tree_leg(ctx, rank, world)
        except Exception as e:
            sharded_tree = {"error": repr(e)}
        ctx.set_points(frame)
    # --collective auto: the same joint fit once more over the one-shot peer exchange, reported beside the RCCL figure
    second = None
    if full and world > 1 and requested == "auto" and kind in ("rccl", "host") and len(hosts) == 1 and not rehearsal_host_only:
        _run_with_timeout(ctx.comm_destroy, 60.0)
        k2, failed2, ctx2 = choose_collective(ctx, rank, world, ["ipc"], token, hosts, round0=8)
        if ctx2 is not ctx:                             # (the peer-exchange attach hung: carry on with the fresh context)
            ctx = ctx2
            ctx.set_points(frame)
        f2 = None
        if k2 == "ipc":
            try:                                    # a side leg on hardware it has never seen must not lose the headline line
                f2 = timed_fit(ctx, args, world, (mu0, cov0, w0), profile=True)
            except Exception as e:                  # (a peer's slice that never arrives fails every rank alike, after ~20 s)
                sys.stderr.write("rank %d: the peer-exchange leg failed: %r\n" % (rank, e))
                second = {"collective": COLLECTIVES["ipc"], "error": "the joint fit failed: %r" % (e,)}
        if f2 is not None:
            med2 = float(np.median(f2["blocks"]))
            same = all(np.array_equal(a, b) for a, b in zip(f2["model"], fit["model"]))
            second = {"collective": COLLECTIVES["ipc"], "value": world * K / med2, "ms_per_step": 1e3 * med2 / K,
                      "allreduce_us": 1e3 * f2["ar_ms"] / max(f2["ar_n"], 1),
                      "identical_model_on_all_ranks": f2["consistent"],
                      "model_bitwise_equal_to_the_headline_fit": bool(same),
                      "max_abs_dmu_vs_the_headline_fit": float(np.abs(f2["model"][1] - fit["model"][1]).max()),
                      "blocks": len(f2["blocks"]),
                      "note": "same frames, same initial parameters, same K-step blocks as `value`; only the all-reduce "
                              "behind the statistics differs (sums in rank order instead of RCCL's reduction order)"}
            consistent = consistent and f2["consistent"]
        elif second is None:
            second = {"collective": COLLECTIVES["ipc"], "error": "could not be set up on every rank: %s" % (failed2,)}
    if world > 1:
        _run_with_timeout(ctx.comm_destroy, 60.0)            # the legs below run on rank 0 alone

    out = None
    if rank == 0:
        med = float(np.median(blocks))
        fused_avg_ms = fused_ms / max(fused_n, 1) if full else None
        collective = COLLECTIVES.get(kind)
        out = {
            "metric": "EM iterations/sec (N points x J components); E-step achieved HBM GB/s",
            "value": world * K / med,
            "unit": "EM it/s (1M-pt x 800-comp frames x iterations per second, all GPUs)",
            "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": 1e3 * med / K,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]/[4]: uniform [0,1)^3 cloud, N=1,000,000 pts per GPU "
                                   "(seed=rank), flat diag GMM J=800 (flavour W), fused device-resident EM, "
                                   "tol=0; N>1: frames are shards of one joint fit, all-reduce of "
                                   "(7J+2) f64 sufficient statistics per iteration",
                       "points_per_gpu": N_POINTS, "components": J_COMP, "cov_type": "diag",
                       "device": info["name"], "compute_units": info["compute_units"],
                       **({"collective": collective, "collective_requested": requested} if collective else {}),
                       **({"rehearsal": "all ranks on ONE device -- flow check, not a measurement"} if rehearsal else {}),
                       **({"fallback": "backend(s) that could not be set up on every rank of this node: %s"
                                       % "; ".join("%s (%s)" % fk for fk in failed_kinds)} if fallback else {})},
            "timing": {"blocks": len(blocks), "steps_per_block": K, "timed_s": float(sum(blocks)),
                       "median_block_ms": med * 1e3, "first_block_it_per_s": world * K / blocks[0],
                       "min_block_it_per_s": world * K / max(blocks), "max_block_it_per_s": world * K / min(blocks),
                       "rule": "value = world x K / median block; every block = K steps between barrier+sync pairs, "
                               "MAX over ranks; one block unless --min-time"},
            "it_per_s_per_gpu": K / med,
            "rank_consistency": {"identical_model_on_all_ranks": fit["consistent"], "checksum": fit["checksum"],
                                 "rule": "sum of the raw 32-bit words of (mu, cov, w, inv_std), plain and position-"
                                         "weighted, all-reduced with max and min over the ranks"},
        }
        if full:
            out["fused_kernel"] = {"avg_ms": fused_avg_ms, "launches": fused_n,
                                   "pairs_per_s": N_POINTS * J_COMP / (fused_avg_ms * 1e-3) if fused_avg_ms else None,
                                   "last_lls": float(lls[-1])}
        if full and world > 1:
            out["allreduce_us"] = 1e3 * ar_ms / max(ar_n, 1)
            out["allreduce_payload_bytes"] = 8 * (7 * 1024 + 2)        # 7 statistics x Jpad(=1024) + sum lpn + n
            out["allreduce_launches"] = ar_n
            if second is not None:
                out["peer_exchange"] = second
            if sharded_tree is not None:
                out["sharded_tree"] = sharded_tree
                out["surplus_collectives"] = sharded_tree.get("surplus_collectives")
        if fused_avg_ms:
            out["roofline_fused"] = fused_roofline(fused_avg_ms * 1e-3, info["compute_units"])
        if not consistent:
            out["error"] = "ranks ended the joint fit with different parameters"

    # ---- --full, rank-0 legs (every N): the materialising E-step's roofline; N = 1: the other hot kernels at their configs ----
    if rank == 0 and full:
        lr = ctx.empty((N_POINTS, J_COMP), np.float32)
        out["roofline"] = estep_roofline_leg(ctx, lr, (mu0, cov0, w0), (inv, mu, w), args)
        if world > 1:
            out["roofline"]["scope"] = "one launch on rank 0's GPU after the joint fit (the kernel is rank-local)"
    if rank == 0 and world == 1 and full:
        # (from the INITIAL parameters, as a caller's own loop starts: inv_cov0 = 1 / sqrt(cov0), gmm_impl.py:122)
        out["materialised_iteration"] = materialised_iteration_leg(ctx, lr, (1.0 / np.sqrt(cov0)).astype(np.float32), mu0, w0)
        out["predict"] = predict_leg(ctx, (inv, mu, w))
        out["estimate_log_prob"] = log_prob_leg(ctx, (inv, mu, w))
        # what a pure 16-byte store stream of the same size reaches on this chip (write ceiling)
        # (best pure-store pattern found, tools/fillbench.py: one workgroup per CU, grid-stride)
        ctx.util_fill(lr, 0.0, False, 0, 1)
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(10):
            ctx.util_fill(lr, 0.0, False, 0, 1)
        ctx.profile_enable(False)
        f_ms, f_n = ctx.profile_get("util_fill")
        out["roofline"]["store_stream_ceiling_GBs"] = 4 * N_POINTS * J_COMP / (f_ms / f_n * 1e-3) / 1e9
        # ... and what the same bytes reach when they are written as 3200-byte ROWS (fillbench mode 5: a workgroup
        # takes 4 consecutive rows per step, its waves split a row): the pattern class the E-step's output is in
        ctx.util_fill(lr, 4.0, False, 5, 1)
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(10):
            ctx.util_fill(lr, 4.0, False, 5, 1)
        ctx.profile_enable(False)
        f_ms, f_n = ctx.profile_get("util_fill")
        out["roofline"]["row_pitch_store_ceiling_GBs"] = 4 * N_POINTS * J_COMP / (f_ms / f_n * 1e-3) / 1e9
        # ... and what a pure store stream reaches when it is OFFERED at a fixed rate like the E-step's rows (fillbench mode 6:
        # the E-step's store pattern without its arithmetic, released by the same StorePacer): the best of three rates around
        # the knee -- the ceiling the paced kernel is up against (un-paced the same stream collapses to ~5.5 TB/s)
        best = 0.0
        for rate in (6600.0, 6800.0, 7000.0):
            for _ in range(3):
                ctx.util_fill(lr, rate, True, 6, 2)
            ctx.profile_reset()
            ctx.profile_enable(True)
            for _ in range(10):
                ctx.util_fill(lr, rate, True, 6, 2)
            ctx.profile_enable(False)
            f_ms, f_n = ctx.profile_get("util_fill")
            best = max(best, 4 * N_POINTS * J_COMP / (f_ms / f_n * 1e-3) / 1e9)
        out["roofline"]["paced_store_stream_ceiling_GBs"] = best
        out["roofline"]["frac_of_paced_store_ceiling"] = out["roofline"]["achieved"] / best
        lr.free()
        for name, leg in (("bunny", bunny_leg), ("hgmm", hgmm_leg), ("tree_1M", tree_1m_leg), ("fullcov", fullcov_leg),
                          ("kmeans_init", kmeans_leg), ("registration", registration_leg),
                          ("published_charts", published_charts_leg), ("replica_pairs", replica_pairs_leg)):
            if name in args.skip:
                continue
            try:
                out[name] = leg(ctx)
            except Exception as e:                                    # a side leg must not lose the headline line
                out[name] = {"error": repr(e)}
    if rank == 0 and world == 1 and full and "collective" not in args.skip:
        try:
            ctx.set_points(frame)
            out["collective_world1"] = collective_world1_leg(ctx, args, (mu0, cov0, w0), out["it_per_s_per_gpu"])
        except Exception as e:
            out["collective_world1"] = {"error": repr(e)}
    if rank == 0:
        if full:
            if not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline_main()
                if world > 1:
                    out["cpu_baseline"]["scope"] = "timed on rank 0's host cores after the joint fit (other ranks idle)"
            else:
                out["cpu_baseline"] = None
            out = split_legs(out, args)
        guard.restore()
        print(json.dumps(out))
        sys.stdout.flush()
        guard = _StdoutGuard()                 # whatever the teardown prints goes to stderr again
    ctx.close()
    if not consistent:
        sys.exit(3)


# ------------------------------------------------------------------------------------------------
# --mode pairs: replica fan-out of INDEPENDENT scan pairs (north_star: "independent scan pairs ... fan out across the
# GPUs"; SURVEY 8e: "Independent scan pairs: no communication ('replicas')")
# ------------------------------------------------------------------------------------------------
PAIR_TARGETS = 16            # distinct perturbed targets a rank cycles through
PAIR_KW = dict(tree_level=3, lambda_c=0.01, ls=20, sig2=0.004)      # the reference GPU file's constants (hgmm_gpu.py:469-477, 687)
PAIR_MAXITER, PAIR_TOL = 20, 1.0e-4                                 # registration_gmmtree's defaults (hgmm_gpu.py:802)


def _quat_rot(q):
    qx, qy, qz, qw = q
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                     [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                     [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])


def scan_pairs(rank, count=PAIR_TARGETS):
    """The rank's scan pairs: source = bun000.ply (40 256 points), target = bun045.ply (40 097 points, another scan of
    the object, ~94 % overlap) placed by its ground-truth pose of the reference's data/bun.conf and then moved by a
    known rigid motion that differs per pair (4-8 deg about a random axis, up to 6 mm; seed = 1000 rank + k).
    -> (source [N,3] f64, [(target [M,3] f64, truth [N,3] f64 = where the source belongs), ...])."""
    g = os.path.join(ROOT, "tests", "golden")
    a = np.load(os.path.join(g, "bun000_xyz.npy")).astype(np.float64)
    b = np.load(os.path.join(g, "bun045_xyz.npy")).astype(np.float64)
    conf = np.load(os.path.join(g, "bun_conf.npz"))
    pose = conf["poses"][list(conf["names"]).index("bun045.ply")]
    world = b @ _quat_rot(pose[3:]) + pose[:3]             # bun.conf convention: p_world = R(q)^T p + t
    out = []
    for k in range(count):
        rs = np.random.RandomState(1000 * rank + k)
        axis = rs.randn(3)
        axis /= np.linalg.norm(axis)
        th = np.deg2rad(rs.uniform(4.0, 8.0))
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        Rd = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        td = rs.uniform(-0.006, 0.006, 3)
        out.append((world @ Rd.T + td, a @ Rd.T + td))
    return a, out


def register_pair(ctx, source, target):
    """ONE unit of work, exactly the reference's call (src/python/hgmm/hgmm_gpu.py:802-807): build the GMM tree of the
    source, register the target against it.  -> (MstepResult, registration iterations)."""
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    gt = GMMTree(source, ctx=ctx, **PAIR_KW)
    res = gt.registration(target, PAIR_MAXITER, PAIR_TOL)
    return res, int(gt.n_iter_)


PHASES = []           # phases_ms of every batched call (list.append is atomic): where a step's wall time went, per thread


def register_batch(ctx, source, targets):
    """B units of work through the same launches (hgmm_amd.hgmm.hgmm_gpu.registration_gmmtree_batch): every pair's tree and
    transformation are bitwise what register_pair returns for it (tests/test_tree_batch_gpu.py).
    -> ([MstepResult ...], [registration iterations ...])."""
    from hgmm_amd.hgmm.hgmm_gpu import registration_gmmtree_batch
    res, info = registration_gmmtree_batch([(source, t) for t in targets], maxiter=PAIR_MAXITER, tol=PAIR_TOL, ctx=ctx,
                                           return_info=True, **PAIR_KW)
    PHASES.append(info.get("phases_ms"))
    return res, info["registration_iters"]


def pairs_cpu_baseline():
    """The oracle (oracle/hgmm_tree.py: the CPU twin's buildGMMTree + GMMTree.registration restated in NumPy) on a
    BOUNDED sample of the same pair: every 8th point of both scans, same constants."""
    from oracle import hgmm_tree
    a, pairs = scan_pairs(0, 1)
    S, Tg = a[::8], pairs[0][0][::8]
    L = PAIR_KW["tree_level"]
    T = hgmm_tree.n_total(L)
    idx = np.random.RandomState(72).randint(T, size=T)
    t0 = time.perf_counter()
    pi, mu, cov, tr = hgmm_tree.build_tree(S, L, float(PAIR_KW["ls"]), 1e-4, idx, PAIR_KW["sig2"], 1000)
    t1 = time.perf_counter()
    _, _, _, trace = hgmm_tree.register(Tg, pi, mu, cov, L, PAIR_KW["lambda_c"], PAIR_MAXITER, PAIR_TOL)
    t2 = time.perf_counter()
    return {"value": 1.0 / (t2 - t0), "unit": "pairs/s on the sample", "cores": 1, "host_cpu_count": os.cpu_count(),
            "kind": "port",
            "sample": "oracle.hgmm_tree.build_tree + register on every 8th point of the pair (%d / %d points), L=3: "
                      "build %.2f s (%s level iterations), registration %.2f s (%d iterations); the cost is linear in "
                      "the points, so the full pair is ~8x this" % (len(S), len(Tg), t1 - t0, list(tr.iters_per_level),
                                                                   t2 - t1, len(trace))}


def pairs_main(args):
    """One process per GPU, NO communicator: every rank registers its own scan pairs on its own context; the ranks only
    meet over plain TCP for the timing barrier and the max-over-ranks block time.  `value` = pairs registered per second
    by all ranks together."""
    guard = _StdoutGuard()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import hgmm_amd
    from hgmm_amd import parallel
    rehearsal = "HGMM_BENCH_DEVICE" in os.environ and world > 1
    device = int(os.environ["HGMM_BENCH_DEVICE"]) if rehearsal else local_rank
    if not rehearsal:
        for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
            vis = [v for v in os.environ.get(var, "").split(",") if v.strip()]
            if vis and len(vis) <= local_rank:
                device = local_rank % len(vis)
                break
    import queue
    import threading
    # C contexts per GPU, each driven by its own thread: a 40 k-point pair is ~120 level-iterations of three small kernels --
    # latency chains that leave most of the chip idle -- so a second pair in flight on the same GPU nearly doubles the
    # rate (hgmm_amd.replicas.ReplicaPool(contexts_per_device=...) is the same thing as a product API)
    C = max(1, int(args.contexts_per_gpu))
    Bt = max(1, int(args.batch))                      # pairs per context and step that share every launch (1: the serial call)
    ctxs = [hgmm_amd.Context(device) for _ in range(C)]
    ctx = ctxs[0]
    info = ctx.device_info()
    group = parallel.TcpGroup(rank, world)
    source, pairs = scan_pairs(rank)
    # The scans ARE float32 (the .ply files; the reference's GPU file also casts, hgmm_gpu.py:472 points.astype(np.float32)):
    # handed over as float32 the mirrors evaluate the build's stop rule in float32 (hgmm_tree_set_precision; tables, E-step,
    # moments and registration stay float64, the trees are the float64 trees bit for bit whenever the iteration counts agree --
    # tests/test_tree_batch_gpu.py); handed over as float64 everything is float64.  --scan-dtype picks what is timed as
    # `value`; the other kind is timed behind it (`other_scan_dtype`).
    kinds = {"float32": (source.astype(np.float32), [t.astype(np.float32) for t, _ in pairs]),
             "float64": (source, [t for t, _ in pairs])}
    active = {"kind": args.scan_dtype}
    K, W = args.steps, args.warmup
    iters, errs, starts, done = [], [], [], []
    last = [None] * C                                 # per context: (pair indices, results, iterations) of its last timed step
    failures = []

    def worker(wi, q_in, q_out):
        c = ctxs[wi]
        step = 0
        try:
            with hgmm_amd.use_context(c):
                while True:
                    n_steps = q_in.get()
                    if n_steps is None:
                        return
                    for _ in range(abs(n_steps)):
                        ks = [(wi + C * (step * Bt + j)) % len(pairs) for j in range(Bt)]
                        src_k, tgt_k = kinds[active["kind"]]
                        if Bt == 1:
                            res, n_it = register_pair(c, src_k, tgt_k[ks[0]])
                            results, n_its = [res], [n_it]
                        else:
                            results, n_its = register_batch(c, src_k, [tgt_k[k] for k in ks])
                        if n_steps > 0 and active["kind"] == args.scan_dtype:   # (negative: warm-up, nothing recorded)
                            iters.extend(n_its)
                            done.extend((r.transformation, k) for r, k in zip(results, ks))    # judged after the timing
                            last[wi] = (ks, results, n_its)
                        step += 1
                    c.synchronize()
                    q_out.put(wi)
        except BaseException as e:                                              # noqa: BLE001 -- the main thread reports it
            failures.append(repr(e))
            q_out.put(wi)

    q_ins = [queue.SimpleQueue() for _ in range(C)]
    q_out = queue.SimpleQueue()
    threads = [threading.Thread(target=worker, args=(wi, q_ins[wi], q_out), daemon=True) for wi in range(C)]
    for t in threads:
        t.start()

    def run_steps(n_steps):
        for q in q_ins:
            q.put(n_steps)
        for _ in range(C):
            q_out.get()
        if failures:
            raise RuntimeError("a replica failed: %s" % failures[0])

    def barrier():
        for c in ctxs:
            c.synchronize()
        group.barrier()

    run_steps(-max(W, 1))
    blocks = []
    while True:
        barrier()
        t0 = time.perf_counter()
        run_steps(K)                                                            # K steps = K pairs on each of the C contexts
        dt_local = time.perf_counter() - t0
        barrier()
        blocks.append(float(group.allgather_f64([dt_local]).max()))          # identical on every rank
        if enough_blocks(blocks, args.min_time):
            break
    if rank == 0 and args.dump_outputs:
        # the transformations (and iteration counts) of the last timed step, context by context, pair by pair
        rows = [(k, r, n) for ks, results, n_its in last for k, r, n in zip(ks, results, n_its)]
        dump_outputs(args.dump_outputs, {"pair_index": [k for k, _, _ in rows],
                                         "rot": [np.asarray(r.transformation.rot, np.float64) for _, r, _ in rows],
                                         "t": [np.asarray(r.transformation.t, np.float64) for _, r, _ in rows],
                                         "registration_iterations": [n for _, _, n in rows]})
    # --full: the other kind of scans, timed the same way (half the time)
    other_kind = "float64" if args.scan_dtype == "float32" else "float32"
    other_blocks = []
    if args.full and not args.no_other_dtype:
        active["kind"] = other_kind
        run_steps(-max(W, 1))
        while True:
            barrier()
            t0 = time.perf_counter()
            run_steps(K)
            dt_local = time.perf_counter() - t0
            barrier()
            other_blocks.append(float(group.allgather_f64([dt_local]).max()))
            if enough_blocks(other_blocks, args.min_time, share=0.5):
                break
        active["kind"] = args.scan_dtype
    for q in q_ins:
        q.put(None)
    for t in threads:
        t.join(30)
    # accuracy of what was timed (the method has no outlier model: on these partially overlapping scans it settles a
    # few millimetres off the ground truth, tests/test_tree_gpu.py::test_registration_real_scan_pair_against_bun_conf);
    # every distinct (pair, transformation) is judged once, outside the timed blocks
    seen = {}
    for tf, k in done:
        key = (k, np.asarray(tf.rot).tobytes(), np.asarray(tf.t).tobytes())
        if key not in seen:
            truth = pairs[k][1]
            seen[key] = (float(np.linalg.norm(tf.transform(source) - truth, axis=1).mean()),
                         float(np.linalg.norm(source - truth, axis=1).mean()))
        errs.append(seen[key][0])
        starts.append(seen[key][1])
    mine = np.array([np.max(errs), np.mean(errs), np.mean(starts), float(np.sum(iters)), float(len(iters))])
    allr = group.allgather_f64(mine)
    ok = bool(allr[:, 0].max() < 0.006)
    # --full: kernel time of one pair under the hipEvent profiler (not part of the timing)
    prof = None
    if args.full:
        ctx.profile_reset()
        ctx.profile_enable(True)
        register_pair(ctx, kinds[args.scan_dtype][0], kinds[args.scan_dtype][1][0])
        ctx.synchronize()
        ctx.profile_enable(False)
        prof = {k: ctx.profile_get(k) for k in ("tree_estep", "tree_loglik", "tree_reg")}
    out = None
    if rank == 0:
        med = float(np.median(blocks))
        n_iter_total, n_pairs = float(allr[:, 3].sum()), float(allr[:, 4].sum())
        out = {
            "metric": "registered scan pairs/sec (registration_gmmtree: GMM-tree build of the source + registration of the target)",
            "value": world * C * K * Bt / med, "unit": "pairs/s (all GPUs)", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": 1e3 * med / K, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f64 (node tables, E-step, moments, registration); f32 pdfs in the build's stop rule (float32 scans: the "
                      "reference GPU file's type, hgmm_gpu.py:472)" if args.scan_dtype == "float32" else "f64"),
            "scan_dtype": args.scan_dtype,
            "other_scan_dtype": ({"scan_dtype": other_kind, "pairs_per_s": world * C * K * Bt / float(np.median(other_blocks)),
                                  "blocks": len(other_blocks)} if other_blocks else None),
            "data": "Stanford bunny scans bun000 / bun045 (tests/golden), poses from the reference's bun.conf",
            "mode": "pairs",
            "config": {"workload": "replicas: every GPU registers its own scan pairs, no communicator -- source bun000.ply "
                                   "(40256 pts), target bun045.ply (40097 pts) placed by bun.conf and moved by a known rigid "
                                   "motion per pair (4-8 deg, <= 6 mm); registration_gmmtree(source, target, maxiter=20, "
                                   "tol=1e-4, tree_level=3, lambda_c=0.01, ls=20, sig2=0.004) = the reference's unit of work "
                                   "(src/python/hgmm/hgmm_gpu.py:802-807); host arrays in, transformation out",
                       "pairs_per_gpu_per_step": C * Bt, "contexts_per_gpu": C, "batch": Bt,
                       "batching": ("registration_gmmtree_batch: %d pairs per context share every launch (forest build in "
                                    "lock-step levels + batched registration, the 6 x 6 solves on the host); results bitwise "
                                    "those of the serial call" % Bt) if Bt > 1 else "none: one registration_gmmtree call per pair",
                       "device": info["name"], "compute_units": info["compute_units"],
                       "parallelism": "replicas x%d GPUs x %d contexts per GPU, one thread each, x %d pairs per launch set "
                                      "(no collective)" % (world, C, Bt),
                       **({"rehearsal": "all ranks on ONE device -- flow check, not a measurement"} if rehearsal else {})},
            "timing": {"blocks": len(blocks), "steps_per_block": K, "timed_s": float(sum(blocks)),
                       "median_block_ms": med * 1e3, "first_block_pairs_per_s": world * C * K * Bt / blocks[0],
                       "rule": "value = world x C x K x batch / median block; a block = K steps (one batch of pairs on each of "
                               "the rank's C contexts, concurrently) between TCP barrier + stream synchronisation on both "
                               "sides, MAX over ranks"},
            "pairs_per_s_per_gpu": C * K * Bt / med,
            "registration_iterations_per_pair": n_iter_total / max(n_pairs, 1),
            "registration_iterations_per_s_per_gpu": (n_iter_total / max(n_pairs, 1)) * C * K * Bt / med,
            "accuracy": {"mean_misalignment_before_mm": 1e3 * float(allr[:, 2].mean()),
                         "mean_misalignment_after_mm": 1e3 * float(allr[:, 1].mean()),
                         "max_misalignment_after_mm": 1e3 * float(allr[:, 0].max()), "bound_mm": 6.0, "ok": ok},
            "kernels_ms_per_pair": {k: {"ms": v[0], "launches": v[1]} for k, v in prof.items()} if prof else None,
            "host_phases_ms_per_batch": ({k: float(np.mean([p[k] for p in PHASES if p])) for k in PHASES[-1]}
                                         if PHASES and PHASES[-1] else None),
            "h2d_note": "every pair's two clouds are uploaded from host arrays through the reference's host-array API (float32 "
                        "scans: 2 x 0.48 MB per pair, widened on the device; float64: 2 x 0.97 MB): `sources_up` + `targets_up` of "
                        "host_phases_ms_per_batch",
            "roofline": None,
            "roofline_note": "latency-bound: ~100 level-iterations of three small kernels per pair on 40 k points "
                             "(SURVEY 8d: 'report wall-time per build, not roofline'); the HBM roofline of the path is "
                             "measured by the default mode's materialising E-step",
        }
        if not ok:
            out["error"] = "a registered pair ended more than 6 mm from its ground truth"
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = pairs_cpu_baseline()
            except Exception as e:
                out["cpu_baseline"] = {"error": repr(e)}
        else:
            out["cpu_baseline"] = None
        guard.restore()
        print(json.dumps(out))
        sys.stdout.flush()
        guard = _StdoutGuard()
    group.barrier()
    group.close()
    for c in ctxs:
        c.close()
    if not ok:
        sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-time", type=float, default=None,
                    help="timed K-step blocks repeat until this many seconds of timed work and three blocks, `value` "
                         "from the median block (default: one block of exactly --steps steps)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the profiled block, rooflines, the side legs, the CPU baseline, the N > 1 "
                         "side fits; --mode pairs: the other scan type, per-pair kernel times, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy")
    ap.add_argument("--mode", default="fit", choices=["fit", "pairs"],
                    help="fit (default): the headline joint EM fit, frames sharded over the GPUs with an all-reduce of the "
                         "sufficient statistics; pairs: independent scan pairs, one registration_gmmtree per GPU and step, "
                         "no communicator")
    ap.add_argument("--contexts-per-gpu", type=int, default=8,
                    help="--mode pairs: engine contexts (and threads) per GPU, each registering its own pairs (default 8)")
    ap.add_argument("--batch", type=int, default=32,
                    help="--mode pairs: pairs every context takes through the SAME launches per step "
                         "(registration_gmmtree_batch; 1 = one registration_gmmtree call per pair, round 5's path)")
    ap.add_argument("--scan-dtype", default="float32", choices=["float32", "float64"],
                    help="--mode pairs: the type the scans are handed over in (float32 = the files' and the reference GPU "
                         "file's type: float32 pdfs in the build's stop rule; float64: float64 throughout)")
    ap.add_argument("--no-other-dtype", action="store_true", help="--mode pairs: skip the timing of the other scan type")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--estep-reps", type=int, default=30)
    ap.add_argument("--skip", default="", help="comma-separated side legs to skip (bunny,hgmm,tree_1M,fullcov,...)")
    ap.add_argument("--collective", default="auto", choices=sorted(FALLBACK_ORDER),
                    help="N > 1: the all-reduce behind the sufficient statistics.  auto (default): `value` over RCCL "
                         "and the same fit once more over the one-shot peer exchange (`peer_exchange`); rccl / ipc / "
                         "host: that backend only.  A backend that cannot be set up on every rank is replaced by the "
                         "next of rccl -> host -> ipc, collectively, and the line says so (config.fallback)")
    args = ap.parse_args()
    args.skip = set(s for s in args.skip.split(",") if s)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args, sys.argv[1:]))
    if args.mode == "pairs":
        pairs_main(args)
    else:
        rank_main(args)


if __name__ == "__main__":
    main()
