#!/usr/bin/env python3
"""Wall time of the resident L2 GMMReg cost (hgmm_l2_set_pairs / hgmm_l2_cost, ``RigidCostFunction.evaluate_many``) and of
what is built on it, next to the path every solve took before it -- ``RigidCostFunction(ctx=...)`` called once per
evaluation (hgmm_gauss_transform: three uploads, one launch, a download of partial sums, NumPy) -- in the same process on
the same device:

    python tools/l2_probe.py [--reps 9] [--pairs 32] [--out FILE.md]

  (a) one cost evaluation at J = 30, 100, 800 (random mixtures in the unit cube, sigma = 0.15): R = 1 and R = 27 hypotheses,
      R calls of ``__call__`` against one ``evaluate_many``; ``l2_cost`` alone is the library call without the chain rule
  (b) the 27-start solve of the multi-start scenario (tests/l2_scenario.py): a loop of ``optimise`` against
      ``optimise_multistart`` on SciPy (lock-step threads over ``evaluate_many``) and on the device solver
      (``solver="device"``: hgmm_l2_solve), with the evaluations of its longest hypothesis
  (c) ``registration_gmmreg_batch`` of --pairs pairs of bun000 / bun045 size (tests/golden; pair b's target is bun045 turned
      by b degrees about z) against the loop of ``registration_gmmreg``, each split into the time of the mixture fits and
      the rest (set-up, solve), the batch through both solvers

Every figure is the median of --reps warmed-up calls (minimum - maximum in brackets) of a host clock around calls that end in
a stream synchronisation.  Markdown on stdout (and into --out)."""
import argparse
import io
import os
import sys
import time
import warnings
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--out", default=None)
args = ap.parse_args()
warnings.filterwarnings("ignore")

import hgmm_amd                                                  # noqa: E402
from hgmm_amd.gmmreg_gpu import cost_functions as cf, gmmreg, gmm as ft    # noqa: E402
import l2_scenario as l2s                                        # noqa: E402

ctx = hgmm_amd.default_context()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=args.reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def fmt2(t, unit=1e6):
    return "%.2f (%.2f - %.2f)" % (t[0] * unit, t[1] * unit, t[2] * unit)


def fmt(t, unit=1e6):
    return "%.0f (%.0f - %.0f)" % (t[0] * unit, t[1] * unit, t[2] * unit)


say("# Resident L2 GMMReg cost: measured on %s" % ctx.device_info()["name"].strip())
say()
say("`tools/l2_probe.py --reps %d --pairs %d`; medians of %d warmed-up calls (minimum - maximum)." % (args.reps, args.pairs, args.reps))
say()
say("## (a) one cost evaluation, microseconds")
say()
say("| J | R | R x `__call__` (hgmm_gauss_transform) | one `evaluate_many` | `l2_cost` alone | ratio |")
say("|---|---|---|---|---|---|")
rs = np.random.RandomState(0)
for J in (30, 100, 800):
    mix = (rs.rand(J, 3), 0.1 + rs.rand(J), rs.rand(J, 3), 0.1 + rs.rand(J))
    old, new = cf.RigidCostFunction(ctx=ctx), cf.RigidCostFunction(ctx=ctx)
    new.set_pairs([mix])
    for R in (1, 27):
        thetas = np.concatenate([rs.randn(R, 4), rs.uniform(-0.1, 0.1, (R, 3))], axis=1)
        poses = [new.to_transformation(th) for th in thetas]
        rots, ts = [p.rot for p in poses], [p.t for p in poses]
        t_old = timed(lambda: [old(th, *mix, 0.15) for th in thetas])
        t_new = timed(lambda: new.evaluate_many(thetas, 0, 0.15))
        t_lib = timed(lambda: ctx.l2_cost(np.zeros(R, np.int32), rots, ts, 0.15))
        say("| %d | %d | %s | %s | %s | %.1f |" % (J, R, fmt(t_old), fmt(t_new), fmt(t_lib), t_old[0] / t_new[0]))

say()
say("## (b) the 27-start solve of the scenario (J = 30, opt_maxiter = 10), milliseconds")
say()
sc = l2s.scenario()
mixes = (sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"])
old_reg = l2s.registration(cf.RigidCostFunction(ctx=ctx), sc)
new_reg = l2s.registration(cf.RigidCostFunction(ctx=ctx), sc)
x0s = [cf.theta_from_transformation(s) for s in sc["starts"]]
serial = [old_reg.optimise(*mixes, x0, l2s.OPT_MAXITER, l2s.OPT_TOL) for x0 in x0s]
multi = new_reg.optimise_multistart(*mixes, sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL)
t_old = timed(lambda: [old_reg.optimise(*mixes, x0, l2s.OPT_MAXITER, l2s.OPT_TOL) for x0 in x0s], warm=1)
t_new = timed(lambda: new_reg.optimise_multistart(*mixes, sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL), warm=1)
dev_reg = l2s.registration(cf.RigidCostFunction(ctx=ctx), sc)
dev = dev_reg.optimise_multistart(*mixes, sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL, solver="device")
longest = max(int(r.nfev) for r in dev)
t_dev = timed(lambda: dev_reg.optimise_multistart(*mixes, sc["starts"], l2s.OPT_MAXITER, l2s.OPT_TOL, solver="device"), warm=1)
ids27, sig27 = np.zeros(27, np.int32), np.full(27, sc["sigma"])
t_lib = timed(lambda: ctx.l2_solve(ids27, x0s, sig27, l2s.OPT_MAXITER, l2s.OPT_TOL), warm=1)
say("| path | evaluations | device round trips | ms | winner | degrees from the truth |")
say("|---|---|---|---|---|---|")
best = int(np.argmin([r.fun for r in serial]))
say("| loop of `optimise` | %d | %d | %s | %d | %.1f |" % (
    sum(r.nfev for r in serial), sum(r.nfev for r in serial), fmt(t_old, 1e3), best,
    l2s.angle_deg(old_reg._cost_fn.to_transformation(serial[best].x).rot, sc["truth_rot"])))
say("| `optimise_multistart` | %d | %d | %s | %d | %.1f |" % (
    sum(r.nfev for r in multi), max(r.nfev for r in multi), fmt(t_new, 1e3), new_reg.best_index_,
    l2s.angle_deg(new_reg._cost_fn.to_transformation(multi[new_reg.best_index_].x).rot, sc["truth_rot"])))
say("| `optimise_multistart(solver=\"device\")` | %d | %d evaluations deep, 1 waited for | %s | %d | %.1f |" % (
    sum(r.nfev for r in dev), longest, fmt2(t_dev, 1e3), dev_reg.best_index_,
    l2s.angle_deg(dev_reg._cost_fn.to_transformation(dev[dev_reg.best_index_].x).rot, sc["truth_rot"])))
say("| `Context.l2_solve` alone | %d | %d evaluations deep, 1 waited for | %s | | |" % (sum(r.nfev for r in dev), longest, fmt2(t_lib, 1e3)))
say()
say("Ratios of the medians: loop / SciPy multi-start %.2f, SciPy multi-start / device solver %.1f." % (
    t_old[0] / t_new[0], t_new[0] / t_dev[0]))
say("The device solve: the longest hypothesis takes %d evaluations of two launches each (the host enqueues at most 3 more behind "
    "its end), %.1f microseconds per evaluation of the longest in `Context.l2_solve`; nfev per start %s." % (
        longest, t_lib[0] * 1e6 / longest, [int(r.nfev) for r in dev]))
say("nit and status equal to SciPy's multi-start in %d of 27 starts." % sum(
    (int(a.nit), int(a.status)) == (int(b.nit), int(b.status)) for a, b in zip(dev, multi)))

say()
say("## (c) %d pairs of bun000 / bun045 size, n_gmm_components = 50, milliseconds for all pairs" % args.pairs)
say()
golden = os.path.join(ROOT, "tests", "golden")
src, tgt0 = np.load(os.path.join(golden, "bun000_xyz.npy")).astype(np.float64), np.load(os.path.join(golden, "bun045_xyz.npy")).astype(np.float64)
pairs = []
for b in range(args.pairs):
    a = np.deg2rad(float(b))
    turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    pairs.append((src, tgt0 @ turn.T))
fit_s = [0.0]


def clocked(fn):
    def run(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            fit_s[0] += time.perf_counter() - t0
    return run


ft.GMM_GPU.compute = clocked(ft.GMM_GPU.compute)                  # the loop's fits
ft.GMM_GPU_Base.fit_batch = clocked(ft.GMM_GPU_Base.fit_batch)    # the batch's


def run_split(fn):
    total, fits = [], []
    for k in range(args.reps + 1):
        fit_s[0] = 0.0
        t0 = time.perf_counter()
        with redirect_stdout(io.StringIO()):
            fn()
        if k:                                                       # (the first is the warm-up)
            total.append(time.perf_counter() - t0)
            fits.append(fit_s[0])
    rest = [a - b for a, b in zip(total, fits)]
    return [(float(np.median(v)), float(np.min(v)), float(np.max(v))) for v in (total, fits, rest)]


loop = run_split(lambda: [gmmreg.registration_gmmreg(s, t) for s, t in pairs])
batch = run_split(lambda: gmmreg.registration_gmmreg_batch(pairs))
batch_dev = run_split(lambda: gmmreg.registration_gmmreg_batch(pairs, solver="device"))
say("| path | whole call | mixture fits | the rest (set-up, solve) |")
say("|---|---|---|---|")
say("| loop of `registration_gmmreg` | %s | %s | %s |" % tuple(fmt(t, 1e3) for t in loop))
say("| `registration_gmmreg_batch` | %s | %s | %s |" % tuple(fmt(t, 1e3) for t in batch))
say("| `registration_gmmreg_batch(solver=\"device\")` | %s | %s | %s |" % tuple(fmt(t, 1e3) for t in batch_dev))
say()
say("Ratios of the medians: whole %.2f, fits %.2f, rest %.2f." % tuple(a[0] / b[0] for a, b in zip(loop, batch)))
say("SciPy batch / device batch: whole %.2f, fits %.2f, rest %.2f." % tuple(a[0] / b[0] for a, b in zip(batch, batch_dev)))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
