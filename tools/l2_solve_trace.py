#!/usr/bin/env python3
"""The launches of the device L2 solve (hgmm_l2_solve) for a kernel trace: the 27-start solve of the multi-start scenario
(tests/l2_scenario.py, J = 30, opt_maxiter = 10), two warm-up calls and then [reps] more:
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o kt -- python tools/l2_solve_trace.py [reps]
    python tools/trace_summary.py <dir>
l2_solve_step_kernel's row is the step kernel's own time (one wave per hypothesis; lane 0 runs the serial part);
l2_solve_cost_kernel's the fused cost over the trial poses.  Both include the launches behind a hypothesis' end, whose
workgroups return at their first load."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hgmm_amd                                                  # noqa: E402
from hgmm_amd.gmmreg_gpu import cost_functions as cf             # noqa: E402
import l2_scenario as l2s                                        # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ctx = hgmm_amd.default_context()
sc = l2s.scenario()
ctx.l2_set_pairs([(sc["mu_s"], sc["phi_s"], sc["mu_t"], sc["phi_t"])])
x0s = np.stack([cf.theta_from_transformation(s) for s in sc["starts"]])
for _ in range(2 + reps):
    out = ctx.l2_solve(np.zeros(27, np.int32), x0s, sc["sigma"], l2s.OPT_MAXITER, l2s.OPT_TOL)
print("%d solves of 27 starts; nfev: sum %d, longest %d; accepted steps (nit): sum %d" % (
    2 + reps, int(out[4].sum()), int(out[4].max()), int(out[3].sum())))
