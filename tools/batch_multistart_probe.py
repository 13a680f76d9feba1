#!/usr/bin/env python3
"""What K start poses for each of B pairs cost (profiles/tree_batch_multistart.md).  bun000 / bun045 pairs at bench.py's
PAIR_KW (L = 3, 20 iterations, tol 1e-4); every pair has a source of its own -- a seeded subsample of bun000 of ragged size
(30 000 .. 40 000 points; 38 000 .. 40 000 at L = 5), so the trees differ and the lock-step levels last as long as their slowest cloud -- and its own
target (bench.scan_pairs: bun045 placed by its ground-truth pose, moved by 4-8 degrees per pair).  K starts about the
target's centroid: the identity (K = 1), +-10 degrees about two axes with it (5), the 27-start grid.  On ONE context, wall clock
from host arrays to results, median (min - max) of REPS warm repeats:
  (a) registration_gmmtree_batch(pairs, starts=...)          (b) [registration_gmmtree(s, t, starts=...) for s, t in pairs]
  (c) registration_gmmtree_batch(pairs): no starts, the floor
and at the library level the hypotheses grouped by pair (the mirror's order) against interleaved round-robin over the pairs.
    python tools/batch_multistart_probe.py [--quick] [--deep-only]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench            # noqa: E402
import hgmm_amd         # noqa: E402
from hgmm_amd.hgmm.hgmm_gpu import (RigidTransformation, euler_matrix_xyz, registration_gmmtree,  # noqa: E402
                                    registration_gmmtree_batch, rotation_starts)

REPS = 5
MAXITER, TOL = bench.PAIR_MAXITER, bench.PAIR_TOL


def make_pairs(B, fewest=30000):
    """(L = 5: the default initial rows are drawn from the tree's 37 448 node numbers, so a source has at least as many points)"""
    source, targets = bench.scan_pairs(0, count=B)
    rs = np.random.RandomState(7)
    pairs = []
    for b in range(B):
        n = int(rs.randint(fewest, 40001))
        pairs.append((source[np.sort(rs.choice(len(source), n, replace=False))], targets[b][0]))
    return pairs


def starts_for(K, target):
    c = target.mean(axis=0)
    if K == 27:
        return rotation_starts(centre=c)
    rots = [np.identity(3)]
    if K == 5:
        rots += [euler_matrix_xyz(*np.deg2rad(a)) for a in ([10.0, 0, 0], [-10.0, 0, 0], [0, 0, 10.0], [0, 0, -10.0])]
    assert len(rots) == K
    return [RigidTransformation(r, c - r @ c) for r in rots]


def timed(ctx, call, reps=REPS):
    call()
    ctx.synchronize()
    ms, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms), last


def fmt(m, per):
    return "%.2f (%.2f - %.2f)" % (m[0] / per, m[1] / per, m[2] / per)


def case(ctx, B, K, kw):
    pairs = make_pairs(B, 30000 if kw["tree_level"] < 5 else 38000)
    starts = [starts_for(K, t) for _, t in pairs]
    a = timed(ctx, lambda: registration_gmmtree_batch(pairs, MAXITER, TOL, ctx=ctx, starts=starts, return_info=True, **kw))
    b = timed(ctx, lambda: [registration_gmmtree(s, t, MAXITER, TOL, starts=st, ctx=ctx, **kw) for (s, t), st in zip(pairs, starts)])
    c = timed(ctx, lambda: registration_gmmtree_batch(pairs, MAXITER, TOL, ctx=ctx, **kw))
    res, info = a[3]
    same = all(np.array_equal(x.transformation.rot, y.transformation.rot) and np.array_equal(x.transformation.t, y.transformation.t)
               and x.best_index_ == y.best_index_ and x.score[:8] == y.score[:8] for x, y in zip(res, b[3]))
    assert same, "B = %d, K = %d: the batch and the loop of serial calls differ" % (B, K)
    iters = [i for p in info["hypothesis_iters"] for i in p]
    ph = info["phases_ms"]
    print("| %d | %d | %s | %.3f | %s | %.2f | %s | %.1f / %.1f / %.1f / %.1f / %.1f | %d - %d | %.3f |"
          % (B, K, fmt(a, B), a[0] / (B * K), fmt(b, B), b[0] / a[0], fmt(c, B), ph["sources_up"] + ph["prepare"], ph["build"],
             ph["targets_up"], ph["register"], ph["score"] + ph["results"], min(iters), max(iters),
             float(np.mean([r.score.fitness for r in res]))), flush=True)


def order_case(ctx, B, K, L):
    """the library call alone: R = B K hypotheses grouped by pair against round-robin over the pairs (tol = 0: equal work)"""
    pairs = make_pairs(B, 30000 if L < 5 else 38000)
    kw = dict(bench.PAIR_KW, tree_level=L)
    registration_gmmtree_batch(pairs, 1, TOL, ctx=ctx, **kw)                 # (leaves the forest and its targets resident)
    st = [starts_for(K, t) for _, t in pairs]
    rot = np.stack([s.rot for ss in st for s in ss])
    t = np.stack([s.t for ss in st for s in ss])
    grouped = np.repeat(np.arange(B), K)
    perm = np.arange(B * K).reshape(B, K).T.reshape(-1)                      # hypothesis k of every pair, then k + 1
    run = lambda rows: ctx.tree_register_batch_multi(grouped[rows], rot[rows], t[rows], 1.0, kw["lambda_c"], MAXITER, 0.0)
    g = timed(ctx, lambda: run(np.arange(B * K)))
    i = timed(ctx, lambda: run(perm))
    assert np.array_equal(g[3][0][perm], i[3][0]) and np.array_equal(g[3][1][perm], i[3][1])
    print("| %d | %d | %d | %s | %s |" % (L, B, K, fmt(g, 1), fmt(i, 1)), flush=True)


def main():
    quick = "--quick" in sys.argv
    ctx = hgmm_amd.Context(0)
    head = ("| B | K | (a) batch with starts, ms / pair | (a) ms / hypothesis | (b) loop of serial multi-starts, ms / pair | (b) / (a) | "
            "(c) batch without starts, ms / pair | (a) phases, ms per call: up+prepare / build / targets / register / score+results | "
            "iterations | mean fitness |")
    rule = "|" + "---|" * 10
    if "--deep-only" not in sys.argv:
        print("L = %d, %d iterations, tol %g; median (min - max) of %d warm repeats" % (bench.PAIR_KW["tree_level"], MAXITER, TOL, REPS))
        print(head + "\n" + rule)
        for B in ((1, 2) if quick else (1, 8, 32)):
            for K in ((1, 5) if quick else (1, 5, 27)):
                case(ctx, B, K, bench.PAIR_KW)
    print("\nL = 5")
    print(head + "\n" + rule)
    case(ctx, 2 if quick else 8, 5 if quick else 27, dict(bench.PAIR_KW, tree_level=5))
    print("\nhypothesis order, tree_register_batch_multi alone, 20 iterations with tol = 0, ms per call")
    print("| L | B | K | grouped by pair | interleaved |\n|---|---|---|---|---|")
    for L, B, K in (((3, 2, 5),) if quick else ((3, 32, 27), (3, 8, 27), (5, 8, 27))):
        order_case(ctx, B, K, L)
    ctx.close()


if __name__ == "__main__":
    main()
