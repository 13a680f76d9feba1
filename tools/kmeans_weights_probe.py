#!/usr/bin/env python3
"""What per-point weights of the KMeans initialiser cost and buy (profiles/kmeans_weights.md).

    python tools/kmeans_weights_probe.py buys            bun000, 4 mm centroids, k = 100: the full scan's inertia under the
                                                         centres of (a) its own fit, (b) the count-weighted centroid fit,
                                                         (c) the unweighted centroid fit -- device and CPU restatement
    python tools/kmeans_weights_probe.py cost [--rounds R]
                                                         N = 10^6, k = 800: seeding ms per centre and Lloyd ms per iteration,
                                                         unweighted and weighted entries interleaved in one process
    python tools/kmeans_weights_probe.py plain --root DIR [--rounds R]
                                                         the unweighted entries alone, of the tree at DIR (a checkout of the
                                                         parent commit with its library built): the figure to hold `cost`'s
                                                         unweighted rows against
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _voxel_centroids(P, size):
    key = np.floor((P - P.min(axis=0)) / size).astype(np.int64)
    _, inv, counts = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    sums = np.zeros((len(counts), 3))
    np.add.at(sums, inv.reshape(-1), P)
    return sums / counts[:, None], counts.astype(np.float64)


def _inertia(P, centres):
    best = np.full(len(P), np.inf)
    for a in range(0, len(centres), 50):
        d = ((P[:, None, :] - centres[None, a:a + 50, :]) ** 2).sum(axis=2)
        best = np.minimum(best, d.min(axis=1))
    return float(best.sum())


def buys(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    P = np.load(os.path.join(ROOT, "tests", "golden", "bun000_xyz.npy")).astype(np.float64)
    C, cnt = _voxel_centroids(P, 0.004)
    k = 100
    print("bun000: %d points -> %d centroids of 4 mm voxels (counts %d .. %d), k = %d" % (len(P), len(C), cnt.min(),
                                                                                         cnt.max(), k))
    rows = []
    if not args.cpu_only:
        import hgmm_amd
        from hgmm_amd.kmeans import KMeans
        ctx = hgmm_amd.Context(0)
        mk = lambda: KMeans(n_clusters=k, random_state=1, max_iter=50, n_init=1, ctx=ctx)     # noqa: E731
        rows.append(("device", mk().fit(P).cluster_centers_, mk().fit(C, sample_weight=cnt).cluster_centers_,
                     mk().fit(C).cluster_centers_))
    from oracle import kmeans as okm
    import _kmeans_weight_oracle as W
    rows.append(("CPU restatement", okm.fit(P, k)["cluster_centers_"], W.fit_w(C, cnt, k)["cluster_centers_"],
                 okm.fit(C, k)["cluster_centers_"]))
    print("| side | (a) full scan's own fit | (b) count-weighted centroids | (c) unweighted centroids | (b) recovers |")
    print("|---|---|---|---|---|")
    for side, a, b, c in rows:
        ia, ib, ic = _inertia(P, a), _inertia(P, b), _inertia(P, c)
        print("| %s | %.6f | %.6f | %.6f | %.0f %% of (c) - (a) |" % (side, ia, ib, ic, 100 * (ic - ib) / (ic - ia)))


def _time_round(ctx, k, first, rand, centres, weighted, iters=10):
    kw = {"weighted": True} if weighted else {}
    t0 = time.perf_counter()
    ctx.kmeans_plusplus(k, first, rand, **kw)
    t_seed = time.perf_counter() - t0
    c = centres.copy()
    t0 = time.perf_counter()
    _, n_iter, _, _ = ctx.kmeans_lloyd(c, iters, 0.0, **kw)
    t_lloyd = (time.perf_counter() - t0) / max(n_iter, 1)
    return t_seed * 1e3 / k, t_lloyd * 1e3


def _fmt(v):
    v = np.asarray(v)
    return "%.4f (%.4f .. %.4f)" % (np.median(v), v.min(), v.max())


def cost(args, plain_only=False):
    sys.path.insert(0, args.root or ROOT)
    import hgmm_amd
    from hgmm_amd.kmeans import KMeans
    n, k = 1_000_000, 800
    rs = np.random.RandomState(0)
    X = rs.rand(n, 3)
    Xc = X - X.mean(axis=0)
    w = rs.randint(1, 40, n).astype(np.float64)
    ru = np.random.RandomState(1)
    first = int(ru.randint(n))
    rand = ru.uniform(size=(k - 1, 2 + int(np.log(k))))
    ctx = hgmm_amd.Context(0)
    ctx.set_points(Xc)
    if not plain_only:
        ctx.tree_set_source_weights(w)
    settings = [False] if plain_only else [False, True]
    centres = {}
    for s in settings:                                       # warm-up, and the start of the Lloyd iterations
        centres[s] = ctx.kmeans_plusplus(k, first, rand, **({"weighted": True} if s else {}))[1]
        _time_round(ctx, k, first, rand, centres[s], s)
    res = {s: [] for s in settings}
    for _ in range(args.rounds):
        for s in settings:
            res[s].append(_time_round(ctx, k, first, rand, centres[s], s))
    fits = {s: [] for s in settings}
    for _ in range(3):
        for s in settings:
            t0 = time.perf_counter()
            km = KMeans(n_clusters=k, random_state=1, max_iter=50, n_init=1, ctx=ctx)
            km.fit(X, sample_weight=w) if s else km.fit(X)
            fits[s].append((time.perf_counter() - t0) * 1e3)
    print("uniform 10^6 points, k = %d, %d rounds%s; median (min .. max)" % (k, args.rounds,
                                                                           ", tree %s" % args.root if args.root else ""))
    print("| entries | seeding ms / centre | Lloyd ms / iteration (10 iterations) | whole fit ms (3 fits) |")
    print("|---|---|---|---|")
    for s in settings:
        a = np.array(res[s])
        print("| %s | %s | %s | %s |" % ("weighted, counts 1..39" if s else "unweighted", _fmt(a[:, 0]), _fmt(a[:, 1]),
                                         _fmt(fits[s])))
    if not plain_only:
        a, b = np.array(res[False]), np.array(res[True])
        print("weighted against unweighted: seeding %+.1f %%, Lloyd %+.1f %%, fit %+.1f %%"
              % (100 * (np.median(b[:, 0]) / np.median(a[:, 0]) - 1), 100 * (np.median(b[:, 1]) / np.median(a[:, 1]) - 1),
                 100 * (np.median(fits[True]) / np.median(fits[False]) - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["buys", "cost", "plain"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--root", default=None)
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    if args.what == "buys":
        buys(args)
    else:
        cost(args, plain_only=args.what == "plain")


if __name__ == "__main__":
    main()
