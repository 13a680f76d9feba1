#!/usr/bin/env python3
"""What per-point weights of the SOURCE cloud (hgmm_tree_set_source_weights) cost and buy -> profiles/tree_source_weights.md.

    python tools/source_weights_probe.py [--out FILE] [--parent-lib LIB] [--parent-tree DIR] [--reps N]
                                         [--skip-gpu] [--skip-pairs] [--skip-buys]

ISA (no GPU needed): instructions, VGPRs (+ AGPRs), SGPRs, LDS and scratch of the E-step, log-likelihood and partition kernels
of the build, read from the gfx950 code object (tools/isa_count.py's disassembly + the code object's metadata notes), the
weighted instantiations beside the unweighted ones and, with ``--parent-lib``, beside the same kernels of the parent
commit's library.

The unweighted path did not move / what weights cost: wall time of hgmm_tree_build (the call ends in a synchronisation)
through the C ABI -- so that the parent's library, which lacks the new entries, runs the very same driver code -- of the C4
build (bun000, 40 256 points, L = 4, ls = 20) and of a 10^6-point L = 4 build (ls = 80, sig2 = 0.00034, bench.py's), one
child process per library and setting, the settings alternating, ``--reps`` repetitions after two warm-up builds each:
median and min .. max.  Settings: the parent's library, this commit's without weights, this commit's with w == 1 resident
(the WEIGHTED kernels; bitwise the unweighted tree).  Per launch: the profiler's hipEvent time (hgmm_profile_*) of the
tree_estep and tree_loglik launch brackets.  ``--parent-tree``: ``bench.py --mode pairs`` in both trees, alternating.

What weights buy: the bun000 <- bun045 pair (tools/gate_probe.py: bun045 at its bun_conf.npz placement, moved by 8 deg / 5 mm)
at bench.py's pairs settings (L = 3, lambda_c = 0.01, ls = 20, sig2 = 0.004; maxiter 30, tol 1e-6), both scans reduced to 4 mm
and to 8 mm voxel centroids; the source tree built with and without the counts, the target registered with and without:
mean distance (mm) of the full moved scan at the resulting pose from its place at the full-scan pose and from its ground-truth
placement, and the build's wall time beside the full scan's."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_count                                                     # noqa: E402

PKG = "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd"
LIB = os.path.join(ROOT, PKG, "libhgmm_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
K_TREE_ESTEP, K_TREE_LOGLIK = 3, 4                                   # include/hgmm.h: HGMM_K_TREE_ESTEP, HGMM_K_TREE_LOGLIK
KERNELS = re.compile(r"tree_estep_kernel|tree_loglik|tree_ll_estep|forest_estep|forest_ll_estep|scatter_kernel")


# ---- ISA ------------------------------------------------------------------------------------------------------------------
def code_object_notes(lib):
    """-> {mangled kernel: {vgpr_count, agpr_count, sgpr_count, group_segment_fixed_size, private_segment_fixed_size}}"""
    tmp = tempfile.mkdtemp(prefix="hgmm_notes_")
    out = {}
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], check=True, capture_output=True, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)], check=True,
                                 capture_output=True, text=True).stdout
            cur = {}
            for line in txt.split("\n"):
                m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip()
                if k == "agpr_count":                                 # (the first key of a kernel's entry)
                    if "name" in cur:
                        out[cur["name"]] = cur
                    cur = {}
                if k in ("agpr_count", "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size"):
                    cur[k] = int(v)
                if k == "name" and v.startswith("_Z"):
                    cur["name"] = v
            if "name" in cur:
                out[cur["name"]] = cur
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def isa_rows(lib):
    """-> {short kernel name: (instructions, vgpr, agpr, sgpr, lds bytes, scratch bytes)}"""
    notes, dis = code_object_notes(lib), isa_count.disassemble(lib)
    names = [k for k in notes if KERNELS.search(k)]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = {}
    for k, d in zip(names, dem):
        short = re.sub(r"\(.*", "", d).replace("hgmm::", "").replace("void ", "")
        n = notes[k]
        rows[short] = (len(dis.get(k, [])), n.get("vgpr_count"), n.get("agpr_count"), n.get("sgpr_count"),
                       n.get("group_segment_fixed_size"), n.get("private_segment_fixed_size"))
    return rows


def isa_table(parent_lib=None):
    cur = isa_rows(LIB)
    par = isa_rows(parent_lib) if parent_lib else {}
    parent_of = lambda s: par.get(s) or par.get(s.replace(", false>", ">")) or par.get(re.sub(r"<false>$", "", s))
    lines = ["| kernel | instructions | VGPR + AGPR | SGPR | LDS B | scratch B | parent: instructions / VGPR + AGPR / SGPR / LDS |",
             "|---|---|---|---|---|---|---|"]
    for s in sorted(cur):
        i, v, a, sg, lds, scr = cur[s]
        p = parent_of(s)
        ptxt = "%d / %d + %d / %d / %d" % (p[0], p[1], p[2], p[3], p[4]) if p else "--"
        lines.append("| `%s` | %d | %d + %d | %d | %d | %d | %s |" % (s, i, v, a, sg, lds, scr, ptxt))
    return "\n".join(lines)


# ---- timing through the C ABI (one child process per library and setting) -------------------------------------------------
def workloads():
    bunny = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    rs = np.random.RandomState(0)
    uni = rs.rand(1000000, 3)                                         # bench.py's uniform million
    out = []
    for name, P, L, ls, sig2 in (("C4: bun000, 40 256 points, L = 4", bunny, 4, 20.0, 0.004),
                                 ("uniform 10^6 points, L = 4", uni, 4, 80.0, 0.00034)):
        T = 8 * (8 ** L - 1) // 7
        out.append((name, np.ascontiguousarray(P), L, ls, sig2, np.ascontiguousarray(P[np.random.RandomState(72).randint(T, size=T)])))
    return out


def child(lib_path, weighted, reps):
    """runs in a process of its own: -> JSON {workload: {wall_ms: [...], estep_us, loglik_us, iters}}"""
    lib = C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    vp, dp = C.c_void_p, C.c_void_p
    lib.hgmm_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.hgmm_destroy.argtypes = [vp]
    lib.hgmm_last_error.argtypes, lib.hgmm_last_error.restype = [vp], C.c_char_p
    lib.hgmm_set_points_f64.argtypes = [vp, dp, C.c_int64]
    lib.hgmm_tree_build.argtypes = [vp, C.c_int, C.c_double, C.c_double, dp, C.c_double, C.c_int, dp, dp, dp, dp, dp, dp, C.c_int, dp]
    lib.hgmm_profile_enable.argtypes = [vp, C.c_int]
    lib.hgmm_profile_reset.argtypes = [vp]
    lib.hgmm_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    h = vp()

    def ok(rc):
        if rc != 0:
            raise RuntimeError("hgmm call failed (%d): %s" % (rc, lib.hgmm_last_error(h)))
    ok(lib.hgmm_create(0, C.byref(h)))
    res = {}
    for name, P, L, ls, sig2, init_mu in workloads():
        T = len(init_mu)
        ok(lib.hgmm_set_points_f64(h, P.ctypes.data, len(P)))
        if weighted:
            lib.hgmm_tree_set_source_weights.argtypes = [vp, dp, C.c_int64]
            w = np.ones(len(P))
            ok(lib.hgmm_tree_set_source_weights(h, w.ctypes.data, len(P)))
        pi, mu, cov, iters = np.empty(T), np.empty((T, 3)), np.empty((T, 9)), np.zeros(L, np.int32)

        def run():
            t0 = time.perf_counter()
            ok(lib.hgmm_tree_build(h, L, ls, 1e-4, init_mu.ctypes.data, sig2, 1000, pi.ctypes.data, mu.ctypes.data,
                                   cov.ctypes.data, None, iters.ctypes.data, None, 0, None))
            return 1e3 * (time.perf_counter() - t0)
        run(), run()
        wall = [run() for _ in range(reps)]
        # per launch, in a build of its own: the profiler's events slow the host down
        ok(lib.hgmm_profile_reset(h))
        ok(lib.hgmm_profile_enable(h, 1))
        run()
        ok(lib.hgmm_profile_enable(h, 0))
        per = {}
        for key, kid in (("estep_us", K_TREE_ESTEP), ("loglik_us", K_TREE_LOGLIK)):
            ms, n = C.c_double(), C.c_int64()
            ok(lib.hgmm_profile_get(h, kid, C.byref(ms), C.byref(n)))
            per[key] = 1e3 * ms.value / max(n.value, 1)
            per[key.replace("_us", "_launches")] = int(n.value)
        res[name] = dict(wall_ms=wall, iters=[int(v) for v in iters], pi_sum=float(pi[:8].sum()), **per)
    lib.hgmm_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib_path, weighted, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, "1" if weighted else "0", str(reps)],
                         capture_output=True, text=True, timeout=300)
    for line in out.stdout.split("\n"):
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError("child failed (%d):\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-2000:]))


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (np.median(v), min(v), max(v))


def cost_section(parent_lib, reps, rounds=2):
    settings = ([("parent commit", parent_lib, False)] if parent_lib else []) + \
               [("this commit, no weights", LIB, False), ("this commit, w == 1 resident", LIB, True)]
    acc = {}
    for _ in range(rounds):                                           # (alternating: drift shows between the rounds)
        for label, lib, weighted in settings:
            r = run_child(lib, weighted, reps)
            for wl, d in r.items():
                a = acc.setdefault(wl, {}).setdefault(label, {"wall_ms": [], "estep_us": [], "loglik_us": [], "iters": d["iters"],
                                                              "launches": (d["estep_launches"], d["loglik_launches"])})
                a["wall_ms"] += d["wall_ms"]
                a["estep_us"].append(d["estep_us"])
                a["loglik_us"].append(d["loglik_us"])
                assert a["iters"] == d["iters"], (wl, label)
    lines = []
    for wl, by in acc.items():
        lines += ["", "**%s** (%d builds per setting in %d processes; iterations per level %s)" %
                  (wl, rounds * reps, rounds, next(iter(by.values()))["iters"]), "",
                  "| setting | build wall ms: median (min .. max) | tree_estep bracket us / launch | tree_loglik bracket us / launch |",
                  "|---|---|---|---|"]
        for label, a in by.items():
            lines.append("| %s | %s | %s | %s |" % (label, spread(a["wall_ms"]), ", ".join("%.2f" % v for v in a["estep_us"]),
                                                   ", ".join("%.2f" % v for v in a["loglik_us"])))
        assert len({tuple(a["iters"]) for a in by.values()}) == 1, "the settings must run the same iterations"
    return "\n".join(lines)


def pairs_section(parent_tree, reps):
    trees = [("parent commit", parent_tree), ("this commit", ROOT)]
    vals = {k: [] for k, _ in trees}
    for _ in range(reps):
        for label, tree in trees:
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--mode", "pairs", "--steps", "8", "--warmup", "2",
                                  "--no-cpu-baseline", "--no-other-dtype"], cwd=tree, capture_output=True, text=True, timeout=240)
            line = [l for l in out.stdout.split("\n") if l.startswith("{")]
            if not line:
                raise RuntimeError("bench.py --mode pairs failed in %s:\n%s" % (tree, out.stderr[-2000:]))
            vals[label].append(float(json.loads(line[-1])["value"]))
    lines = ["", "**`bench.py --gpus 1 --mode pairs --steps 8 --warmup 2`** (%d runs per tree, alternating)" % reps, "",
             "| tree | pairs / s: median (min .. max) |", "|---|---|"]
    for label, _ in trees:
        lines.append("| %s | %s |" % (label, spread(vals[label])))
    return "\n".join(lines)


# ---- what weights buy -----------------------------------------------------------------------------------------------------
def buys_section():
    import hgmm_amd
    from gate_probe import LC, error_mm, scan_pair
    from hgmm_amd.hgmm.hgmm_gpu import GMMTree
    from hgmm_amd.pointcloud_io import voxel_down_sample
    ctx = hgmm_amd.Context(0)
    a, world, moved = scan_pair()
    kw = dict(tree_level=3, lambda_c=LC, ls=20, sig2=0.004, ctx=ctx)

    def pose(src, sw, tgt, tw):
        GMMTree(src, source_weights=sw, **kw)                         # (warm-up)
        t0 = time.perf_counter()
        gt = GMMTree(src, source_weights=sw, **kw)
        build_ms = 1e3 * (time.perf_counter() - t0)
        tf = gt.registration(tgt, 30, 1e-6, weights=tw).transformation.inverse()
        return (np.asarray(tf.rot), np.asarray(tf.t)), build_ms

    def dist(p, q):
        return 1e3 * np.linalg.norm((moved @ p[0].T + p[1]) - (moved @ q[0].T + q[1]), axis=1).mean()
    full, full_ms = pose(a, None, moved, None)
    lines = ["", "Full scans (%d <- %d points): %.2f mm from the ground-truth placement; GMMTree build (upload + build + download) "
             "%.2f ms." % (len(a), len(moved), error_mm(moved, world, *full), full_ms), "",
             "| voxel | source / target points | source tree | target | mm to the full-scan pose | mm to the ground truth | build ms |",
             "|---|---|---|---|---|---|---|"]
    for mm in (4, 8):
        sc, sn = voxel_down_sample(a, 1e-3 * mm, return_counts=True)
        tc, tn = voxel_down_sample(moved, 1e-3 * mm, return_counts=True)
        for sw in (None, sn):
            for tw in (None, tn):
                p, ms = pose(sc, sw, tc, tw)
                lines.append("| %d mm | %d / %d | %s | %s | %.2f | %.2f | %.2f |" %
                             (mm, len(sc), len(tc), "counts" if sw is not None else "unweighted",
                              "counts" if tw is not None else "unweighted", dist(p, full), error_mm(moved, world, *p), ms))
    ctx.close()
    return "\n".join(lines)


def main():
    if "--child" in sys.argv:
        k = sys.argv.index("--child")
        return child(sys.argv[k + 1], sys.argv[k + 2] == "1", int(sys.argv[k + 3]))
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    out_path = arg("--out", os.path.join(ROOT, "profiles", "tree_source_weights.md"))
    parent_lib, parent_tree, reps = arg("--parent-lib"), arg("--parent-tree"), int(arg("--reps", "5"))
    parts = ["# What per-point weights of the source cloud cost and buy (`hgmm_tree_set_source_weights`)", "",
             "Written by `tools/source_weights_probe.py`.", "", "## Code objects (gfx950)", "", isa_table(parent_lib)]
    if "--skip-gpu" not in sys.argv:
        parts += ["", "## The unweighted path against the parent, and what resident weights cost", cost_section(parent_lib, reps)]
        if parent_tree and "--skip-pairs" not in sys.argv:
            parts.append(pairs_section(parent_tree, reps))
        if "--skip-buys" not in sys.argv:
            parts += ["", "## What weights buy: bun000 <- bun045, both scans reduced to voxel centroids", buys_section()]
    text = "\n".join(parts) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
