#!/usr/bin/env python3
"""What per-point weights of the flat full-covariance fit (hgmm_fullcov_fit_weighted) cost and buy -> profiles/fullcov_weights.md.

    python tools/fullcov_weights_probe.py [--out FILE] [--parent-lib LIB] [--parent-tree DIR] [--reps N]
                                          [--skip-gpu] [--skip-bench] [--skip-buys]

ISA (no GPU needed): instructions, VGPRs (+ AGPRs), SGPRs, spills, LDS and scratch of the full-covariance E-step kernels, read
from the gfx950 code object (tools/isa_count.py's disassembly + the code object's metadata notes), the weighted kernels beside
the unweighted ones and, with ``--parent-lib``, beside the same kernels of the parent commit's library.

What weights buy: bun000 (40 256 points) reduced to 4 mm voxel centroids with their counts; the flat full-covariance fit at
J = 16 and J = 100 of the centroids under the counts, of the centroids alone and of the full scan, all three from the same
initial coordinates (J of the centroids): max |d pi| and max |d mu| of either centroid model against the full-scan model, and
the mean log-density of the FULL scan under each of the three models (hgmm_fullcov_estep's q / N).

What weights cost: the profiler's hipEvent time (hgmm_profile_*) per launch of the HGMM_K_FULL_FUSED / HGMM_K_FULL_PASS /
HGMM_K_FULL_MOMENTS brackets through the C ABI -- so that the parent's library, which lacks the new entries, runs the same
driver code -- at N = 10^6 (uniform), J = 800 and at bun000 size, J = 800, in both precisions and on the two-pass path, one
child process per library and setting, the settings alternating, ``--reps`` fits of 4 iterations each after a warm-up fit:
median and min .. max.  Settings: the parent's library, this commit's unweighted entry, this commit's weighted entry with
w == 1 resident (bitwise the unweighted fit).  Per wave of one workgroup: the phase clocks (hgmm_fullcov_phase_clocks) of the
float64 kernel at 10^6 x 800, weighted beside unweighted.  ``--parent-tree``: ``bench.py --gpus 1`` in both trees, alternating."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_count                                                     # noqa: E402
from source_weights_probe import code_object_notes, spread          # noqa: E402

PKG = "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd"
LIB = os.path.join(ROOT, PKG, "libhgmm_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K_FULL_PASS, K_FULL_MOMENTS, K_FULL_FUSED = 7, 8, 12                  # include/hgmm.h: HGMM_K_FULL_*
KERNELS = re.compile(r"full_(fused|pass|moments)")
ITERS = 4


# ---- ISA ------------------------------------------------------------------------------------------------------------------
def spill_counts(lib):
    """-> {mangled kernel: (sgpr spills, vgpr spills)} from the code object's notes"""
    import shutil
    import tempfile
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    tmp = tempfile.mkdtemp(prefix="hgmm_notes_")
    out = {}
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], check=True, capture_output=True, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            txt = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp, f)], check=True,
                                 capture_output=True, text=True).stdout
            for block in txt.split(".agpr_count:")[1:]:
                name = re.search(r"\.name:\s*(_Z\S+)", block)
                sg, vg = re.search(r"\.sgpr_spill_count:\s*(\d+)", block), re.search(r"\.vgpr_spill_count:\s*(\d+)", block)
                if name:
                    out[name.group(1)] = (int(sg.group(1)) if sg else 0, int(vg.group(1)) if vg else 0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def isa_rows(lib):
    notes, dis, spills = code_object_notes(lib), isa_count.disassemble(lib), spill_counts(lib)
    names = [k for k in notes if KERNELS.search(k)]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = {}
    for k, d in zip(names, dem):
        short = re.sub(r"\(.*", "", d).replace("hgmm::", "").replace("void ", "")
        n = notes[k]
        rows[short] = (len(dis.get(k, [])), n.get("vgpr_count"), n.get("agpr_count"), n.get("sgpr_count"), spills.get(k, (0, 0)),
                       n.get("group_segment_fixed_size"), n.get("private_segment_fixed_size"))
    return rows


def isa_table(parent_lib=None):
    cur = isa_rows(LIB)
    par = isa_rows(parent_lib) if parent_lib else {}
    lines = ["| kernel | instructions | VGPR + AGPR | SGPR | spilled SGPR / VGPR | static LDS B | scratch B | parent: instructions / VGPR / SGPR / scratch |",
             "|---|---|---|---|---|---|---|---|"]
    for s in sorted(cur):
        i, v, a, sg, (ss, vs), lds, scr = cur[s]
        p = par.get(s)
        ptxt = "%d / %d / %d / %d" % (p[0], p[1], p[3], p[6]) if p else "--"
        lines.append("| `%s` | %d | %d + %d | %d | %d / %d | %d | %d | %s |" % (s, i, v, a, sg, ss, vs, lds, scr, ptxt))
    return "\n".join(lines)


# ---- timing through the C ABI (one child process per library and setting) -------------------------------------------------
def workloads():
    bunny = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    uni = np.random.RandomState(0).rand(1000000, 3)                   # bench.py's uniform million
    out = []
    for name, P in (("uniform 10^6 points, J = 800", uni), ("bun000, 40 256 points, J = 800", bunny)):
        idx = np.random.RandomState(800).choice(len(P), 800, replace=False)
        out.append((name, np.ascontiguousarray(P), 800, np.ascontiguousarray(P[idx])))
    return out


def child(lib_path, weighted, reps):
    """runs in a process of its own: -> JSON {workload: {path: {us: [...] per launch, launches, q}}, clocks}"""
    lib = C.CDLL(lib_path, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    lib.hgmm_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.hgmm_destroy.argtypes = [vp]
    lib.hgmm_last_error.argtypes, lib.hgmm_last_error.restype = [vp], C.c_char_p
    lib.hgmm_set_points_f64.argtypes = [vp, vp, C.c_int64]
    fit = lib.hgmm_fullcov_fit_weighted if weighted else lib.hgmm_fullcov_fit
    fit.argtypes = [vp, C.c_int, C.c_double, C.c_double, vp, C.c_double, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    lib.hgmm_tree_set_precision.argtypes = [vp, C.c_int]
    lib.hgmm_config_set.argtypes = [vp, C.c_char_p, C.c_int]
    lib.hgmm_profile_enable.argtypes = [vp, C.c_int]
    lib.hgmm_profile_reset.argtypes = [vp]
    lib.hgmm_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.hgmm_fullcov_phase_clocks.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    h = vp()

    def ok(rc):
        if rc != 0:
            raise RuntimeError("hgmm call failed (%d): %s" % (rc, lib.hgmm_last_error(h)))
    ok(lib.hgmm_create(0, C.byref(h)))
    res = {}
    for name, P, J, init_mu in workloads():
        ok(lib.hgmm_set_points_f64(h, P.ctypes.data, len(P)))
        if weighted:
            lib.hgmm_tree_set_source_weights.argtypes = [vp, vp, C.c_int64]
            w = np.ones(len(P))
            ok(lib.hgmm_tree_set_source_weights(h, w.ctypes.data, len(P)))
        pi, mu, cov, q = np.empty(J), np.empty((J, 3)), np.empty((J, 9)), np.zeros(ITERS)
        qlen = C.c_int()

        def run():
            ok(fit(h, J, 1e-30, 1e-4, init_mu.ctypes.data, 0.00034, ITERS, pi.ctypes.data, mu.ctypes.data, cov.ctypes.data,
                   None, q.ctypes.data, ITERS, C.byref(qlen)))
        by_path = {}
        for path, prec, two, kids in (("float64 one-pass", 0, 0, (K_FULL_FUSED,)), ("float32 tile", 1, 0, (K_FULL_FUSED,)),
                                      ("float64 two-pass", 0, 1, (K_FULL_PASS, K_FULL_MOMENTS))):
            ok(lib.hgmm_tree_set_precision(h, prec))
            ok(lib.hgmm_config_set(h, b"fullcov_two_pass", two))
            run()                                                     # warm-up
            us, launches = [], 0
            for _ in range(reps):
                ok(lib.hgmm_profile_reset(h))
                ok(lib.hgmm_profile_enable(h, 1))
                run()
                ok(lib.hgmm_profile_enable(h, 0))
                total = 0.0
                for kid in kids:
                    ms, n = C.c_double(), C.c_int64()
                    ok(lib.hgmm_profile_get(h, kid, C.byref(ms), C.byref(n)))
                    total += 1e3 * ms.value / max(n.value, 1)          # (two-pass: one pass + one moments launch per iteration)
                    launches = int(n.value)
                us.append(total)
            by_path[path] = dict(us=us, launches=launches, q=[float(v) for v in q])
        ok(lib.hgmm_tree_set_precision(h, 0))
        ok(lib.hgmm_config_set(h, b"fullcov_two_pass", 0))
        if len(P) == 1000000:                                         # phase clocks of the float64 kernel, one fit
            clocks = (C.c_int64 * 32)()
            ok(lib.hgmm_fullcov_phase_clocks(h, 1, None))
            run()
            ok(lib.hgmm_fullcov_phase_clocks(h, 0, clocks))
            by_path["clocks"] = [int(v) for v in clocks]
        res[name] = by_path
    lib.hgmm_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib_path, weighted, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, "1" if weighted else "0", str(reps)],
                         capture_output=True, text=True, timeout=300)
    for line in out.stdout.split("\n"):
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError("child failed (%d):\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-2000:]))


def cost_section(parent_lib, reps, rounds=2):
    settings = ([("parent commit, hgmm_fullcov_fit", parent_lib, False)] if parent_lib else []) + \
               [("this commit, hgmm_fullcov_fit", LIB, False), ("this commit, hgmm_fullcov_fit_weighted, w == 1", LIB, True)]
    acc, clocks = {}, {}
    for _ in range(rounds):                                           # (alternating: drift shows between the rounds)
        for label, lib, weighted in settings:
            for wl, by_path in run_child(lib, weighted, reps).items():
                for path, d in by_path.items():
                    if path == "clocks":
                        clocks[label] = d
                        continue
                    a = acc.setdefault(wl, {}).setdefault(path, {}).setdefault(label, {"us": [], "q": d["q"]})
                    a["us"] += d["us"]
                    assert a["q"] == d["q"], (wl, path, label)
    lines = []
    for wl, paths in acc.items():
        lines += ["", "**%s** (%d fits of %d iterations per setting in %d processes; E-step bracket per launch)" %
                  (wl, rounds * reps, ITERS, rounds), "",
                  "| path | setting | us / launch: median (min .. max) | against this commit's unweighted entry |", "|---|---|---|---|"]
        for path, by in paths.items():
            base = np.median(by["this commit, hgmm_fullcov_fit"]["us"])
            qs = {tuple(a["q"]) for a in by.values()}
            for label, a in by.items():
                lines.append("| %s | %s | %s | %+.1f %% |" % (path, label, spread(a["us"]), 100.0 * (np.median(a["us"]) / base - 1.0)))
            lines.append("| %s | q traces of the settings | %s | |" % (path, "bitwise equal" if len(qs) == 1 else "DIFFER"))
    if clocks:
        lines += ["", "**Phase clocks, float64 one-pass kernel at 10^6 x 800** (hgmm_fullcov_phase_clocks: cycles of workgroup 7 over "
                  "one fit's %d launches, the wave with the longest total; A pdfs, B row sums / features, C statistics, wait barriers)" %
                  (ITERS + 1), "", "| setting | A | B | C | wait | total |", "|---|---|---|---|---|---|"]
        for label, c in clocks.items():
            waves = np.array(c).reshape(8, 4)
            wv = waves[np.argmax(waves.sum(1))]
            lines.append("| %s | %d | %d | %d | %d | %d |" % (label, wv[0], wv[1], wv[2], wv[3], wv.sum()))
    return "\n".join(lines)


def bench_section(parent_tree, reps):
    trees = [("parent commit", parent_tree), ("this commit", ROOT)]
    vals, unit = {k: [] for k, _ in trees}, ""
    for _ in range(reps):
        for label, tree in trees:
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"],
                                 cwd=tree, capture_output=True, text=True, timeout=400)
            line = [l for l in out.stdout.split("\n") if l.startswith("{")]
            if not line:
                raise RuntimeError("bench.py failed in %s:\n%s" % (tree, out.stderr[-2000:]))
            r = json.loads(line[-1])
            vals[label].append(float(r["value"]))
            unit = "%s, %s" % (r.get("metric", "value"), r.get("unit", ""))
    lines = ["", "**`bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline`** (%d runs per tree, alternating; %s)" % (reps, unit), "",
             "| tree | headline: median (min .. max) |", "|---|---|"]
    for label, _ in trees:
        lines.append("| %s | %s |" % (label, spread(vals[label])))
    return "\n".join(lines)


# ---- what weights buy -----------------------------------------------------------------------------------------------------
def buys_section():
    import hgmm_amd
    ctx = hgmm_amd.Context(0)
    full = np.load(os.path.join(GOLDEN, "bun000_xyz.npy")).astype(np.float64)
    cent, cnt = ctx.voxel_down_sample(full, 0.004)
    lines = ["", "bun000: %d points -> %d centroids of 4 mm voxels (counts 1 .. %d).  ls = 1.0, sig2 = 0.00034, at most 200 "
             "iterations; the three fits start from the same %s centroids' coordinates." % (len(full), len(cent), cnt.max(), "J"), "",
             "| J | model | iterations | max abs d pi vs full scan | max abs d mu vs full scan (mm) | mean log-density of the full scan |",
             "|---|---|---|---|---|---|"]
    for J in (16, 100):
        idx = np.random.RandomState(J).choice(len(cent), J, replace=False)
        init = cent[idx]
        fits = []
        for label, P, w in (("full scan", full, None), ("centroids under their counts", cent, cnt.astype(np.float64)),
                            ("centroids, unweighted", cent, None)):
            ctx.set_points(P)
            if w is not None:
                ctx.tree_set_source_weights(w)
            pi, mu, cov, _, q = ctx.fullcov_fit(J, 1.0, 1e-4, init, 0.00034, 200, weighted=w is not None)
            fits.append((label, pi, mu, cov, len(q)))
        ref = fits[0]
        ctx.set_points(full)
        for label, pi, mu, cov, n_it in fits:
            q = ctx.fullcov_estep(pi, mu, cov)[4]
            lines.append("| %d | %s | %d | %.3g | %.3g | %.4f |" % (J, label, n_it, np.abs(pi - ref[1]).max(),
                                                                   1e3 * np.abs(mu - ref[2]).max(), q / len(full)))
    ctx.close()
    return "\n".join(lines)


def main():
    if "--child" in sys.argv:
        k = sys.argv.index("--child")
        return child(sys.argv[k + 1], sys.argv[k + 2] == "1", int(sys.argv[k + 3]))
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    out_path = arg("--out", os.path.join(ROOT, "profiles", "fullcov_weights.md"))
    parent_lib, parent_tree, reps = arg("--parent-lib"), arg("--parent-tree"), int(arg("--reps", "5"))
    parts = ["# What per-point weights of the flat full-covariance fit cost and buy (`hgmm_fullcov_fit_weighted`)", "",
             "Written by `tools/fullcov_weights_probe.py`.", "", "## Code objects (gfx950)", "", isa_table(parent_lib)]
    if "--skip-gpu" not in sys.argv:
        if "--skip-buys" not in sys.argv:
            parts += ["", "## (a) What weights buy: the full scan's model from its 4 mm centroids", buys_section()]
        parts += ["", "## (b) The unweighted launch against the parent, and what the weighted launch costs", cost_section(parent_lib, reps)]
        if parent_tree and "--skip-bench" not in sys.argv:
            parts += ["", "## (c) The benchmark's headline", bench_section(parent_tree, max(2, reps // 2))]
    text = "\n".join(parts) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
