"""Wall and device time of the Relaxed PCS prover on one MI355X:

  merkle   sc_merkle_commit of Goldilocks tables of 2^n entries (sc_table_generate), n = 20, 24, 28
  prover   relaxed_pcs.Prover.new for p = 11, m = 6, 7, 8: sc_table_extend_grid (one launch per variable) + the commitment

Per size: one warm-up call, then --reps calls timed on the host (the commit reads its root back, so the call ends when the tree
is done), and the launch log (option time_kernels) for every kernel's device time and bytes.  A tree over N leaves costs
3N - 2 SHA-256 compressions (a leaf is one, a node two).

VALU bound: the ISA of merkle_level_kernel (`make -C thaler-study_amd/csrc isa`) holds one node = two compressions; its VALU
instruction count / 2 is the cost of a compression, and 256 CU x 4 SIMD x 32 lanes per cycle x 2.4 GHz is the peak lane rate.
That peak assumes 32-bit integer VALU issues at the f32 rate the guide measures (v_fma_f32 wave64: 2 cycles); nobody has
measured that for these instructions, so the fraction is an estimate against an unmeasured bound.

Grid traffic: the floor is 8 * 2^m bytes read + 8 * p^m written (the zero padding up to N is a memset); the launches are one per variable (not fused), and their
records state what each reads and writes.

CPU baseline: the same compression function (kernels/sha256.hpp) compiled with g++ -O2 for the host, one core, n = 20.

  python tools/pcs_timing.py [--reps 5] [--limit 600] [--trace]    every step in a child process under its own time limit;
                                                                  writes profiles/pcs_timing.json and profiles/pcs_summary.md;
                                                                  --trace adds a rocprofv3 --kernel-trace --stats run whose
                                                                  stats go to profiles/pcs_kernel_stats.csv
  python tools/pcs_timing.py --step merkle|prover [--reps 5]       one step, one JSON line
"""
import argparse
import ctypes
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thaler-study_amd", "csrc")
PROFILES = os.path.join(ROOT, "profiles")
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9
MERKLE_SIZES = (20, 24, 28)
PROVER_SIZES = (6, 7, 8)


def _timed(ctx, fn, reps):
    fn()   # warm-up (code objects, pool)
    ctx.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        walls.append(time.perf_counter() - t0)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    fn()
    ctx.synchronize()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    return walls, log


def run_step(step, reps):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    rp = pkg.relaxed_pcs
    out = {"step": step, "sizes": {}}
    if step == "merkle":
        ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
        for n in MERKLE_SIZES:
            t = pkg.DenseMultilinearExtension.generate(ctx, 0x7EE0000 + n, n)
            walls, log = _timed(ctx, lambda: rp.merkle_commit(ctx, t).close(), reps)
            kernels = {}
            for r in log:
                if r["kind"] == "merkle":
                    k = kernels.setdefault(pkg._lib.MERKLE_KERNELS[r["kf"]], {"launches": 0, "ms": 0.0})
                    k["launches"] += 1
                    k["ms"] += r["ms"]
            wall = statistics.median(walls)
            comp = 3 * (1 << n) - 2
            out["sizes"][str(n)] = {"wall_ms": wall * 1e3, "wall_all_ms": [w * 1e3 for w in walls], "compressions": comp,
                                    "compressions_per_s": comp / wall, "root": rp.merkle_commit(ctx, t).root().hex(), "kernels": kernels,
                                    "device_ms": sum(k["ms"] for k in kernels.values())}
            del t
    else:
        p = 11
        F = pkg.Field(p)
        ctx = pkg.Context(F, device=0)
        for m in PROVER_SIZES:
            poly = pkg.DenseMultilinearExtension.generate(ctx, 0x9C1D0000 + m, m)
            walls, log = _timed(ctx, lambda: rp.Prover.new(ctx, poly), reps)
            N = 1
            while N < p ** m:
                N *= 2
            grid = [r for r in log if r["kind"] == "grid_extend"]
            merkle = [r for r in log if r["kind"] == "merkle"]
            g_read = sum(r["bytes_read"] for r in grid)
            g_written = sum(r["bytes_written"] for r in grid)
            g_ms = sum(r["ms"] for r in grid)
            floor = 8 * (1 << m) + 8 * p ** m      # the table once in, every grid value once out (the padding is a memset)
            wall = statistics.median(walls)
            out["sizes"][str(m)] = {"p": p, "points": p ** m, "N": N, "wall_ms": wall * 1e3, "wall_all_ms": [w * 1e3 for w in walls],
                                    "grid": {"launches": len(grid), "ms": g_ms, "bytes_read": g_read, "bytes_written": g_written,
                                             "floor_bytes": floor, "traffic_over_floor": (g_read + g_written) / floor,
                                             "GBps_model": (g_read + g_written) / (g_ms * 1e-3) / 1e9 if g_ms else None,
                                             "per_launch": [{"kf": r["kf"], "ms": r["ms"], "bytes_read": r["bytes_read"],
                                                             "bytes_written": r["bytes_written"]} for r in grid]},
                                    "merkle_ms": sum(r["ms"] for r in merkle), "compressions": 3 * N - 2}
    return out


def valu_per_compression():
    """VALU instructions of one node of merkle_level_kernel (two compressions) / 2, from the built ISA"""
    subprocess.check_call(["make", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, "build", "sumcheck_hip.s")).read()
    m = re.search(r"^(_ZN2sc19merkle_level_kernel\S*):[^\n]*\n(.*?)\n\.Lfunc_end", text, flags=re.S | re.M)
    body = m.group(2)
    valu = [l.split()[0] for l in body.split("\n") if l.strip().startswith("v_")]
    counts = {}
    for v in valu:
        counts[v] = counts.get(v, 0) + 1
    return len(valu) / 2.0, dict(sorted(counts.items(), key=lambda kv: -kv[1])[:10])


def cpu_baseline(n=20):
    out = tempfile.mkdtemp()
    so = os.path.join(out, "libpcs_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "cpp", "pcs_host_harness.cpp")])
    lib = ctypes.CDLL(so)
    N = 1 << n
    vals = (ctypes.c_uint64 * N)(*range(N))
    root = (ctypes.c_uint32 * 8)()
    secs = ctypes.c_double()
    lib.ph_root(vals, n, root, ctypes.byref(secs))
    shutil.rmtree(out, ignore_errors=True)
    return {"n": n, "ms": secs.value * 1e3, "compressions_per_s": (3 * N - 2) / secs.value}


def summary(res):
    v = res["valu_per_compression"]
    bound = res["valu_bound_compressions_per_s"]
    lines = ["# Relaxed PCS on one MI355X: grid evaluation and SHA-256 Merkle commitment", "",
             "Measured by `tools/pcs_timing.py` (wall times: median of %d calls, host clock around the call; device times: HIP events "
             "of the launch log)." % res["reps"], "",
             "## Merkle commitment, Goldilocks tables (sc_table_generate)", "",
             "| n | wall ms | device ms | compressions | compressions/s | fraction of the VALU bound (estimate) |", "|---|---|---|---|---|---|"]
    for n, r in res["steps"]["merkle"]["sizes"].items():
        lines.append("| %s | %.3f | %.3f | %d | %.3g | %.0f %% |" % (n, r["wall_ms"], r["device_ms"], r["compressions"], r["compressions_per_s"],
                                                             100 * r["compressions_per_s"] / bound))
    lines += ["", "Kernels at the largest n: " + ", ".join("%s %d launch(es) %.3f ms" % (k, d["launches"], d["ms"])
                                                          for k, d in res["steps"]["merkle"]["sizes"][str(MERKLE_SIZES[-1])]["kernels"].items()), "",
              "**VALU bound (an estimate, not a measurement).** `merkle_level_kernel` spends %d VALU instructions on one node (two "
              "compressions, the second with the constant padding schedule folded in): %.0f per compression.  256 CU × 4 SIMD × 32 "
              "lanes/cycle × 2.4 GHz = %.3g lane-ops/s gives %.3g compressions/s.  That peak assumes 32-bit integer VALU issues at the "
              "f32 rate the guide measures (`v_fma_f32` wave64: 2 cycles); nobody has measured it for `v_alignbit_b32` / `v_bitop3_b32` "
              "/ `v_add3_u32`.  Most frequent instructions: %s." % (2 * v, v, PEAK_LANE_OPS, bound, res["valu_top"]), "",
              "**CPU baseline**: the same compression function compiled with g++ -O2, one core, n = %d: %.1f ms = %.3g compressions/s; "
              "the GPU commit at n = 20 is %.0f× that." % (res["cpu"]["n"], res["cpu"]["ms"], res["cpu"]["compressions_per_s"],
                                                          res["steps"]["merkle"]["sizes"]["20"]["compressions_per_s"] / res["cpu"]["compressions_per_s"]),
              "", "## Prover.new, p = 11 (grid evaluation + commitment)", "",
              "| m | p^m | N | wall ms | grid launches | grid ms | grid bytes (read + written) | floor bytes (8·2^m + 8·p^m) | traffic / floor | merkle ms |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for m, r in res["steps"]["prover"]["sizes"].items():
        g = r["grid"]
        lines.append("| %s | %d | %d | %.3f | %d | %.3f | %d | %d | %.3f | %.3f |" % (m, r["points"], r["N"], r["wall_ms"], g["launches"], g["ms"],
                                                                               g["bytes_read"] + g["bytes_written"], g["floor_bytes"],
                                                                               g["traffic_over_floor"], r["merkle_ms"]))
    lines += ["", "The grid is built one launch per variable (`grid_extend_kernel`, launch kind 17), not fused: the intermediate "
              "tables cost about p/(p−2) times the output in writes, plus their reads (the traffic / floor column, from the "
              "launch records).  The zero padding past p^m, 8·(N − p^m) bytes, is a memset and is in neither column.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=("merkle", "prover"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds each child step may take")
    ap.add_argument("--trace", action="store_true", help="also one rocprofv3 --kernel-trace --stats run of both steps")
    ap.add_argument("--summary-only", action="store_true", help="rewrite profiles/pcs_summary.md from profiles/pcs_timing.json")
    args = ap.parse_args()
    if args.summary_only:
        with open(os.path.join(PROFILES, "pcs_timing.json")) as fh:
            res = json.load(fh)
        for m, r in res["steps"]["prover"]["sizes"].items():
            g = r["grid"]
            g["floor_bytes"] = 8 * (1 << int(m)) + 8 * r["points"]
            g["traffic_over_floor"] = (g["bytes_read"] + g["bytes_written"]) / g["floor_bytes"]
        with open(os.path.join(PROFILES, "pcs_timing.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.join(PROFILES, "pcs_summary.md"), "w") as fh:
            fh.write(summary(res))
        return
    if args.step:
        print(json.dumps(run_step(args.step, args.reps)))
        return
    res = {"reps": args.reps, "steps": {}}
    for step in ("merkle", "prover"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if p.returncode != 0:
            print(json.dumps({"step": step, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}))
            sys.exit(1)                                  # nothing more on the GPU after a failed step
        res["steps"][step] = json.loads(p.stdout.strip().splitlines()[-1])
    if args.trace:
        d = tempfile.mkdtemp()
        for step in ("merkle", "prover"):
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(d, step), "-o", step, "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--step", step, "--reps", "1"]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            if p.returncode != 0:
                print(json.dumps({"trace": step, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}))
                sys.exit(1)
        rows = []
        for step in ("merkle", "prover"):
            for f in glob.glob(os.path.join(d, step, "**", "*kernel_stats.csv"), recursive=True):
                with open(f) as fh:
                    text = fh.read().splitlines()
                rows += ([text[0]] if not rows else []) + text[1:]
        with open(os.path.join(PROFILES, "pcs_kernel_stats.csv"), "w") as fh:
            fh.write("\n".join(rows) + "\n")
        shutil.rmtree(d, ignore_errors=True)
    v, top = valu_per_compression()
    res["valu_per_compression"] = v
    res["valu_top"] = ", ".join("%s %d" % kv for kv in top.items())
    res["valu_bound_compressions_per_s"] = PEAK_LANE_OPS / v
    res["cpu"] = cpu_baseline()
    with open(os.path.join(PROFILES, "pcs_timing.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(PROFILES, "pcs_summary.md"), "w") as fh:
        fh.write(summary(res))
    print(json.dumps({k: res[k] for k in ("valu_per_compression", "valu_bound_compressions_per_s", "cpu")}))


if __name__ == "__main__":
    main()
