"""Device and wall time of the grand product argument on one MI355X, Goldilocks, on generated tables of 2^n entries.

Per size, medians over --reps runs:
  * the tree: the top launch (SC_KIND_PRODUCT_TREE from layer n) at LV = 1, 2, 3 (option gp_tree_lv) with its rate against the
    tree's 6.29 TB/s copy figure, and the whole build at the default schedule (launch log and host clock)
  * the proof: sc_gp_prove on the host clock at gp_host_log = 0, 6, 8, 9, 10, 11, 12, and at the context's default
  * the yardstick - what a user could do before: the same layers through sc_zerocheck_prove(L_k, R_k, zero table), L_k and R_k
    wrapped by sc_table_from_device over a copy of each layer, in the same process; the ratio to the new path
  * the largest SC_KIND_PRODUCT_PASS launches of a proof at the default: bytes, time, rate

  python tools/grand_product_timing.py [--reps 5] [--sizes 20,22,24,26] [--out profiles]
writes <out>/grand_product_timing.json and <out>/grand_product_summary.md."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402

COPY_TBS = 6.29
HOST_LOGS = [0, 6, 8, 9, 10, 11, 12]


def logged(ctx, fn, reps):
    """fn() reps times under the launch log: (the last result, per-launch medians in launch order, wall seconds of every run)"""
    fn()
    ctx.synchronize()
    runs, walls, out = [], [], None
    ctx.set_option("time_kernels", 1)
    for _ in range(reps):
        ctx.launch_log()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        walls.append(time.perf_counter() - t0)
        runs.append(ctx.launch_log())
    ctx.set_option("time_kernels", 0)
    assert all(len(r) == len(runs[0]) for r in runs)
    med = []
    for i, x in enumerate(runs[0]):
        y = dict(x)
        y["ms"] = statistics.median(r[i]["ms"] for r in runs)
        med.append(y)
    return out, med, walls


def wall_only(ctx, fn, reps):
    fn()
    ctx.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        walls.append(time.perf_counter() - t0)
    return walls


def ms(walls):
    return {"median": 1e3 * statistics.median(walls), "min": 1e3 * min(walls)}


def rate(x):
    x["tb_s"] = (x["bytes_read"] + x["bytes_written"]) / (x["ms"] * 1e-3) / 1e12
    x["share_of_copy"] = x["tb_s"] / COPY_TBS
    return x


def measure(pkg, n, reps):
    gp, rp = pkg.grand_product, pkg.r1cs
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    MLE = pkg.DenseMultilinearExtension
    table = MLE.generate(ctx, 1000 + n, n)
    default_T, default_lv = ctx.get_option("gp_host_log"), ctx.get_option("gp_tree_lv")
    res = {"n": n, "default_gp_host_log": default_T, "default_gp_tree_lv": default_lv, "tree_top": [], "prove_wall_ms": {}}

    def build():
        gp.ProductTree(ctx, table).close()
    # 1. the tree
    for lv in (1, 2, 3):
        ctx.set_option("gp_tree_lv", lv)
        _, log, walls = logged(ctx, build, reps)
        top = rate(dict([x for x in log if x["kind"] == "product_tree"][0]))
        top["build_wall_ms"] = ms(walls)
        top["build_launch_ms"] = sum(x["ms"] for x in log if x["kind"] == "product_tree")
        top["launches"] = len([x for x in log if x["kind"] == "product_tree"])
        res["tree_top"].append(top)
    ctx.set_option("gp_tree_lv", default_lv)
    _, log, walls = logged(ctx, build, reps)
    res["tree_build"] = {"launches": [rate(dict(x)) for x in log if x["kind"] == "product_tree"], "wall_ms": ms(walls)}
    # 2. the proof
    tree = gp.ProductTree(ctx, table)
    for T in HOST_LOGS:
        ctx.set_option("gp_host_log", T)
        res["prove_wall_ms"][str(T)] = ms(wall_only(ctx, lambda: gp.prove(tree, seed_r=5), reps))
    ctx.set_option("gp_host_log", default_T)
    proof, log, walls = logged(ctx, lambda: gp.prove(tree, seed_r=5), reps)
    res["prove_default"] = {"wall_ms": ms(walls), "launches": len([x for x in log if x["kind"] == "product_pass"]),
                            "launch_ms": sum(x["ms"] for x in log if x["kind"] == "product_pass")}
    passes = sorted((rate(dict(x)) for x in log if x["kind"] == "product_pass"), key=lambda x: -x["bytes_read"])
    res["largest_passes"] = passes[:6]
    # 3. the yardstick: one sc_zerocheck_prove(L_k, R_k, 0) per layer over copies of the layers
    layers = []
    for k in range(1, n):
        src = tree.layer(k + 1) if k + 1 < n else table.clone()
        ptr = ctx.lib.sc_table_device_ptr(src.h)
        L = MLE.from_device(ctx, ptr, k, keep=src)
        R = MLE.from_device(ctx, ptr + (8 << k), k, keep=src)
        zero = MLE.from_evaluations_vec(ctx, k, np.zeros(1 << k, dtype=np.uint64))
        layers.append((L, R, zero, [F.from_int(3 + i) for i in range(k)]))

    def yardstick():
        for L, R, zero, tau in layers:
            rp.zerocheck_prove(ctx, L, R, zero, tau, None, seed_r=5)
    _, log, walls = logged(ctx, yardstick, reps)
    res["yardstick"] = {"wall_ms": ms(walls), "launches": len([x for x in log if x["kind"] == "zerocheck"]),
                        "launch_ms": sum(x["ms"] for x in log if x["kind"] == "zerocheck")}
    res["yardstick_over_new"] = res["yardstick"]["wall_ms"]["median"] / res["prove_default"]["wall_ms"]["median"]
    del layers
    tree.close()
    ctx.close()
    return res


def summary(results, reps):
    out = ["# Grand product argument on one MI355X (Goldilocks)", "",
           "`tools/grand_product_timing.py --reps %d`; launch times are medians over the runs, from the launch log; wall times are" % reps,
           "the host clock around the call and a stream synchronisation.", ""]
    for r in results:
        n = r["n"]
        out += ["## n = %d" % n, "", "Top launch of the tree (from layer %d) by layers per launch, and the whole build with that setting:" % n, "",
                "| LV | MiB moved | us | TB/s | share of %.2f TB/s | launches | build, launches us | build, wall ms (median) |" % COPY_TBS, "|---|---|---|---|---|---|---|---|"]
        for x in r["tree_top"]:
            out.append("| %d | %.1f | %.1f | %.3f | %.1f %% | %d | %.1f | %.3f |" % (x["kf"], (x["bytes_read"] + x["bytes_written"]) / 2**20, 1e3 * x["ms"], x["tb_s"],
                                                                                   100 * x["share_of_copy"], x["launches"], 1e3 * x["build_launch_ms"], x["build_wall_ms"]["median"]))
        out += ["", "Build at the default schedule (gp_tree_lv = %d): %.3f ms wall (median), launches: %s." % (
            r["default_gp_tree_lv"], r["tree_build"]["wall_ms"]["median"],
            ", ".join("kf %d from layer %d %.1f us" % (x["kf"], x["log_in"], 1e3 * x["ms"]) for x in r["tree_build"]["launches"])), "",
            "sc_gp_prove, wall ms by gp_host_log:", "", "| gp_host_log | median | min |", "|---|---|---|"]
        for T, v in r["prove_wall_ms"].items():
            out.append("| %s | %.3f | %.3f |" % (T, v["median"], v["min"]))
        d, y = r["prove_default"], r["yardstick"]
        out += ["", "At the default gp_host_log = %d: %.3f ms wall (median), %d launches, %.3f ms inside them." % (
            r["default_gp_host_log"], d["wall_ms"]["median"], d["launches"], d["launch_ms"]),
            "The same layers through sc_zerocheck_prove(L_k, R_k, 0): %.3f ms wall (median), %d launches, %.3f ms inside them: x %.2f of the new path." % (
                y["wall_ms"]["median"], y["launches"], y["launch_ms"], r["yardstick_over_new"]), "",
            "Largest SC_KIND_PRODUCT_PASS launches:", "", "| log_in | folded | MiB moved | us | TB/s | share of %.2f TB/s |" % COPY_TBS, "|---|---|---|---|---|---|"]
        for x in r["largest_passes"]:
            out.append("| %d | %d | %.1f | %.1f | %.3f | %.1f %% |" % (x["log_in"], x["kf"], (x["bytes_read"] + x["bytes_written"]) / 2**20, 1e3 * x["ms"], x["tb_s"],
                                                                     100 * x["share_of_copy"]))
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,22,24,26")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results = []
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("grand_product_timing", "python tools/grand_product_timing.py --reps %d --sizes %s" % (args.reps, args.sizes))
    for n in [int(x) for x in args.sizes.split(",")]:
        results.append(measure(pkg, n, args.reps))
        print("n = %d: prove %s, yardstick x %.2f" % (n, json.dumps(results[-1]["prove_wall_ms"]), results[-1]["yardstick_over_new"]), flush=True)
        with open(os.path.join(args.out, "grand_product_timing.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results}, f, indent=1)
        with open(os.path.join(args.out, "grand_product_summary.md"), "w") as f:
            f.write(summary(results, args.reps) + "\n")


if __name__ == "__main__":
    main()
