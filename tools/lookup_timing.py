"""Device and wall time of the LogUp lookup on one MI355X, Goldilocks, on generated tables of 2^n entries.

Per size, medians over --reps runs:
  * the trees: the top launch (SC_KIND_FRACTION_TREE from layer n) at LV = 1, 2, 3 (option fr_tree_lv), all-ones and general numerator,
    with its rate against the 6.29 TB/s copy figure, and the whole build (launch log and host clock)
  * the proof: sc_frac_prove on the host clock at fr_host_log = 0, 6, 8, 9, 10, 11, 12, and at the context's default
  * the first folding launch of the top layer (SC_KIND_FRACTION_PASS, kf = 1, the largest log_in): bytes, time, rate
  * the yardstick - the parent's nearest equivalent: two sc_gp_prove runs on tables of the same n in the same process; the ratio
  * sc_lookup_count: the count launch in G entries/s at m = 8, 13, 14, 20, uniform and all-equal indices (the contended case)
and once, at (n, m) = --lookup: prove_lookup step by step on the host clock.

  python tools/lookup_timing.py [--reps 5] [--sizes 20,22,24,26] [--lookup 24,16] [--out profiles]
writes <out>/lookup_timing.json and <out>/lookup_summary.md."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from grand_product_timing import COPY_TBS, HOST_LOGS, logged, ms, rate, wall_only  # noqa: E402

COUNT_LOGS = [8, 13, 14, 20]
MODES = (("ones", True), ("general", False))


def measure(pkg, n, reps):
    lu, gp = pkg.logup, pkg.grand_product
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    MLE = pkg.DenseMultilinearExtension
    q, p = MLE.generate(ctx, 1000 + n, n), MLE.generate(ctx, 2000 + n, n)
    default_T, default_lv = ctx.get_option("fr_host_log"), ctx.get_option("fr_tree_lv")
    res = {"n": n, "default_fr_host_log": default_T, "default_fr_tree_lv": default_lv, "tree": [], "prove_wall_ms": {}, "prove_default": {},
           "first_fold": {}, "count": []}
    # 1. the trees
    for name, ones in MODES:
        for lv in (1, 2, 3):
            ctx.set_option("fr_tree_lv", lv)
            _, log, walls = logged(ctx, lambda: lu.FractionTree(ctx, q, None if ones else p).close(), reps)
            log = [x for x in log if x["kind"] == "fraction_tree"]
            top = rate(dict(log[0]))
            top.update(mode=name, build_wall_ms=ms(walls), build_launch_ms=sum(x["ms"] for x in log), launches=len(log))
            res["tree"].append(top)
    ctx.set_option("fr_tree_lv", default_lv)
    # 2, 3. the proof
    for name, ones in MODES:
        tree = lu.FractionTree(ctx, q, None if ones else p)
        res["prove_wall_ms"][name] = {}
        for T in HOST_LOGS:
            ctx.set_option("fr_host_log", T)
            res["prove_wall_ms"][name][str(T)] = ms(wall_only(ctx, lambda: lu.prove(tree, seed_r=5), reps))
        ctx.set_option("fr_host_log", default_T)
        _, log, walls = logged(ctx, lambda: lu.prove(tree, seed_r=5), reps)
        log = [x for x in log if x["kind"] == "fraction_pass"]
        res["prove_default"][name] = {"wall_ms": ms(walls), "launches": len(log), "launch_ms": sum(x["ms"] for x in log)}
        folds = sorted((x for x in log if x["kf"] == 1), key=lambda x: -x["log_in"])
        if folds:
            res["first_fold"][name] = rate(dict(folds[0]))
        tree.close()
    # 4. the yardstick: two grand products over tables of the same n
    trees = [gp.ProductTree(ctx, q), gp.ProductTree(ctx, p)]

    def yardstick():
        for t in trees:
            gp.prove(t, seed_r=5)
    _, log, walls = logged(ctx, yardstick, reps)
    log = [x for x in log if x["kind"] == "product_pass"]
    res["yardstick"] = {"wall_ms": ms(walls), "launches": len(log), "launch_ms": sum(x["ms"] for x in log)}
    for name, _ in MODES:
        res["prove_default"][name]["over_two_gp"] = res["prove_default"][name]["wall_ms"]["median"] / res["yardstick"]["wall_ms"]["median"]
    for t in trees:
        t.close()
    del p
    # 5. the multiplicities: w = q's words looked up in a table of its first 2^m words (generated words are distinct for all that matters:
    # a repeated word only moves counts between equal entries' indices, which the time does not see)
    rng = np.random.default_rng(n)
    words = q.to_evaluations()
    for m in [m for m in COUNT_LOGS if m <= n]:
        t_words = np.ascontiguousarray(words[:1 << m])
        table = MLE.from_evaluations_vec(ctx, m, t_words)
        for pattern in ("uniform", "all_equal"):
            idx = (rng.integers(0, 1 << m, size=1 << n) if pattern == "uniform" else np.full(1 << n, (1 << m) // 2)).astype(np.uint32)
            w = MLE.from_evaluations_vec(ctx, n, t_words[idx])
            out, log, walls = logged(ctx, lambda: lu.multiplicities(ctx, w, table, idx), reps)
            assert out[1] == 0
            count = [x for x in log if x["kind"] == "lookup_count" and x["kf"] == 0][0]
            res["count"].append({"m": m, "pattern": pattern, "lds": count["ks"], "ms": count["ms"], "g_entries_s": (1 << n) / (count["ms"] * 1e-3) / 1e9,
                                 "call_wall_ms": ms(walls)})
            del w, out
    ctx.close()
    return res


def lookup_steps(pkg, n, m):
    """prove_lookup's steps, one by one on the host clock (a range table, plain openings, Reed-Solomon rows)"""
    lu, lp, r1cs = pkg.logup, pkg.ligero_pcs, pkg.r1cs
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    MLE = pkg.DenseMultilinearExtension
    rng, steps = random.Random(1), []

    def timed(name, fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        steps.append({"step": name, "ms": 1e3 * (time.perf_counter() - t0)})
        return out
    idx = np.random.default_rng(1).integers(0, 1 << m, size=1 << n).astype(np.uint32)
    R = (1 << 64) % F.p
    t_words = (np.arange(1 << m, dtype=object) * R % F.p).astype(np.uint64)
    w, t = MLE.from_evaluations_vec(ctx, n, t_words[idx]), MLE.from_evaluations_vec(ctx, m, t_words)
    pw = timed("commit w", lambda: lp.Prover.commit(ctx, w, log_cols=n // 2, log_blowup=1))
    vw = lp.Verifier(F, n, n // 2, 1, pw.root(), 8)
    P = lu.LookupProver(pw, t, idx)
    pm = timed("count and commit mult", lambda: P.commit_mult(lambda mult: lp.Prover.commit(ctx, mult, log_cols=m // 2, log_blowup=1)))
    V = lu.LookupVerifier(F, vw, lp.Verifier(F, m, m // 2, 1, pm.root(), 8), lambda point: lu.range_table_eval(F, point))
    roots = timed("affine maps and trees", lambda: P.roots(V.draw_alpha(rng)))
    V.receive_roots(*roots)
    for which, name in enumerate(("w", "t")):
        timed("fraction sum, %s side" % name, lambda: P.prove(which, V.frac[which].challenger(rng)))
        point, _ = V.opening(which)
        pcs = (P.pcs_w, P.pcs_mult)[which]
        opened = timed("opening, %s side" % name, lambda: r1cs.open_committed(pcs, V.pcs[which], point, rng))
        V.finish(which, opened)
    P.close()
    pw.close()
    ctx.close()
    return {"n": n, "m": m, "steps": steps, "total_ms": sum(s["ms"] for s in steps)}


def summary(results, lookup, reps):
    out = ["# LogUp lookups on one MI355X (Goldilocks)", "",
           "`tools/lookup_timing.py --reps %d`; launch times are medians over the runs, from the launch log; wall times are the host" % reps,
           "clock around the call and a stream synchronisation.", ""]
    for r in results:
        n = r["n"]
        out += ["## n = %d" % n, "", "Top launch of the trees (from layer %d) by layers per launch, and the whole build with that setting:" % n, "",
                "| numerator | LV | MiB moved | us | TB/s | share of %.2f TB/s | launches | build, launches us | build, wall ms (median) |" % COPY_TBS,
                "|---|---|---|---|---|---|---|---|---|"]
        for x in r["tree"]:
            out.append("| %s | %d | %.1f | %.1f | %.3f | %.1f %% | %d | %.1f | %.3f |" % (
                x["mode"], x["kf"], (x["bytes_read"] + x["bytes_written"]) / 2**20, 1e3 * x["ms"], x["tb_s"], 100 * x["share_of_copy"], x["launches"],
                1e3 * x["build_launch_ms"], x["build_wall_ms"]["median"]))
        out += ["", "sc_frac_prove, wall ms (median / min) by fr_host_log:", "", "| fr_host_log | ones | general |", "|---|---|---|"]
        for T in r["prove_wall_ms"]["ones"]:
            a, b = r["prove_wall_ms"]["ones"][T], r["prove_wall_ms"]["general"][T]
            out.append("| %s | %.3f / %.3f | %.3f / %.3f |" % (T, a["median"], a["min"], b["median"], b["min"]))
        y = r["yardstick"]
        out += ["", "At the default fr_host_log = %d, against two sc_gp_prove runs on tables of the same n (%.3f ms wall median, %d launches, %.3f ms inside them):" % (
            r["default_fr_host_log"], y["wall_ms"]["median"], y["launches"], y["launch_ms"]), "",
            "| numerator | wall ms (median) | launches | ms inside them | over two sc_gp_prove |", "|---|---|---|---|---|"]
        for name, d in r["prove_default"].items():
            out.append("| %s | %.3f | %d | %.3f | x %.2f |" % (name, d["wall_ms"]["median"], d["launches"], d["launch_ms"], d["over_two_gp"]))
        out += ["", "First folding launch of the top layer:", "", "| numerator | tables | log_in | MiB moved | us | TB/s | share of %.2f TB/s |" % COPY_TBS,
                "|---|---|---|---|---|---|---|"]
        for name, x in r["first_fold"].items():
            out.append("| %s | %d | %d | %.1f | %.1f | %.3f | %.1f %% |" % (name, x["ks"], x["log_in"], (x["bytes_read"] + x["bytes_written"]) / 2**20, 1e3 * x["ms"],
                                                                         x["tb_s"], 100 * x["share_of_copy"]))
        out += ["", "sc_lookup_count, the count launch over 2^%d entries:" % n, "", "| m | indices | LDS histograms | us | G entries/s | call, wall ms (median) |",
                "|---|---|---|---|---|---|"]
        for x in r["count"]:
            out.append("| %d | %s | %s | %.1f | %.2f | %.3f |" % (x["m"], x["pattern"], "yes" if x["lds"] else "no", 1e3 * x["ms"], x["g_entries_s"],
                                                                 x["call_wall_ms"]["median"]))
        out.append("")
    if lookup:
        out += ["## prove_lookup step by step, (n, m) = (%d, %d), range table, plain openings, one run on the host clock" % (lookup["n"], lookup["m"]), "",
                "| step | ms |", "|---|---|"]
        out += ["| %s | %.3f |" % (s["step"], s["ms"]) for s in lookup["steps"]]
        out += ["| total | %.3f |" % lookup["total_ms"], ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,22,24,26")
    ap.add_argument("--lookup", default="24,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results, lookup = [], None
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("lookup_timing", "python tools/lookup_timing.py --reps %d --sizes %s --lookup %s" % (args.reps, args.sizes, args.lookup))

    def write():
        with open(os.path.join(args.out, "lookup_timing.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results, "lookup": lookup}, f, indent=1)
        with open(os.path.join(args.out, "lookup_summary.md"), "w") as f:
            f.write(summary(results, lookup, args.reps) + "\n")
    for n in [int(x) for x in args.sizes.split(",") if x]:
        results.append(measure(pkg, n, args.reps))
        print("n = %d: prove %s" % (n, json.dumps(results[-1]["prove_default"])), flush=True)
        write()
    if args.lookup:
        n, m = (int(x) for x in args.lookup.split(","))
        lookup = lookup_steps(pkg, n, m)
        print("lookup (%d, %d): %.1f ms" % (n, m, lookup["total_ms"]), flush=True)
        write()


if __name__ == "__main__":
    main()
