"""Device and wall time of the sum-of-products sumcheck with challenges from the quadratic extension on one MI355X, Goldilocks,
next to sc_sumprod_prove on the same tables in the same process.  Medians over --reps runs (five by default), after one run that is
not counted.  At n in --sizes and T in 1, 5: launches, time inside them from the launch log, bytes per second against the byte model,
per round; and the ratio of the two proofs in bytes and in time.  No number is gated.

  python tools/ext_sumcheck_timing.py [--reps 5] [--sizes 23,25,27] [--out profiles]
writes <out>/ext_sumcheck_summary.json and <out>/ext_sumcheck_summary.md."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from grand_product_timing import COPY_TBS, logged, ms, rate  # noqa: E402

PAIRS = (1, 5)
KINDS = ("sumprod_pass", "sumprod_ext_pass")


def totals(passes):
    moved = sum(x["bytes_read"] + x["bytes_written"] for x in passes)
    inside = sum(x["ms"] for x in passes)
    return {"launches": len(passes), "launch_ms": inside, "bytes": moved, "tb_s": moved / (inside * 1e-3) / 1e12, "rounds": passes}


def measure(pkg, n, T, reps):
    mo, xs = pkg.multiopen, pkg.ext_sumcheck
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    MLE = pkg.DenseMultilinearExtension
    w = F.from_int(pkg.ext_field.nonresidue(F.p))
    a = [MLE.generate(ctx, 100 + k, n) for k in range(T)]
    b = [MLE.generate(ctx, 200 + k, n) for k in range(T)]
    res = {"n": n, "pairs": T, "wall_ms": {}}
    _, log, walls = logged(ctx, lambda: mo.sumprod_prove(ctx, a, b, seed_r=7), reps)
    res["base"] = totals([rate(dict(x)) for x in log if x["kind"] in KINDS])
    res["wall_ms"]["sumprod_prove"] = ms(walls)
    _, log, walls = logged(ctx, lambda: xs.sumprod_prove_ext(ctx, w, a, b, seed_r=7), reps)
    res["ext"] = totals([rate(dict(x)) for x in log if x["kind"] in KINDS])
    res["wall_ms"]["sumprod_prove_ext"] = ms(walls)
    res["bytes_ratio"] = res["ext"]["bytes"] / res["base"]["bytes"]
    res["launch_ms_ratio"] = res["ext"]["launch_ms"] / res["base"]["launch_ms"]
    del a, b
    ctx.close()
    return res


def summary(results, reps, prov):
    out = ["# The sum-of-products sumcheck with extension-field challenges on one MI355X (Goldilocks, w = 7)", "",
           "`tools/ext_sumcheck_timing.py --reps %d`; sources %s, commit %s.  Launch times are medians over the runs, from the launch log; wall" % (
               reps, prov["csrc_sha16"], prov["commit"]),
           "times are the host clock around the call and a stream synchronisation.  The comparison is sc_sumprod_prove on the same tables in",
           "the same process.  Shares are of the %.2f TB/s a device-to-device copy reaches.  Nothing here is gated." % COPY_TBS, "",
           "| n | T | proof | launches | ms inside them | GiB moved (byte model) | TB/s | call wall ms |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for name, key, wall in (("sc_sumprod_prove", "base", "sumprod_prove"), ("sc_sumprod_prove_ext", "ext", "sumprod_prove_ext")):
            x = r[key]
            out.append("| %d | %d | %s | %d | %.3f | %.2f | %.3f | %.3f |" % (r["n"], r["pairs"], name, x["launches"], x["launch_ms"], x["bytes"] / 2**30, x["tb_s"],
                                                                            r["wall_ms"][wall]["median"]))
    out += ["", "| n | T | bytes, extension / base | time inside launches, extension / base |", "|---|---|---|---|"]
    for r in results:
        out.append("| %d | %d | %.3f | %.3f |" % (r["n"], r["pairs"], r["bytes_ratio"], r["launch_ms_ratio"]))
    out += ["", "## The first five rounds, each next to its base-field counterpart", "",
            "| n | T | round | base: us / TB/s | extension: kf | us / TB/s | bytes ratio | time ratio |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for j, (x, y) in enumerate(list(zip(r["base"]["rounds"], r["ext"]["rounds"]))[:5]):
            out.append("| %d | %d | %d | %.1f / %.2f | %s | %.1f / %.2f | %.2f | %.2f |" % (
                r["n"], r["pairs"], j, 1e3 * x["ms"], x["tb_s"], "round 0 (kind 37)" if y["kind"] == "sumprod_pass" else str(y["kf"]), 1e3 * y["ms"], y["tb_s"],
                (y["bytes_read"] + y["bytes_written"]) / (x["bytes_read"] + x["bytes_written"]), y["ms"] / x["ms"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="23,25,27")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results = []
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("ext_sumcheck_timing", "python tools/ext_sumcheck_timing.py --reps %d --sizes %s" % (args.reps, args.sizes))

    def write():
        with open(os.path.join(args.out, "ext_sumcheck_summary.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results}, f, indent=1)
        with open(os.path.join(args.out, "ext_sumcheck_summary.md"), "w") as f:
            f.write(summary(results, args.reps, prov) + "\n")
    for n in [int(x) for x in args.sizes.split(",") if x]:
        for T in PAIRS:
            results.append(measure(pkg, n, T, args.reps))
            print("n = %d, T = %d: %s bytes x %.3f, launch time x %.3f" % (n, T, json.dumps(results[-1]["wall_ms"]), results[-1]["bytes_ratio"],
                                                                         results[-1]["launch_ms_ratio"]), flush=True)
            write()


if __name__ == "__main__":
    main()
