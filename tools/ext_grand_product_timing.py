"""Device and wall time of the grand product argument over the quadratic extension on one MI355X, Goldilocks, w = 7, next to
sc_gp_create + sc_gp_prove on the same table in the same process.  Medians over --reps runs (five by default), after one run that is
not counted; launch times from the launch log.  At n in --sizes: launches, time inside them, bytes against the byte model (the
recorded bytes are checked against the model computed here), TB/s per launch kind, the eq table's share of a proof's launch time,
and the ratios of the two arguments in bytes and in time.  No number is gated.

The base-field proof's eq tables (eq_table_kernel) leave no launch record, the extension's do (SC_KIND_EXT_EQ_TABLE): the time ratio is
given with and without them.

  python tools/ext_grand_product_timing.py [--reps 5] [--sizes 20,24,26,28] [--out profiles]
writes <out>/ext_grand_product_summary.json and <out>/ext_grand_product_summary.md."""
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

BASE_KINDS = ("product_tree", "product_pass")
EXT_KINDS = ("ext_product_tree", "ext_product_pass", "ext_eq_table")
BIG = 20      # the launches of at least 2^BIG entries carry a kind's rate


def model_bytes(n, T, lv, tail, ext):
    """(tree bytes, pass bytes, eq bytes) by the byte models of include/sumcheck_hip.h at gp_host_log = T, gp_tree_lv = lv"""
    word = 16 if ext else 8
    tree, m = 0, n
    while m > tail:
        step = min(lv, m - tail)
        tree += ((8 if m == n else word) << m) + (word << m) - (word << (m - step))
        m -= step
    tree += ((8 if m == n else word) << m) + (word << m) - word
    passes = eq = 0
    te = max(T, 1)
    for k in range(T + 1, n):
        leaf = ext and k == n - 1
        if ext:
            eq += 16 * k + (16 << k)
        passes += (word << k) + 2 * ((8 if leaf else word) << k)
        for j in range(1, k - te + 1):
            i = k - j + 1
            first = leaf and j == 1
            passes += (word << i) + 2 * ((8 if first else word) << i) + 3 * (word << (i - 1))
    return tree, passes, eq


def totals(records):
    moved = sum(x["bytes_read"] + x["bytes_written"] for x in records)
    inside = sum(x["ms"] for x in records)
    return {"launches": len(records), "launch_ms": inside, "bytes": moved, "tb_s": moved / (inside * 1e-3) / 1e12 if inside else 0.0}


def by_kind(records, kinds):
    out = {}
    for kind in kinds:
        out[kind] = totals([x for x in records if x["kind"] == kind])
        out[kind]["big"] = totals([x for x in records if x["kind"] == kind and x["log_in"] >= BIG])
    return out


def measure(pkg, n, reps):
    gp, xg = pkg.grand_product, pkg.ext_grand_product
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    w = F.from_int(pkg.ext_field.nonresidue(F.p))
    table = pkg.DenseMultilinearExtension.generate(ctx, 1000 + n, n)
    T, lv = ctx.get_option("gp_host_log"), ctx.get_option("gp_tree_lv")
    alpha, beta = (F.neg(F.one), 0), (F.from_int(123456789), F.from_int(987654321))     # the permutation check's leaves gamma - t
    res = {"n": n, "gp_host_log": T, "gp_tree_lv": lv, "wall_ms": {}}

    def both(create, prove, kinds):
        trees = []

        def build():
            while trees:
                trees.pop().close()
            trees.append(create())
        _, tree_log, tree_walls = logged(ctx, build, reps)
        _, proof_log, proof_walls = logged(ctx, lambda: prove(trees[0]), reps)
        trees.pop().close()
        records = [rate(dict(x)) for x in tree_log + proof_log if x["kind"] in kinds]
        out = totals(records)
        out["kinds"] = by_kind(records, kinds)
        out["largest"] = sorted((x for x in records if x["log_in"] >= n - 2), key=lambda x: -x["ms"])[:8]
        return out, ms(tree_walls), ms(proof_walls)
    res["base"], res["wall_ms"]["sc_gp_create"], res["wall_ms"]["sc_gp_prove"] = both(
        lambda: gp.ProductTree(ctx, table), lambda t: gp.prove(t, seed_r=7), BASE_KINDS)
    res["ext"], res["wall_ms"]["sc_gp_create_ext"], res["wall_ms"]["sc_gp_prove_ext"] = both(
        lambda: xg.ExtProductTree(ctx, w, table, alpha, beta), lambda t: xg.prove_ext(t, seed_r=7), EXT_KINDS)
    # the recorded bytes are the byte model's
    bt, bp, _ = model_bytes(n, T, lv, gp.TAIL_LOG, False)
    et, ep, ee = model_bytes(n, T, lv, xg.TAIL_LOG, True)
    kb, ke = res["base"]["kinds"], res["ext"]["kinds"]
    assert (kb["product_tree"]["bytes"], kb["product_pass"]["bytes"]) == (bt, bp), "base-field records against the byte model"
    assert (ke["ext_product_tree"]["bytes"], ke["ext_product_pass"]["bytes"], ke["ext_eq_table"]["bytes"]) == (et, ep, ee), "extension records against the byte model"
    res["model_bytes_ratio"] = (et + ep + ee) / (bt + bp)
    res["bytes_ratio"] = res["ext"]["bytes"] / res["base"]["bytes"]
    res["launch_ms_ratio"] = res["ext"]["launch_ms"] / res["base"]["launch_ms"]
    eq_ms = ke["ext_eq_table"]["launch_ms"]
    res["launch_ms_ratio_without_eq"] = (res["ext"]["launch_ms"] - eq_ms) / res["base"]["launch_ms"]
    proof_ms = eq_ms + ke["ext_product_pass"]["launch_ms"]
    res["eq_share_of_proof_launch_ms"] = eq_ms / proof_ms if proof_ms else 0.0
    del table
    ctx.close()
    return res


def summary(results, reps, prov):
    out = ["# The grand product argument over the quadratic extension on one MI355X (Goldilocks, w = 7)", "",
           "`tools/ext_grand_product_timing.py --reps %d`; sources %s, commit %s.  Launch times are medians over the runs, from the launch log; wall" % (
               reps, prov["csrc_sha16"], prov["commit"]),
           "times are the host clock around the call and a stream synchronisation.  The comparison is sc_gp_create + sc_gp_prove on the same",
           "table in the same process, at the default gp_host_log and gp_tree_lv.  The leaves are gamma - t (alpha = -1, beta in K).  The recorded",
           "bytes of both arguments equal the byte model's, launch by launch in total (asserted by the tool).  The base-field proof's eq tables",
           "leave no launch record; the extension's do, so the time ratio is given with and without them.  Shares are of the %.2f TB/s a" % COPY_TBS,
           "device-to-device copy reaches.  Nothing here is gated.", "",
           "| n | argument | launches | ms inside them | GiB moved (byte model) | TB/s | create wall ms | prove wall ms |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for name, key, cw, pw in (("sc_gp_*", "base", "sc_gp_create", "sc_gp_prove"), ("sc_gp_*_ext", "ext", "sc_gp_create_ext", "sc_gp_prove_ext")):
            x = r[key]
            out.append("| %d | %s | %d | %.3f | %.2f | %.3f | %.3f | %.3f |" % (r["n"], name, x["launches"], x["launch_ms"], x["bytes"] / 2**30, x["tb_s"],
                                                                            r["wall_ms"][cw]["median"], r["wall_ms"][pw]["median"]))
    out += ["", "| n | bytes, extension / base (= the byte model's) | time inside launches, extension / base | the same without the eq tables | eq tables' share of the proof's launch time |",
            "|---|---|---|---|---|"]
    for r in results:
        out.append("| %d | %.3f | %.3f | %.3f | %.1f %% |" % (r["n"], r["bytes_ratio"], r["launch_ms_ratio"], r["launch_ms_ratio_without_eq"],
                                                          100 * r["eq_share_of_proof_launch_ms"]))
    out += ["", "## Per launch kind (all launches; and those of at least 2^%d entries, which carry the rate)" % BIG, "",
            "| n | kind | launches | ms | TB/s | launches >= 2^%d | ms | TB/s | share of a copy |" % BIG, "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for key in ("base", "ext"):
            for kind, x in r[key]["kinds"].items():
                b = x["big"]
                out.append("| %d | %s | %d | %.3f | %.3f | %d | %.3f | %.3f | %.0f %% |" % (r["n"], kind, x["launches"], x["launch_ms"], x["tb_s"], b["launches"],
                                                                                       b["launch_ms"], b["tb_s"], 100 * b["tb_s"] / COPY_TBS))
    out += ["", "## The longest launches of the top layers", "", "| n | kind | kf | ks | log_in | us | TB/s |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for x in r["ext"]["largest"]:
            out.append("| %d | %s | %d | %d | %d | %.1f | %.2f |" % (r["n"], x["kind"], x["kf"], x["ks"], x["log_in"], 1e3 * x["ms"], x["tb_s"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,24,26,28")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results, skipped = [], []
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("ext_grand_product_timing", "python tools/ext_grand_product_timing.py --reps %d --sizes %s" % (args.reps, args.sizes))

    def write():
        with open(os.path.join(args.out, "ext_grand_product_summary.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results, "skipped": skipped}, f, indent=1)
        with open(os.path.join(args.out, "ext_grand_product_summary.md"), "w") as f:
            text = summary(results, args.reps, prov)
            for n, why in skipped:
                text += "\n\nn = %d was not measured: %s" % (n, why)
            f.write(text + "\n")
    for n in [int(x) for x in args.sizes.split(",") if x]:
        try:
            results.append(measure(pkg, n, args.reps))
        except pkg.SumcheckHipError as exc:      # (the pool does not hold it)
            skipped.append((n, str(exc)))
            print("n = %d: %s" % (n, exc), flush=True)
            write()
            continue
        r = results[-1]
        print("n = %d: %s bytes x %.3f (model %.3f), launch time x %.3f (x %.3f without eq), eq share %.1f %%" % (
            n, json.dumps(r["wall_ms"]), r["bytes_ratio"], r["model_bytes_ratio"], r["launch_ms_ratio"], r["launch_ms_ratio_without_eq"],
            100 * r["eq_share_of_proof_launch_ms"]), flush=True)
        write()


if __name__ == "__main__":
    main()
