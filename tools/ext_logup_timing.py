"""Device and wall time of LogUp's fraction sums over the quadratic extension on one MI355X, Goldilocks, w = 7, next to
sc_frac_create + sc_frac_prove on the materialised tables (q = beta0 - t by sc_table_affine) in the same process, in both numerator
forms (a table of multiplicities; all ones).  Medians over --reps runs (five by default), after one run that is not counted; launch
times from the launch log.  At n in --sizes: launches, time inside them, bytes against the byte model (the recorded bytes are
checked against the model computed here), TB/s per launch kind and of the planes-in fold alone, the eq table's share of a proof's
launch time, and the ratios of the two arguments in bytes and in time - the trees and the passes separately.  No number is gated.

The base-field proof's eq tables (eq_table_kernel) leave no launch record, the extension's do (SC_KIND_EXT_EQ_TABLE): the time ratio is
given with and without them.

  python tools/ext_logup_timing.py [--reps 5] [--sizes 20,24,28] [--out profiles]
writes <out>/ext_logup_summary.json and <out>/ext_logup_summary.md."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from ext_grand_product_timing import BIG, by_kind, totals  # noqa: E402
from grand_product_timing import COPY_TBS, logged, ms, rate  # noqa: E402

BASE_KINDS = ("fraction_tree", "fraction_pass")
EXT_KINDS = ("ext_fraction_tree", "ext_fraction_pass", "ext_eq_table")


def model_bytes(n, T, lv, tail, ext, ones):
    """(tree bytes, pass bytes, eq bytes) by the byte models of include/sumcheck_hip.h at fr_host_log = T, fr_tree_lv = lv"""
    word = 32 if ext else 16     # bytes of one entry of both trees
    tree, m = 0, n
    while True:
        step = min(lv, m - tail) if m > tail else 0
        tree += ((8 if ones else 16) if m == n else word) << m
        tree += (word << m) - (word << (m - step)) if step else (word << m) - word
        if not step:
            break
        m -= step
    passes = eq = 0
    te = max(T, 1)
    for k in range(T + 1, n):
        leaf = k == n - 1
        nt = 3 if ones and leaf else 5

        def read(i, base_words):
            if not ext:
                return (8 * nt) << i
            return (16 << i) + ((8 * (nt - 1) * (1 if base_words else 2)) << i)
        if ext:
            eq += 16 * k + (16 << k)
        passes += read(k, leaf)
        for j in range(1, k - te + 1):
            i = k - j + 1
            passes += read(i, leaf and j == 1) + (((16 if ext else 8) * nt) << (i - 1))
    return tree, passes, eq


def measure(pkg, n, reps, ones):
    lu, xl = pkg.logup, pkg.ext_logup
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    w = F.from_int(pkg.ext_field.nonresidue(F.p))
    table = pkg.DenseMultilinearExtension.generate(ctx, 1000 + n, n)
    numer = None if ones else pkg.DenseMultilinearExtension.generate(ctx, 2000 + n, n)
    T, lv = ctx.get_option("fr_host_log"), ctx.get_option("fr_tree_lv")
    minus_one, beta = F.neg(F.one), (F.from_int(123456789), F.from_int(987654321))     # a lookup's denominators alpha_c - t
    q = pkg.grand_product.table_affine(ctx, table, minus_one, beta[0])                 # the base-field argument reads a stored table
    res = {"n": n, "numerator": "ones" if ones else "table", "fr_host_log": T, "fr_tree_lv": lv, "wall_ms": {}}

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
        return out, ms(tree_walls), ms(proof_walls), records
    res["base"], res["wall_ms"]["sc_frac_create"], res["wall_ms"]["sc_frac_prove"], _ = both(
        lambda: lu.FractionTree(ctx, q, numer), lambda t: lu.prove(t, seed_r=7), BASE_KINDS)
    res["ext"], res["wall_ms"]["sc_frac_create_ext"], res["wall_ms"]["sc_frac_prove_ext"], records = both(
        lambda: xl.ExtFractionTree(ctx, w, numer, table, (minus_one, 0), beta), lambda t: xl.prove_ext(t, seed_r=7), EXT_KINDS)
    # the recorded bytes are the byte model's
    bt, bp, _ = model_bytes(n, T, lv, lu.TAIL_LOG, False, ones)
    et, ep, ee = model_bytes(n, T, lv, xl.TAIL_LOG, True, ones)
    kb, ke = res["base"]["kinds"], res["ext"]["kinds"]
    assert (kb["fraction_tree"]["bytes"], kb["fraction_pass"]["bytes"]) == (bt, bp), "base-field records against the byte model"
    assert (ke["ext_fraction_tree"]["bytes"], ke["ext_fraction_pass"]["bytes"], ke["ext_eq_table"]["bytes"]) == (et, ep, ee), "extension records against the byte model"
    res["model_bytes_ratio"] = (et + ep + ee) / (bt + bp)
    res["bytes_ratio"] = res["ext"]["bytes"] / res["base"]["bytes"]
    res["tree_bytes_ratio"], res["pass_bytes_ratio"] = et / bt, ep / bp
    res["launch_ms_ratio"] = res["ext"]["launch_ms"] / res["base"]["launch_ms"]
    res["tree_launch_ms_ratio"] = ke["ext_fraction_tree"]["launch_ms"] / kb["fraction_tree"]["launch_ms"]
    res["pass_launch_ms_ratio"] = ke["ext_fraction_pass"]["launch_ms"] / kb["fraction_pass"]["launch_ms"]
    eq_ms = ke["ext_eq_table"]["launch_ms"]
    res["launch_ms_ratio_without_eq"] = (res["ext"]["launch_ms"] - eq_ms) / res["base"]["launch_ms"]
    proof_ms = eq_ms + ke["ext_fraction_pass"]["launch_ms"]
    res["eq_share_of_proof_launch_ms"] = eq_ms / proof_ms if proof_ms else 0.0
    # the folds alone: planes in (every fold but the first of layer n - 1, which reads base words), at 2^BIG entries and more
    folds = [x for x in records if x["kind"] == "ext_fraction_pass" and x["kf"] == 1 and x["log_in"] >= min(BIG, n - 2)]
    res["planes_in_fold"] = totals([x for x in folds if x["log_in"] != n - 1])
    res["leaf_in_fold"] = totals([x for x in folds if x["log_in"] == n - 1])
    del table, numer, q
    ctx.close()
    return res


def summary(results, reps, prov):
    out = ["# LogUp's fraction sums over the quadratic extension on one MI355X (Goldilocks, w = 7)", "",
           "`tools/ext_logup_timing.py --reps %d`; sources %s, commit %s.  Launch times are medians over the runs, from the launch log; wall" % (
               reps, prov["csrc_sha16"], prov["commit"]),
           "times are the host clock around the call and a stream synchronisation.  The comparison is sc_frac_create + sc_frac_prove on the",
           "materialised tables (q = beta0 - t, stored) in the same process, at the default fr_host_log and fr_tree_lv.  The leaves are",
           "(p, alpha_c - t) (alpha = -1, beta = alpha_c in K), p a table or all ones.  The recorded bytes of both arguments equal the byte",
           "model's, launch by launch in total (asserted by the tool).  The base-field proof's eq tables leave no launch record; the extension's",
           "do, so the time ratio is given with and without them.  Shares are of the %.2f TB/s a device-to-device copy reaches.  Nothing here" % COPY_TBS,
           "is gated.", "",
           "| n | numerator | argument | launches | ms inside them | GiB moved (byte model) | TB/s | create wall ms | prove wall ms |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for name, key, cw, pw in (("sc_frac_*", "base", "sc_frac_create", "sc_frac_prove"), ("sc_frac_*_ext", "ext", "sc_frac_create_ext", "sc_frac_prove_ext")):
            x = r[key]
            out.append("| %d | %s | %s | %d | %.3f | %.2f | %.3f | %.3f | %.3f |" % (r["n"], r["numerator"], name, x["launches"], x["launch_ms"], x["bytes"] / 2**30,
                                                                                 x["tb_s"], r["wall_ms"][cw]["median"], r["wall_ms"][pw]["median"]))
    out += ["", "| n | numerator | bytes, ext / base (= the byte model's) | trees' bytes | passes' bytes | time inside launches, ext / base | trees | passes | all without the eq tables | eq tables' share of the proof's launch time |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        out.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f %% |" % (
            r["n"], r["numerator"], r["bytes_ratio"], r["tree_bytes_ratio"], r["pass_bytes_ratio"], r["launch_ms_ratio"], r["tree_launch_ms_ratio"],
            r["pass_launch_ms_ratio"], r["launch_ms_ratio_without_eq"], 100 * r["eq_share_of_proof_launch_ms"]))
    out += ["", "## The folds of the pass (launches of at least 2^%d entries)" % BIG, "",
            "| n | numerator | fold | launches | ms | TB/s | share of a copy |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for name, key in (("planes in", "planes_in_fold"), ("leaves in (layer n - 1, round 1)", "leaf_in_fold")):
            x = r[key]
            out.append("| %d | %s | %s | %d | %.3f | %.3f | %.0f %% |" % (r["n"], r["numerator"], name, x["launches"], x["launch_ms"], x["tb_s"], 100 * x["tb_s"] / COPY_TBS))
    out += ["", "## Per launch kind (all launches; and those of at least 2^%d entries, which carry the rate)" % BIG, "",
            "| n | numerator | kind | launches | ms | TB/s | launches >= 2^%d | ms | TB/s | share of a copy |" % BIG, "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for key in ("base", "ext"):
            for kind, x in r[key]["kinds"].items():
                b = x["big"]
                out.append("| %d | %s | %s | %d | %.3f | %.3f | %d | %.3f | %.3f | %.0f %% |" % (r["n"], r["numerator"], kind, x["launches"], x["launch_ms"], x["tb_s"],
                                                                                            b["launches"], b["launch_ms"], b["tb_s"], 100 * b["tb_s"] / COPY_TBS))
    out += ["", "## The longest launches of the top layers", "", "| n | numerator | kind | kf | ks | log_in | us | TB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for x in r["ext"]["largest"]:
            out.append("| %d | %s | %s | %d | %d | %d | %.1f | %.2f |" % (r["n"], r["numerator"], x["kind"], x["kf"], x["ks"], x["log_in"], 1e3 * x["ms"], x["tb_s"]))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,24,28")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results, skipped = [], []
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("ext_logup_timing", "python tools/ext_logup_timing.py --reps %d --sizes %s" % (args.reps, args.sizes))

    def write():
        with open(os.path.join(args.out, "ext_logup_summary.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results, "skipped": skipped}, f, indent=1)
        with open(os.path.join(args.out, "ext_logup_summary.md"), "w") as f:
            text = summary(results, args.reps, prov)
            for n, form, why in skipped:
                text += "\n\nn = %d (%s) was not measured: %s" % (n, form, why)
            f.write(text + "\n")
    for n in [int(x) for x in args.sizes.split(",") if x]:
        for ones in (False, True):
            try:
                results.append(measure(pkg, n, args.reps, ones))
            except pkg.SumcheckHipError as exc:      # (the pool does not hold it)
                skipped.append((n, "ones" if ones else "table", str(exc)))
                print("n = %d: %s" % (n, exc), flush=True)
                write()
                continue
            r = results[-1]
            print("n = %d, %s: %s bytes x %.3f (model %.3f), launch time x %.3f (trees x %.3f, passes x %.3f, x %.3f without eq), eq share %.1f %%, "
                  "planes-in fold %.3f TB/s" % (n, r["numerator"], json.dumps(r["wall_ms"]), r["bytes_ratio"], r["model_bytes_ratio"], r["launch_ms_ratio"],
                                                r["tree_launch_ms_ratio"], r["pass_launch_ms_ratio"], r["launch_ms_ratio_without_eq"],
                                                100 * r["eq_share_of_proof_launch_ms"], r["planes_in_fold"]["tb_s"]), flush=True)
            write()


if __name__ == "__main__":
    main()
