"""Device and wall time of SPARK over LogUp on one MI355X, Goldilocks, over r1cs.synthetic_instance's shape at
(s, m) = (20, 20), (22, 22), (24, 24): the one combined matrix of 2^(s+2) x 2^m with 7 * 2^s entries (row k 2^s + i = row i of
matrix k), built with numpy as tools/r1cs_timing.py builds its instance.

Per size, medians over --reps runs:
  * sc_spark_create: wall, and its launches (SC_KIND_SPARK_INDEX) from the launch log
  * the gather (SC_KIND_SPARK_GATHER) in G entries/s, next to sc_r1cs_bind_rows on the same entries in the same process - the
    parent's nearest equivalent, a gather plus a segmented sum (its SC_KIND_SPMV product launch)
  * the tuple launches (SC_KIND_SPARK_TUPLE) next to sc_table_affine on tables of the same lengths
  * sc_product3_prove next to sc_zerocheck_prove(a, b, zero table) on tables of the same length
and once, at (s, m) = --whole (the lists of triples of the host instance bound its size): r1cs.prove_and_verify_sublinear step by
step on the host clock next to r1cs.prove_and_verify, and the verifier's own time (every call into the two verifiers but the
openings) next to R1CS.bind_eval.  No number is gated.

  python tools/spark_timing.py [--reps 5] [--sizes 20,22,24] [--whole 14,14] [--out profiles]
writes <out>/spark_timing.json and <out>/spark_summary.md."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from grand_product_timing import COPY_TBS, logged, ms, rate, wall_only  # noqa: E402
from r1cs_timing import ROW_NNZ  # noqa: E402

QUERIES = 8


def build_instance(pkg, ctx, s, m, seed):
    """(device instance, the combined matrix's rows, cols, vals): tools/r1cs_timing.py's instance, whose C values come from the
    device's own A z and B z"""
    rp, F = pkg.r1cs, ctx.field
    p = F.p
    rng = np.random.default_rng(seed)
    n_rows, n_cols, half = 1 << s, 1 << m, 1 << (m - 1)
    z = np.zeros(n_cols, dtype=np.uint64)
    z[0] = F.one
    z[half:] = rng.integers(0, p, size=half, dtype=np.uint64)
    rows = np.repeat(np.arange(n_rows, dtype=np.uint32), ROW_NNZ)
    AB = [(rows, rng.integers(0, n_cols, size=rows.size, dtype=np.uint32), rng.integers(0, p, size=rows.size, dtype=np.uint64)) for _ in range(2)]
    empty = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    zt = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m, z)
    probe = rp.DeviceR1CS.from_arrays(ctx, s, m, AB + [empty])
    az, bz, _ = probe.mul(zt)
    a, b = az.to_evaluations().astype(object), bz.to_evaluations().astype(object)
    probe.close()
    cvals = (a * b * pow(2**64, -1, p) % p).astype(np.uint64)
    crow = np.arange(n_rows, dtype=np.uint32)
    mats = AB + [(crow, np.zeros(n_rows, dtype=np.uint32), cvals)]
    dense = rp.DeviceR1CS.from_arrays(ctx, s, m, mats)
    comb_rows = np.concatenate([M[0] + np.uint32(k << s) for k, M in enumerate(mats)])
    return dense, comb_rows, np.concatenate([M[1] for M in mats]), np.concatenate([M[2] for M in mats])


def measure(pkg, s, m, reps):
    sp, rp, gp = pkg.spark, pkg.r1cs, pkg.grand_product
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    MLE = pkg.DenseMultilinearExtension
    dense, rows, cols, vals = build_instance(pkg, ctx, s, m, 1000 + s)
    nnz, ell = int(rows.size), sp.log_len(rows.size)
    res = {"s": s, "m": m, "a": s + 2, "b": m, "nnz": nnz, "l": ell, "wall_ms": {}}
    keep = []

    def create():
        for x in keep:
            x.close()
        keep[:] = [sp.SparseCommitment(ctx, s + 2, m, rows, cols, vals, commit=False)]
    _, log, walls = logged(ctx, create, reps)
    res["wall_ms"]["spark_create"] = ms(walls)
    res["create"] = [x for x in log if x["kind"] == "spark_index"]
    sc = keep[0]
    rx, ry = [F.from_int(3 + i) for i in range(s)], [F.from_int(5 + i) for i in range(m)]
    rho = [F.from_int(5), F.from_int(6), F.from_int(7)]
    U, W = dense.row_weights(rx, rho), sp.table_eq(ctx, ry)
    # the gather, next to bind_rows over the same entries
    (er, ec), log, walls = logged(ctx, lambda: sp.gather(ctx, sc, U, W), reps)
    g = [x for x in log if x["kind"] == "spark_gather"][0]
    res["wall_ms"]["gather"] = ms(walls)
    res["gather"] = dict(g, entries=1 << ell, g_entries_s=(1 << ell) / (g["ms"] * 1e-3) / 1e9)
    _, log, walls = logged(ctx, lambda: dense.bind_rows(rx, rho), reps)
    y = [x for x in log if x["kind"] == "spmv" and x["kf"] == 0][0]
    res["wall_ms"]["bind_rows"] = ms(walls)
    res["bind_rows"] = dict(y, entries=nnz, g_entries_s=nnz / (y["ms"] * 1e-3) / 1e9)
    # the tuples, next to table_affine
    alpha, beta = F.from_int(123456789), F.from_int(987654321)
    _, log, walls = logged(ctx, lambda: sp.denominators(ctx, sc, "row", U, er, alpha, beta), reps)
    res["wall_ms"]["denominators_row"] = ms(walls)
    res["tuple"] = [rate(dict(x)) for x in log if x["kind"] == "spark_tuple"]
    res["affine"] = []
    for t in (er, U):
        walls = wall_only(ctx, lambda: gp.table_affine(ctx, t, alpha, beta), reps)
        res["affine"].append({"log_in": t.num_vars(), "wall_ms": ms(walls)})
    # the triple-product proof, next to the zerocheck over tables of the same length
    val = sc.table("val")
    _, log, walls = logged(ctx, lambda: sp.product3_prove(ctx, val, er, ec, seed_r=7), reps)
    res["wall_ms"]["product3_prove"] = ms(walls)
    res["product3"] = {"launches": len([x for x in log if x["kind"] == "product_pass"]), "launch_ms": sum(x["ms"] for x in log if x["kind"] == "product_pass")}
    zero = MLE.from_evaluations_vec(ctx, ell, np.zeros(1 << ell, dtype=np.uint64))
    tau = [F.from_int(9 + i) for i in range(ell)]
    _, log, walls = logged(ctx, lambda: rp.zerocheck_prove(ctx, er, ec, zero, tau, None, seed_r=7), reps)
    res["wall_ms"]["zerocheck_prove"] = ms(walls)
    res["zerocheck"] = {"launches": len([x for x in log if x["kind"] == "zerocheck"]), "launch_ms": sum(x["ms"] for x in log if x["kind"] == "zerocheck")}
    sc.close()
    dense.close()
    ctx.close()
    return res


class Clock:
    """the host time spent inside the calls it wraps"""

    def __init__(self):
        self.s = 0.0

    def __call__(self, fn):
        def timed(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kwargs)
            finally:
                self.s += time.perf_counter() - t0
        return timed


def whole_run(pkg, s, m):
    """both arguments over one synthetic instance, plain openings, Reed-Solomon rows; the sublinear one step by step"""
    sp, rp, lp = pkg.spark, pkg.r1cs, pkg.ligero_pcs
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    R, io, w = rp.synthetic_instance(F, s, m, 5)
    dev = rp.DeviceR1CS(ctx, R)
    steps, c = [], m // 2

    def timed(name, fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        steps.append({"step": name, "ms": 1e3 * (time.perf_counter() - t0)})
        return out

    def sides():
        prover = rp.Prover(ctx, dev, io, w, log_cols=c, log_blowup=1)
        return prover, lp.Verifier(F, m - 1, c, 1, prover.root(), QUERIES)
    # the argument whose verifier reads the instance
    prover, pv = sides()
    verifier = rp.Verifier(R, io, prover.root(), pv)
    t0 = time.perf_counter()
    assert rp.prove_and_verify(prover, verifier, random.Random(1)) is True
    ctx.synchronize()
    plain_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = R.bind_eval(verifier.rx, verifier.ry, verifier.rho)
    bind_eval_ms = 1e3 * (time.perf_counter() - t0)
    prover.close()
    # the sublinear one
    instance = timed("commit the instance (once per matrix)", lambda: dev.commit_instance())
    prover, pv = sides()
    V = rp.SublinearVerifier(F, s, m, io, prover.root(), pv, instance.verifiers(QUERIES))
    rng, vc = random.Random(1), Clock()
    fin = timed("sumcheck 1", lambda: prover.sumcheck1(vc(V.draw_tau)(rng), vc(lambda j, e: V.round1(j, e, rng))))
    vc(V.receive_finals)(*fin)
    rho = vc(V.draw_rho)(rng)
    timed("bind_rows", lambda: prover.bind(rho))
    timed("sumcheck 2", lambda: prover.sumcheck2(vc(lambda j, e: V.round2(j, e, rng))))
    U, W = timed("row weights and eq(r_y, .)", lambda: (dev.row_weights(prover.rx, rho), sp.table_eq(ctx, prover.ry)))
    S = sp.Verifier(F, instance.a, instance.b, instance.ell, V.instance_pcs, vc(V.u_eval), vc(V.w_eval))
    P = sp.Prover(instance, U, W)
    timed("gather and commit er, ec", P.gather_commit)
    vc(S.receive_commitments)(sp.opening_verifier(F, P.pcs["er"], QUERIES), sp.opening_verifier(F, P.pcs["ec"], QUERIES))
    fin = timed("triple-product sumcheck", lambda: P.sumcheck(vc(S.receive_claim), vc(lambda j, e: S.round(j, e, rng))))
    vc(S.receive_finals)(*fin)
    alpha, beta = vc(S.draw_lookup)(rng)
    for dim in sp.DIMS:
        roots = timed("denominators and trees, %s" % dim, lambda: P.lookup_roots(dim, alpha, beta))
        vc(S.receive_roots)(dim, *roots)
        for side, name in enumerate(("w", "t")):
            timed("fraction sum, %s, %s side" % (dim, name), lambda: P.lookup_prove(dim, side, vc(S.frac[dim][side].challenger(rng))))
    opened = {}

    def open_all():
        for table, at, point in S.openings():
            ver = S.pcs[table] if table in sp.TABLES else sp.opening_verifier(F, P.pcs[table], QUERIES)
            opened[(table, at)] = rp.open_committed(P.pcs[table], ver, point, rng)
    timed("nine openings (both sides)", open_all)
    vc(S.finish)(opened)
    assert S.v == want, "the SPARK exchange hands over T~(r_y)"
    w_value = timed("opening of w (both sides)", lambda: rp.open_committed(prover.pcs, pv, V.point(), rng))
    assert vc(V.finish)(w_value, S.v) is True
    P.close()
    prover.close()
    instance.close()
    dev.close()
    ctx.close()
    return {"s": s, "m": m, "nnz": sum(len(M) for M in R.matrices), "l": instance.ell, "steps": steps, "sublinear_ms": sum(x["ms"] for x in steps[1:]),
            "prove_and_verify_ms": plain_ms, "verifier_own_ms": 1e3 * vc.s, "bind_eval_ms": bind_eval_ms}


def summary(results, whole, reps):
    out = ["# SPARK over LogUp on one MI355X (Goldilocks)", "",
           "`tools/spark_timing.py --reps %d`; launch times are medians over the runs, from the launch log; wall times are the host" % reps,
           "clock around the call and a stream synchronisation.  Nothing here is gated.", ""]
    for r in results:
        out += ["## (s, m) = (%d, %d): 2^%d x 2^%d, nnz = %d, l = %d" % (r["s"], r["m"], r["a"], r["b"], r["nnz"], r["l"]), "",
                "| launch | kf | ks | log_in | MiB moved | us | TB/s | share of %.2f TB/s |" % COPY_TBS, "|---|---|---|---|---|---|---|---|"]
        for name, xs in (("spark_index", r["create"]), ("spark_tuple", r["tuple"])):
            for x in xs:
                x = rate(dict(x))
                out.append("| %s | %d | %d | %d | %.1f | %.1f | %.3f | %.1f %% |" % (name, x["kf"], x["ks"], x["log_in"], (x["bytes_read"] + x["bytes_written"]) / 2**20,
                                                                                   1e3 * x["ms"], x["tb_s"], 100 * x["share_of_copy"]))
        g, y = r["gather"], r["bind_rows"]
        out += ["", "Gather, both dimensions in one launch: %d entries in %.1f us, %.2f G entries/s.  sc_r1cs_bind_rows' product launch over the same matrix: "
                "%d entries in %.1f us, %.2f G entries/s." % (g["entries"], 1e3 * g["ms"], g["g_entries_s"], y["entries"], 1e3 * y["ms"], y["g_entries_s"]), "",
                "sc_table_affine on tables of the tuples' lengths, wall ms (median): " +
                ", ".join("2^%d: %.3f" % (x["log_in"], x["wall_ms"]["median"]) for x in r["affine"]) + ".", "",
                "sc_product3_prove: %d launches, %.3f ms inside them; sc_zerocheck_prove(er, ec, zero): %d launches, %.3f ms inside them." % (
                    r["product3"]["launches"], r["product3"]["launch_ms"], r["zerocheck"]["launches"], r["zerocheck"]["launch_ms"]), "",
                "| call | wall ms, median | min |", "|---|---|---|"]
        out += ["| %s | %.3f | %.3f |" % (k, v["median"], v["min"]) for k, v in r["wall_ms"].items()]
        out.append("")
    if whole:
        out += ["## The whole argument at (s, m) = (%d, %d), nnz = %d, l = %d: one run on the host clock, plain openings" % (whole["s"], whole["m"], whole["nnz"], whole["l"]),
                "", "| step of prove_and_verify_sublinear | ms |", "|---|---|"]
        out += ["| %s | %.3f |" % (x["step"], x["ms"]) for x in whole["steps"]]
        out += ["| total without the commitment to the instance | %.3f |" % whole["sublinear_ms"], "",
                "prove_and_verify on the same instance: %.3f ms.  The verifiers' own host time in the sublinear run, every call but the openings: %.3f ms; "
                "R1CS.bind_eval, which it replaces: %.3f ms." % (whole["prove_and_verify_ms"], whole["verifier_own_ms"], whole["bind_eval_ms"]), ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--whole", default="14,14")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results, whole = [], None
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("spark_timing", "python tools/spark_timing.py --reps %d --sizes %s --whole %s" % (args.reps, args.sizes, args.whole))

    def write():
        with open(os.path.join(args.out, "spark_timing.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results, "whole": whole}, f, indent=1)
        with open(os.path.join(args.out, "spark_summary.md"), "w") as f:
            f.write(summary(results, whole, args.reps) + "\n")
    if args.whole:
        s, m = (int(x) for x in args.whole.split(","))
        whole = whole_run(pkg, s, m)
        print("whole (%d, %d): sublinear %.1f ms, plain %.1f ms" % (s, m, whole["sublinear_ms"], whole["prove_and_verify_ms"]), flush=True)
        write()
    for n in [int(x) for x in args.sizes.split(",") if x]:
        results.append(measure(pkg, n, n, args.reps))
        print("(%d, %d): %s" % (n, n, json.dumps(results[-1]["wall_ms"])), flush=True)
        write()


if __name__ == "__main__":
    main()
