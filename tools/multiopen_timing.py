"""Device and wall time of the batched openings on one MI355X, Goldilocks.  Every figure stands beside what it is measured
against; the parent's own calls are the comparison.  Medians over --reps runs (five by default), after one run that is not counted:

  * sc_table_eq_sum at n in --sizes and count in 1, 7, 16: its one launch (SC_KIND_EQ_SUM) from the launch log and the wall time
    of the call, next to `count` calls of sc_table_eq at the same n - the only way to the same factors without it
  * sc_sumprod_prove at the same n and T = 5: launches, time inside them from the launch log, bytes per second against the byte
    model; next to sc_product3_prove on three tables of the same length
and once, at (s, m) = --whole, plain openings, in one process: r1cs.prove_and_verify_sublinear and its batched form step by step on
the host clock, split into the same parts; the openings' bytes both ways (ligero_pcs.opening_bytes, multiopen.batch_opening_bytes);
the host verifiers' time inside the openings both ways; and what the T sc_ligero_combine_rows calls of each joint opening cost.
No number is gated.

  python tools/multiopen_timing.py [--reps 5] [--sizes 23,25,27] [--whole 14,14] [--out profiles]
writes <out>/multiopen_timing.json and <out>/multiopen_summary.md."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
import provenance  # noqa: E402
from grand_product_timing import COPY_TBS, logged, ms, rate, wall_only  # noqa: E402
from spark_timing import Clock  # noqa: E402

QUERIES = 8
COUNTS = (1, 7, 16)
PAIRS = 5


def measure(pkg, n, reps):
    mo, sp = pkg.multiopen, pkg.spark
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    MLE = pkg.DenseMultilinearExtension
    res = {"n": n, "eq_sum": [], "wall_ms": {}}
    points = [[F.from_int(3 + 31 * k + i) for i in range(n)] for k in range(max(COUNTS))]
    coeffs = [F.from_int(7 + k) for k in range(max(COUNTS))]
    for count in COUNTS:
        _, log, walls = logged(ctx, lambda: mo.table_eq_sum(ctx, points[:count], coeffs[:count]), reps)
        x = rate(dict([y for y in log if y["kind"] == "eq_sum"][0]))
        x["count"] = count
        x["wall_ms"] = ms(walls)

        def eq_tables():
            for k in range(count):
                sp.table_eq(ctx, points[k])
        x["table_eq_calls_wall_ms"] = ms(wall_only(ctx, eq_tables, reps))
        x["g_entry_points_s"] = count * (1 << n) / (x["ms"] * 1e-3) / 1e9
        res["eq_sum"].append(x)
    a = [MLE.generate(ctx, 100 + k, n) for k in range(PAIRS)]
    b = [MLE.generate(ctx, 200 + k, n) for k in range(PAIRS)]
    _, log, walls = logged(ctx, lambda: mo.sumprod_prove(ctx, a, b, seed_r=7), reps)
    passes = [rate(dict(x)) for x in log if x["kind"] == "sumprod_pass"]
    res["wall_ms"]["sumprod_prove"] = ms(walls)
    moved = sum(x["bytes_read"] + x["bytes_written"] for x in passes)
    inside = sum(x["ms"] for x in passes)
    res["sumprod"] = {"pairs": PAIRS, "launches": len(passes), "launch_ms": inside, "bytes": moved, "tb_s": moved / (inside * 1e-3) / 1e12,
                      "first": passes[0], "second": passes[1]}
    _, log, walls = logged(ctx, lambda: sp.product3_prove(ctx, a[0], a[1], a[2], seed_r=7), reps)
    passes = [rate(dict(x)) for x in log if x["kind"] == "product_pass"]
    res["wall_ms"]["product3_prove"] = ms(walls)
    moved = sum(x["bytes_read"] + x["bytes_written"] for x in passes)
    inside = sum(x["ms"] for x in passes)
    res["product3"] = {"launches": len(passes), "launch_ms": inside, "bytes": moved, "tb_s": moved / (inside * 1e-3) / 1e12, "first": passes[0],
                       "second": passes[1]}
    del a, b
    ctx.close()
    return res


def whole_run(pkg, s, m, batched):
    """the sublinear argument over one synthetic instance, plain openings, Reed-Solomon rows, step by step: with the nine single
    openings and the opening of w, or with batched openings"""
    sp, rp, lp, mo = pkg.spark, pkg.r1cs, pkg.ligero_pcs, pkg.multiopen
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
    instance = dev.commit_instance()
    prover = rp.Prover(ctx, dev, io, w, log_cols=c, log_blowup=1)
    pv = lp.Verifier(F, m - 1, c, 1, prover.root(), QUERIES)
    V = rp.SublinearVerifier(F, s, m, io, prover.root(), pv, instance.verifiers(QUERIES))
    rng, vc, oc, cc = random.Random(1), Clock(), Clock(), Clock()      # the verifiers outside the openings; inside them; the combine calls
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
    fractions = 0.0
    for dim in sp.DIMS:
        roots = timed("denominators and trees, %s" % dim, lambda: P.lookup_roots(dim, alpha, beta))
        vc(S.receive_roots)(dim, *roots)
        for side, name in enumerate(("w", "t")):
            timed("fraction sum, %s, %s side" % (dim, name), lambda: P.lookup_prove(dim, side, vc(S.frac[dim][side].challenger(rng))))
            fractions += steps[-1]["ms"]
    out = {"s": s, "m": m, "nnz": sum(len(M) for M in R.matrices), "l": instance.ell, "batched": batched}

    def single(pr, ver, point):
        gamma = oc(ver.draw_gamma)(rng)
        oc(ver.receive)(*pr.combine(point, gamma))
        return oc(ver.verify)(point, pr.open_columns(oc(ver.draw_columns)(rng)))
    if not batched:
        opened = {}

        def open_all():
            for table, at, point in S.openings():
                ver = S.pcs[table] if table in sp.TABLES else sp.opening_verifier(F, P.pcs[table], QUERIES)
                opened[(table, at)] = single(P.pcs[table], ver, point)
        timed("nine openings (both sides)", open_all)
        vc(S.finish)(opened)
        w_value = timed("opening of w (both sides)", lambda: single(prover.pcs, pv, V.point()))
        assert vc(V.finish)(w_value, S.v) is True
        shapes = [(P.pcs[t].num_vars, P.pcs[t].log_cols) for t, _ in sp.OPENINGS] + [(m - 1, c)]
        out["opening_bytes"] = sum(lp.opening_bytes(nv, lc, 1, QUERIES) for nv, lc in shapes)
        out["openings_ms"] = steps[-2]["ms"] + steps[-1]["ms"]
    else:
        tables = dict(instance.tables, er=P.er, ec=P.ec)
        point_w = V.point()
        claims = timed("the ten values (P evaluates its tables)", lambda: [mo.Claim(t, pt, tables[t].evaluate(pt)) for t, _, pt in S.openings()]
                       + [mo.Claim("w", point_w, prover.pcs.poly.evaluate(point_w))])
        vc(S.finish)({key: cl.value for key, cl in zip(sp.OPENINGS, claims)})
        assert vc(V.finish)(claims[-1].value, S.v) is True
        provers, verifiers = dict(P.pcs, w=prover.pcs), dict(S.pcs, w=pv)
        shapes = {t: (v.num_vars, v.log_cols, v.log_blowup, v.code) for t, v in verifiers.items()}
        groups, out["opening_bytes"], combine_launch_ms = [], 0, []

        def open_groups():
            for shape, names, group in mo.group_claims(claims, shapes):
                groups.append({"tables": list(names), "claims": len(group), "num_vars": shape[0], "log_cols": shape[1]})
                if len(group) == 1:
                    assert single(provers[names[0]], verifiers[names[0]], group[0].point) == group[0].value
                    out["opening_bytes"] += lp.opening_bytes(shape[0], shape[1], 1, QUERIES)
                    continue
                out["opening_bytes"] += mo.batch_opening_bytes(shape[0], shape[1], 1, QUERIES, len(names))
                GV = mo.Verifier(F, shape[:3], {t: verifiers[t].root for t in names}, QUERIES, shape[3])
                GP = mo.Prover(ctx, {t: provers[t] for t in names})
                try:
                    GP.begin(group, oc(GV.draw_rho)(group, rng), names)
                    GP.sumcheck(oc(lambda j, e: GV.round(j, e, rng)))
                    gamma = oc(GV.draw_gamma)(rng)
                    ctx.synchronize()
                    ctx.set_option("time_kernels", 1)
                    ctx.launch_log()
                    rows = cc(lambda: (GP.combine(gamma), ctx.synchronize())[0])()
                    combine_launch_ms.append(sum(x["ms"] for x in ctx.launch_log() if x["kind"] == "ligero"))
                    ctx.set_option("time_kernels", 0)
                    oc(GV.receive)(*rows)
                    oc(GV.verify)(GP.open_columns(oc(GV.draw_columns)(rng)))
                finally:
                    GP.close()
        timed("all openings, batched (both sides)", open_groups)
        out["groups"] = groups
        out["openings_ms"] = steps[-1]["ms"] + steps[-2]["ms"]
        out["combine_calls_wall_ms"] = 1e3 * cc.s
        out["combine_launch_ms"] = sum(combine_launch_ms)
    P.close()
    prover.close()
    instance.close()
    dev.close()
    ctx.close()
    out.update(steps=steps, total_ms=sum(x["ms"] for x in steps), fractions_ms=fractions, verifier_own_ms=1e3 * vc.s,
               verifier_in_openings_ms=1e3 * oc.s)
    return out


def summary(results, whole, reps, prov):
    out = ["# Batched openings on one MI355X (Goldilocks)", "",
           "`tools/multiopen_timing.py --reps %d`; sources %s, commit %s.  Launch times are medians over the runs, from the launch log; wall" % (
               reps, prov["csrc_sha16"], prov["commit"]),
           "times are the host clock around the call and a stream synchronisation.  Nothing here is gated.", ""]
    for r in results:
        out += ["## n = %d" % r["n"], "", "| sc_table_eq_sum | launch us | G entry-points/s | write TB/s | call wall ms | `count` sc_table_eq calls, wall ms |",
                "|---|---|---|---|---|---|"]
        for x in r["eq_sum"]:
            out.append("| count = %d | %.1f | %.1f | %.3f | %.3f | %.3f |" % (x["count"], 1e3 * x["ms"], x["g_entry_points_s"], x["tb_s"], x["wall_ms"]["median"],
                                                                              x["table_eq_calls_wall_ms"]["median"]))
        a, b = r["sumprod"], r["product3"]
        out += ["", "| proof | tables | launches | ms inside them | GiB moved (byte model) | TB/s | share of %.2f TB/s | round 0 us / TB/s | round 1 us / TB/s | call wall ms |" % COPY_TBS,
                "|---|---|---|---|---|---|---|---|---|---|"]
        for name, x, tabs, key in (("sc_sumprod_prove, T = %d" % a["pairs"], a, 2 * a["pairs"], "sumprod_prove"), ("sc_product3_prove", b, 3, "product3_prove")):
            out.append("| %s | %d | %d | %.3f | %.2f | %.3f | %.1f %% | %.1f / %.2f | %.1f / %.2f | %.3f |" % (
                name, tabs, x["launches"], x["launch_ms"], x["bytes"] / 2**30, x["tb_s"], 100 * x["tb_s"] / COPY_TBS, 1e3 * x["first"]["ms"], x["first"]["tb_s"],
                1e3 * x["second"]["ms"], x["second"]["tb_s"], r["wall_ms"][key]["median"]))
        out.append("")
    if whole:
        one, bat = whole
        out += ["## The whole argument at (s, m) = (%d, %d), nnz = %d, l = %d: one run each on the host clock, plain openings, one process" % (
            one["s"], one["m"], one["nnz"], one["l"]), "", "| part | prove_and_verify_sublinear, ms | batched form, ms |", "|---|---|---|"]
        pick = lambda r, pre: sum(x["ms"] for x in r["steps"] if x["step"].startswith(pre))   # noqa: E731
        for name, pre in (("sumcheck 1", "sumcheck 1"), ("bind_rows", "bind_rows"), ("sumcheck 2", "sumcheck 2"), ("row weights and eq(r_y, .)", "row weights"),
                          ("gather and commit er, ec", "gather"), ("triple-product sumcheck", "triple"), ("denominators and trees", "denominators"),
                          ("the four fraction sums", "fraction sum")):
            out.append("| %s | %.3f | %.3f |" % (name, pick(one, pre), pick(bat, pre)))
        out += ["| the openings, both sides (batched: the ten values, then the groups) | %.3f | %.3f |" % (one["openings_ms"], bat["openings_ms"]),
                "| total | %.3f | %.3f |" % (one["total_ms"], bat["total_ms"]), "",
                "Bytes of the openings: %d from ligero_pcs.opening_bytes over the ten single openings; %d batched (multiopen.batch_opening_bytes per joint "
                "opening, opening_bytes per single one)." % (one["opening_bytes"], bat["opening_bytes"]), "",
                "Host verifiers' time inside the openings: %.3f ms single, %.3f ms batched; outside them %.3f and %.3f ms." % (
                    one["verifier_in_openings_ms"], bat["verifier_in_openings_ms"], one["verifier_own_ms"], bat["verifier_own_ms"]), "",
                "The groups: " + "; ".join("%s (%d claims, n = %d, c = %d)" % (", ".join(g["tables"]), g["claims"], g["num_vars"], g["log_cols"]) for g in bat["groups"]) + ".",
                "", "The sc_ligero_combine_rows calls of the joint openings, one per commitment: %.3f ms on the host clock (with the host additions), %.3f ms "
                "inside their launches." % (bat["combine_calls_wall_ms"], bat["combine_launch_ms"]), ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="23,25,27")
    ap.add_argument("--whole", default="14,14")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results, whole = [], None
    os.makedirs(args.out, exist_ok=True)
    prov = provenance.record("multiopen_timing", "python tools/multiopen_timing.py --reps %d --sizes %s --whole %s" % (args.reps, args.sizes, args.whole))

    def write():
        with open(os.path.join(args.out, "multiopen_timing.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "provenance": prov, "results": results, "whole": whole}, f, indent=1)
        with open(os.path.join(args.out, "multiopen_summary.md"), "w") as f:
            f.write(summary(results, whole, args.reps, prov) + "\n")
    if args.whole:
        s, m = (int(x) for x in args.whole.split(","))
        whole_run(pkg, s, m, True)                       # (one run that is not counted: first-use costs of the process)
        whole = [whole_run(pkg, s, m, False), whole_run(pkg, s, m, True)]
        print("whole (%d, %d): single %.1f ms, batched %.1f ms" % (s, m, whole[0]["total_ms"], whole[1]["total_ms"]), flush=True)
        write()
    for n in [int(x) for x in args.sizes.split(",") if x]:
        results.append(measure(pkg, n, args.reps))
        print("n = %d: %s" % (n, json.dumps(results[-1]["wall_ms"])), flush=True)
        write()


if __name__ == "__main__":
    main()
