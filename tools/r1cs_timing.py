"""Device and wall time of the R1CS argument's prover steps on one MI355X, Goldilocks, over r1cs.synthetic_instance's shape at
(s, m) = (20, 20), (22, 22), (24, 24): A and B with three random entries per row, C with one entry per row at column 0 - the dense
constant column - and the value (A z)_i (B z)_i.  The instance is built with numpy (the lists of triples of synthetic_instance
are out of reach at these sizes); the C values come from the device's own A z and B z.

Per size, from the launch log (option time_kernels), the median of --reps runs of each launch:
  * every cubic launch (SC_KIND_ZEROCHECK): bytes, time, rate, and the rate as a share of the tree's 6.29 TB/s copy figure
  * the sparse products (SC_KIND_SPMV) in both directions, product and carry launch, with nnz/s
  * bind_rows at the dense constant column beside a variant of the same instance whose C column is spread out (entry i at
    column i mod 2^m; that variant is not satisfied - only its bind_rows is timed)
and on the host clock: commit of w, mul, the cubic sumcheck, bind_rows, sc_prove(T, z) - beside sc_prove on two generated tables
of 2^m entries in the same process - and one plain opening of w.

  python tools/r1cs_timing.py [--reps 5] [--sizes 20,22,24] [--out profiles]
writes <out>/r1cs_timing.json and <out>/r1cs_summary.md."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

COPY_TBS = 6.29
ROW_NNZ = 3


def build_instance(pkg, ctx, s, m, seed):
    """(device instance, spread variant, z table, w table, nnz per matrix)"""
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
    wt = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m - 1, z[half:].copy())
    probe = rp.DeviceR1CS.from_arrays(ctx, s, m, AB + [empty])
    az, bz, _ = probe.mul(zt)
    a, b = az.to_evaluations().astype(object), bz.to_evaluations().astype(object)
    probe.close()
    cvals = (a * b * pow(2**64, -1, p) % p).astype(np.uint64)       # the Montgomery product, times z[0] = 1
    crow = np.arange(n_rows, dtype=np.uint32)
    dense = rp.DeviceR1CS.from_arrays(ctx, s, m, AB + [(crow, np.zeros(n_rows, dtype=np.uint32), cvals)])
    spread = rp.DeviceR1CS.from_arrays(ctx, s, m, AB + [(crow, (crow % n_cols).astype(np.uint32), cvals)])
    return dense, spread, zt, wt, [rows.size, rows.size, n_rows]


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


def measure(pkg, s, m, reps):
    rp, lp, mm = pkg.r1cs, pkg.ligero_pcs, pkg.matrix_multiplication
    F = pkg.Field(pkg.GOLDILOCKS)
    ctx = pkg.Context(F)
    t0 = time.perf_counter()
    dense, spread, zt, wt, nnz = build_instance(pkg, ctx, s, m, 1000 + s)
    build_s = time.perf_counter() - t0
    res = {"s": s, "m": m, "nnz": nnz, "build_s": build_s, "wall_ms": {}}

    def ms(walls):
        return {"median": 1e3 * statistics.median(walls), "min": 1e3 * min(walls)}
    tabs, log, walls = logged(ctx, lambda: dense.mul(zt), reps)
    res["wall_ms"]["mul"] = ms(walls)
    res["mul"] = [x for x in log if x["kind"] == "spmv"]
    az, bz, cz = tabs
    tau = [F.from_int(3 + i) for i in range(s)]
    zc, log, walls = logged(ctx, lambda: rp.zerocheck_prove(ctx, az, bz, cz, tau, None, seed_r=7), reps)
    assert zc[0] == 0, "the instance is satisfied: c1 must be 0"
    res["wall_ms"]["zerocheck"] = ms(walls)
    res["zerocheck"] = [x for x in log if x["kind"] == "zerocheck"]
    rx, rho = zc[2], [F.from_int(5), F.from_int(6), F.from_int(7)]
    T, log, walls = logged(ctx, lambda: dense.bind_rows(rx, rho), reps)
    res["wall_ms"]["bind_rows"] = ms(walls)
    res["bind_rows_dense_column"] = [x for x in log if x["kind"] == "spmv"]
    _, log, walls = logged(ctx, lambda: spread.bind_rows(rx, rho), reps)
    res["wall_ms"]["bind_rows_spread"] = ms(walls)
    res["bind_rows_spread_column"] = [x for x in log if x["kind"] == "spmv"]
    g = mm.G(T, zt)
    res["wall_ms"]["sc_prove_T_z"] = ms(wall_only(ctx, lambda: mm.prove(ctx, g, 11), reps))
    ga = mm.G(pkg.DenseMultilinearExtension.generate(ctx, 1, m), pkg.DenseMultilinearExtension.generate(ctx, 2, m))
    res["wall_ms"]["sc_prove_generated"] = ms(wall_only(ctx, lambda: mm.prove(ctx, ga, 11), reps))
    keep = []

    def commit():
        for pr in keep:
            pr.close()
        keep[:] = [lp.Prover.commit(ctx, wt)]
    res["wall_ms"]["commit_w"] = ms(wall_only(ctx, commit, reps))
    pcs = keep[0]
    res["commit_shape"] = {"num_vars": pcs.num_vars, "log_cols": pcs.log_cols, "log_blowup": pcs.log_blowup}
    point = [F.from_int(9 + i) for i in range(m - 1)]
    gamma = [F.from_int(2 + i) for i in range(1 << pcs.log_rows)]
    res["wall_ms"]["open_w_8_columns"] = ms(wall_only(ctx, lambda: (pcs.combine(point, gamma), pcs.open_columns(list(range(8)))), reps))
    pcs.close()
    for x in res["zerocheck"]:
        x["tb_s"] = (x["bytes_read"] + x["bytes_written"]) / (x["ms"] * 1e-3) / 1e12
        x["share_of_copy"] = x["tb_s"] / COPY_TBS
    for key, n in (("mul", None), ("bind_rows_dense_column", sum(nnz)), ("bind_rows_spread_column", sum(nnz))):
        k = 0
        for x in res[key]:
            if x["kf"] == 0:
                x["nnz"] = n if n is not None else nnz[k]
                k += 1
                x["gnnz_s"] = x["nnz"] / (x["ms"] * 1e-3) / 1e9
    dense.close()
    spread.close()
    ctx.close()
    return res


def summary(results, reps):
    out = ["# R1CS argument: prover steps on one MI355X (Goldilocks)", "",
           "`tools/r1cs_timing.py --reps %d`; the launch times are medians over the runs, from the launch log." % reps, ""]
    for r in results:
        out += ["## (s, m) = (%d, %d), nnz = %s" % (r["s"], r["m"], r["nnz"]), "", "Cubic launches (SC_KIND_ZEROCHECK):", "",
                "| round | log_in | folded | MiB moved | us | TB/s | share of %.2f TB/s |" % COPY_TBS, "|---|---|---|---|---|---|---|"]
        for j, x in enumerate(r["zerocheck"]):
            out.append("| %d | %d | %d | %.3f | %.1f | %.3f | %.1f %% |" % (j, x["log_in"], x["kf"], (x["bytes_read"] + x["bytes_written"]) / 2**20,
                                                                          1e3 * x["ms"], x["tb_s"], 100 * x["share_of_copy"]))
        out += ["", "Sparse products (SC_KIND_SPMV; kf 0 = product with the zeroing of its output, 1 = carries):", "",
                "| call | transposed | kf | nnz | us | Gnnz/s |", "|---|---|---|---|---|---|"]
        for key in ("mul", "bind_rows_dense_column", "bind_rows_spread_column"):
            for x in r[key]:
                out.append("| %s | %d | %d | %s | %.1f | %s |" % (key, x["ks"], x["kf"], x.get("nnz", ""), 1e3 * x["ms"],
                                                                  "%.2f" % x["gnnz_s"] if "gnnz_s" in x else ""))
        d = sum(x["ms"] for x in r["bind_rows_dense_column"])
        sp = sum(x["ms"] for x in r["bind_rows_spread_column"])
        out += ["", "bind_rows, both launches: %.1f us at the dense constant column, %.1f us with the column spread out (x %.2f)." % (1e3 * d, 1e3 * sp, d / sp),
                "", "Wall time of the steps (ms, median / min), commitment shape %s:" % r["commit_shape"], "", "| step | median | min |", "|---|---|---|"]
        for k, v in r["wall_ms"].items():
            out.append("| %s | %.3f | %.3f |" % (k, v["median"], v["min"]))
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    pkg = entry.load_package()
    results = []
    os.makedirs(args.out, exist_ok=True)
    for n in [int(x) for x in args.sizes.split(",")]:
        results.append(measure(pkg, n, n, args.reps))
        print("(%d, %d): %s" % (n, n, json.dumps(results[-1]["wall_ms"])), flush=True)
        with open(os.path.join(args.out, "r1cs_timing.json"), "w") as f:
            json.dump({"reps": args.reps, "copy_tb_s": COPY_TBS, "results": results}, f, indent=1)
        with open(os.path.join(args.out, "r1cs_summary.md"), "w") as f:
            f.write(summary(results, args.reps) + "\n")


if __name__ == "__main__":
    main()
