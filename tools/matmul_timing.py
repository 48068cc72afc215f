"""Wall time of sc_matmul (C = A * B of 2^n x 2^n field matrices, Goldilocks) on its two paths:

  mfma   option matmul_path = 1: the byte repack + matmul_mfma_kernel (v_mfma_i32_16x16x64_i8, 15 diagonal accumulators)
  valu   option matmul_path = 2: matmul_tiled_kernel (the field's lazy multiply-add, 64 x 64 tiles)

for n = 10, 12, 13.  Per size: one warm-up call, then --reps calls timed on the host around ctx.synchronize(), and the
launch log (option time_kernels) for each kernel's device time.  Rates: the matrix-core path does 2^(3n) * 64 byte
multiply-adds (8 x 8 byte pairs per word product); the VALU path 2^(3n) word multiply-adds, also quoted as the same
2^(3n) * 64 byte-MAC equivalents so that the two read against one figure, the int8 dense peak of MI355X_MICROARCH.md
section Matrix cores (2x the BF16 rate: ~5.0e15 int8 ops/s = 2.5e15 MAC/s).

  python tools/matmul_timing.py [--sizes 10 12 13] [--reps 3] [--limit 600] [--out F]    each path in a child process of its
                                                                                          own, under its own time limit
  python tools/matmul_timing.py --step mfma [--sizes ...]                                 one path, one JSON line
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("mfma", "valu")
I8_PEAK_MACS = 2.5e15


def run_step(step, sizes, reps):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    mm = pkg.matrix_multiplication
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
    ctx.set_option("matmul_path", {"mfma": 1, "valu": 2}[step])
    out = {"step": step, "sizes": {}}
    for n in sizes:
        A = pkg.DenseMultilinearExtension.generate(ctx, 0xA5A5000000000001 + n, 2 * n)
        B = pkg.DenseMultilinearExtension.generate(ctx, 0xB6B6000000000002 + n, 2 * n)
        C = mm.matmul(ctx, n, A, B)   # warm-up (code objects, pool)
        ctx.synchronize()
        head = [int(x) for x in C.to_evaluations()[:4]]
        del C
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            C = mm.matmul(ctx, n, A, B)
            ctx.synchronize()
            walls.append(time.perf_counter() - t0)
            del C
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
        kernels = {}
        for _ in range(reps):
            C = mm.matmul(ctx, n, A, B)
            ctx.synchronize()
            del C
            for r in ctx.launch_log():
                if r["kind"] == "matmul":
                    kernels.setdefault(pkg._lib.MATMUL_KERNELS[r["kf"]], []).append(r)
        ctx.set_option("time_kernels", 0)
        wall = statistics.median(walls)
        macs = float(1 << (3 * n)) * 64
        rec = {"wall_ms": wall * 1e3, "wall_all_ms": [w * 1e3 for w in walls], "outputs_head": head,
               "byte_macs": macs, "fraction_of_i8_peak": macs / wall / I8_PEAK_MACS, "kernels": {}}
        for name, rs in kernels.items():
            ms = statistics.median(r["ms"] for r in rs)
            k = {"ms": ms, "bytes_read": rs[0]["bytes_read"], "bytes_written": rs[0]["bytes_written"],
                 "model_GBps": (rs[0]["bytes_read"] + rs[0]["bytes_written"]) / (ms * 1e-3) / 1e9}
            if name != "matmul_bytes_kernel":
                k["fraction_of_i8_peak"] = macs / (ms * 1e-3) / I8_PEAK_MACS
            rec["kernels"][name] = k
        out["sizes"][str(n)] = rec
        del A, B
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10, 12, 13])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds each child step may take")
    ap.add_argument("--out", help="also write the JSON line here")
    args = ap.parse_args()
    if args.step:
        res = run_step(args.step, args.sizes, args.reps)
    else:
        res = {"field": "goldilocks", "sizes": args.sizes, "steps": {}}
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--sizes"] + [str(n) for n in args.sizes]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                res["steps"][step] = {"error": "time limit (%d s)" % args.limit}
                break
            if p.returncode != 0:
                res["steps"][step] = {"error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}
                break                                  # nothing more on the GPU after a failed step
            res["steps"][step] = json.loads(p.stdout.strip().splitlines()[-1])
        s = res["steps"]
        if all(x in s and "sizes" in s[x] for x in STEPS):
            for n in map(str, args.sizes):
                assert s["mfma"]["sizes"][n]["outputs_head"] == s["valu"]["sizes"][n]["outputs_head"], n
            res["speedup_mfma_vs_valu"] = {n: s["valu"]["sizes"][n]["wall_ms"] / s["mfma"]["sizes"][n]["wall_ms"] for n in map(str, args.sizes)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
