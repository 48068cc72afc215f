"""Wall time of sc_prove_batch (B independent product sumchecks of n variables, Goldilocks, one launch per pass for the whole
batch) against B sequential sc_prove calls on the same instances, for n = 12, 16, 20 and B = 1, 8, 64, 256.

Per (n, B): the instances pair tables from a pool of 8 per side (generated on the device); one warm-up call of each form,
then --reps calls of each timed on the host (both calls return with every result on the host; the ctypes arguments are built
once, outside the timed region).  The c_1 of every instance must agree between the two forms.  Then one batch under the
launch log (option time_kernels): each batched pass's device time and the bytes it must move (B x both tables in, B x both
folded tables out), as GB/s.

  python tools/batch_timing.py [--sizes 12 16 20] [--batches 1 8 64 256] [--reps 5] [--limit 600] [--out F]
        every size in a child process of its own, under its own time limit
  python tools/batch_timing.py --step 16 [--batches ...]          one size, one JSON line
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_R = 0xC7C7000000000003


def run_step(n, batches, reps):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lib = pkg.load()
    u64p = pkg._lib.u64p
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
    k = 8
    ta = [pkg.DenseMultilinearExtension.generate(ctx, 0xA5A5000000000001 + 97 * t + n, n) for t in range(k)]
    tb = [pkg.DenseMultilinearExtension.generate(ctx, 0xB6B6000000000002 + 89 * t + n, n) for t in range(k)]
    out = {"n": n, "batches": {}}
    for B in batches:
        pa = [ta[i % k] for i in range(B)]
        pb = [tb[(3 * i + i // k) % k] for i in range(B)]
        arr_a = (ctypes.c_void_p * B)(*[t.h for t in pa])
        arr_b = (ctypes.c_void_p * B)(*[t.h for t in pb])
        seeds = np.array([(SEED_R + i) % 2**64 for i in range(B)], dtype=np.uint64)
        c1 = np.zeros(B, dtype=np.uint64)
        ev = np.zeros(3 * n * B, dtype=np.uint64)
        ch = np.zeros(n * B, dtype=np.uint64)
        c1s = np.zeros(B, dtype=np.uint64)
        evs = np.zeros(3 * n * B, dtype=np.uint64)
        chs = np.zeros(n * B, dtype=np.uint64)
        no_draw = ctypes.cast(None, pkg._lib.DRAW_BATCH_FN)
        no_draw1 = ctypes.cast(None, pkg._lib.DRAW_FN)
        args = (ctx.h, B, arr_a, arr_b, no_draw, None, seeds.ctypes.data_as(u64p), c1.ctypes.data_as(u64p), ev.ctypes.data_as(u64p),
                ch.ctypes.data_as(u64p))
        one = [(ctx.h, pa[i].h, pb[i].h, no_draw1, None, int(seeds[i]),
                ctypes.cast(c1s.ctypes.data + 8 * i, u64p), ctypes.cast(evs.ctypes.data + 24 * n * i, u64p),
                ctypes.cast(chs.ctypes.data + 8 * n * i, u64p)) for i in range(B)]

        def batch():
            ctx.check(lib.sc_prove_batch(*args))

        def sequential():
            for a in one:
                ctx.check(lib.sc_prove(*a))

        batch()
        sequential()
        ctx.synchronize()
        assert np.array_equal(c1, c1s) and np.array_equal(ev, evs) and np.array_equal(ch, chs), (n, B)
        tb_, ts_ = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            batch()
            ctx.synchronize()
            tb_.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            sequential()
            ctx.synchronize()
            ts_.append(time.perf_counter() - t0)
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
        batch()
        ctx.synchronize()
        log = ctx.launch_log()
        ctx.set_option("time_kernels", 0)
        wb, ws = statistics.median(tb_), statistics.median(ts_)
        kernels = [{"kf": r["kf"], "ks": r["ks"], "log_in": r["log_in"], "ms": r["ms"], "bytes": r["bytes_read"] + r["bytes_written"],
                    "GBps": (r["bytes_read"] + r["bytes_written"]) / (r["ms"] * 1e-3) / 1e9} for r in log if r["kind"] == "batch_pass"]
        out["batches"][str(B)] = {"batch_ms": wb * 1e3, "sequential_ms": ws * 1e3, "speedup": ws / wb,
                                  "batch_us_per_proof": wb * 1e6 / B, "sequential_us_per_proof": ws * 1e6 / B,
                                  "batch_all_ms": [t * 1e3 for t in tb_], "sequential_all_ms": [t * 1e3 for t in ts_],
                                  "first_pass_stream_GBps": (2 * 8 * (1 << n) * B) / wb / 1e9, "kernels": kernels,
                                  "c1_head": [int(x) for x in c1[:2]]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int)
    ap.add_argument("--sizes", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds each child step may take")
    ap.add_argument("--out", help="also write the JSON line here")
    args = ap.parse_args()
    if args.step is not None:
        res = run_step(args.step, args.batches, args.reps)
    else:
        res = {"field": "goldilocks", "sizes": {}}
        for n in args.sizes:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", str(n), "--reps", str(args.reps), "--batches"] + [str(b) for b in args.batches]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                res["sizes"][str(n)] = {"error": "time limit (%d s)" % args.limit}
                break
            if p.returncode != 0:
                res["sizes"][str(n)] = {"error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}
                break                                  # nothing more on the GPU after a failed step
            res["sizes"][str(n)] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
