"""Wall and device time of the Ligero-style commitment on one MI355X, Goldilocks tables (sc_table_generate):

  encode   sc_rs_encode_rows alone at (n, c, rho) = (20, 10, 1), (24, 12, 1), (26, 13, 1), (26, 12, 2)
  commit   sc_ligero_commit (encode + column hash + tree), sc_ligero_combine_rows with two weight vectors, 64 openings

Per shape: two warm-up calls, then --reps calls timed on the host around a device synchronise (each call ends in one), and the
launch log (option time_kernels) for every kernel's device time and bytes.  The encoder has to read the table once and write
the codewords once, 8 * 2^n + 8 * 2^(n + rho) bytes: that over the time is the rate, reported against the 8 TB/s peak and the
6.29 TB/s a plain copy reaches on this chip (the yardstick: a copy also reads and writes every word once).  The column hash
costs ceil((8 R + 9) / 64) SHA-256 compressions per column (the data blocks and the padding), the levels above 2 per node.

CPU row: the same sc_rs_encode_rows shape through tests/ligero_ref.py's numpy transform on one core (arrays of Python
integers: Goldilocks products do not fit int64), at (20, 10, 1) only.

  python tools/ligero_timing.py [--reps 10] [--limit 600] [--out profiles] [--trace]
        every step in a child process under its own time limit; writes <out>/ligero_timing.json and <out>/ligero_summary.md;
        --trace adds a rocprofv3 --kernel-trace --stats run of the encode step, stats to <out>/ligero_kernel_stats.csv
  python tools/ligero_timing.py --step encode|commit [--reps 10]      one step, one JSON line
  python tools/ligero_timing.py --skip-cpu ... ; python tools/ligero_timing.py --cpu-only    the GPU part and the CPU row apart
  python tools/ligero_timing.py --code expander [--reps 10]
        the linear-time expander code (sc_xc_encode_rows) at (n, c) = (20, 10), (24, 12), (26, 13):
        in ONE child process per shape list, sc_rs_encode_rows (rho = 1) and sc_xc_encode_rows on Goldilocks, sc_xc_encode_rows on
        2^64 - 59 (which Reed-Solomon cannot serve), and the expander commit on both fields; writes <out>/expander_timing.json and
        <out>/expander_summary.md: the encode time, its ratio to rs_encode_rows_kernel at the same shape in the same run, and its
        rate on 24 * 2^n bytes against the 6.29 TB/s copy rate.  The default --code rs is everything above, unchanged.
  python tools/ligero_timing.py --long [--reps 7]
        rows longer than the LDS (sc_rs_encode_rows_long) at (n, c, rho) = (24, 16, 1), (26, 17, 1),
        (26, 16, 2), (28, 17, 1), each beside the in-LDS shape of the same n and rho (c = 14 - rho), in ONE child process: the
        device time of the two launches and their rate on the modelled bytes, their sum against rs_encode_rows_kernel,
        column_leaf_kernel at both widths, the commit's wall time, and the wall time and size of a 64-column opening at both
        widths; writes <out>/ligero_long_timing.json and <out>/ligero_long_summary.md.
  python tools/ligero_timing.py --long --code expander [--reps 7]
        expander-code rows longer than the LDS (sc_xc_encode_rows_long) at (n, c) = (24, 16), (26, 17),
        (28, 17) over Goldilocks and 2^64 - 59, each beside the in-LDS expander shape (c = 13) of the same n, in ONE child process:
        the device time of every launch, the gathers per second of the level launches, their sum against xc_encode_rows_kernel,
        column_leaf_kernel at both widths, the commit's wall time, and the wall time and size of a 64-column opening at both
        widths; writes <out>/expander_long_timing.json and <out>/expander_long_summary.md.
  python tools/ligero_timing.py --fold [--reps 5]
        folded openings (sc_ligero_fold_*) at (n, rho) = (24, 1), (26, 1), (28, 1) with the shape
        fold_log_cols picks for 128 queries, Goldilocks, in ONE child process: the device time of every fold launch
        and its rate on the record's bytes against the 6.29 TB/s copy rate, the wall time of begin, prove and query against the
        wall time of the plain opening (sc_ligero_combine_rows + sc_ligero_open_columns) of the same commitment, the wall
        time of FoldVerifier.verify, and one sc_rs_fold alone (no tree) at M = 2^16, 2^20, 2^24; writes
        <out>/ligero_fold_timing.json and <out>/ligero_fold_summary.md.
  python tools/ligero_timing.py --fold --summary-only --parent A.json B.json
        adds two --fold runs of the parent commit to ligero_fold_timing.json and their launch-by-launch table to the summary.
  python tools/ligero_timing.py --fold-staged [--reps 5]
        staged folded openings (sc_ligero_fold_begin_staged) at the shapes of --fold: the (log_cols,
        schedule) fold_shape picks beside the binary folded opening at fold_log_cols' shape, in ONE child process: every fold
        launch, the wall time of begin, prove and query, the merkle device time, the wall time of FoldVerifier.verify and the
        bytes; writes <out>/ligero_fold_staged_timing.json and <out>/ligero_fold_staged_summary.md.
"""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((20, 10, 1), (24, 12, 1), (26, 13, 1), (26, 12, 2))
PEAK_BPS = 8.0e12
COPY_BPS = 6.29e12          # the measured copy rate of the chip (read + write bytes per second)
MERKLE_LEAF_CPS = 2.7e10    # merkle_leaf_kernel at n = 28, profiles/pcs_summary.md
OPENINGS = 64
XC_SHAPES = ((20, 10), (24, 12), (26, 13))
LONG_SHAPES = ((24, 16, 1), (26, 17, 1), (26, 16, 2), (28, 17, 1))
XC_LONG_SHAPES = ((24, 16), (26, 17), (28, 17))
XC_LONG_KERNELS = {0: "copy", 1: "down", 2: "inner", 3: "up"}
P59 = 2**64 - 59
FOLD_SHAPES = ((24, 1), (26, 1), (28, 1))
FOLD_QUERIES = 128
FOLD_ALONE_LOGS = (16, 20, 24)


def _timed(ctx, fn, reps):
    for _ in range(2):   # warm-up (code objects, pool, the twiddle table)
        fn()
    ctx.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        walls.append(time.perf_counter() - t0)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    fn()
    ctx.synchronize()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    return walls, log


def leaf_compressions(r, log_len):
    return ((8 * (1 << r) + 9 + 63) // 64) << log_len


def run_step(step, reps):
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lp = pkg.ligero_pcs
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
    F = ctx.field
    out = {"step": step, "shapes": {}}
    for n, c, rho in SHAPES:
        key = "%d,%d,%d" % (n, c, rho)
        t = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + n, n)
        if step == "encode":
            walls, log = _timed(ctx, lambda: lp.rs_encode_rows(ctx, t, c, rho), reps)
            [rec] = [r for r in log if r["kind"] == "rs_encode"]
            wall = statistics.median(walls)
            moved = rec["bytes_read"] + rec["bytes_written"]
            out["shapes"][key] = {"wall_ms": wall * 1e3, "wall_all_ms": [w * 1e3 for w in walls], "device_ms": rec["ms"], "bytes": moved,
                                  "wall_Bps": moved / wall, "device_Bps": moved / (rec["ms"] * 1e-3)}
        else:
            r = n - c
            walls, log = _timed(ctx, lambda: lp.Prover.commit(ctx, t, c, rho).close(), reps)
            kernels = {}
            for rec in log:
                name = {"rs_encode": "rs_encode_rows_kernel", "ligero": "column_leaf_kernel"}.get(rec["kind"]) or pkg._lib.MERKLE_KERNELS[rec["kf"]]
                k = kernels.setdefault(name, {"launches": 0, "ms": 0.0})
                k["launches"] += 1
                k["ms"] += rec["ms"]
            prover = lp.Prover.commit(ctx, t, c, rho)
            import random
            rng = random.Random(n)
            weights = [[F.rand(rng) for _ in range(1 << r)] for _ in range(2)]
            cw, clog = _timed(ctx, lambda: prover.combine_rows(weights), max(2, reps // 3))
            cols = [rng.randrange(1 << (c + rho)) for _ in range(OPENINGS)]
            ow, olog = _timed(ctx, lambda: prover.open_columns(cols), max(2, reps // 3))
            comp = leaf_compressions(r, c + rho)
            leaf_ms = kernels["column_leaf_kernel"]["ms"]
            out["shapes"][key] = {"commit_wall_ms": statistics.median(walls) * 1e3, "commit_wall_all_ms": [w * 1e3 for w in walls], "kernels": kernels,
                                  "leaf_compressions": comp, "leaf_compressions_per_s": comp / (leaf_ms * 1e-3), "root": prover.root().hex(),
                                  "combine_wall_ms": statistics.median(cw) * 1e3,
                                  "combine_device_ms": sum(x["ms"] for x in clog), "combine_bytes_read": clog[0]["bytes_read"],
                                  "open_wall_ms": statistics.median(ow) * 1e3, "open_device_ms": sum(x["ms"] for x in olog)}
            prover.close()
        del t
    return out


def run_expander(reps):
    """--code expander: per shape the two encoders on Goldilocks, the expander encoder on 2^64 - 59, and the expander commit"""
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lp = pkg.ligero_pcs
    out = {"step": "expander", "shapes": {}}
    ctxs = {"gold": pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0), "p59": pkg.Context(pkg.Field(P59), device=0)}
    for n, c in XC_SHAPES:
        row = {}
        for name, ctx in ctxs.items():
            t = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + n, n)
            runs = [("xc", "xc_encode", lambda: lp.xc_encode_rows(ctx, t, c))]
            if name == "gold":
                runs.insert(0, ("rs", "rs_encode", lambda: lp.rs_encode_rows(ctx, t, c, 1)))
            for tag, kind, fn in runs:
                walls, log = _timed(ctx, fn, reps)
                [rec] = [r for r in log if r["kind"] == kind]
                row["%s_%s" % (tag, name)] = {"wall_ms": statistics.median(walls) * 1e3, "device_ms": rec["ms"],
                                              "bytes": rec["bytes_read"] + rec["bytes_written"]}
            walls, log = _timed(ctx, lambda: lp.Prover.commit(ctx, t, c, 1, code="expander").close(), max(2, reps // 3))
            row["commit_%s" % name] = {"wall_ms": statistics.median(walls) * 1e3,
                                       "encode_ms": sum(r["ms"] for r in log if r["kind"] == "xc_encode"),
                                       "leaf_ms": sum(r["ms"] for r in log if r["kind"] == "ligero"),
                                       "tree_ms": sum(r["ms"] for r in log if r["kind"] == "merkle")}
            del t
        out["shapes"]["%d,%d" % (n, c)] = row
    return out


def run_long(reps):
    """--long: per shape the long encoder and commitment beside the in-LDS ones of the same n and rho"""
    import random
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lp = pkg.ligero_pcs
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
    out = {"step": "long", "shapes": {}}
    for n, c, rho in LONG_SHAPES:
        t = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + n, n)
        row = {}
        for tag, cc, encode, commit in (("long", c, lp.rs_encode_rows_long, lp.Prover.commit_long), ("short", 14 - rho, lp.rs_encode_rows, lp.Prover.commit)):
            walls, log = _timed(ctx, lambda: encode(ctx, t, cc, rho), reps)
            enc = [r for r in log if r["kind"] in ("rs_long", "rs_encode")]
            cw, clog = _timed(ctx, lambda: commit(ctx, t, cc, rho).close(), max(2, reps // 3))
            prover = commit(ctx, t, cc, rho)
            rng = random.Random(n)
            cols = [rng.randrange(1 << (cc + rho)) for _ in range(OPENINGS)]
            ow, olog = _timed(ctx, lambda: prover.open_columns(cols), max(2, reps // 3))
            prover.close()
            row[tag] = {"log_cols": cc, "encode_wall_ms": statistics.median(walls) * 1e3,
                        "launches": [{"kf": r["kf"], "ks": r["ks"], "ms": r["ms"], "bytes": r["bytes_read"] + r["bytes_written"]} for r in enc],
                        "encode_device_ms": sum(r["ms"] for r in enc),
                        "commit_wall_ms": statistics.median(cw) * 1e3,
                        "commit_encode_ms": sum(r["ms"] for r in clog if r["kind"] in ("rs_long", "rs_encode")),
                        "leaf_ms": sum(r["ms"] for r in clog if r["kind"] == "ligero"),
                        "tree_ms": sum(r["ms"] for r in clog if r["kind"] == "merkle"),
                        "open_wall_ms": statistics.median(ow) * 1e3, "open_device_ms": sum(r["ms"] for r in olog),
                        "open_bytes": lp.opening_bytes(n, cc, rho, OPENINGS)}
        out["shapes"]["%d,%d,%d" % (n, c, rho)] = row
        del t
    return out


def run_xc_long(reps):
    """--long --code expander: per shape and field the long expander encoder and commitment beside the in-LDS ones (c = 13)"""
    import random
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lp = pkg.ligero_pcs
    out = {"step": "xc_long", "shapes": {}}
    ctxs = {"gold": pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0), "p59": pkg.Context(pkg.Field(P59), device=0)}
    short_c = pkg.expander_code.MAX_LOG_COLS
    for n, c in XC_LONG_SHAPES:
        row = {}
        for name, ctx in ctxs.items():
            t = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + n, n)
            for tag, cc, encode, commit in (("long", c, lp.xc_encode_rows_long, lp.Prover.commit_long), ("short", short_c, lp.xc_encode_rows, lp.Prover.commit)):
                walls, log = _timed(ctx, lambda: encode(ctx, t, cc), reps)
                enc = [r for r in log if r["kind"] in ("xc_long", "xc_encode")]
                cw, clog = _timed(ctx, lambda: commit(ctx, t, cc, 1, code="expander").close(), max(2, reps // 3))
                prover = commit(ctx, t, cc, 1, code="expander")
                rng = random.Random(n)
                cols = [rng.randrange(2 << cc) for _ in range(OPENINGS)]
                ow, olog = _timed(ctx, lambda: prover.open_columns(cols), max(2, reps // 3))
                prover.close()
                row["%s_%s" % (tag, name)] = {
                    "log_cols": cc, "encode_wall_ms": statistics.median(walls) * 1e3,
                    "launches": [{"kind": r["kind"], "kf": r["kf"], "ks": r["ks"], "ms": r["ms"], "bytes_read": r["bytes_read"],
                                  "bytes_written": r["bytes_written"]} for r in enc],
                    "encode_device_ms": sum(r["ms"] for r in enc),
                    "commit_wall_ms": statistics.median(cw) * 1e3,
                    "commit_encode_ms": sum(r["ms"] for r in clog if r["kind"] in ("xc_long", "xc_encode")),
                    "leaf_ms": sum(r["ms"] for r in clog if r["kind"] == "ligero"),
                    "tree_ms": sum(r["ms"] for r in clog if r["kind"] == "merkle"),
                    "open_wall_ms": statistics.median(ow) * 1e3, "open_device_ms": sum(r["ms"] for r in olog),
                    "open_bytes": lp.opening_bytes(n, cc, 1, OPENINGS)}
            del t
        out["shapes"]["%d,%d" % (n, c)] = row
    return out


def run_fold(reps):
    """--fold: per shape the folded opening beside the plain opening of the same commitment"""
    import ctypes
    import random
    import numpy as np
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lp = pkg.ligero_pcs
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
    F = ctx.field
    out = {"step": "fold", "queries": FOLD_QUERIES, "shapes": {}}
    for n, rho in FOLD_SHAPES:
        c = lp.fold_log_cols(n, rho, FOLD_QUERIES)
        t = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + n, n)
        prover = lp.Prover.commit_long(ctx, t, c, rho)
        rng = random.Random(n)
        point = [F.rand(rng) for _ in range(n)]
        gamma = [F.rand(rng) for _ in range(1 << (n - c))]
        alphas = [F.rand(rng) for _ in range(c)]
        beta = F.rand(rng)
        indices = [rng.randrange(1 << (c + rho - 1)) for _ in range(FOLD_QUERIES)]
        # the plain opening: the two combined rows to the host (the C call: no Python lists of 2^c words), 128 columns
        weights = np.ascontiguousarray(np.array([gamma, lp.eq_weights(F, point[c:])], dtype=np.uint64).reshape(-1))
        rows = np.zeros(2 << c, dtype=np.uint64)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        cols = [rng.randrange(1 << (c + rho)) for _ in range(FOLD_QUERIES)]

        def plain():
            ctx.check(ctx.lib.sc_ligero_combine_rows(ctx.h, prover.h, weights.ctypes.data_as(u64p), 2, rows.ctypes.data_as(u64p)))
            prover.open_columns(cols)
        walls = {"begin": [], "prove": [], "query": [], "plain": []}
        logs = []
        for rep in range(2 * reps + 2):         # two warm-up runs, `reps` timed ones, `reps` with the launch log on
            timed, logged = 2 <= rep < reps + 2, rep >= reps + 2
            t0 = time.perf_counter()
            opening = prover.fold_begin(point, gamma)
            t1 = time.perf_counter()
            if logged:
                ctx.set_option("time_kernels", 1)
                ctx.launch_log()
            opening.prove(beta, lambda i, e, root: alphas[i])
            t2 = time.perf_counter()
            if logged:
                logs.append(ctx.launch_log())
                ctx.set_option("time_kernels", 0)
            opened = opening.query(indices)
            t3 = time.perf_counter()
            opening.close()
            plain()
            t4 = time.perf_counter()
            if timed:
                for key, a, b in (("begin", t0, t1), ("prove", t1, t2), ("query", t2, t3), ("plain", t3, t4)):
                    walls[key].append(b - a)
        # the verifier, on the device prover's messages
        v = lp.FoldVerifier(F, n, c, rho, prover.root(), FOLD_QUERIES)
        opening = prover.fold_begin(point, v.draw_gamma(rng))
        v.receive_claims(*opening.claims)
        final = opening.prove(v.draw_beta(rng), lambda i, e, root: v.round(i, e, root, rng))[3]
        v.receive_final(final)
        opened = opening.query(v.draw_queries(rng))
        t0 = time.perf_counter()
        value = v.verify(point, opened)
        verify_s = time.perf_counter() - t0
        opening.close()
        assert value == t.evaluate(point), "the folded opening was accepted with a wrong value"
        prover.close()
        # a launch's device time: the median over the logged runs, which all queue the same launches in the same order
        log = [dict(r, ms=statistics.median(x[k]["ms"] for x in logs), ms_all=[x[k]["ms"] for x in logs]) for k, r in enumerate(logs[0])]
        folds = [r for r in log if r["kind"] == "rs_fold"]
        out["shapes"]["%d,%d,%d" % (n, c, rho)] = {
            "log_cols": c, "fold_opening_bytes": lp.fold_opening_bytes(n, c, rho, FOLD_QUERIES),
            "plain_opening_bytes_same_shape": lp.opening_bytes(n, c, rho, FOLD_QUERIES),
            "plain_opening_bytes_best_shape": lp.opening_bytes(n, lp.long_log_cols(n, rho, FOLD_QUERIES), rho, FOLD_QUERIES),
            "launches": [{"kf": r["kf"], "ks": r["ks"], "ms": r["ms"], "ms_all": r["ms_all"], "bytes": r["bytes_read"] + r["bytes_written"]} for r in folds],
            "fold_device_ms": sum(r["ms"] for r in folds),
            "prove_device_ms": {k: sum(r["ms"] for r in log if r["kind"] == k) for k in sorted({r["kind"] for r in log})},
            "wall_ms": {k: statistics.median(w) * 1e3 for k, w in walls.items()}, "verify_wall_ms": verify_s * 1e3}
        del t
    # one stand-alone sc_rs_fold per length: the fold without a tree, which no launch of an opening above M = 4 is
    out["standalone"] = []
    for log_m in FOLD_ALONE_LOGS:
        u = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + log_m, log_m)
        alpha = F.rand(random.Random(log_m))
        for _ in range(2):
            lp.rs_fold(ctx, u, alpha)
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
        for _ in range(reps):
            lp.rs_fold(ctx, u, alpha)
        ctx.synchronize()
        recs = [r for r in ctx.launch_log() if r["kind"] == "rs_fold"]
        ctx.set_option("time_kernels", 0)
        out["standalone"].append({"kf": recs[0]["kf"], "ks": log_m, "ms": statistics.median(r["ms"] for r in recs), "ms_all": [r["ms"] for r in recs],
                                  "bytes": recs[0]["bytes_read"] + recs[0]["bytes_written"]})
        del u
    return out


def run_fold_staged(reps):
    """--fold-staged: per (n, rho) the staged opening at fold_shape's shape beside the binary folded opening at fold_log_cols' shape"""
    import random
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    lp = pkg.ligero_pcs
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS), device=0)
    F = ctx.field
    out = {"step": "fold_staged", "queries": FOLD_QUERIES, "shapes": {}}
    for n, rho in FOLD_SHAPES:
        t = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE0000 + n, n)
        c_staged, schedule = lp.fold_shape(n, rho, FOLD_QUERIES)
        row = {}
        for name, c, arities in (("binary", lp.fold_log_cols(n, rho, FOLD_QUERIES), None), ("staged", c_staged, schedule)):
            prover = lp.Prover.commit_long(ctx, t, c, rho)
            rng = random.Random(n)
            point = [F.rand(rng) for _ in range(n)]
            gamma = [F.rand(rng) for _ in range(1 << (n - c))]
            alphas = [F.rand(rng) for _ in range(c)]
            beta = F.rand(rng)
            indices = [rng.randrange(1 << (c + rho - (arities[0] if arities else 1))) for _ in range(FOLD_QUERIES)]
            walls = {"begin": [], "prove": [], "query": []}
            log, qlog = [], []
            for rep in range(reps + 3):             # two warm-up runs, `reps` timed ones, one with the launch log on
                timed, logged = 2 <= rep < reps + 2, rep == reps + 2
                t0 = time.perf_counter()
                opening = prover.fold_begin(point, gamma, arities)
                t1 = time.perf_counter()
                if logged:
                    ctx.set_option("time_kernels", 1)
                    ctx.launch_log()
                opening.prove(beta, lambda i, e, root: alphas[i])
                t2 = time.perf_counter()
                if logged:
                    log = ctx.launch_log()
                opening.query(indices)
                t3 = time.perf_counter()
                if logged:
                    qlog = ctx.launch_log()
                    ctx.set_option("time_kernels", 0)
                opening.close()
                if timed:
                    for key, a, b in (("begin", t0, t1), ("prove", t1, t2), ("query", t2, t3)):
                        walls[key].append(b - a)
            # the verifier, on the device prover's messages
            v = lp.FoldVerifier(F, n, c, rho, prover.root(), FOLD_QUERIES, arities=arities)
            opening = prover.fold_begin(point, v.draw_gamma(rng), arities)
            v.receive_claims(*opening.claims)
            final = opening.prove(v.draw_beta(rng), lambda i, e, root: v.round(i, e, root, rng))[3]
            v.receive_final(final)
            opened = opening.query(v.draw_queries(rng))
            t0 = time.perf_counter()
            value = v.verify(point, opened)
            verify_s = time.perf_counter() - t0
            opening.close()
            assert value == t.evaluate(point), "the folded opening was accepted with a wrong value"
            prover.close()
            folds = [r for r in log if r["kind"] in ("rs_fold", "rs_fold_many")]
            row[name] = {
                "log_cols": c, "arities": list(arities) if arities else [1] * c, "trees": (len(arities) if arities else c) - 1,
                "opening_bytes": lp.fold_opening_bytes(n, c, rho, FOLD_QUERIES, arities=arities),
                "launches": [{"kind": r["kind"], "kf": r["kf"], "ks": r["ks"], "ms": r["ms"], "bytes": r["bytes_read"] + r["bytes_written"]} for r in folds],
                "fold_device_ms": sum(r["ms"] for r in folds), "merkle_device_ms": sum(r["ms"] for r in log if r["kind"] == "merkle"),
                "query_gather_launches": len([r for r in qlog if r["kind"] == "ligero" and r["kf"] == 2]),
                "prove_device_ms": {k: sum(r["ms"] for r in log if r["kind"] == k) for k in sorted({r["kind"] for r in log})},
                "wall_ms": {k: statistics.median(w) * 1e3 for k, w in walls.items()}, "verify_wall_ms": verify_s * 1e3}
        row["plain_opening_bytes_best_shape"] = lp.opening_bytes(n, lp.long_log_cols(n, rho, FOLD_QUERIES), rho, FOLD_QUERIES)
        out["shapes"]["%d,%d" % (n, rho)] = row
        del t
    return out


def fold_staged_summary(res):
    step = res["steps"]["fold_staged"]
    lines = ["# Staged folded Ligero openings on one MI355X: up to three variables per committed layer beside the binary fold", "",
             "Measured by `python tools/ligero_timing.py --fold-staged --reps %d`: every figure comes from ONE process.  Goldilocks, tables "
             "from `sc_table_generate`, %d queries; `staged` is the (log_cols, schedule) `fold_shape` picks, `binary` the folded opening of "
             "DESIGN.md section 9 item 13 at the shape `fold_log_cols` picks - two commitments of the same table.  Device times: HIP "
             "events of the launch log, option `time_kernels`, one instrumented run; wall times: medians after two warm-up runs, Python "
             "wrappers included.  There is no threshold on speed here: the deliverable is the smaller opening and the fewer trees." %
             (res["reps"], step["queries"]), "",
             "## The opening", "",
             "| (n, rho) | opening | log_cols | schedule | trees | opening bytes | begin wall ms | prove wall ms | query wall ms | total ms | "
             "fold launches device ms | merkle device ms | gather launches per query batch | FoldVerifier.verify wall ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, row in step["shapes"].items():
        for name in ("binary", "staged"):
            r, w = row[name], row[name]["wall_ms"]
            sched = "all ones" if name == "binary" else "(%s)" % ", ".join(str(a) for a in r["arities"])
            lines.append("| (%s) | %s | %d | %s | %d | %d | %.2f | %.2f | %.2f | %.2f | %.3f | %.3f | %d | %.1f |" % (
                key.replace(",", ", "), name, r["log_cols"], sched, r["trees"], r["opening_bytes"], w["begin"], w["prove"], w["query"],
                w["begin"] + w["prove"] + w["query"], r["fold_device_ms"], r["merkle_device_ms"], r["query_gather_launches"], r["verify_wall_ms"]))
    lines += ["", "The plain opening at its best shape, for scale: " +
              ", ".join("(%s) %d bytes" % (k.replace(",", ", "), row["plain_opening_bytes_best_shape"]) for k, row in step["shapes"].items()) + ".",
              "", "## Every fold launch of one staged opening", "",
              "| (n, rho) | log2 M | variables folded | device ms | bytes read + written | TB/s | of the 6.29 TB/s copy rate |", "|---|---|---|---|---|---|---|"]
    for key, row in step["shapes"].items():
        for r in row["staged"]["launches"]:
            bps = r["bytes"] / (r["ms"] * 1e-3) if r["ms"] > 0 else float("nan")
            lines.append("| (%s) | %d | %d | %.4f | %d | %.3f | %.1f %% |" % (key.replace(",", ", "), r["ks"], r["kf"], r["ms"], r["bytes"], bps / 1e12,
                                                                       100 * bps / COPY_BPS))
    lines += ["", "## Device time of one prove call, by launch kind (ms)", ""]
    for key, row in step["shapes"].items():
        for name in ("binary", "staged"):
            lines.append("- (%s) %s: " % (key.replace(",", ", "), name) + ", ".join("%s %.3f" % (k, v) for k, v in row[name]["prove_device_ms"].items()))
    if res.get("notes"):
        lines += ["", "## What the figures say", ""] + res["notes"]
    return "\n".join(lines) + "\n"


def fold_against_parents(step, parents):
    """the fold launches of this run beside the same launches of two runs of the parent commit (--parent): the margin of a
    launch is the difference between the two parent runs, and `over` is what this run exceeds the slower parent run plus it by"""
    lines = ["", "## Against the parent commit: device ms of every fold launch", "",
             "Two runs of the same command on the parent commit, same machine, same session.  margin = |parent run 1 - parent run 2|; "
             "over = this run - (max of the parent runs + margin), shown where positive.", "",
             "| launch | log2 M | hashed | parent run 1 | parent run 2 | margin | this run | over |", "|---|---|---|---|---|---|---|---|"]

    def row(label, ks, hashed, a, b, x):
        over = x - (max(a, b) + abs(a - b))
        return "| %s | %s | %s | %.4f | %.4f | %.4f | %.4f | %s |" % (label, ks, hashed, a, b, abs(a - b), x, "%.4f" % over if over > 0 else "-")
    for key, cur in step["shapes"].items():
        label = "(%s)" % key.replace(",", ", ")
        pa, pb = (p["shapes"][key] for p in parents)
        for r, a, b in zip(cur["launches"], pa["launches"], pb["launches"]):
            lines.append(row(label, r["ks"], "yes" if r["kf"] else "no", a["ms"], b["ms"], r["ms"]))
        lines.append(row(label, "sum", "", pa["fold_device_ms"], pb["fold_device_ms"], cur["fold_device_ms"]))
    for r, a, b in zip(step.get("standalone", []), *(p.get("standalone", []) for p in parents)):
        lines.append(row("sc_rs_fold alone", r["ks"], "yes" if r["kf"] else "no", a["ms"], b["ms"], r["ms"]))
    return lines


def fold_summary(res):
    step = res["steps"]["fold"]
    lines = ["# Folded Ligero openings on one MI355X: the fold launches, the prover's three calls, the host verifier", "",
             "Measured by `python tools/ligero_timing.py --fold --reps %d`: every figure comes from ONE process.  Goldilocks, tables from "
             "`sc_table_generate`, %d queries, the shape `fold_log_cols` picks.  Device times: HIP events of the launch log, option "
             "`time_kernels`, each launch's median over as many instrumented runs as timed ones; wall times: medians after two warm-up "
             "runs, Python wrappers included.  A fold of "
             "M words reads 8 M bytes and writes 4 M, plus 8 M of digests where it hashes (every launch but the last of an opening); "
             "the yardstick is the chip's measured copy rate, 6.29 TB/s." % (res["reps"], step["queries"]), "",
             "## Every fold launch of one opening", "",
             "| (n, c, rho) | log2 M | hashed | device ms | bytes read + written | TB/s | of the 6.29 TB/s copy rate |", "|---|---|---|---|---|---|---|"]
    for key, row in step["shapes"].items():
        for r in row["launches"]:
            bps = r["bytes"] / (r["ms"] * 1e-3) if r["ms"] > 0 else float("nan")
            lines.append("| (%s) | %d | %s | %.4f | %d | %.3f | %.1f %% |" % (key.replace(",", ", "), r["ks"], "yes" if r["kf"] else "no", r["ms"],
                                                                         r["bytes"], bps / 1e12, 100 * bps / COPY_BPS))
    if step.get("standalone"):
        lines += ["", "## One sc_rs_fold alone: the fold without a tree", "",
                  "Median device time of %d launches after two warm-up calls." % res["reps"], "",
                  "| log2 M | hashed | device ms | bytes read + written | TB/s | of the 6.29 TB/s copy rate |", "|---|---|---|---|---|---|"]
        for r in step["standalone"]:
            bps = r["bytes"] / (r["ms"] * 1e-3)
            lines.append("| %d | %s | %.4f | %d | %.3f | %.1f %% |" % (r["ks"], "yes" if r["kf"] else "no", r["ms"], r["bytes"], bps / 1e12,
                                                                  100 * bps / COPY_BPS))
    if res.get("parents"):
        lines += fold_against_parents(step, [p["steps"]["fold"] for p in res["parents"]])
    lines += ["", "## The opening: folded against plain, same commitment", "",
              "| (n, c, rho) | begin wall ms | prove wall ms | query wall ms | folded total ms | plain (combine + open_columns) wall ms | "
              "all rs_fold launches device ms | FoldVerifier.verify wall ms | folded opening bytes | plain bytes at this shape | plain bytes at its best shape |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, row in step["shapes"].items():
        w = row["wall_ms"]
        lines.append("| (%s) | %.2f | %.2f | %.2f | %.2f | %.2f | %.3f | %.1f | %d | %d | %d |" % (
            key.replace(",", ", "), w["begin"], w["prove"], w["query"], w["begin"] + w["prove"] + w["query"], w["plain"], row["fold_device_ms"],
            row["verify_wall_ms"], row["fold_opening_bytes"], row["plain_opening_bytes_same_shape"], row["plain_opening_bytes_best_shape"]))
    lines += ["", "## Device time of one prove call, by launch kind (ms)", ""]
    for key, row in step["shapes"].items():
        lines.append("- (%s): " % key.replace(",", ", ") + ", ".join("%s %.3f" % (k, v) for k, v in row["prove_device_ms"].items()))
    if res.get("notes"):
        lines += ["", "## What binds", ""] + res["notes"]
    return "\n".join(lines) + "\n"


def xc_long_summary(res):
    fields = (("gold", "Goldilocks"), ("p59", "2^64 - 59"))
    lines = ["# Expander-code rows longer than the LDS on one MI355X: levels through global memory beside the in-LDS encoder", "",
             "Measured by `python tools/ligero_timing.py --long --code expander --reps %d`: every figure, the in-LDS (c = 13) columns "
             "included, comes from ONE process.  Tables from `sc_table_generate`.  Device times: HIP events of the launch log, option "
             "`time_kernels`; wall times: medians after two warm-up calls.  A level launch gathers 8·R·2^lm words of 8 bytes (down: 32 per "
             "output, R·2^(lm-2) outputs; up: 16 per output, R·2^(lm-1) outputs); the gather rates below are those counts over the "
             "launch's device time and are measurements of this run, not figures from a data sheet." % res["reps"], "",
             "## The launches", "",
             "| (n, c) | field | launch | lm | device ms | bytes read + written | G gathers/s |", "|---|---|---|---|---|---|---|"]
    shapes = res["steps"]["xc_long"]["shapes"]
    for key, row in shapes.items():
        n = int(key.split(",")[0])
        for name, label in fields:
            lo = row["long_" + name]
            for r in lo["launches"]:
                gathers = (8 << (n - lo["log_cols"] + r["ks"])) if r["kf"] in (1, 3) else 0
                lines.append("| (%s) | %s | %s | %d | %.3f | %d | %s |" % (
                    key.replace(",", ", "), label, XC_LONG_KERNELS[r["kf"]], r["ks"], r["ms"], r["bytes_read"] + r["bytes_written"],
                    "%.1f" % (gathers / (r["ms"] * 1e-3) / 1e9) if gathers else "-"))
    lines += ["", "## The encoder: all launches against xc_encode_rows_kernel at c = 13", "",
              "| (n, c) | field | long: launches | long: device ms | wall ms | in-LDS (c = 13) device ms | wall ms | long / in-LDS |", "|---|---|---|---|---|---|---|---|"]
    for key, row in shapes.items():
        for name, label in fields:
            lo, sh = row["long_" + name], row["short_" + name]
            lines.append("| (%s) | %s | %d | %.3f | %.3f | %.3f | %.3f | %.2f |" % (
                key.replace(",", ", "), label, len(lo["launches"]), lo["encode_device_ms"], lo["encode_wall_ms"], sh["encode_device_ms"],
                sh["encode_wall_ms"], lo["encode_device_ms"] / sh["encode_device_ms"]))
    lines += ["", "## The commitment and a %d-column opening, at both widths" % OPENINGS, "",
              "| (n, c) | field | width | commit wall ms | encode ms | column_leaf_kernel ms | tree ms | open wall ms | open device ms | opening bytes |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for key, row in shapes.items():
        for name, label in fields:
            for tag in ("long", "short"):
                k = row["%s_%s" % (tag, name)]
                lines.append("| (%s) | %s | c = %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %d |" % (
                    key.replace(",", ", "), label, k["log_cols"], k["commit_wall_ms"], k["commit_encode_ms"], k["leaf_ms"], k["tree_ms"],
                    k["open_wall_ms"], k["open_device_ms"], k["open_bytes"]))
    if res.get("notes"):
        lines += ["", "## What binds", ""] + res["notes"]
    return "\n".join(lines) + "\n"


def long_summary(res):
    lines = ["# Ligero rows longer than the LDS on one MI355X: the four-step transform beside the in-LDS encoder", "",
             "Measured by `python tools/ligero_timing.py --long --reps %d`: every figure, the in-LDS columns included, comes from ONE "
             "process.  Goldilocks, tables from `sc_table_generate`.  Device times: HIP events of the launch log, option `time_kernels`; "
             "wall times: medians after two warm-up calls.  Modelled bytes: the column step reads 8·2^n and writes 8·2^(n+rho), the row "
             "step reads and writes 8·2^(n+rho); the in-LDS encoder reads 8·2^n and writes 8·2^(n+rho).  The yardstick is the chip's "
             "measured copy rate, 6.29 TB/s." % res["reps"], "",
             "## The encoder", "",
             "| (n, c, rho) | a + b | column step ms | TB/s | row step ms | TB/s | sum ms | in-LDS (c = 14 - rho) ms | long / in-LDS |", "|---|---|---|---|---|---|---|---|---|"]
    shapes = res["steps"]["long"]["shapes"]
    for key, row in shapes.items():
        lo, sh = row["long"], row["short"]
        s0, s1 = lo["launches"]
        lines.append("| (%s) | %d + %d | %.3f | %.2f | %.3f | %.2f | %.3f | %.3f | %.2f |" % (
            key.replace(",", ", "), s0["ks"], s1["ks"], s0["ms"], s0["bytes"] / (s0["ms"] * 1e-3) / 1e12, s1["ms"],
            s1["bytes"] / (s1["ms"] * 1e-3) / 1e12, lo["encode_device_ms"], sh["encode_device_ms"], lo["encode_device_ms"] / sh["encode_device_ms"]))
    lines += ["", "## The commitment and a %d-column opening, at both widths" % OPENINGS, "",
              "| (n, c, rho) | width | commit wall ms | encode ms | column_leaf_kernel ms | tree ms | open wall ms | open device ms | opening bytes |",
              "|---|---|---|---|---|---|---|---|---|"]
    for key, row in shapes.items():
        for tag in ("long", "short"):
            k = row[tag]
            lines.append("| (%s) | c = %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %d |" % (
                key.replace(",", ", "), k["log_cols"], k["commit_wall_ms"], k["commit_encode_ms"], k["leaf_ms"], k["tree_ms"], k["open_wall_ms"],
                k["open_device_ms"], k["open_bytes"]))
    if res.get("notes"):
        lines += ["", "## What binds", ""] + res["notes"]
    return "\n".join(lines) + "\n"


def expander_summary(res):
    lines = ["# Expander code 1 on one MI355X: sc_xc_encode_rows beside sc_rs_encode_rows", "",
             "Measured by `python tools/ligero_timing.py --code expander --reps %d`: every row below, the Reed-Solomon column included, "
             "comes from ONE process, so the xc / rs ratio compares two kernels of the same run (`profiles/ligero_summary.md`, the "
             "default `--code rs` run, is a separate process and its `rs_encode_rows_kernel` times differ by a few per cent).  Device "
             "times: HIP events of the launch log, option `time_kernels`; wall times: median of %d calls after two warm-up calls.  Tables from "
             "`sc_table_generate`.  Both encoders read 8·2^n bytes and write 8·2^(n+1): 24·2^n in all, the same floor; the yardstick "
             "is the chip's measured copy rate, 6.29 TB/s." % (res["reps"], res["reps"]), "",
             "| (n, c) | field | xc_encode_rows_kernel device ms | wall ms | rs_encode_rows_kernel device ms (Goldilocks, rho = 1) | xc / rs | "
             "TB/s on 24·2^n bytes | of the 6.29 TB/s copy rate |", "|---|---|---|---|---|---|---|---|"]
    for key, row in res["steps"]["expander"]["shapes"].items():
        rs = row["rs_gold"]
        for name, label in (("gold", "Goldilocks"), ("p59", "2^64 - 59")):
            x = row["xc_" + name]
            bps = x["bytes"] / (x["device_ms"] * 1e-3)
            lines.append("| (%s) | %s | %.3f | %.3f | %.3f | %.1f | %.3f | %.1f %% |" % (key.replace(",", ", "), label, x["device_ms"], x["wall_ms"],
                                                                                   rs["device_ms"], x["device_ms"] / rs["device_ms"], bps / 1e12,
                                                                                   100 * bps / COPY_BPS))
    lines += ["", "## sc_ligero_commit_code(SC_CODE_EXPANDER): encode + column hash + tree", "",
              "| (n, c) | field | commit wall ms | encode ms | column hash ms | tree ms |", "|---|---|---|---|---|---|"]
    for key, row in res["steps"]["expander"]["shapes"].items():
        for name, label in (("gold", "Goldilocks"), ("p59", "2^64 - 59")):
            k = row["commit_" + name]
            lines.append("| (%s) | %s | %.3f | %.3f | %.3f | %.3f |" % (key.replace(",", ", "), label, k["wall_ms"], k["encode_ms"], k["leaf_ms"], k["tree_ms"]))
    return "\n".join(lines) + "\n"


def cpu_row(n=20, c=10, rho=1):
    """the same encoding through the numpy reference of the tests, one core"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ligero_ref as ref
    p = ref.GOLD
    table = [(0x9E3779B97F4A7C15 * (i + 1)) % p for i in range(1 << n)]
    t0 = time.perf_counter()
    ref.encode(table, c, rho, p)
    secs = time.perf_counter() - t0
    return {"shape": "%d,%d,%d" % (n, c, rho), "ms": secs * 1e3, "Bps": (8 * (1 << n) + 8 * (1 << (n + rho))) / secs}


def summary(res):
    lines = ["# Ligero-style commitment on one MI355X: row encoding, column hash, openings", "",
             "Measured by `python tools/ligero_timing.py --reps %d` (wall times: median of %d calls after two warm-up calls, host clock "
             "around the call and a device synchronise; device times: HIP events of the launch log, option `time_kernels`).  Goldilocks, "
             "tables from `sc_table_generate`." % (res["reps"], res["reps"]), "",
             "## sc_rs_encode_rows (`rs_encode_rows_kernel`, one launch)", "",
             "Bytes are the floor the kernel meets: 8·2^n read + 8·2^(n+rho) written.  The yardstick is the chip's measured copy rate, "
             "6.29 TB/s: a copy also reads and writes each word once.", "",
             "| (n, c, rho) | wall ms | device ms | bytes | wall TB/s | device TB/s | device / 8 TB/s peak | device / 6.29 TB/s copy |", "|---|---|---|---|---|---|---|---|"]
    for key, r in res["steps"]["encode"]["shapes"].items():
        lines.append("| (%s) | %.3f | %.3f | %d | %.2f | %.2f | %.0f %% | %.0f %% |" % (key.replace(",", ", "), r["wall_ms"], r["device_ms"], r["bytes"],
                                                                                  r["wall_Bps"] / 1e12, r["device_Bps"] / 1e12,
                                                                                  100 * r["device_Bps"] / PEAK_BPS, 100 * r["device_Bps"] / COPY_BPS))
    cpu = res.get("cpu") or {"shape": "20,10,1", "ms": float("nan"), "Bps": float("nan")}
    lines += ["", "**CPU row** (one core, the numpy reference of `tests/ligero_ref.py`, arrays of Python integers): shape (%s) in %.0f ms = "
              "%.3g B/s." % (cpu["shape"].replace(",", ", "), cpu["ms"], cpu["Bps"]), "",
              "## sc_ligero_commit, sc_ligero_combine_rows (M = 2), %d openings" % OPENINGS, "",
              "| (n, c, rho) | commit wall ms | encode ms | column hash ms | tree ms | leaf compressions | compressions/s | vs merkle_leaf_kernel 2.7e10/s | "
              "combine wall ms | combine device ms | open wall ms | open device ms |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, r in res["steps"]["commit"]["shapes"].items():
        k = r["kernels"]
        tree = sum(v["ms"] for name, v in k.items() if name.startswith("merkle"))
        lines.append("| (%s) | %.3f | %.3f | %.3f | %.3f | %d | %.3g | %.2f | %.3f | %.3f | %.3f | %.3f |" % (
            key.replace(",", ", "), r["commit_wall_ms"], k["rs_encode_rows_kernel"]["ms"], k["column_leaf_kernel"]["ms"], tree, r["leaf_compressions"],
            r["leaf_compressions_per_s"], r["leaf_compressions_per_s"] / MERKLE_LEAF_CPS, r["combine_wall_ms"], r["combine_device_ms"],
            r["open_wall_ms"], r["open_device_ms"]))
    lines += ["", "The column hash runs one lane per column: at L = 2^14 that is 2^14 lanes, one wave on each of the 256 CUs, against the "
              "2^24 lanes `merkle_leaf_kernel` spreads over the chip at n = 28 - the same compression function on the same chip, so the "
              "ratio column is what that occupancy costs.  The combine and open wall times include the host's copies of the weights, "
              "the values and the paths.", ""]
    if res.get("notes"):
        lines += ["## What binds the encoder", ""] + res["notes"] + [""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=("encode", "commit", "expander", "long", "xc_long", "fold", "fold_staged"))
    ap.add_argument("--fold", action="store_true", help="folded openings beside the plain opening (ligero_fold_summary.md)")
    ap.add_argument("--fold-staged", action="store_true", help="staged folded openings beside the binary fold (ligero_fold_staged_summary.md)")
    ap.add_argument("--long", action="store_true", help="rows longer than the LDS beside the in-LDS encoder (ligero_long_summary.md)")
    ap.add_argument("--code", choices=("rs", "expander"), default="rs", help="expander: the expander code beside Reed-Solomon (expander_summary.md)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=600, help="seconds each child step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of ligero_timing.json / ligero_summary.md")
    ap.add_argument("--trace", action="store_true", help="also one rocprofv3 --kernel-trace --stats run of the encode step")
    ap.add_argument("--skip-cpu", action="store_true", help="leave the CPU row out (add it later with --cpu-only)")
    ap.add_argument("--cpu-only", action="store_true", help="measure the CPU row alone (no GPU needed), add it to ligero_timing.json, rewrite the summary")
    ap.add_argument("--summary-only", action="store_true", help="rewrite ligero_summary.md from ligero_timing.json")
    ap.add_argument("--parent", nargs=2, metavar="JSON", help="with --fold --summary-only: two ligero_fold_timing.json of the parent commit to set this run against")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ligero_timing.json")
    if (args.long or args.fold or args.fold_staged) and not args.step:
        step, stem, render = ("xc_long", "expander_long", xc_long_summary) if args.code == "expander" else ("long", "ligero_long", long_summary)
        if args.fold:
            step, stem, render = "fold", "ligero_fold", fold_summary
        if args.fold_staged:
            step, stem, render = "fold_staged", "ligero_fold_staged", fold_staged_summary
        long_path = os.path.join(args.out, stem + "_timing.json")
        if args.summary_only:
            with open(long_path) as fh:
                res = json.load(fh)
            if args.parent:
                res["parents"] = [json.load(open(f)) for f in args.parent]
                with open(long_path, "w") as fh:
                    json.dump(res, fh, indent=1)
        else:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            if p.returncode != 0:
                print(json.dumps({"step": step, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}))
                sys.exit(1)
            res = {"reps": args.reps, "steps": {step: json.loads(p.stdout.strip().splitlines()[-1])}}
            with open(long_path, "w") as fh:
                json.dump(res, fh, indent=1)
        with open(os.path.join(args.out, stem + "_summary.md"), "w") as fh:
            fh.write(render(res))
        if args.fold_staged:
            print(json.dumps({k: {name: {"bytes": row[name]["opening_bytes"], "fold_device_ms": round(row[name]["fold_device_ms"], 3),
                                         **{t: round(v, 2) for t, v in row[name]["wall_ms"].items()}} for name in ("binary", "staged")}
                              for k, row in res["steps"][step]["shapes"].items()}))
            return
        if args.fold:
            print(json.dumps({k: {"fold_device_ms": round(row["fold_device_ms"], 3), **{t: round(v, 2) for t, v in row["wall_ms"].items()}}
                              for k, row in res["steps"][step]["shapes"].items()}))
            return
        print(json.dumps({k: {t: round(v["encode_device_ms"], 3) for t, v in row.items()} for k, row in res["steps"][step]["shapes"].items()}))
        return
    if args.summary_only or args.cpu_only:
        with open(path) as fh:
            res = json.load(fh)
        if args.cpu_only:
            res["cpu"] = cpu_row()
            with open(path, "w") as fh:
                json.dump(res, fh, indent=1)
        with open(os.path.join(args.out, "ligero_summary.md"), "w") as fh:
            fh.write(summary(res))
        return
    if args.step:
        runs = {"expander": run_expander, "long": run_long, "xc_long": run_xc_long, "fold": run_fold, "fold_staged": run_fold_staged}
        print(json.dumps(runs[args.step](args.reps) if args.step in runs else run_step(args.step, args.reps)))
        return
    if args.code == "expander":
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "expander", "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if p.returncode != 0:
            print(json.dumps({"step": "expander", "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}))
            sys.exit(1)
        res = {"reps": args.reps, "steps": {"expander": json.loads(p.stdout.strip().splitlines()[-1])}}
        with open(os.path.join(args.out, "expander_timing.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.join(args.out, "expander_summary.md"), "w") as fh:
            fh.write(expander_summary(res))
        print(json.dumps({k: {t: round(v["device_ms"], 3) for t, v in row.items() if "device_ms" in v} for k, row in res["steps"]["expander"]["shapes"].items()}))
        return
    res = {"reps": args.reps, "steps": {}}
    for step in ("encode", "commit"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if p.returncode != 0:
            print(json.dumps({"step": step, "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}))
            sys.exit(1)                                  # nothing more on the GPU after a failed step
        res["steps"][step] = json.loads(p.stdout.strip().splitlines()[-1])
    if args.trace:
        d = tempfile.mkdtemp()
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "encode", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--step", "encode", "--reps", "1"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if p.returncode != 0:
            print(json.dumps({"trace": "encode", "error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}))
            sys.exit(1)
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            shutil.copy(f, os.path.join(args.out, "ligero_kernel_stats.csv"))
        shutil.rmtree(d, ignore_errors=True)
    if not args.skip_cpu:
        res["cpu"] = cpu_row()
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out, "ligero_summary.md"), "w") as fh:
        fh.write(summary(res))
    print(json.dumps({"encode_device_TBps": {k: round(v["device_Bps"] / 1e12, 3) for k, v in res["steps"]["encode"]["shapes"].items()}, "cpu": res.get("cpu")}))


if __name__ == "__main__":
    main()
