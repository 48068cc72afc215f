"""End-to-end time of the GKR prover on one circuit (default: 6 layers of 2^20 gates over Goldilocks), three ways:

  host     Prover.new(..., sparse=True): Circuit.evaluate in Python, every layer re-uploaded, its gate list re-checked and
           copied by sc_gkr_prover_create_sparse
  device   Prover.new(..., device=True): the circuit uploaded once, evaluated on the GPU, the layer provers made from the
           device-resident gate list and tables
  onecall  DeviceCircuit.from_arrays + prove_circuit (sc_gkr_prove_circuit): the whole prover in one native call

Each is timed from the prover's construction to the last layer's final message, driven with scripted challenges and no
Verifier (its dense wiring tables would have 4^20 entries per layer).  The Python Circuit is built before the clock starts,
its gate arrays cached on it (the host path would build them too).  `onecall` also reads circuit_layer_kernel's time per
layer from the launch log (option time_kernels) and rates it against the 20 B/gate streamed model (12 B of gate words,
one 8-B store; the two 8-B gathers are not counted).

  python tools/gkr_circuit_timing.py [--k 20] [--depth 6] [--limit 900]      every step in a child process of its own, each
                                                                             under its own time limit; one JSON line
  python tools/gkr_circuit_timing.py --step onecall [--k 20] [--depth 6]     one step, one JSON line (what the parent runs)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("host", "device", "onecall")


def make_arrays(k, depth, seed=20):
    gen = np.random.default_rng(seed)
    ks = [k] * (depth + 1)
    arrays = [(gen.integers(0, 2, 1 << k, dtype=np.int32), gen.integers(0, 1 << k, 1 << k, dtype=np.uint32),
               gen.integers(0, 1 << k, 1 << k, dtype=np.uint32)) for _ in range(depth)]
    return ks, arrays, gen


def run_step(step, k, depth):
    sys.path.insert(0, ROOT)
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    gp, scp = pkg.gkr_protocol, pkg.sum_check_protocol
    ctx = pkg.Context(pkg.Field(pkg.GOLDILOCKS))
    F = ctx.field
    ks, arrays, gen = make_arrays(k, depth)
    inputs = gen.integers(0, F.p, 1 << k, dtype=np.uint64)                 # Montgomery words
    n_draws = gp.transcript_sizes(ks)["draws"]
    draws = [int(x) for x in gen.integers(0, F.p, n_draws, dtype=np.uint64)]
    # warm-up on the book circuit: code objects, pool, first launches
    book = gp.Circuit([gp.CircuitLayer([gp.Gate("mul", [0, 1]), gp.Gate("mul", [2, 3])]),
                       gp.CircuitLayer([gp.Gate("mul", [0, 0]), gp.Gate("mul", [1, 1]), gp.Gate("mul", [1, 2]), gp.Gate("mul", [3, 3])])], 4)
    gp.prove_circuit(ctx, gp.DeviceCircuit(ctx, book), F.from_ints([3, 2, 3, 1]))
    out = {"step": step, "k": k, "depth": depth, "field": "goldilocks"}
    if step in ("host", "device"):
        t0 = time.perf_counter()
        circuit = gp.Circuit([gp.CircuitLayer([gp.Gate("add" if t == 0 else "mul", [int(a), int(b)]) for t, a, b in zip(*arr)])
                              for arr in arrays], 1 << k)
        for layer, arr in zip(circuit.layers, arrays):
            layer._arrays = arr
        out["circuit_build_s"] = time.perf_counter() - t0
        win = inputs.tolist()
        ctx.synchronize()
        t0 = time.perf_counter()
        prover = gp.Prover.new(ctx, circuit, win, sparse=(step == "host"), device=(step == "device"))
        begin = prover.start_protocol()
        t_new = time.perf_counter()
        t = k
        r_i = draws[:k]
        for i in range(depth):
            n = 2 * k
            prover.start_round(i, r_i)
            for j in range(n):
                if j == n - 1:
                    prover.receive_verifier_msg(gp.VerifierMessage.SumCheckRoundResult(scp.VerifierRoundResult.JthRound(draws[t + n - 1])))
                pm = prover.round_msg(j)
                if j < n - 1:
                    prover.receive_verifier_msg(gp.VerifierMessage.SumCheckRoundResult(scp.VerifierRoundResult.JthRound(draws[t + j])))
            assert pm.kind == "FinalRoundMessage"
            ch, r_line = draws[t:t + n], draws[t + n]
            r_i = [F.add(b, F.mul(r_line, F.sub(c, b))) for b, c in zip(ch[:k], ch[k:])]
            t += n + 1
        t1 = time.perf_counter()
        out.update(total_s=t1 - t0, new_and_begin_s=t_new - t0, layers_s=t1 - t_new, outputs_head=[int(x) for x in begin.circuit_outputs[:4]],
                   last_q=[dict(pm.q.coeffs).get(d, 0) for d in range(4)])
    else:
        ctx.synchronize()
        t0 = time.perf_counter()
        dc = gp.DeviceCircuit.from_arrays(ctx, ks, arrays)
        t_up = time.perf_counter()
        rec = gp.prove_circuit(ctx, dc, inputs, draw=lambda t, e: draws[t])
        t1 = time.perf_counter()
        out.update(total_s=t1 - t0, upload_s=t_up - t0, prove_s=t1 - t_up, outputs_head=rec["circuit_outputs"][:4],
                   last_q=rec["layers"][-1]["q"][:4])
        # circuit_layer_kernel per layer, from the launch log (3 evaluations; the median per layer)
        ctx.set_option("time_kernels", 1)
        ctx.launch_log(reset=True)
        per_layer = [[] for _ in range(depth)]
        for _ in range(3):
            vals = dc.evaluate(inputs)
            del vals
            recs = [r for r in ctx.launch_log() if r["kind"] == "circuit"]
            assert len(recs) == depth, recs
            for j, r in enumerate(recs):                   # launched from the input up
                per_layer[depth - 1 - j].append(r["ms"])
        ctx.set_option("time_kernels", 0)
        out["kernel_per_layer"] = [kernel_rates(statistics.median(ms), k) for ms in per_layer]
    return out


def kernel_rates(ctx_ms, k):
    gates = 1 << k
    return {"ms": ctx_ms, "streamed_GBps": 20 * gates / (ctx_ms * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--limit", type=int, default=900, help="seconds each child step may take")
    ap.add_argument("--out", help="also write the JSON line here")
    args = ap.parse_args()
    if args.step:
        res = run_step(args.step, args.k, args.depth)
    else:
        res = {"k": args.k, "depth": args.depth, "steps": {}}
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--k", str(args.k), "--depth", str(args.depth)]
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
        if all(x in s and "total_s" in s[x] for x in STEPS):
            assert s["host"]["outputs_head"] == s["device"]["outputs_head"] == s["onecall"]["outputs_head"]
            assert s["host"]["last_q"] == s["device"]["last_q"] == s["onecall"]["last_q"]
            res["speedup_vs_host"] = {x: s["host"]["total_s"] / s[x]["total_s"] for x in ("device", "onecall")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
