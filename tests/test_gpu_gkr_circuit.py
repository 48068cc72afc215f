"""A GKR circuit resident on the GPU (sc_circuit_*): Circuit::evaluate by circuit_layer_kernel, the layer prover made from
the device gate list (sc_gkr_prover_create_circuit), the whole prover in one call (sc_gkr_prove_circuit) and the
interactive Prover in device mode - against the oracle's restatement of the protocol (pyref.circuit_evaluate,
pyref.gkr_transcript), against the host sparse path where the dense oracle cannot go, and the refusals."""
import ctypes
import random

import numpy as np
import pytest

from conftest import load_package
from test_gpu_gkr import make_circuit, random_circuit
from test_host_protocols import BOOK, THREE, gkr_draw_count
from util import GOLD, pid, pyref

pytestmark = pytest.mark.gpu

P59 = 2**64 - 59
THREE_FIELDS = [GOLD, P59, 389]
BOTH_FIELDS = [GOLD, 389]
BOOK_CASE = (BOOK, 4, [3, 2, 3, 1])
THREE_CASE = (THREE, 8, [0, 1] * 4)


def ks_of(layers, num_inputs):
    return [(len(l) - 1).bit_length() for l in layers] + [(num_inputs - 1).bit_length()]


def np_layers(layers):
    return [(np.array([0 if t == "add" else 1 for t, _, _ in l], dtype=np.int32), np.array([a for _, a, _ in l], dtype=np.uint32),
             np.array([b for _, _, b in l], dtype=np.uint32)) for l in layers]


def edge_circuit(rng, ks):
    """random_circuit plus the gates worth singling out: in0 == in1, and a run of gates that all read one input"""
    layers = random_circuit(rng, ks)
    for layer in layers:
        n = len(layer)
        for a in range(0, n, 3):
            t, i0, _ = layer[a]
            layer[a] = (t, i0, i0)
        for a in range(n // 2, n // 2 + max(n // 4, 1)):
            layer[a] = (layer[a][0], 0, layer[a][2] if a % 2 else 0)
    return layers


def poly_from_evals(e, p):
    """coefficients of the quadratic through (0, e0), (1, e1), (2, e2), canonical ints"""
    inv2 = pow(2, -1, p)
    c2 = (e[2] - 2 * e[1] + e[0]) * inv2 % p
    return [e[0] % p, (e[1] - e[0] - c2) % p, c2]


def poly_eval(c, x, p):
    return sum(ci * pow(x, i, p) for i, ci in enumerate(c)) % p


# ---- 1. evaluation against the oracle -----------------------------------------------------------------------------

@pytest.mark.parametrize("p", THREE_FIELDS, ids=pid)
def test_evaluate_matches_oracle(p):
    pkg = load_package()
    gp = pkg.gkr_protocol
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    rng = random.Random(p % 10007)
    cases = [BOOK_CASE, THREE_CASE]
    for ks in ([1, 2, 3, 2], [3, 5, 4], [0, 4, 6, 6], [12, 14, 13]):
        cases.append((edge_circuit(rng, ks), 1 << ks[-1], [rng.randrange(p) for _ in range(1 << ks[-1])]))
    for n_case, (layers, num_inputs, inputs) in enumerate(cases):
        want = pyref.circuit_evaluate(layers, inputs, p)
        k = ks_of(layers, num_inputs)
        # the reference-shaped constructor for the two book circuits, the array one for the rest
        dc = gp.DeviceCircuit(ctx, make_circuit(pkg, layers, num_inputs)) if n_case < 2 else \
            gp.DeviceCircuit.from_arrays(ctx, k, np_layers(layers))
        vals = dc.evaluate(F.from_ints(inputs))
        assert len(vals) == len(layers)
        for i, v in enumerate(vals):
            assert v.num_vars() == k[i]
            assert F.to_ints(v.to_evaluations()) == want[i], (n_case, i)
    assert [F.to_ints(v.to_evaluations()) for v in
            gp.DeviceCircuit(ctx, make_circuit(pkg, BOOK, 4)).evaluate(F.from_ints([3, 2, 3, 1]))] == [[36, 6], [9, 4, 6, 1]]


def test_evaluate_shows_in_the_launch_log():
    pkg = load_package()
    gp = pkg.gkr_protocol
    ctx = pkg.Context(pkg.Field(GOLD))
    ctx.set_option("time_kernels", 1)
    ctx.launch_log(reset=True)
    k = [10, 12, 11]
    dc = gp.DeviceCircuit.from_arrays(ctx, k, np_layers(random_circuit(random.Random(1), k)))
    dc.evaluate(ctx.field.from_ints(range(1 << 11)))
    recs = [r for r in ctx.launch_log() if r["kind"] == "circuit"]
    assert [(r["log_in"], r["kf"]) for r in recs] == [(12, 11), (10, 12)]      # from the input up
    assert [r["bytes_read"] + r["bytes_written"] for r in recs] == [20 << 12, 20 << 10]


# ---- 2. evaluation at scale -----------------------------------------------------------------------------------------

def _big_arrays(gen, k):
    out = []
    for i in range(len(k) - 1):
        n, n_next = 1 << k[i], 1 << k[i + 1]
        out.append((gen.integers(0, 2, n, dtype=np.int32), gen.integers(0, n_next, n, dtype=np.uint32),
                    gen.integers(0, n_next, n, dtype=np.uint32)))
    return out


@pytest.mark.parametrize("p", [389, GOLD], ids=pid)
def test_evaluate_at_scale(p):
    """layers of 2^22 gates; every layer checked from the device's own layer below it (the input: the one uploaded) -
    every gate over p = 389 (numpy), a random sample of 2^16 gates per layer over Goldilocks"""
    pkg = load_package()
    gp = pkg.gkr_protocol
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    gen = np.random.default_rng(22)
    k = [22, 22, 21, 22]
    arrays = _big_arrays(gen, k)
    inp = gen.integers(0, p, 1 << k[-1], dtype=np.uint64)             # any word < p is a Montgomery word
    dc = gp.DeviceCircuit.from_arrays(ctx, k, arrays)
    vals = [v.to_evaluations() for v in dc.evaluate(inp)] + [inp]
    for i, (t, a, b) in enumerate(arrays):
        below, got = vals[i + 1], vals[i]
        if p == 389:
            rinv = pow(2**64, -1, p)
            can = lambda m: (m.astype(np.int64) * rinv) % p               # Montgomery word -> canonical (m < 389)
            x, y, z = can(below)[a], can(below)[b], can(got)
            want = np.where(t == 1, (x * y) % p, (x + y) % p)
            assert np.array_equal(z, want), i
        else:
            for g in gen.integers(0, 1 << k[i], 1 << 16):
                x, y = int(below[a[g]]), int(below[b[g]])
                assert int(got[g]) == (F.mul(x, y) if t[g] else F.add(x, y)), (i, int(g))


# ---- 3. the whole prover in one call --------------------------------------------------------------------------------

class ScriptedDraw:
    """draw(t, evals) from a list of canonical ints; records which draws came with a round's sums"""

    def __init__(self, F, draws):
        self.F, self.draws, self.seen = F, list(draws), []

    def __call__(self, t, evals):
        assert t == len(self.seen)
        self.seen.append(None if evals is None else self.F.to_ints(evals))
        return self.F.from_int(self.draws[t])


def check_against_transcript(F, rec, ref, inputs, p):
    """rec (Montgomery words, prove_circuit) equals ref (canonical ints, pyref.gkr_transcript); the claim chain holds"""
    assert F.to_ints(rec["circuit_outputs"]) == ref["circuit_outputs"]
    assert F.to_ints(rec["r_0"]) == ref["r_0"]
    assert F.to_int(rec["layers"][0]["c_1"]) == pyref.mle_evaluate(ref["circuit_outputs"], ref["r_0"], p)
    for i, (a, b) in enumerate(zip(rec["layers"], ref["layers"])):
        assert F.to_int(a["c_1"]) == b["c_1"], i
        ev = [F.to_ints(e) for e in a["evals"]]
        assert ev == [list(e) for e in b["evals"]], i
        assert [poly_from_evals(e, p) for e in ev] == [c + [0] * (3 - len(c)) for c in b["coeffs"]], i
        assert F.to_ints(a["challenges"]) == b["challenges"], i
        assert F.to_ints(a["q"]) == b["q"] + [0] * (len(a["q"]) - len(b["q"])), i
        assert F.to_int(a["r_line"]) == b["r_line"] and F.to_ints(a["r_next"]) == b["r_next"], i
    last = rec["layers"][-1]
    assert poly_eval(F.to_ints(last["q"]), F.to_int(last["r_line"]), p) == \
        pyref.mle_evaluate([x % p for x in inputs], F.to_ints(last["r_next"]), p)


def expected_silent_draws(k):
    """draw indices that follow no round message: r_0, and per layer final_random_point and the line draw"""
    out, t = list(range(k[0])), k[0]
    for kn in k[1:]:
        out += [t + 2 * kn - 1, t + 2 * kn]
        t += 2 * kn + 1
    return out


def prove_and_check(pkg, ctx, layers, num_inputs, inputs, draws, p):
    gp = pkg.gkr_protocol
    F = ctx.field
    k = ks_of(layers, num_inputs)
    ref = pyref.gkr_transcript(layers, num_inputs, inputs, draws, p)
    dc = gp.DeviceCircuit.from_arrays(ctx, k, np_layers(layers))
    draw = ScriptedDraw(F, draws)
    rec = gp.prove_circuit(ctx, dc, F.from_ints(inputs), draw=draw)
    check_against_transcript(F, rec, ref, inputs, p)
    assert len(draw.seen) == len(draws)
    assert [t for t, e in enumerate(draw.seen) if e is None] == expected_silent_draws(k)
    # a draw that follows a round message sees that round's sums
    rounds = [e for l in ref["layers"] for e in l["evals"][:-1]]
    assert [e for e in draw.seen if e is not None] == [list(e) for e in rounds]
    return rec


@pytest.mark.parametrize("p", BOTH_FIELDS, ids=pid)
@pytest.mark.parametrize("case", [BOOK_CASE, THREE_CASE], ids=["book", "three_layer"])
def test_prove_circuit_reference_circuits(case, p):
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    layers, num_inputs, inputs = case
    for seed in range(6):
        rng = random.Random(100 + seed)
        draws = [rng.randrange(p) for _ in range(gkr_draw_count(layers, num_inputs))]
        rec = prove_and_check(pkg, ctx, layers, num_inputs, inputs, draws, p)
        if p == 389:
            assert ctx.field.to_ints(rec["circuit_outputs"]) == ([36, 6] if layers is BOOK else [2, 2])


@pytest.mark.parametrize("p", BOTH_FIELDS, ids=pid)
def test_prove_circuit_random_deep(p):
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    rng = random.Random(p % 1000 + 1)
    for ks in ([1, 2, 3, 2], [2, 3, 4, 4, 3], [3, 5, 4], [1, 1, 1, 1]):
        layers = random_circuit(rng, ks)
        num_inputs = 1 << ks[-1]
        inputs = [rng.randrange(p) for _ in range(num_inputs)]
        draws = [rng.randrange(p) for _ in range(gkr_draw_count(layers, num_inputs))]
        prove_and_check(pkg, ctx, layers, num_inputs, inputs, draws, p)


@pytest.mark.parametrize("p", BOTH_FIELDS, ids=pid)
def test_prove_circuit_synthetic_challenger(p):
    """draw=None: challenge t = to_mont(splitmix64(seed_r + t + 1) mod p)"""
    pkg = load_package()
    gp = pkg.gkr_protocol
    ctx = pkg.Context(pkg.Field(p))
    rng = random.Random(5)
    ks = [2, 3, 4, 3]
    layers = random_circuit(rng, ks)
    inputs = [rng.randrange(p) for _ in range(1 << ks[-1])]
    seed_r = 0x5EED
    draws = [pyref.synth_challenge(seed_r, t + 1, p) for t in range(gkr_draw_count(layers, 1 << ks[-1]))]
    ref = pyref.gkr_transcript(layers, 1 << ks[-1], inputs, draws, p)
    dc = gp.DeviceCircuit.from_arrays(ctx, ks, np_layers(layers))
    rec = gp.prove_circuit(ctx, dc, ctx.field.from_ints(inputs), seed_r=seed_r)
    check_against_transcript(ctx.field, rec, ref, inputs, p)


# ---- 4. the interactive Prover in device mode, driven by the existing Verifier -------------------------------------

class Scripted:
    """RngF fed from a list (canonical ints -> Montgomery words), in the order the reference draws"""

    def __init__(self, F, draws):
        self.F, self.draws, self.used = F, list(draws), 0

    def draw(self):
        v = self.F.from_int(self.draws[self.used])
        self.used += 1
        return v


def dense(F, poly, n):
    out = [0] * n
    for d, c in poly.coeffs:
        out[d] = F.to_int(c)
    return out


def run_protocol_device(pkg, ctx, layers, num_inputs, inputs, draws):
    """the message loop of protocol_test_from_book / three_layer_protocol_test with Prover.new(..., device=True)"""
    gp = pkg.gkr_protocol
    F = ctx.field
    circuit = make_circuit(pkg, layers, num_inputs)
    rng = Scripted(F, draws)
    win = F.from_ints(inputs).tolist()
    prover = gp.Prover.new(ctx, circuit, win, device=True)
    assert prover.evaluation is None                       # nothing of the layers on the host
    begin = prover.start_protocol()
    verifier = gp.Verifier.new(ctx, circuit)
    msg = verifier.receive_prover_msg(begin, rng)
    r_i = msg.r
    rec = {"circuit_outputs": F.to_ints(begin.circuit_outputs), "r_0": F.to_ints(r_i), "m_0": F.to_int(verifier.m[0]), "layers": []}
    for i in range(len(circuit.layers)):
        start = prover.start_round(i, r_i)
        num_vars = 2 * circuit.num_vars_at(i + 1)
        assert start.kind == "StartSumCheck" and start.num_vars == num_vars and start.round == i
        assert verifier.receive_prover_msg(start, rng).kind == "RoundStarted"
        coeffs = []
        for j in range(num_vars - 1):
            pm = prover.round_msg(j)
            assert pm.kind == "SumCheckProverMessage"
            coeffs.append(dense(F, pm.p, 3))
            vm = verifier.receive_prover_msg(pm, rng)
            assert vm.kind == "SumCheckRoundResult" and not vm.res.is_final()
            prover.receive_verifier_msg(vm)
        prover.receive_verifier_msg(verifier.final_random_point(rng))
        pm = prover.round_msg(num_vars - 1)
        assert pm.kind == "FinalRoundMessage"
        coeffs.append(dense(F, pm.p, 3))
        vm = verifier.receive_prover_msg(pm, rng)
        assert vm.kind == "R"
        r_i = vm.r
        rec["layers"].append({"c_1": F.to_int(start.c_1), "coeffs": coeffs, "q": dense(F, pm.q, num_vars // 2 + 1),
                              "r_next": F.to_ints(r_i), "m_next": F.to_int(verifier.m[-1])})
    rec["check_input"] = verifier.check_input(win)
    assert rng.used == len(draws)
    return rec, verifier


def compare(rec, ref):
    assert rec["circuit_outputs"] == ref["circuit_outputs"]
    assert rec["r_0"] == ref["r_0"] and rec["m_0"] == ref["m_0"]
    for i, (a, b) in enumerate(zip(rec["layers"], ref["layers"])):
        assert a["c_1"] == b["c_1"], i
        assert a["coeffs"] == [c + [0] * (3 - len(c)) for c in b["coeffs"]], i
        assert a["q"] == b["q"] + [0] * (len(a["q"]) - len(b["q"])), i
        assert a["r_next"] == b["r_next"] and a["m_next"] == b["m_next"], i
    assert rec["check_input"] == ref["check_input"]


@pytest.mark.parametrize("p", BOTH_FIELDS, ids=pid)
def test_device_prover_driven_by_verifier(p):
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    rng = random.Random(31)
    cases = [BOOK_CASE, THREE_CASE]
    for ks in ([2, 3, 4, 4, 3], [3, 5, 4]):
        cases.append((random_circuit(rng, ks), 1 << ks[-1], [rng.randrange(p) for _ in range(1 << ks[-1])]))
    for layers, num_inputs, inputs in cases:
        for seed in range(3):
            draws = [rng.randrange(p) for _ in range(gkr_draw_count(layers, num_inputs))]
            rec, verifier = run_protocol_device(pkg, ctx, layers, num_inputs, inputs, draws)
            assert rec["check_input"] is True
            compare(rec, pyref.gkr_transcript(layers, num_inputs, inputs, draws, p))
            # change one input whose weight eq(r_d, x) in the final claim is not zero (sum_x eq(r_d, x) = 1: one exists)
            x = next(x for x, e in enumerate(eq_table(F.to_ints(verifier.r[-1]), p)) if e)
            bad = F.from_ints(inputs[:x] + [(inputs[x] + 1) % p] + inputs[x + 1:]).tolist()
            assert verifier.check_input(bad) is False


# ---- 5. beyond the dense oracle ----------------------------------------------------------------------------------------

def eq_table(r, p):
    t = [1]
    for rj in r:
        t = [x * (1 - rj) % p for x in t] + [x * rj % p for x in t]
    return t


def verify_canonical(k, layers_np, outputs, inputs, tr, p):
    """the GKR verifier over canonical ints with add_i / mul_i evaluated from the gate list: sum over gates of
    eq(r_i, a) eq(b*, in0) eq(c*, in1).  tr: {"r_0", "layers": [{"c_1", "coeffs", "challenges", "q", "r_line"}]}"""
    r = tr["r_0"]
    m = pyref.mle_evaluate(outputs, r, p)
    for i, (t, a, b) in enumerate(layers_np):
        L = tr["layers"][i]
        kn = k[i + 1]
        assert L["c_1"] == m, i
        claim, ch = m, L["challenges"]
        for j, c in enumerate(L["coeffs"]):
            assert (poly_eval(c, 0, p) + poly_eval(c, 1, p)) % p == claim, (i, j)
            claim = poly_eval(c, ch[j], p)
        bs, cs = ch[:kn], ch[kn:]
        er, eb, ec = eq_table(r, p), eq_table(bs, p), eq_table(cs, p)
        add_v = mul_v = 0
        for g in range(len(t)):
            v = er[g] * eb[int(a[g])] % p * ec[int(b[g])] % p
            if t[g]:
                mul_v += v
            else:
                add_v += v
        q = L["q"]
        q0, q1 = poly_eval(q, 0, p), poly_eval(q, 1, p)
        assert claim == (add_v * (q0 + q1) + mul_v * q0 * q1) % p, i
        r = [(x + L["r_line"] * (y - x)) % p for x, y in zip(bs, cs)]
        m = poly_eval(q, L["r_line"], p)
    assert pyref.mle_evaluate(inputs, r, p) == m


def test_beyond_the_dense_oracle():
    """depth 4, 2^16-gate layers: the one-call transcript equals the host sparse path's, message for message (that path's
    Prover driven directly: the Verifier's dense wiring tables would have 4^16 entries per layer), and a verifier over
    canonical ints accepts it"""
    pkg = load_package()
    gp, scp = pkg.gkr_protocol, pkg.sum_check_protocol
    p = GOLD
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    gen = np.random.default_rng(16)
    k = [16, 16, 16, 16, 16]
    arrays = _big_arrays(gen, k)
    inputs = [int(x) for x in gen.integers(0, p, 1 << k[-1], dtype=np.uint64)]
    draws = [int(x) for x in gen.integers(0, p, k[0] + sum(2 * kn + 1 for kn in k[1:]), dtype=np.uint64)]
    win = F.from_ints(inputs)
    dc = gp.DeviceCircuit.from_arrays(ctx, k, arrays)
    rec = gp.prove_circuit(ctx, dc, win, draw=lambda t, e: F.from_int(draws[t]))
    # the host sparse path, same challenges
    circuit = gp.Circuit([gp.CircuitLayer([gp.Gate("add" if tt == 0 else "mul", [int(x), int(y)]) for tt, x, y in zip(*arr)])
                          for arr in arrays], 1 << k[-1])
    host = gp.Prover.new(ctx, circuit, win.tolist(), sparse=True)
    assert host.start_protocol().circuit_outputs == rec["circuit_outputs"]
    t = k[0]
    r_i = [F.from_int(x) for x in draws[:t]]
    assert r_i == rec["r_0"]
    for i in range(len(arrays)):
        L = rec["layers"][i]
        n = 2 * k[i + 1]
        start = host.start_round(i, r_i)
        assert start.c_1 == L["c_1"], i
        ch = [F.from_int(x) for x in draws[t:t + n]]
        for j in range(n):
            if j == n - 1:
                host.receive_verifier_msg(gp.VerifierMessage.SumCheckRoundResult(scp.VerifierRoundResult.JthRound(ch[n - 1])))
            pm = host.round_msg(j)
            assert dense(F, pm.p, 3) == poly_from_evals(F.to_ints(L["evals"][j]), p), (i, j)
            if j < n - 1:
                host.receive_verifier_msg(gp.VerifierMessage.SumCheckRoundResult(scp.VerifierRoundResult.JthRound(ch[j])))
        assert pm.kind == "FinalRoundMessage" and dense(F, pm.q, n // 2 + 1) == F.to_ints(L["q"]), i
        assert L["challenges"] == ch
        r_line = F.from_int(draws[t + n])
        assert L["r_line"] == r_line
        r_i = [F.add(b, F.mul(r_line, F.sub(c, b))) for b, c in zip(ch[:n // 2], ch[n // 2:])]
        assert r_i == L["r_next"], i
        t += n + 1
    tr = {"r_0": F.to_ints(rec["r_0"]), "layers": [
        {"c_1": F.to_int(L["c_1"]), "coeffs": [poly_from_evals(F.to_ints(e), p) for e in L["evals"]],
         "challenges": F.to_ints(L["challenges"]), "q": F.to_ints(L["q"]), "r_line": F.to_int(L["r_line"])} for L in rec["layers"]]}
    verify_canonical(k, arrays, F.to_ints(rec["circuit_outputs"]), inputs, tr, p)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

def expect(pkg, code, fn, *needles):
    with pytest.raises(pkg.SumcheckHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for n in needles:
        assert n in str(ei.value), (n, str(ei.value))


def still_works(pkg, ctx):
    gp = pkg.gkr_protocol
    F = ctx.field
    dc = gp.DeviceCircuit(ctx, make_circuit(pkg, BOOK, 4))
    assert F.to_ints(dc.evaluate(F.from_ints([3, 2, 3, 1]))[0].to_evaluations()) == [36, 6]
    rec = gp.prove_circuit(ctx, dc, F.from_ints([3, 2, 3, 1]), seed_r=9)
    assert F.to_ints(rec["circuit_outputs"]) == [36, 6]


def test_refusals_leave_the_context_usable():
    pkg = load_package()
    gp = pkg.gkr_protocol
    lib = pkg.load()
    p = 389
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    k = [2, 3, 2]
    base = np_layers(random_circuit(random.Random(2), k))

    def with_gate(layer, field, gate, value):
        arrs = [tuple(a.copy() for a in l) for l in base]
        arrs[layer][field][gate] = value
        return arrs

    expect(pkg, 1, lambda: gp.DeviceCircuit.from_arrays(ctx, k, with_gate(1, 0, 5, 2)), "layer 1 gate 5", "type 2")
    still_works(pkg, ctx)
    expect(pkg, 1, lambda: gp.DeviceCircuit.from_arrays(ctx, k, with_gate(0, 2, 3, 1 << k[1])), "layer 0 gate 3")
    expect(pkg, 1, lambda: gp.DeviceCircuit.from_arrays(ctx, k, with_gate(1, 1, 0, 1 << 20)), "layer 1 gate 0")
    still_works(pkg, ctx)
    # wrong k: a layer that reads no variables, or more than the sparse prover's 2^26
    expect(pkg, 1, lambda: gp.DeviceCircuit.from_arrays(ctx, [2, 0], base[:1]), "layer 0")
    expect(pkg, 1, lambda: gp.DeviceCircuit.from_arrays(ctx, [2, 27], base[:1]), "layer 0")
    still_works(pkg, ctx)
    dc = gp.DeviceCircuit.from_arrays(ctx, k, base)
    # wrong input length
    short = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, k[-1] - 1, F.from_ints(range(1 << (k[-1] - 1))))
    expect(pkg, 1, lambda: dc.evaluate(short), "input")
    expect(pkg, 1, lambda: gp.prove_circuit(ctx, dc, short), "input")
    still_works(pkg, ctx)
    # i >= depth
    inp = F.from_ints(range(1 << k[-1]))
    vals = dc.evaluate(inp)
    expect(pkg, 1, lambda: gp.CircuitLayerProver(ctx, dc, 2, [F.one] * k[1], vals[1]), "layer 2")
    expect(pkg, 1, lambda: gp.CircuitLayerProver(ctx, dc, 0, [F.one] * k[0], vals[0]), "layer 0")    # w_next of the wrong layer
    still_works(pkg, ctx)
    # a circuit from another context
    ctx2 = pkg.Context(pkg.Field(p))
    inp2 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx2, k[-1], inp)
    hs = (ctypes.c_void_p * 2)()
    expect(pkg, 1, lambda: ctx2.check(lib.sc_circuit_evaluate(ctx2.h, dc.h, inp2.h, hs)), "another context")
    expect(pkg, 1, lambda: ctx2.check(lib.sc_circuit_destroy(ctx2.h, dc.h)), "another context")
    out = ctypes.c_void_p()
    r = np.array([F.one] * k[0], dtype=np.uint64)
    expect(pkg, 1, lambda: ctx2.check(lib.sc_gkr_prover_create_circuit(ctx2.h, dc.h, 0, r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                                        inp2.h, ctypes.byref(out))), "another context")
    still_works(pkg, ctx2)
    still_works(pkg, ctx)
    # a one-device multi-device handle: no circuit is ever made on it, and the calls refuse it before looking at the circuit
    m = pkg.Context(pkg.Field(p), devices=[0, 0])
    expect(pkg, 6, lambda: gp.DeviceCircuit.from_arrays(m, k, base), "multi-device")
    minp = pkg.DenseMultilinearExtension.from_evaluations_vec(m, k[-1], inp)
    expect(pkg, 6, lambda: m.check(lib.sc_circuit_evaluate(m.h, dc.h, minp.h, hs)), "multi-device")
    expect(pkg, 6, lambda: m.check(lib.sc_circuit_evaluate(m.h, None, minp.h, hs)), "multi-device")
    expect(pkg, 6, lambda: m.check(lib.sc_gkr_prover_create_circuit(m.h, dc.h, 0, r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                                     minp.h, ctypes.byref(out))), "multi-device")
    expect(pkg, 6, lambda: gp.prove_circuit(m, dc, minp), "multi-device")
    del minp
    m.close()
    still_works(pkg, ctx)
    # a circuit destroyed while its context lives: the context makes, evaluates and proves a new one
    dc.close()
    del vals
    layers = random_circuit(random.Random(3), [2, 3, 2])
    inputs = [5, 7, 11, 13]
    draws = [random.Random(4).randrange(p) for _ in range(gkr_draw_count(layers, 4))]
    prove_and_check(pkg, ctx, layers, 4, inputs, draws, p)
    still_works(pkg, ctx)
