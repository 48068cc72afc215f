"""CPU-only: the batched-opening reference (tests/multiopen_ref.py) against the dense definitions; the package's host Verifier
(thaler-study_amd/multiopen.py) against the reference prover - honest runs are accepted, every single tampered message is refused
with its own error; batch_opening_bytes against the serialised messages; group_claims; and the per-element code of
kernels/multiopen.hpp, compiled for the host and run stand-alone (tests/cpp/multiopen_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import ligero_ref as lref
import multiopen_ref as ref
from conftest import ROOT, load_package
from multiopen_ref import GOLD, P64

MO = load_package().multiopen            # (the module under test: without it nothing here can run)

FIELDS = [(257, "rs"), (GOLD, "rs"), (P64, "expander")]
IDS = ["p257", "gold", "p64m59"]
SIZES = [(1, 1, 1), (2, 2, 3), (4, 3, 5), (5, 8, 16)]          # (n, T, K)


def case(p, n, T, K, seed):
    """(tables, claims) in canonical integers: every table carries a claim; with K > T the first further claim repeats claim 0's
    (table, point) pair, the next one repeats a table at a new point, the rest fall on random tables; points mix 0, 1, p - 1 in"""
    rng = random.Random(1000 * n + 100 * T + K + seed)
    tables = {"t%d" % t: [rng.randrange(p) for _ in range(1 << n)] for t in range(T)}
    names = list(tables)

    def point():
        return [rng.choice([0, 1, p - 1, rng.randrange(p), rng.randrange(p), rng.randrange(p)]) for _ in range(n)]
    claims = []
    for k in range(K):
        if k < T:
            name, pt = names[k], point()
        elif k == T:
            name, pt = claims[0][0], list(claims[0][1])
        elif k == T + 1:
            name, pt = names[T - 1], point()
        else:
            name, pt = rng.choice(names), point()
        claims.append((name, pt, lref.mle_eval(tables[name], pt, p)))
    return tables, claims


class AllColumns(random.Random):
    """the verifier's randomness of the tamper tests: field words as random.Random gives them, column indices 0, 1, 2, .. in turn -
    with `queries` = the number of columns every column is opened, and whether a tampered row is caught does not hang on the draw"""

    def __init__(self, seed):
        super().__init__(seed)
        self.turn = 0

    def randrange(self, start, stop=None, step=1):
        if stop is None and start <= 1 << 16:      # (a column index: the codewords here have at most 2^16 columns, the fields more words)
            self.turn += 1
            return (self.turn - 1) % start
        return super().randrange(start, stop, step)


def drive(pkg, p, code, n, T, K, seed, tamper=None, swap_roots=None, queries=None, all_columns=False):
    """the reference prover against the package's Verifier; tamper(tag, args) -> args rewrites one of the prover's messages (in
    canonical integers).  Returns (transcript, verifier)"""
    mo, F = pkg.multiopen, pkg.Field(p)
    tables, claims = case(p, n, T, K, seed)
    c = (n + 1) // 2
    prover = ref.RefProver(tables, c, p, code)
    roots = prover.roots()
    if swap_roots:
        a, b = swap_roots
        roots[a], roots[b] = roots[b], roots[a]
    L = 1 << (c + 1)
    queries = L if all_columns else (queries or 6)
    V = mo.Verifier(F, (n, c, 1), roots, queries, code)
    rng = AllColumns(seed + 7) if all_columns else random.Random(seed + 7)
    tamper = tamper or (lambda tag, args: args)

    def send(tag, *args):
        args = tamper(tag, args)
        if tag == "claims":
            return F.to_int(V.draw_rho([mo.Claim(name, lref.mont(p, pt), lref.mont(p, [v])[0]) for name, pt, v in args[0]], rng))
        if tag == "round":
            return F.to_int(V.round(args[0], lref.mont(p, args[1]), rng))
        if tag == "gamma":
            return [lref.canon(p, g) for g in V.draw_gamma(rng)]
        if tag == "rows":
            return V.receive(lref.mont(p, args[0]), lref.mont(p, args[1]))
        if tag == "columns":
            return V.draw_columns(rng)
        if tag == "open":
            return V.verify({t: [(j, lref.mont(p, col), pkg.ligero_pcs.ColumnPath(j, path, F)) for j, col, path in cols] for t, cols in args[0].items()})
        raise AssertionError(tag)
    out = ref.exchange(prover, claims, send)
    out.update(tables=tables, claims=claims, c=c, queries=queries)
    return out, V


@pytest.mark.parametrize("p,code", FIELDS, ids=IDS)
@pytest.mark.parametrize("n,T,K", SIZES)
def test_reference_against_the_dense_definitions(p, code, n, T, K):
    tables, claims = case(p, n, T, K, 0)
    names = list(tables)
    rng = random.Random(K)
    rho = rng.randrange(p)
    coeff = ref.powers(rho, K, p)
    assert len({name for name, _, _ in claims}) == T
    if K > T:
        assert (claims[T][0], claims[T][1]) == (claims[0][0], claims[0][1])           # a repeated (table, point) pair
    if K > T + 1:
        assert claims[T + 1][0] == names[T - 1] and claims[T + 1][1] != claims[T - 1][1]   # a table with two points
    E = ref.weight_tables(names, claims, rho, p)
    # the claim identity: sum_x sum_t f_t E_t = sum_k rho^k v_k
    total = sum(f * e for t in names for f, e in zip(tables[t], E[t])) % p
    assert total == sum(ck * v for ck, (_, _, v) in zip(coeff, claims)) % p
    rounds, z, finals, e = ref.sumcheck([tables[t] for t in names], [E[t] for t in names], p, lambda j, msg: rng.randrange(p))
    assert len(rounds) == len(z) == n and (rounds[0][0] + rounds[0][1]) % p == total
    claim = total
    for msg, r in zip(rounds, z):
        assert (msg[0] + msg[1]) % p == claim
        claim = ref.quadratic_at(msg, r, p)
        assert ref.quadratic_at(msg, 2, p) == msg[2]
    # the final identity: c = sum_t e_t f_t(z), e_t = sum_{k : t_k = t} rho^k eq(r_k, z), both by their definitions
    assert finals == [lref.mle_eval(tables[t], z, p) for t in names]
    assert e == [sum(ck * ref.eq_at(pt, z, p) for ck, (name, pt, _) in zip(coeff, claims) if name == t) % p for t in names]
    assert e == [lref.mle_eval(E[t], z, p) for t in names]
    assert claim == sum(et * ft for et, ft in zip(e, finals)) % p


@pytest.mark.parametrize("p,code", FIELDS, ids=IDS)
@pytest.mark.parametrize("n,T,K", SIZES)
def test_host_verifier_accepts_the_reference_prover(pkg, p, code, n, T, K):
    """over 257 only honest runs are tested: a random tamper can pass there by chance"""
    out, V = drive(pkg, p, code, n, T, K, 3)
    assert out["verdict"] is True
    F = pkg.Field(p)
    assert [F.to_int(x) for x in V.z] == out["z"] and [F.to_int(x) for x in V.e] == out["e"]
    # the size of the messages
    c = out["c"]
    assert len(ref.serialise(out)) == pkg.multiopen.batch_opening_bytes(n, c, 1, out["queries"], T)
    if T == 1:
        assert pkg.multiopen.batch_opening_bytes(n, c, 1, 6, 1) == pkg.ligero_pcs.opening_bytes(n, c, 1, 6) + 24 * n


def bump(tag_wanted, pick):
    def tamper(tag, args):
        return pick(args) if tag == tag_wanted else args
    return tamper


def refused(pkg, p, code, size, err, attrs, **kwargs):
    n, T, K = size
    with pytest.raises(err) as ei:
        drive(pkg, p, code, n, T, K, 5, all_columns=True, **kwargs)
    assert type(ei.value) is err, ei.value
    for k, want in attrs.items():
        assert getattr(ei.value, k) == want, (k, getattr(ei.value, k), want)
    return ei.value


@pytest.mark.parametrize("p,code", FIELDS[1:], ids=IDS[1:])
@pytest.mark.parametrize("n,T,K", [(2, 2, 3), (4, 3, 5)])
def test_host_verifier_refuses_every_single_tamper(pkg, p, code, n, T, K):
    """Goldilocks and 2^64 - 59 only: over 257 a random tamper can pass by chance (a changed word meets a zero weight with
    probability 1/257), so that field sees honest runs alone.  Every column is opened (AllColumns): which error a tampered row
    earns does not depend on the columns drawn"""
    mo, lp, size = pkg.multiopen, pkg.ligero_pcs, (n, T, K)
    c = (n + 1) // 2
    assert drive(pkg, p, code, n, T, K, 5, all_columns=True)[0]["verdict"] is True
    # a changed claimed value
    for k in range(K):
        def pick(args, k=k):
            claims = list(args[0])
            claims[k] = (claims[k][0], claims[k][1], (claims[k][2] + 1) % p)
            return (claims,)
        refused(pkg, p, code, size, mo.RoundMismatch, {"round": 0}, tamper=bump("claims", pick))
    # each value of each round: H(0), H(1) break the round's own sum, H(2) the claim it hands on
    for j in range(n):
        for t in range(3):
            def pick(args, j=j, t=t):
                if args[0] != j:
                    return args
                msg = list(args[1])
                msg[t] = (msg[t] + 1) % p
                return (j, msg)
            if t < 2:
                refused(pkg, p, code, size, mo.RoundMismatch, {"round": j}, tamper=bump("round", pick))
            elif j + 1 < n:
                refused(pkg, p, code, size, mo.RoundMismatch, {"round": j + 1}, tamper=bump("round", pick))
            else:
                refused(pkg, p, code, size, mo.FinalMismatch, {}, tamper=bump("round", pick))
    # a word of u_gamma, a word of u_z
    for at in (0, (1 << c) - 1):
        def pick_gamma(args, at=at):
            u = list(args[0])
            u[at] = (u[at] + 1) % p
            return (u, args[1])

        def pick_z(args, at=at):
            u = list(args[1])
            u[at] = (u[at] + 1) % p
            return (args[0], u)
        refused(pkg, p, code, size, lp.ProximityMismatch, {}, tamper=bump("rows", pick_gamma))
        refused(pkg, p, code, size, mo.FinalMismatch, {}, tamper=bump("rows", pick_z))
    # a u_z changed so that <u_z, eq(z[:c])> stays: the columns catch it
    state = {}

    def pick_kept(args):
        z_lo = state["z"][:c]
        w = lref.eq_weights(z_lo, p)
        u = list(args[1])
        u[0] = (u[0] + w[1]) % p
        u[1] = (u[1] - w[0]) % p
        return (args[0], u)
    honest, V = drive(pkg, p, code, n, T, K, 5, all_columns=True)
    state["z"] = honest["z"]                      # (the same seed draws the same challenges)
    assert any(x for x in lref.eq_weights(state["z"][:c], p)[:2])
    refused(pkg, p, code, size, mo.EvalMismatch, {}, tamper=bump("rows", pick_kept))
    # a column word of each commitment, a path byte of each, a swapped root
    names = list(honest["tables"])
    for t in names:
        def pick_word(args, t=t):
            op = {k: list(v) for k, v in args[0].items()}
            j, col, path = op[t][1]
            op[t][1] = (j, [(col[0] + 1) % p] + list(col[1:]), path)
            return (op,)

        def pick_path(args, t=t):
            op = {k: list(v) for k, v in args[0].items()}
            j, col, path = op[t][0]
            op[t][0] = (j, col, [bytes([path[0][0] ^ 1]) + path[0][1:]] + list(path[1:]))
            return (op,)
        assert refused(pkg, p, code, size, mo.MerkleMismatch, {"table": t}, tamper=bump("open", pick_word)).table == t
        refused(pkg, p, code, size, mo.MerkleMismatch, {"table": t}, tamper=bump("open", pick_path))
    refused(pkg, p, code, size, mo.MerkleMismatch, {"table": names[0]}, swap_roots=(names[0], names[1]))
    assert issubclass(mo.MerkleMismatch, lp.MerkleMismatch)


def test_group_claims_on_mixed_shapes(pkg):
    mo = pkg.multiopen
    shapes = {"a": (4, 2), "b": (4, 2), "c": (3, 2), "d": (4, 2), "e": (5, 3)}
    claims = [("a", [1], 1), ("c", [2], 2), ("b", [3], 3), ("a", [4], 4), ("e", [5], 5), ("c", [6], 6), ("d", [7], 7)]
    groups = mo.group_claims(claims, shapes)
    assert [(s, t, [c.value for c in cl]) for s, t, cl in groups] == [((4, 2), ["a", "b", "d"], [1, 3, 4, 7]), ((3, 2), ["c"], [2, 6]), ((5, 3), ["e"], [5])]
    assert all(isinstance(c, mo.Claim) for _, _, cl in groups for c in cl)
    with pytest.raises(ValueError):
        mo.group_claims([("zz", [1], 1)], shapes)
    # the limits of a group: a ninth table or a seventeenth claim opens a new group of the same shape
    many = {"t%d" % i: (1,) for i in range(10)}
    groups = mo.group_claims([("t%d" % i, [0], i) for i in range(10)], many)
    assert [len(t) for _, t, _ in groups] == [8, 2]
    groups = mo.group_claims([("t0", [0], i) for i in range(20)], many)
    assert [len(cl) for _, _, cl in groups] == [16, 4]


def test_verifier_guards(pkg):
    mo, F = pkg.multiopen, pkg.Field(GOLD)
    root = b"\0" * 32
    with pytest.raises(ValueError):
        mo.Verifier(F, (0, 0, 1), {"a": root}, 4)
    with pytest.raises(ValueError):
        mo.Verifier(F, (4, 2, 1), {}, 4)
    with pytest.raises(ValueError):
        mo.Verifier(F, (4, 2, 1), {"t%d" % i: root for i in range(9)}, 4)
    with pytest.raises(ValueError):
        mo.Verifier(F, (4, 5, 1), {"a": root}, 4)
    V = mo.Verifier(F, (2, 1, 1), {"a": root, "b": root}, 4)
    rng = random.Random(1)
    with pytest.raises(ValueError):
        V.draw_rho([("a", [0, 0], 0)], rng)                       # b carries no claim
    with pytest.raises(ValueError):
        V.draw_rho([("a", [0, 0], 0), ("c", [0, 0], 0)], rng)     # c is no commitment of the group
    with pytest.raises(ValueError):
        V.draw_rho([("a", [0, 0], 0), ("b", [0], 0)], rng)        # a point of the wrong length
    with pytest.raises(ValueError):
        V.draw_rho([("a", [0, 0], 0), ("b", [0, 0], 0)] * 9, rng)  # eighteen claims
    with pytest.raises(mo.Error):
        V.round(0, [0, 0, 0], rng)                                # before rho
    with pytest.raises(mo.Error):
        V.draw_gamma(rng)
    V.draw_rho([("a", [0, 0], 0), ("b", [0, 0], 0)], rng)
    with pytest.raises(mo.Error):
        V.round(1, [0, 0, 0], rng)
    with pytest.raises(mo.Error):
        V.receive([0, 0], [0, 0])
    with pytest.raises(mo.Error):
        V.draw_columns(rng)
    with pytest.raises(mo.Error):
        V.verify({})


def test_prove_claims_refuses_a_fold_verifier(pkg):
    """before anything touches a device: the prover objects are never reached"""
    mo, lp, F = pkg.multiopen, pkg.ligero_pcs, pkg.Field(GOLD)
    fv = lp.FoldVerifier(F, 4, 2, 1, b"\0" * 32, 4)
    with pytest.raises(ValueError, match="folded opening"):
        mo.prove_claims(None, {"a": None}, {"a": fv}, [("a", [0] * 4, 0), ("a", [1] * 4, 0)], random.Random(0))
    with pytest.raises(ValueError):
        mo.prove_claims(None, {}, {}, [("a", [0] * 4, 0)], random.Random(0))


def test_constants_match_the_kernel_header(pkg):
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "multiopen.hpp")).read()
    header = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    mo = pkg.multiopen
    for name, value in (("kEqSumMaxCount", mo.MAX_CLAIMS), ("kEqSumLoLog", mo.LO_LOG), ("kEqSumMaxLog", mo.MAX_LOG), ("kSumprodMaxPairs", mo.MAX_TABLES)):
        assert value == int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)), name
    assert "#define SC_KIND_EQ_SUM 36 " in header and "#define SC_KIND_SUMPROD_PASS 37 " in header
    names = pkg._lib.KIND_NAMES
    assert (names[36], names[37]) == ("eq_sum", "sumprod_pass")
    assert mo.batch_opening_bytes(14, 7, 1, 8, 5) == 8 * (3 * 14 + 2 * 128) + 8 * 5 * (8 * 128 + 32 * 8)


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/multiopen_host_harness.cpp, built and run stand-alone: the low table entry, the high factor and the per-entry sum of
    eq_sum_kernel, the fold and accumulate of the pass item, and the host rounds, against naive 128-bit loops on the edge words,
    both fields"""
    exe = tmp_path / "multiopen_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "multiopen_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "multiopen host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
