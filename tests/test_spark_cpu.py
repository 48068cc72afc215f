"""CPU-only: the SPARK reference (tests/spark_ref.py) against the dense definitions; the package's host Verifier
(thaler-study_amd/spark.py) against the reference prover - honest runs are accepted, every single tampered message is refused with
its own error; r1cs.SublinearVerifier next to r1cs.Verifier on the same instances; and the per-element code of kernels/spark.hpp,
compiled for the host and run stand-alone (tests/cpp/spark_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import r1cs_ref
import spark_cases as cases
import spark_ref as ref
import test_r1cs_cpu as rc
from conftest import ROOT, load_package
from spark_cases import GOLD, P64

SPARK = load_package().spark            # (the module under test: without it nothing here can run)

FIELDS = [257, GOLD, P64]
IDS = {257: "p257", GOLD: "gold", P64: "p64m59"}
SHAPES = [(1, 1, 1), (2, 3, 2), (3, 3, 4), (4, 2, 5)]          # (a, b, l)
NNZ = {1: 1, 2: 3, 4: 13, 5: 29}                              # l -> nnz: every list but the first is padded


def shape_case(p, a, b, ell, seed=0):
    triples, U, W = cases.case(p, a, b, NNZ[ell], 100 * a + 10 * b + ell + seed)
    assert ref.log_len(len(triples)) == ell
    return triples, U, W


@pytest.mark.parametrize("p", FIELDS, ids=[IDS[p] for p in FIELDS])
@pytest.mark.parametrize("a,b,ell", SHAPES)
def test_reference_against_the_dense_definitions(p, a, b, ell):
    triples, U, W = shape_case(p, a, b, ell)
    rng = random.Random(ell)
    _, rows, cols, vals = ref.pad(triples)
    N = 1 << ell
    assert len(rows) == len(cols) == len(vals) == N and list(zip(rows, cols, vals))[:len(triples)] == triples
    assert all(t == (0, 0, 0) for t in list(zip(rows, cols, vals))[len(triples):])
    # the padding counts in cr[0] and cc[0]
    cr, cc = ref.counts(rows, a), ref.counts(cols, b)
    assert sum(cr) == sum(cc) == N
    assert cr[0] == sum(1 for t in triples if t[0] == 0) + N - len(triples) and cc[0] == sum(1 for t in triples if t[1] == 0) + N - len(triples)
    assert cr == [rows.count(i) for i in range(1 << a)] and cc == [cols.count(j) for j in range(1 << b)]
    # with U = eq(r_x, .), W = eq(r_y, .) the claim is M~(r_x, r_y) of the dense matrix
    rx, ry = [rng.randrange(p) for _ in range(a)], [rng.randrange(p) for _ in range(b)]
    M = ref.dense(a, b, triples, p)
    ex, ey = ref.eq_table(rx, p), ref.eq_table(ry, p)
    assert sum(v * ex[i] * ey[j] for i, j, v in zip(rows, cols, vals)) % p == ref.dense_eval(M, rx, ry, p)
    # the tuple identity of both dimensions at an alpha outside the keys
    beta = rng.randrange(1, p)
    alpha = cases.alpha_outside(triples, U, W, beta, p, a, b, rng, {})
    for dim, (lhs, rhs) in cases.sums(triples, U, W, alpha, beta, p, a, b).items():
        assert lhs == rhs, dim
    # the whole exchange: the reference verifier accepts, and what it accepts is the dense sum
    words = random.Random(7 + ell)

    def draw():
        return words.randrange(4, p)
    state = {}
    V = ref.Verify(p, a, b, ell, lambda z: ref.mle_eval(U, z, p), lambda z: ref.mle_eval(W, z, p), draw)

    def send(tag, *args):
        if tag == "beta":                                     # alpha outside the keys, as above
            state["beta"] = V.send("beta")
            return state["beta"]
        if tag == "alpha":
            V.alpha = cases.alpha_outside(triples, U, W, state["beta"], p, a, b, words, {})
            return V.alpha
        return V.send(tag, *args)
    out = ref.exchange(p, a, b, triples, U, W, send)
    assert V.finish() == out["v"] == sum(M[i][j] * U[i] * W[j] for i in range(1 << a) for j in range(1 << b)) % p
    assert out["c1"] == out["v"] and len(out["rounds"]) == ell
    for msg in out["rounds"]:
        assert ref.cubic_at(msg, 2, p) == msg[2] and ref.cubic_at(msg, 3, p) == msg[3]
    # the finals and the last claims are the tables' extensions by their definition
    T = out["tables"]
    assert out["finals"] == tuple(ref.mle_eval(T[name], out["r"], p) for name in ("val", "er", "ec"))
    for dim, e, cnt in (("row", "er", "cr"), ("col", "ec", "cc")):
        w, t = out["fracs"][dim]
        assert w["claims"] == (1 % p, (out["alpha"] - ref.mle_eval(T[dim], w["point"], p) - out["beta"] * ref.mle_eval(T[e], w["point"], p)) % p)
        assert t["claims"][0] == ref.mle_eval(T[cnt], t["point"], p)


@pytest.mark.parametrize("p", FIELDS, ids=[IDS[p] for p in FIELDS])
@pytest.mark.parametrize("a,b,ell", SHAPES)
def test_host_verifier_accepts_the_reference_prover(pkg, p, a, b, ell):
    """over 257 (and, by the same path, over the larger fields) alpha is drawn outside the keys: spark_cases.alpha_outside says why"""
    triples, U, W = shape_case(p, a, b, ell)
    v, out = cases.drive(pkg, p, a, b, triples, U, W, 5)
    assert v == ref.mont(out["v"], p)


def bump(p, tag_wanted, pick):
    """a tamper: the message `tag_wanted` with pick(args) -> args applied"""
    def tamper(tag, args):
        return pick(args) if tag == tag_wanted else args
    return tamper


def refused(pkg, p, shape, err, attrs, **kwargs):
    a, b, ell = shape
    triples, U, W = shape_case(p, a, b, ell)
    with pytest.raises(err) as ei:
        cases.drive(pkg, p, a, b, triples, U, W, 9, **kwargs)
    assert type(ei.value) is err
    for k, want in attrs.items():
        assert getattr(ei.value, k) == want, (k, getattr(ei.value, k), want)


@pytest.mark.parametrize("p", FIELDS, ids=[IDS[p] for p in FIELDS])
@pytest.mark.parametrize("a,b,ell", [(2, 3, 2), (4, 2, 5)])
def test_host_verifier_refuses_every_single_tamper(pkg, p, a, b, ell):
    """challenges are words >= 4 (spark_cases.Draws says why); over 257 alpha is drawn outside the keys and, where the prover's
    tables are dishonest, where the two sums differ (spark_cases.alpha_outside)"""
    sp, shape = pkg.spark, (a, b, ell)
    # a changed v
    refused(pkg, p, shape, sp.RoundMismatch, {"round": 0}, tamper=bump(p, "v", lambda args: ((args[0] + 1) % p,)))
    # each value of every round: H(0), H(1) break the round's own sum, H(2), H(3) the claim it hands on
    for j in range(ell):
        for t in range(4):
            def pick(args, j=j, t=t):
                if args[0] != j:
                    return args
                msg = list(args[1])
                msg[t] = (msg[t] + 1) % p
                return (j, msg)
            if t < 2:
                refused(pkg, p, shape, sp.RoundMismatch, {"round": j}, tamper=bump(p, "round", pick))
            elif j + 1 < ell:
                refused(pkg, p, shape, sp.RoundMismatch, {"round": j + 1}, tamper=bump(p, "round", pick))
            else:
                refused(pkg, p, shape, sp.FinalMismatch, {}, tamper=bump(p, "round", pick))
    # each final
    for k in range(3):
        def pick(args, k=k):
            fin = list(args[0])
            fin[k] = (fin[k] + 1) % p
            return (tuple(fin),)
        refused(pkg, p, shape, sp.FinalMismatch, {}, tamper=bump(p, "finals", pick))
    # a root
    for dim in ("row", "col"):
        def pick(args, dim=dim):
            if args[0] != dim:
                return args
            return (dim, ((args[1][0] + 1) % p, args[1][1]), args[2])
        refused(pkg, p, shape, sp.LookupMismatch, {"dim": dim}, tamper=bump(p, "roots", pick))
    # a changed word of er or ec, a changed count: the transcript is the dishonest prover's own, the sums differ
    triples, U, W = shape_case(p, a, b, ell)
    _, rows, cols, _ = ref.pad(triples)
    er, ec = [U[i] for i in rows], [W[j] for j in cols]
    cr, cc = ref.counts(rows, a), ref.counts(cols, b)
    for name, table, dim in (("er", er, "row"), ("ec", ec, "col"), ("cr", cr, "row"), ("cc", cc, "col")):
        for at in (0, len(table) - 1):
            bad = list(table)
            bad[at] = (bad[at] + 1) % p
            refused(pkg, p, shape, sp.LookupMismatch, {"dim": dim}, dishonest={name: bad})
    # each of the nine opened values
    which = {("val", "r"): "val", ("er", "r"): "er", ("ec", "r"): "ec", ("er", "z_row"): "den_w row", ("row", "z_row"): "den_w row",
             ("ec", "z_col"): "den_w col", ("col", "z_col"): "den_w col", ("cr", "zt_row"): "cr", ("cc", "zt_col"): "cc"}
    assert sorted(which) == sorted(ref.OPENINGS) == sorted(sp.OPENINGS)
    for (table, at), name in which.items():
        def pick(args, table=table, at=at):
            if (args[0], args[1]) != (table, at):
                return args
            return (table, at, args[2], (args[3] + 1) % p)
        refused(pkg, p, shape, sp.InputMismatch, {"which": name}, tamper=bump(p, "open", pick))
    # a wrong u_eval, a wrong w_eval: the verifier's own table is not the prover's
    F = pkg.Field(p)
    refused(pkg, p, shape, sp.InputMismatch, {"which": "u"},
            u_eval=lambda z: F.add(ref.mont(ref.mle_eval(U, ref.canon_list(z, p), p), p), F.one))
    refused(pkg, p, shape, sp.InputMismatch, {"which": "w"},
            w_eval=lambda z: F.add(ref.mont(ref.mle_eval(W, ref.canon_list(z, p), p), p), F.one))

    # a last claim about the all-ones numerator that is not 1
    def not_one(V):
        V.frac["col"][0].a = F.add(V.frac["col"][0].a, F.one)
    refused(pkg, p, shape, sp.NumeratorMismatch, {"dim": "col"}, before_finish=not_one)


def test_verifier_guards(pkg):
    sp, O = pkg.spark, cases.Opening
    pcs = lambda ell, a, b: {"row": O(ell), "col": O(ell), "val": O(ell), "cr": O(a), "cc": O(b)}   # noqa: E731
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(3), 1, 1, 1, pcs(1, 1, 1), None, None)
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(257), 2, 2, 10, pcs(10, 2, 2), None, None)          # 257 <= 2^10
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(257), 9, 2, 3, pcs(3, 9, 2), None, None)            # nor above 2^9 row indices
    sp.Verifier(pkg.Field(257), 8, 2, 3, pcs(3, 8, 2), None, None)                # 257 > 2^8
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(GOLD), 0, 2, 3, pcs(3, 0, 2), None, None)
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(GOLD), 2, 29, 3, pcs(3, 2, 29), None, None)
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(GOLD), 2, 2, 3, pcs(3, 2, 3), None, None)           # cc over three variables
    V = sp.Verifier(pkg.Field(GOLD), 2, 2, 3, pcs(3, 2, 2), None, None)
    rng = random.Random(1)
    with pytest.raises(sp.Error):
        V.receive_claim(5)                                                        # before the roots of er and ec
    with pytest.raises(sp.Error):
        V.receive_commitments(O(2), O(3))
    V.receive_commitments(O(3), O(3))
    with pytest.raises(sp.Error):
        V.round(0, [0, 0, 0, 0], rng)                                             # before v
    with pytest.raises(sp.Error):
        V.draw_lookup(rng)                                                        # alpha and beta only after the finals
    with pytest.raises(sp.Error):
        V.openings()


def test_constants_match_the_kernel_header(pkg):
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "spark.hpp")).read()
    header = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    sp = pkg.spark
    assert sp.MAX_LOG == int(re.search(r"constexpr int kSparkMaxLog = (\d+);", text).group(1))
    for k, name in enumerate(sp.TABLES):
        assert re.search(r"#define SC_SPARK_%s %d\n" % (name.upper(), k), header), name
    names = pkg._lib.KIND_NAMES
    assert (names[33], names[34], names[35]) == ("spark_index", "spark_gather", "spark_tuple")
    assert [sp.log_len(n) for n in (1, 2, 3, 4, 5, 1024, 1025)] == [ref.log_len(n) for n in (1, 2, 3, 4, 5, 1024, 1025)] == [1, 1, 2, 2, 3, 10, 11]


# ---- the R1CS verifier that holds no matrices --------------------------------------------------------------------------

def combined(mats, s):
    """the triples of the one combined matrix: row k 2^s + i holds entry (i, j) of matrix k"""
    return [((k << s) + i, j, v) for k, M in enumerate(mats) for i, j, v in M]


def run_both(pkg, p, code, s, m, seed, flip=False):
    """the same instance and witness under r1cs.Verifier and under r1cs.SublinearVerifier (the reference provers of
    tests/test_r1cs_cpu.py and tests/spark_ref.py); returns what each run returned or raised"""
    rp = pkg.r1cs
    out = []
    for sublinear in (False, True):
        try:
            out.append(rc.run(pkg, p, code, s, m, seed, "w" if flip else None) if not sublinear else run_sublinear(pkg, p, code, s, m, seed, flip))
        except rp.Error as exc:
            out.append(exc)
    return out


def run_sublinear(pkg, p, code, s, m, seed, flip):
    rp, F = pkg.r1cs, pkg.Field(p)
    mats, io, w = rc.instance(p, s, m, seed)
    if flip:
        col = mats[0][0][1] - (1 << (m - 1))              # rc.run's "w": a witness word the first constraint reads
        w = list(w)
        w[col] = (w[col] + 1) % p
    prover = rc.MontProver(pkg, p, code, s, m, mats, io, w)
    root = prover.root()
    pv = pkg.ligero_pcs.Verifier(F, m - 1, prover.log_cols, 1, root, rc.QUERIES, code=code)
    triples = combined(mats, s)
    a, b, ell = s + 2, m, ref.log_len(len(triples))
    O = cases.Opening
    verifier = rp.SublinearVerifier(F, s, m, ref.mont_list(io, p), root, pv, {"row": O(ell), "col": O(ell), "val": O(ell), "cr": O(a), "cc": O(b)})
    assert verifier.r1cs is None
    rng = random.Random(seed + 1)
    finals = prover.sumcheck1(verifier.draw_tau(rng), lambda j, e: verifier.round1(j, e, rng))
    verifier.receive_finals(*finals)
    rho = verifier.draw_rho(rng)
    prover.bind(rho)
    prover.sumcheck2(lambda j, e: verifier.round2(j, e, rng))
    # T~(r_y) from the SPARK exchange over the combined matrix, the verifier's own u_eval and w_eval against the tables' definitions
    rx, ry, rho_c = ref.canon_list(verifier.rx, p), ref.canon_list(verifier.ry, p), ref.canon_list(rho, p)
    ex = ref.eq_table(rx, p)
    U = [rk * e % p for rk in rho_c for e in ex] + [0] * (1 << s)
    W = ref.eq_table(ry, p)
    probe = random.Random(3)
    for _ in range(3):
        z = [probe.randrange(p) for _ in range(a)]
        assert ref.canon(verifier.u_eval(ref.mont_list(z, p)), p) == ref.mle_eval(U, z, p)
        z = [probe.randrange(p) for _ in range(b)]
        assert ref.canon(verifier.w_eval(ref.mont_list(z, p)), p) == ref.mle_eval(W, z, p)
    t_value, _ = cases.drive(pkg, p, a, b, triples, U, W, seed + 2, u_eval=verifier.u_eval, w_eval=verifier.w_eval)
    assert ref.canon(t_value, p) == r1cs_ref.bind_eval_dense(mats, s, m, rx, ry, rho_c, p)
    w_value = rp.open_committed(prover.pcs, pv, verifier.point(), rng)
    return verifier.finish(w_value, t_value)


@pytest.mark.parametrize("p,code", rc.FIELDS, ids=["gold", "p64m59", "p257"])
@pytest.mark.parametrize("s,m", [(1, 2), (3, 3), (6, 5)])
def test_sublinear_verifier_next_to_the_verifier(pkg, p, code, s, m):
    """both accept the honest run; both refuse one flipped witness word, at the same message.  Over 257 the combined matrix of
    (6, 5) has 2^9 entries, more than the field has words for its counts: refused"""
    rp = pkg.r1cs
    if p == 257 and (s, m) == (6, 5):
        with pytest.raises(ValueError):
            run_sublinear(pkg, p, code, s, m, 40, False)
        return
    assert run_both(pkg, p, code, s, m, 40 + s) == [True, True]
    bad = run_both(pkg, p, code, s, m, 40 + s, flip=True)
    assert all(type(e) is rp.RoundMismatch and (e.phase, e.round) == (1, 0) for e in bad), bad


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/spark_host_harness.cpp, built and run stand-alone: the gather item, the tuple item with both key forms, the
    padding / validation routine and the index-to-Montgomery step against naive 128-bit loops, both fields"""
    exe = tmp_path / "spark_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "spark_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "spark host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
