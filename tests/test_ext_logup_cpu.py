"""CPU-only: LogUp's fraction sums over K = F_p[X] / (X^2 - w).  The big-integer reference (tests/ext_logup_ref.py) against its own
identities and, with alpha and beta in the base field and every drawn c1 = 0, against the base-field reference of
tests/logup_ref.py; the package's host verifiers (ext_logup.Verifier, LookupVerifier over ligero_pcs.ExtVerifier) against reference
provers - honest runs accepted, every tampered word refused with its own error; and the per-element code of
kernels/ext_fraction.hpp, compiled for the host and run stand-alone (tests/cpp/ext_fr_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import expander_ref
import ext_logup_ref as ref
import ext_ref as xref
import ligero_ref as lref
import logup_ref as bref
from conftest import ROOT, load_package
from test_ext_gp_cpu import AllColumns, canon, mont
from wide_words import WIDE, wid

PKG = load_package()
XL = PKG.ext_logup                        # (the module under test: without it nothing here can run)

GOLD = lref.GOLD
P64 = 2**64 - 59
MODULI = WIDE + [GOLD, 257]
SIZES = list(range(1, 7))
FORMS = [False, True]                     # the numerator: a table, all ones


def mid(p):
    return "gold" if p == GOLD else wid(p)


def word(p, rng):
    return rng.choice([0, 1, p - 1] + [rng.randrange(p)] * 3)


def elem(p, rng):
    return (word(p, rng), word(p, rng))


def case(p, n, ones, seed):
    """(pt, t, alpha, beta): alpha nonzero, components and entries from the edge words and random ones; pt None for all ones"""
    rng = random.Random(1000 * n + 10 * seed + ones)
    t = [word(p, rng) for _ in range(1 << n)]
    pt = None if ones else [word(p, rng) for _ in range(1 << n)]
    alpha = elem(p, rng)
    while alpha == (0, 0):
        alpha = elem(p, rng)
    return pt, t, alpha, elem(p, rng)


@pytest.mark.parametrize("ones", FORMS, ids=["table", "ones"])
@pytest.mark.parametrize("p", MODULI, ids=mid)
@pytest.mark.parametrize("n", SIZES)
def test_reference_round_and_final_identities(p, n, ones):
    w = xref.nonresidue(p)
    pt, t, alpha, beta = case(p, n, ones, 0)
    rng = random.Random(n)
    proof = ref.prove(pt, t, alpha, beta, p, w, lambda k, j, msg: elem(p, rng))
    top_p, top_q = ref.leaves(pt, t, alpha, beta, p, w)
    P, Q = ref.tree(top_p, top_q, p, w)
    assert proof["root"] == (P[0][0], Q[0][0])
    # P / Q = sum_i p_i / q_i, wherever no denominator is zero
    if all(q != (0, 0) for q in top_q):
        total = (0, 0)
        for num, den in zip(top_p, top_q):
            total = xref.kadd(total, xref.kmul(num, xref.kinv(den, p, w), p, w), p)
        assert xref.kmul(total, Q[0][0], p, w) == P[0][0]
    assert len(proof["challenges"]) == ref.n_challenges(n) and len(proof["point"]) == n
    kadd, kmul, ksub = xref.kadd, xref.kmul, xref.ksub
    z, (a, b), at, lam = [], proof["root"], 0, (0, 0)
    for k in range(n):
        if k >= 1:
            lam = proof["challenges"][at]
            assert lam == proof["lambdas"][k]
            at += 1
        rs = proof["challenges"][at:at + k]
        rho = proof["challenges"][at + k]
        at += k + 1
        claim = kadd(a, kmul(lam, b, p, w), p)
        assert len(proof["rounds"][k]) == k
        for msg, r in zip(proof["rounds"][k], rs):
            assert kadd(msg[0], msg[1], p) == claim                                       # the round identity
            assert ref.cubic_at(msg, (2, 0), p, w) == msg[2] and ref.cubic_at(msg, (3, 0), p, w) == msg[3]
            claim = ref.cubic_at(msg, r, p, w)
        pl, pr, ql, qr = proof["finals"][k]
        num, den = kadd(kmul(pl, qr, p, w), kmul(pr, ql, p, w), p), kmul(ql, qr, p, w)
        if k == 0:
            assert (num, den) == (a, b)
        else:
            assert kmul(ref.eq_point(z, rs, p, w), kadd(num, kmul(lam, den, p, w), p), p, w) == claim   # the final identity
        a, b = kadd(pl, kmul(rho, ksub(pr, pl, p), p, w), p), kadd(ql, kmul(rho, ksub(qr, ql, p), p, w), p)
        z = rs + [rho]
        # the claims handed on are the extensions of layer k + 1 at z_(k+1)
        assert ref.kmle(P[k + 1], z, p, w) == a and ref.kmle(Q[k + 1], z, p, w) == b
    assert at == len(proof["challenges"]) and z == proof["point"] and (a, b) == proof["claims"]
    # b_n = beta + alpha t~(z_n), a_n = p~(z_n) or 1
    assert b == kadd(beta, kmul(alpha, xref.mle_eval(t, z, p, w), p, w), p)
    assert a == (xref.mle_eval(pt, z, p, w) if pt is not None else (1, 0))
    assert ref.verify(n, p, w, proof, lambda k, j, msg, it=iter(proof["challenges"]): next(it), ones=ones) == (z, a, b)


@pytest.mark.parametrize("ones", FORMS, ids=["table", "ones"])
@pytest.mark.parametrize("p", MODULI, ids=mid)
@pytest.mark.parametrize("n", SIZES)
def test_reference_in_the_base_field_limit_is_the_base_field_argument(p, n, ones):
    """beta = (beta0, 0), alpha = (alpha0, 0), every drawn c1 = 0: the c0 words are logup_ref's transcript over q = beta0 + alpha0 t,
    every c1 word is 0"""
    w = xref.nonresidue(p)
    pt, t, _, _ = case(p, n, ones, 1)
    rng = random.Random(3 * n)
    alpha0, beta0 = rng.randrange(1, p), word(p, rng)
    ch = [word(p, rng) for _ in range(ref.n_challenges(n))]
    got = ref.prove(pt, t, (alpha0, 0), (beta0, 0), p, w, lambda k, j, msg, it=iter(ch): (next(it), 0))
    want = bref.prove(pt, [(beta0 + alpha0 * x) % p for x in t], p, lambda k, j, msg, it=iter(ch): next(it))
    flat = [got["root"], got["claims"], got["point"], got["challenges"]] + got["finals"] + [msg for layer in got["rounds"] for msg in layer]
    assert all(e[1] == 0 for group in flat for e in group)
    assert tuple(e[0] for e in got["root"]) == want["root"] and tuple(e[0] for e in got["claims"]) == want["claims"]
    assert [[[h[0] for h in msg] for msg in layer] for layer in got["rounds"]] == want["rounds"]
    assert [tuple(e[0] for e in fin) for fin in got["finals"]] == want["finals"]
    assert [z[0] for z in got["point"]] == want["point"] and [c[0] for c in got["challenges"]] == want["challenges"]


# ---- the package's host Verifier over the reference prover ------------------------------------------------------------------------

def mont_proof(F, proof):
    m = lambda e: mont(F, e)   # noqa: E731
    return XL.Proof(tuple(m(e) for e in proof["root"]), [[[m(h) for h in msg] for msg in layer] for layer in proof["rounds"]],
                    [tuple(m(e) for e in fin) for fin in proof["finals"]], [m(z) for z in proof["point"]], tuple(m(e) for e in proof["claims"]),
                    [m(c) for c in proof["challenges"]])


@pytest.mark.parametrize("ones", FORMS, ids=["table", "ones"])
@pytest.mark.parametrize("p", MODULI, ids=mid)
@pytest.mark.parametrize("n", SIZES)
def test_host_verifier_accepts_the_reference_prover(p, n, ones):
    """interactively (the verifier draws, message by message) and over the recorded proof"""
    F = PKG.Field(p)
    w = xref.nonresidue(p)
    pt, t, alpha, beta = case(p, n, ones, 2)
    layers = ref.tree(*ref.leaves(pt, t, alpha, beta, p, w), p, w)
    V = XL.Verifier(F, F.from_int(w), n, ones=ones)
    draw = V.challenger(random.Random(5), (mont(F, layers[0][0][0]), mont(F, layers[1][0][0])))
    proof = ref.prove(pt, t, alpha, beta, p, w, lambda k, j, msg: canon(F, draw(k, j, [mont(F, m) for m in msg])), layers=layers)
    point, a, b = V.result()
    assert (point, a, b) == ([mont(F, z) for z in proof["point"]], mont(F, proof["claims"][0]), mont(F, proof["claims"][1]))
    tv = mont(F, xref.mle_eval(t, proof["point"], p, w))
    pv = None if ones else mont(F, xref.mle_eval(pt, proof["point"], p, w))
    assert V.check_input(pv, tv, mont(F, alpha), mont(F, beta)) is True
    mp = mont_proof(F, proof)
    assert XL.Verifier(F, F.from_int(w), n, ones=ones).verify(mp, mp.challenges) == (point, a, b)


@pytest.mark.parametrize("p", MODULI, ids=mid)
def test_host_verifier_refuses_every_changed_word(p):
    """n = 4: each word of each round, of each final and of each input value.  The challenges' components are random words >= 4: the
    cubic's Lagrange weights at such a point are all nonzero, so a changed H(2) or H(3) always changes the claim handed on"""
    F = PKG.Field(p)
    w = xref.nonresidue(p)
    n = 4
    rng = random.Random(p % 1000 + 9)
    t = [rng.randrange(1, p) for _ in range(1 << n)]
    pt = [rng.randrange(1, p) for _ in range(1 << n)]
    alpha, beta = (rng.randrange(1, p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))
    ch = [(rng.randrange(4, p), rng.randrange(4, p)) for _ in range(ref.n_challenges(n))]
    proof = ref.prove(pt, t, alpha, beta, p, w, lambda k, j, msg, it=iter(ch): next(it))
    good = mont_proof(F, proof)
    wm = F.from_int(w)
    assert XL.Verifier(F, wm, n).verify(good, good.challenges) == (good.point, good.claims[0], good.claims[1])

    def bump(e, c):
        return (F.add(e[0], F.one), e[1]) if c == 0 else (e[0], F.add(e[1], F.one))
    for k in range(n):
        for j in range(k):
            for word_at in range(8):
                rounds = [[list(msg) for msg in layer] for layer in good.rounds]
                rounds[k][j][word_at // 2] = bump(rounds[k][j][word_at // 2], word_at % 2)
                bad = good._replace(rounds=rounds)
                # H(0), H(1) break the round's own sum; H(2), H(3) the claim it hands on: the next round, or the layer's finals
                if word_at < 4 or j + 1 < k:
                    with pytest.raises(XL.RoundMismatch) as ei:
                        XL.Verifier(F, wm, n).verify(bad, good.challenges)
                    assert (ei.value.layer, ei.value.round) == (k, j if word_at < 4 else j + 1)
                else:
                    with pytest.raises(XL.FinalMismatch) as ei:
                        XL.Verifier(F, wm, n).verify(bad, good.challenges)
                    assert ei.value.layer == k
        for word_at in range(8):
            finals = [list(f) for f in good.finals]
            finals[k][word_at // 2] = bump(finals[k][word_at // 2], word_at % 2)
            bad = good._replace(finals=[tuple(f) for f in finals])
            with pytest.raises(XL.RootMismatch if k == 0 else XL.FinalMismatch):
                XL.Verifier(F, wm, n).verify(bad, good.challenges)
    V = XL.Verifier(F, wm, n)
    V.verify(good, good.challenges)
    tv, pv = mont(F, xref.mle_eval(t, proof["point"], p, w)), mont(F, xref.mle_eval(pt, proof["point"], p, w))
    assert V.check_input(pv, tv, mont(F, alpha), mont(F, beta)) is True
    for c in range(2):
        with pytest.raises(XL.InputMismatch) as ei:
            V.check_input(bump(pv, c), tv, mont(F, alpha), mont(F, beta))
        assert ei.value.which == "p"
        with pytest.raises(XL.InputMismatch) as ei:
            V.check_input(pv, bump(tv, c), mont(F, alpha), mont(F, beta))
        assert ei.value.which != "p"
    with pytest.raises(XL.Error):
        V.check_input(None, tv, mont(F, alpha), mont(F, beta))
    # a numerator that is not all ones under ones=True
    with pytest.raises(XL.NumeratorMismatch):
        XL.Verifier(F, wm, n, ones=True).verify(good, good.challenges)
    # out of order, and the constructor's refusals
    V = XL.Verifier(F, wm, n)
    with pytest.raises(XL.Error):
        V.lam(1, random.Random(0))                          # before begin
    V.begin(*good.root)
    with pytest.raises(XL.Error):
        V.lam(1, random.Random(0))                          # layer 0 has no lambda
    with pytest.raises(XL.Error):
        V.round(1, 0, [(0, 0)] * 4, random.Random(0))
    with pytest.raises(XL.Error):
        V.result()
    with pytest.raises(ValueError):
        XL.Verifier(F, F.from_int(4), n)                    # a square
    with pytest.raises(ValueError):
        XL.Verifier(F, wm, 0)
    with pytest.raises(ValueError):
        XL.Verifier(PKG.Field(3), 2, 2)


# ---- the lookup over reference commitments ----------------------------------------------------------------------------------------

def lookup_exchange(p, code, table, committed_w, committed_mult, proved_w, proved_mult, seed):
    """the exchange of ext_logup.prove_lookup_ext with reference provers: the commitments are to committed_w and committed_mult
    (tests/ligero_ref.py or tests/expander_ref.py), the fraction sums run over proved_w and proved_mult (the same tables for an
    honest prover); the package's LookupVerifier over two ligero_pcs.ExtVerifier checks every message"""
    LP, F = PKG.ligero_pcs, PKG.Field(p)
    w = xref.nonresidue(p)
    wm = F.from_int(w)
    provers, verifiers, cs = [], [], []
    for committed in (committed_w, committed_mult):
        nv = len(committed).bit_length() - 1
        c = (nv + 1) // 2
        prover = expander_ref.RefProver(committed, c, p) if code == "expander" else lref.RefProver(committed, c, 1, p)
        provers.append(prover)
        cs.append(c)
        verifiers.append(LP.ExtVerifier(F, nv, c, 1, prover.root(), 1 << (c + 1), code=code, w=wm))
    rng = AllColumns(seed)
    V = XL.LookupVerifier(F, wm, verifiers[0], verifiers[1], lambda point: mont(F, ref.kmle([(x, 0) for x in table], [canon(F, z) for z in point], p, w)))
    alpha = canon(F, V.draw_alpha(rng))
    minus_one = (p - 1, 0)
    sides = ((None, proved_w), (proved_mult, table))
    trees = [ref.tree(*ref.leaves(num, den, minus_one, alpha, p, w), p, w) for num, den in sides]
    V.receive_roots(*[(mont(F, P[0][0]), mont(F, Q[0][0])) for P, Q in trees])
    for which, committed in enumerate((committed_w, committed_mult)):
        draw = V.frac[which].challenger(rng)
        ref.prove(sides[which][0], sides[which][1], minus_one, alpha, p, w, lambda k, j, msg: canon(F, draw(k, j, [mont(F, m) for m in msg])),
                  layers=trees[which])
        mpoint, _ = V.opening(which)
        point = [canon(F, z) for z in mpoint]
        # one opening of the commitment at the point of K^n, as tests/test_ext_cpu.py's open_ext forms it
        pv, c = verifiers[which], cs[which]
        g = lref.canon(p, pv.draw_gamma(rng))
        eq0, eq1 = zip(*xref.eq_weights(point[c:], p, w))
        pv.receive(lref.mont(p, lref.combine(committed, c, g, p)), lref.mont(p, lref.combine(committed, c, list(eq0), p)),
                   lref.mont(p, lref.combine(committed, c, list(eq1), p)))
        cols = provers[which].open_columns(pv.draw_columns(rng))
        opened = pv.verify(mpoint, [(j, lref.mont(p, col), LP.ColumnPath(j, path, F)) for j, col, path in cols])
        assert canon(F, opened) == xref.mle_eval(committed, point, p, w)
        V.finish(which, opened)
    return True


@pytest.mark.parametrize("p,code,n,m", [(GOLD, "rs", 4, 3), (GOLD, "rs", 5, 4), (P64, "expander", 4, 3), (P64, "expander", 3, 4)],
                         ids=["gold-4-3", "gold-5-4", "p64m59-expander-4-3", "p64m59-expander-3-4"])
def test_lookup_exchange_over_reference_commitments(p, code, n, m):
    rng = random.Random(10 * n + m)
    table = [word(p, rng) for _ in range(1 << m)]
    table = [x if table.index(x) == j else (x + 7 * j + 3) % p for j, x in enumerate(table)]   # (distinct enough: duplicates only split counts)
    idx = [rng.randrange(1 << m) for _ in range(1 << n)]
    wit = [table[j] for j in idx]
    mult, bad = bref.multiplicities(wit, table, idx)
    assert bad == 0 and sum(mult) == 1 << n
    assert lookup_exchange(p, code, table, wit, mult, wit, mult, 31) is True
    # a witness entry outside the table: it is not counted, and the two sums differ
    outside = next(x for x in range(2, p) if x not in table)
    wit2 = list(wit)
    wit2[3] = outside
    mult2, bad2 = bref.multiplicities(wit2, table, idx)
    assert bad2 == 1
    with pytest.raises(XL.LookupMismatch):
        lookup_exchange(p, code, table, wit2, mult2, wit2, mult2, 31)
    # a wrong multiplicity
    mult3 = list(mult)
    mult3[2] = (mult3[2] + 1) % p
    with pytest.raises(XL.LookupMismatch):
        lookup_exchange(p, code, table, wit, mult3, wit, mult3, 31)
    # a word changed after the commitment: the sums agree (the prover adds what it holds now), the opening does not
    wit4, idx4 = list(wit), list(idx)
    idx4[5] = (idx4[5] + 1) % (1 << m)
    wit4[5] = table[idx4[5]]
    if wit4 != wit:
        mult4, _ = bref.multiplicities(wit4, table, idx4)
        with pytest.raises(XL.InputMismatch) as ei:
            lookup_exchange(p, code, table, wit, mult4, wit4, mult4, 31)
        assert ei.value.which == "w"
        with pytest.raises(XL.InputMismatch) as ei:
            lookup_exchange(p, code, table, wit4, mult, wit4, mult4, 31)
        assert ei.value.which == "mult"


def test_lookup_verifier_refusals_and_the_range_table():
    LP, F = PKG.ligero_pcs, PKG.Field(GOLD)
    wm = F.from_int(7)
    ext = [LP.ExtVerifier(F, 4, 2, 1, b"\0" * 32, 4, w=wm) for _ in range(2)]
    V = XL.LookupVerifier(F, wm, ext[0], ext[1], None)
    with pytest.raises(XL.Error):
        V.receive_roots(((1, 0), (1, 0)), ((1, 0), (1, 0)))             # before alpha
    V.draw_alpha(random.Random(1))
    for roots in ((((1, 0), (0, 0)), ((1, 0), (1, 0))), (((1, 0), (1, 0)), ((1, 0), (0, 0))), (((1, 0), (1, 1)), ((1, 0), (1, 0)))):
        with pytest.raises(XL.LookupMismatch):
            V.receive_roots(*roots)                                      # a zero denominator, unequal sums
    with pytest.raises(ValueError):
        XL.LookupVerifier(F, wm, ext[0], LP.Verifier(F, 4, 2, 1, b"\0" * 32, 4), None)
    with pytest.raises(ValueError):
        XL.LookupVerifier(F, F.from_int(11), ext[0], ext[1], None)      # another w
    F257 = PKG.Field(257)
    small = [LP.ExtVerifier(F257, 9, 4, 1, b"\0" * 32, 4, code="expander", w=F257.from_int(3)) for _ in range(2)]
    with pytest.raises(ValueError):
        XL.LookupVerifier(F257, F257.from_int(3), small[0], small[1], None)   # p <= 2^max(n, m)
    # prove_lookup_ext refuses such a modulus before it touches the commitment
    import types
    fake = types.SimpleNamespace(ctx=types.SimpleNamespace(field=F257), num_vars=9)
    with pytest.raises(ValueError):
        XL.prove_lookup_ext(fake, None, small[0], None, types.SimpleNamespace(num_vars=lambda: 4), [], random.Random(0), F257.from_int(3))
    # the range table's extension in K is sum_j 2^j z_j, which is its extension by the definition
    p, w, mm = GOLD, 7, 5
    rng = random.Random(4)
    point = [elem(p, rng) for _ in range(mm)]
    K = PKG.ext_field.QuadExt(F, wm)
    want = xref.mle_eval(list(range(1 << mm)), point, p, w)
    assert ref.range_eval(point, p) == want
    assert canon(F, XL.range_table_eval(K, [mont(F, z) for z in point])) == want


def test_constants_and_bindings_match_the_headers():
    header = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "ext_fraction.hpp")).read()
    fr_text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "fraction.hpp")).read()
    for value, name, label in ((42, "SC_KIND_EXT_FRACTION_TREE", "ext_fraction_tree"), (43, "SC_KIND_EXT_FRACTION_PASS", "ext_fraction_pass")):
        assert "#define %s %d " % (name, value) in header and PKG._lib.KIND_NAMES[value] == label
    assert "#define SC_ABI_VERSION 6" in header and PKG._lib.ABI_VERSION == 6
    assert "constexpr int kExtFrTailLog = kFrTailLog - 1;" in text and "static_assert(kExtFrTailLog == 10 &&" in text
    assert XL.TAIL_LOG == int(re.search(r"constexpr int kFrTailLog = (\d+);", fr_text).group(1)) - 1 == 10
    assert XL.MAX_LOG == int(re.search(r"constexpr int kFrMaxLog = (\d+);", fr_text).group(1))
    assert re.search(r"typedef void \(\*sc_draw_frac_ext_fn\)\(void\* user, size_t layer, size_t round, const uint64_t\* msg, uint64_t out\[2\]\);", header)
    for name in ("sc_frac_create_ext", "sc_frac_destroy_ext", "sc_frac_root_ext", "sc_frac_layer_ext", "sc_frac_prove_ext"):
        assert name in PKG._lib.SIGNATURES
    assert XL.n_challenges(5) == ref.n_challenges(5) == bref.n_challenges(5)


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/ext_fr_host_harness.cpp, built and run stand-alone: the tree item at LV = 1, 2, 3 in its three forms, the two
    accumulate forms with their twelve-to-eight map, the leaf-in folds and the host rounds at n = 1 .. 6, against naive schoolbook
    128-bit loops on the edge words, Goldilocks in both field types and 2^64 - 59"""
    exe = tmp_path / "ext_fr_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "ext_fr_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ext fr host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
