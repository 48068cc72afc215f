"""CPU-only: the grand product argument over K = F_p[X] / (X^2 - w).  The big-integer reference (tests/ext_gp_ref.py) against its own
identities and, with alpha = 1, beta = 0 and every drawn c1 = 0, against the base-field reference of tests/grand_product_ref.py; the
package's host verifiers (ext_grand_product.Verifier, PermutationVerifier over ligero_pcs.ExtVerifier) against reference provers -
honest runs accepted, every tampered word refused with its own error; and the per-element code of kernels/ext_grand_product.hpp,
compiled for the host and run stand-alone (tests/cpp/ext_gp_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import expander_ref
import ext_gp_ref as ref
import ext_ref as xref
import grand_product_ref as bref
import ligero_ref as lref
from conftest import ROOT, load_package
from wide_words import WIDE, wid

PKG = load_package()
XG = PKG.ext_grand_product                # (the module under test: without it nothing here can run)

GOLD = lref.GOLD
P64 = 2**64 - 59
MODULI = WIDE + [GOLD, 257]
SIZES = list(range(1, 7))


def mid(p):
    return "gold" if p == GOLD else wid(p)


def word(p, rng):
    return rng.choice([0, 1, p - 1] + [rng.randrange(p)] * 3)


def elem(p, rng):
    return (word(p, rng), word(p, rng))


def table_of(p, n, seed):
    rng = random.Random(1000 * n + seed)
    return [word(p, rng) for _ in range(1 << n)]


def case(p, n, seed):
    """(t, alpha, beta): alpha nonzero, components from the edge words and random ones"""
    rng = random.Random(77 * n + seed)
    alpha = elem(p, rng)
    while alpha == (0, 0):
        alpha = elem(p, rng)
    return table_of(p, n, seed), alpha, elem(p, rng)


@pytest.mark.parametrize("p", MODULI, ids=mid)
@pytest.mark.parametrize("n", SIZES)
def test_reference_round_and_final_identities(p, n):
    w = xref.nonresidue(p)
    t, alpha, beta = case(p, n, 0)
    rng = random.Random(n)
    proof = ref.prove(t, alpha, beta, p, w, lambda k, j, msg: elem(p, rng))
    V = ref.tree(ref.leaves(t, alpha, beta, p, w), p, w)
    # the product by its definition
    prod = (1, 0)
    for x in t:
        prod = xref.kmul(prod, xref.kadd(beta, (alpha[0] * x % p, alpha[1] * x % p), p), p, w)
    assert proof["product"] == prod == V[0][0]
    assert len(proof["challenges"]) == ref.n_challenges(n) and len(proof["point"]) == n
    z, claim, at = [], proof["product"], 0
    for k in range(n):
        rs = proof["challenges"][at:at + k]
        rho = proof["challenges"][at + k]
        at += k + 1
        assert len(proof["rounds"][k]) == k
        for msg, r in zip(proof["rounds"][k], rs):
            assert xref.kadd(msg[0], msg[1], p) == claim                                  # the round identity
            assert ref.cubic_at(msg, (2, 0), p, w) == msg[2] and ref.cubic_at(msg, (3, 0), p, w) == msg[3]
            claim = ref.cubic_at(msg, r, p, w)
        l, r2 = proof["finals"][k]
        assert xref.kmul(ref.eq_point(z, rs, p, w), xref.kmul(l, r2, p, w), p, w) == claim  # the final identity
        claim = xref.kadd(l, xref.kmul(rho, xref.ksub(r2, l, p), p, w), p)
        z = rs + [rho]
        # the claim handed on is V_(k+1)~(z_(k+1))
        eq = xref.eq_weights(z, p, w)
        value = (0, 0)
        for e, v in zip(eq, V[k + 1]):
            value = xref.kadd(value, xref.kmul(e, v, p, w), p)
        assert value == claim
    assert z == proof["point"] and claim == proof["claim"]
    # c_n = beta + alpha t~(z_n)
    assert claim == xref.kadd(beta, xref.kmul(alpha, xref.mle_eval(t, z, p, w), p, w), p)
    assert ref.verify(n, p, w, proof, lambda k, j, msg, it=iter(proof["challenges"]): next(it)) == (z, claim)


@pytest.mark.parametrize("p", MODULI, ids=mid)
@pytest.mark.parametrize("n", SIZES)
def test_reference_in_the_base_field_limit_is_the_base_field_argument(p, n):
    """alpha = (1, 0), beta = 0, every drawn c1 = 0: the c0 words are grand_product_ref's transcript, every c1 word is 0"""
    w = xref.nonresidue(p)
    t = table_of(p, n, 1)
    rng = random.Random(3 * n)
    ch = [word(p, rng) for _ in range(ref.n_challenges(n))]
    got = ref.prove(t, (1, 0), (0, 0), p, w, lambda k, j, msg, it=iter(ch): (next(it), 0))
    want = bref.prove(t, p, lambda k, j, msg, it=iter(ch): next(it))
    assert got["product"] == (want["product"], 0) and got["claim"] == (want["claim"], 0)
    assert [[[h[0] for h in msg] for msg in layer] for layer in got["rounds"]] == want["rounds"]
    assert all(h[1] == 0 for layer in got["rounds"] for msg in layer for h in msg)
    assert [(l[0], r[0]) for l, r in got["finals"]] == want["finals"] and all(l[1] == 0 and r[1] == 0 for l, r in got["finals"])
    assert [z[0] for z in got["point"]] == want["point"] and all(z[1] == 0 for z in got["point"])
    assert [c[0] for c in got["challenges"]] == want["challenges"]


# ---- the package's host Verifier over the reference prover ------------------------------------------------------------------------

def mont(F, e):
    return (F.from_int(e[0]), F.from_int(e[1]))


def canon(F, e):
    return (F.to_int(e[0]), F.to_int(e[1]))


def mont_proof(F, proof):
    m = lambda e: mont(F, e)   # noqa: E731
    return XG.Proof(m(proof["product"]), [[[m(h) for h in msg] for msg in layer] for layer in proof["rounds"]],
                    [(m(l), m(r)) for l, r in proof["finals"]], [m(z) for z in proof["point"]], m(proof["claim"]), [m(c) for c in proof["challenges"]])


@pytest.mark.parametrize("p", MODULI, ids=mid)
@pytest.mark.parametrize("n", SIZES)
def test_host_verifier_accepts_the_reference_prover(p, n):
    """interactively (the verifier draws, message by message) and over the recorded proof"""
    F = PKG.Field(p)
    w = xref.nonresidue(p)
    t, alpha, beta = case(p, n, 2)
    V = XG.Verifier(F, F.from_int(w), n)
    draw = V.challenger(random.Random(5), mont(F, ref.tree(ref.leaves(t, alpha, beta, p, w), p, w)[0][0]))
    proof = ref.prove(t, alpha, beta, p, w, lambda k, j, msg: canon(F, draw(k, j, [mont(F, m) for m in msg])))
    point, claim = V.result()
    assert (point, claim) == ([mont(F, z) for z in proof["point"]], mont(F, proof["claim"]))
    value = mont(F, xref.mle_eval(t, proof["point"], p, w))
    assert V.check_input(value, mont(F, alpha), mont(F, beta)) is True
    mp = mont_proof(F, proof)
    assert XG.Verifier(F, F.from_int(w), n).verify(mp, mp.challenges) == (point, claim)


def tamper_challenges(p, n, seed):
    """components that are random words >= 4: the cubic's Lagrange weights at such a point are all nonzero, so a changed H(2) or H(3)
    always changes the claim handed on"""
    rng = random.Random(seed)
    return [(rng.randrange(4, p), rng.randrange(4, p)) for _ in range(ref.n_challenges(n))]


@pytest.mark.parametrize("p", MODULI, ids=mid)
def test_host_verifier_refuses_every_changed_word(p):
    F = PKG.Field(p)
    w = xref.nonresidue(p)
    n = 4
    rng = random.Random(p % 1000 + 9)
    t = [rng.randrange(1, p) for _ in range(1 << n)]
    alpha, beta = (rng.randrange(1, p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))
    ch = tamper_challenges(p, n, 21)
    proof = ref.prove(t, alpha, beta, p, w, lambda k, j, msg, it=iter(ch): next(it))
    good = mont_proof(F, proof)
    wm = F.from_int(w)
    assert XG.Verifier(F, wm, n).verify(good, good.challenges) == (good.point, good.claim)

    def bump(e, c):
        return (F.add(e[0], F.one), e[1]) if c == 0 else (e[0], F.add(e[1], F.one))
    for k in range(n):
        for j in range(k):
            for word_at in range(8):
                rounds = [[list(msg) for msg in layer] for layer in good.rounds]
                rounds[k][j][word_at // 2] = bump(rounds[k][j][word_at // 2], word_at % 2)
                bad = good._replace(rounds=rounds)
                # H(0), H(1) break the round's own sum; H(2), H(3) the claim it hands on: the next round, or the layer's finals
                if word_at < 4:
                    with pytest.raises(XG.RoundMismatch) as ei:
                        XG.Verifier(F, wm, n).verify(bad, good.challenges)
                    assert (ei.value.layer, ei.value.round) == (k, j)
                elif j + 1 < k:
                    with pytest.raises(XG.RoundMismatch) as ei:
                        XG.Verifier(F, wm, n).verify(bad, good.challenges)
                    assert (ei.value.layer, ei.value.round) == (k, j + 1)
                else:
                    with pytest.raises(XG.FinalMismatch) as ei:
                        XG.Verifier(F, wm, n).verify(bad, good.challenges)
                    assert ei.value.layer == k
        for word_at in range(4):
            finals = [list(f) for f in good.finals]
            finals[k][word_at // 2] = bump(finals[k][word_at // 2], word_at % 2)
            bad = good._replace(finals=[tuple(f) for f in finals])
            with pytest.raises(XG.ProductMismatch if k == 0 else XG.FinalMismatch):
                XG.Verifier(F, wm, n).verify(bad, good.challenges)
    V = XG.Verifier(F, wm, n)
    V.verify(good, good.challenges)
    value = mont(F, xref.mle_eval(t, proof["point"], p, w))
    assert V.check_input(value, mont(F, alpha), mont(F, beta)) is True
    for c in range(2):
        with pytest.raises(XG.InputMismatch):
            V.check_input(bump(value, c), mont(F, alpha), mont(F, beta))
    # out of order, and the constructor's refusals
    V = XG.Verifier(F, wm, n)
    with pytest.raises(XG.Error):
        V.round(1, 0, [(0, 0)] * 4, random.Random(0))      # before begin
    V.begin(good.product)
    with pytest.raises(XG.Error):
        V.round(1, 0, [(0, 0)] * 4, random.Random(0))      # layer 0 has no rounds
    with pytest.raises(XG.Error):
        V.result()
    with pytest.raises(ValueError):
        XG.Verifier(F, F.from_int(4), n)                   # a square
    with pytest.raises(ValueError):
        XG.Verifier(F, wm, 0)
    with pytest.raises(ValueError):
        XG.Verifier(PKG.Field(3), 2, 2)


# ---- the permutation check over reference commitments ---------------------------------------------------------------------------

class AllColumns(random.Random):
    """field words as random.Random gives them, column indices 0, 1, 2, .. in turn: with `queries` = the number of columns every
    column is opened, and whether a changed word is caught does not hang on the draw"""

    def __init__(self, seed):
        super().__init__(seed)
        self.turn = 0

    def randrange(self, start, stop=None, step=1):
        if stop is None and start <= 1 << 16:
            self.turn += 1
            return (self.turn - 1) % start
        return super().randrange(start, stop, step)


def permutation_exchange(p, code, committed_a, committed_b, proved_a, proved_b, seed):
    """the exchange of ext_grand_product.prove_permutation_ext with reference provers: the commitments are to committed_a and
    committed_b (tests/ligero_ref.py or tests/expander_ref.py), the grand products run over proved_a and proved_b (the same tables
    for an honest prover); the package's PermutationVerifier over two ligero_pcs.ExtVerifier checks every message"""
    LP, F = PKG.ligero_pcs, PKG.Field(p)
    w = xref.nonresidue(p)
    wm = F.from_int(w)
    n = len(committed_a).bit_length() - 1
    c = (n + 1) // 2
    L = 1 << (c + 1)
    provers, verifiers = [], []
    for table in (committed_a, committed_b):
        prover = expander_ref.RefProver(table, c, p) if code == "expander" else lref.RefProver(table, c, 1, p)
        provers.append(prover)
        verifiers.append(LP.ExtVerifier(F, n, c, 1, prover.root(), L, code=code, w=wm))
    rng = AllColumns(seed)
    V = XG.PermutationVerifier(F, wm, verifiers[0], verifiers[1])
    gamma = canon(F, V.draw_gamma(rng))
    minus_one = (p - 1, 0)
    trees = [ref.tree(ref.leaves(t, minus_one, gamma, p, w), p, w) for t in (proved_a, proved_b)]
    V.receive_products(mont(F, trees[0][0][0]), mont(F, trees[1][0][0]))
    for which, (committed, proved) in enumerate(((committed_a, proved_a), (committed_b, proved_b))):
        draw = V.gp[which].challenger(rng)
        ref.prove(proved, minus_one, gamma, p, w, lambda k, j, msg: canon(F, draw(k, j, [mont(F, m) for m in msg])), layers=trees[which])
        mpoint, _ = V.opening(which)
        point = [canon(F, z) for z in mpoint]
        # one opening of the commitment at the point of K^n, as tests/test_ext_cpu.py's open_ext forms it
        pv = verifiers[which]
        g = lref.canon(p, pv.draw_gamma(rng))
        eq0, eq1 = zip(*xref.eq_weights(point[c:], p, w))
        pv.receive(lref.mont(p, lref.combine(committed, c, g, p)), lref.mont(p, lref.combine(committed, c, list(eq0), p)),
                   lref.mont(p, lref.combine(committed, c, list(eq1), p)))
        cols = provers[which].open_columns(pv.draw_columns(rng))
        opened = pv.verify(mpoint, [(j, lref.mont(p, col), LP.ColumnPath(j, path, F)) for j, col, path in cols])
        assert canon(F, opened) == xref.mle_eval(committed, point, p, w)
        V.finish(which, opened)
    return True


@pytest.mark.parametrize("p,code,n", [(GOLD, "rs", 4), (GOLD, "rs", 5), (P64, "expander", 4), (P64, "expander", 3)],
                         ids=["gold-4", "gold-5", "p64m59-expander-4", "p64m59-expander-3"])
def test_permutation_exchange_over_reference_commitments(p, code, n):
    rng = random.Random(n)
    a = [word(p, rng) for _ in range(1 << n)]
    b = list(a)
    rng.shuffle(b)
    assert permutation_exchange(p, code, a, b, a, b, 31) is True
    # a changed entry: the products differ
    b2 = list(b)
    b2[3] = (b2[3] + 1) % p
    with pytest.raises(XG.PermutationMismatch):
        permutation_exchange(p, code, a, b2, a, b2, 31)
    # a word changed after the commitment: the products agree (b is a permutation of what the prover multiplies), the opening does not
    a2 = list(a)
    a2[5] = (a2[5] + 1) % p
    b3 = list(a2)
    rng.shuffle(b3)
    with pytest.raises(XG.InputMismatch):
        permutation_exchange(p, code, a, b3, a2, b3, 31)


def test_permutation_verifier_refusals():
    LP, F = PKG.ligero_pcs, PKG.Field(GOLD)
    wm = F.from_int(7)
    ext = [LP.ExtVerifier(F, 4, 2, 1, b"\0" * 32, 4, w=wm) for _ in range(2)]
    V = XG.PermutationVerifier(F, wm, ext[0], ext[1])
    with pytest.raises(XG.Error):
        V.receive_products((1, 0), (1, 0))                 # before gamma
    with pytest.raises(ValueError):
        XG.PermutationVerifier(F, wm, ext[0], LP.Verifier(F, 4, 2, 1, b"\0" * 32, 4))
    with pytest.raises(ValueError):
        XG.PermutationVerifier(F, wm, ext[0], LP.ExtVerifier(F, 5, 2, 1, b"\0" * 32, 4, w=wm))
    with pytest.raises(ValueError):
        XG.PermutationVerifier(F, F.from_int(11), ext[0], ext[1])      # another w


def test_constants_and_bindings_match_the_headers():
    header = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "ext_grand_product.hpp")).read()
    gp_text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "grand_product.hpp")).read()
    for value, name, label in ((39, "SC_KIND_EXT_PRODUCT_TREE", "ext_product_tree"), (40, "SC_KIND_EXT_PRODUCT_PASS", "ext_product_pass"),
                               (41, "SC_KIND_EXT_EQ_TABLE", "ext_eq_table")):
        assert "#define %s %d " % (name, value) in header and PKG._lib.KIND_NAMES[value] == label
    assert "constexpr int kExtGpTailLog = kGpTailLog - 1;" in text
    assert XG.TAIL_LOG == int(re.search(r"constexpr int kGpTailLog = (\d+);", gp_text).group(1)) - 1 == 11
    assert XG.MAX_LOG == int(re.search(r"constexpr int kGpMaxLog = (\d+);", gp_text).group(1))
    assert re.search(r"typedef void \(\*sc_draw_gp_ext_fn\)\(void\* user, size_t layer, size_t round, const uint64_t\* msg, uint64_t out\[2\]\);", header)
    for name in ("sc_gp_create_ext", "sc_gp_destroy_ext", "sc_gp_product_ext", "sc_gp_layer_ext", "sc_gp_prove_ext"):
        assert name in PKG._lib.SIGNATURES


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/ext_gp_host_harness.cpp, built and run stand-alone: the leaf map and its folded form, the tree item at LV = 1, 2, 3,
    the accumulate with its twelve-to-eight map, the eq table and the host rounds, against naive schoolbook 128-bit loops on the edge
    words, both field types"""
    exe = tmp_path / "ext_gp_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "ext_gp_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ext gp host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
