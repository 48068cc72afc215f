"""CPU-only: the quadratic extension (thaler-study_amd/ext_field.py) and its laws; the extension sumcheck reference (tests/ext_ref.py)
against its own identities and, with every drawn c1 = 0, against the base-field reference of tests/multiopen_ref.py; the package's
host verifiers (ext_sumcheck.Verifier, ligero_pcs.ExtVerifier) against reference provers - honest runs accepted, tampered messages
refused with their own errors; and the per-element code of kernels/ext_sumprod.hpp, compiled for the host and run stand-alone
(tests/cpp/ext_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import expander_ref
import ext_ref as ref
import ligero_ref as lref
import multiopen_ref as mref
from conftest import ROOT, load_package
from wide_words import WIDE, wid

PKG = load_package()
XF = PKG.ext_field                       # (the modules under test: without them nothing here can run)
XS = PKG.ext_sumcheck

GOLD = lref.GOLD
P64 = 2**64 - 59
MODULI = WIDE + [GOLD, 257]
SIZES = [(1, 1), (2, 2), (4, 3), (5, 8)]          # (n, T)


def mid(p):
    return "gold" if p == GOLD else wid(p)


def test_nonresidues():
    assert [XF.nonresidue(p) for p in (GOLD, P64, 2**61 - 1, 2**32 + 15, 257)] == [7, 2, 3, 3, 3]
    for p in MODULI:
        g = XF.nonresidue(p)
        assert g == ref.nonresidue(p) and pow(g, (p - 1) // 2, p) == p - 1
        assert all(pow(h, (p - 1) // 2, p) == 1 for h in range(2, g))
    F = PKG.Field(GOLD)
    with pytest.raises(ValueError):
        XF.QuadExt(F, F.from_int(4))                 # a square
    with pytest.raises(ValueError):
        XF.QuadExt(F, GOLD)                          # not a word below p
    assert XF.QuadExt(F).w == F.from_int(7)


@pytest.mark.parametrize("p", MODULI, ids=mid)
def test_quadext_laws(p):
    F = PKG.Field(p)
    K = XF.QuadExt(F)
    w = F.to_int(K.w)
    rng = random.Random(p)
    edge = [0, 1, p - 1]

    def elem():
        return (F.from_int(rng.choice(edge + [rng.randrange(p)] * 3)), F.from_int(rng.choice(edge + [rng.randrange(p)] * 3)))

    def canon(a):
        return (F.to_int(a[0]), F.to_int(a[1]))
    assert K.mul(K.x, K.x) == (K.w, 0)
    xinv = K.inv(K.x)
    assert K.mul(K.x, xinv) == K.one
    assert K.scale(K.mul(xinv, xinv), K.w) == K.one                        # w (X^-1)^2 = 1
    for _ in range(200):
        a, b, c = elem(), elem(), elem()
        # against the schoolbook product of the reference
        assert canon(K.mul(a, b)) == ref.kmul(canon(a), canon(b), p, w)
        assert canon(K.add(a, b)) == ref.kadd(canon(a), canon(b), p) and canon(K.sub(a, b)) == ref.ksub(canon(a), canon(b), p)
        assert K.mul(a, b) == K.mul(b, a) and K.mul(K.mul(a, b), c) == K.mul(a, K.mul(b, c))
        assert K.mul(a, K.add(b, c)) == K.add(K.mul(a, b), K.mul(a, c))
        assert K.mul(a, K.one) == a and K.add(a, K.neg(a)) == K.zero and K.sub(a, b) == K.add(a, K.neg(b))
        assert K.mul(K.from_base(a[0]), b) == K.scale(b, a[0])
        if a != K.zero:
            assert K.mul(a, K.inv(a)) == K.one and canon(K.inv(a)) == ref.kinv(canon(a), p, w)
    with pytest.raises(ZeroDivisionError):
        K.inv(K.zero)
    # eq weights: they sum to one, and a base table's extension at a point of K is (sum eq.c0 f, sum eq.c1 f)
    point = [elem() for _ in range(4)]
    eq = K.eq_weights(point)
    total = K.zero
    for e in eq:
        total = K.add(total, e)
    assert total == K.one and [canon(e) for e in eq] == ref.eq_weights([canon(z) for z in point], p, w)
    table = [rng.randrange(p) for _ in range(16)]
    value = K.zero
    for x, e in zip(table, eq):
        value = K.add(value, K.scale(e, F.from_int(x)))
    assert canon(value) == ref.mle_eval(table, [canon(z) for z in point], p, w)


def tables_of(p, n, T, seed):
    rng = random.Random(100 * n + T + seed)
    words = [0, 1, p - 1]
    return ([[rng.choice(words + [rng.randrange(p)] * 5) for _ in range(1 << n)] for _ in range(T)],
            [[rng.choice(words + [rng.randrange(p)] * 5) for _ in range(1 << n)] for _ in range(T)])


@pytest.mark.parametrize("p", [GOLD, P64, 2**32 + 15, 257], ids=mid)
@pytest.mark.parametrize("n,T", SIZES)
def test_reference_round_and_final_identities(p, n, T):
    w = ref.nonresidue(p)
    a, b = tables_of(p, n, T, 0)
    rng = random.Random(n)
    c1, rounds, z, fa, fb = ref.sumcheck(a, b, p, w, lambda j, msg: (rng.randrange(p), rng.randrange(p)))
    total = sum(x * y for ta, tb in zip(a, b) for x, y in zip(ta, tb)) % p
    assert c1 == (total, 0) and len(rounds) == len(z) == n
    assert all(m[1] == 0 for m in rounds[0])                  # round 0 is over base tables
    claim = c1
    for msg, r in zip(rounds, z):
        assert ref.kadd(msg[0], msg[1], p) == claim
        assert ref.quadratic_at(msg, (2, 0), p, w) == msg[2]
        claim = ref.quadratic_at(msg, r, p, w)
    assert fa == [ref.mle_eval(t, z, p, w) for t in a] and fb == [ref.mle_eval(t, z, p, w) for t in b]
    final = (0, 0)
    for x, y in zip(fa, fb):
        final = ref.kadd(final, ref.kmul(x, y, p, w), p)
    assert final == claim


@pytest.mark.parametrize("p", [GOLD, P64], ids=mid)
@pytest.mark.parametrize("n,T", SIZES)
def test_reference_with_base_challenges_is_the_base_field_sumcheck(p, n, T):
    w = ref.nonresidue(p)
    a, b = tables_of(p, n, T, 1)
    rs = [random.Random(n + j).randrange(p) for j in range(n)]
    c1, rounds, z, fa, fb = ref.sumcheck(a, b, p, w, lambda j, msg: (rs[j], 0))
    b_rounds, b_z, b_fa, b_fb = mref.sumcheck(a, b, p, lambda j, msg: rs[j])
    assert [[m[0] for m in msg] for msg in rounds] == b_rounds and all(m[1] == 0 for msg in rounds for m in msg)
    assert [r[0] for r in z] == b_z and [x[0] for x in fa] == b_fa and [x[0] for x in fb] == b_fb
    assert all(x[1] == 0 for x in fa + fb)


@pytest.mark.parametrize("p", [GOLD, P64, 257], ids=mid)
@pytest.mark.parametrize("n,T", SIZES)
def test_host_verifier_accepts_the_reference_prover(p, n, T):
    F = PKG.Field(p)
    w = ref.nonresidue(p)
    a, b = tables_of(p, n, T, 2)
    V = XS.Verifier(F, F.from_int(w), n)
    rng = random.Random(5)

    def mont(e):
        return (F.from_int(e[0]), F.from_int(e[1]))

    def draw(j, msg):
        if j == 0:
            V.start(mont(ref.kadd(msg[0], msg[1], p)))
        r = V.round(j, [mont(m) for m in msg], rng)
        return (F.to_int(r[0]), F.to_int(r[1]))
    c1, rounds, z, fa, fb = ref.sumcheck(a, b, p, w, draw)
    assert V.final([mont(x) for x in fa], [mont(x) for x in fb]) is True
    assert [mont(r) for r in z] == V.z


@pytest.mark.parametrize("p", [GOLD, P64], ids=mid)
def test_host_verifier_refuses_a_changed_round_value_and_final(p):
    F = PKG.Field(p)
    w = ref.nonresidue(p)
    n, T = 4, 3
    a, b = tables_of(p, n, T, 3)

    def mont(e):
        return (F.from_int(e[0]), F.from_int(e[1]))

    def run(tamper_round=None, tamper_word=None, tamper_final=False):
        V = XS.Verifier(F, F.from_int(w), n)
        rng = random.Random(6)

        def draw(j, msg):
            if j == 0:
                V.start(mont(ref.kadd(msg[0], msg[1], p)))
            msg = [list(m) for m in msg]
            if j == tamper_round:
                msg[tamper_word // 2][tamper_word % 2] = (msg[tamper_word // 2][tamper_word % 2] + 1) % p
            r = V.round(j, [mont(m) for m in msg], rng)
            return (F.to_int(r[0]), F.to_int(r[1]))
        _, _, _, fa, fb = ref.sumcheck(a, b, p, w, draw)
        fa = [mont(x) for x in fa]
        if tamper_final:
            fa[0] = (fa[0][0], F.add(fa[0][1], F.one))
        return V.final(fa, [mont(x) for x in fb])
    assert run() is True
    for j in range(n):
        for word in range(6):
            # H(0), H(1) break the round's own sum, H(2) the claim it hands on
            want = j if word < 4 else j + 1
            with pytest.raises(XS.RoundMismatch if want < n else XS.FinalMismatch) as ei:
                run(j, word)
            if want < n:
                assert ei.value.round == want
    with pytest.raises(XS.FinalMismatch):
        run(tamper_final=True)
    V = XS.Verifier(F, F.from_int(w), n)
    with pytest.raises(XS.Error):
        V.round(0, [(0, 0)] * 3, random.Random(0))         # before the claim
    with pytest.raises(ValueError):
        XS.Verifier(F, F.from_int(4), n)                   # a square
    with pytest.raises(ValueError):
        XS.Verifier(F, F.from_int(w), 0)


class AllColumns(random.Random):
    """field words as random.Random gives them, column indices 0, 1, 2, .. in turn: with `queries` = the number of columns every
    column is opened, and whether a tampered row is caught does not hang on the draw"""

    def __init__(self, seed):
        super().__init__(seed)
        self.turn = 0

    def randrange(self, start, stop=None, step=1):
        if stop is None and start <= 1 << 16:
            self.turn += 1
            return (self.turn - 1) % start
        return super().randrange(start, stop, step)


def open_ext(p, code, n, seed, tamper=None, all_columns=True):
    """a reference commitment opened at a point of K^n against the package's ExtVerifier; returns (value, expected value)"""
    LP, F = PKG.ligero_pcs, PKG.Field(p)
    w = ref.nonresidue(p)
    rng = random.Random(seed)
    table = [rng.choice([0, 1, p - 1] + [rng.randrange(p)] * 5) for _ in range(1 << n)]
    c = (n + 1) // 2
    prover = expander_ref.RefProver(table, c, p) if code == "expander" else lref.RefProver(table, c, 1, p)
    L = 1 << (c + 1)
    V = LP.ExtVerifier(F, n, c, 1, prover.root(), L if all_columns else 6, code=code, w=F.from_int(w))
    vrng = AllColumns(seed + 1) if all_columns else random.Random(seed + 1)
    point = [(rng.choice([0, 1, p - 1, rng.randrange(p)]), rng.choice([0, 1, p - 1, rng.randrange(p), rng.randrange(p)])) for _ in range(n)]
    gamma = lref.canon(p, V.draw_gamma(vrng))
    eq0, eq1 = zip(*ref.eq_weights(point[c:], p, w))
    msg = {"u_gamma": lref.combine(table, c, gamma, p), "u_z0": lref.combine(table, c, list(eq0), p), "u_z1": lref.combine(table, c, list(eq1), p)}
    if tamper:
        tamper("rows", msg)
    V.receive(lref.mont(p, msg["u_gamma"]), lref.mont(p, msg["u_z0"]), lref.mont(p, msg["u_z1"]))
    cols = [[j, list(col), list(path)] for j, col, path in prover.open_columns(V.draw_columns(vrng))]
    if tamper:
        tamper("open", cols)
    mpoint = [(F.from_int(z[0]), F.from_int(z[1])) for z in point]
    value = V.verify(mpoint, [(j, lref.mont(p, col), LP.ColumnPath(j, path, F)) for j, col, path in cols])
    return (F.to_int(value[0]), F.to_int(value[1])), ref.mle_eval(table, point, p, w)


@pytest.mark.parametrize("p,code", [(257, "rs"), (GOLD, "rs"), (P64, "expander")], ids=["p257", "gold", "p64m59"])
@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_ext_verifier_accepts_honest_openings(p, code, n):
    for all_columns in (True, False):
        value, want = open_ext(p, code, n, 11 * n, all_columns=all_columns)
        assert value == want


@pytest.mark.parametrize("p,code", [(GOLD, "rs"), (P64, "expander")], ids=["gold", "p64m59"])
@pytest.mark.parametrize("n", [2, 5])
def test_ext_verifier_refuses_every_single_tamper(p, code, n):
    """every column is opened: which error a tampered message earns does not depend on the columns drawn"""
    LP = PKG.ligero_pcs
    c = (n + 1) // 2

    def bump(tag_wanted, change):
        def tamper(tag, msg):
            if tag == tag_wanted:
                change(msg)
        return tamper

    def word(name, at):
        def change(msg):
            msg[name][at] = (msg[name][at] + 1) % p
        return change
    for at in (0, (1 << c) - 1):
        with pytest.raises(LP.EvalMismatch):
            open_ext(p, code, n, 13, bump("rows", word("u_z1", at)))
        with pytest.raises(LP.EvalMismatch):
            open_ext(p, code, n, 13, bump("rows", word("u_z0", at)))
        with pytest.raises(LP.ProximityMismatch):
            open_ext(p, code, n, 13, bump("rows", word("u_gamma", at)))

    def column_word(cols):
        cols[1][1][0] = (cols[1][1][0] + 1) % p

    def path_byte(cols):
        cols[0][2][0] = bytes([cols[0][2][0][0] ^ 1]) + cols[0][2][0][1:]
    with pytest.raises(LP.MerkleMismatch):
        open_ext(p, code, n, 13, bump("open", column_word))
    with pytest.raises(LP.MerkleMismatch):
        open_ext(p, code, n, 13, bump("open", path_byte))
    F = PKG.Field(p)
    V = LP.ExtVerifier(F, 4, 2, 1, b"\0" * 32, 4, code=code)
    with pytest.raises(LP.Error):
        V.receive([0] * 4, [0] * 4, [0] * 4)               # before draw_gamma
    V.draw_gamma(random.Random(0))
    with pytest.raises(LP.Error):
        V.receive([0] * 4, [0] * 4, [0] * 3)
    with pytest.raises(LP.Error):
        V.verify([(0, 0)] * 4, [])                         # before draw_columns


def test_constants_and_bindings_match_the_headers():
    header = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "multiopen.hpp")).read()
    assert "#define SC_KIND_SUMPROD_EXT_PASS 38 " in header
    assert PKG._lib.KIND_NAMES[38] == "sumprod_ext_pass"
    assert XS.MAX_TABLES == int(re.search(r"constexpr int kSumprodMaxPairs = (\d+);", text).group(1))
    assert re.search(r"typedef void \(\*sc_draw_ext_fn\)\(void\* user, size_t round, const uint64_t msg\[6\], uint64_t out\[2\]\);", header)
    for name in ("sc_sumprod_prove_ext", "sc_table_evaluate_ext"):
        assert name in PKG._lib.SIGNATURES


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/ext_host_harness.cpp, built and run stand-alone: the K-product, both folds, the accumulate with its nine-to-six
    map, and the host rounds, against naive schoolbook 128-bit loops on the edge words, both fields"""
    exe = tmp_path / "ext_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "ext_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ext host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
