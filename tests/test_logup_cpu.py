"""CPU-only: the LogUp reference (tests/logup_ref.py) against the dense definitions, the package's host Verifier and
LookupVerifier (thaler-study_amd/logup.py) against the reference prover - honest runs are accepted, every single tampered message
is refused with its own error - and the SC_HD and host-finish code of kernels/fraction.hpp, compiled for the host and run
stand-alone (tests/cpp/fr_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import logup_cases as cases
import logup_ref as ref
from conftest import ROOT

FIELDS = [257, cases.GOLD, cases.P64]


def table(p, n, seed, zero_at=None, nonzero=True):
    rng = random.Random(seed)
    edge = [e for e in (0, 1, p - 1, p - 2, (p - 1) // 2, 2**64 % p, (2**32 - 1) % p) if e or not nonzero]
    t = [rng.choice(edge) if rng.random() < 0.3 else rng.randrange(1 if nonzero else 0, p) for _ in range(1 << n)]
    if zero_at is not None:
        t[zero_at] = 0
    return t


def challenges(p, count, seed, low=0):
    """canonical challenges: 0, 1, p - 1 and random words mixed (low = 0), or random words >= low"""
    rng = random.Random(seed)
    if low:
        return [rng.randrange(low, p) for _ in range(count)]
    return [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(count)]


@pytest.mark.parametrize("ones", [False, True], ids=["general", "ones"])
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_reference_against_the_dense_definitions(p, n, ones):
    qt = table(p, n, 100 + n)                       # denominators: nonzero
    pt = None if ones else table(p, n, 200 + n, nonzero=False)
    P, Q = ref.tree(pt, qt, p)
    assert len(P) == len(Q) == n + 1 and Q[n] == qt and P[n] == (pt if pt is not None else [1] * (1 << n))
    assert [len(v) for v in P] == [len(v) for v in Q] == [1 << k for k in range(n + 1)]
    # the root: P / Q = sum_i p_i / q_i
    total = sum(a * pow(b, -1, p) for a, b in zip(P[n], qt)) % p
    assert P[0][0] * pow(Q[0][0], -1, p) % p == total
    rng = random.Random(n)
    for k in range(n):
        half = 1 << k
        PL, PR, QL, QR = P[k + 1][:half], P[k + 1][half:], Q[k + 1][:half], Q[k + 1][half:]
        z, lam = [rng.randrange(p) for _ in range(k)], rng.randrange(p)
        # the layer identity: p_k~(z) + lam q_k~(z) = sum_x eq(z, x) (PL QR + PR QL + lam QL QR)(x), the extensions by their definition
        eq = ref.eq_table(z, p)
        want = (ref.mle_eval(P[k], z, p) + lam * ref.mle_eval(Q[k], z, p)) % p
        assert want == sum(e * (pl * qr + pr * ql + lam * ql * qr) for e, pl, pr, ql, qr in zip(eq, PL, PR, QL, QR)) % p
        # eq by its definition
        for x in range(half):
            w = 1
            for j in range(k):
                w = w * (z[j] if (x >> j) & 1 else 1 - z[j]) % p
            assert eq[x] == w
        # the combining step: p_(k+1)~(r, rho) = pl + rho (pr - pl), and the same for q
        r, rho = [rng.randrange(p) for _ in range(k)], rng.randrange(p)
        for lo, hi, whole in ((PL, PR, P[k + 1]), (QL, QR, Q[k + 1])):
            l, h = ref.mle_eval(lo, r, p), ref.mle_eval(hi, r, p)
            assert ref.mle_eval(whole, r + [rho], p) == (l + rho * (h - l)) % p
    # the whole proof: the verifier accepts, and the last claims are the tables' extensions at the point
    ch = challenges(p, ref.n_challenges(n), 7 * n)
    it, it2 = iter(ch), iter(ch)
    proof = ref.prove(pt, qt, p, lambda k, j, msg: next(it))
    assert proof["challenges"] == ch and proof["root"] == (P[0][0], Q[0][0])
    point, a, b = ref.verify(n, p, proof, lambda k, j, msg: next(it2), ones=ones)
    assert (point, (a, b)) == (proof["point"], proof["claims"])
    assert ref.mle_eval(P[n], point, p) == a and ref.mle_eval(qt, point, p) == b
    if ones:
        assert a == 1 and all(f[:2] == (1, 1) for f in proof["finals"][n - 1:])
    for k in range(n):
        for msg in proof["rounds"][k]:
            assert len(msg) == 4 and ref.cubic_at(msg, 2, p) == msg[2] and ref.cubic_at(msg, 3, p) == msg[3]


@pytest.mark.parametrize("p", FIELDS)
def test_reference_with_a_zero_denominator(p):
    for at in (0, 16, 31):
        qt = table(p, 5, 3, zero_at=at)
        P, Q = ref.tree(None, qt, p)
        assert Q[0] == [0]
        ch = challenges(p, ref.n_challenges(5), at)
        it = iter(ch)
        proof = ref.prove(None, qt, p, lambda k, j, msg: next(it), layers=(P, Q))
        it = iter(ch)
        point, a, b = ref.verify(5, p, proof, lambda k, j, msg: next(it), ones=True)
        assert ref.mle_eval(qt, point, p) == b


@pytest.mark.parametrize("ones", [False, True], ids=["general", "ones"])
@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 5])
def test_host_verifier_accepts_the_reference_prover(pkg, p, n, ones):
    lu, F = pkg.logup, pkg.Field(p)
    qt = table(p, n, 11 * n)
    pt = None if ones else table(p, n, 13 * n, nonzero=False)
    ch = challenges(p, ref.n_challenges(n), n)
    proof = cases.ref_proof(pkg, pt, qt, p, ch)
    V = lu.Verifier(F, n, ones=ones)
    point, a, b = V.verify(proof, proof.challenges)
    assert point == proof.point and (a, b) == proof.claims
    at = [ref.canon(x, p) for x in point]
    q_value = ref.mont(ref.mle_eval(qt, at, p), p)
    assert V.check_input(q_value, None if ones else ref.mont(ref.mle_eval(pt, at, p), p))
    # interactive: the reference prover under the verifier's own draws sees the same transcript
    rng = random.Random(5)
    V2 = lu.Verifier(F, n, ones=ones)
    P, Q = ref.tree(pt, qt, p)
    draw = V2.challenger(rng, (ref.mont(P[0][0], p), ref.mont(Q[0][0], p)))
    live = cases.ref_proof(pkg, pt, qt, p, draw=lambda k, j, msg: ref.canon(draw(k, j, cases.mont_list(msg, p)), p))
    assert V2.result() == (live.point,) + live.claims
    assert lu.Verifier(F, n, ones=ones).verify(live, live.challenges) == (live.point,) + live.claims
    # a random.Random in place of the recorded words draws what the interactive run drew
    assert lu.Verifier(F, n, ones=ones).verify(live, random.Random(5)) == (live.point,) + live.claims


@pytest.mark.parametrize("ones", [False, True], ids=["general", "ones"])
@pytest.mark.parametrize("p", FIELDS)
def test_host_verifier_refuses_every_single_tamper(pkg, p, ones):
    """challenges are random words >= 4: a changed H(2) or H(3) goes unnoticed exactly when the round's challenge is one of the
    other three interpolation points (the cubic's Lagrange weight of the changed value is 0 there).  Denominators are nonzero: a
    changed numerator final is multiplied by the other side's denominator final"""
    lu, F, n = pkg.logup, pkg.Field(p), 5
    qt = table(p, n, 77)
    pt = None if ones else table(p, n, 78, nonzero=False)
    ch = challenges(p, ref.n_challenges(n), 9, low=4)
    proof = cases.ref_proof(pkg, pt, qt, p, ch)
    assert lu.Verifier(F, n, ones=ones).verify(proof, proof.challenges) == (proof.point,) + proof.claims
    listed = cases.tampers(n)
    assert len(listed) == 2 + 12 + 4 * n + 3
    for name, where, expected in listed:
        bad, words = cases.apply_tamper(pkg, proof, where, F)
        cases.expect_refusal(pkg, lu.Verifier(F, n, ones=ones), bad, words, expected)
    # a changed input word: the transcript is accepted, the table's extension at the point is not the claim
    V = lu.Verifier(F, n, ones=ones)
    point, _, _ = V.verify(proof, proof.challenges)
    at = [ref.canon(x, p) for x in point]
    p_value = None if ones else ref.mont(ref.mle_eval(pt, at, p), p)
    q2 = list(qt)
    q2[13] = (q2[13] + 1) % p
    with pytest.raises(lu.InputMismatch) as ei:
        V.check_input(ref.mont(ref.mle_eval(q2, at, p), p), p_value)
    assert ei.value.which == "q"
    if not ones:
        p2 = list(pt)
        p2[13] = (p2[13] + 1) % p
        with pytest.raises(lu.InputMismatch) as ei:
            V.check_input(ref.mont(ref.mle_eval(qt, at, p), p), ref.mont(ref.mle_eval(p2, at, p), p))
        assert ei.value.which == "p"
        # a numerator that is not all ones, under a verifier that was told it is
        with pytest.raises(lu.NumeratorMismatch):
            lu.Verifier(F, n, ones=True).verify(proof, proof.challenges)


def test_verifier_guards(pkg):
    lu = pkg.logup
    with pytest.raises(ValueError):
        lu.Verifier(pkg.Field(3), 4)
    with pytest.raises(ValueError):
        lu.Verifier(pkg.Field(257), 0)
    with pytest.raises(ValueError):
        lu.Verifier(pkg.Field(257), 29)
    V = lu.Verifier(pkg.Field(257), 2)
    with pytest.raises(lu.Error):
        V.round(1, 0, [0, 0, 0, 0], random.Random(1))      # before begin()
    V.begin(5, 7)
    with pytest.raises(lu.Error):
        V.round(1, 0, [0, 0, 0, 0], random.Random(1))      # layer 0 has no rounds: its finals come first
    with pytest.raises(lu.Error):
        V.lam(1, random.Random(1))                         # nor a lambda
    with pytest.raises(lu.Error):
        V.result()


# ---- the lookup --------------------------------------------------------------------------------------------------------

class _Opening:
    """stands where the verifier of a commitment's openings stands in LookupVerifier: only num_vars is read on the CPU"""

    def __init__(self, num_vars):
        self.num_vars = num_vars


def lookup_case(p, n, m, kind, seed):
    """(w, t, idx) in canonical integers: the range table t_j = j or a table of distinct random words"""
    rng = random.Random(seed)
    t = list(range(1 << m))
    if kind != "range":
        seen = set()
        while len(seen) < 1 << m:
            seen.add(rng.randrange(p))
        t = sorted(seen)
        rng.shuffle(t)
    idx = [rng.randrange(1 << m) for _ in range(1 << n)]
    return [t[j] for j in idx], t, idx


def alpha_outside(p, w, t, rng):
    """alpha with no alpha - w_i and no alpha - t_j equal to 0.  Over p = 257 a random alpha hits one of the at most 2^m + 2^n
    words with probability up to 1/6 here, so it is drawn again until it is outside {w_i} u {t_j}: every denominator is then
    invertible and the claim the test checks is the paper's"""
    used = set(w) | set(t)
    while True:
        alpha = rng.randrange(p)
        if alpha not in used:
            return alpha


def run_lookup(pkg, p, n, m, w, t, mult, alpha, seed, table_eval):
    """the reference prover of both sides under a package LookupVerifier; the openings are the extensions by their definition"""
    lu, F = pkg.logup, pkg.Field(p)
    V = lu.LookupVerifier(F, _Opening(n), _Opening(m), table_eval)

    class Fixed:
        def draw(self):
            return ref.mont(alpha, p)
    assert V.draw_alpha(Fixed()) == ref.mont(alpha, p)
    sides = [(None, [(alpha - x) % p for x in w]), (list(mult), [(alpha - x) % p for x in t])]
    trees = [ref.tree(pt, qt, p) for pt, qt in sides]
    V.receive_roots(*[(ref.mont(P[0][0], p), ref.mont(Q[0][0], p)) for P, Q in trees])
    rng = random.Random(seed)
    for which, (pt, qt) in enumerate(sides):
        draw = V.frac[which].challenger(rng)
        ref.prove(pt, qt, p, lambda k, j, msg: ref.canon(draw(k, j, cases.mont_list(msg, p)), p), layers=trees[which])
        point, _ = V.opening(which)
        opened = ref.mle_eval(w if which == 0 else mult, [ref.canon(x, p) for x in point], p)
        V.finish(which, ref.mont(opened, p))
    return True


@pytest.mark.parametrize("kind", ["range", "random"])
@pytest.mark.parametrize("n,m", [(4, 3), (3, 5)])
@pytest.mark.parametrize("p", FIELDS)
def test_lookup_verifier(pkg, p, n, m, kind):
    """over 257 alpha is drawn outside {w_i} u {t_j} (alpha_outside says why); the larger fields take the same path"""
    lu, F = pkg.logup, pkg.Field(p)
    w, t, idx = lookup_case(p, n, m, kind, 10 * n + m)
    mult, bad = ref.multiplicities(w, t, idx)
    assert bad == 0 and sum(mult) == 1 << n and mult == [idx.count(j) for j in range(1 << m)]
    if kind == "range":
        assert list(lu.range_indices(F, cases.mont_list(w, p))) == idx
        table_eval = lambda point: lu.range_table_eval(F, point)   # noqa: E731
        z = [random.Random(1).randrange(p) for _ in range(m)]
        assert ref.range_eval(z, p) == ref.mle_eval(t, z, p) == ref.canon(lu.range_table_eval(F, cases.mont_list(z, p)), p)
    else:
        table_eval = lambda point: ref.mont(ref.mle_eval(t, [ref.canon(x, p) for x in point], p), p)   # noqa: E731
    rng = random.Random(n + m)
    alpha = alpha_outside(p, w, t, rng)
    # the claim itself, by its definition
    inv = lambda x: pow(x, -1, p)   # noqa: E731
    assert sum(inv(alpha - x) for x in w) % p == sum(c * inv(alpha - x) for c, x in zip(mult, t)) % p
    assert run_lookup(pkg, p, n, m, w, t, mult, alpha, 3, table_eval) is True
    # a w_i outside t: it is not counted, and the sums differ
    outside = next(x for x in range(p) if x not in set(t) and x != alpha)
    w2 = list(w)
    w2[5] = outside
    mult2, bad2 = ref.multiplicities(w2, t, idx)
    assert bad2 == 1 and sum(mult2) == (1 << n) - 1
    with pytest.raises(lu.LookupMismatch):
        run_lookup(pkg, p, n, m, w2, t, mult2, alpha_outside(p, w2, t, rng), 3, table_eval)
    # a wrong multiplicity
    mult3 = list(mult)
    mult3[2] += 1
    with pytest.raises(lu.LookupMismatch):
        run_lookup(pkg, p, n, m, w, t, mult3, alpha, 3, table_eval)
    # a public table that is not the prover's: step 7
    V = lu.LookupVerifier(F, _Opening(n), _Opening(m), lambda point: F.add(int(table_eval(point)), F.one))
    with pytest.raises(lu.InputMismatch):
        run_lookup_with(V, pkg, p, w, t, mult, alpha)


def run_lookup_with(V, pkg, p, w, t, mult, alpha):
    """run_lookup's steps under a given LookupVerifier"""
    class Fixed:
        def draw(self):
            return ref.mont(alpha, p)
    V.draw_alpha(Fixed())
    sides = [(None, [(alpha - x) % p for x in w]), (list(mult), [(alpha - x) % p for x in t])]
    trees = [ref.tree(pt, qt, p) for pt, qt in sides]
    V.receive_roots(*[(ref.mont(P[0][0], p), ref.mont(Q[0][0], p)) for P, Q in trees])
    rng = random.Random(4)
    for which, (pt, qt) in enumerate(sides):
        draw = V.frac[which].challenger(rng)
        ref.prove(pt, qt, p, lambda k, j, msg: ref.canon(draw(k, j, cases.mont_list(msg, p)), p), layers=trees[which])
        point, _ = V.opening(which)
        V.finish(which, ref.mont(ref.mle_eval(w if which == 0 else mult, [ref.canon(x, p) for x in point], p), p))


def test_lookup_layer_refuses_a_field_too_small_for_the_counts(pkg):
    lu = pkg.logup
    with pytest.raises(ValueError):
        lu.LookupVerifier(pkg.Field(257), _Opening(10), _Opening(3), None)     # 257 <= 2^10
    with pytest.raises(ValueError):
        lu.LookupVerifier(pkg.Field(257), _Opening(3), _Opening(9), None)      # nor above 2^9
    lu.LookupVerifier(pkg.Field(257), _Opening(8), _Opening(3), None)          # 257 > 2^8


def test_constants_match_the_kernel_header(pkg):
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "fraction.hpp")).read()
    lu = pkg.logup
    assert lu.MAX_LOG == int(re.search(r"constexpr int kFrMaxLog = (\d+);", text).group(1))
    assert lu.TAIL_LOG == int(re.search(r"constexpr int kFrTailLog = (\d+);", text).group(1))
    assert 2 * 8 << lu.TAIL_LOG == 32 << 10, "two tables of the tail fit in 32 KiB"
    assert lu.TREE_LV_MAX == int(re.search(r"constexpr int kFrTreeLvMax = (\d+);", text).group(1))
    assert lu.HOST_LOG_MAX == int(re.search(r"constexpr int kFrHostLogMax = (\d+);", text).group(1))
    assert lu.LOOKUP_LDS_LOG == int(re.search(r"constexpr int kLookupLdsLog = (\d+);", text).group(1))
    assert 4 << lu.LOOKUP_LDS_LOG == 32 << 10, "the counters of the largest LDS histogram are 32 KiB"
    names = pkg._lib.KIND_NAMES
    assert (names[30], names[31], names[32]) == ("fraction_tree", "fraction_pass", "lookup_count")


def test_lookup_seed_separates_the_sums():
    """the fixed rng seed of the GPU test's refused lookup (tests/test_gpu_logup.py, MISMATCH_SEED): with one w_i moved outside t the
    two fraction sums differ at the alpha that seed draws"""
    import test_gpu_logup as g
    p = cases.GOLD
    w, t, mult, alpha = g.mismatch_case(p)
    inv = lambda x: pow(x, -1, p)   # noqa: E731
    assert not set(w) <= set(t) and alpha not in set(w) | set(t)
    assert sum(inv(alpha - x) for x in w) % p != sum(c * inv(alpha - x) for c, x in zip(mult, t)) % p


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/fr_host_harness.cpp, built and run stand-alone: the tree item at LV = 1, 2, 3 (ones and general), both accumulates
    and the host finish against naive 128-bit loops, both fields"""
    exe = tmp_path / "fr_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "fr_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fr host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
