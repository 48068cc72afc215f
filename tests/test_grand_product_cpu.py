"""CPU-only: the grand product argument's reference (tests/grand_product_ref.py) against the dense definitions, the package's
host Verifier (thaler-study_amd/grand_product.py) against the reference prover - honest runs are accepted, every single
tampered message is refused with its own error - and the SC_HD and host-finish code of kernels/grand_product.hpp, compiled for
the host and run stand-alone (tests/cpp/gp_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import grand_product_cases as cases
import grand_product_ref as ref
from conftest import ROOT

FIELDS = [257, cases.GOLD, cases.P64]


def table(p, n, seed, zero_at=None):
    rng = random.Random(seed)
    edge = [e for e in (1, p - 1, p - 2, (p - 1) // 2, 2**64 % p, (2**32 - 1) % p) if e]   # (nonzero: a zero makes every later claim 0)
    t = [rng.choice(edge) if rng.random() < 0.3 else rng.randrange(1, p) for _ in range(1 << n)]
    if zero_at is not None:
        t[zero_at] = 0
    return t


def challenges(p, count, seed, low=0):
    """canonical challenges: 0, 1, p - 1 and random words mixed (low = 0), or random words >= low"""
    rng = random.Random(seed)
    if low:
        return [rng.randrange(low, p) for _ in range(count)]
    return [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(count)]


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_reference_against_the_dense_definitions(p, n):
    t = table(p, n, 100 + n)
    V = ref.tree(t, p)
    assert len(V) == n + 1 and V[n] == t and [len(v) for v in V] == [1 << k for k in range(n + 1)]
    prod = 1
    for x in t:
        prod = prod * x % p
    assert V[0] == [prod]
    rng = random.Random(n)
    for k in range(n):
        half = 1 << k
        L, R = V[k + 1][:half], V[k + 1][half:]
        z = [rng.randrange(p) for _ in range(k)]
        # the layer identity: V_k~(z) = sum_x eq(z, x) L_k(x) R_k(x), V_k~ by its definition
        eq = ref.eq_table(z, p)
        assert ref.mle_eval(V[k], z, p) == sum(e * l * r for e, l, r in zip(eq, L, R)) % p
        # eq by its definition
        for x in range(half):
            want = 1
            for j in range(k):
                want = want * (z[j] if (x >> j) & 1 else 1 - z[j]) % p
            assert eq[x] == want
        # the combining step: V_(k+1)~(r, rho) = l + rho (r' - l)
        r, rho = [rng.randrange(p) for _ in range(k)], rng.randrange(p)
        l, r2 = ref.mle_eval(L, r, p), ref.mle_eval(R, r, p)
        assert ref.mle_eval(V[k + 1], r + [rho], p) == (l + rho * (r2 - l)) % p
    # the whole proof: the verifier accepts, and the last claim is the table's extension at the point
    ch = challenges(p, cases.n_challenges(n), 7 * n)
    it, it2 = iter(ch), iter(ch)
    proof = ref.prove(t, p, lambda k, j, msg: next(it))
    assert proof["challenges"] == ch and proof["product"] == prod
    point, claim = ref.verify(n, p, proof, lambda k, j, msg: next(it2))
    assert (point, claim) == (proof["point"], proof["claim"]) and ref.mle_eval(t, point, p) == claim
    # every round's message against the claim it must meet, and the folds against the extension
    for k in range(n):
        for j, msg in enumerate(proof["rounds"][k]):
            assert len(msg) == 4 and ref.cubic_at(msg, 2, p) == msg[2] and ref.cubic_at(msg, 3, p) == msg[3]


@pytest.mark.parametrize("p", FIELDS)
def test_reference_product_with_a_zero_entry(p):
    for at in (0, 16, 31):
        t = table(p, 5, 3, zero_at=at)
        V = ref.tree(t, p)
        assert V[0] == [0]
        ch = challenges(p, cases.n_challenges(5), at)
        it = iter(ch)
        proof = ref.prove(t, p, lambda k, j, msg: next(it), layers=V)
        it = iter(ch)
        point, claim = ref.verify(5, p, proof, lambda k, j, msg: next(it))
        assert ref.mle_eval(t, point, p) == claim


@pytest.mark.parametrize("p", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 5])
def test_host_verifier_accepts_the_reference_prover(pkg, p, n):
    gp, F = pkg.grand_product, pkg.Field(p)
    t = table(p, n, 11 * n)
    ch = challenges(p, cases.n_challenges(n), n)
    proof = cases.ref_proof(pkg, t, p, ch)
    V = gp.Verifier(F, n)
    point, claim = V.verify(proof, proof.challenges)
    assert point == proof.point and claim == proof.claim
    assert V.check_input(ref.mont(ref.mle_eval(t, [ref.canon(x, p) for x in point], p), p))
    # interactive: the reference prover under the verifier's own draws sees the same transcript
    rng = random.Random(5)
    V2 = gp.Verifier(F, n)
    draw = V2.challenger(rng, ref.mont(ref.tree(t, p)[0][0], p))
    live = cases.ref_proof(pkg, t, p, draw=lambda k, j, msg: ref.canon(draw(k, j, cases.mont_list(msg, p)), p))
    assert V2.result() == (live.point, live.claim)
    assert gp.Verifier(F, n).verify(live, live.challenges) == (live.point, live.claim)
    # a random.Random in place of the recorded words draws what the interactive run drew
    assert gp.Verifier(F, n).verify(live, random.Random(5)) == (live.point, live.claim)


@pytest.mark.parametrize("p", FIELDS)
def test_host_verifier_refuses_every_single_tamper(pkg, p):
    """challenges are random words >= 4: a changed H(2) or H(3) goes unnoticed exactly when the round's challenge is one of
    the other three interpolation points (the cubic's Lagrange weight of the changed value is 0 there)"""
    gp, F, n = pkg.grand_product, pkg.Field(p), 5
    t = table(p, n, 77)
    ch = challenges(p, cases.n_challenges(n), 9, low=4)
    proof = cases.ref_proof(pkg, t, p, ch)
    assert gp.Verifier(F, n).verify(proof, proof.challenges) == (proof.point, proof.claim)
    listed = cases.tampers(n)
    assert len(listed) == 1 + 12 + 2 * n
    for name, where, expected in listed:
        cases.expect_refusal(pkg, gp.Verifier(F, n), cases.apply_tamper(pkg, proof, where, F), proof.challenges, expected)
    # a changed input word: the transcript is accepted, the table's extension at the point is not the claim
    t2 = list(t)
    t2[13] = (t2[13] + 1) % p
    V = gp.Verifier(F, n)
    point, _ = V.verify(proof, proof.challenges)
    with pytest.raises(gp.InputMismatch):
        V.check_input(ref.mont(ref.mle_eval(t2, [ref.canon(x, p) for x in point], p), p))


def test_verifier_guards(pkg):
    gp = pkg.grand_product
    with pytest.raises(ValueError):
        gp.Verifier(pkg.Field(3), 4)
    with pytest.raises(ValueError):
        gp.Verifier(pkg.Field(257), 0)
    with pytest.raises(ValueError):
        gp.Verifier(pkg.Field(257), 29)
    V = gp.Verifier(pkg.Field(257), 2)
    with pytest.raises(gp.Error):
        V.round(1, 0, [0, 0, 0, 0], random.Random(1))      # before begin()
    V.begin(5)
    with pytest.raises(gp.Error):
        V.round(1, 0, [0, 0, 0, 0], random.Random(1))      # layer 0 has no rounds: its finals come first
    with pytest.raises(gp.Error):
        V.result()


def test_constants_match_the_kernel_header(pkg):
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "grand_product.hpp")).read()
    gp = pkg.grand_product
    assert gp.MAX_LOG == int(re.search(r"constexpr int kGpMaxLog = (\d+);", text).group(1))
    assert gp.TAIL_LOG == int(re.search(r"constexpr int kGpTailLog = (\d+);", text).group(1)) <= 12
    assert gp.HOST_LOG_MAX == int(re.search(r"constexpr int kGpHostLogMax = (\d+);", text).group(1))
    assert pkg._lib.KIND_NAMES[28] == "product_tree" and pkg._lib.KIND_NAMES[29] == "product_pass"


def test_permutation_seed_separates_the_products():
    """the fixed rng seed of the GPU test's mismatch case (tests/test_gpu_grand_product.py, MISMATCH_SEED): with one word of b
    changed the two products differ at the gamma that seed draws"""
    import test_gpu_grand_product as g
    p = cases.GOLD
    a, b, gamma = g.mismatch_case(p)
    pa = pb = 1
    for x, y in zip(a, b):
        pa, pb = pa * (gamma - x) % p, pb * (gamma - y) % p
    assert sorted(a) != sorted(b) and pa != pb


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/gp_host_harness.cpp, built and run stand-alone: the tree item at LV = 1, 2, 3, the cubic item and the host
    finish against naive 128-bit loops, both fields"""
    exe = tmp_path / "gp_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "gp_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "gp host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
