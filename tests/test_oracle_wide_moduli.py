"""The C oracle (oracle/sc_oracle.c) against the big-integer restatement (oracle/pyref.py) on the full-width generic moduli
the GPU suite checks the kernels with (util.WIDE): the product, triangle and W transcripts, the GKR wiring tables and a whole
GKR transcript, on tables and challenges made of the words where the carries of the Montgomery arithmetic happen.  The GPU
tests of tests/test_gpu_wide_moduli.py compare against the C oracle where pyref is too slow; this file is why that is sound.
No GPU needed."""
import random

import numpy as np
import pytest

from test_host_protocols import gkr_draw_count
from util import GOLD, oracle, pyref
from wide_words import (DIFF_CLASSES, WIDE, classes_of, classes_present, degenerate_challenges, diff_classes, edge_table, edge_words, octet_table,
                        select_challenges, stride_classes, wid)


def is_prime(n):
    """Miller-Rabin with the first twelve prime bases: deterministic below 3.3 * 10^24"""
    if n < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for q in bases:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_wide_moduli_are_prime():
    assert all(is_prime(p) for p in WIDE + [GOLD])
    assert not any(is_prime(m) for m in (561, 3215031751, 4294967291 * 4294967279, 2**64 - 1, 2**61 + 1))
    assert WIDE[0] > WIDE[1] > 2**63 > WIDE[2] and WIDE[3] > 2**32 > WIDE[4]


def can(p, ws):
    """Montgomery words -> canonical ints, in Python (not through the oracle's own conversion)"""
    rinv = pow(2**64, -1, p)
    return [int(w) * rinv % p for w in np.atleast_1d(ws)]


def can1(p, w):
    return can(p, [w])[0]


def mont(p, xs):
    return np.array([x * 2**64 % p for x in xs], dtype=np.uint64)


def words(o, p, size, rng):
    """raw (Montgomery) words for the oracle and the canonical ints they stand for, for pyref"""
    raw = edge_table(p, size, rng)
    return raw, can(p, raw)


def chal(o, p, n, rng):
    """challenges: p-1 and p-2 first (as raw words), then edge words and uniform residues"""
    raw = edge_table(p, n, rng)
    raw[:2] = [p - 1, p - 2][:n]
    return raw, can(p, raw)


@pytest.mark.parametrize("p", WIDE + [GOLD], ids=wid)
def test_prove_matches_pyref(p):
    o = oracle(p)
    rng = np.random.default_rng(p % 1009)
    for n in (1, 2, 3, 5):
        for _ in range(2):
            a, ac = words(o, p, 1 << n, rng)
            b, bc = words(o, p, 1 << n, rng)
            ch, chc = chal(o, p, n, rng)
            t = pyref.transcript(ac, bc, chc, p)
            res = o.prove(a, b, ch)
            assert res["status"] == 0 and can1(p, res["c_1"]) == t["c_1"], n
            assert [can(p, r) for r in res["evals"]] == t["evals"], n
            assert [can(p, r) for r in res["coeffs"]] == t["coeffs"], n
            assert can1(p, res["final_eval"]) == t["final_eval"], n
    # every word the same edge word: the largest products the arithmetic meets
    for w in edge_words(p):
        a = np.full(8, w, dtype=np.uint64)
        ch = np.array([p - 1, p - 2, w], dtype=np.uint64)
        t = pyref.transcript(can(p, a), can(p, a[::-1].copy()), can(p, ch), p)
        res = o.prove(a, a[::-1].copy(), ch)
        assert [can(p, r) for r in res["evals"]] == t["evals"] and can1(p, res["final_eval"]) == t["final_eval"], w


@pytest.mark.parametrize("p", WIDE + [GOLD], ids=wid)
def test_tri_prove_matches_pyref(p):
    o = oracle(p)
    rng = np.random.default_rng(p % 1013)
    for k in (1, 2):
        adj, adjc = words(o, p, 1 << (2 * k), rng)
        ch, chc = chal(o, p, 3 * k, rng)
        t = pyref.tri_transcript(adjc, k, chc, p)
        res = o.tri_prove(adj, k, ch)
        assert res["status"] == 0 and can1(p, res["c_1"]) == t["c_1"], k
        assert [can(p, r) for r in res["evals"]] == t["evals"], k
        assert can1(p, res["final_eval"]) == t["final_eval"], k


@pytest.mark.parametrize("p", WIDE + [GOLD], ids=wid)
def test_w_prove_matches_pyref(p):
    o = oracle(p)
    rng = np.random.default_rng(p % 1019)
    for k in (1, 2, 3):
        add, addc = words(o, p, 1 << (2 * k), rng)
        mul, mulc = words(o, p, 1 << (2 * k), rng)
        w, wc = words(o, p, 1 << k, rng)
        ch, chc = chal(o, p, 2 * k, rng)
        t = pyref.w_transcript(addc, mulc, wc, wc, chc, p)
        res = o.w_prove(add, mul, w, w, ch)
        assert res["status"] == 0 and can1(p, res["c_1"]) == t["c_1"], k
        assert [can(p, r) for r in res["evals"]] == t["evals"], k
        assert can1(p, res["final_eval"]) == t["final_eval"], k


def random_layers(rng, ks):
    """layers[i]: 2^ks[i] gates reading layer i+1; every third gate reads one input twice"""
    layers = []
    for i in range(len(ks) - 1):
        n_next = 1 << ks[i + 1]
        layer = [(rng.choice(["add", "mul"]), rng.randrange(n_next), rng.randrange(n_next)) for _ in range(1 << ks[i])]
        layers.append([(t, a, a if g % 3 == 0 else b) for g, (t, a, b) in enumerate(layer)])
    return layers


@pytest.mark.parametrize("p", WIDE + [GOLD], ids=wid)
def test_wiring_fixed_matches_pyref(p):
    o = oracle(p)
    rng = random.Random(p % 1021)
    nrng = np.random.default_rng(p % 1021)
    for k_i, k_next in ((1, 1), (3, 2), (2, 3), (4, 2)):
        layer = random_layers(rng, [k_i, k_next])[0]
        r, rc = chal(o, p, k_i, nrng)
        add, mul = pyref.wiring_fixed(layer, k_next, rc, p)
        oa, om = o.wiring_fixed(layer, k_next, r)
        assert can(p, oa) == add and can(p, om) == mul, (k_i, k_next)
    # many gates on one slot: the sums wrap mod p
    layer = [("add" if g % 2 else "mul", 1, 0) for g in range(16)]
    r = np.array([p - 1, p - 2, p - 1, (p - 1) // 2], dtype=np.uint64)
    add, mul = pyref.wiring_fixed(layer, 1, can(p, r), p)
    oa, om = o.wiring_fixed(layer, 1, r)
    assert can(p, oa) == add and can(p, om) == mul


@pytest.mark.parametrize("p", WIDE + [GOLD], ids=wid)
def test_gkr_transcript_layers_match_the_oracle(p):
    """pyref.gkr_transcript (the whole protocol on canonical ints) layer by layer against the C oracle's wiring tables and
    W transcript at the same r_i and challenges"""
    o = oracle(p)
    rng = random.Random(p % 1031)
    ew = edge_words(p)
    for ks in ([1, 2, 2], [2, 1, 3], [1, 1, 1, 1]):
        layers = random_layers(rng, ks)
        inputs = [can1(p, rng.choice(ew)) if j % 2 else rng.randrange(p) for j in range(1 << ks[-1])]
        draws = [can1(p, rng.choice(ew)) if j % 3 else rng.randrange(p) for j in range(gkr_draw_count(layers, 1 << ks[-1]))]
        ref = pyref.gkr_transcript(layers, 1 << ks[-1], inputs, draws, p)
        assert ref["check_input"]
        vals = pyref.circuit_evaluate(layers, inputs, p)
        r_i = ref["r_0"]
        for i, lr in enumerate(ref["layers"]):
            oa, om = o.wiring_fixed(layers[i], ks[i + 1], mont(p, r_i))
            w = mont(p, vals[i + 1])
            res = o.w_prove(oa, om, w, w, mont(p, lr["challenges"]))
            assert res["status"] == 0 and can1(p, res["c_1"]) == lr["c_1"], (ks, i)
            assert [can(p, r) for r in res["evals"]] == [list(e) for e in lr["evals"]], (ks, i)
            r_i = lr["r_next"]


# ---- the inputs of tests/test_gpu_pass_edge_words.py ----------------------------------------------------------------------

# which corners of wide_words.classes_of exist below each modulus, by reasoning: two words below p sum to 2^64 or more only
# where p > 2^63; a borrow leaves a low limb of 0 only where two words below p differ by a multiple of 2^32, i.e. p > 2^32
_ABSENT = {2**64 - 59: set(), 2**63 + 29: set(), GOLD: set(), 2**61 - 1: {"sum_2_64", "sum_carry"}, 2**32 + 15: {"sum_2_64", "sum_carry"},
           2**32 - 5: {"sum_2_64", "sum_carry", "borrow_low_zero"}}


@pytest.mark.parametrize("p", WIDE + [GOLD], ids=wid)
def test_octet_tables_and_degenerate_challenges(p):
    """octet tables with degenerate challenges are legal inputs on which the C oracle and pyref agree word for word (the GPU
    tests compare the passes with the oracle on them), every transcript word is below p, and the tables really hold every
    difference / sum class that exists for p at the strides 1, 2 and 4"""
    o = oracle(p)
    pairs = diff_classes(p)
    assert all(0 <= lo < p and 0 <= hi < p for lo, hi in pairs) and len(set(pairs)) == len(pairs) <= 20
    assert classes_present(p) == set(DIFF_CLASSES) - _ABSENT[p]
    # the pairs the classes are named after
    assert "borrow_low_ones" in classes_of(p, 1, 0) and "diff_minus_one" in classes_of(p, 1, 0)
    assert "sum_p" in classes_of(p, 1, p - 1) and "sum_p" in classes_of(p, 2**64 % p, p - 2**64 % p)
    assert classes_of(p, 0, 0) == {"diff_zero"}
    if p > 2**63:
        assert {"sum_2_64", "diff_zero"} <= classes_of(p, 2**63, 2**63)
    if p > 0xFFFFFFFF00000000:
        assert "sum_p_to_2_64" in classes_of(p, 0xFFFFFFFF00000000, 2**32 - 1)
    one = 2**64 % p
    assert degenerate_challenges(p, 8) == [0, one, p - 1, 1, p - 2, (p + 1) // 2, 0, one]
    rng = np.random.default_rng(p % 1033)
    for n in (8, 13):
        for _ in range(2):
            t = octet_table(p, 1 << n, rng)
            assert t.dtype == np.uint64 and t.size == 1 << n and int(t.max()) < p
            for s in (1, 2, 4):
                assert stride_classes(p, t, s) >= classes_present(p), (n, s, classes_present(p) - stride_classes(p, t, s))
    # shifted octets: a fold by select_challenges leaves a table of octets with every class again (checked with the oracle's fold)
    for n, k in ((13, 3), (14, 4)):
        t = octet_table(p, 1 << n, rng, shift=k)
        sel = np.array(select_challenges(p, k), dtype=np.uint64)
        folded = o.fix_variables(t, sel)
        assert np.array_equal(folded, t[sum(1 << j for j in range(k) if sel[j]):: 1 << k]) and int(t.max()) < p, (n, k)
        for s in (1, 2, 4):
            assert stride_classes(p, folded, s) >= classes_present(p), (n, k, s)
    for n, k in ((3, 0), (6, 0), (8, 0), (6, 2), (8, 4)):
        a, b = octet_table(p, 1 << n, rng, shift=k), octet_table(p, 1 << n, rng, shift=k)
        ch = np.array((select_challenges(p, k) + degenerate_challenges(p, n))[:n], dtype=np.uint64)
        t = pyref.transcript(can(p, a), can(p, b), can(p, ch), p)
        res = o.prove(a, b, ch)
        assert res["status"] == 0 and can1(p, res["c_1"]) == t["c_1"], n
        assert [can(p, r) for r in res["evals"]] == t["evals"], n
        assert [can(p, r) for r in res["coeffs"]] == t["coeffs"], n
        assert can1(p, res["final_eval"]) == t["final_eval"], n
        assert res["c_1"] < p and res["final_eval"] < p and int(np.max(res["evals"])) < p and int(np.max(res["coeffs"])) < p, n
