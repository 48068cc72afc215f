"""No GPU: the inputs of tests/layered_edge_cases.py carry what tests/test_gpu_layered_edge_words.py needs them to carry, and the
big-integer references it compares the kernels with hold at every modulus (they had only ever run at three): a prover the
reference's own verifier accepts, transcripts that pass their round checks, finals that are the extensions of the inputs at the
challenges by the definition."""
import os
import re

import numpy as np
import pytest

import grand_product_ref as gref
import layered_edge_cases as lc
import logup_ref as lref
import multiopen_ref as mref
import r1cs_ref as rref
import spark_ref as sref
from layered_edge_cases import INPUTS, MODULI, STRIDES, canon_list
from wide_words import classes_present, degenerate_challenges, edge_words, select_challenges, stride_classes, wid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COVER = 11
# what a table without zero words cannot meet: the only pair of diff_classes(p) on this corner is (2^32, 0) where 2^63 + 7 >= p
DENOMINATOR_LOSES = {2**61 - 1: {"borrow_low_zero"}, 2**32 + 15: {"borrow_low_zero"}}


# ---- the inputs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_octet_inputs_meet_every_class_at_every_stride(p):
    want = classes_present(p)
    ins = lc.pass_inputs(p, N_COVER, 16)
    for name in ("octet", "octet-odd"):
        tables, _ = ins[name]
        assert len(tables) == 16
        for k, t in enumerate(tables):
            assert t.shape == (1 << N_COVER,) and t.dtype == np.uint64 and int(t.max()) < p
            for s in STRIDES:
                assert stride_classes(p, t, s) >= want, (name, k, s, sorted(want - stride_classes(p, t, s)))


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_denominator_table_loses_only_the_classes_that_need_a_zero(p):
    want = classes_present(p)
    lost = DENOMINATOR_LOSES.get(p, set())
    assert lost <= want
    t, met = lc.denominator_table(p, N_COVER, np.random.default_rng(p % 1009))
    assert not (t == 0).any() and int(t.max()) < p
    for s in STRIDES:
        assert met[s] == stride_classes(p, t, s)
        assert want - met[s] == lost, (s, sorted(want - met[s]))
    # the denominators the GPU tests use are such tables
    for name in ("octet", "octet-odd"):
        d = lc.denominators_of(p, N_COVER, name)
        assert not (d == 0).any()
        for s in STRIDES:
            assert want - stride_classes(p, d, s) == lost, (name, s)
    for name in ("edge", "pm1"):
        assert not (lc.denominators_of(p, N_COVER, name) == 0).any()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_challenges_are_the_ones_the_inputs_are_built_for(p):
    one = 2**64 % p
    for n in (3, N_COVER):
        ins = lc.pass_inputs(p, n, 3)
        assert set(ins) == set(INPUTS)
        assert ins["octet"][1] == degenerate_challenges(p, n) and ins["octet"][1][:2] == [0, one]
        assert ins["octet-odd"][1] == (select_challenges(p, 3) + degenerate_challenges(p, n - 3)) and ins["octet-odd"][1][:3] == [0, one, one]
        assert set(ins["edge"][1]) <= set(edge_words(p))
        assert ins["pm1"][1] == [p - 1 - (j % 3) for j in range(n)] and all((t == p - 1).all() for t in ins["pm1"][0])
        assert ins["carry"][1] == ([one] + degenerate_challenges(p, n))[:n]
        for t in ins["carry"][0]:
            assert not (t == 0).any() and int(t.max()) < p and lc.carry_quads(p, t) >= max(2, len(t) // 16)
        assert np.array_equal(lc.denominators_of(p, n, "carry"), lc.pass_inputs(p, n, 2)["carry"][0][1])
        for name in INPUTS:
            assert len(ins[name][1]) == n and all(0 <= c < p for c in ins[name][1])
    assert lc.pass_inputs(p, 3, 3) is lc.pass_inputs(p, 3, 3), "computed once"


@pytest.mark.parametrize("a", [5, 14])
def test_run_indices_have_the_runs_where_the_threads_and_waves_are(a):
    idx, runs = lc.run_indices(a)
    top = (1 << a) - 1
    assert len(idx) == lc.SPARK_NNZ and len(idx) % 4 and len(idx) % 256 and sref.log_len(len(idx)) == lc.SPARK_L
    assert int(idx.max()) == top and int(idx.min()) >= 0
    first, end = runs["run"]
    assert first % 4 and end % 4 and (idx[first:end] == top).all() and idx[first - 1] != top and idx[end] != top
    waves = [w for w in range(len(idx) // 256) if first <= 256 * w and 256 * (w + 1) <= end]
    assert len(waves) >= 3, "several whole waves hold the one index"
    f0, f1 = runs["four"]
    assert f0 % 4 == 0 and f1 == f0 + 4 and len(set(idx[f0:f1])) == 1
    assert len(set(idx[f0 - 4:f0])) > 1 and idx[f0 - 1] != idx[f0] and len(set(idx[f1:f1 + 4])) > 1 and idx[f1] != idx[f0]
    t0, t1 = runs["threes"]
    odd_places = set()
    for base in range(t0, t1, 4):
        vals, counts = np.unique(idx[base:base + 4], return_counts=True)
        assert sorted(counts) == [1, 3], base
        odd_places.add(int(np.flatnonzero(idx[base:base + 4] == vals[np.argmin(counts)])[0]))
    assert t0 % 4 == 0 and odd_places == {0, 1, 2, 3}
    u0, u1 = runs["uniform"]
    assert u1 == len(idx) and len(set(idx[u0:u1])) > min(1 << a, 16) // 2
    for small in lc.small_run_indices(a):
        assert len(small) < 256 and sref.log_len(len(small)) == 6


def test_launch_logs_of_the_proofs():
    """the sequences the existing launch-log tests of the five proofs expect, at their sizes"""
    assert lc.pass_log(13, 4) == [(0, 13)] + [(1, 13 - j + 1) for j in range(1, 10)]
    assert lc.pass_log(3, 0) == [(0, 3), (1, 3), (1, 2)] and lc.pass_log(3, 4) == [] and lc.pass_log(1, 0) == []
    assert lc.layered_log(3, 0) == [(0, 1), (0, 2), (1, 2)] and lc.layered_log(3, 2) == []
    want = []
    for k in range(5, 13):
        want.append((0, k))
        want += [(1, k - j + 1) for j in range(1, k - 4 + 1)]
    assert lc.layered_log(13, 4) == want
    assert lc.zerocheck_log(3) == [(0, 3), (1, 3), (1, 2)]


def test_constants_match_the_kernel_headers():
    def const(header, name):
        text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", header)).read()
        return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert lc.GP_TAIL_LOG == const("grand_product.hpp", "kGpTailLog")
    assert lc.FR_TAIL_LOG == const("fraction.hpp", "kFrTailLog")
    assert lc.LOOKUP_LDS_LOG == const("fraction.hpp", "kLookupLdsLog")
    assert lc.EQ_SUM_LO_LOG == const("multiopen.hpp", "kEqSumLoLog")
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "field.hpp")).read() + open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels.hpp")).read()
    assert re.search(r"constexpr int kBlock = %d;" % lc.BLOCK, text) and re.search(r"constexpr int kWave = %d;" % lc.WAVE, text)


# ---- the references at every modulus -----------------------------------------------------------------------------------

CASES = [(p, n, name) for p in MODULI for n in (5, 11) for name in INPUTS]
CASE_IDS = ["%s-%d-%s" % (wid(p), n, name) for p, n, name in CASES]


def replay(ch):
    return lc.layer_draw(ch)


@pytest.mark.parametrize("p,n,name", CASES, ids=CASE_IDS)
def test_grand_product_reference_is_accepted_by_its_verifier(p, n, name):
    t, ch, layers, proof = lc.gp_reference(p, n, name)
    tc, cc = canon_list(t, p), canon_list(ch, p)
    assert layers[n] == tc and proof["product"] == layers[0][0] != 0
    assert any(x != 0 for layer in layers for x in layer)
    point, claim = gref.verify(n, p, proof, replay(cc))
    assert (point, claim) == (proof["point"], proof["claim"])
    assert claim == gref.mle_eval(tc, point, p)
    assert proof["challenges"] == [cc[j] for k in range(n) for j in range(k + 1)]


@pytest.mark.parametrize("ones", [True, False], ids=["ones", "general"])
@pytest.mark.parametrize("p,n,name", CASES, ids=CASE_IDS)
def test_logup_reference_is_accepted_by_its_verifier(p, n, name, ones):
    pt, qt, ch, (P, Q), proof = lc.fr_reference(p, n, name, ones)
    qc, cc = canon_list(qt, p), canon_list(ch, p)
    pc = [1 % p] * len(qc) if ones else canon_list(pt, p)
    assert Q[n] == qc and P[n] == pc and proof["root"] == (P[0][0], Q[0][0]) and Q[0][0] != 0
    point, a, b = lref.verify(n, p, proof, replay(cc), ones=ones)
    assert (point, (a, b)) == (proof["point"], proof["claims"])
    assert a == lref.mle_eval(pc, point, p) and b == lref.mle_eval(qc, point, p)
    assert len(proof["challenges"]) == lref.n_challenges(n)


def eq_at(a, b, p):
    out = 1
    for x, y in zip(a, b):
        out = out * (x * y + (1 - x) * (1 - y)) % p
    return out


@pytest.mark.parametrize("p,n,name", CASES, ids=CASE_IDS)
def test_cubic_references_pass_their_round_checks(p, n, name):
    """r1cs_ref.zerocheck and spark_ref.product3_prove: H(0) + H(1) is the running claim, the next claim is the cubic at the
    challenge, the finals are the extensions of the inputs and meet the last claim"""
    tabs, tau, ch, (c1, rounds, finals) = lc.zc_reference(p, n, name)
    tc, cc, ctau = [canon_list(t, p) for t in tabs], canon_list(ch, p), canon_list(tau, p)
    claim = c1
    for e, r in zip(rounds, cc):
        assert len(e) == 4 and (e[0] + e[1]) % p == claim
        claim = rref.cubic_at(e, r, p)
    assert len(rounds) == n and tuple(finals) == tuple(gref.mle_eval(t, cc, p) for t in tc)
    assert eq_at(ctau, cc, p) * (finals[0] * finals[1] - finals[2]) % p == claim
    assert all(any(e) for e in rounds), "tau and the challenges leave an eq table that is not all zero: the rounds say something"

    tabs3, ch3, (c1, rounds, rs, finals) = lc.p3_reference(p, n, name)
    assert ch3 == ch and rs == cc and all(x is y for x, y in zip(tabs3, tabs)), "the same three tables"
    claim = c1
    for e, r in zip(rounds, cc):
        assert len(e) == 4 and (e[0] + e[1]) % p == claim
        claim = sref.cubic_at(e, r, p)
    assert len(rounds) == n and tuple(finals) == tuple(gref.mle_eval(t, cc, p) for t in tc)
    assert finals[0] * finals[1] * finals[2] % p == claim
    assert c1 == sum(x * y * z for x, y, z in zip(*tc)) % p


@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("p,n,name", CASES, ids=CASE_IDS)
def test_sum_of_products_reference_passes_its_round_checks(p, n, name, T):
    a, b, ch, (rounds, rs, fa, fb) = lc.sp_reference(p, n, name, T)
    assert len(a) == len(b) == T
    if T == 3:
        assert a[2] is b[1] and b[2] is a[0], "one table in several pairs"
    ac, bc, cc = [canon_list(t, p) for t in a], [canon_list(t, p) for t in b], canon_list(ch, p)
    assert rs == cc and len(rounds) == n
    claim = sum(x * y for s, t in zip(ac, bc) for x, y in zip(s, t)) % p
    for e, r in zip(rounds, cc):
        assert len(e) == 3 and (e[0] + e[1]) % p == claim
        claim = mref.quadratic_at(e, r, p)
    assert fa == [gref.mle_eval(t, cc, p) for t in ac] and fb == [gref.mle_eval(t, cc, p) for t in bc]
    assert sum(x * y for x, y in zip(fa, fb)) % p == claim
