"""No GPU: the inputs of tests/ext_edge_cases.py carry what tests/test_gpu_ext_edge_words.py needs them to carry - the planes the
reference's own fold holds at the round a kernel receives them meet every corner of wide_words.classes_of, the carry quads survive
into both planes - and the reference it compares the kernels with (tests/ext_ref.py) passes its round checks and its final check on
every such input at every modulus, and agrees with the closed form over constant planes."""
import numpy as np
import pytest

import ext_edge_cases as ec
import ext_ref as ref
from ext_edge_cases import MODULI
from layered_edge_cases import carry_quads
from util import GOLD
from wide_words import classes_present, degenerate_challenges, edge_words, octet_table, wid

N_COVER = 11
T = 3
# Classes a position cannot meet, by name, with the reason - {(input, position): {class: reason}}.  None is needed: the planes are
# injected word for word, zeros included, so the octet planes keep every pair of diff_classes(p) at stride 1 and the cross tables
# every pair across the two components.  The cap: nothing for "entry", at most the classes that need a zero word for "c0", "c1".
EXCUSED = {}
NEED_A_ZERO_WORD = {"borrow_low_zero"}          # where 2^63 + 7 >= p the only pair on this corner is (2^32, 0)


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_inject_puts_both_planes_into_round_1_word_for_word(p):
    w = ref.nonresidue(p)
    rng = np.random.default_rng(p % 1009)
    for E0, E1 in ((octet_table(p, 64, rng), octet_table(p, 64, rng)), ec.cross_planes(p, 64, rng),
                   (np.full(8, p - 1, dtype=np.uint64), np.full(8, p - 1, dtype=np.uint64))):
        u = ec.inject(p, E0, E1)
        assert u.dtype == np.uint64 and len(u) == 2 * len(E0) and int(u.max()) < p
        c0, c1 = ec.planes_at(p, w, u, [ec.x_of(p)], 1)
        assert c0 == [int(x) for x in E0] and c1 == [int(x) for x in E1]
    assert [int(x) for x in ec.inject(p, [p - 1] * 2, [p - 1] * 2)] == [p - 1, p - 2] * 2


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_planes_meet_every_class_in_both_planes_and_across_them(p):
    """at the round whose launch receives them (planes: 1, planes-deep: 2), from the reference's own fold: each octet-plane
    table at the neighbours of its c0 and of its c1 plane, each cross table across the components of its entries and across the
    components of its differences"""
    w, want = ref.nonresidue(p), classes_present(p)
    ins = ec.ext_inputs(p, N_COVER, T)
    for name, rnd in ec.COVER_ROUND.items():
        a, b, ch = ins[name]
        excused = {pos: set(EXCUSED.get((name, pos), {})) for pos in ("c0", "c1", "entry")}
        assert not excused["entry"] and excused["c0"] <= NEED_A_ZERO_WORD and excused["c1"] <= NEED_A_ZERO_WORD
        for t in (a[0], b[0]):
            met = ec.plane_classes(p, w, [t], ch, rnd)
            assert met["c0"] >= want - excused["c0"], (name, sorted(want - met["c0"]))
            assert met["c1"] >= want - excused["c1"], (name, sorted(want - met["c1"]))
        for t in (a[1], b[1]):
            assert ec.plane_classes(p, w, [t], ch, rnd)["entry"] >= want, name
            assert ec.diff_sum_classes(p, w, [t], ch, rnd) >= want, name
        met = ec.plane_classes(p, w, a + b, ch, rnd)
        for pos in ("c0", "c1", "entry"):
            assert met[pos] >= want - excused[pos], (name, pos)
    assert set(ec.COVER_ROUND) == {n for n in ec.NAMES if n.startswith("planes")}


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_inputs_are_the_ones_the_gpu_tests_are_built_for(p):
    one, X, w = ec.one_of(p), ec.x_of(p), ref.nonresidue(p)
    for n in (4, N_COVER):
        ins = ec.ext_inputs(p, n, T)
        assert set(ins) == set(ec.names_of(p)) and ("const-down" in ins) == (p == GOLD)
        cyc = degenerate_challenges(p, n + 1)
        for name, (a, b, ch) in ins.items():
            assert len(a) == len(b) == T and len(ch) == n and all(0 <= c < p for r in ch for c in r)
            for t in a + b:
                assert t.shape == (1 << n,) and t.dtype == np.uint64 and int(t.max()) < p and not t.flags.writeable
            if name.startswith("const"):
                assert all(t is a[0] for t in a + b), "one array as every a_t and b_t"
            else:
                assert a[2] is b[1] and b[2] is a[0] and len({id(t) for t in a + b}) == 4, "one table in several pairs"
        assert all(ins[name][2][0] == X for name in ins if name.startswith(("planes", "const")) or name == "carry-planes")
        assert ins["planes-deep-even"][2][1] == (0, 0) and ins["planes-deep-odd"][2][1] == (one, 0)
        assert ins["planes-deep-odd"][2][2:] == [(cyc[j], cyc[j + 1]) for j in range(n - 2)] and ins["planes-deep-odd"][2][2] == X
        assert ins["late-x"][2][:3] == [(0, 0), (one, 0), X]
        assert ins["carry-base"][2][0] == (one, 0) and ins["carry-planes"][2][1] == (one, 0)
        for name in ("planes", "edge", "const"):
            assert {c for r in ins[name][2][1:] for c in r} <= set(edge_words(p))
        assert set(ins["edge"][2][0]) <= set(edge_words(p))
        # late-x: the c1 plane is all zero until X arrives and holds differences of table words after it
        table, ch = ins["late-x"][0][0], ins["late-x"][2]
        assert not any(ec.planes_at(p, w, table, ch, 2)[1])
        c0, c1 = ec.planes_at(p, w, table, ch, 3)
        assert c1 == [(int(table[8 * i + 6]) - int(table[8 * i + 2])) % p for i in range(len(c1))] and any(c1)
        assert c0 == [int(table[8 * i + 2]) for i in range(len(c0))]
        # const: both planes constant from round 1 to the end
        table, ch = ins["const"][0][0], ins["const"][2]
        assert np.array_equal(table, ec.inject(p, [p - 1] * (len(table) // 2), [p - 1] * (len(table) // 2)))
        assert ec.const_input(p, n, T, "const") == ins["const"] and ec.const_input(p, 1, 8, "const")[2] == [X]
        for rnd in (1, 2, n):
            assert ec.planes_at(p, w, table, ch, rnd) == ([p - 1] * (1 << (n - rnd)), [p - 1] * (1 << (n - rnd)))
    assert ec.ext_inputs(p, 4, T) is ec.ext_inputs(p, 4, T), "computed once"


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_carry_inputs_keep_a_carry_quad_in_every_plane(p):
    """at n = 4: the base tables themselves under r_0 = (one, 0), and both planes of the injected ones at round 1, where
    r_1 = (one, 0) folds them - and at round 2 the odd entries y have come through as y (the reference reduces), which is what
    the kernels' last correction of add must deliver"""
    w = ref.nonresidue(p)
    for n in (4, N_COVER):
        a, b, ch = ec.ext_inputs(p, n, T)["carry-base"]
        for t in a + b:
            assert not (t == 0).any() and carry_quads(p, t) >= 1
        a, b, ch = ec.ext_inputs(p, n, T)["carry-planes"]
        for t in a + b:
            for k, plane in enumerate(ec.planes_at(p, w, t, ch, 1)):
                assert carry_quads(p, plane) >= 1, (n, k)
                folded = ec.planes_at(p, w, t, ch, 2)[k]
                assert folded == plane[1::2]
                assert any(lo + p < 2**64 and hi < lo for lo, hi in zip(folded[0::2], folded[1::2])), "the next difference borrows"


CASES = [(p, name) for p in MODULI for name in ec.names_of(p)]


@pytest.mark.parametrize("p,name", CASES, ids=["%s-%s" % (wid(p), name) for p, name in CASES])
def test_reference_passes_its_round_checks_and_its_final_check(p, name):
    n, w = 4, ref.nonresidue(p)
    a, b, cc, (c1, rounds, rs, fa, fb) = ec.ext_reference(p, n, T, name)
    assert rs == cc == ec.canon_pairs(ec.ext_inputs(p, n, T)[name][2], p) and len(rounds) == n
    ac, bc = [ec.canon_list(t, p) for t in a], [ec.canon_list(t, p) for t in b]
    assert c1 == (sum(x * y for s, t in zip(ac, bc) for x, y in zip(s, t)) % p, 0)
    assert all(m[1] == 0 for m in rounds[0])
    claim = c1
    for msg, r in zip(rounds, cc):
        assert ref.kadd(msg[0], msg[1], p) == claim
        assert ref.quadratic_at(msg, (2, 0), p, w) == msg[2]
        claim = ref.quadratic_at(msg, r, p, w)
    assert fa == [ref.mle_eval(t, cc, p, w) for t in ac] and fb == [ref.mle_eval(t, cc, p, w) for t in bc]
    final = (0, 0)
    for x, y in zip(fa, fb):
        final = ref.kadd(final, ref.kmul(x, y, p, w), p)
    assert final == claim
    assert ec.ext_reference(p, n, T, name) is ec.ext_reference(p, n, T, name), "computed once"


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_closed_form_over_constant_planes_is_the_reference(p):
    w = ref.nonresidue(p)
    rinv = pow(2**64, -1, p)
    words = [p - 1, 1, 0, ec.DOWN_WORD % p, 2**64 % p]
    for n in (1, 2, 5, 8):
        for count in (1, 3, 8):
            for k in range(2 if n == 8 else len(words)):
                e_raw = (words[k], words[(k + n) % len(words)] if count != 3 else words[k])
                e = (e_raw[0] * rinv % p, e_raw[1] * rinv % p)
                table = ec.canon_list(ec.inject(p, [e_raw[0]] * (1 << (n - 1)), [e_raw[1]] * (1 << (n - 1))), p)
                rng = np.random.default_rng([n, count, k])
                ch = ec.canon_pairs([ec.x_of(p)] + ec.edge_pairs(p, n - 1, rng), p)
                c1, rounds, rs, fa, fb = ref.sumcheck([table] * count, [table] * count, p, w, lambda j, msg: ch[j])
                assert (c1, rounds, fa, fb) == ec.const_transcript(p, w, n, count, e), (n, count, e_raw)
    # the inputs the GPU tests run, at the sizes the reference reaches
    for name in ec.names_of(p):
        if name.startswith("const"):
            e = ec.canon_list([ec.const_word(p, name)] * 2, p)
            for n in (4, 8):
                c1, rounds, rs, fa, fb = ec.ext_reference(p, n, T, name)[3]
                assert (c1, rounds, fa, fb) == ec.const_transcript(p, w, n, T, e)
