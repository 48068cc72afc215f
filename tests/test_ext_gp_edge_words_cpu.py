"""No GPU: the inputs of tests/ext_gp_edge_cases.py carry what tests/test_gpu_ext_gp_edge_words.py needs them to carry.  The tables
E, L, R a launch reads are taken from the reference's own tree and fold (ext_gp_edge_cases.tables_at), never from a formula of the
builder: they meet every corner of wide_words.classes_of in the plane an input targets and across the components of an entry, the
carry quads arrive in the targeted plane, E has no zero entry where chosen words sit under it, every injected word is observable,
and the reference (tests/ext_gp_ref.py) passes its own round and final identities on every input and agrees with the closed form
over a constant table."""
import os
import re

import numpy as np
import pytest

import ext_gp_edge_cases as gc
import ext_gp_ref as ref
import ext_ref as xref
from conftest import ROOT
from ext_edge_cases import canon_list, canon_pairs
from ext_gp_edge_cases import MODULI
from layered_edge_cases import carry_quads
from wide_words import classes_present, diff_classes, edge_words, wid

N_LEAF = 12              # 2^11 chosen words per table of layer n - 1, as the GPU file runs it
N_OBSERVE = 6
# Classes a position cannot meet, by name, with the reason - {(input, position): {class: reason}}.  It stays empty: the leaf maps
# keep the zero words of an octet table (d != 0) and the injection is word for word.  No class may be excused.
EXCUSED = {}


def size_of(name):
    """the n at which the targeted layer of an input holds 2^(N_LEAF - 1) chosen words per table (planes2-*: 13, planes3-*: 14)"""
    return N_LEAF + (int(name[6]) - 1 if name[6:7] in ("2", "3") else 0)


def test_nothing_is_excused():
    assert EXCUSED == {}


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_leaf_maps_are_few_and_of_the_stated_form(p):
    maps = gc.leaf_maps(p)
    assert 1 <= len(maps) <= 4 and all(s in (1, -1) and 0 < d < p for s, d in maps)
    assert gc.names_of(p)[:len(maps)] == gc.leaf_entry_names(p) and len(set(gc.names_of(p))) == len(maps) + len(gc.FIXED)
    one = gc.one_of(p)
    for name, (s, d) in zip(gc.leaf_entry_names(p), maps):
        inp = gc.gp_input(p, 4, name)
        assert inp.alpha == (one, one if s > 0 else p - one) and inp.beta == (0, d)
    assert gc.gp_input(p, 4, "leaf-c1")[1:3] == ((one, one), (1, 0))
    perm = gc.gp_input(p, 4, "leaf-perm")
    assert perm.alpha == (p - one, 0) and set(perm.beta) <= set(edge_words(p))


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_chosen_words_meet_every_class_in_the_targeted_plane(p):
    """at the launch each input names, in L and in R: the neighbours (2 i, 2 i + 1) of the c0 plane (leaf-entry-*, leaf-deep-*,
    planes-c0, planes2-c0, planes3-c0) or of the c1 plane (leaf-c1, planes-c1, planes2-c1, planes3-c1) - and E has no zero entry
    there.  Which inputs are checked follows from their `plane`: every one that targets a single plane with an octet table"""
    want = classes_present(p)
    checked = set()
    for name in gc.names_of(p) + gc.TREE_ONLY:
        inp = gc.gp_input(p, size_of(name), name)
        tabs = gc.tables_at(p, inp)
        if name != "edge":
            assert not any(a == 0 and b == 0 for a, b in zip(*tabs["E"])), (name, "E has a zero entry at the covered launch")
        if inp.plane in ("c0", "c1") and "carry" not in name:
            for which in "LR":
                met = gc.table_classes(p, tabs[which])[inp.plane]
                assert met >= want, (name, which, sorted(want - met))
                assert len(tabs[which][0]) == 1 << (size_of(name) - inp.depth - 1 - inp.cover[1]) >= 1 << 10
            checked.add(name)
    octets = {name for name in gc.names_of(p) + gc.TREE_ONLY if name.startswith(("leaf-entry-", "leaf-c1", "leaf-deep", "planes")) and "carry" not in name}
    assert checked == octets and {"planes3-c0", "planes3-c1"} <= checked


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_entries_meet_every_class_across_their_components(p):
    """(c0[i], c1[i]) of L and R: the leaf-entry-* inputs taken together at the leaves, the planes-entry inputs taken together in
    layer n - 1, each of which holds the pair it was solved for"""
    want = classes_present(p)
    met = set()
    for name in gc.leaf_entry_names(p):
        tabs = gc.tables_at(p, gc.gp_input(p, N_LEAF, name))
        met |= gc.table_classes(p, tabs["L"])["entry"] | gc.table_classes(p, tabs["R"])["entry"]
    assert met >= want, sorted(want - met)
    met = set()
    inputs = gc.entry_inputs(p)
    pairs = gc.entry_pairs(p)
    assert len(inputs) == len(pairs) and set(diff_classes(p)) - set(pairs) == {(0, 0)}, "only the zero of K is left out"
    for inp, (lo, hi) in zip(inputs, pairs):
        assert inp.cover == (gc.ENTRY_N - 2, 0) and len(inp.table) == 1 << gc.ENTRY_N
        tabs = gc.tables_at(p, inp)
        for which in "LR":
            entries = list(zip(*tabs[which]))
            assert all(e == (lo, hi) for e in entries[0::2]) and len(set(entries)) > 1, (lo, hi)
        assert not any(a == 0 and b == 0 for a, b in zip(*tabs["E"]))
        met |= gc.table_classes(p, ([lo], [hi]))["entry"]
    assert met >= want, sorted(want - met)


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_injection_is_word_for_word(p):
    """the reference's tree holds the chosen words in the plane and the layer the builder means, at depth 1, 2 and 3, and ones above
    them; the deep leaf inputs hand the even (odd) leaves to round 1"""
    w, one = xref.nonresidue(p), gc.one_of(p)
    rng = np.random.default_rng(p % 1009)
    for n, depth in ((5, 1), (6, 2), (7, 3), (4, 2)):
        for plane in ("c0", "c1"):
            u = rng.integers(0, p, size=1 << (n - depth), dtype=np.uint64)
            u[0], u[1] = 0, p - 1
            t, alpha, beta = gc.inject(p, n, depth, u, plane)
            assert t.dtype == np.uint64 and int(t.max()) < p and (t[len(u):] == gc.base_word(p)).all()
            V = ref.tree(ref.leaves(canon_list(t, p), tuple(canon_list(alpha, p)), tuple(canon_list(beta, p)), p, w), p, w)
            got = [tuple(gc.mont_list(e, p)) for e in V[n - depth]]
            other = (lambda x: (x - one) % p) if plane == "c0" else (lambda x: one)
            assert got == [(int(x), other(int(x))) if plane == "c0" else (other(int(x)), int(x)) for x in u]
            assert all(e == (1, 0) for e in V[n][len(u):])
    for name, low in (("leaf-deep-even", 0), ("leaf-deep-odd", 1)):
        inp = gc.gp_input(p, 6, name)
        tabs = gc.tables_at(p, inp)
        assert tabs["L"][0] == [int(x) for x in inp.table[low:32:2]] and tabs["R"][0] == [int(x) for x in inp.table[32 + low::2]]
        assert tabs["L"][1] == [(int(x) + 1) % p for x in inp.table[low:32:2]]
    assert gc.gp_input(p, 6, "planes-c1") is gc.gp_input(p, 6, "planes-c1"), "computed once"
    assert not gc.gp_input(p, 6, "planes-c1").table.flags.writeable


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_carry_inputs_keep_their_quads_in_the_targeted_plane(p):
    """before the fold by (one, 0) the targeted planes of L and R hold carry quads; after it (the launch the input names) the odd
    entries have come through as they were - the reference reduces, which is what the last correction of add must deliver - and the
    next difference borrows against a word y with y + p < 2^64"""
    for name, planes in (("leaf-carry", (0, 1)), ("planes-carry-c0", (0,)), ("planes-carry-c1", (1,))):
        for n in (4, N_LEAF):
            inp = gc.gp_input(p, n, name)
            layer, rnd = inp.cover
            assert rnd == 1 and inp.challenges[gc.challenge_index(layer, 0)] == (gc.one_of(p), 0)
            before, after = gc.tables_at(p, inp, layer, 0), gc.tables_at(p, inp)
            for c in planes:
                quads = {which: carry_quads(p, before[which][c]) if len(before[which][c]) >= 4 else 0 for which in "LR"}
                # 2^11 entries: quads in L and in R; sixteen: about half of four quads are built, wherever they fall
                assert min(quads.values()) >= 64 if n == N_LEAF else sum(quads.values()) >= 1, (name, n, c, quads)
                for which in "LR":
                    plane, folded = before[which][c], after[which][c]
                    assert folded == plane[1::2]
                    if quads[which]:
                        assert any(lo + p < 2**64 and hi < lo for lo, hi in zip(folded[0::2], folded[1::2])), "the next difference borrows"


def covered_messages(p, r):
    """what the covered layer sends: its rounds and its finals (edge: the whole transcript - its E may be zero on half its entries)"""
    k = r.input.cover[0]
    return r.out if r.input.plane is None else (r.out["rounds"][k], r.out["finals"][k])


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_every_injected_word_is_observable(p):
    """n = 6 (planes-entry: its own n): one added to any single injected word changes what the covered layer sends"""
    inputs = [gc.gp_input(p, N_OBSERVE, name) for name in gc.names_of(p)] + gc.entry_inputs(p)
    for inp in inputs:
        base = covered_messages(p, gc._reference(p, inp))
        for i in range(inp.injected):
            t = np.array(inp.table)
            t[i] = (int(t[i]) + 1) % p
            assert covered_messages(p, gc._reference(p, inp._replace(table=t))) != base, (inp.cover, inp.plane, i)


CASES = [(p, name) for p in MODULI for name in gc.names_of(p) + ("planes-entry",)]


@pytest.mark.parametrize("p,name", CASES, ids=["%s-%s" % (wid(p), name) for p, name in CASES])
def test_reference_passes_its_round_checks_and_its_final_check(p, name):
    """n = 5: no product is 0, every challenge is the raw pair the input names, and the reference's own verifier accepts"""
    w = xref.nonresidue(p)
    refs = gc.entry_references(p) if name == "planes-entry" else [gc.gp_reference(p, 5, name)]
    for r in refs:
        n, out = 5, r.out
        assert out["product"] != (0, 0), "no input has product 0"
        assert r.alpha != (0, 0) and out["challenges"] == r.challenges == canon_pairs(r.input.challenges, p) and len(r.challenges) == ref.n_challenges(n)
        assert all(0 <= c < p for pair in r.input.challenges for c in pair) and int(r.input.table.max()) < p
        if name == "edge":
            e = set(edge_words(p))
            assert {c for pair in r.input.challenges for c in pair} | set(r.input.alpha) | set(r.input.beta) <= e
        point, claim = ref.verify(n, p, w, out, lambda k, j, msg, it=iter(r.challenges): next(it))
        assert (point, claim) == (out["point"], out["claim"])
        assert claim == xref.kadd(r.beta, xref.kmul(r.alpha, xref.mle_eval(r.table, point, p, w), p, w), p)
    assert gc.gp_reference(p, 5, gc.FIXED[0]) is gc.gp_reference(p, 5, gc.FIXED[0]), "computed once"


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_products_at_the_sizes_of_the_gpu_file_are_not_zero(p):
    """a zero leaf would make the product 0 and the low layers of the tree all zero: none at n = 4, 12 (13 for planes2)"""
    for name in gc.names_of(p):
        for n in (4, size_of(name)):
            inp = gc.gp_input(p, n, name)
            assert not gc._zero_leaf(p, inp.table, inp.alpha, inp.beta), (name, n)


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_closed_form_over_a_constant_table_is_the_reference(p):
    w = xref.nonresidue(p)
    for n in range(3, 9):
        r = gc._reference(p, gc.const_input(p, n))
        leaf = ref.leaves(r.table[:1], r.alpha, r.beta, p, w)[0]
        assert tuple(gc.mont_list(leaf, p)) == (p - 1, p - 1), "p - 1 in both planes of the leaves"
        assert gc.const_transcript(p, w, n, leaf, r.challenges) == r.out, n
    # other constants, other challenges
    rng = np.random.default_rng(p % 1013)
    for n in (3, 5):
        v = (int(rng.integers(1, p, dtype=np.uint64)), int(rng.integers(0, p, dtype=np.uint64)))
        cc = canon_pairs(gc.edge_pairs(p, ref.n_challenges(n), rng), p)
        out = ref.prove([1] * (1 << n), v, (0, 0), p, w, lambda k, j, msg, it=iter(cc): next(it))
        assert gc.const_transcript(p, w, n, v, cc) == out


def test_constants_are_the_headers():
    """kExtGpTailLog = 11, kBlock, kWave: the GPU file chooses its sizes by them"""
    def text(name):
        return open(os.path.join(ROOT, "thaler-study_amd", "csrc", name)).read()
    assert "constexpr int kExtGpTailLog = kGpTailLog - 1;" in text("kernels/ext_grand_product.hpp")
    assert gc.TAIL_LOG == int(re.search(r"constexpr int kGpTailLog = (\d+);", text("kernels/grand_product.hpp")).group(1)) - 1 == 11
    both = text("field.hpp") + text("kernels.hpp")
    assert re.search(r"constexpr int kBlock = %d;" % gc.BLOCK, both) and re.search(r"constexpr int kWave = %d;" % gc.WAVE, both)
