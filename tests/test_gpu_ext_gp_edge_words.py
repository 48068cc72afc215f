"""GPU: the grand product over K = F_p[X] / (X^2 - w) (ext_gp_tree_kernel<F, LV, LEAF_IN>, ext_gp_tree_tail_kernel<F, LEAF_IN>,
ext_gp_pass_kernel<F, FOLD, LEAF_IN>, ext_eq_table_kernel and the host finish, reached through sc_gp_create_ext and sc_gp_prove_ext)
on worst-case words in BOTH planes, for every kind of field and with few blocks.

tests/test_gpu_ext_grand_product.py draws alpha and beta from {0, 1, p - 1, random} on four moduli, so the c1 plane of the leaves and
both planes of every tree layer only ever held arbitrary words there.  The inputs here are tests/ext_gp_edge_cases.py's: leaf maps
alpha = (one, +-one), beta = (0, d) that put an octet table itself into a plane of the leaves, tables whose upper part is constant
under beta = 1 - alpha c so that chosen words land in one plane of layer n - 1, n - 2 or n - 3, one small proof per pair of
wide_words.diff_classes with that pair as an ENTRY of a tree layer, carry tables (a fold by one leaves a word that needed the last
correction of add, and the next round borrows against it), edge words everywhere, and a constant table whose transcript is a closed
form.  tests/test_ext_gp_edge_words_cpu.py checks that coverage, and the reference, without a GPU.  The moduli are the six of
wide_words.WIDE + [GOLD].

Every check is bit for bit against tests/ext_gp_ref.py or the closed form; there is no tolerance anywhere."""
import gc as pygc

import numpy as np
import pytest

import ext_gp_edge_cases as gc
import ext_ref as xref
import test_gpu_ext_grand_product as base
from ext_gp_edge_cases import MODULI
from test_gpu_ext_grand_product import XG, ctx_of, device, host_log, m2, plane, pool, records, upload, w_of, want_log, want_of, want_tree_log
from util import GOLD
from wide_words import wid

pytestmark = pytest.mark.gpu

SMALL_N = 4
FEW_N = 13
FEW_MODULI = (GOLD, 2**64 - 59, 2**63 + 29, 2**32 - 5)
DEEP_N = 20                         # one block: 2^18 units / 256 threads = 1024 products per accumulator in round 0 of layer 19


def teardown_module(module):
    base.teardown_module(module)


def large_n(name):
    """2^11 chosen words in the targeted layer: n = 12 for the leaves and layer n - 1, n = 13 for layer n - 2"""
    return 13 if name.startswith("planes2") else 12


def proof_of(pkg, p, r, H, blocks=None, log=None):
    """one proof over a reference's input; the input table is unchanged (device() checks it) and the pool's books balance"""
    ctx = ctx_of(pkg, p)
    before = pool(ctx)
    got = device(pkg, p, r.input.table, r.alpha, r.beta, r.challenges, H, blocks, log)
    if pool(ctx) != before:
        pygc.collect()          # (only where something is still waiting for the collector: a collection costs more than a small proof)
    assert pool(ctx) == before, "the pool's books balance after a proof"
    return got


def check_transcript(pkg, p, r):
    n = len(r.input.table).bit_length() - 1
    want = want_of(p, r.out)
    assert want.challenges == r.input.challenges and (m2(p, r.alpha), m2(p, r.beta)) == (r.input.alpha, r.input.beta), "raw words go in as named"
    outs = []
    for H in sorted({0, host_log(pkg, p)}):
        log = []
        outs.append(proof_of(pkg, p, r, H, None, log))
        assert outs[-1] == want, H
        assert records(log) == want_log(n, max(H, 1), H), H
    assert len(outs) == 2 and outs[0] == outs[1], "transcripts at different gp_host_log are identical"


CASES = [(p, n, name) for p in MODULI for name in gc.names_of(p) for n in (SMALL_N, large_n(name))]


@pytest.mark.parametrize("p,n,name", CASES, ids=["%s-%d-%s" % (wid(p), n, name) for p, n, name in CASES])
def test_transcript_is_the_reference_bit_for_bit(pkg, p, n, name):
    """gp_host_log = 0 (every layer and every round but the last on the device) and the default: product, every round's eight words,
    the finals, the point and the claim; the launches are the byte model's"""
    r = gc.gp_reference(p, n, name)
    if name == "const":
        leaf = tuple(gc.canon_list((p - 1, p - 1), p))
        assert r.out == gc.const_transcript(p, xref.nonresidue(p), n, leaf, r.challenges)
    check_transcript(pkg, p, r)


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_every_pair_as_an_entry_of_a_tree_layer(pkg, p):
    """planes-entry: one proof at n = 5 per pair (lo, hi) of diff_classes(p) but the zero of K, layer 4 holding the pair as an entry:
    the operand sums of ext_mul in the tree's tail and in the accumulate of layer 3 add lo + hi"""
    for r in gc.entry_references(p):
        check_transcript(pkg, p, r)


LEAF_NAMES = ("leaf-c1", "leaf-perm", "leaf-deep-even", "leaf-deep-odd", "leaf-carry")      # and every leaf-entry-* of the modulus
TREES = [(p, n, lv, name) for p in MODULI for name in gc.leaf_entry_names(p) + LEAF_NAMES for n in (12, 13, 14) for lv in (1, 2, 3)]
TREES += [(p, n, lv, "planes%s-%s" % (d, c)) for p in MODULI for n, lv, d in ((13, 1, ""), (15, 2, "2"), (17, 3, "3")) for c in ("c0", "c1")]


@pytest.mark.parametrize("p,n,lv,name", TREES, ids=["%s-%d-lv%d-%s" % (wid(p), n, lv, name) for p, n, lv, name in TREES])
def test_tree_product_and_every_layer(pkg, p, n, lv, name):
    """every leaf input (each has its own table and leaf map) at n = 12 .. 14 under gp_tree_lv = 1 .. 3: ext_gp_tree_kernel<LV,
    leaves in> at every LV over chosen leaves - the whole set of leaf-entry-* maps, the shifted octets, the carry words.
    planes-c* at n = 13, lv 1; planes2-c* at n = 15, lv 2; planes3-c* (the upper seven eighths constant) at n = 17, lv 3: the launch
    with planes in reads the layer - 12, 13, 14 - that holds the chosen words, at every LV, and the tail reads their products.  Both
    planes of every layer, the product and the launches"""
    ctx = ctx_of(pkg, p)
    inp, alpha, beta, layers = gc.tree_reference(p, n, name)
    table = upload(pkg, ctx, inp.table)
    base_lv = ctx.get_option("gp_tree_lv")
    ctx.set_option("gp_tree_lv", lv)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    try:
        tree = XG.ExtProductTree(ctx, w_of(p), table, inp.alpha, inp.beta)
        log = ctx.launch_log()
    finally:
        ctx.set_option("gp_tree_lv", base_lv)
        ctx.set_option("time_kernels", 0)
    assert records(log) == want_tree_log(n, lv)
    assert tree.num_vars == n and tree.product == m2(p, layers[0][0]) != (0, 0)
    for k in range(n):
        c0, c1 = tree.layer(k)
        for c, got in enumerate((c0.to_evaluations(), c1.to_evaluations())):
            assert got.shape == (1 << k,) and np.array_equal(got, plane(p, layers[k], c)), (n, k, c)
    assert np.array_equal(table.to_evaluations(), inp.table), "the input table is unchanged"
    tree.close()


FEW = [(p, name) for p in FEW_MODULI for name in ("leaf-entry-0", "leaf-carry", "planes-c1", "edge")]


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("p,name", FEW, ids=["%s-%s" % (wid(p), name) for p, name in FEW])
def test_few_blocks(pkg, p, name, blocks):
    """n = 13, every round on the device: with max_blocks = 3 threads take uneven numbers of trips through the grid-stride loops and
    finish_pass hands off across three blocks, with max_blocks = 1 one block does everything (the tree too)"""
    r = gc.gp_reference(p, FEW_N, name)
    log = []
    assert proof_of(pkg, p, r, 0, blocks, log) == want_of(p, r.out)
    assert records(log) == want_log(FEW_N, 1, 0)


def closed_form(p, n):
    """(the constant input's reference record without a reference run, the closed form in words)"""
    r = gc._reference(p, gc.const_input(p, n), prove=False)
    leaf = tuple(gc.canon_list((p - 1, p - 1), p))
    return r, want_of(p, gc.const_transcript(p, xref.nonresidue(p), n, leaf, r.challenges))


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_constant_planes_against_the_closed_form(pkg, p):
    """n = 13, p - 1 in both planes of every leaf, with every block and with one: against the closed form, every round on the device"""
    r, want = closed_form(p, FEW_N)
    for blocks in (None, 1):
        assert proof_of(pkg, p, r, 0, blocks) == want, blocks


@pytest.mark.parametrize("p", [GOLD, 2**64 - 59], ids=wid)
def test_constant_planes_1024_products_per_accumulator(pkg, p):
    """n = 20, one block, one table of 8 MiB: 1024 products per lazy accumulator in round 0 of layer 19, 512 in layer 18, ... - the
    only proof above n = 13; the closed form needs no reference over 2^20 entries"""
    r, want = closed_form(p, DEEP_N)
    assert proof_of(pkg, p, r, 0, 1) == want
