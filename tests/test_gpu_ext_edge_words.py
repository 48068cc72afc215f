"""GPU: the extension-field sumcheck (ext_sumprod_pass_kernel<F, T, BASE_IN>, ext_fold_kernel<F, BASE_IN> and their host twins
ext_host_rounds, ext_host_evaluate, reached through sc_sumprod_prove_ext and sc_table_evaluate_ext) on worst-case words in BOTH
planes, for every kind of field and with few blocks.

tests/test_gpu_ext_sumcheck.py feeds octet tables as base tables: the first fold mixes them with the challenge, so the c1 plane,
the operand sums x0 + x1, y0 + y1 of the Karatsuba products (ext_accumulate, ext_mul) and the per-component a(2) = a1 + (a1 - a0)
only ever saw arbitrary words there, on four moduli, under canonical challenges.  The inputs here are tests/ext_edge_cases.py's: a
base table folded by X = (0, one) is c0[i] = u[2 i], c1[i] = u[2 i + 1] - u[2 i], so inject() puts chosen words into both planes of
the launch of round 1 - octet tables per plane, cross tables whose entries and whose differences carry the corners of
wide_words.classes_of ACROSS the two components (a sum of two components above 2^64 exists for p > 2^63), carry tables per plane
(a fold by one leaves a word that needed the last correction of add, and the next round borrows against it: an unreduced sum is
congruent to the right one and shows only through that borrow), constant planes whose transcript is a closed form up to 8192
products per lazy accumulator - under challenges whose components are raw corner words.  tests/test_ext_edge_words_cpu.py checks
that coverage, and the reference, without a GPU.  The moduli are the six of wide_words.WIDE + [GOLD].

Every check is bit for bit against tests/ext_ref.py or the closed form; there is no tolerance anywhere."""
import numpy as np
import pytest

import ext_edge_cases as ec
import ext_ref as ref
import test_gpu_ext_sumcheck as base
from ext_edge_cases import MODULI
from test_gpu_ext_sumcheck import XS, ctx_of, device, host_log, records, upload, w_of, want_log, want_of
from util import GOLD
from wide_words import wid

pytestmark = pytest.mark.gpu

T = 3
SIZES = (4, 11)                     # every round in ext_host_rounds at the default hand-over; the injected launch as the last one
FEW_N = 13
FEW_NAMES = ("planes", "carry-base", "carry-planes")
MANY_T = 8
DEEP_N = 20                         # one block, T = 8: 2^18 units / 256 threads * 8 = 8192 products per accumulator in round 1
EVAL_NAMES = ("planes", "planes-deep-even", "planes-deep-odd", "late-x", "carry-base", "carry-planes", "edge")


def teardown_module(module):
    base.teardown_module(module)


def closed_form(p, n, count, name):
    """const_transcript in words, with the challenges of the input in their place"""
    e = ec.canon_list([ec.const_word(p, name)] * 2, p)
    c1, rounds, fa, fb = ec.const_transcript(p, ref.nonresidue(p), n, count, e)
    cc = ec.canon_pairs(ec.const_input(p, n, count, name)[2], p)
    return want_of(p, (c1, rounds, cc, fa, fb))


CASES = [(p, n, name) for p in MODULI for n in SIZES for name in ec.names_of(p)]


@pytest.mark.parametrize("p,n,name", CASES, ids=["%s-%d-%s" % (wid(p), n, name) for p, n, name in CASES])
def test_transcript_is_the_reference_bit_for_bit(pkg, p, n, name):
    """gp_host_log = 0 (every round but the last on the device) and the default (n = 4: every round in ext_host_rounds, from base
    words; n = 11: the launch of round 1, which the planes are injected into, is the last one and ext_host_rounds goes on from
    what it wrote).  c1, all 6 n values, the challenges and the 2 * 2 T finals; the same transcript at both"""
    a, b, cc, out = ec.ext_reference(p, n, T, name)
    want = want_of(p, out)
    assert want[2] == ec.ext_inputs(p, n, T)[name][2], "the challenges go in as the raw words the input names"
    if name.startswith("const"):
        assert want == closed_form(p, n, T, name)
    outs = [device(pkg, p, a, b, cc, H) for H in sorted({0, host_log(pkg, p)})]
    assert len(outs) == 2
    for got in outs:
        assert got == want
    assert outs[0] == outs[1], "transcripts at different gp_host_log are identical"


FEW = [(p, name) for p in MODULI for name in FEW_NAMES]


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("p,name", FEW, ids=["%s-%s" % (wid(p), name) for p, name in FEW])
def test_few_blocks(pkg, p, name, blocks):
    """n = 13, every round on the device: with max_blocks = 3 threads take uneven numbers of trips through the grid-stride loop
    and finish_pass hands off across three blocks, with max_blocks = 1 one block does everything"""
    a, b, cc, out = ec.ext_reference(p, FEW_N, T, name)
    log = []
    assert device(pkg, p, a, b, cc, 0, blocks, log) == want_of(p, out)
    assert records(log) == want_log(FEW_N, T, 1)


MANY = [(p, name) for p in MODULI for name in ec.names_of(p) if name.startswith("const")]


@pytest.mark.parametrize("p,name", MANY, ids=["%s-%s" % (wid(p), name) for p, name in MANY])
def test_constant_planes_64_products_per_accumulator(pkg, p, name):
    """n = 13, T = 8, one block: a thread takes 8 trips of 8 pairs in the launch of round 1 and adds 64 products of (p - 1)^2
    and of (p - 2)^2 (const-down: of a multiple of 2^96) to its accumulators; against the closed form, every round on the device"""
    a, b, ch = ec.const_input(p, FEW_N, MANY_T, name)
    log = []
    assert device(pkg, p, a, b, ec.canon_pairs(ch, p), 0, 1, log) == closed_form(p, FEW_N, MANY_T, name)
    assert records(log) == want_log(FEW_N, MANY_T, 1)


@pytest.mark.parametrize("p", [GOLD, 2**64 - 59], ids=wid)
def test_constant_planes_8192_products_per_accumulator(pkg, p):
    """n = 20, T = 8, one block, one shared table of 8 MiB: 8192 products per accumulator in the launch of round 1, 4096 in the
    next, ... - the only case above n = 13; against the closed form"""
    a, b, ch = ec.const_input(p, DEEP_N, MANY_T, "const")
    assert device(pkg, p, a, b, ec.canon_pairs(ch, p), 0, 1) == closed_form(p, DEEP_N, MANY_T, "const")


EVAL = [(p, n, name) for p in MODULI for n in SIZES + (FEW_N,) for name in EVAL_NAMES]


@pytest.mark.parametrize("p,n,name", EVAL, ids=["%s-%d-%s" % (wid(p), n, name) for p, n, name in EVAL])
def test_table_evaluate_ext_at_the_inputs_own_challenges(pkg, p, n, name):
    """ext_fold_kernel and ext_host_evaluate over the a tables of pairs 0 and 1 (planes: octet planes and a cross table) at the
    input's challenges as the point, at both hand-overs.  The fold-only launches take their grid from strided_grid, which does
    not read max_blocks: the value with max_blocks = 1 set pins that it does not depend on it"""
    a, _, ch = ec.ext_inputs(p, n, T)[name]
    ctx = ctx_of(pkg, p)
    default, blocks = host_log(pkg, p), ctx.get_option("max_blocks")
    for table in a[:2]:
        want = tuple(ec.mont_list(ref.mle_eval(ec.canon_list(table, p), ec.canon_pairs(ch, p), p, ref.nonresidue(p)), p))
        t = upload(pkg, ctx, table)
        try:
            for H in (0, default):
                for mb in (blocks, 1):
                    ctx.set_option("gp_host_log", H)
                    ctx.set_option("max_blocks", mb)
                    assert XS.table_evaluate_ext(ctx, w_of(p), t, ch) == want, (H, mb)
        finally:
            ctx.set_option("gp_host_log", default)
            ctx.set_option("max_blocks", blocks)
        assert np.array_equal(t.to_evaluations(), table), "the input is never written"
