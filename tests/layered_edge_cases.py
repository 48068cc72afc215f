"""Inputs and references shared by tests/test_layered_edge_words_cpu.py and tests/test_gpu_layered_edge_words.py: the layered
sumcheck passes (gp_pass_kernel, fr_pass_kernel, zc_pass_kernel, sumprod_pass_kernel), their trees and the element-wise kernels
beside them on the words of tests/wide_words.py, for every modulus.  Nothing here imports the package or touches a GPU.

All tables and challenges are RAW (Montgomery) words; the big-integer references (grand_product_ref, logup_ref, r1cs_ref,
spark_ref, multiopen_ref) take canonical integers, converted with canon_list / mont_list.

  pass_inputs(p, n, count)        {name: (count tables of 2^n words, n challenge words)} for the names of INPUTS
  without_zeros, denominator_table   a table a product tree or a fraction sum can stand on, and the classes it still meets
  layer_draw(ch)                  the challenger of a layered proof (grand product, LogUp) over n challenge words
  *_reference(p, n, name, ..)     the reference transcript of one proof over one input, computed once and never changed
  run_indices(a)                  the run-shaped index list of spark_index_kernel with the places of its runs"""
import functools

import numpy as np

import grand_product_ref as gref
import logup_ref as lref
import multiopen_ref as mref
import r1cs_ref as rref
import spark_ref as sref
from util import GOLD
from wide_words import (WIDE, degenerate_challenges, edge_table, edge_words, octet_table, select_challenges, stride_classes)

MODULI = WIDE + [GOLD]
INPUTS = ("octet", "octet-odd", "edge", "pm1", "carry")
STRIDES = (1, 2, 4)

# constants of the kernel headers the GPU tests choose their sizes by (tests/test_layered_edge_words_cpu.py pins them)
GP_TAIL_LOG = 12         # kGpTailLog: the product tree's one-block tail
FR_TAIL_LOG = 11         # kFrTailLog: the fraction trees' one-block tail
LOOKUP_LDS_LOG = 13      # kLookupLdsLog: histograms of up to 2^13 counters are kept in LDS
EQ_SUM_LO_LOG = 7        # kEqSumLoLog: the low index bits of eq_sum_kernel
BLOCK = 256              # kBlock
WAVE = 64                # kWave

canon_list, mont_list = gref.canon_list, gref.mont_list


def _freeze(arrays):
    for t in arrays:
        t.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pass_inputs(p, n, count):
    """{name: (tables, challenges)}: `count` tables of 2^n raw words and n raw challenge words per name of INPUTS.
    octet: octet tables under the degenerate cycle - round 0 sees the stride-1 pairs, after r0 = 0 round 1 sees stride 2, after
    r1 = one round 2 sees stride 4.  octet-odd: fresh octet tables under select_challenges(p, 3) and then the degenerate cycle.
    edge: edge tables under challenges drawn from edge_words(p).  pm1: every word p - 1 under p - 1 - (j % 3).
    carry: carry_table under the field's one and then the degenerate cycle"""
    size = 1 << n
    out = {}
    for k, name in enumerate(INPUTS):
        rng = np.random.default_rng([p % 1000003, n, count, k])
        if name == "octet":
            tables, ch = [octet_table(p, size, rng) for _ in range(count)], degenerate_challenges(p, n)
        elif name == "octet-odd":
            tables = [octet_table(p, size, rng) for _ in range(count)]
            ch = (select_challenges(p, 3) + degenerate_challenges(p, max(n - 3, 0)))[:n]
        elif name == "edge":
            tables = [edge_table(p, size, rng) for _ in range(count)]
            e = edge_words(p)
            ch = [e[int(i)] for i in rng.integers(0, len(e), size=n)]
        elif name == "pm1":
            tables, ch = [np.full(size, p - 1, dtype=np.uint64) for _ in range(count)], [p - 1 - (j % 3) for j in range(n)]
        else:
            tables, ch = [carry_table(p, size, rng) for _ in range(count)], ([2**64 % p] + degenerate_challenges(p, n))[:n]
        out[name] = (_freeze(tables), [int(x) for x in ch])
    return out


def carry_table(p, size, rng, share=0.5):
    """`size` >= 4 raw words, none zero, in which about `share` of the aligned quads (every quad when there are fewer than four)
    are (u0, y, u2, a) with y < u0, y < 2^64 - p, u2 <= a < y.  A fold by the field's one hands on the odd entries as
    u0 + (y - u0 + p) = y + p, a sum inside [p, 2^64) that only the last correction of add brings below p, and u2 + (a - u2) = a,
    which needs none; the next round's difference a - y then borrows against that word.  A sum left unreduced is congruent
    to the right one, and products and lazy accumulators do not care: it is this borrow that turns it into a wrong value.
    The rest are uniform nonzero residues"""
    t = rng.integers(1, p, size=size, dtype=np.uint64)
    n_quads = size // 4
    built = range(n_quads) if n_quads < 4 else np.sort(rng.permutation(n_quads)[:max(1, int(round(n_quads * share)))])
    for k, q in enumerate(built):
        y = (3, 5, 58)[k % 3]
        a = int(rng.integers(1, y))
        u0 = (p - 1, y + 1, int(rng.integers(y + 1, p, dtype=np.uint64)))[(k // 3) % 3]
        t[4 * q:4 * q + 4] = (u0, y, int(rng.integers(1, a + 1)), a)
    return t


def carry_quads(p, t):
    """how many aligned quads of t are carry_table's"""
    q = [[int(x) for x in row] for row in np.asarray(t).reshape(-1, 4)]
    return sum(1 for u0, y, u2, a in q if y < u0 and y < 2**64 - p and y + p < 2**64 and 0 < u2 <= a < y)


def without_zeros(p, t):
    """a copy of t with its zero words replaced by p - 2: a zero makes a product 0 and most low layers of a tree all zero, and
    the fraction sum refuses a zero denominator root"""
    t = np.array(t, dtype=np.uint64)
    t[t == 0] = p - 2
    return t


def denominator_table(p, n, rng):
    """(an octet table of 2^n words without its zeros, {stride: the classes it still meets})"""
    t = without_zeros(p, octet_table(p, 1 << n, rng))
    return t, {s: stride_classes(p, t, s) for s in STRIDES}


def denominators_of(p, n, name):
    """the denominator table of an input: table 1 of pass_inputs(p, n, 2) without its zeros - for the octet inputs the table
    denominator_table builds"""
    return _freeze([without_zeros(p, pass_inputs(p, n, 2)[name][0][1])])[0]


def layer_draw(ch):
    """draw(layer, round, msg) of a layered proof over n challenge words: round j of every layer, its rho (j = layer) and the
    lambda of the next layer (j = layer + 1) take ch[j], so the top layers meet the challenges in the order pass_inputs means"""
    return lambda k, j, msg: ch[j]


# ---- the references, one per (modulus, size, input): computed once, shared, never changed -------------------------------

@functools.lru_cache(maxsize=None)
def p3_reference(p, n, name):
    """(three tables, challenges, (c1, rounds, challenges, finals) canonical)"""
    tabs, ch = pass_inputs(p, n, 3)[name]
    cc = canon_list(ch, p)
    return tabs, ch, sref.product3_prove(*[canon_list(t, p) for t in tabs], p, lambda j, msg: cc[j])


@functools.lru_cache(maxsize=None)
def zc_reference(p, n, name):
    """(three tables, tau, challenges, (c1, rounds, finals) canonical); tau is the degenerate cycle, except that where tau_j and
    r_j are 0 and one (either way round) tau_j is r_j: the fold by r_j would leave an eq table of zeros there, and every later
    round's values would be 0 whatever the kernel did"""
    tabs, ch = pass_inputs(p, n, 3)[name]
    one = 2**64 % p
    tau = [r if {t, r} == {0, one} else t for t, r in zip(degenerate_challenges(p, n), ch)]
    return tabs, tau, ch, rref.zerocheck(*[canon_list(t, p) for t in tabs], canon_list(tau, p), canon_list(ch, p), p)


@functools.lru_cache(maxsize=None)
def sp_reference(p, n, name, T):
    """(a tables, b tables, challenges, (rounds, challenges, finals_a, finals_b) canonical).  With T = 3 pair 2 reads pair 1's b
    table as its a table and pair 0's a table as its b table: one table in several pairs"""
    tabs, ch = pass_inputs(p, n, 16)[name]
    a, b = list(tabs[:T]), list(tabs[8:8 + T])
    if T == 3:
        a[2], b[2] = b[1], a[0]
    cc = canon_list(ch, p)
    return a, b, ch, mref.sumcheck([canon_list(t, p) for t in a], [canon_list(t, p) for t in b], p, lambda j, msg: cc[j])


@functools.lru_cache(maxsize=None)
def gp_reference(p, n, name):
    """(table, challenges, the reference's tree layers, its proof dict (canonical)): the table is denominators_of"""
    _, ch = pass_inputs(p, n, 2)[name]
    t = denominators_of(p, n, name)
    tc = canon_list(t, p)
    layers = gref.tree(tc, p)
    return t, ch, layers, gref.prove(tc, p, layer_draw(canon_list(ch, p)), layers=layers)


@functools.lru_cache(maxsize=None)
def fr_reference(p, n, name, ones):
    """(numerator table or None, denominator table, challenges, the reference's (P, Q) layers, its proof dict (canonical)): the
    numerator is table 0 of the input with its zeros, the denominator is denominators_of"""
    tabs, ch = pass_inputs(p, n, 2)[name]
    pt, qt = (None if ones else tabs[0]), denominators_of(p, n, name)
    pc, qc = (None if ones else canon_list(pt, p)), canon_list(qt, p)
    layers = lref.tree(pc, qc, p)
    return pt, qt, ch, layers, lref.prove(pc, qc, p, layer_draw(canon_list(ch, p)), layers=layers)


# ---- the launches a proof leaves in the log ------------------------------------------------------------------------------

def pass_log(n, host_log):
    """[(kf, log_in)] of the launches of one sumcheck (sc_product3_prove, sc_sumprod_prove) over tables of 2^n entries: none when
    the tables have at most 2^host_log entries, else the rounds down to tables of 2^max(host_log, 1) entries"""
    te = n if n <= host_log else max(host_log, 1)
    return [(0, n)] + [(1, n - j + 1) for j in range(1, n - te + 1)] if n > te else []


def layered_log(n, host_log):
    """[(kf, log_in)] of the launches of a layered proof over a table of 2^n entries: the layers <= host_log leave none, every
    other layer k its round 0 and the folds down to tables of 2^max(host_log, 1) entries"""
    te = max(host_log, 1)
    out = []
    for k in range(host_log + 1, n):
        out += [(0, k)] + [(1, k - j + 1) for j in range(1, k - te + 1)]
    return out


def zerocheck_log(n):
    """[(kf, log_in)] of sc_zerocheck_prove: every round is a launch"""
    return [(0, n)] + [(1, n - j + 1) for j in range(1, n)]


# ---- run-shaped index lists for spark_index_kernel -----------------------------------------------------------------------

SPARK_L = 13
SPARK_NNZ = (1 << SPARK_L) - 259          # no multiple of 4 or of 256; padded with zeros to 2^13


def run_indices(a, nnz=SPARK_NNZ):
    """(nnz indices below 2^a, a >= 3, {run: (first, end)}).  A thread of spark_index_kernel owns four consecutive entries, a
    wave 256.  In order:
      run     one index (2^a - 1, the largest) over [2, 1027): it starts and ends off a 4-boundary and covers the waves 1, 2, 3
      four    [1028, 1032): exactly four equal indices in one thread; the threads before and after hold other indices
      threes  [1032, 1096): sixteen threads with three equal indices and one different, the odd one in every place
      uniform [1096, nnz): uniform indices
    and behind them the zero padding up to the next power of two"""
    M = 1 << a
    rng = np.random.default_rng([a, nnz])
    idx = rng.integers(0, M, size=nnz)
    idx[0], idx[1] = 1, 2
    idx[2:1027] = M - 1
    idx[1027] = M - 2
    idx[1028:1032] = 3
    for k in range(16):
        base = 1032 + 4 * k
        idx[base:base + 4] = 4 + k % (M - 5)
        idx[base + k % 4] = 5 + k % (M - 5)
    return idx.astype(np.int64), {"run": (2, 1027), "four": (1028, 1032), "threes": (1032, 1096), "uniform": (1096, nnz)}


def small_run_indices(a):
    """two lists shorter than a wave's 256 entries, so that the loop runs with a part of one wave active: 61 copies of index 0
    (with the padding every active thread holds four zeros: one add for the wave) and 61 copies of 2^a - 1 (the last active
    thread holds one of them and three zeros of the padding)"""
    return [np.zeros(61, dtype=np.int64), np.full(61, (1 << a) - 1, dtype=np.int64)]
