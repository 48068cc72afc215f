"""GPU: the layered sumcheck passes (gp_pass_kernel under sc_gp_prove and sc_product3_prove, fr_pass_kernel with a general and an
all-ones numerator, zc_pass_kernel, sumprod_pass_kernel<T>), their trees and the element-wise kernels beside them (table_affine,
spark_tuple, eq_sum, spark_index, spark_gather) on worst-case words, for every kind of field and with few blocks.

These kernels take sub(e[1], e[0]) of neighbouring entries and extend by repeated adds (gp_accumulate, zc_accumulate,
fr_accumulate), form u0 + r (u1 - u0) and difference the folded entries (zc_fold4), or a1 + (a1 - a0) (sp_accumulate); the
correcting branches of the device's sub, add, acc_mac depend on where such a difference or sum lands, and on uniform words they
fire about once in 2^32.  The inputs are tests/layered_edge_cases.py's: wide_words.octet_table, whose differences and sums at
strides 1, 2, 4 sit on every corner of wide_words.classes_of, under challenges that are 0 or the field's one, so the patterns
survive the folds (tests/test_layered_edge_words_cpu.py checks that coverage, and the references, without a GPU); edge tables
under edge challenges; all p - 1; and carry_table, on which a fold by the field's one leaves sums inside [p, 2^64) that the next
round's difference borrows against - a sum that add leaves unreduced is congruent to the right one and passes through products
and lazy accumulators unseen, so on the octet tables a whole transcript stays right under such a build; it is the borrow that
turns it into a wrong value.  The moduli are the six of wide_words.WIDE + [GOLD].

Every check is bit for bit against the big-integer references; there is no tolerance anywhere.

What max_blocks reaches.  The passes and the trees size their grids by it: at n = 13 with max_blocks = 3 a round of 2^12 units
is 3 blocks of 256 threads, so threads take 6 or 5 trips through the grid-stride loop and finish_pass hands off across three
blocks; with max_blocks = 1 one block takes 16 trips and there is no hand-off.  eq_sum_kernel, spark_index_kernel,
spark_gather_kernel, spark_tuple_kernel and table_affine_kernel take their grid from strided_grid (8 blocks per CU at most; the
LDS histogram of spark_index_kernel from the list's length alone) and do not read max_blocks: their tests set it as well, which
pins that their result does not depend on it, and reach several trips per thread by their sizes instead - spark_index_kernel with
LDS histograms walks a list of 2^13 in one block, eight trips per thread."""
import contextlib

import numpy as np
import pytest

import grand_product_ref as gref
import layered_edge_cases as lc
import logup_cases
import logup_ref as lref
import spark_ref as sref
import wide_words as ww
from layered_edge_cases import INPUTS, MODULI, canon_list, mont_list
from ligero_common import context_cache, mont_np
from test_gpu_multiopen import eq_sum_ref
from util import GOLD
from wide_words import wid

pytestmark = pytest.mark.gpu

ctx_of, teardown_module = context_cache()

SIZES = (3, 11)                     # one octet (the two-unit fold launch); the size whose octet tables meet every class
FEW_N = 13                          # 2^12 units in round 0: sixteen blocks' worth
FEW_MODULI = [GOLD, 2**64 - 59, 2**32 + 15]
FEW_BLOCKS = (1, 3)


@contextlib.contextmanager
def options(ctx, **opts):
    """the options set for the body and put back whatever happens"""
    old = {k: ctx.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def logged(ctx, kind, fn):
    """(fn(), [(kf, log_in, ks)] of the launches of `kind` it made)"""
    with options(ctx, time_kernels=1):
        ctx.launch_log()
        out = fn()
        log = [(x["kf"], x["log_in"], x["ks"]) for x in ctx.launch_log() if x["kind"] == kind]
    return out, log


def upload(pkg, ctx, t):
    return pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, len(t).bit_length() - 1, np.ascontiguousarray(t, dtype=np.uint64))


def uploaded(pkg, ctx, tables):
    """{id(array): device table}: tables that are one array are one device table"""
    dev = {}
    for t in tables:
        if id(t) not in dev:
            dev[id(t)] = upload(pkg, ctx, t)
    return dev


def unchanged(dev, tables):
    for t in tables:
        assert np.array_equal(dev[id(t)].to_evaluations(), t), "the inputs are never written"


# ---- the five proofs: run(pkg, p, n, name, variant) -> (device transcript, reference transcript in words) ----------------
# variant: T of the sum of products, ones of the fraction sum, None for the rest

def run_product3(pkg, p, n, name, _):
    ctx = ctx_of(pkg, p)
    tabs, ch, (c1, rounds, rs, finals) = lc.p3_reference(p, n, name)
    want = (gref.mont(c1, p), [mont_list(m, p) for m in rounds], mont_list(rs, p), tuple(mont_list(finals, p)))
    assert want[2] == ch
    dev = uploaded(pkg, ctx, tabs)
    got = pkg.spark.product3_prove(ctx, *[dev[id(t)] for t in tabs], lambda j, msg: ch[j])
    unchanged(dev, tabs)
    return got, want


def run_zerocheck(pkg, p, n, name, _):
    ctx = ctx_of(pkg, p)
    tabs, tau, ch, (c1, rounds, finals) = lc.zc_reference(p, n, name)
    want = (gref.mont(c1, p), [mont_list(m, p) for m in rounds], ch, tuple(mont_list(finals, p)))
    dev = uploaded(pkg, ctx, tabs)
    got = pkg.r1cs.zerocheck_prove(ctx, *[dev[id(t)] for t in tabs], tau, lambda j, e: ch[j])
    unchanged(dev, tabs)
    return got, want


def run_sumprod(pkg, p, n, name, T):
    ctx = ctx_of(pkg, p)
    a, b, ch, (rounds, rs, fa, fb) = lc.sp_reference(p, n, name, T)
    c1 = (rounds[0][0] + rounds[0][1]) % p
    want = (gref.mont(c1, p), [mont_list(m, p) for m in rounds], mont_list(rs, p), mont_list(fa, p), mont_list(fb, p))
    assert want[2] == ch
    dev = uploaded(pkg, ctx, a + b)
    assert len(dev) == (2 * T if T != 3 else 4)
    got = pkg.multiopen.sumprod_prove(ctx, [dev[id(t)] for t in a], [dev[id(t)] for t in b], lambda j, msg: ch[j])
    unchanged(dev, a + b)
    return got, want


def run_logup(pkg, p, n, name, ones):
    ctx = ctx_of(pkg, p)
    pt, qt, ch, _, proof = lc.fr_reference(p, n, name, ones)
    want = logup_cases.as_proof(pkg, proof, p)
    q = upload(pkg, ctx, qt)
    p_table = None if ones else upload(pkg, ctx, pt)
    tree = pkg.logup.FractionTree(ctx, q, p_table)
    try:
        got = pkg.logup.prove(tree, lc.layer_draw(ch))
    finally:
        tree.close()
    assert np.array_equal(q.to_evaluations(), qt) and (ones or np.array_equal(p_table.to_evaluations(), pt)), "the inputs are never written"
    return got, want


def run_grand_product(pkg, p, n, name, _):
    ctx = ctx_of(pkg, p)
    t, ch, _, proof = lc.gp_reference(p, n, name)
    m = lambda xs: mont_list(xs, p)   # noqa: E731
    want = pkg.grand_product.Proof(gref.mont(proof["product"], p), [[m(msg) for msg in layer] for layer in proof["rounds"]],
                                   [tuple(m(f)) for f in proof["finals"]], m(proof["point"]), gref.mont(proof["claim"], p), m(proof["challenges"]))
    assert want.product != 0, "the lower layers are not all zero"
    table = upload(pkg, ctx, t)
    tree = pkg.grand_product.ProductTree(ctx, table)
    try:
        got = pkg.grand_product.prove(tree, lc.layer_draw(ch))
    finally:
        tree.close()
    assert np.array_equal(table.to_evaluations(), t), "the input is never written"
    return got, want


def fraction_log(n, host_log, ones):
    """layered_log with the tables a launch reads: three in the top layer of an all-ones numerator, five everywhere else"""
    out, te = [], max(host_log, 1)
    for k in range(host_log + 1, n):
        nt = 3 if ones and k == n - 1 else 5
        out += [(0, k, nt)] + [(1, k - j + 1, nt) for j in range(1, k - te + 1)]
    return out


# family: (run, the option of its hand-over to the host or None, launch kind, log(n, host_log, variant) -> [(kf, log_in, ks)])
FAMILIES = {
    "product3": (run_product3, "gp_host_log", "product_pass", lambda n, H, v: [(kf, m, 1) for kf, m in lc.pass_log(n, H)]),
    "zerocheck": (run_zerocheck, None, "zerocheck", lambda n, H, v: [(kf, m, 1) for kf, m in lc.zerocheck_log(n)]),
    "sumprod": (run_sumprod, "gp_host_log", "sumprod_pass", lambda n, H, T: [(kf, m, T) for kf, m in lc.pass_log(n, H)]),
    "logup": (run_logup, "fr_host_log", "fraction_pass", fraction_log),
    "grand_product": (run_grand_product, "gp_host_log", "product_pass", lambda n, H, v: [(kf, m, 1) for kf, m in lc.layered_log(n, H)]),
}
# (family, variant, id): both numerator modes of fr_pass_kernel, T = 1, 3, 8 of sumprod_pass_kernel
VARIANTS = [("product3", None, "product3"), ("zerocheck", None, "zerocheck"), ("sumprod", 1, "sumprod-T1"), ("sumprod", 3, "sumprod-T3"),
            ("sumprod", 8, "sumprod-T8"), ("logup", True, "logup-ones"), ("logup", False, "logup-general"), ("grand_product", None, "grand_product")]
VARIANT_IDS = [v[2] for v in VARIANTS]


def first_difference(got, want):
    """where two transcripts part, for the message of a failure"""
    if isinstance(want, (list, tuple)) and isinstance(got, (list, tuple)) and len(got) == len(want):
        for k, (g, w) in enumerate(zip(got, want)):
            if g != w:
                return (k,) + first_difference(g, w)
    return ()


# ---- a. the passes, every modulus ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family,variant,vid", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_pass_is_the_reference_on_edge_words(pkg, p, family, variant, vid, n, name):
    """the hand-over to the host at 0 (every round the device can run is a launch) and at the context's default: each transcript
    is the reference's, and the two are one.  sc_zerocheck_prove has no hand-over: every round is a launch"""
    run, option, kind, log_of = FAMILIES[family]
    ctx = ctx_of(pkg, p)
    outs = []
    for H in ((0, ctx.get_option(option)) if option else (None,)):
        with options(ctx, **({option: H} if option else {})):
            (got, want), log = logged(ctx, kind, lambda: run(pkg, p, n, name, variant))
        assert got == want, (wid(p), vid, n, name, H, first_difference(got, want))
        assert log == log_of(n, H or 0, variant), (vid, n, H, log)
        outs.append(got)
    assert all(o == outs[0] for o in outs[1:]), "transcripts at different hand-overs are identical"


# ---- b. few blocks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("family,variant,vid", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("p", FEW_MODULI, ids=wid)
def test_pass_with_few_blocks(pkg, p, family, variant, vid, name):
    """n = 13, every round on the device: with max_blocks = 3 threads take uneven numbers of trips through the grid-stride loop
    and finish_pass hands off across three blocks, with max_blocks = 1 one block does everything.  Each transcript is the
    reference's and the one at the default max_blocks, and the launches of the family are in the log"""
    run, option, kind, log_of = FAMILIES[family]
    ctx = ctx_of(pkg, p)
    host = {option: 0} if option else {}
    want_log = log_of(FEW_N, 0, variant)
    assert len(want_log) >= FEW_N - 1 and max(m for _, m, _ in want_log) >= FEW_N - 1, "every round of the largest tables is a launch"
    with options(ctx, **host):
        (base, want), log = logged(ctx, kind, lambda: run(pkg, p, FEW_N, name, variant))
    assert base == want, (wid(p), vid, name, "default", first_difference(base, want))
    assert log == want_log
    for blocks in FEW_BLOCKS:
        with options(ctx, max_blocks=blocks, **host):
            assert ctx.get_option("max_blocks") == blocks
            (got, _), log = logged(ctx, kind, lambda: run(pkg, p, FEW_N, name, variant))
        assert got == want, (wid(p), vid, name, blocks, first_difference(got, want))
        assert got == base and log == want_log, (vid, blocks, log)


# ---- c. the trees ----------------------------------------------------------------------------------------------------------

_TREES = {}


def tree_tables(p, source):
    """(numerator words, denominator words, product-tree layers, fraction-tree layers with and without the numerator): computed
    once, shared, never changed.  edge: the product tree keeps the zeros of its edge table, the denominators lose them"""
    key = (p, source)
    if key not in _TREES:
        rng = np.random.default_rng([p % 1000003, FEW_N, len(source)])
        if source == "edge":
            num, gp_t = ww.edge_table(p, 1 << FEW_N, rng), ww.edge_table(p, 1 << FEW_N, rng)
            den = lc.without_zeros(p, gp_t)
        else:
            num = ww.octet_table(p, 1 << FEW_N, rng)
            den, _ = lc.denominator_table(p, FEW_N, rng)
            gp_t = den
        nc, dc = canon_list(num, p), canon_list(den, p)
        for t in (num, den, gp_t):
            t.setflags(write=False)
        _TREES[key] = (num, den, gp_t, gref.tree(canon_list(gp_t, p), p), {True: lref.tree(None, dc, p), False: lref.tree(nc, dc, p)})
    return _TREES[key]


def fraction_tree_schedule(n, lv):
    out, m = [], n
    while m > lc.FR_TAIL_LOG:
        step = min(lv, m - lc.FR_TAIL_LOG)
        out.append((step, m))
        m -= step
    return out + [(0, m)]


@pytest.mark.parametrize("blocks", [3, None], ids=["3-blocks", "default"])
@pytest.mark.parametrize("source", ["edge", "denominator"])
@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_trees_root_and_every_layer(pkg, p, source, blocks):
    """n = 13: the tail kernel and the launches above it (one of gp_tree_kernel; fr_tree_kernel by the default fr_tree_lv), with
    three blocks several trips per thread"""
    ctx = ctx_of(pkg, p)
    n = FEW_N
    assert pkg.grand_product.TAIL_LOG == lc.GP_TAIL_LOG < n and pkg.logup.TAIL_LOG == lc.FR_TAIL_LOG < n
    num, den, gp_t, gp_layers, fr_layers = tree_tables(p, source)
    with options(ctx, **({"max_blocks": blocks} if blocks else {})):
        table = upload(pkg, ctx, gp_t)
        tree, log = logged(ctx, "product_tree", lambda: pkg.grand_product.ProductTree(ctx, table))
        try:
            assert [(kf, m) for kf, m, _ in log] == [(1, 13), (0, 12)]
            assert tree.num_vars == n and tree.product == gref.mont(gp_layers[0][0], p)
            for k in range(n):
                assert np.array_equal(tree.layer(k).to_evaluations(), mont_np(p, gp_layers[k])), ("product tree", k)
        finally:
            tree.close()
        assert np.array_equal(table.to_evaluations(), gp_t)
        q = upload(pkg, ctx, den)
        for ones in (True, False):
            P, Q = fr_layers[ones]
            p_table = None if ones else upload(pkg, ctx, num)
            tree, log = logged(ctx, "fraction_tree", lambda: pkg.logup.FractionTree(ctx, q, p_table))
            try:
                assert [(kf, m) for kf, m, _ in log] == fraction_tree_schedule(n, ctx.get_option("fr_tree_lv"))
                assert tree.root == (gref.mont(P[0][0], p), gref.mont(Q[0][0], p)) and Q[0][0] != 0
                for k in range(n):
                    for which, layer in ((0, P[k]), (1, Q[k])):
                        assert np.array_equal(tree.layer(k, which).to_evaluations(), mont_np(p, layer)), ("fraction tree", ones, k, which)
            finally:
                tree.close()
            assert np.array_equal(q.to_evaluations(), den) and (ones or np.array_equal(p_table.to_evaluations(), num))


# ---- d. the element-wise kernels, every modulus ----------------------------------------------------------------------------

def edge_pairs(p):
    """(alpha, beta) walked over all of edge_words(p): every word stands as alpha and as beta, against itself and against the
    words one place and half the list further on"""
    e = ww.edge_words(p)
    return [(e[i], e[(i + shift) % len(e)]) for shift in (0, 1, len(e) // 2) for i in range(len(e))]


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_table_affine_on_octet_tables(pkg, p):
    ctx = ctx_of(pkg, p)
    for size in (2, 4, 1 << 11):
        t = ww.octet_table(p, size, np.random.default_rng([p % 1000003, size]))
        tc = canon_list(t, p)
        table = upload(pkg, ctx, t)
        for alpha, beta in edge_pairs(p):
            got = pkg.grand_product.table_affine(ctx, table, alpha, beta).to_evaluations()
            assert np.array_equal(got, mont_np(p, gref.affine(tc, gref.canon(alpha, p), gref.canon(beta, p), p))), (size, alpha, beta)
        assert np.array_equal(table.to_evaluations(), t)


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_spark_tuples_on_octet_tables(pkg, p):
    """sc_spark_denominators: spark_tuple_kernel with the key stream (den_w) and with the index as the key (den_t), over lists of
    2 (the tail), 4 (one thread) and 2^11 entries"""
    ctx = ctx_of(pkg, p)
    for ell in (1, 2, 11):
        rng = np.random.default_rng([p % 1000003, ell])
        a = b = ell
        nnz = 1 << ell
        rows, cols = rng.integers(0, 1 << a, size=nnz), rng.integers(0, 1 << b, size=nnz)
        rows[0], rows[-1] = (1 << a) - 1, 0
        sc = pkg.spark.SparseCommitment(ctx, a, b, rows, cols, ww.edge_table(p, nnz, rng), commit=False)
        try:
            assert sc.ell == ell
            ew, tw = ww.octet_table(p, 1 << ell, rng), ww.octet_table(p, 1 << a, rng)
            e, t = upload(pkg, ctx, ew), upload(pkg, ctx, tw)
            e_c, t_c = canon_list(ew, p), canon_list(tw, p)
            for alpha, beta in edge_pairs(p):
                (den_w, den_t), log = logged(ctx, "spark_tuple", lambda: pkg.spark.denominators(ctx, sc, "row", t, e, alpha, beta))
                assert [(kf, m) for kf, m, _ in log] == [(0, ell), (1, a)]
                want_w, want_t = sref.denominators([int(i) for i in rows], e_c, t_c, gref.canon(alpha, p), gref.canon(beta, p), p)
                assert np.array_equal(den_w.to_evaluations(), mont_np(p, want_w)), (ell, alpha, beta)
                assert np.array_equal(den_t.to_evaluations(), mont_np(p, want_t)), (ell, alpha, beta)
            assert np.array_equal(t.to_evaluations(), tw) and np.array_equal(e.to_evaluations(), ew), "the inputs are unchanged"
        finally:
            sc.close()


def eq_sum_case(p, n, count, seed, corners=False):
    """(points, coeffs) of raw edge words; corners: also the coordinates x at which the kernel's own difference one - x borrows
    and leaves a low limb of 0xFFFFFFFF (x = one + 1 mod 2^32) or of 0 (x = one + 2^32), and one - 1"""
    e = ww.edge_words(p)
    if corners:
        one = 2**64 % p
        e = e + [w for w in (one + 1, one + 2**32 + 1, one + 2**32, one - 1) if 0 <= w < p and w not in e]
    rng = np.random.default_rng([p % 1000003, n, count, seed])
    points = [[e[int(i)] for i in rng.integers(0, len(e), size=n)] for _ in range(count)]
    return points, [e[int(i)] for i in rng.integers(0, len(e), size=count)]


def check_eq_sum(pkg, p, n, count, seed, corners=False):
    ctx = ctx_of(pkg, p)
    points, coeffs = eq_sum_case(p, n, count, seed, corners)
    t, log = logged(ctx, "eq_sum", lambda: pkg.multiopen.table_eq_sum(ctx, points, coeffs))
    assert log == [(0, n, count)]
    want = eq_sum_ref(p, [canon_list(pt, p) for pt in points], canon_list(coeffs, p))
    got = t.to_evaluations()
    assert got.shape == (1 << n,) and np.array_equal(got, mont_np(p, want)), (wid(p), n, count)
    return got


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_eq_sum_on_edge_words(pkg, p):
    """n = 1, 7 (no high part), 8 and 9 (one and two high bits) with 1 and 16 points, coordinates and coefficients from the edge
    words and once more with the corners of the kernel's own 1 - x among them; n = 13 (a chunk of 64 high indices) at
    max_blocks = 3 and at the default: the same table"""
    assert pkg.multiopen.LO_LOG == lc.EQ_SUM_LO_LOG == 7
    ctx = ctx_of(pkg, p)
    for n in (1, 7, 8, 9):
        for count in (1, 16):
            check_eq_sum(pkg, p, n, count, 0)
            check_eq_sum(pkg, p, n, count, 2, corners=True)
    base = check_eq_sum(pkg, p, 13, 3, 1)
    with options(ctx, max_blocks=3):
        assert np.array_equal(check_eq_sum(pkg, p, 13, 3, 1), base)


def padded(idx, ell):
    out = np.zeros(1 << ell, dtype=np.int64)
    out[:len(idx)] = idx
    return out


def check_index_and_gather(pkg, p, a, b, rows, cols, vals, U, W):
    """sc_spark_create and sc_spark_gather of one list: the five tables and the gathered two, word for word; returns (cr, cc)"""
    ctx = ctx_of(pkg, p)
    ell = sref.log_len(len(rows))
    prow, pcol = padded(rows, ell), padded(cols, ell)
    sc, log = logged(ctx, "spark_index", lambda: pkg.spark.SparseCommitment(ctx, a, b, rows, cols, vals, commit=False))
    try:
        assert log == [(0, ell, 1 if a <= lc.LOOKUP_LDS_LOG else 0), (1, a, 0), (0, ell, 1 if b <= lc.LOOKUP_LDS_LOG else 0), (1, b, 0)]
        assert sc.ell == ell
        word_of = {m: mont_np(p, list(range(1 << m))) for m in {a, b}}          # the Montgomery word of every index
        want = {"row": word_of[a][prow], "col": word_of[b][pcol], "val": np.concatenate([vals, np.zeros((1 << ell) - len(vals), dtype=np.uint64)]),
                "cr": mont_np(p, sref.counts([int(i) for i in prow], a)), "cc": mont_np(p, sref.counts([int(i) for i in pcol], b))}
        assert np.array_equal(want["cr"], mont_np(p, np.bincount(prow, minlength=1 << a)))
        assert np.array_equal(want["cc"], mont_np(p, np.bincount(pcol, minlength=1 << b)))
        got = {}
        for name in pkg.spark.TABLES:
            got[name] = sc.table(name).to_evaluations()
            assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (wid(p), a, b, name)
        Ut, Wt = upload(pkg, ctx, U), upload(pkg, ctx, W)
        (er, ec), log = logged(ctx, "spark_gather", lambda: pkg.spark.gather(ctx, sc, Ut, Wt))
        assert [m for _, m, _ in log] == [ell]
        assert np.array_equal(er.to_evaluations(), U[prow]) and np.array_equal(ec.to_evaluations(), W[pcol]), (wid(p), a, b, "gather")
        assert np.array_equal(Ut.to_evaluations(), U) and np.array_equal(Wt.to_evaluations(), W), "the inputs are unchanged"
    finally:
        sc.close()
    return got["cr"], got["cc"]


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_spark_index_and_gather_on_runs(pkg, p):
    """the run-shaped lists of layered_edge_cases.run_indices, l = 13: rows over 2^5 counters (LDS histograms: one block, eight
    trips per thread) and columns over 2^14 (global counters, above kLookupLdsLog), at max_blocks = 1, 3 and the default - the
    counts are the same; then two lists shorter than a wave, so that spark_count4 ballots with a part of a wave active"""
    ctx = ctx_of(pkg, p)
    a, b = 5, lc.LOOKUP_LDS_LOG + 1
    assert pkg.logup.LOOKUP_LDS_LOG == lc.LOOKUP_LDS_LOG
    rng = np.random.default_rng(p % 1000003)
    rows, cols = lc.run_indices(a)[0], lc.run_indices(b)[0]
    vals = ww.edge_table(p, len(rows), rng)
    U, W = ww.edge_table(p, 1 << a, rng), ww.edge_table(p, 1 << b, rng)
    assert sref.log_len(len(rows)) == lc.SPARK_L and int(rows.max()) == (1 << a) - 1 and int(cols.max()) == (1 << b) - 1
    counts = [check_index_and_gather(pkg, p, a, b, rows, cols, vals, U, W)]
    for blocks in (1, 3):
        with options(ctx, max_blocks=blocks):
            counts.append(check_index_and_gather(pkg, p, a, b, rows, cols, vals, U, W))
    for cr, cc in counts[1:]:
        assert np.array_equal(cr, counts[0][0]) and np.array_equal(cc, counts[0][1]), "the counts do not depend on max_blocks"
    # the same lists with rows and columns exchanged: the runs over global counters, the uniform part over LDS histograms
    check_index_and_gather(pkg, p, b, a, cols, rows, vals, W, U)
    for small_r, small_c in zip(lc.small_run_indices(a), lc.small_run_indices(b)):
        check_index_and_gather(pkg, p, a, b, small_r, small_c, vals[:len(small_r)], U, W)
