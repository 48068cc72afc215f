"""GPU: LogUp's fraction sums over K = F_p[X] / (X^2 - w) (sc_frac_*_ext; thaler-study_amd/ext_logup.py) against the big-integer
reference of tests/ext_logup_ref.py, bit for bit: the transcript at every form of the pass and every hand-over to the host, in both
numerator forms, four moduli, few blocks; the trees at every layer of all four planes and every schedule around the tail limit;
against sc_frac_prove in the base-field limit; the launch log against the byte model; every refusal; the pool's books; and the
lookup between two Ligero commitments (Reed-Solomon and expander code) with alpha in K.

Tables come from wide_words.octet_table; the components of alpha, beta and the challenges from {0, 1, p - 1, random}."""
import ctypes
import gc
import random

import numpy as np
import pytest

import ext_logup_ref as ref
import ext_ref as xref
import ligero_ref as lref
import wide_words as ww
from conftest import load_package
from ligero_common import context_cache, expect
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu
XL = load_package().ext_logup             # (the module under test: without it nothing here can run)

ctx_of, teardown_module = context_cache()
GOLD = lref.GOLD
P64, P61, P32 = 2**64 - 59, 2**61 - 1, 2**32 + 15
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1", P32: "p32p15"}
QUERIES = 8
TAIL = 10
FORMS = [False, True]                     # the numerator: a table, all ones
FORM_IDS = {False: "table", True: "ones"}


def upload(pkg, ctx, words):
    return pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, len(words).bit_length() - 1, np.ascontiguousarray(words, dtype=np.uint64))


def pool(ctx):
    return ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")


def host_log(pkg, p):
    """the context's fr_host_log as it was created (the tests put it back)"""
    ctx = ctx_of(pkg, p)
    if not hasattr(ctx, "_fr_default"):
        ctx._fr_default = ctx.get_option("fr_host_log")
    return ctx._fr_default


def w_of(p):
    """w as a Montgomery word"""
    return lref.mont(p, [xref.nonresidue(p)])[0]


def m2(p, e):
    return tuple(lref.mont(p, e))


def pick_word(p, rng):
    return rng.choice([0, 1, p - 1, rng.randrange(p)])


def challenges(p, n, rng):
    """canonical challenges in the order drawn with components from {0, 1, p - 1, random}; among them (0, 1) = X itself,
    (p - 1, p - 1) and one with c1 = 0, as far as n allows"""
    ch = [(pick_word(p, rng), pick_word(p, rng)) for _ in range(ref.n_challenges(n))]
    ch[-1] = (p - 1, p - 1)
    if len(ch) >= 3:
        ch[0] = (rng.randrange(p), 0)
        ch[len(ch) // 2] = (0, 1)
    return ch


def leaf_map(p, rng):
    alpha = (pick_word(p, rng), pick_word(p, rng))
    while alpha == (0, 0):
        alpha = (pick_word(p, rng), pick_word(p, rng))
    return alpha, (pick_word(p, rng), pick_word(p, rng))


def tables(p, n, ones, seed):
    t = ww.octet_table(p, 1 << n, np.random.default_rng(seed))
    return (None if ones else ww.octet_table(p, 1 << n, np.random.default_rng(seed + 5000))), t


def canon_or_none(p, words):
    return None if words is None else lref.canon(p, words)


_REF = {}


def reference(p, n, ones, seed):
    """(numerators as raw words or None, table of raw words, alpha, beta, canonical challenges, the reference transcript): computed
    once, shared, never changed"""
    key = (p, n, ones, seed)
    if key not in _REF:
        pt, t = tables(p, n, ones, seed)
        rng = random.Random(seed + 1)
        alpha, beta = leaf_map(p, rng)
        ch = challenges(p, n, rng)
        out = ref.prove(canon_or_none(p, pt), lref.canon(p, t), alpha, beta, p, xref.nonresidue(p), lambda k, j, msg, it=iter(ch): next(it))
        _REF[key] = (pt, t, alpha, beta, ch, out)
    return _REF[key]


def want_of(p, out):
    m = lambda e: m2(p, e)   # noqa: E731
    return XL.Proof(tuple(m(e) for e in out["root"]), [[[m(h) for h in msg] for msg in layer] for layer in out["rounds"]],
                    [tuple(m(e) for e in fin) for fin in out["finals"]], [m(z) for z in out["point"]], tuple(m(e) for e in out["claims"]),
                    [m(c) for c in out["challenges"]])


def draw_order(n):
    """(layer, round, elements of the message) of every draw: per layer its rounds, rho, and the lambda of the next layer"""
    out = []
    for k in range(n):
        out += [(k, j, 4) for j in range(k + 1)]
        if k + 1 < n:
            out.append((k, k + 1, 0))
    return out


def device(pkg, p, pt, t, alpha, beta, ch_canon, H, blocks=None, log=None, lv=None):
    """sc_frac_create_ext and sc_frac_prove_ext at fr_host_log = H (and max_blocks = blocks, fr_tree_lv = lv) under the fixed
    challenges; the draw also checks the order it is called in and the width of every message.  log: a list that receives the launch
    records of the proof"""
    ctx = ctx_of(pkg, p)
    n = len(t).bit_length() - 1
    words = [m2(p, c) for c in ch_canon]
    seen = []

    def draw(layer, j, msg):
        seen.append((layer, j, len(msg)))
        assert all(len(m) == 2 for m in msg)
        return words[len(seen) - 1]
    base, base_blocks, base_lv = host_log(pkg, p), ctx.get_option("max_blocks"), ctx.get_option("fr_tree_lv")
    table = upload(pkg, ctx, t)
    numer = upload(pkg, ctx, pt) if pt is not None else None
    ctx.set_option("fr_host_log", H)
    if blocks:
        ctx.set_option("max_blocks", blocks)
    if lv:
        ctx.set_option("fr_tree_lv", lv)
    try:
        tree = XL.ExtFractionTree(ctx, w_of(p), numer, table, m2(p, alpha), m2(p, beta))
        if log is not None:
            ctx.set_option("time_kernels", 1)
            ctx.launch_log()
        proof = XL.prove_ext(tree, draw)
        if log is not None:
            log.extend(ctx.launch_log())
        tree.close()
    finally:
        ctx.set_option("fr_host_log", base)
        ctx.set_option("max_blocks", base_blocks)
        ctx.set_option("fr_tree_lv", base_lv)
        ctx.set_option("time_kernels", 0)
    assert seen == draw_order(n)
    assert np.array_equal(table.to_evaluations(), t), "the input is never written"
    assert numer is None or np.array_equal(numer.to_evaluations(), pt), "the numerators are never written"
    return proof


# ---- 1. the full transcript against the reference ---------------------------------------------------------------------------------

SMALL = [(GOLD, n, ones) for n in range(1, 7) for ones in FORMS]


@pytest.mark.parametrize("p,n,ones", SMALL, ids=["%s-%d-%s" % (IDS[p], n, FORM_IDS[o]) for p, n, o in SMALL])
def test_transcript_at_every_form_of_the_pass(pkg, p, n, ones):
    """fr_host_log = 0: n = 1 everything on the host, the leaves too; n = 2 the leaf-in pass without a fold as the only launch; n = 3
    the leaf-in fold; n = 4 a planes-in fold after it; n = 5, 6 two and more in a row - and in each the lower layers read planes
    from the tree.  Also at the default, where all of it is on the host"""
    pt, t, alpha, beta, ch, out = reference(p, n, ones, 700 + n)
    want = want_of(p, out)
    for H in (0, host_log(pkg, p)):
        assert device(pkg, p, pt, t, alpha, beta, ch, H) == want, H


BIG = [(n, ones) for n in (11, 12, 13) for ones in FORMS]


@pytest.mark.parametrize("n,ones", BIG, ids=["%d-%s" % (n, FORM_IDS[o]) for n, o in BIG])
def test_transcript_at_every_hand_over(pkg, n, ones):
    """n = 11, 12, 13 cross the tail limit of the tree with the leaves in at LV = 1, 2, 3"""
    p = GOLD
    pt, t, alpha, beta, ch, out = reference(p, n, ones, 700 + n)
    want = want_of(p, out)
    outs = [device(pkg, p, pt, t, alpha, beta, ch, H) for H in sorted({0, 3, host_log(pkg, p)})]
    for got in outs:
        assert got == want
    assert all(o == outs[0] for o in outs[1:]), "transcripts at different fr_host_log are identical"
    assert device(pkg, p, pt, t, alpha, beta, ch, 3, lv=1) == want, "and at another fr_tree_lv"


WIDE_SIZES = [(p, n) for p in (P64, P61, P32) for n in (1, 3, 7, 12)]


@pytest.mark.parametrize("p,n", WIDE_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in WIDE_SIZES])
def test_transcript_over_the_generic_field(pkg, p, n):
    for ones in FORMS:
        pt, t, alpha, beta, ch, out = reference(p, n, ones, 800 + n)
        want = want_of(p, out)
        for H in sorted({0, host_log(pkg, p)}):
            assert device(pkg, p, pt, t, alpha, beta, ch, H) == want, (ones, H)


def want_log(n, te, T, ones):
    """(kind, kf, ks, log_in, bytes read, bytes written) of every launch of a proof at fr_host_log = T: per layer k > T its eq table,
    round 0 over the layer's tables and one folding launch per later device round.  ks = the words per entry of L and R read: in
    layer n - 1 they are base words until the first fold has run, and with an all-ones numerator that layer has three tables"""
    out = []
    for k in range(T + 1, n):
        leaf = k == n - 1
        nt = 3 if ones and leaf else 5
        out.append(("ext_eq_table", 0, 0, k, 16 * k, 16 << k))
        ks = (nt - 1) * (1 if leaf else 2)
        out.append(("ext_fraction_pass", 0, ks, k, (16 << k) + ((8 * ks) << k), 0))
        for j in range(1, k - te + 1):
            m = k - j + 1
            ks = (nt - 1) * (1 if leaf and j == 1 else 2)
            out.append(("ext_fraction_pass", 1, ks, m, (16 << m) + ((8 * ks) << m), (16 * nt) << (m - 1)))
    return out


def records(log):
    return [(x["kind"], x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log
            if x["kind"] in ("ext_eq_table", "ext_fraction_pass", "ext_fraction_tree")]


@pytest.mark.parametrize("ones", FORMS, ids=["table", "ones"])
@pytest.mark.parametrize("blocks", [1, 3])
def test_few_blocks(pkg, blocks, ones):
    """n = 13, every round on the device: with max_blocks = 3 threads take uneven numbers of trips through the grid-stride loops and
    finish_pass hands off across three blocks, with max_blocks = 1 one block does everything (the tree too).  The transcript is the
    reference's and the launches are the byte model's"""
    p, n = GOLD, 13
    pt, t, alpha, beta, ch, out = reference(p, n, ones, 700 + n)
    log = []
    assert device(pkg, p, pt, t, alpha, beta, ch, 0, blocks, log) == want_of(p, out)
    assert records(log) == want_log(n, 1, 0, ones)


# ---- 2. the trees, every layer ----------------------------------------------------------------------------------------------------

_TREES = {}


def reference_tree(p, n, ones, seed):
    key = (p, n, ones, seed)
    if key not in _TREES:
        pt, t = tables(p, n, ones, seed)
        alpha, beta = leaf_map(p, random.Random(seed + 2))
        w = xref.nonresidue(p)
        _TREES[key] = (pt, t, alpha, beta, ref.tree(*ref.leaves(canon_or_none(p, pt), lref.canon(p, t), alpha, beta, p, w), p, w))
    return _TREES[key]


def plane(p, layer, c):
    return np.array(lref.mont(p, [e[c] for e in layer]), dtype=np.uint64)


def want_tree_log(n, lv, ones):
    out, m = [], n
    while True:
        step = min(lv, m - TAIL) if m > TAIL else 0
        ks = (1 if ones else 2) if m == n else 4
        out.append(("ext_fraction_tree", step, ks, m, (8 * ks) << m, (32 << m) - (32 << (m - step)) if step else (32 << m) - 32))
        if not step:
            return out
        m -= step


TREE_SIZES = ([(GOLD, n, lv) for n in range(TAIL + 1, TAIL + 5) for lv in (1, 2, 3)] + [(GOLD, n, 3) for n in (1, 2, 5, TAIL, TAIL + 6)]
              + [(P64, TAIL + 4, 3), (P64, 3, 3)])
TREE_CASES = [(p, n, lv, ones) for p, n, lv in TREE_SIZES for ones in FORMS]


@pytest.mark.parametrize("p,n,lv,ones", TREE_CASES, ids=["%s-%d-lv%d-%s" % (IDS[p], n, lv, FORM_IDS[o]) for p, n, lv, o in TREE_CASES])
def test_tree_root_and_every_layer(pkg, p, n, lv, ones):
    """n = tail limit + 1 .. + 4 under fr_tree_lv = 1, 2, 3: every LV with the leaves in (the first launch) and with planes in, the
    tail with planes in - but LV = 3 with planes in, which needs six layers above the tail: n = tail limit + 6 = 16; n <= the tail
    limit: the tail with the leaves in.  Every layer of all four planes, the root, the launches; in both numerator forms"""
    assert XL.TAIL_LOG == TAIL
    ctx = ctx_of(pkg, p)
    pt, t, alpha, beta, (P, Q) = reference_tree(p, n, ones, 300 + n)
    table = upload(pkg, ctx, t)
    numer = upload(pkg, ctx, pt) if pt is not None else None
    base_lv = ctx.get_option("fr_tree_lv")
    ctx.set_option("fr_tree_lv", lv)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    try:
        tree = XL.ExtFractionTree(ctx, w_of(p), numer, table, m2(p, alpha), m2(p, beta))
        log = ctx.launch_log()
    finally:
        ctx.set_option("fr_tree_lv", base_lv)
        ctx.set_option("time_kernels", 0)
    assert records(log) == want_tree_log(n, lv, ones)
    assert tree.num_vars == n and tree.ones == ones and tree.root == (m2(p, P[0][0]), m2(p, Q[0][0]))
    for k in range(n):
        for which, layers in (("p", P), ("q", Q)):
            c0, c1 = tree.layer(k, which)
            for c, got in enumerate((c0.to_evaluations(), c1.to_evaluations())):
                assert got.shape == (1 << k,) and np.array_equal(got, plane(p, layers[k], c)), (n, k, which, c)
    assert np.array_equal(table.to_evaluations(), t), "the input table is unchanged"
    assert numer is None or np.array_equal(numer.to_evaluations(), pt), "the numerators are unchanged"
    if (n, lv) == (TAIL + 4, 3):
        # the proof at n = 14 passes the host verifier, and its claims are beta + alpha t~(z_n) and p~(z_n)
        F = pkg.Field(p)
        proof = XL.prove_ext(tree, seed_r=11)
        V = XL.Verifier(F, w_of(p), n, ones=ones)
        assert V.verify(proof, proof.challenges) == (proof.point, proof.claims[0], proof.claims[1])
        tv = pkg.ext_sumcheck.table_evaluate_ext(ctx, w_of(p), table, proof.point)
        pv = pkg.ext_sumcheck.table_evaluate_ext(ctx, w_of(p), numer, proof.point) if numer is not None else None
        assert V.check_input(pv, tv, m2(p, alpha), m2(p, beta)) is True
        K = pkg.ext_field.QuadExt(F, w_of(p))
        assert proof.claims[1] == K.add(m2(p, beta), K.mul(m2(p, alpha), tv))
        assert proof.claims[0] == (pv if pv is not None else K.one)
        # the synthetic challenger is the documented one
        draw = ref.synthetic_draw(p, 11)
        assert proof.challenges == [m2(p, draw(0, 0, None)) for _ in range(ref.n_challenges(n))]
        with pytest.raises(XL.InputMismatch):
            V.check_input(pv, (F.add(tv[0], F.one), tv[1]), m2(p, alpha), m2(p, beta))
    tree.close()


# ---- 3. the base-field limit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ones", FORMS, ids=["table", "ones"])
@pytest.mark.parametrize("n", [5, 13])
def test_base_field_limit_is_sc_frac_prove(pkg, n, ones):
    """alpha = (alpha0, 0), beta = (beta0, 0) and every drawn c1 = 0: the c0 words are sc_frac_prove's own output over the table
    sc_table_affine(t) = alpha0 t + beta0, every c1 is 0"""
    p = GOLD
    ctx, F, LU = ctx_of(pkg, p), pkg.Field(p), pkg.logup
    pt, t = tables(p, n, ones, 60 + n)
    rng = random.Random(n)
    alpha0, beta0 = F.from_int(rng.randrange(1, p)), F.from_int(pick_word(p, rng))
    ch = [F.from_int(pick_word(p, rng)) for _ in range(ref.n_challenges(n))]
    table = upload(pkg, ctx, t)
    numer = upload(pkg, ctx, pt) if pt is not None else None
    q = pkg.grand_product.table_affine(ctx, table, alpha0, beta0)
    for H in sorted({0, host_log(pkg, p)}):
        ctx.set_option("fr_host_log", H)
        try:
            base_tree = LU.FractionTree(ctx, q, numer)
            base = LU.prove(base_tree, lambda k, j, msg, it=iter(ch): next(it))
            base_tree.close()
            tree = XL.ExtFractionTree(ctx, w_of(p), numer, table, (alpha0, 0), (beta0, 0))
            got = XL.prove_ext(tree, lambda k, j, msg, it=iter(ch): (next(it), 0))
            tree.close()
        finally:
            ctx.set_option("fr_host_log", host_log(pkg, p))
        flat = [got.root, got.claims, got.point, got.challenges] + got.finals + [msg for layer in got.rounds for msg in layer]
        assert all(e[1] == 0 for group in flat for e in group)
        assert tuple(e[0] for e in got.root) == base.root and tuple(e[0] for e in got.claims) == base.claims
        assert [[[h[0] for h in msg] for msg in layer] for layer in got.rounds] == base.rounds
        assert [tuple(e[0] for e in fin) for fin in got.finals] == base.finals
        assert [z[0] for z in got.point] == base.point and [c[0] for c in got.challenges] == base.challenges


# ---- 4. the launch log and the pool's books ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ones", FORMS, ids=["table", "ones"])
def test_launch_log_against_the_byte_model(pkg, ones):
    p, n = GOLD, 13
    pt, t, alpha, beta, ch, out = reference(p, n, ones, 700 + n)
    T = host_log(pkg, p)
    log = []
    assert device(pkg, p, pt, t, alpha, beta, ch, T, None, log) == want_of(p, out)
    assert n - 1 > T and records(log) == want_log(n, max(T, 1), T, ones)


@pytest.mark.parametrize("p,ones", [(GOLD, False), (GOLD, True), (P64, False)], ids=["gold-table", "gold-ones", "p64m59-table"])
def test_pool_books_balance(pkg, p, ones):
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    n, T = 11, 4
    w = w_of(p)
    gc.collect()
    base = pool(ctx)
    pt, t = tables(p, n, ones, 2)
    table = upload(pkg, ctx, t)
    numer = upload(pkg, ctx, pt) if pt is not None else None
    with_tables = pool(ctx)
    tree = XL.ExtFractionTree(ctx, w, numer, table, (F.one, F.one), (3, 5))
    mid = pool(ctx)
    assert mid[0] == with_tables[0] + 1, "the four heaps are one pool block"
    default = host_log(pkg, p)
    ctx.set_option("fr_host_log", T)
    try:
        XL.prove_ext(tree, seed_r=3)
        assert pool(ctx) == mid, "after a proof"
        c0, c1 = tree.layer(4, "q")
        del c0, c1
        gc.collect()
        assert pool(ctx) == mid, "after the copies of a layer are freed"

        class Boom(Exception):
            pass

        def raising_at(layer, j):
            def draw(k, i, msg):
                if (k, i) == (layer, j):
                    raise Boom()
                return (F.one, F.one)
            return draw
        for where, what in (((9, 2), "a device round"), ((9, 7), "a host round of a device layer"), ((3, 1), "a round of a host layer"), ((9, 9), "a rho"),
                            ((8, 9), "a lambda"), ((10, 1), "the leaf-in fold's round")):
            with pytest.raises(Boom):
                XL.prove_ext(tree, raising_at(*where))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        # the context still proves, and the same transcript
        assert XL.prove_ext(tree, seed_r=3) == XL.prove_ext(tree, seed_r=3)
    finally:
        ctx.set_option("fr_host_log", default)
    tree.close()
    assert pool(ctx) == with_tables, "after close()"
    del table, numer
    gc.collect()
    assert pool(ctx) == base


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(pkg):
    p = GOLD
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    lib, w = ctx.lib, w_of(p)
    gc.collect()
    base = pool(ctx)
    t1 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, np.array([5], dtype=np.uint64))
    t4 = pkg.DenseMultilinearExtension.generate(ctx, 1, 2)
    t8 = pkg.DenseMultilinearExtension.generate(ctx, 1, 3)
    mid = pool(ctx)
    h, o0, o1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    one, zero = (ctypes.c_uint64 * 2)(F.one, 0), (ctypes.c_uint64 * 2)(0, 0)
    # sc_frac_create_ext: NULLs (p alone may be NULL), the lengths, w, alpha and beta
    assert lib.sc_frac_create_ext(ctx.h, w, None, None, one, zero, ctypes.byref(h)) == 1
    assert lib.sc_frac_create_ext(ctx.h, w, None, t4.h, None, zero, ctypes.byref(h)) == 1
    assert lib.sc_frac_create_ext(ctx.h, w, None, t4.h, one, None, ctypes.byref(h)) == 1 and lib.sc_frac_create_ext(ctx.h, w, None, t4.h, one, zero, None) == 1
    assert "a NULL argument" in lib.sc_last_error(ctx.h).decode() and not h.value
    expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, w, None, t1, (F.one, 0), (0, 0)), "at least two")
    expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, w, t8, t4, (F.one, 0), (0, 0)), "p has 8 entries, t has 4")
    expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, F.from_int(4), None, t4, (F.one, 0), (0, 0)), "non-residue")
    expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, F.one, None, t4, (F.one, 0), (0, 0)), "non-residue")
    expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, p, None, t4, (F.one, 0), (0, 0)), "w is not a word below p")
    for bad in ((p, 0), (0, p)):
        expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, w, None, t4, bad, (0, 0)), "not a word below p")
        expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, w, t4, t4, (F.one, 0), bad), "not a word below p")
    expect(pkg, 1, lambda: XL.ExtFractionTree(ctx, w, None, t4, (0, 0), (F.one, 0)), "alpha is zero")
    gc.collect()
    assert pool(ctx) == mid, "a refused call leaves nothing behind"
    tree = XL.ExtFractionTree(ctx, w, t8, t8, (0, F.one), (F.one, F.one))       # alpha = X: zero in c0 only is no zero
    with_tree = pool(ctx)
    # sc_frac_layer_ext: k >= n, which, NULLs, a tree of another context
    expect(pkg, 1, lambda: tree.layer(3, "q"), "layer 3")
    expect(pkg, 1, lambda: tree.layer(0, 2), "which = 2")
    assert lib.sc_frac_layer_ext(ctx.h, tree.h, 0, 0, None, ctypes.byref(o1)) == 1 and lib.sc_frac_layer_ext(ctx.h, tree.h, 0, 0, ctypes.byref(o0), None) == 1
    assert lib.sc_frac_layer_ext(ctx.h, None, 0, 0, ctypes.byref(o0), ctypes.byref(o1)) == 1 and not o0.value and not o1.value
    assert lib.sc_frac_root_ext(None, None) == 1 and lib.sc_frac_root_ext(tree.h, None) == 1
    other = pkg.Context(F)
    assert other.lib.sc_frac_layer_ext(other.h, tree.h, 0, 0, ctypes.byref(o0), ctypes.byref(o1)) == 1
    assert "not an extension fraction tree of this context" in other.lib.sc_last_error(other.h).decode()
    fin, point, claims = (ctypes.c_uint64 * 24)(), (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 4)()
    no_draw = ctypes.cast(None, pkg._lib.DRAW_FRAC_EXT_FN)
    assert other.lib.sc_frac_prove_ext(other.h, tree.h, no_draw, None, 0, None, fin, None, point, claims) == 1
    assert other.lib.sc_frac_destroy_ext(other.h, tree.h) == 1 and other.lib.sc_frac_destroy_ext(other.h, None) == 0
    other.close()
    # sc_frac_prove_ext: NULLs, an unreduced component of a drawn challenge - in a device round, a host round, a rho and a lambda
    assert lib.sc_frac_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, None, None, point, claims) == 1
    assert lib.sc_frac_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, fin, None, None, claims) == 1
    assert lib.sc_frac_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, None) == 1
    assert lib.sc_frac_prove_ext(ctx.h, None, no_draw, None, 0, None, fin, None, point, claims) == 1
    assert lib.sc_frac_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, claims) == 0   # evals and challenges may be NULL
    for H in (0, host_log(pkg, p)):
        ctx.set_option("fr_host_log", H)
        try:
            for bad in ((p, 1), (1, p)):
                for at in ((2, 0), (2, 1), (1, 1), (0, 1)):
                    expect(pkg, 1, lambda: XL.prove_ext(tree, lambda k, j, msg: bad if (k, j) == at else (1, 1)), "unreduced component")
        finally:
            ctx.set_option("fr_host_log", host_log(pkg, p))
    assert pool(ctx) == with_tree
    # p = 3: the cubic through 0 .. 3 does not exist
    c3 = pkg.Context(pkg.Field(3))
    s3 = pkg.DenseMultilinearExtension.from_evaluations_vec(c3, 1, np.array([1, 2], dtype=np.uint64))
    expect(pkg, 6, lambda: XL.ExtFractionTree(c3, 2, None, s3, (1, 0), (0, 0)), "p = 3")
    del s3
    c3.close()
    # a multi-device handle and a sharded context: refused before anything else is looked at
    words = F.from_ints(range(1, 9))
    for make, needle in ((lambda: pkg.Context(F, devices=[0, 0]), "a multi-device handle"), (None, "sharded")):
        if make:
            other = make()
        else:
            other = pkg.Context(F)
            ar, ag = Loopback(2).collectives(0)
            other.comm_init_host(0, 2, ar, ag)
        msg = "runs on a context of one device and one rank (this one is %s)" % needle
        ot = pkg.DenseMultilinearExtension.from_evaluations_vec(other, 3, words)
        expect(pkg, 6, lambda: XL.ExtFractionTree(other, w, None, ot, (F.one, 0), (0, 0)), "sc_frac_create_ext: " + msg)
        assert other.lib.sc_frac_create_ext(other.h, 0, None, None, None, None, None) == 6
        assert other.lib.sc_frac_layer_ext(other.h, tree.h, 0, 0, ctypes.byref(o0), ctypes.byref(o1)) == 6 and not o0.value
        assert other.lib.sc_frac_prove_ext(other.h, tree.h, no_draw, None, 0, None, fin, None, point, claims) == 6
        del ot
        other.close()
    # n > 28 is refused before the table is read: a table handle over 2^29 words that are never touched
    big = ctypes.c_void_p()
    assert lib.sc_table_from_device(ctx.h, ctypes.c_void_p(lib.sc_table_device_ptr(t4.h)), 1 << 29, ctypes.byref(big)) == 0
    assert lib.sc_frac_create_ext(ctx.h, w, None, big, one, zero, ctypes.byref(h)) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode() and not h.value
    assert lib.sc_table_free(ctx.h, big) == 0
    tree.close()
    del t1, t4, t8
    gc.collect()
    assert pool(ctx) == base


# ---- 6. the lookup ------------------------------------------------------------------------------------------------------------------

def verifier_of(pkg, p, prover, code):
    """a fresh verifier of the openings of a commitment"""
    return pkg.ligero_pcs.ExtVerifier(pkg.Field(p), prover.num_vars, prover.log_cols, prover.log_blowup, prover.root(), QUERIES, code=code, w=w_of(p))


def committed(pkg, p, words, code):
    ctx = ctx_of(pkg, p)
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, words), code=code)
    return prover, verifier_of(pkg, p, prover, code)


@pytest.mark.parametrize("p,n,code", [(GOLD, 10, "rs"), (P64, 8, "expander")], ids=["gold-10-rs", "p64m59-8-expander"])
def test_lookup_into_a_range_table(pkg, p, n, code, monkeypatch):
    """every w_i < 2^8, the range table t_j = j of m = 8 variables, whose extension the verifier computes itself in K"""
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    w, m = w_of(p), 8
    K = pkg.ext_field.QuadExt(F, w)
    LU = pkg.logup
    table = upload(pkg, ctx, F.from_ints(range(1 << m)))
    table_eval = lambda point: XL.range_table_eval(K, point)   # noqa: E731
    rng = np.random.default_rng(n)
    wit = np.array(F.from_ints([int(x) for x in rng.integers(0, 1 << m, size=1 << n)]), dtype=np.uint64)

    def run(prover, verifier, words, seed, **kw):
        return XL.prove_lookup_ext(prover, None, verifier, None, table, LU.range_indices(F, words), random.Random(seed), w, table_eval=table_eval, **kw)
    pw, vw = committed(pkg, p, wit, code)
    gc.collect()
    before = pool(ctx)
    assert run(pw, vw, wit, 17) is True
    gc.collect()
    assert pool(ctx) == before, "the trees, the multiplicities and their commitment are given back"
    # the default table_eval is the table's own extension
    assert XL.prove_lookup_ext(pw, None, verifier_of(pkg, p, pw, code), None, table, LU.range_indices(F, wit), random.Random(17), w) is True
    # one entry out of range: it is not counted, and the sums differ; they are the sums over K at the alpha drawn
    wit2 = wit.copy()
    wit2[123] = F.from_int((1 << m) + 5)
    pw2, vw2 = committed(pkg, p, wit2, code)
    with pytest.raises(XL.LookupMismatch) as ei:
        run(pw2, vw2, wit2, 18)
    alpha = tuple(lref.canon(p, K.rand(random.Random(18))))
    wc = xref.nonresidue(p)
    total = (0, 0)
    for x in lref.canon(p, wit2):
        total = xref.kadd(total, xref.kinv(xref.ksub(alpha, (x, 0), p), p, wc), p)
    pr, qr = (tuple(lref.canon(p, e)) for e in ei.value.root_w)
    assert xref.kmul(total, qr, p, wc) == pr
    # one multiplicity off by one: the sums differ
    real = LU.multiplicities

    def off_by_one(c, a, b, idx):
        mult, bad = real(c, a, b, idx)
        words = mult.to_evaluations()
        words[77] = F.add(int(words[77]), F.one)
        return upload(pkg, c, words), bad
    monkeypatch.setattr(XL, "multiplicities", off_by_one)
    with pytest.raises(XL.LookupMismatch):
        run(pw, verifier_of(pkg, p, pw, code), wit, 19)
    monkeypatch.setattr(XL, "multiplicities", real)
    # a word flipped after the commitment: the prover sums what it holds now (still in range), the opening is of what it committed to
    wit3 = wit.copy()
    wit3[5] = F.from_int((F.to_int(int(wit3[5])) + 1) % (1 << m))
    kept = pw.poly
    pw.poly = upload(pkg, ctx, wit3)
    try:
        with pytest.raises(XL.InputMismatch) as ei:
            run(pw, verifier_of(pkg, p, pw, code), wit3, 20)
        assert ei.value.which == "w"
    finally:
        pw.poly = kept
    for prover in (pw, pw2):
        prover.close()
