"""GPU: the grand product argument over K = F_p[X] / (X^2 - w) (sc_gp_*_ext; thaler-study_amd/ext_grand_product.py) against the
big-integer reference of tests/ext_gp_ref.py, bit for bit: the transcript at every form of the pass and every hand-over to the host,
four moduli, few blocks; the tree at every layer and every schedule around the tail limit; against sc_gp_prove in the base-field
limit; the launch log against the byte model; every refusal; the pool's books; and the permutation check over Ligero commitments
(Reed-Solomon and expander code) with gamma in K.

Tables come from wide_words.octet_table; the components of alpha, beta and the challenges from {0, 1, p - 1, random}."""
import ctypes
import gc
import random

import numpy as np
import pytest

import ext_gp_ref as ref
import ext_ref as xref
import ligero_ref as lref
import wide_words as ww
from conftest import load_package
from ligero_common import context_cache, expect
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu
XG = load_package().ext_grand_product     # (the module under test: without it nothing here can run)

ctx_of, teardown_module = context_cache()
GOLD = lref.GOLD
P64, P61, P32 = 2**64 - 59, 2**61 - 1, 2**32 + 15
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1", P32: "p32p15"}
QUERIES = 8
TAIL = 11


def upload(pkg, ctx, words):
    return pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, len(words).bit_length() - 1, np.ascontiguousarray(words, dtype=np.uint64))


def pool(ctx):
    return ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")


def host_log(pkg, p):
    """the context's gp_host_log as it was created (the tests put it back)"""
    ctx = ctx_of(pkg, p)
    if not hasattr(ctx, "_gp_default"):
        ctx._gp_default = ctx.get_option("gp_host_log")
    return ctx._gp_default


def w_of(p):
    """w as a Montgomery word"""
    return lref.mont(p, [xref.nonresidue(p)])[0]


def m2(p, e):
    return tuple(lref.mont(p, e))


def pick_word(p, rng):
    return rng.choice([0, 1, p - 1, rng.randrange(p)])


def challenges(p, n, rng):
    """canonical challenges in protocol order with components from {0, 1, p - 1, random}; among them (0, 1) = X itself,
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


_REF = {}


def reference(p, n, seed):
    """(table of raw words, alpha, beta, canonical challenges, the reference transcript): computed once, shared, never changed"""
    key = (p, n, seed)
    if key not in _REF:
        t = ww.octet_table(p, 1 << n, np.random.default_rng(seed))
        rng = random.Random(seed + 1)
        alpha, beta = leaf_map(p, rng)
        ch = challenges(p, n, rng)
        out = ref.prove(lref.canon(p, t), alpha, beta, p, xref.nonresidue(p), lambda k, j, msg, it=iter(ch): next(it))
        _REF[key] = (t, alpha, beta, ch, out)
    return _REF[key]


def want_of(p, out):
    m = lambda e: m2(p, e)   # noqa: E731
    return XG.Proof(m(out["product"]), [[[m(h) for h in msg] for msg in layer] for layer in out["rounds"]], [(m(l), m(r)) for l, r in out["finals"]],
                    [m(z) for z in out["point"]], m(out["claim"]), [m(c) for c in out["challenges"]])


def device(pkg, p, t, alpha, beta, ch_canon, H, blocks=None, log=None):
    """sc_gp_create_ext and sc_gp_prove_ext at gp_host_log = H (and max_blocks = blocks) under the fixed challenges; the draw also
    checks the order it is called in and the width of every message.  log: a list that receives the launch records of the proof"""
    ctx = ctx_of(pkg, p)
    n = len(t).bit_length() - 1
    words = [m2(p, c) for c in ch_canon]
    seen = []

    def draw(layer, j, msg):
        seen.append((layer, j, len(msg)))
        assert all(len(m) == 2 for m in msg)
        return words[len(seen) - 1]
    base, base_blocks = host_log(pkg, p), ctx.get_option("max_blocks")
    table = upload(pkg, ctx, t)
    ctx.set_option("gp_host_log", H)
    if blocks:
        ctx.set_option("max_blocks", blocks)
    try:
        tree = XG.ExtProductTree(ctx, w_of(p), table, m2(p, alpha), m2(p, beta))
        if log is not None:
            ctx.set_option("time_kernels", 1)
            ctx.launch_log()
        proof = XG.prove_ext(tree, draw)
        if log is not None:
            log.extend(ctx.launch_log())
        tree.close()
    finally:
        ctx.set_option("gp_host_log", base)
        ctx.set_option("max_blocks", base_blocks)
        ctx.set_option("time_kernels", 0)
    assert seen == [(k, j, 4 if j < k else 2) for k in range(n) for j in range(k + 1)]
    assert np.array_equal(table.to_evaluations(), t), "the input is never written"
    return proof


# ---- 1. the full transcript against the reference ---------------------------------------------------------------------------------

SMALL = [(GOLD, n) for n in range(1, 7)]


@pytest.mark.parametrize("p,n", SMALL, ids=["%s-%d" % (IDS[p], n) for p, n in SMALL])
def test_transcript_at_every_form_of_the_pass(pkg, p, n):
    """gp_host_log = 0: n = 1 everything on the host, the leaves too; n = 2 the leaf-in pass without a fold as the only launch; n = 3
    the leaf-in fold; n = 4 a planes-in fold after it; n = 5, 6 two and more in a row - and in each the lower layers read planes
    from the tree.  Also at the default, where all of it is on the host"""
    t, alpha, beta, ch, out = reference(p, n, 700 + n)
    want = want_of(p, out)
    for H in (0, host_log(pkg, p)):
        assert device(pkg, p, t, alpha, beta, ch, H) == want, H


@pytest.mark.parametrize("n", [11, 12, 13])
def test_transcript_at_the_default_hand_over(pkg, n):
    p = GOLD
    t, alpha, beta, ch, out = reference(p, n, 700 + n)
    want = want_of(p, out)
    outs = [device(pkg, p, t, alpha, beta, ch, H) for H in sorted({0, 3, host_log(pkg, p)})]
    for got in outs:
        assert got == want
    assert all(o == outs[0] for o in outs[1:]), "transcripts at different gp_host_log are identical"


WIDE_SIZES = [(p, n) for p in (P64, P61, P32) for n in (1, 3, 7, 12)]


@pytest.mark.parametrize("p,n", WIDE_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in WIDE_SIZES])
def test_transcript_over_the_generic_field(pkg, p, n):
    t, alpha, beta, ch, out = reference(p, n, 800 + n)
    want = want_of(p, out)
    for H in sorted({0, host_log(pkg, p)}):
        assert device(pkg, p, t, alpha, beta, ch, H) == want, H


def want_log(n, te, T):
    """(kind, kf, ks, log_in, bytes read, bytes written) of every launch of a proof at gp_host_log = T: per layer k > T its eq table,
    round 0 over the layer's tables and one folding launch per later device round; L and R are base words (ks = 1) in layer n - 1
    until the first fold has run"""
    out = []
    for k in range(T + 1, n):
        leaf = k == n - 1
        out.append(("ext_eq_table", 0, 0, k, 16 * k, 16 << k))
        out.append(("ext_product_pass", 0, 1 if leaf else 2, k, (16 << k) + ((16 if leaf else 32) << k), 0))
        for j in range(1, k - te + 1):
            m = k - j + 1
            first = leaf and j == 1
            out.append(("ext_product_pass", 1, 1 if first else 2, m, (16 << m) + ((16 if first else 32) << m), 48 << (m - 1)))
    return out


def records(log):
    return [(x["kind"], x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log
            if x["kind"] in ("ext_eq_table", "ext_product_pass", "ext_product_tree")]


@pytest.mark.parametrize("blocks", [1, 3])
def test_few_blocks(pkg, blocks):
    """n = 13, every round on the device: with max_blocks = 3 threads take uneven numbers of trips through the grid-stride loops and
    finish_pass hands off across three blocks, with max_blocks = 1 one block does everything (the tree too).  The transcript is the
    reference's and the launches are the byte model's"""
    p, n = GOLD, 13
    t, alpha, beta, ch, out = reference(p, n, 700 + n)
    log = []
    assert device(pkg, p, t, alpha, beta, ch, 0, blocks, log) == want_of(p, out)
    assert records(log) == want_log(n, 1, 0)


# ---- 2. the tree, every layer ---------------------------------------------------------------------------------------------------

_TREES = {}


def reference_tree(p, n, seed):
    key = (p, n, seed)
    if key not in _TREES:
        t = ww.octet_table(p, 1 << n, np.random.default_rng(seed))
        alpha, beta = leaf_map(p, random.Random(seed + 2))
        w = xref.nonresidue(p)
        _TREES[key] = (t, alpha, beta, ref.tree(ref.leaves(lref.canon(p, t), alpha, beta, p, w), p, w))
    return _TREES[key]


def plane(p, layer, c):
    return np.array(lref.mont(p, [e[c] for e in layer]), dtype=np.uint64)


def want_tree_log(n, lv):
    out, m = [], n
    while m > TAIL:
        step = min(lv, m - TAIL)
        ks = 1 if m == n else 2
        out.append(("ext_product_tree", step, ks, m, (8 * ks) << m, (16 << m) - (16 << (m - step))))
        m -= step
    ks = 1 if m == n else 2
    out.append(("ext_product_tree", 0, ks, m, (8 * ks) << m, (16 << m) - 16))
    return out


TREE_SIZES = [(GOLD, n, lv) for n in range(TAIL + 1, TAIL + 5) for lv in (1, 2, 3)] + [(GOLD, n, 3) for n in (1, 2, 5, TAIL, TAIL + 6)] + [(P64, TAIL + 4, 3), (P64, 3, 3)]


@pytest.mark.parametrize("p,n,lv", TREE_SIZES, ids=["%s-%d-lv%d" % (IDS[p], n, lv) for p, n, lv in TREE_SIZES])
def test_tree_product_and_every_layer(pkg, p, n, lv):
    """n = tail limit + 1 .. + 4 under gp_tree_lv = 1, 2, 3: every LV with the leaves in (the first launch) and with planes in, the
    tail with planes in - but LV = 3 with planes in, which needs six layers above the tail: n = tail limit + 6; n <= the tail limit:
    the tail with the leaves in.  Every layer of both planes, the product, the launches"""
    assert XG.TAIL_LOG == TAIL
    ctx = ctx_of(pkg, p)
    t, alpha, beta, layers = reference_tree(p, n, 300 + n)
    table = upload(pkg, ctx, t)
    base_lv = ctx.get_option("gp_tree_lv")
    ctx.set_option("gp_tree_lv", lv)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    try:
        tree = XG.ExtProductTree(ctx, w_of(p), table, m2(p, alpha), m2(p, beta))
        log = ctx.launch_log()
    finally:
        ctx.set_option("gp_tree_lv", base_lv)
        ctx.set_option("time_kernels", 0)
    assert records(log) == want_tree_log(n, lv)
    assert tree.num_vars == n and tree.product == m2(p, layers[0][0])
    for k in range(n):
        c0, c1 = tree.layer(k)
        for c, got in enumerate((c0.to_evaluations(), c1.to_evaluations())):
            assert got.shape == (1 << k,) and np.array_equal(got, plane(p, layers[k], c)), (n, k, c)
    assert np.array_equal(table.to_evaluations(), t), "the input table is unchanged"
    if (n, lv) == (TAIL + 4, 3):
        # the proof at the largest of them passes the host verifier, and its claim is beta + alpha t~(z_n)
        F = pkg.Field(p)
        proof = XG.prove_ext(tree, seed_r=11)
        V = XG.Verifier(F, w_of(p), n)
        assert V.verify(proof, proof.challenges) == (proof.point, proof.claim)
        value = pkg.ext_sumcheck.table_evaluate_ext(ctx, w_of(p), table, proof.point)
        assert V.check_input(value, m2(p, alpha), m2(p, beta)) is True
        K = pkg.ext_field.QuadExt(F, w_of(p))
        assert proof.claim == K.add(m2(p, beta), K.mul(m2(p, alpha), value))
        # the synthetic challenger is the documented one
        draw = ref.synthetic_draw(p, 11)
        assert proof.challenges == [m2(p, draw(0, 0, None)) for _ in range(ref.n_challenges(n))]
        with pytest.raises(XG.InputMismatch):
            V.check_input((F.add(value[0], F.one), value[1]), m2(p, alpha), m2(p, beta))
    tree.close()


# ---- 3. the base-field limit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 13])
def test_base_field_limit_is_sc_gp_prove(pkg, n):
    """alpha = (1, 0), beta = 0 and every drawn c1 = 0: the c0 words are sc_gp_prove's own output on the same table, every c1 is 0"""
    p = GOLD
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    t = ww.octet_table(p, 1 << n, np.random.default_rng(60 + n))
    rng = random.Random(n)
    ch = [F.from_int(pick_word(p, rng)) for _ in range(ref.n_challenges(n))]
    table = upload(pkg, ctx, t)
    for H in sorted({0, host_log(pkg, p)}):
        ctx.set_option("gp_host_log", H)
        try:
            base_tree = pkg.grand_product.ProductTree(ctx, table)
            base = pkg.grand_product.prove(base_tree, lambda k, j, msg, it=iter(ch): next(it))
            base_tree.close()
            tree = XG.ExtProductTree(ctx, w_of(p), table, (F.one, 0), (0, 0))
            got = XG.prove_ext(tree, lambda k, j, msg, it=iter(ch): (next(it), 0))
            tree.close()
        finally:
            ctx.set_option("gp_host_log", host_log(pkg, p))
        assert got.product == (base.product, 0) and got.claim == (base.claim, 0)
        assert [[[h[0] for h in msg] for msg in layer] for layer in got.rounds] == base.rounds
        assert all(h[1] == 0 for layer in got.rounds for msg in layer for h in msg)
        assert [(l[0], r[0]) for l, r in got.finals] == base.finals and all(l[1] == 0 and r[1] == 0 for l, r in got.finals)
        assert [z[0] for z in got.point] == base.point and all(z[1] == 0 for z in got.point)
        assert [c[0] for c in got.challenges] == base.challenges


# ---- 4. the launch log and the pool's books ----------------------------------------------------------------------------------------

def test_launch_log_against_the_byte_model(pkg):
    p, n = GOLD, 13
    t, alpha, beta, ch, out = reference(p, n, 700 + n)
    T = host_log(pkg, p)
    log = []
    assert device(pkg, p, t, alpha, beta, ch, T, None, log) == want_of(p, out)
    assert n - 1 > T and records(log) == want_log(n, max(T, 1), T)


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p):
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    n, T = 11, 4
    w = w_of(p)
    gc.collect()
    base = pool(ctx)
    table = upload(pkg, ctx, ww.octet_table(p, 1 << n, np.random.default_rng(2)))
    with_table = pool(ctx)
    tree = XG.ExtProductTree(ctx, w, table, (F.one, F.one), (3, 5))
    mid = pool(ctx)
    assert mid[0] == with_table[0] + 1, "the tree is one pool block"
    default = host_log(pkg, p)
    ctx.set_option("gp_host_log", T)
    try:
        XG.prove_ext(tree, seed_r=3)
        assert pool(ctx) == mid, "after a proof"
        c0, c1 = tree.layer(4)
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
                            ((10, 1), "the leaf-in fold's round")):
            with pytest.raises(Boom):
                XG.prove_ext(tree, raising_at(*where))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        # the context still proves, and the same transcript
        assert XG.prove_ext(tree, seed_r=3) == XG.prove_ext(tree, seed_r=3)
    finally:
        ctx.set_option("gp_host_log", default)
    tree.close()
    assert pool(ctx) == with_table, "after close()"
    del table
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
    # sc_gp_create_ext: NULLs, the length, w, alpha and beta
    assert lib.sc_gp_create_ext(ctx.h, w, None, one, zero, ctypes.byref(h)) == 1 and lib.sc_gp_create_ext(ctx.h, w, t4.h, None, zero, ctypes.byref(h)) == 1
    assert lib.sc_gp_create_ext(ctx.h, w, t4.h, one, None, ctypes.byref(h)) == 1 and lib.sc_gp_create_ext(ctx.h, w, t4.h, one, zero, None) == 1
    assert "a NULL argument" in lib.sc_last_error(ctx.h).decode() and not h.value
    expect(pkg, 1, lambda: XG.ExtProductTree(ctx, w, t1, (F.one, 0), (0, 0)), "at least two")
    expect(pkg, 1, lambda: XG.ExtProductTree(ctx, F.from_int(4), t4, (F.one, 0), (0, 0)), "non-residue")
    expect(pkg, 1, lambda: XG.ExtProductTree(ctx, F.one, t4, (F.one, 0), (0, 0)), "non-residue")
    expect(pkg, 1, lambda: XG.ExtProductTree(ctx, p, t4, (F.one, 0), (0, 0)), "w is not a word below p")
    for bad in ((p, 0), (0, p)):
        expect(pkg, 1, lambda: XG.ExtProductTree(ctx, w, t4, bad, (0, 0)), "not a word below p")
        expect(pkg, 1, lambda: XG.ExtProductTree(ctx, w, t4, (F.one, 0), bad), "not a word below p")
    expect(pkg, 1, lambda: XG.ExtProductTree(ctx, w, t4, (0, 0), (F.one, 0)), "alpha is zero")
    gc.collect()
    assert pool(ctx) == mid, "a refused call leaves nothing behind"
    tree = XG.ExtProductTree(ctx, w, t8, (0, F.one), (F.one, F.one))          # alpha = X: zero in c0 only is no zero
    with_tree = pool(ctx)
    # sc_gp_layer_ext: k >= n, NULLs, a tree of another context
    expect(pkg, 1, lambda: tree.layer(3), "layer 3")
    assert lib.sc_gp_layer_ext(ctx.h, tree.h, 0, None, ctypes.byref(o1)) == 1 and lib.sc_gp_layer_ext(ctx.h, tree.h, 0, ctypes.byref(o0), None) == 1
    assert lib.sc_gp_layer_ext(ctx.h, None, 0, ctypes.byref(o0), ctypes.byref(o1)) == 1 and not o0.value and not o1.value
    assert lib.sc_gp_product_ext(None, None) == 1 and lib.sc_gp_product_ext(tree.h, None) == 1
    other = pkg.Context(F)
    assert other.lib.sc_gp_layer_ext(other.h, tree.h, 0, ctypes.byref(o0), ctypes.byref(o1)) == 1
    assert "not an extension product tree of this context" in other.lib.sc_last_error(other.h).decode()
    fin, point, claim = (ctypes.c_uint64 * 12)(), (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 2)()
    no_draw = ctypes.cast(None, pkg._lib.DRAW_GP_EXT_FN)
    assert other.lib.sc_gp_prove_ext(other.h, tree.h, no_draw, None, 0, None, fin, None, point, claim) == 1
    assert other.lib.sc_gp_destroy_ext(other.h, tree.h) == 1 and other.lib.sc_gp_destroy_ext(other.h, None) == 0
    other.close()
    # sc_gp_prove_ext: NULLs, an unreduced component of a drawn challenge - in a device round, a host round and a rho
    assert lib.sc_gp_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, None, None, point, claim) == 1
    assert lib.sc_gp_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, fin, None, None, claim) == 1
    assert lib.sc_gp_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, None) == 1
    assert lib.sc_gp_prove_ext(ctx.h, None, no_draw, None, 0, None, fin, None, point, claim) == 1
    assert lib.sc_gp_prove_ext(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, claim) == 0   # evals and challenges may be NULL
    for H in (0, host_log(pkg, p)):
        ctx.set_option("gp_host_log", H)
        try:
            for bad in ((p, 1), (1, p)):
                for at in ((2, 0), (2, 1), (1, 1)):
                    expect(pkg, 1, lambda: XG.prove_ext(tree, lambda k, j, msg: bad if (k, j) == at else (1, 1)), "unreduced component")
        finally:
            ctx.set_option("gp_host_log", host_log(pkg, p))
    assert pool(ctx) == with_tree
    # p = 3: the cubic through 0 .. 3 does not exist
    c3 = pkg.Context(pkg.Field(3))
    s3 = pkg.DenseMultilinearExtension.from_evaluations_vec(c3, 1, np.array([1, 2], dtype=np.uint64))
    expect(pkg, 6, lambda: XG.ExtProductTree(c3, 2, s3, (1, 0), (0, 0)), "p = 3")
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
        expect(pkg, 6, lambda: XG.ExtProductTree(other, w, ot, (F.one, 0), (0, 0)), "sc_gp_create_ext: " + msg)
        assert other.lib.sc_gp_create_ext(other.h, 0, None, None, None, None) == 6
        assert other.lib.sc_gp_layer_ext(other.h, tree.h, 0, ctypes.byref(o0), ctypes.byref(o1)) == 6 and not o0.value
        assert other.lib.sc_gp_prove_ext(other.h, tree.h, no_draw, None, 0, None, fin, None, point, claim) == 6
        del ot
        other.close()
    # n > 28 is refused before the table is read: a table handle over 2^29 words that are never touched
    big = ctypes.c_void_p()
    assert lib.sc_table_from_device(ctx.h, ctypes.c_void_p(lib.sc_table_device_ptr(t4.h)), 1 << 29, ctypes.byref(big)) == 0
    assert lib.sc_gp_create_ext(ctx.h, w, big, one, zero, ctypes.byref(h)) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode() and not h.value
    assert lib.sc_table_free(ctx.h, big) == 0
    tree.close()
    del t1, t4, t8
    gc.collect()
    assert pool(ctx) == base


# ---- 6. the permutation check -----------------------------------------------------------------------------------------------------

def verifier_of(pkg, p, prover, code):
    """a fresh verifier of the openings of a commitment"""
    return pkg.ligero_pcs.ExtVerifier(pkg.Field(p), prover.num_vars, prover.log_cols, prover.log_blowup, prover.root(), QUERIES, code=code, w=w_of(p))


def committed(pkg, p, words, code):
    ctx = ctx_of(pkg, p)
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, words), code=code)
    return prover, verifier_of(pkg, p, prover, code)


@pytest.mark.parametrize("p,n,code", [(GOLD, 10, "rs"), (P64, 8, "expander")], ids=["gold-10-rs", "p64m59-8-expander"])
def test_permutation_check(pkg, p, n, code):
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    w = w_of(p)
    a = ww.octet_table(p, 1 << n, np.random.default_rng(n))
    b = a[np.random.default_rng(n + 1).permutation(1 << n)]
    pa, va = committed(pkg, p, a, code)
    pb, vb = committed(pkg, p, b, code)
    assert XG.prove_permutation_ext(pa, pb, va, vb, random.Random(17), w) is True
    # a changed entry: the products differ, and they are the products of gamma - a and gamma - b in K at the gamma drawn
    b2 = b.copy()
    b2[123] = F.add(int(b2[123]), F.one)
    pb2, vb2 = committed(pkg, p, b2, code)
    va = verifier_of(pkg, p, pa, code)
    with pytest.raises(XG.PermutationMismatch) as ei:
        XG.prove_permutation_ext(pa, pb2, va, vb2, random.Random(18), w)
    K = pkg.ext_field.QuadExt(F, w)
    gamma = tuple(lref.canon(p, K.rand(random.Random(18))))
    wc = xref.nonresidue(p)
    prods = []
    for table in (a, b2):
        acc = (1, 0)
        for x in lref.canon(p, table):
            acc = xref.kmul(acc, xref.ksub(gamma, (x, 0), p), p, wc)
        prods.append(m2(p, acc))
    assert (ei.value.product_a, ei.value.product_b) == tuple(prods)
    # a word flipped after the commitment: the prover multiplies what it holds now, the opening is of what it committed to
    a3 = a.copy()
    a3[5] = F.add(int(a3[5]), F.one)
    b3 = a3[np.random.default_rng(n + 2).permutation(1 << n)]
    pb3, vb3 = committed(pkg, p, b3, code)
    va = verifier_of(pkg, p, pa, code)
    kept = pa.poly
    pa.poly = upload(pkg, ctx, a3)
    try:
        with pytest.raises(XG.InputMismatch):
            XG.prove_permutation_ext(pa, pb3, va, vb3, random.Random(19), w)
    finally:
        pa.poly = kept
    for prover in (pa, pb, pb2, pb3):
        prover.close()
