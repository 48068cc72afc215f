"""GPU: the grand product argument (sc_gp_*, sc_table_affine; thaler-study_amd/grand_product.py) against the big-integer
reference of tests/grand_product_ref.py, word for word: the product tree at every remainder of its schedule, the proof at every
hand-over to the host, the host Verifier over device messages with every single tamper, the permutation check over Ligero
commitments, the refusals and the pool's books.

Tables come from wide_words.edge_table.  Its zero words make the product 0 and most low layers of the tree all zero, so the
tables here replace a zero by p - 2 (nonzero_table) except where zeros are the point of the test."""
import ctypes
import gc
import random

import numpy as np
import pytest

import grand_product_cases as cases
import grand_product_ref as ref
import wide_words as ww
from grand_product_cases import GOLD, P61, P64
from ligero_common import context_cache, expect, mont_np
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

ctx_of, teardown_module = context_cache()
QUERIES = 8
MISMATCH_SEED = 2024
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1"}


def nonzero_table(p, n, seed):
    t = ww.edge_table(p, 1 << n, np.random.default_rng(seed))
    t[t == 0] = p - 2
    return t


def upload(pkg, ctx, t):
    return pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, len(t).bit_length() - 1, np.ascontiguousarray(t, dtype=np.uint64))


def default_T(pkg, p):
    """the context's gp_host_log as it was created (the tests put it back)"""
    ctx = ctx_of(pkg, p)
    if not hasattr(ctx, "_gp_default"):
        ctx._gp_default = ctx.get_option("gp_host_log")
    return ctx._gp_default


_REF = {}


def reference(p, n, seed, zeros=False):
    """(table words, canonical table, tree layers, canonical challenges, reference proof dict): computed once, shared, never changed"""
    key = (p, n, seed, zeros)
    if key not in _REF:
        t = ww.edge_table(p, 1 << n, np.random.default_rng(seed)) if zeros else nonzero_table(p, n, seed)
        tc = ref.canon_list(t, p)
        layers = ref.tree(tc, p)
        rng = random.Random(seed + 1)
        ch = [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(cases.n_challenges(n))]
        it = iter(ch)
        _REF[key] = (t, tc, layers, ch, ref.prove(tc, p, lambda k, j, msg: next(it), layers=layers))
    return _REF[key]


# ---- the tree --------------------------------------------------------------------------------------------------------

TREE_SIZES = [(GOLD, n) for n in range(1, 17)] + [(P64, n) for n in (1, 2, 3, 12, 13, 14, 16)]


def check_tree(pkg, p, t):
    ctx = ctx_of(pkg, p)
    n = len(t).bit_length() - 1
    layers = ref.tree(ref.canon_list(t, p), p)
    table = upload(pkg, ctx, t)
    tree = pkg.grand_product.ProductTree(ctx, table)
    assert tree.num_vars == n and tree.product == ref.mont(layers[0][0], p)
    for k in range(n):
        got = tree.layer(k).to_evaluations()
        assert got.shape == (1 << k,) and np.array_equal(got, mont_np(p, layers[k])), (n, k)
    assert np.array_equal(table.to_evaluations(), t), "the input table is unchanged"
    tree.close()
    return layers


@pytest.mark.parametrize("p,n", TREE_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in TREE_SIZES])
def test_tree_product_and_every_layer(pkg, p, n):
    """n = 1 .. 12: the tail kernel alone; 13, 14, 15: one launch of LV = 1, 2, 3 above it; 16: LV = 3 then 1"""
    assert pkg.grand_product.TAIL_LOG == 12
    check_tree(pkg, p, nonzero_table(p, n, 40 + n))


@pytest.mark.parametrize("n", [5, 15])
def test_tree_with_one_zero_entry(pkg, n):
    for at in (0, 1 << (n - 1), (1 << n) - 1):
        t = nonzero_table(GOLD, n, 3 * n)
        t[at] = 0
        layers = check_tree(pkg, GOLD, t)
        assert layers[0] == [0] and all(sum(1 for x in layer if x == 0) == 1 for layer in layers)


def test_tree_with_the_zeros_of_the_edge_table(pkg):
    check_tree(pkg, GOLD, ww.edge_table(GOLD, 1 << 14, np.random.default_rng(5)))


@pytest.mark.parametrize("n,want", [(9, [(0, 9)]), (13, [(1, 13), (0, 12)]), (16, [(3, 16), (1, 13), (0, 12)]), (17, [(3, 17), (2, 14), (0, 12)])])
def test_tree_launch_log(pkg, n, want):
    ctx = ctx_of(pkg, GOLD)
    table = pkg.DenseMultilinearExtension.generate(ctx, 3, n)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    tree = pkg.grand_product.ProductTree(ctx, table)
    log = [x for x in ctx.launch_log() if x["kind"] == "product_tree"]
    ctx.set_option("time_kernels", 0)
    tree.close()
    assert [(x["kf"], x["log_in"]) for x in log] == want
    for x in log:
        m, lv = x["log_in"], x["kf"]
        assert x["ks"] == 0 and x["bytes_read"] == 8 << m
        assert x["bytes_written"] == (8 << m) - (8 << (m - lv) if lv else 8)


# ---- the proof -------------------------------------------------------------------------------------------------------

def device_proof(pkg, p, t, ch_canon, T):
    """sc_gp_prove at gp_host_log = T under the fixed challenges; the draw also checks the order it is called in"""
    ctx = ctx_of(pkg, p)
    n = len(t).bit_length() - 1
    words = ref.mont_list(ch_canon, p)
    seen = []

    def draw(layer, j, msg):
        seen.append((layer, j, len(msg)))
        return words[len(seen) - 1]
    base = default_T(pkg, p)
    ctx.set_option("gp_host_log", T)
    try:
        tree = pkg.grand_product.ProductTree(ctx, upload(pkg, ctx, t))
        proof = pkg.grand_product.prove(tree, draw)
        tree.close()
    finally:
        ctx.set_option("gp_host_log", base)
    assert seen == [(k, j, 4 if j < k else 2) for k in range(n) for j in range(k + 1)]
    return proof


def assert_same(pkg, p, proof, want):
    """bit for bit: the product, all 4 n (n-1) / 2 values, the finals, the point, the claim (and the challenges handed back)"""
    m = lambda xs: ref.mont_list(xs, p)   # noqa: E731
    assert proof.product == ref.mont(want["product"], p)
    assert proof.rounds == [[m(msg) for msg in layer] for layer in want["rounds"]]
    assert proof.finals == [tuple(m(f)) for f in want["finals"]]
    assert proof.point == m(want["point"]) and proof.claim == ref.mont(want["claim"], p)
    assert proof.challenges == m(want["challenges"])


def hand_overs(pkg, p, n, extra=()):
    return sorted(set([0, default_T(pkg, p)]) | set(extra))


PROOF_SIZES = [(GOLD, n) for n in range(1, 15)] + [(p, n) for p in (P64, P61) for n in (1, 2, 7, 13)]


@pytest.mark.parametrize("p,n", PROOF_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in PROOF_SIZES])
def test_proof_is_the_reference_bit_for_bit(pkg, p, n):
    """gp_host_log = 0 (every round on the device) and the default; at n = 5 and 9 on Goldilocks also 1, 3, n - 1 (the hand-over at
    the first possible launch), n (no device round at all) and 12 (above n)"""
    t, _, _, ch, want = reference(p, n, 500 + n)
    extra = (1, 3, n - 1, n, 12) if p == GOLD and n in (5, 9) else ()
    proofs = []
    for T in hand_overs(pkg, p, n, extra):
        proofs.append(device_proof(pkg, p, t, ch, T))
        assert_same(pkg, p, proofs[-1], want)
    assert all(q == proofs[0] for q in proofs[1:]), "transcripts at different gp_host_log are identical"


def test_proof_over_a_table_with_zeros(pkg):
    t, _, _, ch, want = reference(GOLD, 10, 9, zeros=True)
    assert want["product"] == 0
    for T in hand_overs(pkg, GOLD, 10):
        assert_same(pkg, GOLD, device_proof(pkg, GOLD, t, ch, T), want)


def test_n20_is_accepted_by_the_host_verifier(pkg):
    p, n = GOLD, 20
    ctx, gp = ctx_of(pkg, p), pkg.grand_product
    table = upload(pkg, ctx, nonzero_table(p, n, 20))
    tree = gp.ProductTree(ctx, table)
    proof = gp.prove(tree, seed_r=77)
    V = gp.Verifier(pkg.Field(p), n)
    assert V.verify(proof, proof.challenges) == (proof.point, proof.claim)
    assert V.check_input(table.evaluate(proof.point))
    tree.close()


def test_proof_launch_log(pkg):
    p, n = GOLD, 13
    ctx, T = ctx_of(pkg, p), default_T(pkg, p)
    tree = pkg.grand_product.ProductTree(ctx, upload(pkg, ctx, nonzero_table(p, n, 1)))
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    pkg.grand_product.prove(tree, seed_r=1)
    log = [x for x in ctx.launch_log() if x["kind"] == "product_pass"]
    ctx.set_option("time_kernels", 0)
    tree.close()
    te = max(T, 1)
    want = []
    for k in range(T + 1, n):                       # layers <= T leave no record
        want.append((0, k))                         # round 0 reads the layer's tables
        want += [(1, k - j + 1) for j in range(1, k - te + 1)]
    assert [(x["kf"], x["log_in"]) for x in log] == want
    assert all(x["log_in"] > T for x in log)
    for x in log:
        assert x["ks"] == 1 and x["bytes_read"] == 24 << x["log_in"]
        assert x["bytes_written"] == ((24 << (x["log_in"] - 1)) if x["kf"] else 0)


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_table_affine(pkg, p):
    ctx = ctx_of(pkg, p)
    edge = ww.edge_words(p)
    for size in (2, 1 << 5, 1 << 13):
        t = ww.edge_table(p, size, np.random.default_rng(size))
        table = upload(pkg, ctx, t)
        tc = ref.canon_list(t, p)
        for alpha, beta in [(edge[i % len(edge)], edge[(3 * i + 1) % len(edge)]) for i in range(len(edge))]:
            got = pkg.grand_product.table_affine(ctx, table, alpha, beta).to_evaluations()
            assert np.array_equal(got, mont_np(p, ref.affine(tc, ref.canon(alpha, p), ref.canon(beta, p), p))), (size, alpha, beta)
        assert np.array_equal(table.to_evaluations(), t)


# ---- the argument ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_host_verifier_over_device_messages(pkg, p):
    """an honest device proof is accepted, every single tamper of it is refused by its own error (challenges are random words
    >= 4: tests/test_grand_product_cpu.py says why), a changed input word by the last check"""
    gp, F, n = pkg.grand_product, pkg.Field(p), 6
    ctx = ctx_of(pkg, p)
    t = nonzero_table(p, n, 31)
    rng = random.Random(8)
    ch = [rng.randrange(4, p) for _ in range(cases.n_challenges(n))]
    proof = device_proof(pkg, p, t, ch, default_T(pkg, p))
    V = gp.Verifier(F, n)
    assert V.verify(proof, proof.challenges) == (proof.point, proof.claim)
    table = upload(pkg, ctx, t)
    assert V.check_input(table.evaluate(proof.point))
    for name, where, expected in cases.tampers(n):
        cases.expect_refusal(pkg, gp.Verifier(F, n), cases.apply_tamper(pkg, proof, where, F), proof.challenges, expected)
    t2 = t.copy()
    t2[37] = F.add(int(t2[37]), F.one)
    with pytest.raises(gp.InputMismatch):
        V.check_input(upload(pkg, ctx, t2).evaluate(proof.point))


def committed(pkg, p, words, code, opening):
    """(ligero_pcs.Prover, the verifier of its openings) over a table of Montgomery words"""
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    n = len(words).bit_length() - 1
    c = n // 2
    prover = lp.Prover.commit(ctx, upload(pkg, ctx, words), log_cols=c, log_blowup=1, code=code)
    if opening == "folded":
        return prover, lp.FoldVerifier(F, n, c, 1, prover.root(), QUERIES)
    return prover, lp.Verifier(F, n, c, 1, prover.root(), QUERIES, code=code)


def permutation(pkg, p, a, b, code, opening, seed):
    pa, va = committed(pkg, p, a, code, opening)
    pb, vb = committed(pkg, p, b, code, opening)
    try:
        return pkg.grand_product.prove_permutation(pa, pb, va, vb, random.Random(seed))
    finally:
        pa.close()
        pb.close()


@pytest.mark.parametrize("p,n,code,opening", [(GOLD, 10, "rs", "plain"), (GOLD, 10, "rs", "folded"), (P64, 10, "expander", "plain"), (GOLD, 12, "rs", "plain")],
                         ids=["gold-10-plain", "gold-10-folded", "p64m59-10-expander", "gold-12-plain"])
def test_permutation_is_accepted(pkg, p, n, code, opening):
    a = ww.edge_table(p, 1 << n, np.random.default_rng(n))
    b = a[np.random.default_rng(n + 1).permutation(1 << n)]
    assert permutation(pkg, p, a, b, code, opening, 17) is True


def mismatch_case(p):
    """(a, b, gamma) in canonical integers: b a permutation of a with one word changed, and the gamma MISMATCH_SEED draws first
    (tests/test_grand_product_cpu.py checks on the CPU that the two products differ there)"""
    n = 10
    a = ww.edge_table(p, 1 << n, np.random.default_rng(6))
    b = a[np.random.default_rng(7).permutation(1 << n)].copy()
    b[123] = (int(b[123]) + 1) % p
    gamma = random.Random(MISMATCH_SEED).randrange(p)                 # Field.rand of a random.Random: one randrange(p), canonical
    return ref.canon_list(a, p), ref.canon_list(b, p), gamma


def test_permutation_with_a_changed_word_is_refused(pkg):
    p = GOLD
    a, b, gamma = mismatch_case(p)
    assert pkg.Field(p).rand(random.Random(MISMATCH_SEED)) == ref.mont(gamma, p), "mismatch_case draws gamma as the field does"
    with pytest.raises(pkg.grand_product.PermutationMismatch) as ei:
        permutation(pkg, p, mont_np(p, a), mont_np(p, b), "rs", "plain", MISMATCH_SEED)
    pa = pb = 1
    for x, y in zip(a, b):
        pa, pb = pa * (gamma - x) % p, pb * (gamma - y) % p
    assert (ei.value.product_a, ei.value.product_b) == (ref.mont(pa, p), ref.mont(pb, p))


# ---- refusals and the pool's books -----------------------------------------------------------------------------------

def pool(ctx):
    return ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")


def test_refusals(pkg):
    p = GOLD
    ctx, F, gp = ctx_of(pkg, p), pkg.Field(p), pkg.grand_product
    lib = ctx.lib
    gc.collect()
    base = pool(ctx)
    t1 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, np.array([5], dtype=np.uint64))
    t4 = pkg.DenseMultilinearExtension.generate(ctx, 1, 4)
    h, out = ctypes.c_void_p(), ctypes.c_void_p()
    # sc_gp_create: NULLs, a length below two
    assert lib.sc_gp_create(ctx.h, None, ctypes.byref(h)) == 1 and lib.sc_gp_create(ctx.h, t4.h, None) == 1
    expect(pkg, 1, lambda: gp.ProductTree(ctx, t1), "at least two")
    expect(pkg, 1, lambda: gp.table_affine(ctx, t1, 1, 1), "at least two")
    gc.collect()
    assert pool(ctx)[0] == base[0] + 2                                        # t1 and t4 alone: a refused call leaves nothing behind
    tree = gp.ProductTree(ctx, t4)
    # sc_gp_layer: k >= n, NULLs
    expect(pkg, 1, lambda: tree.layer(4), "layer 4")
    assert lib.sc_gp_layer(ctx.h, tree.h, 0, None) == 1 and lib.sc_gp_layer(ctx.h, None, 0, ctypes.byref(out)) == 1
    assert lib.sc_gp_product(None, None) == 1
    # sc_gp_prove: NULLs, an unreduced draw
    no_draw = ctypes.cast(None, pkg._lib.DRAW_GP_FN)
    fin, point, claim = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    assert lib.sc_gp_prove(ctx.h, tree.h, no_draw, None, 0, None, None, None, point, ctypes.byref(claim)) == 1
    assert lib.sc_gp_prove(ctx.h, tree.h, no_draw, None, 0, None, fin, None, None, ctypes.byref(claim)) == 1
    assert lib.sc_gp_prove(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, None) == 1
    assert lib.sc_gp_prove(ctx.h, None, no_draw, None, 0, None, fin, None, point, ctypes.byref(claim)) == 1
    assert lib.sc_gp_prove(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, ctypes.byref(claim)) == 0   # evals and challenges may be NULL
    expect(pkg, 1, lambda: gp.prove(tree, lambda k, j, msg: p), "unreduced")
    # sc_table_affine: alpha, beta >= p; NULLs
    expect(pkg, 1, lambda: gp.table_affine(ctx, t4, p, 0), "below p")
    expect(pkg, 1, lambda: gp.table_affine(ctx, t4, 0, p), "below p")
    assert lib.sc_table_affine(ctx.h, None, 1, 1, ctypes.byref(out)) == 1 and lib.sc_table_affine(ctx.h, t4.h, 1, 1, None) == 1
    # the option's range
    expect(pkg, 1, lambda: ctx.set_option("gp_host_log", 13), "gp_host_log")
    expect(pkg, 1, lambda: ctx.set_option("gp_host_log", -1), "gp_host_log")
    # p = 3: the cubic through 0 .. 3 does not exist
    c3 = pkg.Context(pkg.Field(3))
    s3 = pkg.DenseMultilinearExtension.from_evaluations_vec(c3, 1, np.array([1, 2], dtype=np.uint64))
    expect(pkg, 6, lambda: gp.ProductTree(c3, s3), "p = 3")
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
        expect(pkg, 6, lambda: gp.ProductTree(other, ot), "sc_gp_create: " + msg)
        expect(pkg, 6, lambda: gp.table_affine(other, ot, 1, 1), "sc_table_affine: " + msg)
        assert other.lib.sc_gp_create(other.h, None, None) == 6
        assert other.lib.sc_gp_layer(other.h, tree.h, 0, ctypes.byref(out)) == 6 and not out.value
        assert other.lib.sc_gp_prove(other.h, tree.h, no_draw, None, 0, None, fin, None, point, ctypes.byref(claim)) == 6
        del ot
        other.close()
    # n > 28 is refused before the table is read: a table handle over 2^29 words that are never touched
    big = ctypes.c_void_p()
    assert lib.sc_table_from_device(ctx.h, ctypes.c_void_p(lib.sc_table_device_ptr(t4.h)), 1 << 29, ctypes.byref(big)) == 0
    assert lib.sc_gp_create(ctx.h, big, ctypes.byref(h)) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode() and not h.value
    assert lib.sc_table_free(ctx.h, big) == 0
    tree.close()
    del t1, t4
    gc.collect()
    assert pool(ctx) == base


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p):
    ctx, F, gp = ctx_of(pkg, p), pkg.Field(p), pkg.grand_product
    n, T = 11, 4
    gc.collect()
    base = pool(ctx)
    table = upload(pkg, ctx, nonzero_table(p, n, 2))
    with_table = pool(ctx)
    tree = gp.ProductTree(ctx, table)
    mid = pool(ctx)
    assert mid[0] == with_table[0] + 1, "the tree is one pool block"
    default = default_T(pkg, p)
    ctx.set_option("gp_host_log", T)
    try:
        gp.prove(tree, seed_r=3)
        assert pool(ctx) == mid, "after a proof"

        class Boom(Exception):
            pass

        def raising_at(layer, j):
            def draw(k, i, msg):
                if (k, i) == (layer, j):
                    raise Boom()
                return F.one
            return draw
        for where, what in (((9, 2), "a device round"), ((9, 7), "a host round of a device layer"), ((3, 1), "a round of a host layer"), ((9, 9), "a rho")):
            with pytest.raises(Boom):
                gp.prove(tree, raising_at(*where))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        # the context still proves, and the same transcript
        assert gp.prove(tree, seed_r=3) == gp.prove(tree, seed_r=3)
    finally:
        ctx.set_option("gp_host_log", default)
    tree.close()
    assert pool(ctx) == with_table, "after close()"
    del table
    gc.collect()
    assert pool(ctx) == base
