"""Folded openings of the Reed-Solomon commitment (sc_rs_fold, sc_ligero_fold_*; csrc/kernels/rs_fold.hpp, DESIGN.md section 9
item 13) against tests/ligero_fold_ref.py: one fold bit for bit at every length from one thread to several blocks, on both field
templates, on both sides of the twist tables' boundary and on worst-case words; at 2^22 and 2^24 words against the device's own
encoder over the fixed message; whole transcripts bit for bit under fixed challenges; the whole protocol with the host
FoldVerifier, honest and tampered; the refusals, the launch log and the pool's books.

A reference prover is built once per (field, shape) and shared by the tests that need it."""
import ctypes
import gc
import random

import numpy as np
import pytest

import ligero_fold_ref as fref
import ligero_ref as ref
from ligero_common import context_cache, expect, mont_np
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD, BABYBEAR, P64S18 = ref.GOLD, ref.BABYBEAR, ref.P64S18
IDS = {GOLD: "gold", BABYBEAR: "babybear", P64S18: "p64s18", 65537: "p65537", 257: "p257"}
CPU_SHAPES = [(3, 3, 1), (5, 1, 1), (6, 3, 1), (7, 2, 2)]
SHAPES = CPU_SHAPES + [(10, 8, 1), (16, 15, 1)]

ctx_of, _close_contexts = context_cache()
_provers = {}


def teardown_module(module):
    _provers.clear()
    _close_contexts(module)


def _id(v):
    return IDS.get(v, str(v))


# ---- 1. one fold, bit for bit ----------------------------------------------------------------------------------------

def fold_equals(pkg, p, words, alphas):
    """sc_rs_fold of the RAW words against the reference's fold of their canonical values"""
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    log_m = len(words).bit_length() - 1
    U = ref.canon(p, words)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, log_m, words)
    for alpha in alphas:
        got = pkg.ligero_pcs.rs_fold(ctx, t, F.from_int(alpha)).to_evaluations()
        want = mont_np(p, fref.fold(U, alpha, p))
        assert got.size == len(words) // 2
        assert np.array_equal(got, want), (p, log_m, alpha, int(np.flatnonzero(got != want)[0]))


def random_words(p, log_m):
    rng = random.Random("%d %d" % (p, log_m))
    return mont_np(p, [rng.randrange(p) for _ in range(1 << log_m)])


@pytest.mark.parametrize("log_m", range(2, 17))
def test_goldilocks_fold_equals_the_reference(pkg, log_m):
    rng = random.Random(log_m)
    fold_equals(pkg, GOLD, random_words(GOLD, log_m), [0, 1, GOLD - 1, rng.randrange(GOLD)])


@pytest.mark.parametrize("p,log_m", [(p, l) for p in (BABYBEAR, 65537) for l in (2, 7, 13, 16)] + [(257, l) for l in range(2, 9)], ids=_id)
def test_generic_fold_equals_the_reference(pkg, p, log_m):
    rng = random.Random(p + log_m)
    fold_equals(pkg, p, random_words(p, log_m), [0, 1, p - 1, rng.randrange(p)])


@pytest.mark.parametrize("kind", ["p-1", "0/p-1"])
def test_full_width_generic_field_on_worst_case_words(pkg, kind):
    p, size = P64S18, 1 << 18                                   # 18 = s: the longest codeword this field has
    words = np.full(size, p - 1, dtype=np.uint64) if kind == "p-1" else np.array([0, p - 1] * (size // 2), dtype=np.uint64)
    fold_equals(pkg, p, words, [p - 1, random.Random(18).randrange(p)])


@pytest.mark.parametrize("log_m", [22, 24])
def test_long_fold_equals_the_encoding_of_the_fixed_message(pkg, log_m):
    """two independent device paths: fold(Enc(m), alpha) and Enc(fix_variables(m, [alpha])); the grid-stride loop runs"""
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, GOLD), pkg.Field(GOLD)
    m = pkg.DenseMultilinearExtension.generate(ctx, 40 + log_m, log_m - 1)
    alpha = F.rand(random.Random(log_m))
    got = lp.rs_fold(ctx, lp.rs_encode_rows_long(ctx, m, log_m - 1, 1), alpha).to_evaluations()
    want = lp.rs_encode_rows_long(ctx, m.fix_variables([alpha]), log_m - 2, 1).to_evaluations()
    assert got.size == 1 << (log_m - 1) and np.array_equal(got, want)


# ---- 2. transcripts --------------------------------------------------------------------------------------------------

def reference_prover(p, n, c, rho):
    key = (p, n, c, rho)
    if key not in _provers:
        rng = random.Random("%d %d %d %d" % key)
        table = [rng.randrange(p) for _ in range(1 << n)]
        _provers[key] = (table, fref.RefFoldProver(table, c, rho, p))
    return _provers[key]


def device_prover(pkg, p, n, c, rho):
    ctx = ctx_of(pkg, p)
    table, _ = reference_prover(p, n, c, rho)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, mont_np(p, table))
    return pkg.ligero_pcs.Prover.commit_long(ctx, poly, c, rho)


@pytest.mark.parametrize("n,c,rho", SHAPES)
@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_transcript_equals_the_reference(pkg, p, n, c, rho):
    F = pkg.Field(p)
    rng = random.Random(n * 100 + c)
    _, want = reference_prover(p, n, c, rho)
    prover = device_prover(pkg, p, n, c, rho)
    assert prover.root() == want.root()
    point = [rng.randrange(p) for _ in range(n)]
    gamma = [rng.randrange(p) for _ in range(1 << (n - c))]
    beta = rng.randrange(p)
    alphas = [rng.randrange(p) for _ in range(c)]
    queries = [0, (1 << (c + rho - 1)) - 1] + [rng.randrange(1 << (c + rho - 1)) for _ in range(4)]
    opening = prover.fold_begin(ref.mont(p, point), ref.mont(p, gamma))
    assert list(opening.claims) == ref.mont(p, want.begin(point, gamma))
    seen = []
    rounds, roots, challenges, final = opening.prove(F.from_int(beta), lambda i, e, root: seen.append((i, e, root)) or F.from_int(alphas[i]))
    w_rounds, w_roots, _, w_final = want.prove(beta, lambda i, e, root: alphas[i])
    assert rounds == [ref.mont(p, e) for e in w_rounds]
    assert roots == w_roots and len(roots) == c - 1
    assert challenges == ref.mont(p, alphas) and final == ref.mont(p, [w_final])[0]
    assert seen == [(i, rounds[i], roots[i - 1] if i else None) for i in range(c)]          # what `draw` is shown
    got = opening.query(queries)
    for (q, lo, hi, layers), (wq, w_lo, w_hi, w_layers) in zip(got, want.query(queries)):
        assert q == wq
        for (j, vals, path), (wj, w_vals, w_sib) in ((lo, w_lo), (hi, w_hi)):
            assert j == wj and vals == ref.mont(p, w_vals) and path.siblings == w_sib
        assert [(list(pair), sib) for pair, sib in layers] == [(ref.mont(p, pair), sib) for pair, sib in w_layers]
    opening.close()
    prover.close()


# ---- 3. the whole protocol -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,c,rho", SHAPES)
@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_open_folded_is_accepted_with_the_value(pkg, p, n, c, rho):
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    rng = random.Random(n + c)
    prover = device_prover(pkg, p, n, c, rho)
    point = [F.rand(rng) for _ in range(n)]
    v = lp.FoldVerifier(F, n, c, rho, prover.root(), 12)
    assert lp.open_folded(prover, v, point, rng) == prover.poly.evaluate(point)
    prover.close()


def test_the_limit_shape(pkg):
    """(n, c, rho) = (24, 23, 1): codewords of 2^24 words, two rows, every layer from 2^23 words down"""
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, GOLD), pkg.Field(GOLD)
    rng = random.Random(24)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 11, 24)
    prover = lp.Prover.commit_long(ctx, poly, 23, 1)
    point = [F.rand(rng) for _ in range(24)]
    v = lp.FoldVerifier(F, 24, 23, 1, prover.root(), 8)
    assert lp.open_folded(prover, v, point, rng) == poly.evaluate(point)
    prover.close()


def test_tampered_device_messages_are_refused(pkg):
    """the tamper cases of tests/test_ligero_fold_cpu.py, once, on the device prover's messages"""
    lp = pkg.ligero_pcs
    p, n, c, rho = GOLD, 6, 3, 1
    F = pkg.Field(p)
    prover = device_prover(pkg, p, n, c, rho)

    def exchange(tamper):
        rng = random.Random(5)
        v = lp.FoldVerifier(F, n, c, rho, prover.root(), 8)
        point = [F.rand(rng) for _ in range(n)]
        opening = prover.fold_begin(point, v.draw_gamma(rng))
        try:
            claims = list(opening.claims)
            if tamper in ("v", "v_gamma"):
                k = tamper == "v_gamma"
                claims[k] = F.add(claims[k], F.one)
            v.receive_claims(*claims)

            def draw(i, e, root):
                if (tamper == "round" and i == c - 1) or (tamper == "round0" and i == 0):
                    e[2 if tamper == "round" else 0] = F.add(e[2 if tamper == "round" else 0], F.one)
                if tamper == "root" and i == 1:
                    root = bytes([root[0] ^ 1]) + root[1:]
                return v.round(i, e, root, rng)

            final = opening.prove(v.draw_beta(rng), draw)[3]
            v.receive_final(F.add(final, F.one) if tamper == "final" else final)
            indices = v.draw_queries(rng)
            asked = list(indices)
            if tamper == "index":
                asked[2] = (asked[2] + 1) % (1 << (c + rho - 1))
            openings = opening.query(asked)
            q, lo, hi, layers = openings[2]
            if tamper == "index":
                openings[2] = (indices[2], lo, hi, layers)
            if tamper == "pair":
                pair, sib = layers[-1]
                openings[2] = (q, lo, hi, layers[:-1] + [((F.add(pair[0], F.one), pair[1]), sib)])
            if tamper == "path":
                pair, sib = layers[0]
                openings[2] = (q, lo, hi, [(pair, [bytes(32)] + sib[1:])] + layers[1:])
            if tamper == "column":
                j, vals, path = lo
                openings[2] = (q, (j, vals[:-1] + [F.add(vals[-1], F.one)], path), hi, layers)
            return v.verify(point, openings), prover.poly.evaluate(point)
        finally:
            opening.close()

    value, want = exchange(None)
    assert value == want
    for tamper, err in (("v", lp.RoundMismatch), ("v_gamma", lp.RoundMismatch), ("round0", lp.RoundMismatch), ("round", lp.EvalMismatch),
                        ("root", lp.MerkleMismatch), ("final", lp.EvalMismatch), ("pair", lp.MerkleMismatch), ("path", lp.MerkleMismatch),
                        ("column", lp.MerkleMismatch), ("index", lp.MerkleMismatch)):
        with pytest.raises(err):
            exchange(tamper)
    prover.close()


# ---- 4. refusals, the launch log, the pool's books -------------------------------------------------------------------

def test_refusals(pkg):
    lp = pkg.ligero_pcs
    g, G = ctx_of(pkg, GOLD), pkg.Field(GOLD)
    rng = random.Random(3)
    poly = pkg.DenseMultilinearExtension.generate(g, 9, 6)
    point, gamma = [G.rand(rng) for _ in range(6)], [G.rand(rng) for _ in range(8)]
    prover = lp.Prover.commit(g, poly, 3, 1)
    # the plain-opening shape, the other code, another context's commitment
    flat = lp.Prover.commit(g, poly, 0, 1)
    expect(pkg, 1, lambda: flat.fold_begin(point, [G.rand(rng) for _ in range(64)]), "plain opening")
    flat.close()
    xc = lp.Prover.commit(g, poly, 3, 1, code="expander")
    expect(pkg, 6, lambda: xc.fold_begin(point, gamma), "expander")
    xc.close()
    other = pkg.Context(G)
    h = ctypes.c_void_p()
    z, gm, claims = lp._words(point), lp._words(gamma), np.zeros(2, dtype=np.uint64)
    assert other.lib.sc_ligero_fold_begin(other.h, prover.h, lp._u64p(z), lp._u64p(gm), lp._u64p(claims), ctypes.byref(h)) == 1 and not h.value
    assert "another context" in other.lib.sc_last_error(other.h).decode()
    # null pointers
    assert g.lib.sc_ligero_fold_begin(g.h, None, lp._u64p(z), lp._u64p(gm), lp._u64p(claims), ctypes.byref(h)) == 1 and not h.value
    assert g.lib.sc_ligero_fold_begin(g.h, prover.h, None, lp._u64p(gm), lp._u64p(claims), ctypes.byref(h)) == 1 and not h.value
    assert g.lib.sc_ligero_fold_begin(g.h, prover.h, lp._u64p(z), lp._u64p(gm), lp._u64p(claims), None) == 1
    assert g.lib.sc_rs_fold(g.h, None, 0, ctypes.byref(h)) == 1 and g.lib.sc_rs_fold(g.h, poly.h, 0, None) == 1
    # unreduced words
    expect(pkg, 1, lambda: prover.fold_begin([GOLD] + point[1:], gamma), "not reduced")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma[:-1] + [GOLD]), "not reduced")
    expect(pkg, 1, lambda: lp.rs_fold(g, poly, GOLD), "not reduced")
    opening = prover.fold_begin(point, gamma)
    assert g.lib.sc_ligero_fold_prove(other.h, opening.h, 0, pkg._lib.DRAW_FOLD_FN(lambda *a: 0), None, lp._u64p(claims), None, None, lp._u64p(claims)) == 1
    other.close()
    # the order of the calls
    expect(pkg, 5, lambda: opening.query([1]), "sc_ligero_fold_prove")
    expect(pkg, 1, lambda: opening.prove(GOLD, lambda i, e, root: 1), "beta")
    expect(pkg, 1, lambda: opening.prove(1, lambda i, e, root: GOLD), "unreduced")
    ev = np.zeros(9, dtype=np.uint64)
    assert g.lib.sc_ligero_fold_prove(g.h, opening.h, 1, pkg._lib.DRAW_FOLD_FN(), None, lp._u64p(ev), None, None, lp._u64p(claims)) == 1   # no draw
    with pytest.raises(ZeroDivisionError):
        opening.prove(1, lambda i, e, root: 1 // 0)             # an exception in `draw` ends the call and comes back
    opening.prove(1, lambda i, e, root: G.from_int(i + 2))       # (a refused prove leaves the opening where it was)
    expect(pkg, 5, lambda: opening.prove(1, lambda i, e, root: 1), "already")
    expect(pkg, 1, lambda: opening.query([3, 8]), "L / 2")       # L / 2 = 8
    assert len(opening.query([7])) == 1
    opening.close()
    prover.close()
    # sc_rs_fold: too short, longer than the field's roots reach, longer than 2^24
    tiny = pkg.DenseMultilinearExtension.from_evaluations_vec(g, 1, G.from_ints([1, 2]))
    expect(pkg, 1, lambda: lp.rs_fold(g, tiny, 1), "at least 4")
    f = ctx_of(pkg, 257)
    expect(pkg, 6, lambda: lp.rs_fold(f, pkg.DenseMultilinearExtension.generate(f, 1, 9), 1), "2-adicity 8", "257")
    expect(pkg, 6, lambda: lp.rs_fold(g, pkg.DenseMultilinearExtension.generate(g, 1, 25), 1), "2^24")
    assert len(lp.rs_fold(g, poly, 1)) == 32                      # the context still works


def test_sharded_and_multi_device_are_refused(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    g = ctx_of(pkg, GOLD)
    poly = pkg.DenseMultilinearExtension.generate(g, 9, 4)
    prover = lp.Prover.commit(g, poly, 2, 1)
    words = F.from_ints(range(16))
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, words)
    expect(pkg, 6, lambda: lp.rs_fold(m, mt, 1), "multi-device")
    h, claims = ctypes.c_void_p(), np.zeros(2, dtype=np.uint64)
    z = lp._words(words[:4])
    assert m.lib.sc_ligero_fold_begin(m.h, prover.h, lp._u64p(z), lp._u64p(z), lp._u64p(claims), ctypes.byref(h)) == 6 and not h.value
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, words)
    expect(pkg, 6, lambda: lp.rs_fold(sh, st, 1), "sharded")
    assert sh.lib.sc_ligero_fold_begin(sh.h, prover.h, lp._u64p(z), lp._u64p(z), lp._u64p(claims), ctypes.byref(h)) == 6 and not h.value
    prover.close()


def test_launch_log(pkg):
    """(16, 15, 1): one rs_fold launch per round, the leaves hashed in it - no column-leaf launch - with the stated records"""
    p, n, c, rho = GOLD, 16, 15, 1
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    rng = random.Random(16)
    prover = device_prover(pkg, p, n, c, rho)
    opening = prover.fold_begin([F.rand(rng) for _ in range(n)], [F.rand(rng), F.rand(rng)])
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    opening.prove(F.rand(rng), lambda i, e, root: F.from_int(i + 3))
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    folds = [x for x in log if x["kind"] == "rs_fold"]
    assert len(folds) == c
    for i, x in enumerate(folds):
        M = 1 << (c + rho - i)
        hashed = i + 1 < c
        assert (x["kf"], x["ks"], x["log_in"]) == (int(hashed), c + rho - i, n), (i, x)
        assert (x["bytes_read"], x["bytes_written"]) == (8 * M, 4 * M + (8 * M if hashed else 0)), (i, x)
    assert not [x for x in log if x["kind"] == "ligero" and x["kf"] == 0]
    # the trees of the layers with more than kMerkleTopNodes leaves run level launches, the others the top kernel alone
    assert [x["kf"] for x in log if x["kind"] == "merkle"].count(2) == c - 1
    opening.close()
    prover.close()


@pytest.mark.parametrize("log_m", [2, 12, 13])
@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_rs_fold_is_the_one_challenge_fold_under_its_own_record(pkg, p, log_m):
    """sc_rs_fold at the smallest codeword and on either side of the twist tables' first length: one launch, recorded as rs_fold
    with kf = 0, and word for word what sc_rs_fold_many gives with that one challenge"""
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    M = 1 << log_m
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, log_m, random_words(p, log_m))
    alpha = F.rand(random.Random(p + log_m))
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    got = pkg.ligero_pcs.rs_fold(ctx, t, alpha)
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert [(x["kind"], x["kf"], x["ks"], x["bytes_read"], x["bytes_written"]) for x in log] == [("rs_fold", 0, log_m, 8 * M, 4 * M)], log
    assert np.array_equal(got.to_evaluations(), pkg.ligero_pcs.rs_fold_many(ctx, t, [alpha]).to_evaluations())


@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_pool_balance(pkg, p):
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    n, c = 14, 12
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, n)

    def workload(refused):
        rng = random.Random(8)
        prover = lp.Prover.commit(ctx, poly, c, 1)
        point = [F.rand(rng) for _ in range(n)]
        if refused:
            expect(pkg, 1, lambda: prover.fold_begin(point, [p] * 4))
            opening = prover.fold_begin(point, [F.rand(rng) for _ in range(4)])
            expect(pkg, 1, lambda: opening.prove(1, lambda i, e, root: p if i == 5 else 1), "unreduced")      # refused half-way
            expect(pkg, 5, lambda: opening.query([0]))
            opening.close()
            expect(pkg, 1, lambda: lp.rs_fold(ctx, poly, p))
        else:
            v = lp.FoldVerifier(F, n, c, 1, prover.root(), 4)
            assert lp.open_folded(prover, v, point, rng) == poly.evaluate(point)
            folded = lp.rs_fold(ctx, poly, 1)
            del folded
        prover.close()

    workload(False)                         # (the tables of this length are workspace of the context, made here)
    gc.collect()
    books = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")
    for refused in (False, True):
        workload(refused)
        gc.collect()
        assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == books, refused
    assert len(lp.rs_fold(ctx, poly, 1)) == 1 << (n - 1)
