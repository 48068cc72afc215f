"""sc_prove_batch on the GPU (kernels/batch.hpp, engine/abi_batch.inc): a batch of independent product sumchecks proved
together must give every instance, word for word, what sc_prove gives it alone - over Goldilocks, full-width generic moduli
and toy moduli, on every size the batched kernel serves, on edge words, against the C oracle, through a caller's draw; with
one launch per pass for the whole batch; with shared and unchanged input tables; and with its refusals.  MatMult on top:
prove_products is accepted by verify_product."""
import ctypes

import numpy as np
import pytest

from conftest import load_package
from test_gpu_sharded import Loopback
from util import GOLD, challenges, load_golden, oracle, pid, pyref
from wide_words import edge_table, wid

pytestmark = pytest.mark.gpu

P64 = 2**64 - 59
P63 = 2**63 + 29
FIELDS = [GOLD, P64, P63, 5, 389]
BATCHES = [1, 2, 3, 17, 64]
SEED_R = pyref.SEED_R

_ctxs = {}


def ctx_of(pkg, p):
    if p not in _ctxs:
        _ctxs[p] = pkg.Context(pkg.Field(p))
    return _ctxs[p]


def fid(p):
    return wid(p) if p in (P64, P63) else pid(p)


def tables(pkg, ctx, n, k, seed):
    """k distinct device tables of 2^n entries (generated on the device)"""
    return [pkg.DenseMultilinearExtension.generate(ctx, seed + 7919 * t + n, n) for t in range(k)]


def instances(pkg, ctx, n, B, seed=0x5EED):
    """B product instances over a pool of up to 8 tables per side (pairs differ from instance to instance)"""
    k = min(B, 8)
    ta, tb = tables(pkg, ctx, n, k, seed), tables(pkg, ctx, n, k, seed + 1)
    mm = pkg.matrix_multiplication
    return [mm.G(ta[i % k], tb[(3 * i + i // k) % k]) for i in range(B)]


def seeds(B, base=SEED_R):
    return [(base + 1000003 * i) % 2**64 for i in range(B)]


def assert_same(batch, singles, what=""):
    assert len(batch) == len(singles)
    for i, ((c1, ev, ch), (c1s, evs, chs)) in enumerate(zip(batch, singles)):
        assert c1 == c1s, "%s instance %d: c_1" % (what, i)
        assert np.array_equal(ev, evs), "%s instance %d: round polynomials" % (what, i)
        assert np.array_equal(ch, chs), "%s instance %d: challenges" % (what, i)


def singles_of(pkg, ctx, gs, sd, draw=None):
    mm = pkg.matrix_multiplication
    out = []
    for g, s in zip(gs, sd):
        c1, ev, ch = mm.prove(ctx, g, s, draw)
        out.append((c1, ev.copy(), ch.copy()))
    return out


# ---- parity with sc_prove ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, 21))
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_parity_with_single_proofs(p, n):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    mm = pkg.matrix_multiplication
    for B in BATCHES:
        gs = instances(pkg, ctx, n, B, seed=0x1000 * B)
        sd = seeds(B)
        assert_same(mm.prove_batch(ctx, gs, sd), singles_of(pkg, ctx, gs, sd), "n=%d B=%d" % (n, B))


@pytest.mark.parametrize("n", [1, 4, 5, 6, 10, 11, 13, 16, 17, 20])
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_parity_on_edge_words(p, n):
    """tables whose entries are largely the words where the field arithmetic carries"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    mm = pkg.matrix_multiplication
    rng = np.random.default_rng(1000 * n + p % 1009)
    B = 5
    gs = [mm.G(pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, edge_table(p, 1 << n, rng, share=0.7)),
               pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, edge_table(p, 1 << n, rng, share=0.7))) for _ in range(B)]
    # one instance entirely of the largest word
    top = np.full(1 << n, p - 1, dtype=np.uint64)
    gs.append(mm.G(pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, top), pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, top)))
    sd = seeds(len(gs), 77)
    assert_same(mm.prove_batch(ctx, gs, sd), singles_of(pkg, ctx, gs, sd), "edge n=%d" % n)


@pytest.mark.parametrize("n", [8, 16, 20])
@pytest.mark.parametrize("p", [GOLD, P64], ids=fid)
def test_against_oracle(p, n):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    o = oracle(p)
    mm = pkg.matrix_multiplication
    B = 4
    sa = [pyref.SEED_A + 31 * i + n for i in range(B)]
    sb = [pyref.SEED_B + 37 * i + n for i in range(B)]
    gs = [mm.G(pkg.DenseMultilinearExtension.generate(ctx, sa[i], n), pkg.DenseMultilinearExtension.generate(ctx, sb[i], n))
          for i in range(B)]
    sd = seeds(B)
    out = mm.prove_batch(ctx, gs, sd)
    for i, (c1, ev, ch) in enumerate(out):
        assert np.array_equal(ch, challenges(o, n, sd[i])), i
        ref = o.prove(o.generate(sa[i], n), o.generate(sb[i], n), ch)
        assert ref["status"] == 0
        assert c1 == ref["c_1"], i
        assert np.array_equal(ev, ref["evals"]), i
        assert gs[i].evaluate([int(x) for x in ch]) == ref["final_eval"], i


def test_fallback_above_twenty_variables():
    """n = 22: the instances go one after another through sc_prove (no batched launch), with the same results"""
    pkg = load_package()
    ctx = ctx_of(pkg, GOLD)
    mm = pkg.matrix_multiplication
    gs = instances(pkg, ctx, 22, 2)
    sd = seeds(2)
    ctx.set_option("time_kernels", 1)
    try:
        ctx.launch_log(reset=True)
        out = mm.prove_batch(ctx, gs, sd)
        kinds = {r["kind"] for r in ctx.launch_log(reset=True)}
    finally:
        ctx.set_option("time_kernels", 0)
    assert "batch_pass" not in kinds and kinds
    assert_same(out, singles_of(pkg, ctx, gs, sd), "n=22")


# ---- the caller's challenges ------------------------------------------------------------------------------------------

def _transcript_draw(F, i, j, e):
    """a challenge that depends on the round's polynomial (a Fiat-Shamir stand-in)"""
    h = pyref.splitmix64((int(e[0]) * 3 + int(e[1]) * 5 + int(e[2]) * 7 + 1000 * i + j) % 2**64)
    return F.from_int(h % F.p)


@pytest.mark.parametrize("n", [1, 3, 7, 13, 17])
@pytest.mark.parametrize("p", [GOLD, P63, 389], ids=fid)
def test_draw_callback(p, n):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    F = ctx.field
    mm = pkg.matrix_multiplication
    B = 6
    gs = instances(pkg, ctx, n, B, seed=0xD0)
    calls = []

    def draw(i, j, e):
        calls.append((i, j))
        return _transcript_draw(F, i, j, e)

    out = mm.prove_batch(ctx, gs, None, draw)
    assert calls == [(i, j) for j in range(n) for i in range(B)]
    for i, g in enumerate(gs):
        single = mm.prove(ctx, g, 0, lambda _u, j, e, i=i: _transcript_draw(F, i, j, [e[0], e[1], e[2]]))
        assert_same([out[i]], [single], "draw instance %d" % i)


# ---- launches ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 10, 16, 20])
def test_launch_count(n):
    """a batch of 64 makes as many launches as one proof makes passes - one batched launch per pass, never 64 times as many"""
    pkg = load_package()
    ctx = ctx_of(pkg, GOLD)
    mm = pkg.matrix_multiplication
    B = 64
    gs = instances(pkg, ctx, n, B)
    ctx.set_option("time_kernels", 1)
    try:
        ctx.launch_log(reset=True)
        mm.prove(ctx, gs[0], SEED_R)
        single = ctx.launch_log(reset=True)
        mm.prove_batch(ctx, gs, seeds(B))
        batch = ctx.launch_log(reset=True)
    finally:
        ctx.set_option("time_kernels", 0)
    plan = [s for s in pkg.schedule.plan_proof(n) if s["action"] != "host_tail"]
    assert len(single) == len(plan) >= 1
    assert [r["kind"] for r in batch] == ["batch_pass"] * len(single)
    for r, s in zip(batch, single):
        assert (r["kf"], r["ks"], r["log_in"]) == (s["kf"], s["ks"], s["log_in"])
        assert r["bytes_read"] == B * (16 << r["log_in"])   # the batch size, by the log's convention


# ---- tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 9, 12, 18])
def test_shared_and_unchanged_tables(n):
    pkg = load_package()
    ctx = ctx_of(pkg, P64)
    mm = pkg.matrix_multiplication
    t = tables(pkg, ctx, n, 2, 0xA11A5)
    before = [x.to_evaluations().copy() for x in t]
    gs = [mm.G(t[0], t[1]), mm.G(t[0], t[0]), mm.G(t[1], t[0]), mm.G(t[0], t[1]), mm.G(t[1], t[1])]
    sd = seeds(len(gs), 5)
    out = mm.prove_batch(ctx, gs, sd)
    for x, b in zip(t, before):
        assert np.array_equal(x.to_evaluations(), b)
    assert_same(out, singles_of(pkg, ctx, gs, sd), "shared n=%d" % n)
    # instances 0 and 3 are the same product: with the same seed, the same transcript
    out2 = mm.prove_batch(ctx, [gs[0], gs[3]], [9, 9])
    assert_same([out2[0]], [out2[1]])


# ---- refusals ---------------------------------------------------------------------------------------------------------

def _raw(pkg, ctx, tabs_a, tabs_b, count=None, seed=None, c1=None, draw=None):
    lib = ctx.lib
    B = len(tabs_a) if count is None else count
    arr_a = (ctypes.c_void_p * max(1, len(tabs_a)))(*[t.h for t in tabs_a]) if tabs_a is not None else None
    arr_b = (ctypes.c_void_p * max(1, len(tabs_b)))(*[t.h for t in tabs_b]) if tabs_b is not None else None
    sd = np.zeros(max(B, 1), dtype=np.uint64)
    out = np.zeros(max(B, 1), dtype=np.uint64)
    cb = pkg._lib.DRAW_BATCH_FN(draw) if draw else ctypes.cast(None, pkg._lib.DRAW_BATCH_FN)
    u64p = pkg._lib.u64p
    return lib.sc_prove_batch(ctx.h, B, arr_a, arr_b, cb, None,
                              sd.ctypes.data_as(u64p) if seed is None else seed,
                              out.ctypes.data_as(u64p) if c1 is None else c1, None, None)


def test_refusals():
    pkg = load_package()
    ctx = ctx_of(pkg, GOLD)
    F = ctx.field
    t4 = tables(pkg, ctx, 4, 2, 0xBAD)
    t3 = tables(pkg, ctx, 3, 1, 0xBAD)
    ctx.set_option("time_kernels", 1)
    try:
        ctx.launch_log(reset=True)
        assert pkg.load().sc_prove_batch(None, 1, None, None, ctypes.cast(None, pkg._lib.DRAW_BATCH_FN), None, None, None, None, None) == 1
        assert _raw(pkg, ctx, [t4[0]], [t4[1]], count=0) == 1                  # count == 0
        assert _raw(pkg, ctx, None, [t4[1]], count=1) == 1                     # NULL arrays
        assert _raw(pkg, ctx, [t4[0]], None, count=1) == 1
        null = ctypes.cast(None, pkg._lib.u64p)
        assert _raw(pkg, ctx, [t4[0]], [t4[1]], seed=null) == 1                # NULL seeds
        assert _raw(pkg, ctx, [t4[0]], [t4[1]], c1=null) == 1                  # NULL c1
        assert _raw(pkg, ctx, [t4[0], t4[0]], [t4[1], t3[0]]) == 1            # a pair whose lengths differ
        assert _raw(pkg, ctx, [t4[0], t3[0]], [t4[1], t3[0]]) == 1            # instances of different sizes
        odd = ctypes.c_void_p()
        three = np.zeros(3, dtype=np.uint64)
        if ctx.lib.sc_table_upload(ctx.h, three.ctypes.data_as(pkg._lib.u64p), 3, ctypes.byref(odd)) == 0:
            class _T:
                h = odd.value
            assert _raw(pkg, ctx, [_T], [_T]) == 1                             # not 2^n long
            ctx.lib.sc_table_free(ctx.h, odd)
        assert ctx.launch_log(reset=True) == []
        # an unreduced challenge from draw: SC_ERR_ARG, as in sc_prove
        assert _raw(pkg, ctx, [t4[0]], [t4[1]], draw=lambda _u, i, j, e: F.p) == 1
        ctx.launch_log(reset=True)
    finally:
        ctx.set_option("time_kernels", 0)
    # a multi-device handle and a sharded context
    m = pkg.Context(pkg.Field(GOLD), devices=[0, 0])
    mA = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    assert _raw(pkg, m, [mA], [mA]) == 6
    del mA
    m.close()
    sh = pkg.Context(pkg.Field(GOLD))
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    sA = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    assert _raw(pkg, sh, [sA], [sA]) == 6
    # the context still works
    mm = pkg.matrix_multiplication
    gs = [mm.G(t4[0], t4[1])]
    assert_same(mm.prove_batch(ctx, gs, [3]), singles_of(pkg, ctx, gs, [3]))


# ---- MatMult -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64, 389], ids=fid)
def test_prove_products_random_pairs(p):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    mm = pkg.matrix_multiplication
    n = 6
    rng = np.random.default_rng(p % 100003)
    pairs = [(rng.integers(0, p, size=1 << (2 * n), dtype=np.uint64), rng.integers(0, p, size=1 << (2 * n), dtype=np.uint64))
             for _ in range(8)]
    proofs = mm.prove_products(ctx, n, pairs)
    assert len(proofs) == 8
    for i, ((A, B), pf) in enumerate(zip(pairs, proofs)):
        assert mm.verify_product(ctx, n, A, B, pf.C, pf), i
        # what prove_product gives the pair alone, with the instance's seed
        one = mm.prove_product(ctx, n, A, B, seed_r=mm._SEED_R + i)
        assert (pf.claim, pf.c_1) == (one.claim, one.c_1)
        assert np.array_equal(pf.evals, one.evals) and np.array_equal(pf.challenges, one.challenges)
    # one product with a wrong entry in C is rejected
    bad = proofs[3].C.to_evaluations().copy()
    bad[17] = (int(bad[17]) + 1) % p
    assert not mm.verify_product(ctx, n, pairs[3][0], pairs[3][1], bad, proofs[3])
    Cs = [pf.C for pf in proofs]
    Cs[5] = bad
    again = mm.prove_products(ctx, n, pairs, Cs=Cs)
    assert not mm.verify_product(ctx, n, pairs[5][0], pairs[5][1], proofs[5].C, again[5])
    assert mm.verify_product(ctx, n, pairs[4][0], pairs[4][1], Cs[4], again[4])


def test_prove_products_book_matrix():
    """matrix_test_from_book (matrix-multiplication/src/lib.rs:203-303) over F_5, batched with a copy of itself"""
    pkg = load_package()
    kat = load_golden("reference_kats.json")["matmul_book"]
    p, n = kat["p"], kat["n"]
    ctx = ctx_of(pkg, p)
    F = ctx.field
    mm = pkg.matrix_multiplication
    A = F.from_ints([x for row in kat["A"] for x in row])
    B = F.from_ints([x for row in kat["B"] for x in row])
    C = F.from_ints([x for row in kat["C"] for x in row])
    proofs = mm.prove_products(ctx, n, [(A, B), (A, B)], Cs=[C, None], seed_r=[1, 2])
    for pf in proofs:
        assert F.to_ints(pf.C.to_evaluations()) == [x for row in kat["C"] for x in row]
        assert mm.verify_product(ctx, n, A, B, C, pf)
    # over F_5 the point may give an entry zero weight in f~_C(r1, r2): change one whose weight is not zero
    x = [int(v) for v in proofs[0].point[n:] + proofs[0].point[:n]]   # (product_claim's variable order, LE over (row << n) | col)

    def weight(idx):
        w = F.one
        for k, xk in enumerate(x):
            w = F.mul(w, xk if (idx >> k) & 1 else F.sub(F.one, xk))
        return w

    idx = next(i for i in range(len(C)) if weight(i) != 0)
    bad = list(C)
    bad[idx] = F.add(int(bad[idx]), F.one)
    assert not mm.verify_product(ctx, n, A, B, bad, proofs[0])
