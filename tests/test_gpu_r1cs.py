"""GPU: the sparse products (sc_r1cs_mul, sc_r1cs_bind_rows) and the cubic sumcheck (sc_zerocheck_prove) word for word against
tests/r1cs_ref.py, the whole R1CS argument (thaler-study_amd/r1cs.py) accepted and every tampered message refused, every refusal
of the limits, and the pool's books.  Exact comparison everywhere."""
import ctypes
import gc
import random

import numpy as np
import pytest

import ligero_ref as lref
import r1cs_ref as ref
import wide_words as ww
from ligero_common import context_cache, expect, mont_np
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD = lref.GOLD
P64 = 2**64 - 59
P61 = 2**61 - 1
ctx_of, teardown_module = context_cache()


def canon_np(p, words):
    return lref.canon(p, [int(x) for x in words])


def device_r1cs(pkg, p, s, m, mats):
    """mats: three lists of (row, col, Montgomery word)"""
    return pkg.r1cs.DeviceR1CS(ctx_of(pkg, p), pkg.r1cs.R1CS(pkg.Field(p), s, m, *mats))


def check_products(pkg, p, s, m, mats, seed):
    """sc_r1cs_mul and sc_r1cs_bind_rows of the instance against the reference, on edge words"""
    ctx = ctx_of(pkg, p)
    rng = np.random.default_rng(seed)
    dev = device_r1cs(pkg, p, s, m, mats)
    cmats = [[(i, j, c) for (i, j, _), c in zip(M, canon_np(p, [v for _, _, v in M]))] for M in mats]
    z = ww.edge_table(p, 1 << m, rng)
    zt = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m, z)
    zc = canon_np(p, z)
    for M, got in zip(cmats, dev.mul(zt)):
        assert canon_np(p, got.to_evaluations()) == ref.sparse_mul(M, s, zc, p)
    assert np.array_equal(zt.to_evaluations(), z)
    rx, rho = [int(x) for x in ww.edge_table(p, s, rng)], [int(x) for x in ww.edge_table(p, 3, rng)]
    T = dev.bind_rows(rx, rho)
    assert canon_np(p, T.to_evaluations()) == ref.bind_rows_sparse(cmats, s, m, lref.canon(p, rx), lref.canon(p, rho), p)
    dev.close()


def random_matrix(p, s, m, nnz, rng):
    vals = ww.edge_table(p, max(nnz, 1), rng)[:nnz]
    return [(int(rng.integers(0, 1 << s)), int(rng.integers(0, 1 << m)), int(v)) for v in vals]


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
@pytest.mark.parametrize("s,m", [(1, 2), (4, 3), (9, 11), (13, 12)])
def test_sparse_products_at_every_size_around_a_block(pkg, p, s, m):
    Nb = pkg.r1cs.SPMV_BLOCK_ENTRIES
    rng = np.random.default_rng(100 * s + m)
    sizes = [0, 1, Nb - 1, Nb, Nb + 1, 3 * Nb + 5]
    for k, nnz in enumerate(sizes):
        # A, B, C of three different sizes per instance, every size in every position over the loop
        mats = [random_matrix(p, s, m, sizes[(k + d) % len(sizes)], rng) for d in (0, 2, 3)]
        check_products(pkg, p, s, m, mats, 7 * k + s)


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_sparse_products_on_the_patterns_that_split_rows_over_blocks(pkg, p):
    Nb = pkg.r1cs.SPMV_BLOCK_ENTRIES
    s, m = 9, 11
    rng = np.random.default_rng(p % 1000)
    n = 3 * Nb + 5
    w = [int(x) for x in ww.edge_table(p, n, rng)]
    one_row = [(37, int(rng.integers(0, 1 << m)), v) for v in w]                 # one row holds everything
    one_col = [(int(rng.integers(0, 1 << s)), 1029, v) for v in w]               # transposed: one column does
    last = [((1 << s) - 1, (1 << m) - 1, v) for v in w[:Nb + 9]]                 # every row (and column) empty but the last
    check_products(pkg, p, s, m, (one_row, one_col, last), 1)
    # row ends (and, transposed, column ends) exactly on block boundaries; a duplicated (row, col) many times over
    rows_eq_blocks = [(r, int(rng.integers(0, 1 << m)), w[e]) for r in (3, 4, 200) for e in range(Nb)]
    cols_eq_blocks = [(int(rng.integers(0, 1 << s)), c, w[e]) for c in (0, 1, 77) for e in range(Nb)]
    dup = [(5, 6, v) for v in w[:Nb + 3]] + [(5, 7, w[0]), (6, 6, w[1])]
    check_products(pkg, p, s, m, (rows_eq_blocks, cols_eq_blocks, dup), 2)
    check_products(pkg, p, s, m, ([], [], []), 3)                                 # all three empty
    check_products(pkg, p, 1, 2, ([(1, 3, w[0])], [], [(0, 0, w[1])] * (Nb + 1)), 4)


def test_sparse_products_of_the_synthetic_instance(pkg):
    """(14, 14): column 0 of C holds an entry per constraint - 2^14 entries of one row of the transposed image, eight blocks"""
    p, s, m = GOLD, 14, 14
    R, io, w = pkg.r1cs.synthetic_instance(pkg.Field(p), s, m, 5)
    assert sum(1 for _, j, _ in R.matrices[2] if j == 0) == 1 << s
    check_products(pkg, p, s, m, R.matrices, 6)


def test_launch_log_shows_the_products_and_their_carries(pkg):
    p, s, m = GOLD, 9, 11
    ctx = ctx_of(pkg, p)
    Nb = pkg.r1cs.SPMV_BLOCK_ENTRIES
    rng = np.random.default_rng(3)
    sizes = (Nb + 1, 0, 5)
    dev = device_r1cs(pkg, p, s, m, [random_matrix(p, s, m, n, rng) for n in sizes])
    zt = pkg.DenseMultilinearExtension.generate(ctx, 1, m)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    out = dev.mul(zt)
    T = dev.bind_rows([1] * s, [1, 2, 3])
    log = [x for x in ctx.launch_log() if x["kind"] == "spmv"]
    ctx.set_option("time_kernels", 0)
    want = []
    for nnz, log_out, ks in [(n, s, 0) for n in sizes] + [(sum(sizes), m, 1)]:
        B = (nnz + Nb - 1) // Nb
        want.append((0, ks, log_out, 24 * nnz, 8 * (1 << log_out) + 24 * B))
        if B:
            want.append((1, ks, log_out, 24 * B, 8 * min(2 * B, 1 << log_out)))
    assert [(x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log] == want
    del out, T
    dev.close()


# ---- the cubic prover ------------------------------------------------------------------------------------------------

def challenge_words(p, n, rng):
    """n raw words: the degenerate cycle (0, one, p - 1, ..) with a random word in every third place"""
    out = ww.degenerate_challenges(p, n)
    return [int(rng.integers(0, p, dtype=np.uint64)) if j % 3 == 2 else int(x) for j, x in enumerate(out)]


def check_zerocheck(pkg, p, s, seed):
    ctx = ctx_of(pkg, p)
    rng = np.random.default_rng(seed)
    tabs = [ww.edge_table(p, 1 << s, rng) for _ in range(3)]
    dev = [pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, s, t) for t in tabs]
    tau, ch = challenge_words(p, s, rng), challenge_words(p, s, rng)[::-1]
    c1, rounds, got_ch, finals = pkg.r1cs.zerocheck_prove(ctx, *dev, tau, lambda j, e: ch[j])
    w_c1, w_rounds, w_finals = ref.zerocheck(*[canon_np(p, t) for t in tabs], lref.canon(p, tau), lref.canon(p, ch), p)
    assert got_ch == ch
    assert lref.canon(p, [c1])[0] == w_c1
    assert [lref.canon(p, e) for e in rounds] == w_rounds
    assert tuple(lref.canon(p, finals)) == w_finals
    for d, t in zip(dev, tabs):
        assert np.array_equal(d.to_evaluations(), t)          # the inputs are unchanged


@pytest.mark.parametrize("s", range(1, 15))
def test_zerocheck_bit_for_bit_goldilocks(pkg, s):
    check_zerocheck(pkg, GOLD, s, s)


@pytest.mark.parametrize("p", [P64, P61], ids=["p64m59", "p61m1"])
@pytest.mark.parametrize("s", [1, 2, 7, 13])
def test_zerocheck_bit_for_bit_generic(pkg, p, s):
    check_zerocheck(pkg, p, s, 50 + s)


def test_zerocheck_synthetic_challenger_is_sc_proves(pkg):
    p, s = GOLD, 6
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    dev = [pkg.DenseMultilinearExtension.generate(ctx, 10 + k, s) for k in range(3)]
    _, _, ch, _ = pkg.r1cs.zerocheck_prove(ctx, *dev, [F.one] * s, None, seed_r=99)
    _, _, want = pkg.matrix_multiplication.prove(ctx, pkg.matrix_multiplication.G(dev[0], dev[1]), 99)
    assert ch == [int(x) for x in want]


def test_zerocheck_at_2_to_20(pkg):
    """the reference is out of reach: the transcript passes the host's round checks, and the finals are sc_table_evaluate of the
    inputs at the challenges (kernels that share no code with the cubic pass)"""
    p, s = GOLD, 20
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    rng = random.Random(20)
    dev = [pkg.DenseMultilinearExtension.generate(ctx, 30 + k, s) for k in range(3)]
    tau = [F.rand(rng) for _ in range(s)]
    c1, rounds, ch, finals = pkg.r1cs.zerocheck_prove(ctx, *dev, tau, lambda j, e: F.rand(rng))
    claim = lref.canon(p, [c1])[0]
    cch, ctau = lref.canon(p, ch), lref.canon(p, tau)
    for e, r in zip(rounds, cch):
        e = lref.canon(p, e)
        assert (e[0] + e[1]) % p == claim
        claim = ref.cubic_at(e, r, p)
    assert list(finals) == [d.evaluate(ch) for d in dev]
    va, vb, vc = lref.canon(p, finals)
    eq = 1
    for t, r in zip(ctau, cch):
        eq = eq * (t * r + (1 - t) * (1 - r)) % p
    assert eq * (va * vb - vc) % p == claim


# ---- the whole argument ----------------------------------------------------------------------------------------------

QUERIES = 8


class Tampering:
    """a Prover whose one named message is corrupted on its way to the verifier"""

    def __init__(self, prover, tamper):
        self.inner, self.tamper, self.F = prover, tamper, prover.field
        self.pcs = self if tamper == "column" else prover.pcs

    def _draw(self, draw, k):
        def d(j, e):
            if j == 0:
                e = list(e)
                e[k] = self.F.add(e[k], self.F.one)
            return draw(j, e)
        return d

    def sumcheck1(self, tau, draw):
        sc1 = self.tamper.startswith("sc1_")
        fin = self.inner.sumcheck1(tau, self._draw(draw, int(self.tamper[4:])) if sc1 else draw)
        return (self.F.add(fin[0], self.F.one),) + tuple(fin[1:]) if self.tamper == "v_A" else fin

    def bind(self, rho):
        self.inner.bind(rho)

    def sumcheck2(self, draw):
        self.inner.sumcheck2(self._draw(draw, 2) if self.tamper == "sc2" else draw)

    # the commitment's prover with one column word off
    def combine(self, point, gamma):
        return self.inner.pcs.combine(point, gamma)

    def open_columns(self, indices):
        out = self.inner.pcs.open_columns(indices)
        j, vals, path = out[1]
        out[1] = (j, [self.F.add(vals[0], self.F.one)] + vals[1:], path)
        return out


def argue(pkg, p, s, m, seed, opening="plain", tamper=None):
    rp, lp = pkg.r1cs, pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    R, io, w = rp.synthetic_instance(F, s, m, seed)
    if tamper == "w":
        col = R.matrices[0][0][1]
        col = col - (1 << (m - 1)) if col >= 1 << (m - 1) else next(j for _, j, _ in R.matrices[0] + R.matrices[1] if j >= 1 << (m - 1)) - (1 << (m - 1))
        w = list(w)
        w[col] = F.add(w[col], F.one)
    dev = rp.DeviceR1CS(ctx, R)
    code = "expander" if opening == "expander" else "rs"
    c = max(1, m // 2) if opening == "folded" else m // 2
    prover = rp.Prover(ctx, dev, io, w, log_cols=c, log_blowup=1, code=code)
    root = prover.root()
    if opening == "folded":
        pv = lp.FoldVerifier(F, m - 1, c, 1, root, QUERIES)
    else:
        pv = lp.Verifier(F, m - 1, c, 1, root, QUERIES, code=code)
    verifier = rp.Verifier(R, io, root, pv)
    rng = random.Random(seed + 1)
    try:
        if tamper == "opened":
            P = prover
            fin = P.sumcheck1(verifier.draw_tau(rng), lambda j, e: verifier.round1(j, e, rng))
            verifier.receive_finals(*fin)
            P.bind(verifier.draw_rho(rng))
            P.sumcheck2(lambda j, e: verifier.round2(j, e, rng))
            return verifier.finish(F.add(rp.open_committed(P.pcs, pv, verifier.point(), rng), F.one))
        return rp.prove_and_verify(Tampering(prover, tamper) if tamper and tamper != "w" else prover, verifier, rng)
    finally:
        prover.close()
        dev.close()


@pytest.mark.parametrize("p,opening", [(GOLD, "plain"), (GOLD, "folded"), (P64, "expander")], ids=["gold-plain", "gold-folded", "p64m59-expander"])
@pytest.mark.parametrize("s,m", [(1, 2), (3, 3), (6, 5), (5, 8), (10, 11), (12, 12)])
def test_the_whole_argument_is_accepted(pkg, p, opening, s, m):
    assert argue(pkg, p, s, m, 31 * s + m, opening) is True


@pytest.mark.parametrize("p,opening", [(GOLD, "plain"), (P64, "expander")], ids=["gold-plain", "p64m59-expander"])
def test_tampered_device_messages_are_refused(pkg, p, opening):
    rp, lp = pkg.r1cs, pkg.ligero_pcs
    s, m = 6, 5

    def refused(tamper, err, **attrs):
        with pytest.raises(err) as ei:
            argue(pkg, p, s, m, 11, opening, tamper)
        for k, v in attrs.items():
            assert getattr(ei.value, k) == v, (tamper, k, getattr(ei.value, k))

    refused("w", rp.RoundMismatch, phase=1, round=0)
    refused("sc1_0", rp.RoundMismatch, phase=1, round=0)
    refused("sc1_1", rp.RoundMismatch, phase=1, round=0)
    refused("sc1_2", rp.RoundMismatch, phase=1, round=1)
    refused("sc1_3", rp.RoundMismatch, phase=1, round=1)
    refused("v_A", rp.FinalMismatch, phase=1)
    refused("sc2", rp.RoundMismatch, phase=2, round=1)
    refused("opened", rp.FinalMismatch, phase=2)
    refused("column", lp.MerkleMismatch)


# ---- refusals and the pool's books -----------------------------------------------------------------------------------

def pool(ctx):
    return ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")


def raw_create(pkg, ctx, s, m, mats):
    arrays = [(np.array([t[0] for t in M], dtype=np.uint32), np.array([t[1] for t in M], dtype=np.uint32), np.array([t[2] for t in M], dtype=np.uint64))
              for M in mats]
    h = ctypes.c_void_p()
    rc = pkg.r1cs.DeviceR1CS.create(ctx, s, m, arrays, h)
    assert (rc == 0) == bool(h.value)
    return rc, h


def test_refusals(pkg):
    p = GOLD
    ctx, F, lib = ctx_of(pkg, p), pkg.Field(p), ctx_of(pkg, GOLD).lib
    rp = pkg.r1cs
    gc.collect()
    base = pool(ctx)
    ok = [(0, 1, F.one)]
    for s, m in ((0, 3), (27, 3), (3, 1), (3, 27)):
        assert raw_create(pkg, ctx, s, m, (ok, [], []))[0] == 1, (s, m)
    for bad in ((8, 0, F.one), (0, 8, F.one), (0, 0, p)):                      # row >= 2^s, col >= 2^m, val >= p
        for k in range(3):
            mats = [ok, ok, ok]
            mats[k] = ok * 5 + [bad]
            assert raw_create(pkg, ctx, 3, 3, mats)[0] == 1, (bad, k)
    assert "entry 5 of matrix 2" in lib.sc_last_error(ctx.h).decode()
    # nnz >= 2^31 is refused before any array is read; NULL arguments
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    nul32, nul64 = (u32p * 3)(), (u64p * 3)()
    h = ctypes.c_void_p()
    assert lib.sc_r1cs_create(ctx.h, 3, 3, nul32, nul32, nul64, (ctypes.c_size_t * 3)(0, 1 << 31, 0), ctypes.byref(h)) == 1
    assert "2^31" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_r1cs_create(ctx.h, 3, 3, nul32, nul32, nul64, (ctypes.c_size_t * 3)(0, 1, 0), ctypes.byref(h)) == 1
    assert lib.sc_r1cs_create(ctx.h, 3, 3, None, nul32, nul64, (ctypes.c_size_t * 3)(), ctypes.byref(h)) == 1
    assert lib.sc_r1cs_create(ctx.h, 3, 3, nul32, nul32, nul64, (ctypes.c_size_t * 3)(), None) == 1
    gc.collect()
    assert pool(ctx) == base                                                   # a failed create leaves nothing behind
    dev = rp.DeviceR1CS(ctx, rp.R1CS(F, 3, 3, ok, ok, ok))
    z4 = pkg.DenseMultilinearExtension.generate(ctx, 1, 4)
    t3 = [pkg.DenseMultilinearExtension.generate(ctx, k, 3) for k in range(3)]
    expect(pkg, 1, lambda: dev.mul(z4), "z has 16 entries")
    expect(pkg, 1, lambda: dev.bind_rows([p, 0, 0], [1, 1, 1]), "rx[0]")
    expect(pkg, 1, lambda: dev.bind_rows([0, 0, 0], [1, p, 1]), "rho[1]")
    expect(pkg, 1, lambda: rp.zerocheck_prove(ctx, t3[0], t3[1], z4, [1, 1, 1]), "equal")
    expect(pkg, 1, lambda: rp.zerocheck_prove(ctx, *t3, [1, p, 1]), "tau[1]")
    expect(pkg, 1, lambda: rp.zerocheck_prove(ctx, *t3, [1, 1, 1], lambda j, e: p), "unreduced")
    fin = (ctypes.c_uint64 * 3)()
    c1 = ctypes.c_uint64()
    no_draw = ctypes.cast(None, pkg._lib.DRAW4_FN)
    tau = (ctypes.c_uint64 * 3)(1, 1, 1)
    assert lib.sc_zerocheck_prove(ctx.h, t3[0].h, t3[1].h, t3[2].h, None, no_draw, None, 0, ctypes.byref(c1), None, None, fin) == 1
    assert lib.sc_zerocheck_prove(ctx.h, t3[0].h, None, t3[2].h, tau, no_draw, None, 0, ctypes.byref(c1), None, None, fin) == 1
    assert lib.sc_zerocheck_prove(ctx.h, t3[0].h, t3[1].h, t3[2].h, tau, no_draw, None, 0, ctypes.byref(c1), None, None, None) == 1
    assert lib.sc_zerocheck_prove(ctx.h, t3[0].h, t3[1].h, t3[2].h, tau, no_draw, None, 0, ctypes.byref(c1), None, None, fin) == 0
    # p = 3: the cubic through 0 .. 3 does not exist
    c3 = pkg.Context(pkg.Field(3))
    s3 = [pkg.DenseMultilinearExtension.from_evaluations_vec(c3, 1, np.array([1, 2], dtype=np.uint64)) for _ in range(3)]
    expect(pkg, 6, lambda: rp.zerocheck_prove(c3, *s3, [1]), "p = 3")
    del s3
    c3.close()
    # a multi-device handle and a sharded context: refused in the words of the commitments
    words = F.from_ints(range(8))
    for make, needle in ((lambda: pkg.Context(F, devices=[0, 0]), "a multi-device handle"), (None, "sharded")):
        if make:
            other = make()
        else:
            other = pkg.Context(F)
            ar, ag = Loopback(2).collectives(0)
            other.comm_init_host(0, 2, ar, ag)
        msg = "runs on a context of one device and one rank (this one is %s)" % needle
        rc, _ = raw_create(pkg, other, 3, 3, (ok, ok, ok))
        assert rc == 6 and ("sc_r1cs_create: " + msg) in other.lib.sc_last_error(other.h).decode()
        ot = [pkg.DenseMultilinearExtension.from_evaluations_vec(other, 3, words) for _ in range(3)]
        expect(pkg, 6, lambda: rp.zerocheck_prove(other, *ot, [1, 1, 1]), "sc_zerocheck_prove: " + msg)
        out = [ctypes.c_void_p() for _ in range(3)]
        assert other.lib.sc_r1cs_mul(other.h, dev.h, ot[0].h, *[ctypes.byref(x) for x in out]) == 6
        rx = (ctypes.c_uint64 * 3)(1, 1, 1)
        assert other.lib.sc_r1cs_bind_rows(other.h, dev.h, rx, rx, ctypes.byref(out[0])) == 6 and not out[0].value
        del ot
        other.close()
    del z4, t3
    dev.close()
    gc.collect()
    assert pool(ctx) == base


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p):
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    gc.collect()
    base = pool(ctx)
    assert argue(pkg, p, 6, 5, 3, "plain" if p == GOLD else "expander") is True
    gc.collect()
    assert pool(ctx) == base, "after an accepted argument"

    class Boom(Exception):
        pass

    def raising(j, e):
        if j == 2:
            raise Boom()
        return F.one
    tabs = [pkg.DenseMultilinearExtension.generate(ctx, k, 8) for k in range(3)]
    mid = pool(ctx)
    with pytest.raises(Boom):
        pkg.r1cs.zerocheck_prove(ctx, *tabs, [F.one] * 8, raising)
    assert pool(ctx) == mid, "after a draw that raised"
    # the context still proves
    pkg.r1cs.zerocheck_prove(ctx, *tabs, [F.one] * 8)
    del tabs
    gc.collect()
    assert pool(ctx) == base
