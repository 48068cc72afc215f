"""GPU: SPARK over LogUp (sc_spark_*, sc_product3_prove, sc_table_eq, sc_r1cs_row_weights; thaler-study_amd/spark.py and the
sublinear verifier of r1cs.py) against numpy and the big-integer reference of tests/spark_ref.py, word for word: the five tables
of a matrix at the last LDS-histogram size and the first global one, the gather and the tuples on edge words, the triple-product
proof at every hand-over to the host, the whole exchange over Ligero commitments (plain, folded, expander code) with every single
tamper of the device's messages, the R1CS argument next to the one whose verifier reads the instance, the refusals and the pool's
books."""
import ctypes
import gc
import random

import numpy as np
import pytest

import spark_cases as cases
import spark_ref as ref
import wide_words as ww
from conftest import load_package
from ligero_common import context_cache, expect, mont_np
from spark_cases import GOLD, P61, P64
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu
SPARK = load_package().spark            # (the module under test: without it nothing here can run)

ctx_of, teardown_module = context_cache()
QUERIES = 8
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1"}
LDS_LOG = 13         # kLookupLdsLog: histograms of up to 2^13 counters are kept in LDS
MISMATCH_SEED = 2025


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


def bare(pkg, ctx, a, b, rows, cols, vals):
    """the device object alone, without commitments"""
    return pkg.spark.SparseCommitment(ctx, a, b, rows, cols, vals, commit=False)


# ---- sc_spark_create / sc_spark_table ----------------------------------------------------------------------------------

def padded(rows, cols, vals):
    ell = ref.log_len(len(rows))
    N = 1 << ell
    out = []
    for x, dt in ((rows, np.int64), (cols, np.int64), (vals, np.uint64)):
        full = np.zeros(N, dtype=dt)
        full[:len(x)] = x
        out.append(full)
    return (ell,) + tuple(out)


def check_tables(pkg, p, a, b, rows, cols, vals, what):
    ctx = ctx_of(pkg, p)
    ell, prow, pcol, pval = padded(rows, cols, vals)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    sc = bare(pkg, ctx, a, b, rows, cols, vals)
    log = [(x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in ctx.launch_log() if x["kind"] == "spark_index"]
    ctx.set_option("time_kernels", 0)
    want_log = []
    for m in (a, b):
        want_log += [(0, 1 if m <= LDS_LOG else 0, ell, 4 << ell, (8 << ell) + (4 << m)), (1, 0, m, 4 << m, 8 << m)]
    assert log == want_log, what
    assert sc.ell == ell
    want = {"row": mont_np(p, prow), "col": mont_np(p, pcol), "val": pval, "cr": mont_np(p, np.bincount(prow, minlength=1 << a)),
            "cc": mont_np(p, np.bincount(pcol, minlength=1 << b))}
    for name in pkg.spark.TABLES:
        got = sc.table(name).to_evaluations()
        assert got.shape == want[name].shape and np.array_equal(got, want[name]), (what, name)
    sc.close()


@pytest.mark.parametrize("a,b", [(1, 1), (5, 8), (13, 13), (14, 12)], ids=["1-1", "5-8", "13-13", "14-12"])
def test_create_builds_the_five_tables(pkg, a, b):
    """(13, 13) is the last size counted in LDS histograms, (14, 12) has the first counted in global memory; nnz = 1, 2, 3 pad a
    list shorter than a thread's unit, 2^10 + 1 and 2^13 - 1 pad by almost a half and by one"""
    p = GOLD
    rng = np.random.default_rng(100 * a + b)
    for nnz in (1, 2, 3, 1 << 10, (1 << 10) + 1, (1 << 13) - 1):
        rows, cols = rng.integers(0, 1 << a, size=nnz), rng.integers(0, 1 << b, size=nnz)
        vals = ww.edge_table(p, nnz, rng)
        check_tables(pkg, p, a, b, rows, cols, vals, "uniform %d" % nnz)
    nnz = 1000
    vals = ww.edge_table(p, nnz, rng)
    last_row, last_col = np.full(nnz, (1 << a) - 1), np.full(nnz, (1 << b) - 1)
    check_tables(pkg, p, a, b, last_row, rng.integers(0, 1 << b, size=nnz), vals, "one row")
    check_tables(pkg, p, a, b, rng.integers(0, 1 << a, size=nnz), last_col, vals, "one column")
    check_tables(pkg, p, a, b, last_row, last_col, vals, "one (row, col) pair")
    check_tables(pkg, p, a, b, np.zeros(nnz, dtype=np.int64), np.zeros(nnz, dtype=np.int64), vals, "the padding's own pair")
    # the count merges runs of one index: runs of four (a thread's unit) that differ from thread to thread, and runs of 256 and
    # more (whole waves) next to a wave that holds two indices
    fours = np.repeat(rng.integers(0, 1 << a, size=nnz // 4), 4)
    waves = np.concatenate([np.full(256, 1), np.full(128, 0), np.full(128, (1 << a) - 1), np.full(nnz - 512, 1)])
    check_tables(pkg, p, a, b, fours, rng.integers(0, 1 << b, size=nnz), vals, "runs of four")
    check_tables(pkg, p, a, b, waves, np.minimum(waves, (1 << b) - 1), vals, "runs of whole waves")


def test_create_over_a_generic_field(pkg):
    p = P64
    rng = np.random.default_rng(3)
    for a, b, nnz in ((1, 1, 2), (5, 8, 777), (14, 12, 5000)):
        check_tables(pkg, p, a, b, rng.integers(0, 1 << a, size=nnz), rng.integers(0, 1 << b, size=nnz), ww.edge_table(p, nnz, rng), (a, b, nnz))


# ---- sc_spark_gather ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
@pytest.mark.parametrize("ell", [1, 2, 3, 10, 13])
def test_gather_word_for_word(pkg, p, ell):
    """l = 1 is the tail (a list of two is smaller than a thread's unit), l = 2 one thread, l = 3 two, l = 13 more than one block"""
    ctx = ctx_of(pkg, p)
    rng = np.random.default_rng(ell)
    for a, b, nnz in ((1, 1, 1 << ell), (7, 5, 1 << ell), (ell, max(1, ell - 1), (1 << ell) - (1 if ell > 1 else 0)), (9, 14, 1 if ell == 1 else (1 << (ell - 1)) + 1)):
        rows, cols = rng.integers(0, 1 << a, size=nnz), rng.integers(0, 1 << b, size=nnz)
        if nnz >= 2:
            rows[0], cols[0], rows[-1], cols[-1] = (1 << a) - 1, 0, 0, (1 << b) - 1
        Uw, Ww = ww.edge_table(p, 1 << a, rng), ww.edge_table(p, 1 << b, rng)
        _, prow, pcol, _ = padded(rows, cols, np.zeros(nnz, dtype=np.uint64))
        sc = bare(pkg, ctx, a, b, rows, cols, ww.edge_table(p, nnz, rng))
        assert sc.ell == ell
        U, W = upload(pkg, ctx, Uw), upload(pkg, ctx, Ww)
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
        er, ec = pkg.spark.gather(ctx, sc, U, W)
        log = [x for x in ctx.launch_log() if x["kind"] == "spark_gather"]
        ctx.set_option("time_kernels", 0)
        assert [(x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log] == [(ell, 24 << ell, 16 << ell)]
        assert np.array_equal(er.to_evaluations(), Uw[prow]) and np.array_equal(ec.to_evaluations(), Ww[pcol]), (a, b, nnz)
        assert np.array_equal(U.to_evaluations(), Uw) and np.array_equal(W.to_evaluations(), Ww), "the inputs are unchanged"
        sc.close()


# ---- sc_spark_denominators ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_denominators_word_for_word(pkg, p):
    """alpha, beta from {0, 1, p - 1, random}; (1, 1) with two entries: both launches take the tail; (5, 8) with 1000 entries: the
    key stream and the index as key over more than one thread; (13, 2) with 2^13 entries: more than one block"""
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    rng = np.random.default_rng(11)
    pick = random.Random(4)
    for a, b, nnz in ((1, 1, 2), (5, 8, 1000), (13, 2, 1 << 13)):
        rows, cols = rng.integers(0, 1 << a, size=nnz), rng.integers(0, 1 << b, size=nnz)
        ell, prow, pcol, _ = padded(rows, cols, np.zeros(nnz, dtype=np.uint64))
        sc = bare(pkg, ctx, a, b, rows, cols, ww.edge_table(p, nnz, rng))
        tables = {"row": (ww.edge_table(p, 1 << a, rng), prow), "col": (ww.edge_table(p, 1 << b, rng), pcol)}
        ew = ww.edge_table(p, 1 << ell, rng)
        e = upload(pkg, ctx, ew)
        e_c = ref.canon_list(ew, p)
        combos = [(x, y) for x in (0, 1, p - 1, None) for y in (0, 1, p - 1, None)]
        if nnz > 2:
            combos = [combos[k] for k in (0, 5, 10, 15, 3, 12)]
        for dim, (tw, idx) in tables.items():
            t = upload(pkg, ctx, tw)
            t_c = ref.canon_list(tw, p)
            for alpha, beta in combos:
                alpha = pick.randrange(p) if alpha is None else alpha
                beta = pick.randrange(p) if beta is None else beta
                ctx.set_option("time_kernels", 1)
                ctx.launch_log()
                den_w, den_t = pkg.spark.denominators(ctx, sc, dim, t, e, ref.mont(alpha, p), ref.mont(beta, p))
                log = [(x["kf"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in ctx.launch_log() if x["kind"] == "spark_tuple"]
                ctx.set_option("time_kernels", 0)
                m = a if dim == "row" else b
                assert log == [(0, ell, 12 << ell, 8 << ell), (1, m, 8 << m, 8 << m)]
                want_w, want_t = ref.denominators([int(i) for i in idx], e_c, t_c, alpha, beta, p)
                assert np.array_equal(den_w.to_evaluations(), mont_np(p, want_w)), (a, b, dim, alpha, beta)
                assert np.array_equal(den_t.to_evaluations(), mont_np(p, want_t)), (a, b, dim, alpha, beta)
            assert np.array_equal(t.to_evaluations(), tw) and np.array_equal(e.to_evaluations(), ew), "the inputs are unchanged"
        sc.close()


# ---- sc_product3_prove -------------------------------------------------------------------------------------------------

_REF = {}


def p3_reference(p, n, seed):
    """(three tables of words, canonical challenges, reference (c1, rounds, challenges, finals)): computed once, shared, never changed"""
    key = (p, n, seed)
    if key not in _REF:
        rng = np.random.default_rng(seed)
        tabs = [ww.edge_table(p, 1 << n, rng) for _ in range(3)]
        pick = random.Random(seed + 1)
        ch = [pick.choice([0, 1, p - 1, pick.randrange(p)]) for _ in range(n)]
        it = iter(ch)
        _REF[key] = (tabs, ch, ref.product3_prove(*[ref.canon_list(t, p) for t in tabs], p, lambda j, msg: next(it)))
    return _REF[key]


def p3_device(pkg, p, tabs, ch_canon, T):
    """sc_product3_prove at gp_host_log = T under the fixed challenges; the draw also checks the order it is called in"""
    ctx = ctx_of(pkg, p)
    words = ref.mont_list(ch_canon, p)
    seen = []

    def draw(j, msg):
        assert len(msg) == 4
        seen.append(j)
        return words[j]
    base = host_log(pkg, p)
    dev = [upload(pkg, ctx, t) for t in tabs]
    ctx.set_option("gp_host_log", T)
    try:
        out = pkg.spark.product3_prove(ctx, *dev, draw)
    finally:
        ctx.set_option("gp_host_log", base)
    assert seen == list(range(len(ch_canon)))
    for d, t in zip(dev, tabs):
        assert np.array_equal(d.to_evaluations(), t), "the inputs are never written"
    return out


P3_SIZES = [(GOLD, n) for n in range(1, 15)] + [(p, n) for p in (P64, P61) for n in (1, 2, 7, 13)]


@pytest.mark.parametrize("p,n", P3_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in P3_SIZES])
def test_product3_is_the_reference_bit_for_bit(pkg, p, n):
    """gp_host_log = 0 (every round but the last on the device) and the default; at n = 5 and 9 on Goldilocks also 1, 3, n - 1 (the
    hand-over at the first possible launch), n (no device round at all) and 12 (above n).  Edge-word tables, challenges from
    {0, 1, p - 1, random}"""
    tabs, ch, (c1, rounds, rs, finals) = p3_reference(p, n, 900 + n)
    want = (ref.mont(c1, p), [ref.mont_list(m, p) for m in rounds], ref.mont_list(rs, p), tuple(ref.mont_list(finals, p)))
    extra = (1, 3, n - 1, n, 12) if p == GOLD and n in (5, 9) else ()
    outs = [p3_device(pkg, p, tabs, ch, T) for T in sorted(set([0, host_log(pkg, p)]) | set(extra))]
    for out in outs:
        assert out == want
    assert all(o == outs[0] for o in outs[1:]), "transcripts at different gp_host_log are identical"


def test_product3_at_2_to_20(pkg):
    """the reference is out of reach: the transcript passes the verifier's round checks, and the finals are sc_table_evaluate of
    the three tables at the challenges"""
    p, n = GOLD, 20
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    tabs = [pkg.DenseMultilinearExtension.generate(ctx, 30 + k, n) for k in range(3)]
    c1, rounds, ch, finals = pkg.spark.product3_prove(ctx, *tabs, seed_r=5)
    assert len(rounds) == len(ch) == n
    V = pkg.grand_product.Verifier(F, 2)
    claim = c1
    for msg, r in zip(rounds, ch):
        assert F.add(msg[0], msg[1]) == claim
        claim = V._cubic_at(msg, r)
    assert F.mul(F.mul(finals[0], finals[1]), finals[2]) == claim
    assert finals == tuple(t.evaluate(ch) for t in tabs)
    # the synthetic challenger is sc_prove's: a draw that returns the same words sees the same transcript
    assert pkg.spark.product3_prove(ctx, *tabs, draw=lambda j, msg: ch[j]) == (c1, rounds, ch, finals)


def test_product3_launch_log(pkg):
    """one launch per device round: round 0 reads the caller's tables, every later one folds; the rounds of the last
    2^max(T, 1) entries leave no record"""
    p, n = GOLD, 13
    ctx, T = ctx_of(pkg, p), host_log(pkg, p)
    tabs = [pkg.DenseMultilinearExtension.generate(ctx, 40 + k, n) for k in range(3)]
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    pkg.spark.product3_prove(ctx, *tabs, seed_r=1)
    log = [x for x in ctx.launch_log() if x["kind"] == "product_pass"]
    ctx.set_option("time_kernels", 0)
    te = max(T, 1)
    want = [(0, n, 1)] + [(1, n - j + 1, 1) for j in range(1, n - te + 1)]
    assert n > te and [(x["kf"], x["log_in"], x["ks"]) for x in log] == want
    for x in log:
        assert x["bytes_read"] == 24 << x["log_in"] and x["bytes_written"] == ((24 << (x["log_in"] - 1)) if x["kf"] else 0)


# ---- sc_table_eq, sc_r1cs_row_weights ----------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_table_eq_and_row_weights(pkg, p):
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    pick = random.Random(2)
    for n in (1, 2, 5, 11):
        r = [pick.choice([0, 1, p - 1, pick.randrange(p)]) for _ in range(n)]
        got = pkg.spark.table_eq(ctx, ref.mont_list(r, p)).to_evaluations()
        assert np.array_equal(got, mont_np(p, ref.eq_table(r, p))), n
    for s, m in ((1, 2), (6, 5)):
        R, _, _ = pkg.r1cs.synthetic_instance(F, s, m, 3)
        dev = pkg.r1cs.DeviceR1CS(ctx, R)
        rx, rho = [pick.randrange(p) for _ in range(s)], [0, 1, pick.randrange(p)]
        got = dev.row_weights(ref.mont_list(rx, p), ref.mont_list(rho, p)).to_evaluations()
        ex = ref.eq_table(rx, p)
        assert np.array_equal(got, mont_np(p, [rk * e % p for rk in rho for e in ex] + [0] * (1 << s)))
        dev.close()


# ---- prove_eval --------------------------------------------------------------------------------------------------------

def eval_case(pkg, p, a, b, ell, seed, code):
    """a matrix of 2^l - 3 entries (padded), U = eq(r_x, .) and W = eq(r_y, .): the claim is M~(r_x, r_y)"""
    ctx = ctx_of(pkg, p)
    triples, _, _ = cases.case(p, a, b, (1 << ell) - 3, seed)
    pick = random.Random(seed)
    rx, ry = [pick.randrange(p) for _ in range(a)], [pick.randrange(p) for _ in range(b)]
    rows, cols, vals = [t[0] for t in triples], [t[1] for t in triples], mont_np(p, [t[2] for t in triples])
    sc = pkg.spark.SparseCommitment(ctx, a, b, rows, cols, vals, commit=pkg.spark.default_commit(code=code))
    U, W = pkg.spark.table_eq(ctx, ref.mont_list(rx, p)), pkg.spark.table_eq(ctx, ref.mont_list(ry, p))
    ex, ey = ref.eq_table(rx, p), ref.eq_table(ry, p)
    want = sum(v * ex[i] * ey[j] for i, j, v in triples) % p
    return sc, U, W, (triples, ex, ey, rx, ry), want


def eq_eval(pkg, p, point):
    """z -> eq(point, z) in Montgomery words, as a verifier computes it: O(len) field operations"""
    F = pkg.Field(p)
    at = ref.mont_list(point, p)

    def f(z):
        out = F.one
        for x, y in zip(at, z):
            xy = F.mul(x, int(y))
            out = F.mul(out, F.add(F.sub(F.sub(F.one, x), int(y)), F.add(xy, xy)))
        return out
    return f


EVALS = [(GOLD, 8, 8, 10, "rs", False), (GOLD, 8, 8, 10, "rs", True), (GOLD, 10, 6, 12, "rs", False), (GOLD, 10, 6, 12, "rs", True),
         (P64, 6, 6, 8, "expander", False)]


@pytest.mark.parametrize("p,a,b,ell,code,folded", EVALS, ids=["gold-8-8-10-plain", "gold-8-8-10-folded", "gold-10-6-12-plain", "gold-10-6-12-folded",
                                                              "p64m59-6-6-8-expander"])
def test_prove_eval_is_accepted(pkg, p, a, b, ell, code, folded):
    ctx = ctx_of(pkg, p)
    gc.collect()
    base = pool(ctx)
    sc, U, W, (_, _, _, rx, ry), want = eval_case(pkg, p, a, b, ell, 10 * a + ell, code)
    assert sc.ell == ell and sorted(sc.roots()) == sorted(pkg.spark.TABLES) and all(len(r) == 32 for r in sc.roots().values())
    v = pkg.spark.prove_eval(sc, sc.verifiers(QUERIES, folded), U, W, eq_eval(pkg, p, rx), eq_eval(pkg, p, ry), random.Random(17))
    assert v == ref.mont(want, p), "the accepted value is M~(r_x, r_y)"
    sc.close()
    del sc, U, W
    gc.collect()
    assert pool(ctx) == base, "after close()"


class Tampering:
    """a spark.Prover whose one named message is changed on its way"""

    def __init__(self, inner, F, what):
        self.inner, self.F, self.what = inner, F, what
        self.pcs = inner.pcs

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def bump(self, x):
        return self.F.add(int(x), self.F.one)

    def sumcheck(self, receive_claim, draw):
        kind = self.what[0]

        def claim(v):
            receive_claim(self.bump(v) if kind == "v" else v)

        def relay(j, e):
            if kind == "round" and j == self.what[1]:
                e = list(e)
                e[self.what[2]] = self.bump(e[self.what[2]])
            return draw(j, e)
        fin = list(self.inner.sumcheck(claim, relay))
        if kind == "final":
            fin[self.what[1]] = self.bump(fin[self.what[1]])
        return tuple(fin)

    def lookup_roots(self, dim, alpha, beta):
        rw, rt = self.inner.lookup_roots(dim, alpha, beta)
        if self.what == ("root", dim):
            rw = (self.bump(rw[0]), rw[1])
        return rw, rt


def exchange(pkg, sc, U, W, u_eval, w_eval, seed, what=None, prover=None):
    """prove_eval's steps by hand (plain openings), with one message changed: what = ("v",) | ("round", j, t) | ("final", k) |
    ("root", dim) | ("open", table, at)"""
    sp, F = pkg.spark, sc.ctx.field
    from_prover = lambda pr: sp.opening_verifier(F, pr, QUERIES)   # noqa: E731
    rng = random.Random(seed)
    V = sp.Verifier(F, sc.a, sc.b, sc.ell, sc.verifiers(QUERIES), u_eval, w_eval)
    inner = prover or sp.Prover(sc, U, W)
    P = Tampering(inner, F, what) if what else inner
    try:
        inner.gather_commit()
        V.receive_commitments(from_prover(inner.pcs["er"]), from_prover(inner.pcs["ec"]))
        V.receive_finals(*P.sumcheck(V.receive_claim, lambda j, e: V.round(j, e, rng)))
        alpha, beta = V.draw_lookup(rng)
        for dim in sp.DIMS:
            V.receive_roots(dim, *P.lookup_roots(dim, alpha, beta))
            for side in range(2):
                inner.lookup_prove(dim, side, V.frac[dim][side].challenger(rng))
        opened = {}
        for table, at, point in V.openings():
            ver = V.pcs[table] if table in sp.TABLES else from_prover(inner.pcs[table])
            opened[(table, at)] = pkg.r1cs.open_committed(inner.pcs[table], ver, point, rng)
            if what == ("open", table, at):
                opened[(table, at)] = F.add(opened[(table, at)], F.one)
        return V.finish(opened)
    finally:
        inner.close()


def test_tampered_device_messages_are_refused(pkg):
    """every single tamper of the device's messages meets its own error.  The challenges come from a random.Random over
    Goldilocks: one of the interpolation points 0 .. 3 among the l of them has probability 2^-60"""
    p, a, b, ell = GOLD, 5, 4, 6
    sp = pkg.spark
    sc, U, W, (_, _, _, rx, ry), _ = eval_case(pkg, p, a, b, ell, 3, "rs")
    ue, we = eq_eval(pkg, p, rx), eq_eval(pkg, p, ry)
    F = pkg.Field(p)
    assert exchange(pkg, sc, U, W, ue, we, 5) is True

    def refused(err, attrs, what=None, **kwargs):
        with pytest.raises(err) as ei:
            exchange(pkg, sc, U, W, kwargs.get("ue", ue), kwargs.get("we", we), 5, what)
        assert type(ei.value) is err
        for k, want in attrs.items():
            assert getattr(ei.value, k) == want, (what, k)
    refused(sp.RoundMismatch, {"round": 0}, ("v",))
    for j in (0, ell // 2, ell - 1):
        for t in range(4):
            if t < 2:
                refused(sp.RoundMismatch, {"round": j}, ("round", j, t))
            elif j + 1 < ell:
                refused(sp.RoundMismatch, {"round": j + 1}, ("round", j, t))
            else:
                refused(sp.FinalMismatch, {}, ("round", j, t))
    for k in range(3):
        refused(sp.FinalMismatch, {}, ("final", k))
    for dim in sp.DIMS:
        refused(sp.LookupMismatch, {"dim": dim}, ("root", dim))
    which = {("val", "r"): "val", ("er", "r"): "er", ("ec", "r"): "ec", ("er", "z_row"): "den_w row", ("row", "z_row"): "den_w row",
             ("ec", "z_col"): "den_w col", ("col", "z_col"): "den_w col", ("cr", "zt_row"): "cr", ("cc", "zt_col"): "cc"}
    for (table, at), name in which.items():
        refused(sp.InputMismatch, {"which": name}, ("open", table, at))
    refused(sp.InputMismatch, {"which": "u"}, ue=lambda z: F.add(ue(z), F.one))
    refused(sp.InputMismatch, {"which": "w"}, we=lambda z: F.add(we(z), F.one))
    sc.close()


def mismatch_case(p):
    """(a, b, triples, U, W, the prover's er with one word changed, alpha, beta) in canonical integers: the case of the refused
    lookup below, with the beta and alpha MISMATCH_SEED draws (after the l = 10 challenges of the sumcheck)"""
    a, b, ell = 6, 5, 10
    triples, U, W = cases.case(p, a, b, 1000, 77)
    _, rows, _, _ = ref.pad(triples)
    er = [U[i] for i in rows]
    er[321] = (er[321] + 1) % p
    rng = random.Random(MISMATCH_SEED)
    for _ in range(ell):
        rng.randrange(p)                                   # Field.rand of a random.Random: one randrange(p), canonical
    beta = rng.randrange(p)
    alpha = rng.randrange(p)
    return a, b, triples, U, W, er, alpha, beta


def test_a_changed_word_of_er_is_refused(pkg):
    """the prover commits to an er that is not U[row] in one word: its sumcheck is consistent, the row lookup is not.  That the
    two fraction sums differ at the alpha and beta MISMATCH_SEED draws is checked here on the CPU, by the definition"""
    p = GOLD
    ctx, sp, F = ctx_of(pkg, p), pkg.spark, pkg.Field(p)
    a, b, triples, Uc, Wc, er_bad, alpha, beta = mismatch_case(p)
    assert alpha not in cases.keys(triples, Uc, Wc, beta, p, er=er_bad)
    s = cases.sums(triples, Uc, Wc, alpha, beta, p, a, b, er=er_bad)
    assert s["row"][0] != s["row"][1] and s["col"][0] == s["col"][1]
    sc = sp.SparseCommitment(ctx, a, b, [t[0] for t in triples], [t[1] for t in triples], mont_np(p, [t[2] for t in triples]))
    U, W = upload(pkg, ctx, mont_np(p, Uc)), upload(pkg, ctx, mont_np(p, Wc))

    class Dishonest(sp.Prover):
        def gather_commit(self):
            _, self.ec = sp.gather(self.ctx, self.sc, self.U, self.W)
            self.er = upload(pkg, ctx, mont_np(p, er_bad))
            for name, t in (("er", self.er), ("ec", self.ec)):
                self.pcs[name] = self.commit(t)
                self.own.append(self.pcs[name])
    with pytest.raises(sp.LookupMismatch) as ei:
        exchange(pkg, sc, U, W, lambda z: U.evaluate(z), lambda z: W.evaluate(z), MISMATCH_SEED, prover=Dishonest(sc, U, W))
    _, rows, _, _ = ref.pad(triples)
    den_w, den_t = ref.denominators(rows, er_bad, Uc, alpha, beta, p)
    import logup_ref
    root_w = tuple(x[0][0] for x in logup_ref.tree(None, den_w, p))
    root_t = tuple(x[0][0] for x in logup_ref.tree(ref.counts(rows, a), den_t, p))
    assert ei.value.dim == "row" and (ei.value.root_w, ei.value.root_t) == (tuple(ref.mont_list(root_w, p)), tuple(ref.mont_list(root_t, p)))
    sc.close()


def test_a_field_too_small_for_the_counts_is_refused(pkg):
    """p = 257 with l = 10: a count may reach 2^10"""
    p = 257
    ctx, sp = ctx_of(pkg, p), pkg.spark
    gc.collect()
    base = pool(ctx)
    rng = np.random.default_rng(1)
    rows, cols, vals = rng.integers(0, 4, size=1000), rng.integers(0, 4, size=1000), rng.integers(0, p, size=1000).astype(np.uint64)
    expect(pkg, 6, lambda: bare(pkg, ctx, 2, 2, rows, cols, vals), "sc_spark_create", "2^10")
    expect(pkg, 6, lambda: bare(pkg, ctx, 9, 2, rows[:100], cols[:100], vals[:100]), "sc_spark_create", "2^9")
    O = cases.Opening
    with pytest.raises(ValueError):
        sp.Verifier(pkg.Field(p), 2, 2, 10, {"row": O(10), "col": O(10), "val": O(10), "cr": O(2), "cc": O(2)}, None, None)
    # 2^8 entries fit: 257 > 2^8
    sc = bare(pkg, ctx, 2, 2, rows[:256], cols[:256], vals[:256])
    assert np.array_equal(sc.table("cr").to_evaluations(), mont_np(p, np.bincount(rows[:256], minlength=4)))
    sc.close()
    gc.collect()
    assert pool(ctx) == base


# ---- the R1CS argument whose verifier holds no matrices ----------------------------------------------------------------

def argue_both(pkg, p, s, m, seed, opening, flip=False):
    """the same instance and witness under r1cs.prove_and_verify and r1cs.prove_and_verify_sublinear; what each returned or raised"""
    rp, lp, sp = pkg.r1cs, pkg.ligero_pcs, pkg.spark
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    R, io, w = rp.synthetic_instance(F, s, m, seed)
    if flip:
        col = next(j for _, j, _ in R.matrices[0] + R.matrices[1] if j >= 1 << (m - 1)) - (1 << (m - 1))
        w = list(w)
        w[col] = F.add(w[col], F.one)
    dev = rp.DeviceR1CS(ctx, R)
    code, folded = ("expander" if opening == "expander" else "rs"), opening == "folded"
    c = max(1, m // 2) if folded else m // 2
    instance = dev.commit_instance(code=code)
    assert (instance.a, instance.b, instance.nnz) == (s + 2, m, sum(len(M) for M in R.matrices))
    out = []
    try:
        for sublinear in (False, True):
            prover = rp.Prover(ctx, dev, io, w, log_cols=c, log_blowup=1, code=code)
            root = prover.root()
            pv = lp.FoldVerifier(F, m - 1, c, 1, root, QUERIES) if folded else lp.Verifier(F, m - 1, c, 1, root, QUERIES, code=code)
            rng = random.Random(seed + 1)
            try:
                if sublinear:
                    verifier = rp.SublinearVerifier(F, s, m, io, root, pv, instance.verifiers(QUERIES, folded))
                    out.append(rp.prove_and_verify_sublinear(prover, instance, verifier, rng))
                else:
                    out.append(rp.prove_and_verify(prover, rp.Verifier(R, io, root, pv), rng))
            except rp.Error as exc:
                out.append(exc)
            finally:
                prover.close()
    finally:
        instance.close()
        dev.close()
    return out


@pytest.mark.parametrize("p,opening", [(GOLD, "plain"), (GOLD, "folded"), (P64, "expander")], ids=["gold-plain", "gold-folded", "p64m59-expander"])
@pytest.mark.parametrize("s,m", [(6, 5), (10, 11), (12, 12)])
def test_sublinear_argument_next_to_the_argument(pkg, p, opening, s, m):
    assert argue_both(pkg, p, s, m, 31 * s + m, opening) == [True, True]


@pytest.mark.parametrize("p,opening", [(GOLD, "plain"), (P64, "expander")], ids=["gold-plain", "p64m59-expander"])
def test_a_flipped_witness_word_is_refused_by_both(pkg, p, opening):
    rp = pkg.r1cs
    bad = argue_both(pkg, p, 6, 5, 8, opening, flip=True)
    assert all(type(e) is rp.RoundMismatch and (e.phase, e.round) == (1, 0) for e in bad), bad


# ---- refusals and the pool's books -------------------------------------------------------------------------------------

def test_refusals(pkg):
    p = GOLD
    ctx, F, sp = ctx_of(pkg, p), pkg.Field(p), pkg.spark
    lib = ctx.lib
    gc.collect()
    base = pool(ctx)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    h, out, out2 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    r3, c3, v3 = (ctypes.c_uint32 * 3)(0, 1, 3), (ctypes.c_uint32 * 3)(0, 1, 1), (ctypes.c_uint64 * 3)(1, 2, 3)
    # sc_spark_create: NULLs, an empty list, the ranges of a and b, a triple outside, a value that is no word below p
    assert lib.sc_spark_create(ctx.h, 2, 1, None, c3, v3, 3, ctypes.byref(h)) == 1 and lib.sc_spark_create(ctx.h, 2, 1, r3, None, v3, 3, ctypes.byref(h)) == 1
    assert lib.sc_spark_create(ctx.h, 2, 1, r3, c3, None, 3, ctypes.byref(h)) == 1 and lib.sc_spark_create(ctx.h, 2, 1, r3, c3, v3, 3, None) == 1
    assert lib.sc_spark_create(ctx.h, 2, 1, r3, c3, v3, 0, ctypes.byref(h)) == 1 and "at least one" in lib.sc_last_error(ctx.h).decode()
    empty = np.zeros(0, dtype=np.uint32)
    expect(pkg, 1, lambda: bare(pkg, ctx, 2, 1, empty, empty, np.zeros(0, dtype=np.uint64)), "at least one")
    for a, b in ((0, 1), (1, 0), (29, 1), (1, 29)):
        assert lib.sc_spark_create(ctx.h, a, b, r3, c3, v3, 3, ctypes.byref(h)) == 1 and "1..28" in lib.sc_last_error(ctx.h).decode()
    expect(pkg, 1, lambda: bare(pkg, ctx, 1, 1, [0, 1, 3], [0, 1, 1], [1, 2, 3]), "entry 2 is (3, 1, 3)")
    expect(pkg, 1, lambda: bare(pkg, ctx, 2, 1, [0, 1, 3], [0, 2, 1], [1, 2, 3]), "entry 1 is (1, 2, 2)")
    expect(pkg, 1, lambda: bare(pkg, ctx, 2, 1, [0, 1, 3], [0, 1, 1], [1, p, 3]), "entry 1")
    assert not h.value
    gc.collect()
    assert pool(ctx) == base, "a refused create leaves nothing behind"
    sc = bare(pkg, ctx, 2, 1, [0, 1, 3], [0, 1, 1], [1, 2, 3])
    assert pool(ctx)[0] == base[0] + 7, "two index streams and five tables"
    t2, t4, t8 = (pkg.DenseMultilinearExtension.generate(ctx, k, n) for k, n in ((1, 1), (2, 2), (3, 3)))
    # sc_spark_table: which, NULLs
    expect(pkg, 1, lambda: sc.table(5), "which = 5")
    expect(pkg, 1, lambda: sc.table(-1), "which = -1")
    assert lib.sc_spark_table(ctx.h, sc.h, 0, None) == 1 and lib.sc_spark_table(ctx.h, None, 0, ctypes.byref(out)) == 1
    # sc_spark_gather: NULLs, lengths
    assert lib.sc_spark_gather(ctx.h, sc.h, None, t2.h, ctypes.byref(out), ctypes.byref(out2)) == 1
    assert lib.sc_spark_gather(ctx.h, sc.h, t4.h, t2.h, None, ctypes.byref(out2)) == 1
    assert lib.sc_spark_gather(ctx.h, None, t4.h, t2.h, ctypes.byref(out), ctypes.byref(out2)) == 1
    expect(pkg, 1, lambda: sp.gather(ctx, sc, t2, t2), "tables of 2 and 2 entries")
    expect(pkg, 1, lambda: sp.gather(ctx, sc, t4, t4), "tables of 4 and 4 entries")
    # sc_spark_denominators: dim, lengths, an unreduced alpha or beta
    expect(pkg, 1, lambda: sp.denominators(ctx, sc, 2, t4, t4, 1, 1), "dim = 2")
    expect(pkg, 1, lambda: sp.denominators(ctx, sc, "row", t2, t4, 1, 1), "tables of 2 and 4 entries")
    expect(pkg, 1, lambda: sp.denominators(ctx, sc, "col", t2, t8, 1, 1), "tables of 2 and 8 entries")
    expect(pkg, 1, lambda: sp.denominators(ctx, sc, "row", t4, t4, p, 1), "not a word below p")
    expect(pkg, 1, lambda: sp.denominators(ctx, sc, "row", t4, t4, 1, p), "not a word below p")
    assert lib.sc_spark_denominators(ctx.h, sc.h, 0, t4.h, t4.h, 1, 1, None, ctypes.byref(out2)) == 1 and not out.value and not out2.value
    # sc_product3_prove: NULLs, lengths, an unreduced draw
    no_draw = ctypes.cast(None, pkg._lib.DRAW4_FN)
    c1, fin = ctypes.c_uint64(), (ctypes.c_uint64 * 3)()
    t1 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, np.array([5], dtype=np.uint64))
    assert lib.sc_product3_prove(ctx.h, t4.h, t4.h, t4.h, no_draw, None, 0, None, None, None, fin) == 1
    assert lib.sc_product3_prove(ctx.h, t4.h, t4.h, t4.h, no_draw, None, 0, ctypes.byref(c1), None, None, None) == 1
    assert lib.sc_product3_prove(ctx.h, None, t4.h, t4.h, no_draw, None, 0, ctypes.byref(c1), None, None, fin) == 1
    assert lib.sc_product3_prove(ctx.h, t4.h, t4.h, t4.h, no_draw, None, 0, ctypes.byref(c1), None, None, fin) == 0   # evals and challenges may be NULL
    expect(pkg, 1, lambda: sp.product3_prove(ctx, t4, t4, t8), "tables of 4, 4 and 8 entries")
    expect(pkg, 1, lambda: sp.product3_prove(ctx, t1, t1, t1), "at least two")
    expect(pkg, 1, lambda: sp.product3_prove(ctx, t4, t4, t4, lambda j, msg: p), "unreduced")
    # sc_table_eq: NULLs, n, an unreduced word
    assert lib.sc_table_eq(ctx.h, None, 2, ctypes.byref(out)) == 1
    expect(pkg, 1, lambda: sp.table_eq(ctx, []), "n = 0")
    expect(pkg, 1, lambda: sp.table_eq(ctx, [1] * 29), "n = 29")
    expect(pkg, 1, lambda: sp.table_eq(ctx, [1, p]), "r[1]")
    # p = 3: the cubic through 0 .. 3 does not exist
    c3x = pkg.Context(pkg.Field(3))
    s3 = pkg.DenseMultilinearExtension.from_evaluations_vec(c3x, 1, np.array([1, 2], dtype=np.uint64))
    expect(pkg, 6, lambda: sp.product3_prove(c3x, s3, s3, s3), "p = 3")
    expect(pkg, 6, lambda: bare(pkg, c3x, 1, 1, [0], [0], [1]), "p = 3")
    del s3
    c3x.close()
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
        expect(pkg, 6, lambda: bare(pkg, other, 2, 1, [0, 1, 3], [0, 1, 1], [1, 2, 3]), "sc_spark_create: " + msg)
        expect(pkg, 6, lambda: sp.product3_prove(other, ot, ot, ot), "sc_product3_prove: " + msg)
        expect(pkg, 6, lambda: sp.table_eq(other, [1, 2]), "sc_table_eq: " + msg)
        assert other.lib.sc_spark_create(other.h, 0, 0, None, None, None, 0, None) == 6
        assert other.lib.sc_spark_table(other.h, sc.h, 0, ctypes.byref(out)) == 6 and not out.value
        assert other.lib.sc_spark_gather(other.h, None, None, None, None, None) == 6
        assert other.lib.sc_spark_denominators(other.h, None, 0, None, None, 0, 0, None, None) == 6
        assert other.lib.sc_product3_prove(other.h, None, None, None, no_draw, None, 0, None, None, None, None) == 6
        assert other.lib.sc_table_eq(other.h, None, 0, None) == 6
        assert other.lib.sc_r1cs_row_weights(other.h, None, None, None, None) == 6
        del ot
        other.close()
    # tables of more than 2^28 entries are refused before they are read: a handle over 2^29 words that are never touched
    big = ctypes.c_void_p()
    assert lib.sc_table_from_device(ctx.h, ctypes.c_void_p(lib.sc_table_device_ptr(t4.h)), 1 << 29, ctypes.byref(big)) == 0
    assert lib.sc_product3_prove(ctx.h, big, big, big, no_draw, None, 0, ctypes.byref(c1), None, None, fin) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_table_free(ctx.h, big) == 0
    sc.close()
    del t1, t2, t4, t8
    gc.collect()
    assert pool(ctx) == base


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p):
    ctx, F, sp = ctx_of(pkg, p), pkg.Field(p), pkg.spark
    n, T = 11, 4
    gc.collect()
    base = pool(ctx)
    tabs = [upload(pkg, ctx, ww.edge_table(p, 1 << n, np.random.default_rng(k))) for k in range(3)]
    mid = pool(ctx)
    default = host_log(pkg, p)
    ctx.set_option("gp_host_log", T)
    try:
        first = sp.product3_prove(ctx, *tabs, seed_r=3)
        assert pool(ctx) == mid, "after a proof"

        class Boom(Exception):
            pass

        def raising_at(j):
            def draw(i, msg):
                if i == j:
                    raise Boom()
                return F.one
            return draw
        for j, what in ((0, "the first device round"), (3, "a device round"), (n - T, "the first host round"), (n - 1, "the last host round")):
            with pytest.raises(Boom):
                sp.product3_prove(ctx, *tabs, raising_at(j))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        # the context still proves, and the same transcript
        assert sp.product3_prove(ctx, *tabs, seed_r=3) == first
    finally:
        ctx.set_option("gp_host_log", default)
    # the matrix: two index streams and five tables, given back by close(); gather and denominators hand out tables alone
    rng = np.random.default_rng(5)
    sc = bare(pkg, ctx, 6, 4, rng.integers(0, 64, size=500), rng.integers(0, 16, size=500), ww.edge_table(p, 500, rng))
    assert pool(ctx)[0] == mid[0] + 7
    U, W = upload(pkg, ctx, ww.edge_table(p, 64, rng)), upload(pkg, ctx, ww.edge_table(p, 16, rng))
    er, ec = sp.gather(ctx, sc, U, W)
    dw, dt = sp.denominators(ctx, sc, "row", U, er, F.one, F.one)
    assert pool(ctx)[0] == mid[0] + 7 + 6
    del er, ec, dw, dt, U, W
    sc.close()
    del tabs
    gc.collect()
    assert pool(ctx) == base
