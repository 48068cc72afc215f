"""GPU: the sum-of-products sumcheck with challenges from the quadratic extension K = F_p[X] / (X^2 - w) (sc_sumprod_prove_ext,
sc_table_evaluate_ext; thaler-study_amd/ext_sumcheck.py) against the big-integer reference of tests/ext_ref.py, bit for bit: the
transcript at every hand-over to the host, every T, four moduli, few blocks; against sc_sumprod_prove when every drawn c1 is 0;
the evaluation at a point of K^n; the launch log against the byte model; every refusal; the pool's books; and the inner-product
argument over Ligero commitments (Reed-Solomon and expander code)."""
import ctypes
import gc
import random

import numpy as np
import pytest

import ext_ref as ref
import ligero_ref as lref
import wide_words as ww
from conftest import load_package
from ligero_common import context_cache, expect
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu
XS = load_package().ext_sumcheck          # (the module under test: without it nothing here can run)

ctx_of, teardown_module = context_cache()
GOLD = lref.GOLD
P64, P61, P32 = 2**64 - 59, 2**61 - 1, 2**32 + 15
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1", P32: "p32p15"}
QUERIES = 8


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
    return lref.mont(p, [ref.nonresidue(p)])[0]


def mont_pairs(p, pairs):
    return [tuple(lref.mont(p, e)) for e in pairs]


def pick_word(p, rng):
    return rng.choice([0, 1, p - 1, rng.randrange(p)])


def challenges(p, n, rng):
    """canonical challenges with components from {0, 1, p - 1, random}; among them (0, 1) = X itself, (p - 1, p - 1) and one with
    c1 = 0, as far as n allows"""
    ch = [(pick_word(p, rng), pick_word(p, rng)) for _ in range(n)]
    ch[n - 1] = (p - 1, p - 1)
    if n >= 2:
        ch[0] = (0, 1)
    if n >= 3:
        ch[1] = (rng.randrange(p), 0)
    return ch


_REF = {}


def reference(p, n, T, seed):
    """(a tables, b tables of raw words, canonical challenges, the reference transcript): computed once, shared, never changed.
    wide_words.octet_table inputs.  With T >= 3 pair 2 reads pair 0's a table as its b table and pair 1's b table as its a table:
    one table in several pairs"""
    key = (p, n, T, seed)
    if key not in _REF:
        rng = np.random.default_rng(seed)
        a = [ww.octet_table(p, 1 << n, rng) for _ in range(T)]
        b = [ww.octet_table(p, 1 << n, rng) for _ in range(T)]
        if T >= 3:
            a[2], b[2] = b[1], a[0]
        ch = challenges(p, n, random.Random(seed + 1))
        out = ref.sumcheck([lref.canon(p, t) for t in a], [lref.canon(p, t) for t in b], p, ref.nonresidue(p), lambda j, msg: ch[j])
        _REF[key] = (a, b, ch, out)
    return _REF[key]


def want_of(p, out):
    c1, rounds, rs, fa, fb = out
    return (tuple(lref.mont(p, c1)), [mont_pairs(p, m) for m in rounds], mont_pairs(p, rs), mont_pairs(p, fa), mont_pairs(p, fb))


def device(pkg, p, a, b, ch_canon, H, blocks=None, log=None):
    """sc_sumprod_prove_ext at gp_host_log = H (and max_blocks = blocks) under the fixed challenges; the draw also checks the order
    it is called in.  Tables that are one array are one device table.  log: a list that receives the launch records"""
    ctx = ctx_of(pkg, p)
    words = mont_pairs(p, ch_canon)
    seen = []

    def draw(j, msg):
        assert len(msg) == 3 and all(len(m) == 2 for m in msg)
        seen.append(j)
        return words[j]
    base, base_blocks = host_log(pkg, p), ctx.get_option("max_blocks")
    dev = {}
    for t in a + b:
        if id(t) not in dev:
            dev[id(t)] = upload(pkg, ctx, t)
    ctx.set_option("gp_host_log", H)
    if blocks:
        ctx.set_option("max_blocks", blocks)
    if log is not None:
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
    try:
        out = XS.sumprod_prove_ext(ctx, w_of(p), [dev[id(t)] for t in a], [dev[id(t)] for t in b], draw)
        if log is not None:
            log.extend(ctx.launch_log())
    finally:
        ctx.set_option("gp_host_log", base)
        ctx.set_option("max_blocks", base_blocks)
        ctx.set_option("time_kernels", 0)
    assert seen == list(range(len(ch_canon)))
    for t in a + b:
        assert np.array_equal(dev[id(t)].to_evaluations(), t), "the inputs are never written"
    return out


SIZES = ([(GOLD, n, 3) for n in range(1, 15)] + [(GOLD, n, T) for T in (1, 2, 5, 8) for n in (1, 2, 7, 13)]
         + [(p, n, 3) for p in (P64, P61, P32) for n in (1, 2, 7, 13)])


@pytest.mark.parametrize("p,n,T", SIZES, ids=["%s-%d-T%d" % (IDS[p], n, T) for p, n, T in SIZES])
def test_transcript_is_the_reference_bit_for_bit(pkg, p, n, T):
    """gp_host_log = 0 (every round but the last on the device: n = 1 all on the host, n = 2 the base-in fold as the last launch,
    n = 3 the first extension-in fold, n = 4 two of them in a row) and the default (the same paths at n = 11 .. 14); at n = 5 and 9,
    T = 3 on Goldilocks also 1, 3, n - 1, n and 12.  c1, all 6 n values, the challenges and the 2 * 2 T finals; and the transcript
    is the same at every gp_host_log"""
    a, b, ch, out = reference(p, n, T, 900 + 20 * T + n)
    want = want_of(p, out)
    assert want[0][1] == 0 and all(m[1] == 0 for m in want[1][0])
    extra = (1, 3, n - 1, n, 12) if (p, T) == (GOLD, 3) and n in (5, 9) else ()
    outs = [device(pkg, p, a, b, ch, H) for H in sorted(set([0, host_log(pkg, p)]) | set(extra))]
    for got in outs:
        assert got == want
    assert all(o == outs[0] for o in outs[1:]), "transcripts at different gp_host_log are identical"


def want_log(n, T, te):
    """(kind, kf, ks, log_in, bytes read, bytes written) of every launch: round 0 is the kind it is"""
    out = [("sumprod_pass", 0, T, n, (2 * T * 8) << n, 0)]
    for j in range(1, n - te + 1):
        m = n - j + 1
        out.append(("sumprod_ext_pass", 1 if j == 1 else 2, T, m, (2 * T * (8 if j == 1 else 16)) << m, (2 * T * 16) << (m - 1)))
    return out


def records(log):
    return [(x["kind"], x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log if x["kind"] in ("sumprod_pass", "sumprod_ext_pass")]


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
@pytest.mark.parametrize("blocks", [1, 3])
def test_few_blocks(pkg, p, blocks):
    """n = 13, every round on the device: with max_blocks = 3 threads take uneven numbers of trips through the grid-stride loop
    and finish_pass hands off across three blocks, with max_blocks = 1 one block does everything.  The transcript is the reference's
    and the launches are the byte model's"""
    n, T = 13, 3
    a, b, ch, out = reference(p, n, T, 900 + 20 * T + n)
    log = []
    assert device(pkg, p, a, b, ch, 0, blocks, log) == want_of(p, out)
    assert records(log) == want_log(n, T, 1)


@pytest.mark.parametrize("T", [1, 5])
def test_launch_log_against_the_byte_model(pkg, T):
    """one launch per device round at the default hand-over: round 0 a sumprod_pass record, round 1 reads base words (kf = 1), every
    later one both planes (kf = 2); the rounds of the last 2^max(H, 1) entries leave no record"""
    p, n = GOLD, 13
    a, b, ch, _ = reference(p, n, T, 900 + 20 * T + n)
    H = host_log(pkg, p)
    log = []
    device(pkg, p, a, b, ch, H, None, log)
    assert n > max(H, 1) and records(log) == want_log(n, T, max(H, 1))
    # sc_table_evaluate_ext: one fold-only launch per coordinate down to the same hand-over, ks = 0, one table's bytes
    ctx = ctx_of(pkg, p)
    t = upload(pkg, ctx, a[0])
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    try:
        XS.table_evaluate_ext(ctx, w_of(p), t, mont_pairs(p, ch))
        log = ctx.launch_log()
    finally:
        ctx.set_option("time_kernels", 0)
    want = [("sumprod_ext_pass", 1 if j == 0 else 2, 0, n - j, (8 if j == 0 else 16) << (n - j), 16 << (n - j - 1)) for j in range(n - max(H, 1))]
    assert [(x["kind"], x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log] == want


@pytest.mark.parametrize("p,n,T", [(GOLD, 13, 3), (GOLD, 4, 8), (P64, 13, 2), (P32, 7, 1)], ids=["gold-13-T3", "gold-4-T8", "p64m59-13-T2", "p32p15-7-T1"])
def test_base_field_challenges_give_sc_sumprod_prove(pkg, p, n, T):
    """every drawn c1 = 0: the c0 words are sc_sumprod_prove's own output on the same tables, every c1 word is 0"""
    ctx = ctx_of(pkg, p)
    rng = np.random.default_rng(n + T)
    a = [upload(pkg, ctx, ww.octet_table(p, 1 << n, rng)) for _ in range(T)]
    b = [upload(pkg, ctx, ww.octet_table(p, 1 << n, rng)) for _ in range(T)]
    pick = random.Random(n)
    rs = lref.mont(p, [pick_word(p, pick) for _ in range(n)])
    for H in (0, host_log(pkg, p)):
        ctx.set_option("gp_host_log", H)
        try:
            c1, rounds, ch, fa, fb = XS.sumprod_prove_ext(ctx, w_of(p), a, b, lambda j, msg: (rs[j], 0))
            base = pkg.multiopen.sumprod_prove(ctx, a, b, lambda j, msg: rs[j])
        finally:
            ctx.set_option("gp_host_log", host_log(pkg, p))
        assert (c1[0], [[m[0] for m in msg] for msg in rounds], [r[0] for r in ch], [x[0] for x in fa], [x[0] for x in fb]) == base
        assert c1[1] == 0 and all(m[1] == 0 for msg in rounds for m in msg) and all(x[1] == 0 for x in ch + fa + fb)


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_table_evaluate_ext_against_the_reference(pkg, p):
    """n = 1 .. 14 at gp_host_log = 0 and the default: all on the host, the base-in fold alone, one and more extension-in folds"""
    ctx = ctx_of(pkg, p)
    w = ref.nonresidue(p)
    for n in range(1, 15):
        rng = np.random.default_rng(50 + n)
        table = ww.octet_table(p, 1 << n, rng)
        point = challenges(p, n, random.Random(n))
        want = tuple(lref.mont(p, ref.mle_eval(lref.canon(p, table), point, p, w)))
        t = upload(pkg, ctx, table)
        for H in (0, host_log(pkg, p)):
            ctx.set_option("gp_host_log", H)
            try:
                assert XS.table_evaluate_ext(ctx, w_of(p), t, mont_pairs(p, point)) == want, (n, H)
            finally:
                ctx.set_option("gp_host_log", host_log(pkg, p))
        assert np.array_equal(t.to_evaluations(), table)


def host_evaluate(p, w, table, point):
    """a base table's extension at a point of K^n from the eq weights, in numpy arrays of Python integers (canonical)"""
    e0, e1 = np.array([1], dtype=object), np.array([0], dtype=object)
    for r0, r1 in point:
        h0, h1 = (e0 * r0 + e1 * (w * r1 % p)) % p, (e0 * r1 + e1 * r0) % p
        e0, e1 = np.concatenate([(e0 - h0) % p, h0]), np.concatenate([(e1 - h1) % p, h1])
    t = np.array(lref.canon(p, table), dtype=object)
    return (int((t * e0).sum() % p), int((t * e1).sum() % p))


def test_at_2_to_20(pkg):
    """n = 20, T = 2: the reference prover is out of reach; the transcript passes the host verifier's round checks and its final
    check, the finals are sc_table_evaluate_ext of the four tables at the challenges, and that in turn is a host evaluation from
    the eq weights"""
    p, n, T = GOLD, 20, 2
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    a = [pkg.DenseMultilinearExtension.generate(ctx, 30 + k, n) for k in range(T)]
    b = [pkg.DenseMultilinearExtension.generate(ctx, 60 + k, n) for k in range(T)]
    c1, rounds, ch, fa, fb = XS.sumprod_prove_ext(ctx, w_of(p), a, b, seed_r=5)
    assert len(rounds) == len(ch) == n
    # the synthetic challenger
    draw = ref.synthetic_draw(p, 5)
    assert ch == mont_pairs(p, [draw(j, None) for j in range(n)])
    V = XS.Verifier(F, w_of(p), n)
    V.start(c1)
    it = iter([x for r in ch for x in r])

    class Replay:
        def draw(self):
            return next(it)
    for j, msg in enumerate(rounds):
        assert V.round(j, msg, Replay()) == ch[j]
    assert V.final(fa, fb) is True
    assert fa == [XS.table_evaluate_ext(ctx, w_of(p), t, ch) for t in a] and fb == [XS.table_evaluate_ext(ctx, w_of(p), t, ch) for t in b]
    point = [tuple(lref.canon(p, r)) for r in ch]
    assert tuple(lref.canon(p, fa[0])) == host_evaluate(p, ref.nonresidue(p), a[0].to_evaluations(), point)
    assert XS.sumprod_prove_ext(ctx, w_of(p), a, b, draw=lambda j, msg: ch[j]) == (c1, rounds, ch, fa, fb)


def test_refusals(pkg):
    p = GOLD
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    lib, w = ctx.lib, w_of(p)
    gc.collect()
    t1 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, np.array([5], dtype=np.uint64))
    t2, t4, t8 = (pkg.DenseMultilinearExtension.generate(ctx, k, n) for k, n in ((1, 1), (2, 2), (3, 3)))
    mid = pool(ctx)
    no_draw = ctypes.cast(None, pkg._lib.DRAW_EXT_FN)
    c1, fa, fb = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 16)()
    two = (ctypes.c_void_p * 2)(t4.h, t4.h)
    hole = (ctypes.c_void_p * 2)(t4.h, None)
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, None, two, no_draw, None, 0, c1, None, None, fa, fb) == 1
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, two, None, no_draw, None, 0, c1, None, None, fa, fb) == 1
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, two, two, no_draw, None, 0, None, None, None, fa, fb) == 1
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, two, two, no_draw, None, 0, c1, None, None, None, fb) == 1
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, two, two, no_draw, None, 0, c1, None, None, fa, None) == 1
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, two, hole, no_draw, None, 0, c1, None, None, fa, fb) == 1 and "pair 1" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 0, two, two, no_draw, None, 0, c1, None, None, fa, fb) == 1 and "1..8" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_sumprod_prove_ext(ctx.h, w, 2, two, two, no_draw, None, 0, c1, None, None, fa, fb) == 0   # evals and challenges may be NULL
    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, w, [t4] * 9, [t4] * 9), "count = 9")
    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, w, [t4, t4], [t4, t8]), "pair 1 has tables of 4 and 8 entries")
    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, w, [t1], [t1]), "at least two")
    # w: a residue, a word that is not below p
    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, F.from_int(4), [t4], [t4]), "non-residue")
    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, F.one, [t4], [t4]), "non-residue")
    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, p, [t4], [t4]), "w is not a word below p")
    expect(pkg, 1, lambda: XS.table_evaluate_ext(ctx, F.from_int(4), t4, [(1, 1)] * 2), "non-residue")
    expect(pkg, 1, lambda: XS.table_evaluate_ext(ctx, p, t4, [(1, 1)] * 2), "w is not a word below p")
    # an unreduced challenge component, in a device round and in a host round, either component
    for H in (0, host_log(pkg, p)):
        ctx.set_option("gp_host_log", H)
        try:
            for bad in ((p, 1), (1, p)):
                for at in (0, 2):
                    expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, w, [t8], [t8], lambda j, msg: bad if j == at else (1, 1)), "unreduced component")
        finally:
            ctx.set_option("gp_host_log", host_log(pkg, p))
    # sc_table_evaluate_ext: NULLs, n, a point of the wrong length, an unreduced component
    pt, out = (ctypes.c_uint64 * 4)(1, 2, 3, 4), (ctypes.c_uint64 * 2)()
    assert lib.sc_table_evaluate_ext(ctx.h, w, None, pt, 2, out) == 1 and lib.sc_table_evaluate_ext(ctx.h, w, t4.h, None, 2, out) == 1
    assert lib.sc_table_evaluate_ext(ctx.h, w, t4.h, pt, 2, None) == 1
    expect(pkg, 1, lambda: XS.table_evaluate_ext(ctx, w, t4, [(1, 1)] * 3), "a table of 4 entries and a point of 3 coordinates")
    assert lib.sc_table_evaluate_ext(ctx.h, w, t1.h, pt, 0, out) == 1 and "a point of 0 coordinates" in lib.sc_last_error(ctx.h).decode()
    expect(pkg, 1, lambda: XS.table_evaluate_ext(ctx, w, t4, [(1, 1), (1, p)]), "component 1 of coordinate 1")
    assert pool(ctx) == mid, "a refused call leaves nothing behind"
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
        expect(pkg, 6, lambda: XS.sumprod_prove_ext(other, w, [ot], [ot]), "sc_sumprod_prove_ext: " + msg)
        expect(pkg, 6, lambda: XS.table_evaluate_ext(other, w, ot, [(1, 1)] * 3), "sc_table_evaluate_ext: " + msg)
        assert other.lib.sc_sumprod_prove_ext(other.h, 0, 0, None, None, no_draw, None, 0, None, None, None, None, None) == 6
        assert other.lib.sc_table_evaluate_ext(other.h, 0, None, None, 0, None) == 6
        del ot
        other.close()


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p):
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    n, H, T, w = 11, 4, 3, w_of(p)
    gc.collect()
    base = pool(ctx)
    a = [upload(pkg, ctx, ww.edge_table(p, 1 << n, np.random.default_rng(k))) for k in range(T)]
    b = [upload(pkg, ctx, ww.edge_table(p, 1 << n, np.random.default_rng(10 + k))) for k in range(T)]
    mid = pool(ctx)
    default = host_log(pkg, p)
    ctx.set_option("gp_host_log", H)
    try:
        first = XS.sumprod_prove_ext(ctx, w, a, b, seed_r=3)
        assert pool(ctx) == mid, "after a proof"
        XS.table_evaluate_ext(ctx, w, a[0], first[2])
        assert pool(ctx) == mid, "after an evaluation"

        class Boom(Exception):
            pass

        def raising_at(j):
            def draw(i, msg):
                if i == j:
                    raise Boom()
                return (F.one, F.one)
            return draw
        for j, what in ((0, "the first device round"), (1, "the base-in round"), (3, "a device round"), (n - H, "the first host round"),
                        (n - 1, "the last host round")):
            with pytest.raises(Boom):
                XS.sumprod_prove_ext(ctx, w, a, b, raising_at(j))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        short = a[0].fix_variables([F.one])
        short_pool = pool(ctx)
        expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, w, a, b[:2] + [short]), "pair 2")
        expect(pkg, 1, lambda: XS.sumprod_prove_ext(ctx, F.from_int(9), a, b), "non-residue")
        assert pool(ctx) == short_pool, "after a refused call"
        del short
        gc.collect()
        # the context still proves, and the same transcript
        assert XS.sumprod_prove_ext(ctx, w, a, b, seed_r=3) == first
    finally:
        ctx.set_option("gp_host_log", default)
    del a, b
    gc.collect()
    assert pool(ctx) == base


@pytest.mark.parametrize("p,n,code", [(GOLD, 10, "rs"), (GOLD, 12, "rs"), (P64, 8, "expander")], ids=["gold-10", "gold-12", "p64m59-8-expander"])
def test_prove_inner_product(pkg, p, n, code):
    """c = sum a b is returned and is the dot product; a word of b flipped after its commitment - the prover's sumcheck runs over
    the changed table, the opening answers from the committed one - is refused at the final check"""
    ctx, F, lp = ctx_of(pkg, p), pkg.Field(p), pkg.ligero_pcs
    gc.collect()
    base = pool(ctx)
    rng = np.random.default_rng(n)
    ta, tb = ww.edge_table(p, 1 << n, rng), ww.edge_table(p, 1 << n, rng)
    a, b = upload(pkg, ctx, ta), upload(pkg, ctx, tb)
    pa, pb = lp.Prover.commit(ctx, a, code=code), lp.Prover.commit(ctx, b, code=code)
    w = w_of(p)

    def verifiers():
        return [lp.ExtVerifier(F, n, pr.log_cols, pr.log_blowup, pr.root(), QUERIES, code=code, w=w) for pr in (pa, pb)]
    c = XS.prove_inner_product(ctx, w, pa, pb, *verifiers(), random.Random(3))
    ca, cb = lref.canon(p, ta), lref.canon(p, tb)
    assert F.to_int(c) == sum(x * y for x, y in zip(ca, cb)) % p
    # one opening on its own: the value is the table's extension at the point
    z = [(F.rand(random.Random(j)), F.rand(random.Random(100 + j))) for j in range(n)]
    assert XS.open_committed_ext(pa, verifiers()[0], z, random.Random(4), w) == XS.table_evaluate_ext(ctx, w, a, z)
    flipped = tb.copy()
    flipped[5] = F.add(int(flipped[5]), F.one)
    pb.poly = upload(pkg, ctx, flipped)
    with pytest.raises(XS.FinalMismatch):
        XS.prove_inner_product(ctx, w, pa, pb, *verifiers(), random.Random(3))
    pb.poly = b
    # verifiers over another w, or plain ones, are refused before anything runs
    with pytest.raises(ValueError):
        XS.prove_inner_product(ctx, w, pa, pb, lp.Verifier(F, n, pa.log_cols, 1, pa.root(), QUERIES, code=code), verifiers()[1], random.Random(3))
    pa.close()
    pb.close()
    del a, b, pa, pb
    gc.collect()
    assert pool(ctx) == base
