"""GPU: batched openings (sc_table_eq_sum, sc_sumprod_prove; thaler-study_amd/multiopen.py and the batched forms of spark.py and
r1cs.py) against numpy and the big-integer reference of tests/multiopen_ref.py, word for word: the weighted eq sum at every width
around the split of its index, the sum-of-products proof at every hand-over to the host, the whole exchange over Ligero commitments
(Reed-Solomon and expander code) with every single tamper of the device's messages, the SPARK and R1CS arguments next to their
single-opening forms, the refusals and the pool's books."""
import ctypes
import gc
import random

import numpy as np
import pytest

import multiopen_ref as ref
import spark_ref as sref
import wide_words as ww
from conftest import load_package
from ligero_common import context_cache, expect, mont_np
from spark_cases import GOLD, P61, P64
from test_gpu_sharded import Loopback
from test_gpu_spark import MISMATCH_SEED, eq_eval, mismatch_case      # (host code: the seed, z -> eq(point, z), the dishonest er)

pytestmark = pytest.mark.gpu
MO = load_package().multiopen            # (the module under test: without it nothing here can run)

ctx_of, teardown_module = context_cache()
QUERIES = 8
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1"}
LO = 7               # kEqSumLoLog


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


def pick_word(p, rng):
    return rng.choice([0, 1, p - 1, rng.randrange(p)])


# ---- sc_table_eq_sum ---------------------------------------------------------------------------------------------------

def eq_sum_ref(p, points, coeffs):
    """sum_k coeffs[k] eq(points[k], .) in canonical integers, a numpy array of Python integers; bit j of the index goes with
    points[k][j]"""
    total = np.zeros(1 << len(points[0]), dtype=object)
    for pt, c in zip(points, coeffs):
        w = np.array([c % p], dtype=object)
        for r in pt:
            hi = w * r % p
            w = np.concatenate([(w - hi) % p, hi])
        total = (total + w) % p
    return total


def eq_sum_device(pkg, p, points, coeffs):
    """the device table and its launch records"""
    ctx = ctx_of(pkg, p)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    t = pkg.multiopen.table_eq_sum(ctx, [sref.mont_list(pt, p) for pt in points], sref.mont_list(coeffs, p))
    log = [(x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in ctx.launch_log() if x["kind"] == "eq_sum"]
    ctx.set_option("time_kernels", 0)
    return t.to_evaluations(), log


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_eq_sum_word_for_word(pkg, p):
    """every n from 1 to lo + 2: no high part up to lo = 7, the first split (one high bit) at 8, two high bits at 9; count 1, 2, 3
    and 16; coordinates and coefficients from {0, 1, p - 1, random}; one launch whose record is the byte model's"""
    rng = random.Random(p % 1000)
    for n in range(1, LO + 3):
        for count in (1, 2, 3, 16):
            points = [[pick_word(p, rng) for _ in range(n)] for _ in range(count)]
            coeffs = [pick_word(p, rng) for _ in range(count)]
            got, log = eq_sum_device(pkg, p, points, coeffs)
            assert log == [(0, count, n, 8 * count * (n + 1), 8 << n)], (n, count)
            assert got.shape == (1 << n,) and np.array_equal(got, mont_np(p, eq_sum_ref(p, points, coeffs))), (n, count)
    # all-random points: no entry is zero by a coordinate
    for n, count in ((LO, 16), (LO + 2, 3), (LO + 2, 16)):
        points = [[rng.randrange(p) for _ in range(n)] for _ in range(count)]
        coeffs = [rng.randrange(p) for _ in range(count)]
        assert np.array_equal(eq_sum_device(pkg, p, points, coeffs)[0], mont_np(p, eq_sum_ref(p, points, coeffs))), (n, count)


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_eq_sum_of_one_point_is_table_eq(pkg, p):
    """count = 1 with the coefficient one: sc_table_eq bit for bit, at every width around the split and at n = 20"""
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    rng = random.Random(3)
    for n in list(range(1, LO + 3)) + [20]:
        r = sref.mont_list([pick_word(p, rng) if n <= LO + 2 else rng.randrange(p) for _ in range(n)], p)
        got = pkg.multiopen.table_eq_sum(ctx, [r], [F.one]).to_evaluations()
        assert np.array_equal(got, pkg.spark.table_eq(ctx, r).to_evaluations()), n


def test_eq_sum_at_2_to_20(pkg):
    """n = 20, three points: many chunks of high indices per block, against numpy"""
    p, n, count = GOLD, 20, 3
    rng = random.Random(20)
    points = [[rng.randrange(p) for _ in range(n)] for _ in range(count)]
    points[1][n - 1], points[2][0] = 1, p - 1
    coeffs = [rng.randrange(p), p - 1, 1]
    got, log = eq_sum_device(pkg, p, points, coeffs)
    assert log == [(0, count, n, 8 * count * (n + 1), 8 << n)]
    assert np.array_equal(got, mont_np(p, eq_sum_ref(p, points, coeffs)))


# ---- sc_sumprod_prove --------------------------------------------------------------------------------------------------

_REF = {}


def sp_reference(p, n, T, seed):
    """(2T tables of words, canonical challenges, reference (rounds, challenges, finals_a, finals_b)): computed once, shared,
    never changed.  With T >= 3 pair 2 reads pair 0's a table as its b table and pair 1's b table as its a table: one table in
    several pairs"""
    key = (p, n, T, seed)
    if key not in _REF:
        rng = np.random.default_rng(seed)
        a = [ww.edge_table(p, 1 << n, rng) for _ in range(T)]
        b = [ww.edge_table(p, 1 << n, rng) for _ in range(T)]
        if T >= 3:
            a[2], b[2] = b[1], a[0]
        pick = random.Random(seed + 1)
        ch = [pick_word(p, pick) for _ in range(n)]
        it = iter(ch)
        _REF[key] = (a, b, ch, ref.sumcheck([sref.canon_list(t, p) for t in a], [sref.canon_list(t, p) for t in b], p, lambda j, msg: next(it)))
    return _REF[key]


def sp_device(pkg, p, a, b, ch_canon, H):
    """sc_sumprod_prove at gp_host_log = H under the fixed challenges; the draw also checks the order it is called in.  Tables that
    are one array are one device table"""
    ctx = ctx_of(pkg, p)
    words = sref.mont_list(ch_canon, p)
    seen = []

    def draw(j, msg):
        assert len(msg) == 3
        seen.append(j)
        return words[j]
    base = host_log(pkg, p)
    dev = {}
    for t in a + b:
        if id(t) not in dev:
            dev[id(t)] = upload(pkg, ctx, t)
    ctx.set_option("gp_host_log", H)
    try:
        out = pkg.multiopen.sumprod_prove(ctx, [dev[id(t)] for t in a], [dev[id(t)] for t in b], draw)
    finally:
        ctx.set_option("gp_host_log", base)
    assert seen == list(range(len(ch_canon)))
    for t in a + b:
        assert np.array_equal(dev[id(t)].to_evaluations(), t), "the inputs are never written"
    return out


def sp_want(p, reference):
    rounds, rs, fa, fb = reference
    c1 = (rounds[0][0] + rounds[0][1]) % p
    return (sref.mont(c1, p), [sref.mont_list(m, p) for m in rounds], sref.mont_list(rs, p), sref.mont_list(fa, p), sref.mont_list(fb, p))


SP_SIZES = ([(GOLD, n, 3) for n in range(1, 15)] + [(GOLD, n, T) for T in (1, 2, 5, 8) for n in (1, 2, 7, 13)]
            + [(p, n, 3) for p in (P64, P61) for n in (1, 2, 7, 13)])


@pytest.mark.parametrize("p,n,T", SP_SIZES, ids=["%s-%d-T%d" % (IDS[p], n, T) for p, n, T in SP_SIZES])
def test_sumprod_is_the_reference_bit_for_bit(pkg, p, n, T):
    """gp_host_log = 0 (every round but the last on the device) and the default; at n = 5 and 9, T = 3 on Goldilocks also 1, 3,
    n - 1 (the hand-over at the first possible launch), n (no device round at all) and 12 (above n).  Edge-word tables,
    challenges from {0, 1, p - 1, random}; c1, all 3 n values, the challenges and the 2 T finals"""
    a, b, ch, reference = sp_reference(p, n, T, 700 + 20 * T + n)
    want = sp_want(p, reference)
    extra = (1, 3, n - 1, n, 12) if (p, T) == (GOLD, 3) and n in (5, 9) else ()
    outs = [sp_device(pkg, p, a, b, ch, H) for H in sorted(set([0, host_log(pkg, p)]) | set(extra))]
    for out in outs:
        assert out == want
    assert all(o == outs[0] for o in outs[1:]), "transcripts at different gp_host_log are identical"


def test_sumprod_at_2_to_20(pkg):
    """n = 20, T = 5: the reference is out of reach; the transcript passes the verifier's round checks, the finals are
    sc_table_evaluate of the ten tables at the challenges, and their products add up to the last claim"""
    p, n, T = GOLD, 20, 5
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    a = [pkg.DenseMultilinearExtension.generate(ctx, 30 + k, n) for k in range(T)]
    b = [pkg.DenseMultilinearExtension.generate(ctx, 60 + k, n) for k in range(T)]
    c1, rounds, ch, fa, fb = pkg.multiopen.sumprod_prove(ctx, a, b, seed_r=5)
    assert len(rounds) == len(ch) == n
    V = pkg.multiopen.Verifier(F, (n, 10, 1), {"t": b"\0" * 32}, 1)
    claim = c1
    for msg, r in zip(rounds, ch):
        assert F.add(msg[0], msg[1]) == claim
        claim = V._quadratic_at(msg, r)
    assert fa == [t.evaluate(ch) for t in a] and fb == [t.evaluate(ch) for t in b]
    total = 0
    for x, y in zip(fa, fb):
        total = F.add(total, F.mul(x, y))
    assert total == claim
    # the synthetic challenger is sc_product3_prove's: the same seed draws the same words
    assert pkg.spark.product3_prove(ctx, a[0], a[1], a[2], seed_r=5)[2] == ch
    assert pkg.multiopen.sumprod_prove(ctx, a, b, draw=lambda j, msg: ch[j]) == (c1, rounds, ch, fa, fb)


def test_sumprod_launch_log(pkg):
    """one launch per device round: round 0 reads the caller's tables, every later one folds; the rounds of the last
    2^max(H, 1) entries leave no record"""
    p, n = GOLD, 13
    ctx, H = ctx_of(pkg, p), host_log(pkg, p)
    for T in (1, 5):
        a = [pkg.DenseMultilinearExtension.generate(ctx, 40 + k, n) for k in range(T)]
        b = [pkg.DenseMultilinearExtension.generate(ctx, 50 + k, n) for k in range(T)]
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
        pkg.multiopen.sumprod_prove(ctx, a, b, seed_r=1)
        log = [x for x in ctx.launch_log() if x["kind"] == "sumprod_pass"]
        ctx.set_option("time_kernels", 0)
        te = max(H, 1)
        want = [(0, n, T)] + [(1, n - j + 1, T) for j in range(1, n - te + 1)]
        assert n > te and [(x["kf"], x["log_in"], x["ks"]) for x in log] == want
        for x in log:
            assert x["bytes_read"] == (2 * T * 8) << x["log_in"] and x["bytes_written"] == (((2 * T * 8) << (x["log_in"] - 1)) if x["kf"] else 0)


# ---- prove_claims ------------------------------------------------------------------------------------------------------

def claims_case(pkg, p, n, T, K, code, seed):
    """T committed edge-word tables of n variables and K claims with their true values: every table carries one; claim T repeats
    claim 0's (table, point) pair, the rest fall on random tables"""
    ctx = ctx_of(pkg, p)
    rng = np.random.default_rng(seed)
    pick = random.Random(seed)
    tables = {"t%d" % t: upload(pkg, ctx, ww.edge_table(p, 1 << n, rng)) for t in range(T)}
    provers = {name: pkg.ligero_pcs.Prover.commit(ctx, t, code=code) for name, t in tables.items()}
    names = list(tables)
    claims = []
    for k in range(K):
        if k < T:
            name, pt = names[k], sref.mont_list([pick_word(p, pick) for _ in range(n)], p)
        elif k == T:
            name, pt = claims[0].table, list(claims[0].point)
        else:
            name, pt = pick.choice(names), sref.mont_list([pick.randrange(p) for _ in range(n)], p)
        claims.append(pkg.multiopen.Claim(name, pt, tables[name].evaluate(pt)))
    return tables, provers, claims


def verifiers_of(pkg, p, provers, queries=QUERIES):
    F = pkg.Field(p)
    return {name: pkg.ligero_pcs.Verifier(F, pr.num_vars, pr.log_cols, pr.log_blowup, pr.root(), queries, code=pr.code) for name, pr in provers.items()}


def close_all(provers):
    for pr in provers.values():
        pr.close()


@pytest.mark.parametrize("p,n,T,K,code", [(GOLD, 10, 5, 7, "rs"), (GOLD, 12, 8, 16, "rs"), (P64, 8, 3, 4, "expander")],
                         ids=["gold-10-5-7", "gold-12-8-16", "p64m59-8-3-4-expander"])
def test_prove_claims_is_accepted(pkg, p, n, T, K, code):
    ctx = ctx_of(pkg, p)
    gc.collect()
    base = pool(ctx)
    tables, provers, claims = claims_case(pkg, p, n, T, K, code, 10 * n + T)
    groups = []
    assert pkg.multiopen.prove_claims(ctx, provers, verifiers_of(pkg, p, provers), claims, random.Random(11), groups) is True
    assert groups == [(tuple(tables), K)], "one group: one joint opening"
    # a wrong claimed value is refused at the first round
    bad = list(claims)
    bad[K - 1] = bad[K - 1]._replace(value=pkg.Field(p).add(bad[K - 1].value, 1))
    with pytest.raises(pkg.multiopen.RoundMismatch) as ei:
        pkg.multiopen.prove_claims(ctx, provers, verifiers_of(pkg, p, provers), bad, random.Random(11))
    assert ei.value.round == 0
    close_all(provers)
    del tables, provers, ei          # (the exception's traceback holds the frames that hold the provers and their tables)
    gc.collect()
    assert pool(ctx) == base, "after close()"


def test_prove_claims_mixed_groups_and_single_openings(pkg):
    """two shapes and a claim alone in its group: a joint opening, the single opening, and a second joint opening, in the order of
    the first claim of each; a wrong value of the single claim is refused by name"""
    p = GOLD
    ctx, mo, F = ctx_of(pkg, p), pkg.multiopen, pkg.Field(p)
    _, pa, ca = claims_case(pkg, p, 6, 2, 3, "rs", 1)
    _, pb, cb = claims_case(pkg, p, 9, 1, 1, "rs", 2)
    _, pc, cc = claims_case(pkg, p, 7, 2, 2, "rs", 3)
    provers = {"a" + k: v for k, v in pa.items()}
    provers.update({"b" + k: v for k, v in pb.items()})
    provers.update({"c" + k: v for k, v in pc.items()})
    claims = [c._replace(table=tag + c.table) for tag, cs in (("a", ca[:1]), ("b", cb), ("c", cc), ("a", ca[1:])) for c in cs]
    groups = []
    assert mo.prove_claims(ctx, provers, verifiers_of(pkg, p, provers), claims, random.Random(2), groups) is True
    assert groups == [(("at0", "at1"), 3), (("bt0",), 1), (("ct0", "ct1"), 2)]
    bad = [c._replace(value=F.add(c.value, 1)) if c.table == "bt0" else c for c in claims]
    with pytest.raises(mo.ClaimMismatch) as ei:
        mo.prove_claims(ctx, provers, verifiers_of(pkg, p, provers), bad, random.Random(2))
    assert ei.value.table == "bt0"
    # the verifiers of one group must agree in `queries`
    vs = verifiers_of(pkg, p, provers)
    vs["at1"] = pkg.ligero_pcs.Verifier(F, 6, pa["t1"].log_cols, 1, pa["t1"].root(), QUERIES + 1)
    with pytest.raises(ValueError, match="different numbers of queries"):
        mo.prove_claims(ctx, provers, vs, claims, random.Random(2))
    close_all(provers)


class Tampering:
    """a multiopen.Prover whose one named message is changed on its way: what = ("round", j, t) | ("u_gamma", k) | ("u_z", k) |
    ("u_z kept",) | ("column", table) | ("path", table)"""

    def __init__(self, inner, F, what, log_cols):
        self.inner, self.F, self.what, self.c = inner, F, what, log_cols

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def bump(self, x):
        return self.F.add(int(x), self.F.one)

    def sumcheck(self, draw):
        def relay(j, e):
            if self.what[0] == "round" and j == self.what[1]:
                e = list(e)
                e[self.what[2]] = self.bump(e[self.what[2]])
            return draw(j, e)
        return self.inner.sumcheck(relay)

    def combine(self, gamma):
        F = self.F
        u_gamma, u_z = self.inner.combine(gamma)
        if self.what[0] == "u_gamma":
            u_gamma[self.what[1]] = self.bump(u_gamma[self.what[1]])
        if self.what[0] == "u_z":
            u_z[self.what[1]] = self.bump(u_z[self.what[1]])
        if self.what[0] == "u_z kept":         # <u_z, eq(z[:c])> stays: + w1 at word 0, - w0 at word 1
            z0 = self.inner.z[0]
            u_z[0], u_z[1] = F.add(u_z[0], z0), F.sub(u_z[1], F.sub(F.one, z0))
        return u_gamma, u_z

    def open_columns(self, indices):
        out = self.inner.open_columns(indices)
        if self.what[0] == "column":
            j, values, path = out[self.what[1]][1]
            out[self.what[1]][1] = (j, values[:-1] + [self.bump(values[-1])], path)
        if self.what[0] == "path":
            j, values, path = out[self.what[1]][0]
            sib = list(path.siblings)
            sib[-1] = bytes([sib[-1][0] ^ 0x80]) + sib[-1][1:]
            out[self.what[1]][0] = (j, values, type(path)(path.index, sib, path.field))
        return out


def group_exchange(pkg, p, provers, claims, seed, what=None, swap_roots=None, bad_claim=None):
    """prove_claims' steps for one group by hand, with one message changed"""
    mo, ctx, F = pkg.multiopen, ctx_of(pkg, p), pkg.Field(p)
    names = list(provers)
    first = provers[names[0]]
    roots = {t: provers[t].root() for t in names}
    if swap_roots:
        x, y = swap_roots
        roots[x], roots[y] = roots[y], roots[x]
    V = mo.Verifier(F, (first.num_vars, first.log_cols, first.log_blowup), roots, QUERIES, first.code)
    inner = mo.Prover(ctx, provers)
    P = Tampering(inner, F, what, first.log_cols) if what else inner
    rng = random.Random(seed)
    seen = list(claims)
    if bad_claim is not None:
        seen[bad_claim] = seen[bad_claim]._replace(value=F.add(seen[bad_claim].value, F.one))
    try:
        inner.begin(claims, V.draw_rho(seen, rng), names)
        P.sumcheck(lambda j, e: V.round(j, e, rng))
        V.receive(*P.combine(V.draw_gamma(rng)))
        return V.verify(P.open_columns(V.draw_columns(rng)))
    finally:
        inner.close()


def test_tampered_device_messages_are_refused(pkg):
    """every single tamper of the device's messages meets its own error.  Reed-Solomon over Goldilocks: a changed word of a
    combined row changes its encoding at every column (delta x^k != 0), and the row changed along (w1, -w0) at all but one, so
    which error is raised does not hang on the columns drawn"""
    p, n, T, K = GOLD, 10, 5, 7
    mo, lp, F = pkg.multiopen, pkg.ligero_pcs, pkg.Field(p)
    ctx = ctx_of(pkg, p)
    gc.collect()
    base = pool(ctx)
    tables, provers, claims = claims_case(pkg, p, n, T, K, "rs", 77)
    mid = pool(ctx)
    c = provers["t0"].log_cols
    assert group_exchange(pkg, p, provers, claims, 5) is True

    def refused(err, attrs, what=None, **kwargs):
        with pytest.raises(err) as ei:
            group_exchange(pkg, p, provers, claims, 5, what, **kwargs)
        assert type(ei.value) is err, (what, ei.value)
        for k, want in attrs.items():
            assert getattr(ei.value, k) == want, (what, k)
        assert pool(ctx) == mid, "a refused exchange gives its weight tables back"
    for k in (0, T, K - 1):
        refused(mo.RoundMismatch, {"round": 0}, bad_claim=k)
    for j in (0, n // 2, n - 1):
        for t in range(3):
            if t < 2:
                refused(mo.RoundMismatch, {"round": j}, ("round", j, t))
            elif j + 1 < n:
                refused(mo.RoundMismatch, {"round": j + 1}, ("round", j, t))
            else:
                refused(mo.FinalMismatch, {}, ("round", j, t))
    for k in (0, (1 << c) - 1):
        refused(lp.ProximityMismatch, {}, ("u_gamma", k))
        refused(mo.FinalMismatch, {}, ("u_z", k))
    refused(mo.EvalMismatch, {}, ("u_z kept",))
    for t in provers:
        refused(mo.MerkleMismatch, {"table": t}, ("column", t))
        refused(mo.MerkleMismatch, {"table": t}, ("path", t))
    refused(mo.MerkleMismatch, {"table": "t1"}, swap_roots=("t1", "t3"))
    close_all(provers)
    del tables, provers
    gc.collect()
    assert pool(ctx) == base


def test_a_fold_verifier_is_refused(pkg):
    p = GOLD
    ctx, mo, lp, F = ctx_of(pkg, p), pkg.multiopen, pkg.ligero_pcs, pkg.Field(p)
    _, provers, claims = claims_case(pkg, p, 6, 2, 3, "rs", 4)
    vs = verifiers_of(pkg, p, provers)
    vs["t1"] = lp.FoldVerifier(F, 6, provers["t1"].log_cols, 1, provers["t1"].root(), QUERIES)
    with pytest.raises(ValueError, match="joint folded opening"):
        mo.prove_claims(ctx, provers, vs, claims, random.Random(1))
    close_all(provers)


# ---- spark.prove_eval_batched ------------------------------------------------------------------------------------------

def eval_case(pkg, p, a, b, ell, seed, code):
    """test_gpu_spark's case on this file's context: a matrix of 2^l - 3 entries (padded), U = eq(r_x, .) and W = eq(r_y, .);
    the claim is M~(r_x, r_y)"""
    import spark_cases as cases
    ctx = ctx_of(pkg, p)
    triples, _, _ = cases.case(p, a, b, (1 << ell) - 3, seed)
    pick = random.Random(seed)
    rx, ry = [pick.randrange(p) for _ in range(a)], [pick.randrange(p) for _ in range(b)]
    rows, cols, vals = [t[0] for t in triples], [t[1] for t in triples], mont_np(p, [t[2] for t in triples])
    sc = pkg.spark.SparseCommitment(ctx, a, b, rows, cols, vals, commit=pkg.spark.default_commit(code=code))
    U, W = pkg.spark.table_eq(ctx, sref.mont_list(rx, p)), pkg.spark.table_eq(ctx, sref.mont_list(ry, p))
    ex, ey = sref.eq_table(rx, p), sref.eq_table(ry, p)
    return sc, U, W, (rx, ry), sum(v * ex[i] * ey[j] for i, j, v in triples) % p


L_GROUP = ("val", "er", "ec", "row", "col")
EVALS = [(GOLD, 8, 8, 10, "rs", [(L_GROUP, 7), (("cr", "cc"), 2)]),
         (GOLD, 8, 8, 8, "rs", [(L_GROUP + ("cr", "cc"), 9)]),
         (P64, 6, 6, 8, "expander", [(L_GROUP, 7), (("cr", "cc"), 2)])]


@pytest.mark.parametrize("p,a,b,ell,code,grouping", EVALS, ids=["gold-8-8-10", "gold-8-8-8", "p64m59-6-6-8-expander"])
def test_prove_eval_batched_next_to_prove_eval(pkg, p, a, b, ell, code, grouping):
    """the same instance and seed under both: the same accepted value, M~(r_x, r_y).  (8, 8, 10): the five tables of l variables
    share one joint opening, cr and cc - one shape, a = b - another.  (8, 8, 8): all seven tables have one shape: one joint opening
    of nine claims"""
    ctx, sp = ctx_of(pkg, p), pkg.spark
    gc.collect()
    base = pool(ctx)
    sc, U, W, (rx, ry), want = eval_case(pkg, p, a, b, ell, 10 * a + ell, code)
    assert sc.ell == ell
    if len(grouping) == 1:
        assert len({(pr.num_vars, pr.log_cols, pr.log_blowup, pr.code) for pr in sc.pcs.values()}) == 1, "the shapes agree"
    groups = []
    v = sp.prove_eval_batched(sc, sc.verifiers(QUERIES), U, W, eq_eval(pkg, p, rx), eq_eval(pkg, p, ry), random.Random(17), groups=groups)
    assert groups == grouping
    single = sp.prove_eval(sc, sc.verifiers(QUERIES), U, W, eq_eval(pkg, p, rx), eq_eval(pkg, p, ry), random.Random(17))
    assert v == single == sref.mont(want, p), "the accepted value is M~(r_x, r_y), as prove_eval accepts it"
    if code == "rs":         # (a FoldVerifier exists over Reed-Solomon commitments only)
        with pytest.raises(ValueError, match="folded opening"):
            sp.prove_eval_batched(sc, sc.verifiers(QUERIES, True), U, W, eq_eval(pkg, p, rx), eq_eval(pkg, p, ry), random.Random(17))
    sc.close()
    del sc, U, W
    gc.collect()
    assert pool(ctx) == base, "after close()"


def test_batched_refuses_a_changed_word_of_er(pkg, monkeypatch):
    """test_gpu_spark's dishonest prover - an er that is not U[row] in one word - under prove_eval_batched: the row lookup fails at
    the same alpha and beta (the draws before them are the same)"""
    p = GOLD
    ctx, sp = ctx_of(pkg, p), pkg.spark
    a, b, triples, Uc, Wc, er_bad, _, _ = mismatch_case(p)
    sc = sp.SparseCommitment(ctx, a, b, [t[0] for t in triples], [t[1] for t in triples], mont_np(p, [t[2] for t in triples]))
    U, W = upload(pkg, ctx, mont_np(p, Uc)), upload(pkg, ctx, mont_np(p, Wc))

    class Dishonest(sp.Prover):
        def gather_commit(self):
            _, self.ec = sp.gather(self.ctx, self.sc, self.U, self.W)
            self.er = upload(pkg, ctx, mont_np(p, er_bad))
            for name, t in (("er", self.er), ("ec", self.ec)):
                self.pcs[name] = self.commit(t)
                self.own.append(self.pcs[name])
    monkeypatch.setattr(sp, "Prover", Dishonest)
    with pytest.raises(sp.LookupMismatch) as ei:
        sp.prove_eval_batched(sc, sc.verifiers(QUERIES), U, W, lambda z: U.evaluate(z), lambda z: W.evaluate(z), random.Random(MISMATCH_SEED))
    assert ei.value.dim == "row"
    sc.close()


# ---- r1cs.prove_and_verify_sublinear_batched ---------------------------------------------------------------------------

def argue_both(pkg, p, s, m, seed, code, flip=False):
    """the same instance and witness under r1cs.prove_and_verify_sublinear and its batched form; what each returned or raised,
    and the batched form's groups"""
    rp, lp = pkg.r1cs, pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    R, io, w = rp.synthetic_instance(F, s, m, seed)
    if flip:
        col = next(j for _, j, _ in R.matrices[0] + R.matrices[1] if j >= 1 << (m - 1)) - (1 << (m - 1))
        w = list(w)
        w[col] = F.add(w[col], F.one)
    dev = rp.DeviceR1CS(ctx, R)
    c = m // 2
    instance = dev.commit_instance(code=code)
    out, groups = [], []
    try:
        for batched in (False, True):
            prover = rp.Prover(ctx, dev, io, w, log_cols=c, log_blowup=1, code=code)
            root = prover.root()
            pv = lp.Verifier(F, m - 1, c, 1, root, QUERIES, code=code)
            rng = random.Random(seed + 1)
            verifier = rp.SublinearVerifier(F, s, m, io, root, pv, instance.verifiers(QUERIES))
            try:
                if batched:
                    out.append(rp.prove_and_verify_sublinear_batched(prover, instance, verifier, rng, groups))
                else:
                    out.append(rp.prove_and_verify_sublinear(prover, instance, verifier, rng))
            except rp.Error as exc:
                out.append(exc)
            finally:
                prover.close()
    finally:
        instance.close()
        dev.close()
    return out, groups


@pytest.mark.parametrize("p,code", [(GOLD, "rs"), (P64, "expander")], ids=["gold-plain", "p64m59-expander"])
@pytest.mark.parametrize("s,m", [(6, 5), (10, 11)])
def test_batched_sublinear_argument_next_to_the_argument(pkg, p, code, s, m):
    ctx = ctx_of(pkg, p)
    gc.collect()
    base = pool(ctx)
    out, groups = argue_both(pkg, p, s, m, 31 * s + m, code)
    assert out == [True, True]
    # ten claims - SPARK's nine and the witness - and the five tables of l variables in one group
    assert sum(k for _, k in groups) == 10 and any(set(L_GROUP) <= set(t) for t, _ in groups) and any("w" in t for t, _ in groups)
    gc.collect()
    assert pool(ctx) == base


def test_a_flipped_witness_word_is_refused_by_both(pkg):
    rp = pkg.r1cs
    bad, _ = argue_both(pkg, GOLD, 6, 5, 8, "rs", flip=True)
    assert all(type(e) is rp.RoundMismatch and (e.phase, e.round) == (1, 0) for e in bad), bad


def test_batched_sublinear_refuses_a_fold_verifier(pkg):
    p, s, m = GOLD, 6, 5
    rp, lp = pkg.r1cs, pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    R, io, w = rp.synthetic_instance(F, s, m, 3)
    dev = rp.DeviceR1CS(ctx, R)
    instance = dev.commit_instance()
    prover = rp.Prover(ctx, dev, io, w, log_cols=2, log_blowup=1)
    root = prover.root()
    try:
        fv = lp.FoldVerifier(F, m - 1, 2, 1, root, QUERIES)
        with pytest.raises(ValueError, match="folded opening"):
            rp.prove_and_verify_sublinear_batched(prover, instance, rp.SublinearVerifier(F, s, m, io, root, fv, instance.verifiers(QUERIES)), random.Random(1))
        pv = lp.Verifier(F, m - 1, 2, 1, root, QUERIES)
        with pytest.raises(ValueError, match="folded opening"):
            rp.prove_and_verify_sublinear_batched(prover, instance, rp.SublinearVerifier(F, s, m, io, root, pv, instance.verifiers(QUERIES, True)),
                                                  random.Random(1))
    finally:
        prover.close()
        instance.close()
        dev.close()


# ---- refusals and the pool's books -------------------------------------------------------------------------------------

def test_refusals(pkg):
    p = GOLD
    ctx, F, mo = ctx_of(pkg, p), pkg.Field(p), pkg.multiopen
    lib = ctx.lib
    gc.collect()
    base = pool(ctx)
    out = ctypes.c_void_p()
    t1 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, np.array([5], dtype=np.uint64))
    t2, t4, t8 = (pkg.DenseMultilinearExtension.generate(ctx, k, n) for k, n in ((1, 1), (2, 2), (3, 3)))
    mid = pool(ctx)
    # sc_table_eq_sum: NULLs, count, n, an unreduced coordinate or coefficient
    pts, cf = (ctypes.c_uint64 * 4)(1, 2, 3, 4), (ctypes.c_uint64 * 2)(1, 1)
    assert lib.sc_table_eq_sum(ctx.h, None, cf, 2, 2, ctypes.byref(out)) == 1 and lib.sc_table_eq_sum(ctx.h, pts, None, 2, 2, ctypes.byref(out)) == 1
    assert lib.sc_table_eq_sum(ctx.h, pts, cf, 2, 2, None) == 1
    assert lib.sc_table_eq_sum(ctx.h, pts, cf, 0, 2, ctypes.byref(out)) == 1 and "1..16" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_table_eq_sum(ctx.h, pts, cf, 2, 0, ctypes.byref(out)) == 1 and "1..28" in lib.sc_last_error(ctx.h).decode()
    expect(pkg, 1, lambda: mo.table_eq_sum(ctx, [[1, 2]] * 17, [1] * 17), "count = 17")
    expect(pkg, 1, lambda: mo.table_eq_sum(ctx, [[1] * 29], [1]), "n = 29")
    expect(pkg, 1, lambda: mo.table_eq_sum(ctx, [[1, 2], [3, p]], [1, 1]), "coordinate 1 of point 1")
    expect(pkg, 1, lambda: mo.table_eq_sum(ctx, [[1, 2], [3, 4]], [1, p]), "coeffs[1]")
    assert not out.value
    # sc_sumprod_prove: NULLs, count, lengths, a table of one entry, an unreduced draw
    no_draw = ctypes.cast(None, pkg._lib.DRAW_FN)
    c1, fa, fb = ctypes.c_uint64(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)()
    two = (ctypes.c_void_p * 2)(t4.h, t4.h)
    hole = (ctypes.c_void_p * 2)(t4.h, None)
    assert lib.sc_sumprod_prove(ctx.h, 2, None, two, no_draw, None, 0, ctypes.byref(c1), None, None, fa, fb) == 1
    assert lib.sc_sumprod_prove(ctx.h, 2, two, None, no_draw, None, 0, ctypes.byref(c1), None, None, fa, fb) == 1
    assert lib.sc_sumprod_prove(ctx.h, 2, two, two, no_draw, None, 0, None, None, None, fa, fb) == 1
    assert lib.sc_sumprod_prove(ctx.h, 2, two, two, no_draw, None, 0, ctypes.byref(c1), None, None, None, fb) == 1
    assert lib.sc_sumprod_prove(ctx.h, 2, two, two, no_draw, None, 0, ctypes.byref(c1), None, None, fa, None) == 1
    assert lib.sc_sumprod_prove(ctx.h, 2, two, hole, no_draw, None, 0, ctypes.byref(c1), None, None, fa, fb) == 1 and "pair 1" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_sumprod_prove(ctx.h, 0, two, two, no_draw, None, 0, ctypes.byref(c1), None, None, fa, fb) == 1 and "1..8" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_sumprod_prove(ctx.h, 2, two, two, no_draw, None, 0, ctypes.byref(c1), None, None, fa, fb) == 0   # evals and challenges may be NULL
    expect(pkg, 1, lambda: mo.sumprod_prove(ctx, [t4] * 9, [t4] * 9), "count = 9")
    expect(pkg, 1, lambda: mo.sumprod_prove(ctx, [t4, t4], [t4, t8]), "pair 1 has tables of 4 and 8 entries")
    expect(pkg, 1, lambda: mo.sumprod_prove(ctx, [t4, t2], [t4, t2]), "pair 1 has tables of 2 and 2 entries, pair 0 of 4")
    expect(pkg, 1, lambda: mo.sumprod_prove(ctx, [t1], [t1]), "at least two")
    expect(pkg, 1, lambda: mo.sumprod_prove(ctx, [t4], [t4], lambda j, msg: p), "unreduced")
    # (a table whose length is no power of two cannot be made: every way to make one refuses it)
    six = np.arange(6, dtype=np.uint64)
    assert lib.sc_table_upload(ctx.h, six.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 6, ctypes.byref(out)) == 1 and not out.value
    assert pool(ctx) == mid, "a refused call leaves nothing behind"
    # tables of more than 2^28 entries are refused before they are read: a handle over 2^29 words that are never touched
    big = ctypes.c_void_p()
    assert lib.sc_table_from_device(ctx.h, ctypes.c_void_p(lib.sc_table_device_ptr(t4.h)), 1 << 29, ctypes.byref(big)) == 0
    bigs = (ctypes.c_void_p * 1)(big)
    assert lib.sc_sumprod_prove(ctx.h, 1, bigs, bigs, no_draw, None, 0, ctypes.byref(c1), None, None, fa, fb) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_table_free(ctx.h, big) == 0
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
        expect(pkg, 6, lambda: mo.table_eq_sum(other, [[1, 2]], [1]), "sc_table_eq_sum: " + msg)
        expect(pkg, 6, lambda: mo.sumprod_prove(other, [ot], [ot]), "sc_sumprod_prove: " + msg)
        assert other.lib.sc_table_eq_sum(other.h, None, None, 0, 0, None) == 6
        assert other.lib.sc_sumprod_prove(other.h, 0, None, None, no_draw, None, 0, None, None, None, None, None) == 6
        del ot
        other.close()
    # the Python layer: a table of the group without a claim, commitments of two shapes in one group
    tables, provers, claims = claims_case(pkg, p, 5, 2, 2, "rs", 9)
    P = mo.Prover(ctx, provers)
    with pytest.raises(ValueError, match="carries no claim"):
        P.begin(claims[:1], F.one, list(provers))
    other_shape = pkg.ligero_pcs.Prover.commit(ctx, provers["t1"].poly, log_cols=2)
    with pytest.raises(ValueError, match="one shape"):
        mo.Prover(ctx, {"t0": provers["t0"], "t1": other_shape}).begin(claims, F.one)
    other_shape.close()
    close_all(provers)
    del t1, t2, t4, t8, tables, provers, claims, P, other_shape
    gc.collect()
    assert pool(ctx) == base


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p):
    ctx, F, mo = ctx_of(pkg, p), pkg.Field(p), pkg.multiopen
    n, H, T = 11, 4, 3
    gc.collect()
    base = pool(ctx)
    a = [upload(pkg, ctx, ww.edge_table(p, 1 << n, np.random.default_rng(k))) for k in range(T)]
    b = [upload(pkg, ctx, ww.edge_table(p, 1 << n, np.random.default_rng(10 + k))) for k in range(T)]
    mid = pool(ctx)
    default = host_log(pkg, p)
    ctx.set_option("gp_host_log", H)
    try:
        first = mo.sumprod_prove(ctx, a, b, seed_r=3)
        assert pool(ctx) == mid, "after a proof"

        class Boom(Exception):
            pass

        def raising_at(j):
            def draw(i, msg):
                if i == j:
                    raise Boom()
                return F.one
            return draw
        for j, what in ((0, "the first device round"), (3, "a device round"), (n - H, "the first host round"), (n - 1, "the last host round")):
            with pytest.raises(Boom):
                mo.sumprod_prove(ctx, a, b, raising_at(j))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        short = a[0].fix_variables([F.one])
        short_pool = pool(ctx)
        expect(pkg, 1, lambda: mo.sumprod_prove(ctx, a, b[:2] + [short]), "pair 2")
        assert pool(ctx) == short_pool, "after a refused call"
        del short
        gc.collect()
        # the context still proves, and the same transcript
        assert mo.sumprod_prove(ctx, a, b, seed_r=3) == first
    finally:
        ctx.set_option("gp_host_log", default)
    # the eq sum hands out one table; a group's prover holds T weight tables until close()
    e = mo.table_eq_sum(ctx, [[F.one] * n], [F.one])
    assert pool(ctx)[0] == mid[0] + 1
    del e
    gc.collect()
    assert pool(ctx) == mid
    provers = {"t%d" % k: pkg.ligero_pcs.Prover.commit(ctx, t, code="rs" if p == GOLD else "expander") for k, t in enumerate(a)}
    held = pool(ctx)
    P = mo.Prover(ctx, provers)
    pt = [F.one] * n
    P.begin([mo.Claim(name, pt, t.evaluate(pt)) for name, t in zip(provers, a)], F.from_int(7))
    assert pool(ctx)[0] == held[0] + T, "one weight table per commitment"
    P.sumcheck(lambda j, msg: F.from_int(j + 2))
    assert pool(ctx)[0] == held[0] + T
    P.close()
    assert pool(ctx) == held, "after close()"
    close_all(provers)
    del a, b, provers, P
    gc.collect()
    assert pool(ctx) == base
