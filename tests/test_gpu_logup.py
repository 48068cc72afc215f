"""GPU: LogUp lookups (sc_frac_*, sc_lookup_count; thaler-study_amd/logup.py) against the big-integer reference of
tests/logup_ref.py, word for word: the fraction-sum trees at every remainder of their schedule, the proof at every hand-over to
the host, the multiplicities against numpy.bincount, the host Verifier over device messages with every single tamper, the whole
lookup over Ligero commitments, the refusals and the pool's books.

Denominators come from wide_words.edge_table with its zeros replaced by p - 2 (nonzero_table) except where a zero is the point
of the test: one zero makes Q = 0 and every claim above it 0.  Numerators keep their zeros."""
import ctypes
import gc
import random

import numpy as np
import pytest

import logup_cases as cases
import logup_ref as ref
import wide_words as ww
from logup_cases import GOLD, P61, P64
from ligero_common import context_cache, expect, mont_np
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

ctx_of, teardown_module = context_cache()
QUERIES = 8
MISMATCH_SEED = 2024
IDS = {GOLD: "gold", P64: "p64m59", P61: "p61m1"}
TAIL = 11          # kFrTailLog (tests/test_logup_cpu.py checks the package's constant against the header)
MODES = [True, False]
MODE_IDS = ["ones", "general"]


def nonzero_table(p, n, seed):
    t = ww.edge_table(p, 1 << n, np.random.default_rng(seed))
    t[t == 0] = p - 2
    return t


def upload(pkg, ctx, t):
    return pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, len(t).bit_length() - 1, np.ascontiguousarray(t, dtype=np.uint64))


def defaults(pkg, p):
    """the context's fr_host_log and fr_tree_lv as it was created (the tests put them back)"""
    ctx = ctx_of(pkg, p)
    if not hasattr(ctx, "_fr_default"):
        ctx._fr_default = (ctx.get_option("fr_host_log"), ctx.get_option("fr_tree_lv"))
    return ctx._fr_default


def tables(p, n, seed, ones):
    """(p words or None, q words)"""
    return (None if ones else ww.edge_table(p, 1 << n, np.random.default_rng(seed + 1000))), nonzero_table(p, n, seed)


_REF = {}


def reference(p, n, seed, ones):
    """(p words, q words, tree layers, canonical challenges, reference proof dict): computed once, shared, never changed"""
    key = (p, n, seed, ones)
    if key not in _REF:
        pt, qt = tables(p, n, seed, ones)
        pc, qc = (None if ones else ref.canon_list(pt, p)), ref.canon_list(qt, p)
        layers = ref.tree(pc, qc, p)
        rng = random.Random(seed + 1)
        ch = [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(ref.n_challenges(n))]
        it = iter(ch)
        _REF[key] = (pt, qt, layers, ch, ref.prove(pc, qc, p, lambda k, j, msg: next(it), layers=layers))
    return _REF[key]


def make_tree(pkg, ctx, pt, qt):
    q = upload(pkg, ctx, qt)
    p_table = upload(pkg, ctx, pt) if pt is not None else None
    return pkg.logup.FractionTree(ctx, q, p_table), p_table, q


# ---- the trees -------------------------------------------------------------------------------------------------------

TREE_SIZES = [(GOLD, n) for n in range(1, 16)] + [(P64, n) for n in (1, 2, 3, TAIL - 1, TAIL, TAIL + 1, TAIL + 2, TAIL + 3)]


def check_tree(pkg, p, pt, qt):
    ctx = ctx_of(pkg, p)
    n = len(qt).bit_length() - 1
    P, Q = ref.tree(None if pt is None else ref.canon_list(pt, p), ref.canon_list(qt, p), p)
    tree, p_table, q_table = make_tree(pkg, ctx, pt, qt)
    assert tree.num_vars == n and tree.root == (ref.mont(P[0][0], p), ref.mont(Q[0][0], p))
    for k in range(n):
        for which, want in ((0, P[k]), (1, Q[k])):
            got = tree.layer(k, which).to_evaluations()
            assert got.shape == (1 << k,) and np.array_equal(got, mont_np(p, want)), (n, k, which)
    assert np.array_equal(q_table.to_evaluations(), qt), "q is unchanged"
    if pt is not None:
        assert np.array_equal(p_table.to_evaluations(), pt), "p is unchanged"
    tree.close()
    return P, Q


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("p,n", TREE_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in TREE_SIZES])
def test_tree_root_and_every_layer(pkg, p, n, ones):
    """n = 1 .. 11: the tail kernel alone; above it the launches of the default fr_tree_lv (tree_schedule).  The numerators
    carry the edge words 0, 1 and p - 1"""
    assert pkg.logup.TAIL_LOG == TAIL
    pt, qt = tables(p, n, 40 + n, ones)
    check_tree(pkg, p, pt, qt)


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("lv", [1, 2, 3])
@pytest.mark.parametrize("n", [12, 13, 14, 15])
def test_tree_at_every_number_of_layers_per_launch(pkg, n, lv, ones):
    """n - 11 = 1 .. 4 layers above the tail: every remainder of every fr_tree_lv, a launch of every instantiated LV among them"""
    ctx = ctx_of(pkg, GOLD)
    _, default = defaults(pkg, GOLD)
    ctx.set_option("fr_tree_lv", lv)
    try:
        check_tree(pkg, GOLD, *tables(GOLD, n, 70 + n, ones))
    finally:
        ctx.set_option("fr_tree_lv", default)


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [5, 14])
def test_tree_with_one_zero_denominator(pkg, n, ones):
    for at in (0, 1 << (n - 1), (1 << n) - 1):
        pt, qt = tables(GOLD, n, 3 * n, ones)
        qt[at] = 0
        P, Q = check_tree(pkg, GOLD, pt, qt)
        assert Q[0] == [0] and all(sum(1 for x in layer if x == 0) == 1 for layer in Q)


def tree_schedule(n, lv):
    """[(kf, log_in)] of the launches of a tree build"""
    out, m = [], n
    while m > TAIL:
        step = min(lv, m - TAIL)
        out.append((step, m))
        m -= step
    return out + [(0, m)]


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [9, 12, 13, 14, 16])
def test_tree_launch_log(pkg, n, ones):
    ctx = ctx_of(pkg, GOLD)
    q = pkg.DenseMultilinearExtension.generate(ctx, 3, n)
    p_table = None if ones else pkg.DenseMultilinearExtension.generate(ctx, 4, n)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    tree = pkg.logup.FractionTree(ctx, q, p_table)
    log = [x for x in ctx.launch_log() if x["kind"] == "fraction_tree"]
    ctx.set_option("time_kernels", 0)
    tree.close()
    assert [(x["kf"], x["log_in"]) for x in log] == tree_schedule(n, defaults(pkg, GOLD)[1])
    assert tree_schedule(16, 2) == [(2, 16), (2, 14), (1, 12), (0, 11)] and tree_schedule(16, 3) == [(3, 16), (2, 13), (0, 11)]
    for x in log:
        m, lv = x["log_in"], x["kf"]
        read_tables = 1 if ones and m == n else 2          # the all-ones numerator is not read
        assert x["ks"] == read_tables and x["bytes_read"] == read_tables * (8 << m)
        assert x["bytes_written"] == 2 * ((8 << m) - (8 << (m - lv) if lv else 8))


# ---- the proof -------------------------------------------------------------------------------------------------------

def expected_calls(n):
    """(layer, round, message words) of every draw, in order"""
    out = []
    for k in range(n):
        out += [(k, j, 4) for j in range(k)] + [(k, k, 4)]
        if k + 1 < n:
            out.append((k, k + 1, 0))
    return out


def device_proof(pkg, p, pt, qt, ch_canon, T):
    """sc_frac_prove at fr_host_log = T under the fixed challenges; the draw also checks the order it is called in"""
    ctx = ctx_of(pkg, p)
    n = len(qt).bit_length() - 1
    words = ref.mont_list(ch_canon, p)
    seen = []

    def draw(layer, j, msg):
        seen.append((layer, j, len(msg)))
        return words[len(seen) - 1]
    base, _ = defaults(pkg, p)
    ctx.set_option("fr_host_log", T)
    try:
        tree, _, _ = make_tree(pkg, ctx, pt, qt)
        proof = pkg.logup.prove(tree, draw)
        tree.close()
    finally:
        ctx.set_option("fr_host_log", base)
    assert seen == expected_calls(n)
    return proof


def assert_same(pkg, p, proof, want):
    """bit for bit: the root, all 4 n (n-1) / 2 values, the finals, the point, the claims (and the challenges handed back)"""
    assert proof == cases.as_proof(pkg, want, p)


def hand_overs(pkg, p, extra=()):
    return sorted(set([0, defaults(pkg, p)[0]]) | set(extra))


PROOF_SIZES = [(GOLD, n) for n in range(1, 14)] + [(p, n) for p in (P64, P61) for n in (1, 2, 7, 12)]


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("p,n", PROOF_SIZES, ids=["%s-%d" % (IDS[p], n) for p, n in PROOF_SIZES])
def test_proof_is_the_reference_bit_for_bit(pkg, p, n, ones):
    """fr_host_log = 0 (every round on the device) and the default; at n = 5 and 9 on Goldilocks also 1, 3, n - 1 (the hand-over at
    the first possible launch), n (no device round at all) and 12 (above n).  Challenges from {0, 1, p - 1, random}"""
    pt, qt, _, ch, want = reference(p, n, 500 + n, ones)
    extra = (1, 3, n - 1, n, 12) if p == GOLD and n in (5, 9) else ()
    proofs = []
    for T in hand_overs(pkg, p, extra):
        proofs.append(device_proof(pkg, p, pt, qt, ch, T))
        assert_same(pkg, p, proofs[-1], want)
    assert all(q == proofs[0] for q in proofs[1:]), "transcripts at different fr_host_log are identical"
    if ones:
        one = ref.mont(1, p)
        assert proofs[0].finals[n - 1][:2] == (one, one) and proofs[0].claims[0] == one


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
def test_proof_over_a_zero_denominator(pkg, ones):
    pt, qt = tables(GOLD, 10, 9, ones)
    qt[517] = 0
    pc, qc = (None if ones else ref.canon_list(pt, GOLD)), ref.canon_list(qt, GOLD)
    rng = random.Random(2)
    ch = [rng.randrange(GOLD) for _ in range(ref.n_challenges(10))]
    it = iter(ch)
    want = ref.prove(pc, qc, GOLD, lambda k, j, msg: next(it))
    assert want["root"][1] == 0
    for T in hand_overs(pkg, GOLD):
        assert_same(pkg, GOLD, device_proof(pkg, GOLD, pt, qt, ch, T), want)


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
def test_n20_is_accepted_by_the_host_verifier(pkg, ones):
    p, n = GOLD, 20
    ctx, lu = ctx_of(pkg, p), pkg.logup
    pt, qt = tables(p, n, 20, ones)
    tree, p_table, q_table = make_tree(pkg, ctx, pt, qt)
    proof = lu.prove(tree, seed_r=77)
    V = lu.Verifier(pkg.Field(p), n, ones=ones)
    assert V.verify(proof, proof.challenges) == (proof.point,) + proof.claims
    assert V.check_input(q_table.evaluate(proof.point), None if ones else p_table.evaluate(proof.point))
    tree.close()


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
def test_proof_launch_log(pkg, ones):
    """layers <= T leave no record; with an all-ones numerator the passes of the top layer read three tables, every other five"""
    p, n = GOLD, 13
    ctx, T = ctx_of(pkg, p), defaults(pkg, p)[0]
    tree, _, _ = make_tree(pkg, ctx, *tables(p, n, 1, ones))
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    pkg.logup.prove(tree, seed_r=1)
    log = [x for x in ctx.launch_log() if x["kind"] == "fraction_pass"]
    ctx.set_option("time_kernels", 0)
    tree.close()
    te = max(T, 1)
    want = []
    for k in range(T + 1, n):
        nt = 3 if ones and k == n - 1 else 5
        want.append((0, k, nt))                         # round 0 reads the layer's tables
        want += [(1, k - j + 1, nt) for j in range(1, k - te + 1)]
    assert want and [(x["kf"], x["log_in"], x["ks"]) for x in log] == want
    for x in log:
        assert x["bytes_read"] == (8 * x["ks"]) << x["log_in"]
        assert x["bytes_written"] == (((8 * x["ks"]) << (x["log_in"] - 1)) if x["kf"] else 0)


# ---- the multiplicities ----------------------------------------------------------------------------------------------

COUNT_SHAPES = [(1, 1), (5, 8), (13, 13), (16, 13), (16, 14), (12, 16)]


def idx_patterns(n, m, rng):
    N, M = 1 << n, 1 << m
    out = {"uniform": rng.integers(0, M, size=N), "zeros": np.zeros(N, dtype=np.int64), "last": np.full(N, M - 1),
           "two": np.where(rng.random(N) < 0.5, 1 % M, M - 2 if M > 2 else 0)}
    if n == m:
        out["permutation"] = rng.permutation(N)
    return {k: v.astype(np.uint32) for k, v in out.items()}


@pytest.mark.parametrize("n,m", COUNT_SHAPES, ids=["%d-%d" % s for s in COUNT_SHAPES])
def test_lookup_count_is_bincount(pkg, n, m):
    """m = 13 is the last size counted in LDS histograms, m = 14 the first counted in global memory"""
    p = GOLD
    ctx, lu = ctx_of(pkg, p), pkg.logup
    assert lu.LOOKUP_LDS_LOG == 13
    rng = np.random.default_rng(100 * n + m)
    t = rng.permutation(1 << 20)[:1 << m].astype(np.uint64) + np.uint64(5)     # distinct words
    table = upload(pkg, ctx, t)
    ctx.set_option("time_kernels", 1)
    for name, idx in idx_patterns(n, m, rng).items():
        w = upload(pkg, ctx, t[idx])
        ctx.launch_log()
        mult, bad = lu.multiplicities(ctx, w, table, idx)
        log = [(x["kf"], x["ks"], x["log_in"]) for x in ctx.launch_log() if x["kind"] == "lookup_count"]
        assert log == [(0, 1 if m <= 13 else 0, n), (1, 0, m)], name
        want = np.bincount(idx, minlength=1 << m)
        assert bad == 0 and np.array_equal(mult.to_evaluations(), mont_np(p, want)), name
    ctx.set_option("time_kernels", 0)
    assert np.array_equal(table.to_evaluations(), t)


@pytest.mark.parametrize("n,m", [(5, 8), (16, 13), (16, 14)], ids=["5-8", "16-13", "16-14"])
def test_lookup_count_leaves_mismatches_out(pkg, n, m):
    p = GOLD
    ctx, lu = ctx_of(pkg, p), pkg.logup
    rng = np.random.default_rng(n + m)
    N = 1 << n
    t = rng.permutation(1 << 20)[:1 << m].astype(np.uint64) + np.uint64(5)
    idx = rng.integers(0, 1 << m, size=N).astype(np.uint32)
    table = upload(pkg, ctx, t)
    for name, change in (("first w", (0, "w")), ("last w", (N - 1, "w")), ("idx = 2^m", (N // 3, 1 << m)), ("idx = 2^32 - 1", (N // 2, 0xFFFFFFFF))):
        at, what = change
        w, bad_idx = t[idx].copy(), idx.copy()
        if what == "w":
            w[at] = 3                              # no word of t
        else:
            bad_idx[at] = what
        mult, bad = lu.multiplicities(ctx, upload(pkg, ctx, w), table, bad_idx)
        want = np.bincount(np.delete(idx, at), minlength=1 << m)
        assert bad == 1 and np.array_equal(mult.to_evaluations(), mont_np(p, want)), name
    # all three at once
    w, bad_idx = t[idx].copy(), idx.copy()
    w[0], w[N - 1], bad_idx[N // 2] = 3, 3, 1 << m
    mult, bad = lu.multiplicities(ctx, upload(pkg, ctx, w), table, bad_idx)
    assert bad == 3 and np.array_equal(mult.to_evaluations(), mont_np(p, np.bincount(np.delete(idx, [0, N // 2, N - 1]), minlength=1 << m)))


# ---- the argument ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_host_verifier_over_device_messages(pkg, p, ones):
    """an honest device proof is accepted, every single tamper of it is refused by its own error (challenges are random words
    >= 4: tests/test_logup_cpu.py says why), a changed input word by the last check"""
    lu, F, n = pkg.logup, pkg.Field(p), 6
    ctx = ctx_of(pkg, p)
    pt, qt = tables(p, n, 31, ones)
    rng = random.Random(8)
    ch = [rng.randrange(4, p) for _ in range(ref.n_challenges(n))]
    proof = device_proof(pkg, p, pt, qt, ch, defaults(pkg, p)[0])
    V = lu.Verifier(F, n, ones=ones)
    assert V.verify(proof, proof.challenges) == (proof.point,) + proof.claims
    q_value = upload(pkg, ctx, qt).evaluate(proof.point)
    p_value = None if ones else upload(pkg, ctx, pt).evaluate(proof.point)
    assert V.check_input(q_value, p_value)
    for name, where, expected in cases.tampers(n):
        bad, words = cases.apply_tamper(pkg, proof, where, F)
        cases.expect_refusal(pkg, lu.Verifier(F, n, ones=ones), bad, words, expected)
    q2 = qt.copy()
    q2[37] = F.add(int(q2[37]), F.one)
    with pytest.raises(lu.InputMismatch):
        V.check_input(upload(pkg, ctx, q2).evaluate(proof.point), p_value)
    if not ones:
        with pytest.raises(lu.NumeratorMismatch):
            lu.Verifier(F, n, ones=True).verify(proof, proof.challenges)


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


def lookup(pkg, p, w, t, idx, code, opening, seed, range_table):
    ctx, F, lu = ctx_of(pkg, p), pkg.Field(p), pkg.logup
    pw, vw = committed(pkg, p, w, code, opening)
    try:
        table_eval = (lambda point: lu.range_table_eval(F, point)) if range_table else None
        return lu.prove_lookup(pw, vw, upload(pkg, ctx, t), idx, random.Random(seed), table_eval=table_eval)
    finally:
        pw.close()


def lookup_tables(p, n, m, range_table, seed):
    """(w words, t words, idx)"""
    rng = np.random.default_rng(seed)
    if range_table:
        t = mont_np(p, list(range(1 << m)))
    else:
        # distinct words, the edge words among them: the table has a quarter of edge words, a dozen distinct, and 3 * 2^(m-1)
        # uniform ones, which np.unique leaves distinct and sorted
        u = np.unique(ww.edge_table(p, 1 << (m + 1), rng, share=0.25))
        edge = np.array(ww.edge_words(p), dtype=np.uint64)
        rest = u[~np.isin(u, edge)]
        assert rest.size + edge.size >= 1 << m
        t = np.concatenate([edge, rest[rng.permutation(rest.size)]])[:1 << m]
        t = t[rng.permutation(1 << m)]
    idx = rng.integers(0, 1 << m, size=1 << n).astype(np.uint32)
    return t[idx], t, idx


LOOKUPS = [(GOLD, 12, 8, True, "rs", "plain"), (GOLD, 12, 8, True, "rs", "folded"), (P64, 10, 10, False, "expander", "plain"), (GOLD, 8, 10, False, "rs", "plain")]


@pytest.mark.parametrize("p,n,m,range_table,code,opening", LOOKUPS, ids=["gold-12-8-range-plain", "gold-12-8-range-folded", "p64m59-10-10-expander", "gold-8-10"])
def test_lookup_is_accepted(pkg, p, n, m, range_table, code, opening):
    w, t, idx = lookup_tables(p, n, m, range_table, n + m)
    if range_table:
        assert np.array_equal(pkg.logup.range_indices(pkg.Field(p), w), idx)
    assert lookup(pkg, p, w, t, idx, code, opening, 17, range_table) is True


def mismatch_case(p):
    """(w, t, mult, alpha) in canonical integers: a lookup of 2^10 entries into the range table of 2^8 with one w_i moved outside
    t, the multiplicities sc_lookup_count then forms, and the alpha MISMATCH_SEED draws first (tests/test_logup_cpu.py checks on
    the CPU that the two fraction sums differ there)"""
    n, m = 10, 8
    rng = np.random.default_rng(6)
    idx = [int(x) for x in rng.integers(0, 1 << m, size=1 << n)]
    t = list(range(1 << m))
    w = [t[j] for j in idx]
    w[123] = 1 << m
    mult, bad = ref.multiplicities(w, t, idx)
    assert bad == 1
    alpha = random.Random(MISMATCH_SEED).randrange(p)                 # Field.rand of a random.Random: one randrange(p), canonical
    return w, t, mult, alpha


def test_lookup_with_an_entry_outside_the_table_is_refused(pkg):
    p = GOLD
    w, t, mult, alpha = mismatch_case(p)
    assert pkg.Field(p).rand(random.Random(MISMATCH_SEED)) == ref.mont(alpha, p), "mismatch_case draws alpha as the field does"
    idx = np.random.default_rng(6).integers(0, 1 << 8, size=1 << 10).astype(np.uint32)   # mismatch_case's: the prover still claims idx[123]
    with pytest.raises(pkg.logup.LookupMismatch) as ei:
        lookup(pkg, p, mont_np(p, w), mont_np(p, t), idx, "rs", "plain", MISMATCH_SEED, True)
    P_w, Q_w = (x[0][0] for x in ref.tree(None, [(alpha - x) % p for x in w], p))
    P_t, Q_t = (x[0][0] for x in ref.tree(mult, [(alpha - x) % p for x in t], p))
    assert (ei.value.root_w, ei.value.root_t) == (tuple(ref.mont_list((P_w, Q_w), p)), tuple(ref.mont_list((P_t, Q_t), p)))


def test_lookup_layer_refuses_a_field_too_small_for_the_counts(pkg):
    """p = 257 with n = 10: a count may reach 2^10"""
    p, n, m = 257, 10, 3
    ctx, lu = ctx_of(pkg, p), pkg.logup
    t = mont_np(p, list(range(1 << m)))
    idx = np.random.default_rng(1).integers(0, 1 << m, size=1 << n).astype(np.uint32)
    base = pool(ctx)
    w, table = upload(pkg, ctx, t[idx]), upload(pkg, ctx, t)
    expect(pkg, 6, lambda: lu.multiplicities(ctx, w, table, idx), "sc_lookup_count", "2^10")
    pw, vw = committed(pkg, p, t[idx], "expander", "plain")
    try:
        with pytest.raises(ValueError):
            lu.prove_lookup(pw, vw, table, idx, random.Random(1))
    finally:
        pw.close()
        del pw, vw
    # the fraction sum itself runs over 257
    tree = lu.FractionTree(ctx, upload(pkg, ctx, nonzero_table(p, 6, 1)))
    proof = lu.prove(tree, seed_r=5)
    assert lu.Verifier(pkg.Field(p), 6, ones=True).verify(proof, proof.challenges) == (proof.point,) + proof.claims
    tree.close()
    del w, table, tree
    gc.collect()
    assert pool(ctx) == base


# ---- refusals and the pool's books -----------------------------------------------------------------------------------

def pool(ctx):
    return ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")


def test_refusals(pkg):
    p = GOLD
    ctx, F, lu = ctx_of(pkg, p), pkg.Field(p), pkg.logup
    lib = ctx.lib
    gc.collect()
    base = pool(ctx)
    t1 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, np.array([5], dtype=np.uint64))
    t4 = pkg.DenseMultilinearExtension.generate(ctx, 1, 4)
    t3 = pkg.DenseMultilinearExtension.generate(ctx, 2, 3)
    h, out = ctypes.c_void_p(), ctypes.c_void_p()
    idx16 = (ctypes.c_uint32 * 16)()
    bad = ctypes.c_uint64()
    # sc_frac_create: NULLs, a length below two, two lengths
    assert lib.sc_frac_create(ctx.h, None, None, ctypes.byref(h)) == 1 and lib.sc_frac_create(ctx.h, None, t4.h, None) == 1
    expect(pkg, 1, lambda: lu.FractionTree(ctx, t1), "at least two")
    expect(pkg, 1, lambda: lu.FractionTree(ctx, t4, t3), "p has 8 entries, q has 16")
    # sc_lookup_count: NULLs, a length below two
    assert lib.sc_lookup_count(ctx.h, None, t4.h, idx16, ctypes.byref(out), ctypes.byref(bad)) == 1
    assert lib.sc_lookup_count(ctx.h, t4.h, None, idx16, ctypes.byref(out), ctypes.byref(bad)) == 1
    assert lib.sc_lookup_count(ctx.h, t4.h, t4.h, None, ctypes.byref(out), ctypes.byref(bad)) == 1
    assert lib.sc_lookup_count(ctx.h, t4.h, t4.h, idx16, None, ctypes.byref(bad)) == 1
    assert lib.sc_lookup_count(ctx.h, t4.h, t4.h, idx16, ctypes.byref(out), None) == 1 and not out.value
    assert lib.sc_lookup_count(ctx.h, t1.h, t4.h, idx16, ctypes.byref(out), ctypes.byref(bad)) == 1 and "at least two" in lib.sc_last_error(ctx.h).decode()
    with pytest.raises(ValueError):
        lu.multiplicities(ctx, t4, t4, np.zeros(8, dtype=np.uint32))
    gc.collect()
    assert pool(ctx)[0] == base[0] + 3                                        # t1, t3 and t4 alone: a refused call leaves nothing behind
    tree = lu.FractionTree(ctx, t4)
    # sc_frac_layer: k >= n, which, NULLs
    expect(pkg, 1, lambda: tree.layer(4, 0), "layer 4")
    expect(pkg, 1, lambda: tree.layer(0, 2), "which = 2")
    assert lib.sc_frac_layer(ctx.h, tree.h, 0, 0, None) == 1 and lib.sc_frac_layer(ctx.h, None, 0, 0, ctypes.byref(out)) == 1
    assert lib.sc_frac_root(None, None) == 1
    # sc_frac_prove: NULLs, an unreduced draw
    no_draw = ctypes.cast(None, pkg._lib.DRAW_FRAC_FN)
    fin, point, claims = (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 2)()
    assert lib.sc_frac_prove(ctx.h, tree.h, no_draw, None, 0, None, None, None, point, claims) == 1
    assert lib.sc_frac_prove(ctx.h, tree.h, no_draw, None, 0, None, fin, None, None, claims) == 1
    assert lib.sc_frac_prove(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, None) == 1
    assert lib.sc_frac_prove(ctx.h, None, no_draw, None, 0, None, fin, None, point, claims) == 1
    assert lib.sc_frac_prove(ctx.h, tree.h, no_draw, None, 0, None, fin, None, point, claims) == 0   # evals and challenges may be NULL
    expect(pkg, 1, lambda: lu.prove(tree, lambda k, j, msg: p), "unreduced")
    # the options' ranges
    expect(pkg, 1, lambda: ctx.set_option("fr_host_log", 13), "fr_host_log")
    expect(pkg, 1, lambda: ctx.set_option("fr_host_log", -1), "fr_host_log")
    expect(pkg, 1, lambda: ctx.set_option("fr_tree_lv", 0), "fr_tree_lv")
    expect(pkg, 1, lambda: ctx.set_option("fr_tree_lv", 4), "fr_tree_lv")
    # p = 3: the cubic through 0 .. 3 does not exist
    c3 = pkg.Context(pkg.Field(3))
    s3 = pkg.DenseMultilinearExtension.from_evaluations_vec(c3, 1, np.array([1, 2], dtype=np.uint64))
    expect(pkg, 6, lambda: lu.FractionTree(c3, s3), "p = 3")
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
        expect(pkg, 6, lambda: lu.FractionTree(other, ot), "sc_frac_create: " + msg)
        expect(pkg, 6, lambda: lu.multiplicities(other, ot, ot, np.zeros(8, dtype=np.uint32)), "sc_lookup_count: " + msg)
        assert other.lib.sc_frac_create(other.h, None, None, None) == 6
        assert other.lib.sc_lookup_count(other.h, None, None, None, None, None) == 6
        assert other.lib.sc_frac_layer(other.h, tree.h, 0, 0, ctypes.byref(out)) == 6 and not out.value
        assert other.lib.sc_frac_prove(other.h, tree.h, no_draw, None, 0, None, fin, None, point, claims) == 6
        del ot
        other.close()
    # n > 28 is refused before the tables are read: a table handle over 2^29 words that are never touched
    big = ctypes.c_void_p()
    assert lib.sc_table_from_device(ctx.h, ctypes.c_void_p(lib.sc_table_device_ptr(t4.h)), 1 << 29, ctypes.byref(big)) == 0
    assert lib.sc_frac_create(ctx.h, None, big, ctypes.byref(h)) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode() and not h.value
    assert lib.sc_lookup_count(ctx.h, big, t4.h, idx16, ctypes.byref(out), ctypes.byref(bad)) == 1 and "2^28" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_table_free(ctx.h, big) == 0
    tree.close()
    del t1, t3, t4
    gc.collect()
    assert pool(ctx) == base


@pytest.mark.parametrize("ones", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_pool_books_balance(pkg, p, ones):
    ctx, F, lu = ctx_of(pkg, p), pkg.Field(p), pkg.logup
    n, T = 11, 4
    gc.collect()
    base = pool(ctx)
    pt, qt = tables(p, n, 2, ones)
    tree, p_table, q_table = make_tree(pkg, ctx, pt, qt)
    mid = pool(ctx)
    assert mid[0] == base[0] + (3 if ones else 4), "the trees are two pool blocks"
    default, _ = defaults(pkg, p)
    ctx.set_option("fr_host_log", T)
    try:
        lu.prove(tree, seed_r=3)
        assert pool(ctx) == mid, "after a proof"

        class Boom(Exception):
            pass

        def raising_at(layer, j):
            def draw(k, i, msg):
                if (k, i) == (layer, j):
                    raise Boom()
                return F.one
            return draw
        for where, what in (((9, 2), "a device round"), ((9, 7), "a host round of a device layer"), ((3, 1), "a round of a host layer"), ((9, 9), "a rho"),
                            ((8, 9), "the lambda of a device layer"), ((2, 3), "the lambda of a host layer")):
            with pytest.raises(Boom):
                lu.prove(tree, raising_at(*where))
            assert pool(ctx) == mid, "after a draw that raised in " + what
        # the context still proves, and the same transcript
        assert lu.prove(tree, seed_r=3) == lu.prove(tree, seed_r=3)
    finally:
        ctx.set_option("fr_host_log", default)
    tree.close()
    del p_table, q_table
    gc.collect()
    assert pool(ctx) == base
