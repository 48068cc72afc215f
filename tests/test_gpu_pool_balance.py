"""The device-buffer pool's books balance: whatever a call allocates goes back when the call, or the object it made, is done.

Every case reads "stat_pool_live_blocks" / "stat_pool_live_words" (sc_ctx_get_option) as a baseline, runs a workload, drops
everything the workload made and expects both counts back at the baseline - on success and after a rejected call.  The
values the workloads compute are checked against the oracle only where that is one line; the other suites cover values.
test_peak_words_equal_the_parents pins the high-water mark of a fixed list of calls to the figures of the commit before the
buffers got owners: a release that moves later shows there as a larger peak.

Shapes: the smallest that reach each allocation pattern (every branch of fold_chain, one and several chunks of the column
dot, the matrix-core square with its byte planes, the batch's four blocks, one prover more than there are tail slots)."""
import gc
import random

import numpy as np
import pytest

from conftest import load_package
from test_gpu_gkr import make_circuit, random_circuit
from test_gpu_multi import device_list
from test_gpu_triangle import random_adj
from test_host_protocols import BOOK
from util import GOLD, TOY_MODULI, challenges, oracle, pid, pyref

pytestmark = pytest.mark.gpu

FIELDS = [GOLD, TOY_MODULI[2]]
ORDER_LE, ORDER_BE = 0, 1
WFOLD_SMALL = {"first_pass_vars": 4, "wfold_min_log": 12, "wfold_always": 1}   # tests/test_gpu_wfold.py

_ctx = {}


def ctx_of(pkg, p):
    """one ordinary context per field for the whole file"""
    if p not in _ctx:
        _ctx[p] = pkg.Context(pkg.Field(p))
    return _ctx[p]


def teardown_module(module):
    for ctx in _ctx.values():
        ctx.close()
    _ctx.clear()


def pool(ctx):
    return ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")


def balanced(ctx, workload, **options):
    """run workload() (its locals die with it) under `options`, collect, and expect the pool where it was"""
    keep = {k: ctx.get_option(k) for k in options}
    base = pool(ctx)
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        workload()
    finally:
        for k, v in keep.items():
            ctx.set_option(k, v)
    gc.collect()
    assert pool(ctx) == base, "blocks / words out of the pool: %r before, %r after" % (base, pool(ctx))


def product(pkg, ctx, n):
    mle = pkg.DenseMultilinearExtension
    return pkg.matrix_multiplication.G(mle.generate(ctx, pyref.SEED_A, n), mle.generate(ctx, pyref.SEED_B, n))


def prove_both_forms(pkg, ctx, n, check=True):
    """sc_prove and the round-by-round prover over one pair of tables; against the oracle up to 2^13 entries"""
    g = product(pkg, ctx, n)
    c1, evals, ch = pkg.matrix_multiplication.prove(ctx, g, pyref.SEED_R)
    native = g.native_prover()
    rounds = [native.round_evals(ctx.field.one if j == 0 else int(ch[j - 1]), j) for j in range(n)]
    assert native.c1() == c1 and np.array_equal(np.array(rounds, dtype=np.uint64).reshape(n, 3), evals)
    if check and n <= 13:
        o = oracle(ctx.field.p)
        ref = o.prove(o.generate(pyref.SEED_A, n), o.generate(pyref.SEED_B, n), challenges(o, n))
        assert c1 == ref["c_1"] and np.array_equal(evals, ref["evals"])


# ---- product prover ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 6, 13, 20])
@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_product_prover(p, n):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    balanced(ctx, lambda: prove_both_forms(pkg, ctx, n))


@pytest.mark.parametrize("n,options", [(14, WFOLD_SMALL), (13, {"use_mailbox": 0}), (13, {"host_tail_log": 0}), (13, {"vars_per_pass": 1})],
                         ids=["wfold", "no_mailbox", "no_host_tail", "one_round_passes"])
@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_product_prover_options(p, n, options):
    """the matrix-core first pass with the five-round fold behind it; sums by copy; the device serves every round; one round per pass"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    balanced(ctx, lambda: prove_both_forms(pkg, ctx, n), **options)


@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_more_provers_than_tail_slots(p):
    """33 provers alive at once: the context has 32 tail slots, so one prover runs without one.  (At n = 6 a block count
    cannot single that prover out: the last pass of every prover leaves no round to hand over, so it folds into pool memory
    with or without a slot.  What the case shows is that all 33 finish with the oracle's sums and give everything back.)"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    n, o = 6, oracle(p)
    ch = challenges(o, n)
    ref = o.prove(o.generate(pyref.SEED_A, n), o.generate(pyref.SEED_B, n), ch)

    def workload():
        g = product(pkg, ctx, n)
        provers = [g.native_prover() for _ in range(33)]
        for j in range(n):
            for pr in provers:
                assert pr.round_evals(ctx.field.one if j == 0 else int(ch[j - 1]), j) == [int(x) for x in ref["evals"][j]]
        assert pool(ctx)[0] > base[0]

    base = pool(ctx)
    balanced(ctx, workload)


# ---- tables ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,k", [(ORDER_LE, k) for k in (0, 1, 3, 5, 10, 16)] + [(ORDER_BE, k) for k in (1, 3, 5)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_fix_variables(p, order, k):
    """n = 16.  LE: every branch of fold_chain (the k = 0 copy, three variables per pass, five on a small table, the segment
    pass from eight up, mixes of them).  BE: one fold at k = 1, the column dot from k = 2 - with one chunk of rows at
    k = 3 and, with 32 rows at k = 5, several chunks and their block of partial rows"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    o = oracle(p)
    r = [int(x) for x in challenges(o, k)]

    def workload():
        t = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A, 16)
        ctx.launch_log()
        out = t.fix_variables(r, order)
        assert len(out) == 1 << (16 - k)
        kinds = [rec["kind"] for rec in ctx.launch_log()]
        if order == ORDER_BE and k >= 2:
            assert "coldot" in kinds, kinds
        # the same polynomial either way: its value at a point of the remaining variables
        rest = [int(x) for x in challenges(o, 16 - k, seed=pyref.SEED_R + 7)]
        assert out.evaluate(rest, order) == t.evaluate(r + rest, order)

    balanced(ctx, workload, time_kernels=1)


@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_evaluate_and_relabel(p):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    o = oracle(p)
    n = 12

    def workload():
        t = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A, n)
        pts = [[int(x) for x in challenges(o, n, seed=pyref.SEED_R + s)] for s in range(5)]
        vals = t.evaluate_many(pts)
        assert vals == [t.evaluate(pt) for pt in pts]
        assert t.evaluate(pts[0], ORDER_BE) == t.evaluate(pts[0][::-1])
        sw = t.relabel(0, 6, 6)
        assert sw.evaluate(pts[0][6:] + pts[0][:6]) == vals[0]
        small = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_B, 5)   # below 2^8 entries: evaluate through a fold chain
        assert small.evaluate(pts[0][:5]) == small.fix_variables(pts[0][:4]).evaluate(pts[0][4:5])

    balanced(ctx, workload)


# ---- GKR W -------------------------------------------------------------------------------------------------------------

def gkr_layer(pkg, ctx, k, seed=11):
    """a random layer of 2^k gates over 2^k values: the circuit, its evaluation (Montgomery words) and a point r_i"""
    F = ctx.field
    rng = random.Random(seed)
    circuit = make_circuit(pkg, random_circuit(rng, [k, k]), 1 << k)
    evaluation = circuit.evaluate(F, [F.from_int(rng.randrange(F.p)) for _ in range(1 << k)])
    r_i = [F.from_int(rng.randrange(F.p)) for _ in range(k)]
    return circuit, evaluation, r_i


def gkr_dense_prove(pkg, ctx, k):
    gp = pkg.gkr_protocol
    circuit, evaluation, r_i = gkr_layer(pkg, ctx, k)
    w = gp.start_round_w(ctx, circuit, evaluation, 0, r_i)   # sc_gkr_wiring at k_i = k_next = k
    c1, evals, ch = gp.prove_w(ctx, w, pyref.SEED_R)
    assert ctx.field.add(int(evals[0][0]), int(evals[0][1])) == c1
    return w, c1, evals, ch


@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_gkr_w(p):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    gp = pkg.gkr_protocol
    k = 5

    def workload():
        w, c1, evals, ch = gkr_dense_prove(pkg, ctx, k)
        # the round-by-round dense prover and the sparse one give the same transcript
        circuit, evaluation, r_i = gkr_layer(pkg, ctx, k)
        for pr in (w.native_prover(), gp.SparseLayerProver(ctx, circuit, evaluation, 0, r_i)):
            assert pr.c1() == c1
            for j in range(2 * k):
                assert pr.round_evals(ctx.field.one if j == 0 else int(ch[j - 1]), j) == [int(x) for x in evals[j]]
        # the generic trait methods
        point = [int(x) for x in ch]
        assert len(w.to_evaluations()) == 1 << (2 * k)
        assert w.fix_variables(point[:7]).evaluate(point[7:]) == w.evaluate(point)

    balanced(ctx, workload)


# ---- triangle counting ---------------------------------------------------------------------------------------------------

def triangle_prove(pkg, ctx, var_len):
    tc = pkg.triangle_counting
    n = 1 << var_len
    m = random_adj(random.Random(3 + var_len), n)
    g = tc.G.new_adj_matrix(ctx, 2 * var_len, sum(m, []))
    c1, evals, ch = tc.prove(ctx, g, pyref.SEED_R)
    return g, m, c1, evals, ch


@pytest.mark.parametrize("var_len", [3, 6], ids=["plain_square", "matrix_core_square"])
@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_triangle(p, var_len):
    """all 3k rounds (both phase changes), in one call and round by round"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)

    def workload():
        g, m, c1, evals, ch = triangle_prove(pkg, ctx, var_len)
        n = len(m)
        tri = sum(1 for x in range(n) for y in range(x) for z in range(y) if m[x][y] and m[y][z] and m[x][z])
        assert ctx.field.to_int(c1) == 6 * tri % p
        pr = g.native_prover()
        assert pr.c1() == c1
        for j in range(3 * var_len):
            assert pr.round_evals(ctx.field.one if j == 0 else int(ch[j - 1]), j) == [int(x) for x in evals[j]]
        assert g.fix_variables([int(x) for x in ch[:4]]).num_vars() == 3 * var_len - 4   # three tables

    balanced(ctx, workload)


# ---- matmul, batch, circuit, PCS -----------------------------------------------------------------------------------------

def batch_prove(pkg, ctx, n=10, B=3):
    mm, mle = pkg.matrix_multiplication, pkg.DenseMultilinearExtension
    gs = [mm.G(mle.generate(ctx, pyref.SEED_A + i, n), mle.generate(ctx, pyref.SEED_B + i, n)) for i in range(B)]
    out = mm.prove_batch(ctx, gs, [pyref.SEED_R + i for i in range(B)])
    return gs, out


@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_matmul_batch_circuit_pcs(p):
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    F = ctx.field
    mm, gp, rp, mle = pkg.matrix_multiplication, pkg.gkr_protocol, pkg.relaxed_pcs, pkg.DenseMultilinearExtension

    def matmul():
        for n in (1, 5):   # the book's 2 x 2, and the smallest product on the matrix cores (with its block of byte planes)
            A, B = mle.generate(ctx, pyref.SEED_A, 2 * n), mle.generate(ctx, pyref.SEED_B, 2 * n)
            C = mm.matmul(ctx, n, A, B)
            a, b, c = (F.to_ints(t.to_evaluations()) for t in (A, B, C))
            N = 1 << n
            assert c[N + 1] == sum(a[N + z] * b[z * N + 1] for z in range(N)) % p

    def batch():
        gs, out = batch_prove(pkg, ctx)
        for i, g in enumerate(gs):
            c1, ev, ch = mm.prove(ctx, g, pyref.SEED_R + i)
            assert out[i][0] == c1 and np.array_equal(out[i][1], ev)

    def circuit():
        dc = gp.DeviceCircuit(ctx, make_circuit(pkg, BOOK, 4))
        inp = F.from_ints([3, 2, 3, 1])
        assert [F.to_ints(v.to_evaluations()) for v in dc.evaluate(inp)] == [[36, 6], [9, 4, 6, 1]]
        assert F.to_ints(gp.prove_circuit(ctx, dc, inp, seed_r=9)["circuit_outputs"]) == [36, 6]
        dc.close()

    def pcs():   # (commit and open; the grid of these fields has too many points: test_extend_grid)
        table = mle.generate(ctx, pyref.SEED_A, 10)
        tree = rp.merkle_commit(ctx, table)
        for path, leaf in tree.open([0, 1, len(table) - 1]):
            assert path.verify_canonical(tree.root(), leaf)
        tree.close()

    for workload in (matmul, batch, circuit, pcs):
        balanced(ctx, workload)


def test_extend_grid():
    """the grid of a four-variable table over F_5 (625 points), with its scratch block, committed and opened"""
    pkg = load_package()
    ctx = ctx_of(pkg, 5)
    rp = pkg.relaxed_pcs

    def workload():
        grid = rp.extend_grid(ctx, pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A, 4))
        tree = rp.merkle_commit(ctx, grid)
        for path, leaf in tree.open([0, 624]):
            assert path.verify_canonical(tree.root(), leaf)
        tree.close()

    balanced(ctx, workload)


# ---- a multi-device handle -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_multi_device_handle(p):
    """two shards (on a one-GPU box: device 0 twice); the statistic is the sum over the shards"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p), devices=device_list(2))

    def sums():
        t = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A, 10)   # one fresh block of 2^9 words on either shard
        assert len(t) == 1 << 10 and pool(ctx) == (base[0] + 2, base[1] + (1 << 10))

    base = pool(ctx)
    try:
        balanced(ctx, sums)
        for n in (1, 9, 16):   # single-entry shards; the host ends the proof; passes on the shards
            balanced(ctx, lambda: prove_both_forms(pkg, ctx, n))
        balanced(ctx, lambda: gkr_dense_prove(pkg, ctx, 5))
        balanced(ctx, lambda: triangle_prove(pkg, ctx, 6))
    finally:
        ctx.close()


# ---- rejected calls ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_rejected_calls_leave_nothing_behind(p):
    """Rejections reached by arguments alone.  Not among them: prover_finish's "more challenges than variables" - the triangle
    prover calls it once per phase with the phase's own pending challenges plus one, never more than the tables have variables,
    and sc_tri_prover_round refuses rounds out of order before it gets there"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    F = ctx.field
    gp, tc, mle = pkg.gkr_protocol, pkg.triangle_counting, pkg.DenseMultilinearExtension
    n = 6

    def refused(fn):
        with pytest.raises(pkg.SumcheckHipError):
            fn()

    def prover_rounds():
        g = product(pkg, ctx, n)
        pr = g.native_prover()
        refused(lambda: pr.round_evals(F.one, 1))          # out of order
        pr.round_evals(F.one, 0)
        refused(lambda: pr.round_evals(p, 1))              # an unreduced challenge
        for j in range(1, n):
            pr.round_evals(F.one, j)
        refused(lambda: pr.round_evals(F.one, n))          # past the end

    def wrong_sizes():
        odd = mle.generate(ctx, pyref.SEED_A, 5)
        refused(lambda: tc._NativeTriProver(tc.G(odd, odd, odd, 3)))              # 2^5 entries are no 2^3 x 2^3 matrix
        small, big = mle.generate(ctx, pyref.SEED_A, 3), mle.generate(ctx, pyref.SEED_B, 7)
        refused(lambda: gp.W.new(big, big, small, small).native_prover())   # add / mul of 2^7 entries over 3 + 3 variables
        refused(lambda: gp.prove_w(ctx, gp.W.new(big, small, small, small), pyref.SEED_R))

    def malformed_gates():
        k = 3
        circuit, evaluation, r_i = gkr_layer(pkg, ctx, k)
        circuit.layers[0].layer[5].inputs[1] = 1 << k       # reads a value the next layer does not have
        circuit.layers[0]._arrays = None
        refused(lambda: gp.SparseLayerProver(ctx, circuit, evaluation, 0, r_i))
        refused(lambda: gp.wiring(ctx, circuit, 0, r_i))
        types = np.zeros(1 << k, dtype=np.int32)
        types[2] = 2
        ins = np.zeros(1 << k, dtype=np.uint32)
        refused(lambda: gp.DeviceCircuit.from_arrays(ctx, [k, k], [(types, ins, ins)]))

    for workload in (prover_rounds, wrong_sizes, malformed_gates):
        balanced(ctx, workload)
    balanced(ctx, lambda: prove_both_forms(pkg, ctx, 13))   # the context stays usable


# ---- peak parity -------------------------------------------------------------------------------------------------------------

# "stat_pool_peak_words" of each call below on a fresh Goldilocks context, "stat_reset" before each, as measured on the parent
# commit 95d24cd with nothing but the three statistics added to it (profiles/pool_peak.md).  Host bookkeeping: exact.
PARENT_PEAK_WORDS = {
    "prove n=20": 2228224,
    "fix_variables n=16 k=10": 65600,
    "dense GKR k=5": 2321,
    "triangle var_len=6": 9224,
    "batch 3 x n=10": 12712,
}
# the round-per-launch sumchecks at n = 12 with gp_host_log = fr_host_log = 1 (eleven device rounds: the first fold and the steady
# hand-over of folded tables), measured the same way on the parent commit 0356acd with nothing but these entries added to it
PARENT_PEAK_WORDS.update({
    "sc_gp_prove n=12": 13824,
    "sc_frac_prove n=12": 26112,
    "sc_zerocheck_prove n=12": 26624,
    "sc_sumprod_prove T=2 n=12": 30720,
    "sc_sumprod_prove_ext T=2 n=12": 43008,
    "sc_gp_prove_ext n=12": 22528,
    "sc_product3_prove n=12": 21504,
})


def with_host_logs_1(ctx, call):
    """call() with the layered and the flat sumchecks handing over to the host at two entries"""
    keep = {k: ctx.get_option(k) for k in ("gp_host_log", "fr_host_log")}
    for k in keep:
        ctx.set_option(k, 1)
    try:
        call()
    finally:
        for k, v in keep.items():
            ctx.set_option(k, v)


def round_per_launch_calls(pkg, ctx, n=12):
    F = ctx.field
    w = F.from_int(pkg.ext_field.nonresidue(F.p))
    tau = [int(x) for x in challenges(oracle(GOLD), n)]

    def tables(count):
        return [pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A + i, n) for i in range(count)]
    calls = [
        ("sc_gp_prove", lambda: pkg.grand_product.prove(pkg.grand_product.ProductTree(ctx, *tables(1)), seed_r=pyref.SEED_R)),
        ("sc_frac_prove", lambda: pkg.logup.prove(pkg.logup.FractionTree(ctx, *tables(2)), seed_r=pyref.SEED_R)),
        ("sc_zerocheck_prove", lambda: pkg.r1cs.zerocheck_prove(ctx, *tables(3), tau, seed_r=pyref.SEED_R)),
        ("sc_sumprod_prove T=2", lambda: pkg.multiopen.sumprod_prove(ctx, tables(2), tables(2), seed_r=pyref.SEED_R)),
        ("sc_sumprod_prove_ext T=2", lambda: pkg.ext_sumcheck.sumprod_prove_ext(ctx, w, tables(2), tables(2), seed_r=pyref.SEED_R)),
        ("sc_gp_prove_ext", lambda: pkg.ext_grand_product.prove_ext(
            pkg.ext_grand_product.ExtProductTree(ctx, w, *tables(1), (F.one, F.one), (3, 5)), seed_r=pyref.SEED_R)),
        ("sc_product3_prove", lambda: pkg.spark.product3_prove(ctx, *tables(3), seed_r=pyref.SEED_R)),
    ]
    return [("%s n=%d" % (name, n), lambda call=call: with_host_logs_1(ctx, call)) for name, call in calls]


def peak_calls(pkg, ctx):
    return [
        ("prove n=20", lambda: pkg.matrix_multiplication.prove(ctx, product(pkg, ctx, 20), pyref.SEED_R)),
        ("fix_variables n=16 k=10", lambda: pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A, 16).fix_variables(
            [int(x) for x in challenges(oracle(GOLD), 10)])),
        ("dense GKR k=5", lambda: gkr_dense_prove(pkg, ctx, 5)),
        ("triangle var_len=6", lambda: triangle_prove(pkg, ctx, 6)),
        ("batch 3 x n=10", lambda: batch_prove(pkg, ctx)),
    ] + round_per_launch_calls(pkg, ctx)


def measure_peaks(pkg):
    ctx = pkg.Context(pkg.Field(GOLD))
    peaks = {}
    for name, call in peak_calls(pkg, ctx):
        gc.collect()
        ctx.set_option("stat_reset", 0)
        call()
        peaks[name] = ctx.get_option("stat_pool_peak_words")
        gc.collect()
    ctx.close()
    return peaks


def test_peak_words_equal_the_parents():
    peaks = measure_peaks(load_package())
    print("stat_pool_peak_words:", peaks)
    assert peaks == PARENT_PEAK_WORDS
