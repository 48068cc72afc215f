"""The folded and the staged folded opening (csrc/kernels/rs_fold.hpp, csrc/engine/abi_fold.inc; DESIGN.md section 9 items 13 and
14) at their limits, bit for bit against tests/ligero_fold_ref.py and tests/ligero_fold_staged_ref.py:

  a. whole transcripts over seven fields - Goldilocks, BabyBear and the five full-width generic primes - on tables that put
     every add / sub corner class on the pairs (U[j], U[j + M/2]), with edge-word points and gammas, beta = p - 1 and 0 and
     degenerate challenges, under four schedules that between them launch all twelve rs_fold_kernel<F, A, AN>, at layer-0
     lengths on both sides of the fold's table switch with a shift, and the binary opening on two of the shapes;
  b. which instantiations ran, read from the launch log;
  c. the whole protocol with the host FoldVerifier on those tables;
  d. sc_rs_fold and sc_rs_fold_many alone against the reference (not against each other);
  e. query batches that take several gather launches with a short last one, and a column opening above the grid cap;
  f. the pool's books after all of (e).

A reference commitment is built once per (field, shape, kind of inputs) and shared by the tests that need it.
tests/test_ligero_fold_limits_cpu.py checks without a GPU that the inputs cover what is said here."""
import gc
import random

import numpy as np
import pytest

import ligero_fold_ref as fref
import ligero_fold_staged_ref as sref
import ligero_ref as ref
import wide_words
from ligero_common import context_cache, mont_np
from ligero_fold_limits_cases import (ALL_PAIRS, BINARY_SHAPES, FIELDS, FOLD_LOGS, GOLD, P64S18, RANDOM_SHAPE, SHAPES, VERIFIER_SHAPES,
                                      edge_inputs, fid, fold_alpha_sets, fold_table, launched_pairs, queries_of, random_inputs)

pytestmark = pytest.mark.gpu

ctx_of, _close_contexts = context_cache()
_refs = {}
LONG_QUERIES = 2500                 # sc_ligero_fold_query gathers 1024 queries per launch: 1024, 1024 and 452
QUERY_CHUNK = 1024
PLAIN = (15, 3, 1)                  # R = 2^12 rows: sc_ligero_open_columns gathers 2^22 / R = 1024 columns per launch; L = 16
PLAIN_OPENINGS = 1100               # 1024 and 76


def teardown_module(module):
    _refs.clear()
    _close_contexts(module)


def _sid(shape):
    return fid(shape[3])


def inputs_and_commitment(p, shape, kind="edge"):
    """(the raw inputs, the canonical table, the shared ligero_ref.RefProver over it)"""
    key = (p, shape, kind)
    if key not in _refs:
        x = (edge_inputs if kind == "edge" else random_inputs)(p, *shape)
        table = ref.canon(p, x["table"])
        _refs[key] = (x, table, ref.RefProver(table, shape[1], shape[2], p))
    return _refs[key]


def device_prover(pkg, p, shape, words):
    """the commitment to the RAW words, uploaded as they are"""
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx_of(pkg, p), shape[0], np.ascontiguousarray(words, dtype=np.uint64))
    return pkg.ligero_pcs.Prover.commit_long(ctx_of(pkg, p), poly, shape[1], shape[2])


def reference_prover(p, shape, table, commitment, staged):
    n, c, rho, arities = shape
    if staged:
        return sref.RefStagedProver(table, c, rho, p, arities, commitment=commitment)
    want = fref.RefFoldProver(table, c, rho, p)
    assert want.root() == commitment.root()
    return want


def as_staged(answers, staged):
    """the answers of a binary opening, (q, lo, hi, layers), in the staged form (q, [lo, hi], layers)"""
    return list(answers) if staged else [(q, [lo, hi], layers) for q, lo, hi, layers in answers]


def assert_answers_equal(p, got, want, parts):
    """every query's columns with their paths and every stage's words and siblings, in order"""
    assert len(got) == len(want)
    mont_of = {}                                    # (the canonical words of the few distinct columns and leaves, converted once)

    def mont(words):
        words = tuple(words)
        if words not in mont_of:
            mont_of[words] = ref.mont(p, words)
        return mont_of[words]

    for k, ((q, cols, stages), (wq, w_cols, w_stages)) in enumerate(zip(got, want)):
        assert q == wq and len(cols) == len(w_cols) == parts and len(stages) == len(w_stages), k
        for (j, vals, path), (wj, w_vals, w_sib) in zip(cols, w_cols):
            assert j == wj and list(vals) == mont(w_vals) and path.siblings == w_sib, (k, q, j)
        for s, ((words, sib), (w_words, w_sib)) in enumerate(zip(stages, w_stages)):
            assert list(words) == mont(w_words) and sib == w_sib, (k, q, s)


def transcript_equals(pkg, p, shape, kind, staged):
    """every message of one opening, device against reference, under the fixed challenges of the inputs"""
    n, c, rho, arities = shape
    x, table, commitment = inputs_and_commitment(p, shape, kind)
    want = reference_prover(p, shape, table, commitment, staged)
    schedule = arities if staged else (1,) * c
    prover = device_prover(pkg, p, shape, x["table"])
    assert prover.root() == want.root()
    opening = prover.fold_begin(x["point"], x["gamma"], arities if staged else None)
    assert list(opening.claims) == ref.mont(p, want.begin(ref.canon(p, x["point"]), ref.canon(p, x["gamma"])))
    seen = []
    rounds, roots, challenges, final = opening.prove(x["beta"], lambda i, e, root: seen.append((i, e, root)) or x["alphas"][i])
    alphas = ref.canon(p, x["alphas"])
    w_rounds, w_roots, _, w_final = want.prove(ref.canon(p, [x["beta"]])[0], lambda i, e, root: alphas[i])
    assert len(rounds) == c and rounds == [ref.mont(p, e) for e in w_rounds]                  # all 3c sums
    assert roots == w_roots and len(roots) == len(schedule) - 1
    assert challenges == x["alphas"] and final == ref.mont(p, [w_final])[0]
    starts = sref.starts(schedule)
    assert seen == [(i, rounds[i], roots[starts.index(i) - 1] if i and i in starts else None) for i in range(c)]
    queries = queries_of(c, rho, arities if staged else None, n * 100 + c)
    assert_answers_equal(p, as_staged(opening.query(queries), staged), as_staged(want.query(queries), staged), 1 << schedule[0])
    opening.close()
    prover.close()


# ---- a. transcripts on worst-case words ------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_staged_transcript_on_worst_case_words(pkg, p, shape):
    transcript_equals(pkg, p, shape, "edge", True)


@pytest.mark.parametrize("shape", BINARY_SHAPES, ids=_sid)
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_binary_transcript_on_worst_case_words(pkg, p, shape):
    transcript_equals(pkg, p, shape, "edge", False)


@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_staged_transcript_on_uniform_words(pkg, p):
    transcript_equals(pkg, p, RANDOM_SHAPE, "random", True)


# ---- b. which instantiations ran -------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64S18], ids=fid)
def test_every_instantiation_is_launched(pkg, p):
    """the (A, AN) of every rs_fold_many record, taken from the record itself: kf is A, and bytes_written = (8M >> A) + 32 (M >> (A +
    AN)) gives AN (no second term: AN = 0).  Over the four shapes that is all twelve pairs, on each field template"""
    ctx = ctx_of(pkg, p)
    ran = set()
    for shape in SHAPES:
        n, c, rho, arities = shape
        x = random_inputs(p, *shape)
        prover = device_prover(pkg, p, shape, x["table"])
        opening = prover.fold_begin(x["point"], x["gamma"], arities)
        ctx.set_option("time_kernels", 1)
        ctx.launch_log()
        opening.prove(x["beta"], lambda i, e, root: x["alphas"][i])
        log = ctx.launch_log()
        ctx.set_option("time_kernels", 0)
        folds = [r for r in log if r["kind"] == "rs_fold_many"]
        assert len(folds) == len(arities) and not [r for r in log if r["kind"] == "rs_fold"]
        for i, r, (a, an) in zip(sref.starts(arities), folds, launched_pairs(arities)):
            log_m = c + rho - i
            M = 1 << log_m
            assert (r["ks"], r["log_in"], r["bytes_read"]) == (log_m, n, 8 * M), (shape, i, r)
            digests = r["bytes_written"] - (8 * M >> r["kf"])
            assert digests >= 0 and digests % 32 == 0
            leaves = digests // 32
            assert leaves == 0 or (leaves & (leaves - 1) == 0 and leaves << r["kf"] < M)
            pair = (r["kf"], log_m - r["kf"] - (leaves.bit_length() - 1) if leaves else 0)
            assert pair == (a, an), (shape, i, r)
            ran.add(pair)
        opening.close()
        prover.close()
    assert ran == ALL_PAIRS


# ---- c. the verifier -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", VERIFIER_SHAPES, ids=_sid)
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_open_folded_on_worst_case_words_is_accepted_with_the_value(pkg, p, shape):
    lp = pkg.ligero_pcs
    n, c, rho, arities = shape
    x, table, _ = inputs_and_commitment(p, shape)
    prover = device_prover(pkg, p, shape, x["table"])
    v = lp.FoldVerifier(pkg.Field(p), n, c, rho, prover.root(), 12, arities=arities)
    value = lp.open_folded(prover, v, x["point"], random.Random(n + c))
    assert value == prover.poly.evaluate(x["point"])
    assert value == ref.mont(p, [ref.mle_eval(table, ref.canon(p, x["point"]), p)])[0]
    assert len(v.roots) == len(arities) - 1 and len(v.indices) == 12
    prover.close()


# ---- d. the fold kernels against the reference -----------------------------------------------------------------------

@pytest.mark.parametrize("log_m", FOLD_LOGS)
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_folds_of_worst_case_words_equal_the_reference(pkg, p, log_m):
    """sc_rs_fold against ligero_fold_ref.fold and sc_rs_fold_many with 1, 2 and 3 alphas against fold_many, of the canonical
    values of raw words that carry every corner class that exists for p on the pairs (j, j + M/2)"""
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, p)
    words = fold_table(p, log_m)
    if 1 << (log_m - 1) >= len(wide_words.diff_classes(p)):
        assert wide_words.half_stride_classes(p, words, log_m) == wide_words.classes_present(p)
    U = ref.canon(p, words)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, log_m, words)
    for alpha in wide_words.degenerate_challenges(p, 6) + [random.Random(p + log_m).randrange(p)]:
        got = lp.rs_fold(ctx, t, alpha).to_evaluations()
        want = mont_np(p, fref.fold(U, ref.canon(p, [alpha])[0], p))
        assert got.size == len(U) // 2
        assert np.array_equal(got, want), ("rs_fold", alpha, int(np.flatnonzero(got != want)[0]))
    for count in (1, 2, 3):
        for alphas in fold_alpha_sets(p, log_m, count):
            got = lp.rs_fold_many(ctx, t, alphas).to_evaluations()
            want = mont_np(p, sref.fold_many(U, ref.canon(p, alphas), p))
            assert got.size == len(U) >> count
            assert np.array_equal(got, want), ("rs_fold_many", alphas, int(np.flatnonzero(got != want)[0]))


# ---- e. queries that take several launches ---------------------------------------------------------------------------

def long_query_list(shape, staged):
    top = 1 << (shape[1] + shape[2] - (shape[3][0] if staged else 1))
    rng = random.Random(LONG_QUERIES)
    return [0, top - 1, 0, top - 1] + [rng.randrange(top) for _ in range(LONG_QUERIES - 4)]


def column_cap():
    """8 blocks per CU: the most blocks a column_open_kernel launch gets"""
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "binary"])
@pytest.mark.parametrize("p", [GOLD, P64S18], ids=fid)
def test_a_fold_query_batch_of_several_launches(pkg, p, staged):
    """2500 queries in one call: per stage after the first the gather runs three times, the last one short, and the column
    opening's one launch has more columns than blocks (the kernel's grid-stride loop runs)"""
    shape = SHAPES[0]
    n, c, rho, arities = shape
    schedule = arities if staged else (1,) * c
    columns = LONG_QUERIES << schedule[0]
    if columns <= column_cap():
        pytest.skip("%d columns fit the %d blocks of one launch on this device: the grid-stride loop would not run" % (columns, column_cap()))
    assert LONG_QUERIES > 2 * QUERY_CHUNK and LONG_QUERIES % QUERY_CHUNK
    ctx = ctx_of(pkg, p)
    x, table, commitment = inputs_and_commitment(p, shape)
    want = reference_prover(p, shape, table, commitment, staged)
    prover = device_prover(pkg, p, shape, x["table"])
    opening = prover.fold_begin(x["point"], x["gamma"], arities if staged else None)
    alphas = ref.canon(p, x["alphas"])
    want.begin(ref.canon(p, x["point"]), ref.canon(p, x["gamma"]))
    final = opening.prove(x["beta"], lambda i, e, root: x["alphas"][i])[3]
    assert final == ref.mont(p, [want.prove(ref.canon(p, [x["beta"]])[0], lambda i, e, root: alphas[i])[3]])[0]
    queries = long_query_list(shape, staged)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    got = opening.query(queries)
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert_answers_equal(p, as_staged(got, staged), as_staged(want.query(queries), staged), 1 << schedule[0])
    # the gathers: chunk by chunk, inside a chunk stage by stage; then the column opening, one launch
    layers = len(schedule) - 1
    chunks = [QUERY_CHUNK, QUERY_CHUNK, LONG_QUERIES - 2 * QUERY_CHUNK]
    gathers = [r for r in log if r["kind"] == "ligero" and r["kf"] == 2]
    assert [r["ks"] for r in gathers] == [k for k in chunks for _ in range(layers)] + [columns]
    starts = sref.starts(schedule)
    for k, r in enumerate(gathers[:-1]):
        s = 1 + k % layers
        moved = chunks[k // layers] * (8 * (1 << schedule[s]) + 32 * (c + rho - starts[s] - schedule[s]))
        assert (r["log_in"], r["bytes_read"], r["bytes_written"]) == (n, moved, moved), (k, r)
    moved = columns * (8 * (1 << (n - c)) + 32 * (c + rho))
    assert (gathers[-1]["bytes_read"], gathers[-1]["bytes_written"]) == (moved, moved)
    opening.close()
    prover.close()


def plain_table(p):
    return np.random.default_rng(PLAIN[0]).integers(0, p, size=1 << PLAIN[0], dtype=np.uint64)


def plain_indices():
    rng = random.Random(PLAIN_OPENINGS)
    L = 1 << (PLAIN[1] + PLAIN[2])
    return [0, L - 1] + [rng.randrange(L) for _ in range(PLAIN_OPENINGS - 2)]


def test_a_plain_opening_of_several_launches(pkg):
    """(n, c, rho) = (15, 3, 1): columns of 2^12 words, so 1100 openings are a launch of 1024 and one of 76"""
    p = GOLD
    n, c, rho = PLAIN
    R, L = 1 << (n - c), 1 << (c + rho)
    ctx = ctx_of(pkg, p)
    words = plain_table(p)
    want = ref.RefProver(ref.canon(p, words), c, rho, p)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, words)
    prover = pkg.ligero_pcs.Prover.commit(ctx, poly, c, rho)
    assert prover.root() == want.root()
    indices = plain_indices()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    got = prover.open_columns(indices)
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    gathers = [r for r in log if r["kind"] == "ligero" and r["kf"] == 2]
    per_launch = (1 << 22) // R
    assert per_launch == 1024 and [r["ks"] for r in gathers] == [per_launch, PLAIN_OPENINGS - per_launch]
    assert [r["bytes_written"] for r in gathers] == [k * (8 * R + 32 * (c + rho)) for k in (per_launch, PLAIN_OPENINGS - per_launch)]
    columns = [(j, ref.mont(p, vals), sib) for j, vals, sib in want.open_columns(range(L))]      # the 16 distinct columns, once
    assert len(got) == PLAIN_OPENINGS
    for k, ((j, vals, path), index) in enumerate(zip(got, indices)):
        assert j == index and (j, vals, path.siblings) == columns[index], (k, index)
    prover.close()


# ---- f. the pool's books ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P64S18], ids=fid)
def test_pool_balance_after_the_long_queries(pkg, p):
    """the device work of all of (e), twice: after the second pass the pool's books are where the first one left them"""
    ctx = ctx_of(pkg, p)
    shape = SHAPES[0]
    x = edge_inputs(p, *shape)

    def workload():
        for staged in (True, False):
            prover = device_prover(pkg, p, shape, x["table"])
            opening = prover.fold_begin(x["point"], x["gamma"], shape[3] if staged else None)
            opening.prove(x["beta"], lambda i, e, root: x["alphas"][i])
            assert len(opening.query(long_query_list(shape, staged))) == LONG_QUERIES
            opening.close()
            prover.close()
        if p == GOLD:
            poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, PLAIN[0], plain_table(p))
            prover = pkg.ligero_pcs.Prover.commit(ctx, poly, PLAIN[1], PLAIN[2])
            assert len(prover.open_columns(plain_indices())) == PLAIN_OPENINGS
            prover.close()
            del poly

    workload()                              # (the tables of these lengths are workspace of the context, made here)
    gc.collect()
    books = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")
    workload()
    gc.collect()
    assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == books
