"""Long Reed-Solomon rows and their folds, EVERY word, up to the limit of 2^24 (sc_rs_encode_rows_long, sc_ligero_commit_long,
sc_rs_fold, sc_rs_fold_many; csrc/kernels/ligero_long.hpp and rs_fold.hpp) against the
compiled textbook reference of tests/rs_plain.py, which shares no code with the kernels and is itself pinned to the Python
references by tests/test_rs_plain_cpu.py.  No sampling: each case is np.array_equal over the whole result.

Encoder: every codeword length l = c + rho from 15 to 24 on dense uniform input over Goldilocks - each length has its own split
(a, b), from (8, 7) to (12, 12), read back from the launch log - both blow-ups, several matrix rows, the full-width generic
template with 2-adicity 34 at 21 and 24, BabyBear at 22 and 23, a prime of 2-adicity 20 at its limit, and worst-case raw words at
l = 21; one commitment at a length hashlib can follow.  Folds: 2^14, 2^17, 2^20 and 2^24 words on tables that carry the
difference-and-sum corner classes on the pairs (j, j + M/2).

All data words are RAW Montgomery words on both sides (the operations are linear in them); roots of unity are the reference's
own and the alphas go to it through ligero_ref.canon.  A reference is computed once per (p, r, c, rho, kind)."""
import random

import numpy as np
import pytest

import ligero_ref as ref
import rs_plain
import wide_words as ww
from ligero_common import context_cache
from ligero_fold_limits_cases import fold_alpha_sets, fold_table

pytestmark = pytest.mark.gpu

GOLD, BABYBEAR = ref.GOLD, ref.BABYBEAR
P64S18, P64S34, P32LO = ref.P64S18, ref.P64S34, ref.P32LO
IDS = {GOLD: "gold", BABYBEAR: "babybear", P64S18: "p64s18", P64S34: "p64s34", P32LO: "p32lo"}

ctx_of, _close_contexts = context_cache()
_reference = {}
_fold_tables = {}


def teardown_module(module):
    _reference.clear()
    _fold_tables.clear()
    _close_contexts(module)


def _id(v):
    return IDS.get(v, str(v))


def first_pairs_classes(p, words, log_m, pairs=32):
    """the corner classes on the first `pairs` pairs (j, j + M/2) of a row of 2^log_m words: where half_stride_table puts the
    pairs of wide_words.diff_classes"""
    h = 1 << (log_m - 1)
    return ww.half_stride_classes(p, np.concatenate([words[:pairs], words[h:h + pairs]]), pairs.bit_length())


def reference(p, r, c, rho, kind="random"):
    """(the table's raw words, E of the plain reference as raw words, flat) of the shape's test table, computed once.  "random":
    uniform residues; the others are worst-case RAW words: every word p - 1, 0 / p - 1 alternating, the edge words of
    tests/wide_words.py, and its table of corner-class pairs at the stride of the first level"""
    key = (p, r, c, rho, kind)
    if key not in _reference:
        size = 1 << (r + c)
        rng = np.random.default_rng([p % 1000, r, c, rho])
        words = {"random": lambda: rng.integers(0, p, size=size, dtype=np.uint64),
                 "p-1": lambda: np.full(size, p - 1, dtype=np.uint64),
                 "0/p-1": lambda: np.array([0, p - 1] * (size // 2), dtype=np.uint64),
                 "edge": lambda: ww.edge_table(p, size, rng, share=1.0),
                 "half_stride": lambda: ww.half_stride_table(p, 1 << r, c, rng)}[kind]()
        assert words.dtype == np.uint64 and words.size == size and int(words.max()) < p
        if kind == "half_stride":
            assert first_pairs_classes(p, words, c) == ww.classes_present(p)
        _reference[key] = (words, rs_plain.encode(p, words, c, rho))
    return _reference[key]


def logged(ctx, fn):
    """(fn's result, the launch records of fn)"""
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    try:
        ctx.launch_log()
        out = fn()
        return out, ctx.launch_log()
    finally:
        ctx.set_option("time_kernels", 0)


def encode_long_equals(pkg, p, log_len, rho, r, kind="random"):
    ctx = ctx_of(pkg, p)
    c = log_len - rho
    n = r + c
    words, want = reference(p, r, c, rho, kind)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, words)
    got, log = logged(ctx, lambda: pkg.ligero_pcs.rs_encode_rows_long(ctx, t, c, rho).to_evaluations())
    # the two launches of the four-step transform, and the split they ran with
    assert [(x["kind"], x["kf"]) for x in log] == [("rs_long", 0), ("rs_long", 1)], log
    a, b = log[0]["ks"], log[1]["ks"]
    assert a + b == log_len and a == (log_len + 1) // 2, (log_len, a, b)
    assert got.size == want.size == 1 << (n + rho)
    assert np.array_equal(got, want), (p, log_len, rho, r, kind, int(np.flatnonzero(got != want)[0]))


# ---- 1. the encoder, every word ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_len", range(15, 25))
def test_goldilocks_every_length(pkg, log_len):
    """(a, b) = (8, 7), (8, 8), (9, 8), (9, 9), (10, 9), (10, 10), (11, 10), (11, 11), (12, 11), (12, 12)"""
    encode_long_equals(pkg, GOLD, log_len, 1, 0)


@pytest.mark.parametrize("log_len,rho,r", [(21, 2, 1), (23, 2, 0), (20, 1, 2)])
def test_goldilocks_blowup_4_and_several_rows(pkg, log_len, rho, r):
    """rho = 2: a - 2 levels of step 0's own and a four-fold duplication; r = 2: the blocks past the first row's"""
    encode_long_equals(pkg, GOLD, log_len, rho, r)


@pytest.mark.parametrize("p,log_len,rho", [(P64S34, 21, 1), (P64S34, 24, 1), (BABYBEAR, 22, 1), (BABYBEAR, 23, 2), (P32LO, 20, 1)], ids=_id)
def test_generic_fields(pkg, p, log_len, rho):
    """the full-width generic template (2-adicity 34) at 2^21 and at the limit, BabyBear, and 0xfff00001 at l = 20 = its 2-adicity"""
    encode_long_equals(pkg, p, log_len, rho, 0)


@pytest.mark.parametrize("kind", ["p-1", "0/p-1", "edge", "half_stride"])
@pytest.mark.parametrize("p", [GOLD, P64S34], ids=_id)
def test_worst_case_words(pkg, p, kind):
    encode_long_equals(pkg, p, 21, 1, 0, kind)


def test_commitment_equals_hashlib_over_the_plain_encoding(pkg):
    """Goldilocks, (l, rho, r) = (18, 1, 1): the root and eight openings against hashlib over the columns of the plain matrix"""
    p, log_len, rho, r = GOLD, 18, 1, 1
    c, L = log_len - rho, 1 << log_len
    ctx = ctx_of(pkg, p)
    words, want = reference(p, r, c, rho)
    E = [ref.canon(p, row) for row in want.reshape(1 << r, L)]
    levels = ref.tree_levels([ref.column_leaf(E, j) for j in range(L)])
    prover = pkg.ligero_pcs.Prover.commit_long(ctx, pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, words), c, rho)
    assert (prover.log_rows, prover.log_cols, prover.log_blowup, prover.code) == (r, c, rho, "rs")
    root = prover.root()
    assert root == levels[-1][0]
    rng = random.Random(18)
    cols = [0, L - 1, L // 2, (1 << 9) - 1] + [rng.randrange(L) for _ in range(4)]
    for (j, vals, path), col in zip(prover.open_columns(cols), cols):
        assert j == col and vals == [int(x) for x in want.reshape(1 << r, L)[:, col]], col
        assert path.siblings == ref.path_of(levels, col) and path.verify_column(root, vals), col
    prover.close()


# ---- 2. the folds, every word -----------------------------------------------------------------------------------------

def fold_input(pkg, p, log_m):
    """(the context, the raw words of tests/ligero_fold_limits_cases.fold_table, the device table)"""
    if (p, log_m) not in _fold_tables:
        words = fold_table(p, log_m)
        assert first_pairs_classes(p, words, log_m) == ww.classes_present(p)
        _fold_tables[(p, log_m)] = words
    ctx, words = ctx_of(pkg, p), _fold_tables[(p, log_m)]
    return ctx, words, pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, log_m, words)


def fold_equals(pkg, ctx, p, words, t, alpha):
    got = pkg.ligero_pcs.rs_fold(ctx, t, alpha).to_evaluations()
    want = rs_plain.fold(p, words, ref.canon(p, [alpha])[0])
    assert got.size == words.size // 2
    assert np.array_equal(got, want), ("rs_fold", p, alpha, int(np.flatnonzero(got != want)[0]))


def fold_many_equals(pkg, ctx, p, words, t, alphas):
    got = pkg.ligero_pcs.rs_fold_many(ctx, t, alphas).to_evaluations()
    want = rs_plain.fold_many(p, words, ref.canon(p, alphas))
    assert got.size == words.size >> len(alphas)
    assert np.array_equal(got, want), ("rs_fold_many", p, alphas, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("log_m", [14, 17])
@pytest.mark.parametrize("p", [GOLD, P64S34, BABYBEAR, P64S18], ids=_id)
def test_folds_of_2_14_and_2_17_words(pkg, p, log_m):
    """sc_rs_fold over the degenerate challenges and a uniform one, sc_rs_fold_many over the three sets of every count"""
    ctx, words, t = fold_input(pkg, p, log_m)
    for alpha in ww.degenerate_challenges(p, 6) + [random.Random(p + log_m).randrange(p)]:
        fold_equals(pkg, ctx, p, words, t, alpha)
    for count in (1, 2, 3):
        for alphas in fold_alpha_sets(p, log_m, count):
            fold_many_equals(pkg, ctx, p, words, t, alphas)


LONG_FOLDS = [(GOLD, 20), (P64S34, 20), (BABYBEAR, 20), (GOLD, 24), (P64S34, 24)]


@pytest.mark.parametrize("p,log_m", LONG_FOLDS, ids=_id)
def test_fold_of_2_20_and_2_24_words(pkg, p, log_m):
    """sc_rs_fold with the raw alpha p - 1 and a uniform one: at 2^24 words 1 / x = w^(L - j) for every j up to 2^23"""
    ctx, words, t = fold_input(pkg, p, log_m)
    for alpha in (p - 1, random.Random(p + log_m).randrange(p)):
        fold_equals(pkg, ctx, p, words, t, alpha)


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("p,log_m", LONG_FOLDS, ids=_id)
def test_fold_many_of_2_20_and_2_24_words(pkg, p, log_m, count):
    ctx, words, t = fold_input(pkg, p, log_m)
    fold_many_equals(pkg, ctx, p, words, t, fold_alpha_sets(p, log_m, count)[2])
