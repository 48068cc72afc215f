"""Expander-code rows longer than the LDS of a CU (sc_xc_encode_rows_long, sc_ligero_commit_code_long;
csrc/kernels/expander_long.hpp).  Every comparison is equality of words or digests: the encoding
against tests/expander_ref.py bit for bit where Python can encode a row (c = 14, 15, 16), on four fields and on worst-case
words; longer rows - up to the limit c = 23 - against check_levels of tests/expander_long_ref.py, which checks sampled outputs
of every level from the downloaded codeword alone; roots against hashlib, openings and row combinations; the whole protocol
with the unchanged Verifier(code="expander"); the dispatch below c = 14; the refusals, the launch log and the pool's books.

Shapes: c = 14 and 15 have one global level and the two inner codes there are (12, 13); c = 16 has two global levels, 18 three,
23 five.  The Python reference is the slow part (seconds for the gather lists of a level, then cached), so a reference
encoding is computed once per (field, shape, table) and shared."""
import ctypes
import gc
import random

import numpy as np
import pytest

import expander_long_ref as xl_ref
import expander_ref as ref
import ligero_ref
import test_gpu_expander as base
import wide_words
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD, P59, BABYBEAR = base.GOLD, base.P59, base.BABYBEAR
IDS = base.IDS


def _id(v):
    return IDS.get(v, str(v))


def teardown_module(module):
    base.teardown_module(module)        # the contexts base.ctx_of made for this file
    _reference.clear()
    _commits.clear()


_reference = {}


def reference(p, r, c, kind="random"):
    """(the table's Montgomery words, E as Montgomery words, flat, the canonical table, E's rows in canonical integers) of the
    shape's test table, computed once and left unchanged.  "random": uniform residues; the other kinds are RAW words, as the
    kernels meet them: every word p - 1, 0 / p - 1 alternating, the octets of tests/wide_words.py"""
    key = (p, r, c, kind)
    if key not in _reference:
        size = 1 << (r + c)
        if kind == "random":
            rng = random.Random("%d %d %d" % (p, r, c))
            table = [rng.randrange(p) for _ in range(size)]
            words = base.mont_np(p, table)
        else:
            words = {"p-1": lambda: np.full(size, p - 1, dtype=np.uint64),
                     "0/p-1": lambda: np.array([0, p - 1] * (size // 2), dtype=np.uint64),
                     "octet": lambda: wide_words.octet_table(p, size, np.random.default_rng(c), share=1.0)}[kind]()
            assert words.dtype == np.uint64 and words.size == size and int(words.max()) < p
            if kind == "octet":
                assert wide_words.stride_classes(p, words, 1) >= wide_words.classes_present(p)
            table = base.canon_of(p, words)
        E = ref.encode_rows(table, c, p)
        _reference[key] = (words, base.mont_np(p, base.flat(E)), table, E)
    return _reference[key]


def encode_long_equals(pkg, p, r, c, kind="random"):
    ctx = base.ctx_of(pkg, p)
    words, want, _, _ = reference(p, r, c, kind)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, words)
    got = pkg.ligero_pcs.xc_encode_rows_long(ctx, t, c).to_evaluations()
    assert got.size == 2 << (r + c)
    assert np.array_equal(got, want), (p, r, c, kind, int(np.flatnonzero(got != want)[0]))


# ---- 1. the encoding, bit for bit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("c", [14, 15])
@pytest.mark.parametrize("p", base.FIELDS, ids=_id)
def test_encode_equals_the_reference(pkg, p, c, r):
    """one global level; inner codes of 2^12 and 2^13 words; the second row one stride further"""
    encode_long_equals(pkg, p, r, c)


def test_encode_with_two_global_levels(pkg):
    encode_long_equals(pkg, P59, 1, 16)


# ---- 2. worst-case words ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["p-1", "0/p-1", "octet"])
@pytest.mark.parametrize("p", [P59, GOLD], ids=_id)
def test_encode_worst_case_words(pkg, p, kind):
    encode_long_equals(pkg, p, 1, 14, kind)


# ---- 3. rows Python cannot encode: every level from the codeword alone -----------------------------------------------

@pytest.mark.parametrize("p,n,c,rows", [(GOLD, 19, 18, (0, 1)), (BABYBEAR, 21, 20, (1,)), (P59, 24, 23, (0, 1))], ids=_id)
def test_levels_of_long_rows(pkg, p, n, c, rows):
    """three, four and five global levels; (24, 23) is the limit: L = 2^24, E of 256 MiB.  check_levels takes the Montgomery
    words as they are (the maps are linear)"""
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, p)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 0x10E6 + c, n)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    E = lp.xc_encode_rows_long(ctx, poly, c)
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    global_levels = list(range(c, 13, -2))
    lm_i = global_levels[-1] - 2
    assert [(x["kind"], x["kf"], x["ks"]) for x in log if x["kf"]] == (
        [("xc_long", 1, lm) for lm in global_levels] + [("xc_long", 2, lm_i)] + [("xc_long", 3, lm) for lm in reversed(global_levels)])
    w = poly.to_evaluations()
    got = E.to_evaluations()
    assert got.size == 2 << n and int(got.max()) < p
    for i in rows:
        xl_ref.check_levels(p, w[i << c:(i + 1) << c], got[i << (c + 1):(i + 1) << (c + 1)], c, positions=1000 * c + i)


# ---- 4. roots, openings, combinations --------------------------------------------------------------------------------

_commits = {}


def ref_commit(p, r, c):
    """(the table's words, the canonical table, E's rows, every level of the hashlib tree over E's columns), once per shape"""
    if (p, r, c) not in _commits:
        words, _, table, E = reference(p, r, c)
        _commits[(p, r, c)] = (words, table, E, ref.tree_levels([ref.column_leaf(E, j) for j in range(2 << c)]))
    return _commits[(p, r, c)]


@pytest.mark.parametrize("r,c", [(0, 14), (2, 14), (1, 15)])
@pytest.mark.parametrize("p", [P59, GOLD], ids=_id)
def test_root_openings_and_combinations(pkg, p, r, c):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, p)
    words, table, E, levels = ref_commit(p, r, c)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, words)
    prover = lp.Prover.commit_long(ctx, poly, c, 1, code="expander")
    assert (prover.log_rows, prover.log_cols, prover.log_blowup, prover.code) == (r, c, 1, "expander")
    root = prover.root()
    assert root == levels[-1][0]
    L = 2 << c
    cols = [0, 1, L // 2 - 1, L // 2, L - 1, 77, 77]
    for (j, vals, path), want in zip(prover.open_columns(cols), cols):
        assert j == want and vals == ligero_ref.mont(p, [row[j] for row in E]), j
        assert path.siblings == [levels[l][(j >> l) ^ 1] for l in range(c + 1)], j
        assert path.verify_column(root, vals)
    base.expect(pkg, 1, lambda: prover.open_columns([L]), "not below L")
    rng = random.Random(r + c)
    weights = [[rng.randrange(p) for _ in range(1 << r)] for _ in range(4)]
    want = [ligero_ref.mont(p, ref.combine(table, c, w, p)) for w in weights]
    for M in (1, 2, 4):
        assert prover.combine_rows([ligero_ref.mont(p, w) for w in weights[:M]]) == want[:M], (r, c, M)
    prover.close()


# ---- 5. the whole protocol -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,n,c", [(P59, 15, 14), (GOLD, 16, 15)], ids=_id)
def test_protocol(pkg, p, n, c):
    """the unchanged Verifier(code="expander") and the five tamper cases of test_gpu_expander.run_protocol"""
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, p)
    words, table, _, levels = ref_commit(p, n - c, c)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, words)
    prover = lp.Prover.commit_long(ctx, poly, c, 1, code="expander")
    assert prover.root() == levels[-1][0]
    rng = random.Random(n)
    base.run_protocol(pkg, prover, poly, table, p, n, c, 8, rng)
    for tamper, err in (("u_z", lp.EvalMismatch), ("u_gamma", lp.ProximityMismatch), ("column", lp.MerkleMismatch),
                        ("path", lp.MerkleMismatch), ("root", lp.MerkleMismatch)):
        with pytest.raises(err):
            base.run_protocol(pkg, prover, poly, table, p, n, c, 8, rng, tamper=tamper)
    prover.close()


# ---- 6. dispatch -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c", [(5, 7), (2, 13)])
def test_short_rows_take_the_single_launch(pkg, r, c):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, P59)
    n = r + c
    poly = pkg.DenseMultilinearExtension.generate(ctx, 77 + c, n)
    short = lp.xc_encode_rows(ctx, poly, c).to_evaluations()
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    long_ = lp.xc_encode_rows_long(ctx, poly, c).to_evaluations()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert np.array_equal(long_, short)
    assert [(x["kind"], x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log] == [
        ("xc_encode", c, (c - 4) // 2, n, 8 << n, 8 << (n + 1))]
    a, b = lp.Prover.commit_long(ctx, poly, c, 1, code="expander"), lp.Prover.commit(ctx, poly, c, 1, code="expander")
    assert a.root() == b.root() and (a.log_rows, a.log_cols, a.log_blowup, a.code) == (r, c, 1, "expander")
    a.close()
    b.close()


def test_commit_code_long_rs_is_commit_long(pkg):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, GOLD)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 9, 16)
    plain = lp.Prover.commit_long(ctx, poly, 14, 1)
    h = ctypes.c_void_p()
    ctx.check(ctx.lib.sc_ligero_commit_code_long(ctx.h, poly.h, 14, 1, 0, ctypes.byref(h)))
    coded = lp.Prover(ctx, poly, h)
    assert coded.root() == plain.root() and (coded.log_rows, coded.log_cols, coded.log_blowup, coded.code) == (2, 14, 1, "rs")
    xp = lp.Prover.commit_long(ctx, poly, 14, 1, code="expander")
    assert xp.code == "expander" and xp.root() != plain.root()
    chosen = lp.Prover.commit_long(ctx, poly, queries=64, code="expander")
    assert chosen.log_cols == lp.long_log_cols(16, 1, 64) and chosen.code == "expander"
    for pr in (plain, coded, xp, chosen):
        pr.close()


def test_the_short_entry_points_keep_their_limit(pkg):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, P59)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 5, 15)
    base.expect(pkg, 6, lambda: lp.xc_encode_rows(ctx, poly, 14), "LDS")
    base.expect(pkg, 6, lambda: lp.Prover.commit(ctx, poly, 14, 1, code="expander"), "LDS")
    assert len(lp.xc_encode_rows_long(ctx, poly, 14)) == 2 << 15


# ---- 7. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(pkg):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, P59)
    F = pkg.Field(P59)
    big = pkg.DenseMultilinearExtension.generate(ctx, 5, 24)
    for fn in (lambda: lp.xc_encode_rows_long(ctx, big, 24), lambda: lp.Prover.commit_long(ctx, big, 24, 1, code="expander")):
        base.expect(pkg, 6, fn, "2^24")
    del big
    c5 = pkg.Context(pkg.Field(5))
    t5 = pkg.DenseMultilinearExtension.from_evaluations_vec(c5, 4, pkg.Field(5).from_ints(range(16)))
    for fn in (lambda: lp.xc_encode_rows_long(c5, t5, 2), lambda: lp.Prover.commit_long(c5, t5, 2, 1, code="expander")):
        base.expect(pkg, 6, fn, "p = 5")
    del t5
    c5.close()
    small = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 3, F.from_ints(range(8)))
    base.expect(pkg, 1, lambda: lp.Prover.commit_long(ctx, small, 1, 2, code="expander"), "log_blowup")
    base.expect(pkg, 1, lambda: lp.Prover.commit_long(ctx, small, 1, 0, code="expander"), "log_blowup")
    base.expect(pkg, 1, lambda: lp.xc_encode_rows_long(ctx, small, 4))                               # log_cols > n
    base.expect(pkg, 1, lambda: lp.Prover.commit_long(ctx, small, 4, 1, code="expander"))
    h = ctypes.c_void_p()
    lib = ctx.lib
    assert lib.sc_ligero_commit_code_long(ctx.h, small.h, 1, 1, 2, ctypes.byref(h)) == 1 and not h.value          # unknown code
    assert "code 2" in lib.sc_last_error(ctx.h).decode()
    assert lib.sc_ligero_commit_code_long(ctx.h, small.h, 1, 1, -1, ctypes.byref(h)) == 1 and not h.value
    assert lib.sc_xc_encode_rows_long(ctx.h, None, 1, ctypes.byref(h)) == 1 and not h.value                       # no table
    assert lib.sc_ligero_commit_code_long(ctx.h, None, 1, 1, 1, ctypes.byref(h)) == 1 and not h.value
    assert lib.sc_xc_encode_rows_long(ctx.h, small.h, 1, None) == 1                                               # no out
    assert lib.sc_ligero_commit_code_long(ctx.h, small.h, 1, 1, 1, None) == 1
    with pytest.raises(ValueError):
        lp.Prover.commit_long(ctx, small, 1, 1, code="ldpc")
    assert len(lp.xc_encode_rows_long(ctx, small, 2)) == 16                                                       # the context still works


def test_sharded_and_multi_device_are_refused(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(P59)
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    base.expect(pkg, 6, lambda: lp.xc_encode_rows_long(m, mt, 2), "multi-device")
    base.expect(pkg, 6, lambda: lp.Prover.commit_long(m, mt, 2, 1, code="expander"), "multi-device")
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    base.expect(pkg, 6, lambda: lp.xc_encode_rows_long(sh, st, 2), "sharded")
    base.expect(pkg, 6, lambda: lp.Prover.commit_long(sh, st, 2, 1, code="expander"), "sharded")


# ---- 8. the launch log -----------------------------------------------------------------------------------------------

def test_launch_log(pkg):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, P59)
    n, c = 17, 16
    R = 1 << (n - c)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, n)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    prover = lp.Prover.commit_long(ctx, poly, c, 1, code="expander")
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert {x["kind"] for x in log} == {"xc_long", "ligero", "merkle"}
    xc = [x for x in log if x["kind"] == "xc_long"]
    assert all(x["log_in"] == n for x in xc)
    if xc[0]["kf"] == 0:
        assert (xc[0]["bytes_read"], xc[0]["bytes_written"]) == (8 << n, 8 << n)
        xc = xc[1:]
    assert [(x["kf"], x["ks"]) for x in xc] == [(1, 16), (1, 14), (2, 12), (3, 14), (3, 16)]
    for x in xc:
        lm = x["ks"]
        want = {1: (8 * R << lm, 8 * R << (lm - 2)), 2: (8 * R << lm, 8 * R << lm), 3: (8 * R << (lm - 1), 8 * R << (lm - 1))}[x["kf"]]
        assert (x["bytes_read"], x["bytes_written"]) == want, x
    assert [(x["kf"], x["ks"], x["bytes_read"], x["bytes_written"]) for x in log if x["kind"] == "ligero"] == [(0, n - c, 8 << (n + 1), 32 * (2 << c))]
    prover.close()


# ---- 9. the pool's books ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [P59, GOLD], ids=_id)
def test_pool_balance(pkg, p):
    """after a long commit, a combine, an opening, an encoding, refused calls and the destroy the pool is where it was"""
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, p)
    F = pkg.Field(p)
    n, c = 16, 14
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, n)
    lp.Prover.commit_long(ctx, poly, c, 1, code="expander").close()    # (the table of inverses is workspace of the context, made here)
    gc.collect()
    books = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")

    def workload():
        rng = random.Random(8)
        prover = lp.Prover.commit_long(ctx, poly, c, 1, code="expander")
        prover.combine([F.rand(rng) for _ in range(n)], [F.rand(rng) for _ in range(1 << (n - c))])
        prover.open_columns([1, 2, 3])
        E = lp.xc_encode_rows_long(ctx, poly, c + 1)
        del E
        base.expect(pkg, 1, lambda: prover.open_columns([2 << c]))
        base.expect(pkg, 1, lambda: lp.Prover.commit_long(ctx, poly, c, 2, code="expander"))
        base.expect(pkg, 1, lambda: lp.xc_encode_rows_long(ctx, poly, n + 1))
        base.expect(pkg, 6, lambda: lp.xc_encode_rows(ctx, poly, c), "LDS")
        prover.close()

    workload()
    gc.collect()
    assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == books
    assert len(lp.xc_encode_rows(ctx, poly, 10)) == 2 << n
