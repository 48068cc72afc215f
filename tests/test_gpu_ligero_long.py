"""Reed-Solomon rows longer than the LDS of a CU (sc_rs_encode_rows_long, sc_ligero_commit_long; csrc/kernels/ligero_long.hpp,
DESIGN.md section 9 item 11) against tests/ligero_ref.py: the encoding bit for bit at every split parity and tile shape the small
lengths reach, on both field templates and on worst-case words; the short lengths through today's single launch; the limit
length L = 2^24 on a sparse table against the defining sum; roots against hashlib; the whole protocol with the unchanged
Verifier; the refusals and the pool's books.

Shapes: l = c + rho = 15, 16, 17 (a, b = 8 7, 8 8, 9 8: 64- and 32-word segments, both parities), 18 .. 20 on BabyBear (whose
reference runs in int64; 9 9, 10 9, 10 10), 18 = s on the widest generic prime, 24 = the limit (12 12, 4-word segments).  A
reference encoding is computed once per (field, shape, table) and shared by the tests that need it."""
import ctypes
import gc
import hashlib
import random

import numpy as np
import pytest

import ligero_ref as ref
import test_gpu_ligero as base
import wide_words as ww
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD, BABYBEAR = ref.GOLD, ref.BABYBEAR
P64S18, P64S34 = ref.P64S18, ref.P64S34
IDS = {GOLD: "gold", BABYBEAR: "babybear", P64S18: "p64s18", P64S34: "p64s34", 65537: "p65537"}


def _id(v):
    return IDS.get(v, str(v))


def teardown_module(module):
    base.teardown_module(module)        # the contexts base.ctx_of made for this file
    _reference.clear()


_reference = {}


def reference(p, r, c, rho, kind="random"):
    """(the table's Montgomery words; E as Montgomery words, flat; the canonical table; E's rows in canonical integers) of the
    shape's test table, computed once.  "random": uniform residues; the other kinds are RAW words, as the kernels meet them:
    every word p - 1, 0 / p - 1 alternating, and the edge words of tests/wide_words.py"""
    key = (p, r, c, rho, kind)
    if key not in _reference:
        size = 1 << (r + c)
        if kind == "random":
            rng = random.Random("%d %d %d %d" % (p, r, c, rho))
            table = [rng.randrange(p) for _ in range(size)]
            words = base.mont_np(p, table)
        else:
            words = {"p-1": lambda: np.full(size, p - 1, dtype=np.uint64),
                     "0/p-1": lambda: np.array([0, p - 1] * (size // 2), dtype=np.uint64),
                     "edge": lambda: ww.edge_table(p, size, np.random.default_rng(r + c), share=1.0)}[kind]()
            assert words.dtype == np.uint64 and words.size == size and int(words.max()) < p
            table = ref.canon(p, words)
        E = ref.encode(table, c, rho, p)
        _reference[key] = (words, base.mont_np(p, base.flat(E)), table, E)
    return _reference[key]


def encode_long_equals(pkg, p, r, c, rho, kind="random"):
    ctx = base.ctx_of(pkg, p)
    words, want, _, _ = reference(p, r, c, rho, kind)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, words)
    got = pkg.ligero_pcs.rs_encode_rows_long(ctx, t, c, rho).to_evaluations()
    assert got.size == 1 << (r + c + rho)
    assert np.array_equal(got, want), (p, r, c, rho, kind, int(np.flatnonzero(got != want)[0]))


# ---- 1. the encoding, bit for bit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [0, 1, 3])
@pytest.mark.parametrize("rho", [1, 2])
@pytest.mark.parametrize("log_len", [15, 16, 17])
def test_goldilocks_equals_the_reference(pkg, log_len, rho, r):
    encode_long_equals(pkg, GOLD, r, log_len - rho, rho)


@pytest.mark.parametrize("kind", ["p-1", "0/p-1"])
def test_goldilocks_worst_case_words(pkg, kind):
    encode_long_equals(pkg, GOLD, 1, 14, 1, kind)


@pytest.mark.parametrize("log_len", [18, 19, 20])
def test_babybear_equals_the_reference(pkg, log_len):
    encode_long_equals(pkg, BABYBEAR, 0, log_len - 1, 1)


@pytest.mark.parametrize("log_len,r,kind", [(15, 0, "random"), (15, 1, "random"), (18, 0, "random"), (18, 1, "random"),
                                            (15, 1, "edge"), (15, 0, "p-1"), (15, 1, "0/p-1")])
def test_full_width_generic_field_equals_the_reference(pkg, log_len, r, kind):
    """0xffffffffffe40001, s = 18: l = 15 and l = 18 = s, and at l = 15 the worst-case tables of tests/wide_words.py"""
    encode_long_equals(pkg, P64S18, r, log_len - 1, 1, kind)


def test_a_field_of_two_adicity_above_32(pkg):
    encode_long_equals(pkg, P64S34, 1, 14, 2)


# ---- 2. up to l = 14: today's path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c,rho", [(3, 5, 1), (0, 12, 2), (2, 13, 1)])
def test_short_rows_take_the_single_launch(pkg, r, c, rho):
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, GOLD)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 77 + c, r + c)
    short = lp.rs_encode_rows(ctx, poly, c, rho).to_evaluations()
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    long_ = lp.rs_encode_rows_long(ctx, poly, c, rho).to_evaluations()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert np.array_equal(long_, short)
    assert [x["kind"] for x in log] == ["rs_encode"]
    a, b = lp.Prover.commit_long(ctx, poly, c, rho), lp.Prover.commit(ctx, poly, c, rho)
    assert a.root() == b.root() and (a.log_rows, a.log_cols, a.log_blowup, a.code) == (r, c, rho, "rs")
    a.close()
    b.close()


# ---- 3. the limit length, on sparse input ----------------------------------------------------------------------------

def test_the_limit_length(pkg):
    """Goldilocks, (n, c, rho) = (23, 23, 1): L = 2^24 = 2^12 2^12, one row, E of 128 MiB, the tree 1 GiB"""
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    ctx = base.ctx_of(pkg, GOLD)
    n, c, rho = 23, 23, 1
    C, L = 1 << c, 1 << (c + rho)
    rng = random.Random(24)
    words = np.zeros(C, dtype=np.uint64)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, words)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    lp.rs_encode_rows_long(ctx, poly, c, rho)                  # the split, from the launch log
    log = [x for x in ctx.launch_log() if x["kind"] == "rs_long"]
    assert [(x["kf"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log] == [
        (0, n, 8 << n, 8 << (n + rho)), (1, n, 8 << (n + rho), 8 << (n + rho))]
    a, b = log[0]["ks"], log[1]["ks"]
    assert a + b == c + rho and max(a, b) <= 14
    L1, L2 = 1 << a, 1 << b
    places = sorted({0, 1, L2 - 1, L2, L2 + 1, C - 1} | {rng.randrange(C) for _ in range(3)})
    values = {k: rng.randrange(1, GOLD) for k in places}
    for k, v in values.items():
        words[k] = F.from_int(v)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, words)
    ctx.launch_log()
    E = lp.rs_encode_rows_long(ctx, poly, c, rho).to_evaluations()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert [(x["kind"], x["kf"]) for x in log] == [("rs_long", 0), ("rs_long", 1)]
    assert E.size == L
    w = ref.omega(GOLD, c + rho)
    for j in [0, 1, L1 - 1, L1, L // 2, L - 1] + [rng.randrange(L) for _ in range(2000)]:
        want = sum(v * pow(w, j * k, GOLD) for k, v in values.items()) % GOLD
        assert int(E[j]) == F.from_int(want), j
    prover = lp.Prover.commit_long(ctx, poly, c, rho)
    assert (prover.log_rows, prover.log_cols, prover.log_blowup) == (0, c, rho)
    root = prover.root()
    cols = [0, L - 1, rng.randrange(L)]
    for (j, vals, path), want in zip(prover.open_columns(cols), cols):
        assert j == want and vals == [int(E[j])] and len(path.siblings) == c + rho and path.verify_column(root, vals)
    prover.close()


# ---- 4. the root against hashlib -------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,log_len,rho", [(0, 15, 1), (1, 15, 2), (3, 16, 1)])
def test_root_equals_hashlib_over_the_reference_encoding(pkg, r, log_len, rho):
    ctx = base.ctx_of(pkg, GOLD)
    c = log_len - rho
    words, _, _, E = reference(GOLD, r, c, rho)
    prover = pkg.ligero_pcs.Prover.commit_long(ctx, pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, words), c, rho)
    assert (prover.log_rows, prover.log_cols, prover.log_blowup, prover.code) == (r, c, rho, "rs")
    assert prover.root() == ref.root_of(E)
    prover.close()


def test_a_real_matrix(pkg):
    """Goldilocks, (n, c, rho) = (21, 19, 1): four rows of 2^20 words, a generated table"""
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    ctx = base.ctx_of(pkg, GOLD)
    n, c, rho = 21, 19, 1
    r, C, L = n - c, 1 << c, 1 << (c + rho)
    R = 1 << r
    poly = pkg.DenseMultilinearExtension.generate(ctx, 0x10E6, n)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    prover = lp.Prover.commit_long(ctx, poly, c, rho)
    root = prover.root()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert [(x["kf"], x["bytes_read"], x["bytes_written"]) for x in log if x["kind"] == "rs_long"] == [
        (0, 8 << n, 8 << (n + rho)), (1, 8 << (n + rho), 8 << (n + rho))]
    assert [(x["kf"], x["ks"], x["bytes_read"], x["bytes_written"]) for x in log if x["kind"] == "ligero"] == [(0, r, 8 << (n + rho), 32 * L)]
    merkle = [(x["kf"], x["bytes_read"], x["bytes_written"]) for x in log if x["kind"] == "merkle"]
    assert merkle == [(1, 32 * (L >> k), 32 * (L >> (k + 1))) for k in range(c + rho - 9)] + [(2, 32 * (1024 - 2), 32 * 511)]
    assert {x["kind"] for x in log} == {"rs_long", "ligero", "merkle"}
    E = lp.rs_encode_rows_long(ctx, poly, c, rho).to_evaluations().reshape(R, L)
    rng = random.Random(21)
    table = base.gold_canon_np(poly.to_evaluations()).reshape(R, C)
    assert int(table[R - 1, 5]) == base._splitmix64(0x10E6 + (R - 1) * C + 5) % GOLD
    w = ref.omega(GOLD, c + rho)
    rows = {}
    for _ in range(16):
        i, j = rng.randrange(R), rng.randrange(L)
        row = rows.setdefault(i, [int(x) for x in table[i]])
        assert int(E[i, j]) == F.from_int(ref.direct(row, w, GOLD, j)), (i, j)
    canon = base.gold_canon_np(E)
    assert all(int(canon[i, j]) == F.to_int(int(E[i, j])) for i, j in [(rng.randrange(R), rng.randrange(L)) for _ in range(1000)])
    cols = np.ascontiguousarray(canon.T).astype("<u8")
    leaves = [hashlib.sha256(cols[j].tobytes()).digest() for j in range(L)]
    assert ref.tree_levels(leaves)[-1][0] == root
    prover.close()


# ---- 5. the whole protocol -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,n,c,rho", [(GOLD, 16, 14, 1), (GOLD, 16, 14, 2), (P64S18, 16, 15, 1)], ids=_id)
def test_protocol(pkg, p, n, c, rho):
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    ctx = base.ctx_of(pkg, p)
    rng = random.Random(n + c + rho)
    table = [rng.randrange(p) for _ in range(1 << n)]
    poly = base.upload(pkg, ctx, p, table)
    prover = lp.Prover.commit_long(ctx, poly, c, rho)
    rp = ref.RefProver(table, c, rho, p)
    root = prover.root()
    assert root == rp.root()

    def run(tamper=None):
        v = lp.Verifier(F, n, c, rho, root if tamper != "root" else bytes([root[0] ^ 1]) + root[1:], 6, code="rs")
        gamma = v.draw_gamma(rng)
        point = [F.rand(rng) for _ in range(n)]
        u_gamma, u_z = prover.combine(point, gamma)
        if tamper is None:
            ru_gamma, ru_z = rp.combine(ref.canon(p, point), ref.canon(p, gamma))
            assert u_gamma == ref.mont(p, ru_gamma) and u_z == ref.mont(p, ru_z)
        if tamper == "u_z":
            u_z[len(u_z) // 2] = F.add(u_z[len(u_z) // 2], F.one)
        if tamper == "u_gamma":
            u_gamma[0] = F.add(u_gamma[0], F.one)
        v.receive(u_gamma, u_z)
        columns = v.draw_columns(rng)
        openings = prover.open_columns(columns)
        if tamper is None:
            for (j, vals, path), (rj, rvals, rsib) in zip(openings, rp.open_columns(columns)):
                assert j == rj and vals == ref.mont(p, rvals) and path.siblings == rsib, j
        if tamper == "column":
            j, vals, path = openings[3]
            openings[3] = (j, [F.add(vals[0], F.one)] + vals[1:], path)
        if tamper == "path":
            j, vals, path = openings[5]
            openings[5] = (j, vals, lp.ColumnPath(j, [bytes(32)] + path.siblings[1:], F))
        value = v.verify(point, openings)
        assert value == F.from_int(ref.mle_eval(table, ref.canon(p, point), p))

    run()
    if (p, rho) == (GOLD, 1):
        for tamper, err in (("u_z", lp.EvalMismatch), ("u_gamma", lp.ProximityMismatch), ("column", lp.MerkleMismatch),
                            ("path", lp.MerkleMismatch), ("root", lp.MerkleMismatch)):
            with pytest.raises(err):
                run(tamper)
    prover.close()


# ---- 6. refusals and books -------------------------------------------------------------------------------------------

def test_refusals(pkg):
    lp = pkg.ligero_pcs
    g = base.ctx_of(pkg, GOLD)
    G = pkg.Field(GOLD)
    big = pkg.DenseMultilinearExtension.generate(g, 5, 24)
    for fn in (lambda: lp.rs_encode_rows_long(g, big, 24, 1), lambda: lp.Prover.commit_long(g, big, 23, 2)):
        base.expect(pkg, 6, fn, "2^24")
    del big
    f = base.ctx_of(pkg, 65537)
    t16 = pkg.DenseMultilinearExtension.generate(f, 5, 16)
    for fn in (lambda: lp.rs_encode_rows_long(f, t16, 16, 1), lambda: lp.Prover.commit_long(f, t16, 15, 2)):
        base.expect(pkg, 6, fn, "2-adicity 16", "65537")
    assert lp.Prover.commit_long(f, t16, 15, 1).log_cols == 15               # c + rho = 16 = s is served
    small = pkg.DenseMultilinearExtension.from_evaluations_vec(g, 3, G.from_ints(range(8)))
    for log_cols, rho in ((1, 0), (1, 3), (4, 1)):
        base.expect(pkg, 1, lambda: lp.rs_encode_rows_long(g, small, log_cols, rho))
        base.expect(pkg, 1, lambda: lp.Prover.commit_long(g, small, log_cols, rho))
    h = ctypes.c_void_p()
    assert g.lib.sc_rs_encode_rows_long(g.h, None, 1, 1, ctypes.byref(h)) == 1 and not h.value
    assert g.lib.sc_ligero_commit_long(g.h, None, 1, 1, ctypes.byref(h)) == 1 and not h.value
    assert g.lib.sc_rs_encode_rows_long(g.h, small.h, 1, 1, None) == 1
    assert g.lib.sc_ligero_commit_long(g.h, small.h, 1, 1, None) == 1
    with pytest.raises(ValueError):
        lp.Prover.commit_long(g, small)
    assert len(lp.rs_encode_rows(g, small, 2, 1)) == 16                      # the context still works


def test_sharded_and_multi_device_are_refused(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    base.expect(pkg, 6, lambda: lp.rs_encode_rows_long(m, mt, 2, 1), "multi-device")
    base.expect(pkg, 6, lambda: lp.Prover.commit_long(m, mt, 2, 1), "multi-device")
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    base.expect(pkg, 6, lambda: lp.rs_encode_rows_long(sh, st, 2, 1), "sharded")
    base.expect(pkg, 6, lambda: lp.Prover.commit_long(sh, st, 2, 1), "sharded")


def test_the_chosen_shape_and_the_pool_balance(pkg):
    """commit_long chooses long_log_cols from the queries; after a long commit, a combine, an opening, the destroy and refused
    calls the pool is where it was, and the context still serves a short encoding"""
    lp = pkg.ligero_pcs
    ctx = base.ctx_of(pkg, GOLD)
    F = pkg.Field(GOLD)
    n, c = 20, 15
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, n)
    chosen = lp.Prover.commit_long(ctx, poly, queries=64)
    assert (chosen.log_cols, chosen.log_rows, chosen.log_blowup) == (lp.long_log_cols(n, 1, 64), n - lp.long_log_cols(n, 1, 64), 1)
    chosen.close()
    lp.Prover.commit_long(ctx, poly, c, 1).close()           # (the tables of this length are workspace of the context, made here)
    gc.collect()
    base_books = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")

    def workload():
        rng = random.Random(8)
        prover = lp.Prover.commit_long(ctx, poly, c, 1)
        prover.combine([F.rand(rng) for _ in range(n)], [F.rand(rng) for _ in range(1 << (n - c))])
        prover.open_columns([1, 2, 3])
        E = lp.rs_encode_rows_long(ctx, poly, c + 1, 2)
        del E
        base.expect(pkg, 1, lambda: prover.open_columns([1 << (c + 1)]))
        base.expect(pkg, 1, lambda: lp.Prover.commit_long(ctx, poly, c, 3))
        base.expect(pkg, 6, lambda: lp.rs_encode_rows(ctx, poly, c, 1), "LDS")            # the short entry point keeps its limit
        prover.close()

    workload()
    gc.collect()
    assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == base_books
    assert len(lp.rs_encode_rows(ctx, poly, 10, 1)) == 1 << (n + 1)
