"""The Ligero-style commitment over the expander code on the GPU (thaler-study_amd/csrc/kernels/expander.hpp,
engine/abi_expander.inc, ligero_pcs with code="expander") against tests/expander_ref.py, bit for bit: the row encoding over four
fields and every c up to 13, the refusals, the dispatch of sc_ligero_commit_code, roots, openings and row combinations of an
expander commitment, the whole protocol with every tampered message, the limit shape (n, c) = (21, 13), the launch log and
the pool's books.

The Python reference costs about a second for the first row of a level (its gather lists are then cached), so shapes are the
smallest that reach each path: every recursion depth (c = 6 .. 13), one row per block and several, codeword lengths on both
sides of the switch between the per-level and the one-block tree kernels."""
import ctypes
import gc
import random

import numpy as np
import pytest

import expander_ref as ref
import ligero_ref
import wide_words
from conftest import load_package
from ligero_common import context_cache, expect, flat, mont_np, upload
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD = 2**64 - 2**32 + 1
P59 = 2**64 - 59
BABYBEAR = 2013265921
FIELDS = [GOLD, P59, BABYBEAR, 257]
BIG = (GOLD, P59)
IDS = {GOLD: "gold", P59: "p59", BABYBEAR: "p2013265921", 257: "p257"}
R64 = 2**64

ctx_of, teardown_module = context_cache()


def canon_of(p, words):
    rinv = pow(R64, -1, p)
    return [int(w) * rinv % p for w in words]


def check_encode(pkg, p, r, c, table):
    ctx = ctx_of(pkg, p)
    E = pkg.ligero_pcs.xc_encode_rows(ctx, upload(pkg, ctx, p, table), c)
    got = E.to_evaluations()
    assert got.size == 2 << (r + c)
    want = mont_np(p, flat(ref.encode_rows(table, c, p)))
    assert np.array_equal(got, want), (p, r, c, int(np.flatnonzero(got != want)[0]))


# ---- 1. the encoding, bit for bit ------------------------------------------------------------------------------------

def _encode_cases():
    return [(p, c) for p in FIELDS for c in range(0, 14 if p in BIG else 12)]


@pytest.mark.parametrize("p,c", _encode_cases(), ids=lambda v: IDS.get(v, str(v)))
def test_encode_equals_the_reference(pkg, p, c):
    rng = random.Random(1000 * c + 1)
    for r in ((0, 1, 3) if c <= 11 else (0, 1)):
        check_encode(pkg, p, r, c, [rng.randrange(p) for _ in range(1 << (r + c))])


@pytest.mark.parametrize("r,c", [(8, 5), (6, 7), (4, 9)])
@pytest.mark.parametrize("p", FIELDS, ids=lambda v: IDS[v])
def test_encode_several_rows_per_block(pkg, p, r, c):
    rng = random.Random(10 * r + c)
    check_encode(pkg, p, r, c, [rng.randrange(p) for _ in range(1 << (r + c))])


@pytest.mark.parametrize("p", FIELDS, ids=lambda v: IDS[v])
def test_encode_worst_case_words(pkg, p):
    """at the field's largest shape: every word p - 1; 0 and p - 1 alternating; raw words built from wide_words.diff_classes"""
    r, c = (1, 13) if p in BIG else (3, 11)
    size = 1 << (r + c)
    check_encode(pkg, p, r, c, [p - 1] * size)
    check_encode(pkg, p, r, c, [0, p - 1] * (size // 2))
    raw = wide_words.octet_table(p, size, np.random.default_rng(c), share=1.0)
    assert wide_words.stride_classes(p, raw, 1) >= wide_words.classes_present(p)
    ctx = ctx_of(pkg, p)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, raw)
    got = pkg.ligero_pcs.xc_encode_rows(ctx, t, c).to_evaluations()
    want = mont_np(p, flat(ref.encode_rows(canon_of(p, raw), c, p)))
    assert np.array_equal(got, want), (p, int(np.flatnonzero(got != want)[0]))


# ---- 2. refusals and dispatch ----------------------------------------------------------------------------------------

def test_refusals(pkg):
    lp = pkg.ligero_pcs
    c5 = pkg.Context(pkg.Field(5))
    t5 = pkg.DenseMultilinearExtension.from_evaluations_vec(c5, 4, pkg.Field(5).from_ints(range(16)))
    for fn in (lambda: lp.xc_encode_rows(c5, t5, 2), lambda: lp.Prover.commit(c5, t5, 2, 1, code="expander")):
        expect(pkg, 6, fn, "p = 5")
    del t5
    c5.close()
    ctx = ctx_of(pkg, P59)
    F = pkg.Field(P59)
    big = pkg.DenseMultilinearExtension.generate(ctx, 5, 15)
    for fn in (lambda: lp.xc_encode_rows(ctx, big, 14), lambda: lp.Prover.commit(ctx, big, 14, 1, code="expander")):
        expect(pkg, 6, fn, "LDS")
    small = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 3, F.from_ints(range(8)))
    expect(pkg, 1, lambda: lp.Prover.commit(ctx, small, 1, 2, code="expander"), "log_blowup")
    expect(pkg, 1, lambda: lp.Prover.commit(ctx, small, 1, 0, code="expander"), "log_blowup")
    expect(pkg, 1, lambda: lp.xc_encode_rows(ctx, small, 4))
    expect(pkg, 1, lambda: lp.Prover.commit(ctx, small, 4, 1, code="expander"))
    h = ctypes.c_void_p()
    assert ctx.lib.sc_ligero_commit_code(ctx.h, small.h, 1, 1, 2, ctypes.byref(h)) == 1 and not h.value          # unknown code
    assert "code 2" in ctx.lib.sc_last_error(ctx.h).decode()
    assert ctx.lib.sc_ligero_commit_code(ctx.h, small.h, 1, 1, -1, ctypes.byref(h)) == 1 and not h.value
    assert ctx.lib.sc_xc_encode_rows(ctx.h, None, 1, ctypes.byref(h)) == 1 and not h.value                       # no table
    assert ctx.lib.sc_ligero_commit_code(ctx.h, None, 1, 1, 1, ctypes.byref(h)) == 1 and not h.value
    assert ctx.lib.sc_ligero_commit_code(ctx.h, small.h, 1, 1, 1, None) == 1
    code = ctypes.c_int(7)
    assert ctx.lib.sc_ligero_code(None, ctypes.byref(code)) == 1
    with pytest.raises(ValueError):
        lp.Prover.commit(ctx, small, 1, 1, code="ldpc")
    # Reed-Solomon is still refused over this field, and the context still works
    expect(pkg, 6, lambda: lp.Prover.commit(ctx, small, 2, 1), "2-adicity 2")
    expect(pkg, 6, lambda: lp.Prover.commit(ctx, small, 2, 1, code="rs"), "2-adicity 2")
    assert len(lp.xc_encode_rows(ctx, small, 2)) == 16


def test_sharded_and_multi_device_are_refused(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(P59)
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: lp.xc_encode_rows(m, mt, 2), "multi-device")
    expect(pkg, 6, lambda: lp.Prover.commit(m, mt, 2, 1, code="expander"), "multi-device")
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: lp.xc_encode_rows(sh, st, 2), "sharded")
    expect(pkg, 6, lambda: lp.Prover.commit(sh, st, 2, 1, code="expander"), "sharded")


def test_commit_code_rs_is_commit(pkg):
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, GOLD)
    rng = random.Random(2)
    table = [rng.randrange(GOLD) for _ in range(1 << 9)]
    poly = upload(pkg, ctx, GOLD, table)
    plain = lp.Prover.commit(ctx, poly, 5, 2)
    h = ctypes.c_void_p()
    ctx.check(ctx.lib.sc_ligero_commit_code(ctx.h, poly.h, 5, 2, 0, ctypes.byref(h)))
    coded = lp.Prover(ctx, poly, h)
    assert coded.root() == plain.root() == ligero_ref.root_of(ligero_ref.encode(table, 5, 2, GOLD))
    assert (coded.log_rows, coded.log_cols, coded.log_blowup, coded.code, plain.code) == (4, 5, 2, "rs", "rs")
    xp = lp.Prover.commit(ctx, poly, 5, 1, code="expander")
    assert (xp.log_rows, xp.log_cols, xp.log_blowup, xp.code) == (4, 5, 1, "expander")
    assert xp.root() != lp.Prover.commit(ctx, poly, 5, 1).root()
    for pr in (plain, coded, xp):
        pr.close()


# ---- 3. roots, openings, combinations --------------------------------------------------------------------------------

_provers = {}


def ref_prover(p, r, c):
    """one reference commitment per shape, shared by the tests below and left unchanged"""
    if (p, r, c) not in _provers:
        rng = random.Random(100 * r + c)
        table = [rng.randrange(p) for _ in range(1 << (r + c))]
        _provers[(p, r, c)] = (table, ref.RefProver(table, c, p))
    return _provers[(p, r, c)]


# L = 256, 512, 1024 leaves: below, at and above the 2 * kMerkleTopNodes = 512 nodes the one-block tree kernel takes; column
# bytes 8, 16 (one hash block with its padding), 64 (a data block and a padding block), 512 (several)
@pytest.mark.parametrize("r", [0, 1, 3, 6])
@pytest.mark.parametrize("c", [7, 8, 9])
@pytest.mark.parametrize("p", [P59, GOLD], ids=lambda v: IDS[v])
def test_root_equals_hashlib_over_the_reference_encoding(pkg, p, r, c):
    ctx = ctx_of(pkg, p)
    table, rp = ref_prover(p, r, c)
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, p, table), c, 1, code="expander")
    assert (prover.log_rows, prover.log_cols, prover.log_blowup, prover.code) == (r, c, 1, "expander")
    root = prover.root()
    assert root == rp.root()
    L = 2 << c
    cols = [0, 1, L // 2 - 1, L // 2, L - 1, 77 % L, 77 % L]
    for (j, vals, path), (rj, rvals, rsib) in zip(prover.open_columns(cols), rp.open_columns(cols)):
        assert j == rj and vals == ligero_ref.mont(p, rvals) and path.siblings == rsib, j
        assert path.verify_column(root, vals)
    expect(pkg, 1, lambda: prover.open_columns([L]), "not below L")
    prover.close()


@pytest.mark.parametrize("r,c", [(0, 7), (3, 8), (6, 9)])
@pytest.mark.parametrize("p", [P59, GOLD], ids=lambda v: IDS[v])
def test_combine_equals_the_reference(pkg, p, r, c):
    ctx = ctx_of(pkg, p)
    table, _ = ref_prover(p, r, c)
    rng = random.Random(r + c)
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, p, table), c, 1, code="expander")
    weights = [[rng.randrange(p) for _ in range(1 << r)] for _ in range(4)]
    want = [ligero_ref.mont(p, ref.combine(table, c, w, p)) for w in weights]
    for M in (1, 2, 4):
        assert prover.combine_rows([ligero_ref.mont(p, w) for w in weights[:M]]) == want[:M], (r, c, M)
    prover.close()


# ---- 4. the protocol -------------------------------------------------------------------------------------------------

def run_protocol(pkg, prover, poly, table, p, n, c, queries, rng, rp=None, tamper=None):
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    root = prover.root()
    v = lp.Verifier(F, n, c, 1, root if tamper != "root" else bytes([root[0] ^ 1]) + root[1:], queries, code="expander")
    gamma = v.draw_gamma(rng)
    point = [F.rand(rng) for _ in range(n)]
    u_gamma, u_z = prover.combine(point, gamma)
    if tamper is None and rp is not None:
        ru_gamma, ru_z = rp.combine(ligero_ref.canon(p, point), ligero_ref.canon(p, gamma))
        assert u_gamma == ligero_ref.mont(p, ru_gamma) and u_z == ligero_ref.mont(p, ru_z)
    if tamper == "u_z":
        u_z[len(u_z) // 2] = F.add(u_z[len(u_z) // 2], F.one)
    if tamper == "u_gamma":
        u_gamma[0] = F.add(u_gamma[0], F.one)
    v.receive(u_gamma, u_z)
    openings = prover.open_columns(v.draw_columns(rng))
    if tamper == "column":
        j, vals, path = openings[3]
        openings[3] = (j, [F.add(vals[0], F.one)] + vals[1:], path)
    if tamper == "path":
        j, vals, path = openings[5]
        openings[5] = (j, vals, lp.ColumnPath(j, [bytes(32)] + path.siblings[1:], F))
    value = v.verify(point, openings)
    assert value == poly.evaluate(point)                                     # sc_table_evaluate, LE
    if table is not None:
        assert value == F.from_int(ligero_ref.mle_eval(table, ligero_ref.canon(p, point), p))


@pytest.mark.parametrize("p,n,c", [(P59, 10, 6), (P59, 9, 4), (GOLD, 12, 8)], ids=lambda v: IDS.get(v, str(v)))
def test_protocol(pkg, p, n, c):
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, p)
    rng = random.Random(n)
    table = [rng.randrange(p) for _ in range(1 << n)]
    poly = upload(pkg, ctx, p, table)
    prover = lp.Prover.commit(ctx, poly, c, 1, code="expander")
    rp = ref.RefProver(table, c, p)
    assert prover.root() == rp.root()
    run_protocol(pkg, prover, poly, table, p, n, c, 16, rng, rp)
    for tamper, err in (("u_z", lp.EvalMismatch), ("u_gamma", lp.ProximityMismatch), ("column", lp.MerkleMismatch),
                        ("path", lp.MerkleMismatch), ("root", lp.MerkleMismatch)):
        with pytest.raises(err):
            run_protocol(pkg, prover, poly, table, p, n, c, 16, rng, rp, tamper=tamper)
    prover.close()


def test_default_shape(pkg):
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, P59)
    prover = lp.Prover.commit(ctx, pkg.DenseMultilinearExtension.generate(ctx, 9, 11), code="expander")
    assert (prover.log_rows, prover.log_cols, prover.log_blowup, prover.code) == (5, 6, 1, "expander")
    assert lp.default_log_cols(28, 1, "expander") == 13
    prover.close()


# ---- 5. the limit shape, with the launch log -------------------------------------------------------------------------

def test_the_limit_shape(pkg):
    """2^64 - 59, (n, c) = (21, 13): L = 2^14, one row per block (128 KiB of LDS), E of 32 MiB"""
    lp = pkg.ligero_pcs
    p = P59
    ctx = ctx_of(pkg, p)
    n, c = 21, 13
    r, C, L = n - c, 1 << c, 2 << c
    R = 1 << r
    poly = pkg.DenseMultilinearExtension.generate(ctx, 0x11CE, n)
    words = poly.to_evaluations().reshape(R, C)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    prover = lp.Prover.commit(ctx, poly, c, 1, code="expander")
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    # the traffic model: the table read once, E written once; then the column hash and the tree, as over Reed-Solomon
    enc = [x for x in log if x["kind"] == "xc_encode"]
    assert [(x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in enc] == [(c, 4, n, 8 << n, 8 << (n + 1))]
    leaf = [x for x in log if x["kind"] == "ligero"]
    assert [(x["kf"], x["ks"], x["bytes_read"], x["bytes_written"]) for x in leaf] == [(0, r, 8 << (n + 1), 32 * L)]
    assert {x["kind"] for x in log} == {"xc_encode", "ligero", "merkle"}
    # the same encoding through sc_xc_encode_rows, downloaded
    E = lp.xc_encode_rows(ctx, poly, c).to_evaluations().reshape(R, L)
    for i in (0, 1, R // 2, R - 1):
        want = ref.encode(canon_of(p, words[i]), p)
        assert np.array_equal(E[i], mont_np(p, want)), i
    rng = random.Random(21)
    j = rng.randrange(L)
    [(jj, vals, path)] = prover.open_columns([j])
    assert jj == j and vals == [int(x) for x in E[:, j]] and path.verify_column(prover.root(), vals)
    # eight whole columns of E through linearity: Enc(sum_i g_i row_i)[j] = sum_i g_i E[i][j]
    run_protocol(pkg, prover, poly, None, p, n, c, 8, rng)
    prover.close()


def test_launch_log_has_one_encode_record(pkg):
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, GOLD)
    n, c = 12, 7
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, n)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    E = lp.xc_encode_rows(ctx, poly, c)
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert [(x["kind"], x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in log] == [("xc_encode", c, 1, n, 8 << n, 8 << (n + 1))]
    del E


# ---- 6. the pool's books ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [P59, GOLD], ids=lambda v: IDS[v])
def test_pool_balance(pkg, p):
    """after a commit, a combine, an opening and the destroy - and after refused calls - the pool is where it was"""
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, p)
    F = pkg.Field(p)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, 12)
    wide = pkg.DenseMultilinearExtension.generate(ctx, 1, 15)
    lp.Prover.commit(ctx, poly, 6, 1, code="expander").close()    # (the table of inverses is workspace of the context, made here)
    gc.collect()
    base = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")

    def workload():
        rng = random.Random(8)
        prover = lp.Prover.commit(ctx, poly, 6, 1, code="expander")
        prover.combine([F.rand(rng) for _ in range(12)], [F.rand(rng) for _ in range(64)])
        prover.open_columns([1, 2, 3])
        E = lp.xc_encode_rows(ctx, poly, 5)
        del E
        expect(pkg, 1, lambda: prover.open_columns([1 << 7]))
        expect(pkg, 1, lambda: lp.Prover.commit(ctx, poly, 6, 2, code="expander"))
        expect(pkg, 1, lambda: lp.xc_encode_rows(ctx, poly, 13))
        expect(pkg, 6, lambda: lp.Prover.commit(ctx, wide, 14, 1, code="expander"))
        expect(pkg, 6, lambda: lp.xc_encode_rows(ctx, wide, 14))
        prover.close()

    workload()
    gc.collect()
    assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == base
