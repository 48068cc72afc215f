"""The Ligero-style commitment on the GPU (thaler-study_amd/ligero_pcs.py, csrc/kernels/ligero.hpp) against tests/ligero_ref.py:
the row encoding bit for bit, the refusals, the root and the openings against hashlib over the reference encoding, the row
combinations, the whole protocol with every tampered message, the limit shape L = 2^14, and the pool's books.

Shapes are the smallest that reach every path of the kernels: every c + rho from 1 to 14 (all register-radix remainders, one
row per block and several), 1 to 64 rows per column hash (one block with its padding, a data block plus a padding block,
several), codeword lengths on both sides of the switch between the per-level and the one-block tree kernels."""
import ctypes
import gc
import hashlib
import random

import numpy as np
import pytest

import ligero_ref as ref
from conftest import load_package
from ligero_common import context_cache, expect, flat, mont_np, upload
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD = ref.GOLD
P59 = 2**64 - 59
IDS = {GOLD: "gold", ref.BABYBEAR: "p2013265921", 65537: "p65537", 257: "p257", P59: "p59"}

ctx_of, teardown_module = context_cache()


# ---- 1. the encoding, bit for bit ------------------------------------------------------------------------------------

def _encode_cases():
    out = []
    for p in ref.FIELDS:
        for log_len in range(1, min(14, ref.ROOTS[p][0]) + 1):
            for rho in (1, 2):
                if log_len - rho >= 0:
                    out.append((p, log_len, rho))
    return out


@pytest.mark.parametrize("p,log_len,rho", _encode_cases(), ids=lambda v: IDS.get(v, str(v)))
def test_encode_equals_the_reference(pkg, p, log_len, rho):
    ctx = ctx_of(pkg, p)
    c = log_len - rho
    rng = random.Random(1000 * log_len + rho)
    shapes = [(r, c) for r in (0, 1, 3)] + ([(5, 0)] if c == 0 else [])
    tables = [((r, cc), [rng.randrange(p) for _ in range(1 << (r + cc))]) for r, cc in shapes]
    if log_len == min(14, ref.ROOTS[p][0]):
        # the largest shape of the field: every word p - 1, and 0 / p - 1 alternating
        tables.append(((3, c), [p - 1] * (8 << c)))
        tables.append(((3, c), [0, p - 1] * (4 << c)))
    for (r, cc), table in tables:
        t = upload(pkg, ctx, p, table)
        E = pkg.ligero_pcs.rs_encode_rows(ctx, t, cc, rho)
        got = E.to_evaluations()
        assert got.size == 1 << (r + cc + rho)
        want = mont_np(p, flat(ref.encode(table, cc, rho, p)))
        assert np.array_equal(got, want), (p, r, cc, rho, int(np.flatnonzero(got != want)[0]))


# ---- 2. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(P59)
    ctx = ctx_of(pkg, P59)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 4, F.from_ints(range(16)))
    for fn in (lambda: lp.rs_encode_rows(ctx, t, 2, 1), lambda: lp.Prover.commit(ctx, t, 2, 1)):
        expect(pkg, 6, fn, "2-adicity 2", str(P59))
    assert lp.Prover.commit(ctx, t, 1, 1).log_rows == 3                      # c + rho = 2 = s is served
    g = ctx_of(pkg, GOLD)
    G = pkg.Field(GOLD)
    big = pkg.DenseMultilinearExtension.generate(g, 5, 14)
    for fn in (lambda: lp.rs_encode_rows(g, big, 14, 1), lambda: lp.Prover.commit(g, big, 13, 2)):
        expect(pkg, 6, fn, "LDS")
    small = pkg.DenseMultilinearExtension.from_evaluations_vec(g, 3, G.from_ints(range(8)))
    for log_cols, rho in ((1, 0), (1, 3), (4, 1)):
        expect(pkg, 1, lambda: lp.rs_encode_rows(g, small, log_cols, rho))
        expect(pkg, 1, lambda: lp.Prover.commit(g, small, log_cols, rho))
    # a table that is not 2^n long cannot be made, and no table at all is refused
    h = ctypes.c_void_p()
    words = np.arange(24, dtype=np.uint64)
    assert g.lib.sc_table_upload(g.h, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 24, ctypes.byref(h)) == 1 and not h.value
    assert g.lib.sc_rs_encode_rows(g.h, None, 1, 1, ctypes.byref(h)) == 1 and not h.value
    assert g.lib.sc_ligero_commit(g.h, None, 1, 1, ctypes.byref(h)) == 1 and not h.value
    assert len(lp.rs_encode_rows(g, small, 2, 1)) == 16                      # the context still works


def test_sharded_and_multi_device_are_refused(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: lp.rs_encode_rows(m, mt, 2, 1), "multi-device")
    expect(pkg, 6, lambda: lp.Prover.commit(m, mt, 2, 1), "multi-device")
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: lp.rs_encode_rows(sh, st, 2, 1), "sharded")
    expect(pkg, 6, lambda: lp.Prover.commit(sh, st, 2, 1), "sharded")


# ---- 3. the root -----------------------------------------------------------------------------------------------------

# (r, log_len): column bytes 8, 16, 32 (one block), 64 (a data block and a padding block), 128 and 512 (several); L = 2, 4, 512,
# 1024 and 2^14 leaves - below, at and above the 2 * kMerkleTopNodes = 512 nodes the one-block kernel takes
ROOT_SHAPES = [(0, 1), (1, 2), (2, 9), (3, 10), (4, 14), (6, 9), (6, 2), (0, 14), (1, 10), (3, 1), (4, 2), (2, 14)]


@pytest.mark.parametrize("r,log_len", ROOT_SHAPES)
@pytest.mark.parametrize("p", [GOLD, 65537], ids=lambda v: IDS[v])
def test_root_equals_hashlib_over_the_reference_encoding(pkg, p, r, log_len):
    ctx = ctx_of(pkg, p)
    rho = 1 + (r + log_len) % 2 if log_len >= 2 else 1
    c = log_len - rho
    rng = random.Random(100 * r + log_len)
    table = [rng.randrange(p) for _ in range(1 << (r + c))]
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, p, table), c, rho)
    assert (prover.log_rows, prover.log_cols, prover.log_blowup) == (r, c, rho)
    assert prover.root() == ref.root_of(ref.encode(table, c, rho, p))
    prover.close()


# ---- 4. row combinations ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c", [(0, 3), (3, 0), (5, 4), (12, 1)])
@pytest.mark.parametrize("p", [GOLD, 65537], ids=lambda v: IDS[v])
def test_combine_equals_the_reference(pkg, p, r, c):
    ctx = ctx_of(pkg, p)
    rng = random.Random(10 * r + c)
    table = [rng.randrange(p) for _ in range(1 << (r + c))]
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, p, table), c, 1)
    weights = [[rng.randrange(p) for _ in range(1 << r)] for _ in range(4)]
    want = [ref.mont(p, ref.combine(table, c, w, p)) for w in weights]
    for M in (1, 2, 3, 4):
        got = prover.combine_rows([ref.mont(p, w) for w in weights[:M]])
        assert got == want[:M], (r, c, M)
    assert prover.combine_rows([]) == []                                     # count = 0: nothing happens
    out = np.zeros(5 << c, dtype=np.uint64)
    w5 = np.zeros(5 << r, dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    assert ctx.lib.sc_ligero_combine_rows(ctx.h, prover.h, w5.ctypes.data_as(u64p), 5, out.ctypes.data_as(u64p)) == 1
    prover.close()


@pytest.mark.parametrize("p", [GOLD, P59], ids=lambda v: IDS[v])
def test_combine_of_worst_case_words(pkg, p):
    """every weight and every entry p - 1 at (r, c) = (12, 1), on both field templates: every product is (p - 1)^2, the largest
    there is, over the longest run a thread accumulates without reducing"""
    ctx = ctx_of(pkg, p)
    r, c = 12, 1
    table = [p - 1] * (1 << (r + c))
    prover = pkg.ligero_pcs.Prover.commit(ctx, upload(pkg, ctx, p, table), c, 1)
    weights = [[p - 1] * (1 << r)] * 4
    want = ref.mont(p, ref.combine(table, c, weights[0], p))
    for M in (1, 4):
        assert prover.combine_rows([ref.mont(p, w) for w in weights[:M]]) == [want] * M
    prover.close()


# ---- 5. openings -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, 65537], ids=lambda v: IDS[v])
def test_open_every_column(pkg, p):
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    ctx = ctx_of(pkg, p)
    r, c, rho = 3, 4, 1
    rng = random.Random(5)
    table = [rng.randrange(p) for _ in range(1 << (r + c))]
    poly = upload(pkg, ctx, p, table)
    prover = lp.Prover.commit(ctx, poly, c, rho)
    rp = ref.RefProver(table, c, rho, p)
    root = prover.root()
    assert root == rp.root()
    L = 1 << (c + rho)
    opened = prover.open_columns(range(L))
    for (j, vals, path), (rj, rvals, rsib) in zip(opened, rp.open_columns(range(L))):
        assert j == rj and vals == ref.mont(p, rvals) and path.siblings == rsib, j
        assert isinstance(path, pkg.relaxed_pcs.Path) and path.verify_column(root, vals)
        assert not path.verify_column(root, [F.add(vals[0], F.one)] + vals[1:])
    repeated = prover.open_columns([7, 7, 0, L - 1, 7])
    assert [(j, v, q.siblings) for j, v, q in repeated] == [(opened[j][0], opened[j][1], opened[j][2].siblings) for j in (7, 7, 0, L - 1, 7)]
    assert prover.open_columns([]) == []
    expect(pkg, 1, lambda: prover.open_columns([L]), "not below L")
    other = pkg.Context(F)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    idx, vals, paths = np.zeros(1, dtype=np.uint64), np.zeros(1 << r, dtype=np.uint64), (ctypes.c_uint8 * (32 * (c + rho)))()
    assert other.lib.sc_ligero_open_columns(other.h, prover.h, idx.ctypes.data_as(u64p), 1, vals.ctypes.data_as(u64p), paths) == 1
    assert "another context" in other.lib.sc_last_error(other.h).decode()
    assert other.lib.sc_ligero_combine_rows(other.h, prover.h, vals.ctypes.data_as(u64p), 1, vals.ctypes.data_as(u64p)) == 1
    assert other.lib.sc_ligero_destroy(other.h, prover.h) == 1
    other.close()
    prover.close()


# ---- 6. the protocol -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,n,c,rho", [(GOLD, 10, 5, 1), (GOLD, 12, 7, 2), (65537, 8, 4, 1)], ids=lambda v: IDS.get(v, str(v)))
def test_protocol(pkg, p, n, c, rho):
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    ctx = ctx_of(pkg, p)
    rng = random.Random(n)
    table = [rng.randrange(p) for _ in range(1 << n)]
    poly = upload(pkg, ctx, p, table)
    prover = lp.Prover.commit(ctx, poly, c, rho)
    rp = ref.RefProver(table, c, rho, p)
    root = prover.root()
    assert root == rp.root()

    def run(tamper=None):
        v = lp.Verifier(F, n, c, rho, root if tamper != "root" else bytes([root[0] ^ 1]) + root[1:], 16)
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
        openings = prover.open_columns(v.draw_columns(rng))
        if tamper == "column":
            j, vals, path = openings[3]
            openings[3] = (j, [F.add(vals[0], F.one)] + vals[1:], path)
        if tamper == "path":
            j, vals, path = openings[5]
            openings[5] = (j, vals, lp.ColumnPath(j, [bytes(32)] + path.siblings[1:], F))
        value = v.verify(point, openings)
        assert value == poly.evaluate(point)                                 # sc_table_evaluate, LE
        assert value == F.from_int(ref.mle_eval(table, ref.canon(p, point), p))

    run()
    for tamper, err in (("u_z", lp.EvalMismatch), ("u_gamma", lp.ProximityMismatch), ("column", lp.MerkleMismatch),
                        ("path", lp.MerkleMismatch), ("root", lp.MerkleMismatch)):
        with pytest.raises(err):
            run(tamper)
    prover.close()


def test_default_shape(pkg):
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, GOLD)
    prover = lp.Prover.commit(ctx, pkg.DenseMultilinearExtension.generate(ctx, 9, 11))
    assert (prover.log_rows, prover.log_cols, prover.log_blowup) == (5, 6, 1)
    assert lp.default_log_cols(28, 1) == 13 and lp.default_log_cols(28, 2) == 12
    prover.close()


# ---- 7. the limit shape ----------------------------------------------------------------------------------------------

def _splitmix64(x):
    m = 2**64 - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def gold_canon_np(words):
    """Goldilocks Montgomery words -> canonical values, in wrapping uint64 arithmetic: x 2^-64 = -floor(m p / 2^64) mod p for the
    m with m p = -x mod 2^64, m = x (2^32 + 1) (checked against big integers by its caller)"""
    x = np.asarray(words, dtype=np.uint64)
    s = np.uint64(32)
    m = x + (x << s)
    h = m - (m >> s) - (m < (m << s)).astype(np.uint64)
    return np.where(h == 0, np.uint64(0), np.uint64(GOLD) - h)


def test_the_limit_shape(pkg):
    """Goldilocks, (n, c, rho) = (22, 13, 1): L = 2^14, one row per block, E of 64 MiB"""
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, GOLD)
    n, c, rho, seed = 22, 13, 1, 0x11CE
    r, C, L = n - c, 1 << c, 1 << (c + rho)
    R = 1 << r
    poly = pkg.DenseMultilinearExtension.generate(ctx, seed, n)
    ctx.synchronize()
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    prover = lp.Prover.commit(ctx, poly, c, rho)
    root = prover.root()
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    # the traffic model: the table read once, E written once; E read once by the column hash; every tree level read and written once
    enc = [x for x in log if x["kind"] == "rs_encode"]
    assert [(x["kf"], x["ks"], x["log_in"], x["bytes_read"], x["bytes_written"]) for x in enc] == [(c, rho, n, 8 << n, 8 << (n + rho))]
    leaf = [x for x in log if x["kind"] == "ligero"]
    assert [(x["kf"], x["ks"], x["bytes_read"], x["bytes_written"]) for x in leaf] == [(0, r, 8 << (n + rho), 32 * L)]
    merkle = [(x["kf"], x["bytes_read"], x["bytes_written"]) for x in log if x["kind"] == "merkle"]
    assert merkle == [(1, 32 * (L >> k), 32 * (L >> (k + 1))) for k in range(5)] + [(2, 32 * (1024 - 2), 32 * 511)]
    assert {x["kind"] for x in log} == {"rs_encode", "ligero", "merkle"}
    # the same encoding through sc_rs_encode_rows, downloaded
    E = lp.rs_encode_rows(ctx, poly, c, rho).to_evaluations().reshape(R, L)
    table_row = lambda i: [_splitmix64(seed + i * C + k) % GOLD for k in range(C)]
    w = ref.omega(GOLD, c + rho)
    for i in (0, R - 1):
        want = ref.ntt_rows_np([table_row(i) + [0] * (L - C)], w, GOLD)[0]
        assert np.array_equal(E[i], mont_np(GOLD, want)), i
    rng = random.Random(22)
    F = pkg.Field(GOLD)
    for _ in range(64):
        i, j = rng.randrange(R), rng.randrange(L)
        assert int(E[i, j]) == F.from_int(ref.direct(table_row(i), w, GOLD, j)), (i, j)
    # the root, with hashlib over the downloaded E
    canon = gold_canon_np(E)
    sample = [(rng.randrange(R), rng.randrange(L)) for _ in range(1000)]
    assert all(int(canon[i, j]) == F.to_int(int(E[i, j])) for i, j in sample)
    cols = np.ascontiguousarray(canon.T).astype("<u8")
    leaves = [hashlib.sha256(cols[j].tobytes()).digest() for j in range(L)]
    assert ref.tree_levels(leaves)[-1][0] == root
    j = rng.randrange(L)
    [(jj, vals, path)] = prover.open_columns([j])
    assert jj == j and vals == [int(x) for x in E[:, j]] and path.verify_column(root, vals)
    prover.close()


# ---- 8. the pool's books ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, 65537], ids=lambda v: IDS[v])
def test_pool_balance(pkg, p):
    """after a commit, a combine, an opening and the destroy - and after refused calls - the pool is where it was"""
    lp = pkg.ligero_pcs
    ctx = ctx_of(pkg, p)
    F = pkg.Field(p)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, 12)
    lp.Prover.commit(ctx, poly, 6, 1).close()        # (the twiddle table of this length is workspace of the context, made here)
    gc.collect()
    base = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")

    def workload():
        rng = random.Random(8)
        prover = lp.Prover.commit(ctx, poly, 6, 1)
        prover.combine([F.rand(rng) for _ in range(12)], [F.rand(rng) for _ in range(64)])
        prover.open_columns([1, 2, 3])
        E = lp.rs_encode_rows(ctx, poly, 5, 2)
        del E
        expect(pkg, 1, lambda: prover.open_columns([1 << 7]))
        expect(pkg, 1, lambda: lp.Prover.commit(ctx, poly, 6, 3))
        prover.close()

    workload()
    gc.collect()
    assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == base
