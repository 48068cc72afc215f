"""The Relaxed PCS on the GPU (relaxed-pcs/src/lib.rs): sc_table_extend_grid against a numpy grid evaluation, the SHA-256 Merkle
commitment and its openings against trees built here with hashlib, the design limit n = 28, and the whole protocol of the
reference's `it_works` with a tampered leaf, path and univariate.  The checkers are test-local: hashlib, and an int64 numpy
MLE over F^m (p < 2^31, so every product is exact)."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from conftest import load_package
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD = 2**64 - 2**32 + 1
P59 = 2**64 - 59
R = 2**64


def expect(pkg, code, fn, *needles):
    with pytest.raises(pkg.SumcheckHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for s in needles:
        assert s in str(ei.value), (s, str(ei.value))


def mont(p, canon):
    return (np.asarray(canon, dtype=np.int64) * (R % p)) % p if p < 2**31 else np.array([int(x) * R % p for x in canon], dtype=np.uint64)


def grid_numpy(table_canon, p, m):
    """W~ at every point of F^m, v_0 the most significant digit, from the 2^m canonical entries (index bit j = variable j)"""
    t = np.asarray(table_canon, dtype=np.int64).reshape((2,) * m) if m else np.asarray(table_canon, dtype=np.int64).reshape(())
    # C-order reshape: axis a holds index bit m-1-a, i.e. variable m-1-a
    v = np.arange(p, dtype=np.int64)
    lag = np.stack([(1 - v) % p, v % p], axis=1)               # (p, 2): the line through (0, f0), (1, f1)
    for a in range(m):
        t = np.moveaxis(np.tensordot(lag, t, axes=([1], [a])) % p, 0, a)
    # axis a is variable m-1-a: put variable 0 first
    return np.transpose(t, tuple(range(m - 1, -1, -1))).reshape(-1) if m else t.reshape(1)


def padded(values, N):
    out = np.zeros(N, dtype=values.dtype)
    out[:values.size] = values
    return out


def leaf_hl(v):
    return hashlib.sha256(int(v).to_bytes(8, "little")).digest()


def levels_hl(canon):
    lev = [[leaf_hl(v) for v in canon]]
    while len(lev[-1]) > 1:
        prev = lev[-1]
        lev.append([hashlib.sha256(prev[2 * k] + prev[2 * k + 1]).digest() for k in range(len(prev) // 2)])
    return lev


def root_hl(canon):
    return levels_hl(canon)[-1][0]


def path_hl(levels, i):
    out = []
    for l in range(len(levels) - 1):
        out.append(levels[l][(i >> l) ^ 1])
    return out


def canon_of(F, words):
    p = F.p
    if p < 2**31:
        rinv = pow(R, -1, p)
        return (np.asarray(words, dtype=np.int64) % p * (rinv % p)) % p
    return [F.to_int(int(w)) for w in words]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


# ---- 1. sc_table_extend_grid -----------------------------------------------------------------------------------------

def _grid_cases():
    out = []
    for p in (3, 5, 7, 11, 17, 257, 65537):
        m = 0
        while p ** m <= 2**20:
            out.append((p, m))
            m += 1
    return out


@pytest.mark.parametrize("p,m", _grid_cases())
def test_extend_grid_equals_numpy(pkg, p, m):
    ctx = pkg.Context(pkg.Field(p))
    rng = np.random.default_rng(p * 100 + m)
    canon = rng.integers(0, p, size=1 << m, dtype=np.int64)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m, mont(p, canon).astype(np.uint64))
    g = pkg.relaxed_pcs.extend_grid(ctx, t)
    want = grid_numpy(canon, p, m)
    N = 1
    while N < p ** m:
        N *= 2
    got = g.to_evaluations()
    assert got.size == N
    assert np.array_equal(got, padded(mont(p, want).astype(np.uint64), N))


def test_extend_grid_at_its_limit_p11_m8(pkg):
    """p^m = 11^8 pads to exactly 2^28: 10^5 random points against the MLE, and the zero padding"""
    p, m = 11, 8
    ctx = pkg.Context(pkg.Field(p))
    rng = np.random.default_rng(118)
    canon = rng.integers(0, p, size=1 << m, dtype=np.int64)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m, mont(p, canon).astype(np.uint64))
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    g = pkg.relaxed_pcs.extend_grid(ctx, t)
    got = g.to_evaluations()
    log = ctx.launch_log()
    assert [r["kf"] for r in log if r["kind"] == "grid_extend"] == list(range(m - 1, -1, -1))
    assert got.size == 1 << 28
    idx = rng.integers(0, p ** m, size=100000)
    digits = np.stack([(idx // p ** (m - 1 - j)) % p for j in range(m)], axis=1)      # v_0 most significant
    x = np.arange(1 << m)
    w = np.ones((idx.size, 1 << m), dtype=np.int64)
    for j in range(m):
        bit = (x >> j) & 1
        w = w * np.where(bit[None, :] == 1, digits[:, j:j + 1], (1 - digits[:, j:j + 1]) % p) % p
    want = (w * canon[None, :] % p).sum(axis=1) % p
    assert np.array_equal(got[idx].astype(np.int64), mont(p, want))
    assert not got[p ** m:].any()


def test_extend_grid_refuses(pkg):
    for p in (GOLD, 2**31 - 1):
        ctx = pkg.Context(pkg.Field(p))
        t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 1, np.array([1, 2], dtype=np.uint64))
        expect(pkg, 6, lambda: pkg.relaxed_pcs.extend_grid(ctx, t), "exceed 2^28")
    ctx = pkg.Context(pkg.Field(5))
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2, np.array([1, 2, 3, 4], dtype=np.uint64))
    h = ctypes.c_void_p()
    rc = ctx.lib.sc_table_extend_grid(ctx.h, t.h, 3, ctypes.byref(h))
    assert rc == 1 and not h.value
    g = pkg.relaxed_pcs.extend_grid(ctx, t)            # the context still works
    assert len(g) == 32


# ---- 2. Merkle roots -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P59], ids=["gold", "p59"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 9, 12, 16, 20])
def test_merkle_root_equals_hashlib(pkg, p, n):
    F = pkg.Field(p)
    ctx = pkg.Context(F)
    rng = random.Random(n)
    canon = [rng.randrange(p) for _ in range(1 << n)]
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, np.array([F.from_int(v) for v in canon], dtype=np.uint64))
    tree = pkg.relaxed_pcs.merkle_commit(ctx, t)
    assert tree.depth == n
    assert tree.root() == root_hl(canon)


@pytest.mark.parametrize("p", [GOLD, P59, 11], ids=["gold", "p59", "p11"])
def test_merkle_root_of_constant_tables(pkg, p):
    F = pkg.Field(p)
    ctx = pkg.Context(F)
    for v in (0, p - 1):
        for n in (0, 5, 10):
            t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, np.full(1 << n, F.from_int(v), dtype=np.uint64))
            assert pkg.relaxed_pcs.merkle_commit(ctx, t).root() == root_hl([v] * (1 << n)), (v, n)


@pytest.mark.parametrize("p,m", [(3, 4), (5, 3), (7, 5), (11, 5), (17, 3)])
def test_merkle_root_of_padded_grids(pkg, p, m):
    F = pkg.Field(p)
    ctx = pkg.Context(F)
    rng = np.random.default_rng(7 * p + m)
    canon = rng.integers(0, p, size=1 << m, dtype=np.int64)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m, mont(p, canon).astype(np.uint64))
    g = pkg.relaxed_pcs.extend_grid(ctx, t)
    want = grid_numpy(canon, p, m)
    assert pkg.relaxed_pcs.merkle_commit(ctx, g).root() == root_hl(list(padded(want, len(g))))


# ---- 3. the design limit: n = 28 -------------------------------------------------------------------------------------

def _splitmix64(x):
    m = 2**64 - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_merkle_at_n28(pkg):
    F = pkg.Field(GOLD)
    ctx = pkg.Context(F)
    seed, n = 0x5EED28, 28
    t = pkg.DenseMultilinearExtension.generate(ctx, seed, n)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    tree = pkg.relaxed_pcs.merkle_commit(ctx, t)
    root = tree.root()
    kinds = [(r["kind"], r["kf"]) for r in ctx.launch_log()]
    assert ("merkle", 0) in kinds and ("merkle", 1) in kinds and ("merkle", 2) in kinds
    ctx.set_option("time_kernels", 0)
    # the 16 slices of 2^24, committed as borrowed tables at offsets, combine to the same root
    base = ctx.lib.sc_table_device_ptr(t.h)
    roots = []
    for k in range(16):
        s = pkg.DenseMultilinearExtension.from_device(ctx, base + 8 * (k << 24), 24, keep=t)
        roots.append(pkg.relaxed_pcs.merkle_commit(ctx, s).root())
        if k == 5:
            # one 2^22 slice in full against hashlib
            s22 = pkg.DenseMultilinearExtension.from_device(ctx, base + 8 * ((k << 24) + (3 << 22)), 22, keep=t)
            words = s22.to_evaluations()
            canon = [_splitmix64(seed + (k << 24) + (3 << 22) + i) % GOLD for i in range(1 << 22)]
            assert [F.to_int(int(w)) for w in words[:64]] == canon[:64]
            assert pkg.relaxed_pcs.merkle_commit(ctx, s22).root() == root_hl(canon)
        del s
    while len(roots) > 1:
        roots = [hashlib.sha256(roots[2 * k] + roots[2 * k + 1]).digest() for k in range(len(roots) // 2)]
    assert roots[0] == root
    # 64 random openings
    rng = random.Random(28)
    idx = [rng.randrange(1 << n) for _ in range(62)] + [0, (1 << n) - 1]
    for i, (path, leaf) in zip(idx, tree.open(idx)):
        assert leaf == _splitmix64(seed + i) % GOLD
        assert len(path.siblings) == n and path.verify_canonical(root, leaf)
        assert not path.verify_canonical(root, (leaf + 1) % GOLD)


# ---- 4. openings -----------------------------------------------------------------------------------------------------

def test_merkle_open_every_leaf_of_a_small_tree(pkg):
    F = pkg.Field(P59)
    ctx = pkg.Context(F)
    n = 10
    rng = random.Random(10)
    canon = [rng.randrange(P59) for _ in range(1 << n)]
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, np.array([F.from_int(v) for v in canon], dtype=np.uint64))
    tree = pkg.relaxed_pcs.merkle_commit(ctx, t)
    levels = levels_hl(canon)
    opened = tree.open(range(1 << n))
    for i, (path, leaf) in enumerate(opened):
        assert leaf == canon[i] and path.index == i
        assert path.siblings == path_hl(levels, i), i
    h = ctypes.c_void_p()
    leaves = np.zeros(1, dtype=np.uint64)
    bad = np.array([1 << n], dtype=np.uint64)
    buf = (ctypes.c_uint8 * (32 * n))()
    rc = ctx.lib.sc_merkle_open(ctx.h, tree.h, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1,
                                leaves.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), buf)
    assert rc == 1 and "not below N" in ctx.lib.sc_last_error(ctx.h).decode()
    del h


def test_merkle_open_batches_at_n20(pkg):
    F = pkg.Field(GOLD)
    ctx = pkg.Context(F)
    n, seed = 20, 77
    t = pkg.DenseMultilinearExtension.generate(ctx, seed, n)
    canon = [_splitmix64(seed + i) % GOLD for i in range(1 << n)]
    levels = levels_hl(canon)
    tree = pkg.relaxed_pcs.merkle_commit(ctx, t)
    assert tree.root() == levels[-1][0]
    rng = random.Random(20)
    for count in (1, 100, 5000):              # 5000: more than one launch of the gather
        idx = [rng.randrange(1 << n) for _ in range(count)]
        for i, (path, leaf) in zip(idx, tree.open(idx)):
            assert leaf == canon[i] and path.siblings == path_hl(levels, i)


# ---- 5. the protocol -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,m", [(5, 2), (11, 3), (11, 4), (11, 5), (11, 6), (11, 7), (11, 8), (17, 6)])
def test_protocol_it_works(pkg, p, m):
    """lib.rs:309-339 with SHA-256: honest replies verify (strict when the restriction has full degree, non-strict always);
    a tampered leaf, path or univariate is rejected"""
    rp = pkg.relaxed_pcs
    F = pkg.Field(p)
    ctx = pkg.Context(F)
    rng = random.Random(1000 * p + m)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, m, np.array([F.rand(rng) for _ in range(1 << m)], dtype=np.uint64))
    prover = rp.Prover.new(ctx, poly)
    root = prover.merkle_root()
    outcomes = set()
    for trial in range(4 if m > 6 else 12):
        strict = rp.Verifier(F, m, 1, root)
        loose = rp.Verifier(F, m, 1, root, strict_degree=False)
        b, c = loose.random_line(rng)
        strict.line = (b, c)
        q = prover.poly_restriction_to_line(b, c)
        point = loose.challenge_prover(rng)
        strict.x, strict.challenge_point = loose.x, point
        path, value = prover.challenge(point)
        assert path.index == rp.leaf_index(F, point)
        loose.commited_univariate(q)
        loose.verify_prover_reply(path, value)
        assert value == poly.evaluate(point)
        try:
            strict.commited_univariate(q)
            strict.verify_prover_reply(path, value)
            outcomes.add("strict accepts")
        except rp.DegreeMismatch:
            assert q.degree() < m
            outcomes.add("strict rejects")
        with pytest.raises(rp.MerkleMismatch):
            loose.verify_prover_reply(path, F.add(value, F.one))
        bad = list(path.siblings)
        bad[-1] = bytes(32)
        with pytest.raises(rp.MerkleMismatch):
            loose.verify_prover_reply(rp.Path(path.index, bad, F), value)
        dense = [0] * (m + 1)
        for d, cf in q.coeffs:
            dense[d] = cf
        dense[0] = F.add(dense[0], F.one)
        loose.commited_univariate(pkg.sum_check_protocol.SparsePolynomial.from_dense(F, dense))
        with pytest.raises(rp.EvalMismatch):
            loose.verify_prover_reply(path, value)
    # (q's top coefficient is the polynomial's top multilinear coefficient times prod_j (c_j - b_j): a polynomial whose top
    # coefficient vanishes never restricts to full degree, so only the reference's own shape is held to both outcomes)
    if p == 5:
        assert outcomes == {"strict accepts", "strict rejects"}, outcomes


def test_merkle_launch_records_at_n14(pkg):
    """2^14 leaves are the smallest tree that runs all three build phases: the leaf kernel up to level 4 (1024 nodes), one level
    launch, the top kernel on 512 nodes.  The records are pinned field by field."""
    F = pkg.Field(GOLD)
    ctx = pkg.Context(F)
    n, seed = 14, 1414
    t = pkg.DenseMultilinearExtension.generate(ctx, seed, n)
    canon = [_splitmix64(seed + i) % GOLD for i in range(1 << n)]
    levels = levels_hl(canon)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    tree = pkg.relaxed_pcs.merkle_commit(ctx, t)

    def merkle_records():
        return [(r["kf"], r["ks"], r["log_in"], r["bytes_read"], r["bytes_written"]) for r in ctx.launch_log() if r["kind"] == "merkle"]

    assert merkle_records() == [(0, 4, 14, 8 << 14, 32 << 10), (1, 5, 14, 32 << 10, 32 << 9), (2, 6, 14, 32 * 1022, 32 * 511)]
    assert tree.root() == levels[-1][0]
    idx = [0, 9001, (1 << n) - 1]
    opened = tree.open(idx)
    m = 3 * (8 * 16 + 32 * 10)
    assert merkle_records() == [(3, 4, 14, m, m)]
    for i, (path, leaf) in zip(idx, opened):
        assert leaf == canon[i] and path.siblings == path_hl(levels, i)
        assert path.verify_canonical(levels[-1][0], leaf)


# ---- 6. contexts that are not served, and the launch log -------------------------------------------------------------

def test_sharded_and_multi_device_are_refused(pkg):
    F = pkg.Field(GOLD)
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: pkg.relaxed_pcs.merkle_commit(m, mt), "multi-device")
    expect(pkg, 6, lambda: pkg.relaxed_pcs.extend_grid(m, mt), "multi-device")
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: pkg.relaxed_pcs.merkle_commit(sh, st), "sharded")
    expect(pkg, 6, lambda: pkg.relaxed_pcs.extend_grid(sh, st), "sharded")


def test_launch_log_names_the_new_kinds(pkg):
    F = pkg.Field(5)
    ctx = pkg.Context(F)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 3, F.from_ints(range(8)))
    g = pkg.relaxed_pcs.extend_grid(ctx, poly)
    tree = pkg.relaxed_pcs.merkle_commit(ctx, g)
    tree.open([3])
    log = ctx.launch_log()
    grid = [r for r in log if r["kind"] == "grid_extend"]
    assert [r["kf"] for r in grid] == [2, 1, 0]
    assert sum(r["bytes_written"] for r in grid) == 8 * (5 * 4 + 25 * 2 + 125)
    assert [r["kf"] for r in log if r["kind"] == "merkle"] == [0, 1, 2, 3] or \
        [r["kf"] for r in log if r["kind"] == "merkle"] == [0, 2, 3]
    assert {r["kind"] for r in log} == {"grid_extend", "merkle"}
    assert all(pkg._lib.MERKLE_KERNELS[r["kf"]] for r in log if r["kind"] == "merkle")
