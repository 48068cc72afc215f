"""C = A * B on the GPU (sc_matmul: the int8 matrix-core kernel and the VALU kernels of kernels/matmul.hpp) and the MatMult
protocol around it (matrix_multiplication.prove_product / verify_product) - against the reference's known answers, pyref's
big-integer product, exact sampled entries, the oracle's G::new and pyref's transcript; the accumulator bound at the largest
size; the refusals and the pool."""
import ctypes
import random

import numpy as np
import pytest

from conftest import load_package
from test_gpu_sharded import Loopback
from util import GOLD, TOY_MODULI, load_golden, oracle, pid, pyref
from wide_words import WIDE, edge_table, wid

pytestmark = pytest.mark.gpu

P59 = 2**64 - 59
R = 2**64
PATHS = {"auto": 0, "mfma": 1, "valu": 2}


def ctx_for(pkg, p, path="auto"):
    ctx = pkg.Context(pkg.Field(p))
    ctx.set_option("matmul_path", PATHS[path])
    return ctx


def paths_for(n):
    """the paths that differ at this size: below 2^4 rows every path is the one-thread-per-entry VALU kernel"""
    return ["auto", "mfma", "valu"] if n >= 4 else ["auto"]


def device_product(pkg, ctx, n, a_words, b_words):
    C = pkg.matrix_multiplication.matmul(ctx, n, a_words, b_words)
    return C.to_evaluations()


def exact_words(a_words, b_words, n, p):
    """the Montgomery words of A * B from raw words, by pyref's big-integer product: (sum a b) R^-1 mod p"""
    N = 1 << n
    A = [[int(x) for x in a_words[i * N:(i + 1) * N]] for i in range(N)]
    B = [[int(x) for x in b_words[i * N:(i + 1) * N]] for i in range(N)]
    rinv = pow(R, -1, p)
    C = pyref.matmul(A, B, p)   # sum a b mod p of the raw words
    return np.array([c * rinv % p for row in C for c in row], dtype=np.uint64)


# ---- exactness ----------------------------------------------------------------------------------------------------

def test_matrix_test_from_book():
    """matrix_test_from_book (matrix-multiplication/src/lib.rs:203-303): the product over F_5, canonical values"""
    pkg = load_package()
    kat = load_golden("reference_kats.json")["matmul_book"]
    p, n = kat["p"], kat["n"]
    for path in ["auto", "mfma", "valu"]:
        ctx = ctx_for(pkg, p, path)
        F = ctx.field
        A = F.from_ints([x for row in kat["A"] for x in row])
        B = F.from_ints([x for row in kat["B"] for x in row])
        C = F.to_ints(device_product(pkg, ctx, n, A, B))
        assert C == [x for row in kat["C"] for x in row], path


@pytest.mark.parametrize("path", ["auto", "mfma", "valu"])
def test_randomized_f5_cases(path):
    """every case of randomized_test's fixture (matrix-multiplication/src/lib.rs:316-352)"""
    pkg = load_package()
    kat = load_golden("reference_kats.json")["matmul_randomized_f5"]
    ctx = ctx_for(pkg, kat["p"], path)
    F = ctx.field
    for case in kat["cases"]:
        n = case["logn"]
        A = F.from_ints([x for row in case["A"] for x in row])
        B = F.from_ints([x for row in case["B"] for x in row])
        assert F.to_ints(device_product(pkg, ctx, n, A, B)) == [x for row in case["C"] for x in row], n


@pytest.mark.parametrize("p", [GOLD] + TOY_MODULI, ids=pid)
def test_exact_small_fields(p):
    pkg = load_package()
    rng = np.random.default_rng(p % 1000)
    ctxs = {path: ctx_for(pkg, p, path) for path in PATHS}
    for n in range(0, 8):
        a = rng.integers(0, p, size=1 << (2 * n), dtype=np.uint64)
        b = rng.integers(0, p, size=1 << (2 * n), dtype=np.uint64)
        want = exact_words(a, b, n, p)
        for path in paths_for(n):
            got = device_product(pkg, ctxs[path], n, a, b)
            assert np.array_equal(got, want), (n, path, int(np.argmax(got != want)))


@pytest.mark.parametrize("p", WIDE, ids=wid)
def test_exact_wide_moduli_edge_words(p):
    pkg = load_package()
    rng = np.random.default_rng(p % 997)
    ctxs = {path: ctx_for(pkg, p, path) for path in PATHS}
    for n in range(0, 8):
        a = edge_table(p, 1 << (2 * n), rng)
        b = edge_table(p, 1 << (2 * n), rng)
        want = exact_words(a, b, n, p)
        for path in paths_for(n):
            got = device_product(pkg, ctxs[path], n, a, b)
            assert np.array_equal(got, want), (n, path, int(np.argmax(got != want)))


# ---- large n -------------------------------------------------------------------------------------------------------

def sample_positions(n, rng, count=256):
    """tile corners (16 x 16 MFMA tiles, 64 x 64 VALU tiles), the last row and column, and random entries"""
    N = 1 << n
    pos = {(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)}
    for t in (15, 16, 63, 64):
        pos |= {(t, t), (t, N - 1 - t), (N - 1, t), (t, N - 1)}
    pos |= {(N - 1, int(j)) for j in rng.integers(0, N, 8)} | {(int(i), N - 1) for i in rng.integers(0, N, 8)}
    while len(pos) < count:
        pos.add((int(rng.integers(0, N)), int(rng.integers(0, N))))
    return sorted(pos)


def check_sampled(a, b, c, n, p, rng):
    N = 1 << n
    A, B, C = a.reshape(N, N), b.reshape(N, N), c.reshape(N, N)
    rinv = pow(R, -1, p)
    cols = {}
    for i, j in sample_positions(n, rng):
        if j not in cols:
            cols[j] = [int(x) for x in B[:, j]]
        row = [int(x) for x in A[i]]
        want = sum(x * y for x, y in zip(row, cols[j])) % p * rinv % p
        assert int(C[i, j]) == want, (n, i, j)


def check_identity(pkg, ctx, n, a, b, C, p, seed):
    """f~_C(r1, r2) == c_1 of the oracle's G::new(A, B, (r1, r2)) - computed without the new kernel"""
    mm = pkg.matrix_multiplication
    o = oracle(p)
    pt = mm.product_point(ctx.field, n, seed)
    fa, fb = o.g_new(n, a, b, np.array(pt, dtype=np.uint64))
    assert mm.product_claim(C, pt) == o.c1(fa, fb), (n, seed)


@pytest.mark.parametrize("p", [GOLD, P59], ids=pid)
@pytest.mark.parametrize("n", [10, 12, 13])
def test_large_sampled_and_identity(n, p):
    pkg = load_package()
    paths = ["auto", "valu"] if n <= 12 else ["auto"]
    for path in paths:
        ctx = ctx_for(pkg, p, path)
        A = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A + n, 2 * n)
        B = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_B + n, 2 * n)
        C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
        a, b, c = A.to_evaluations(), B.to_evaluations(), C.to_evaluations()
        check_sampled(a, b, c, n, p, np.random.default_rng(n))
        for seed in (11, 12):
            check_identity(pkg, ctx, n, a, b, C, p, seed)


# ---- the accumulator bound ---------------------------------------------------------------------------------------

def const_table(pkg, ctx, nv, word):
    import torch
    t = torch.full((1 << nv,), word - (1 << 64) if word >= 1 << 63 else word, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return pkg.DenseMultilinearExtension.from_device(ctx, t.data_ptr(), nv, keep=t)


@pytest.mark.parametrize("p,wa,wb", [(P59, 0, 0), (P59, P59 - 1, P59 - 1), (P59, 0, P59 - 1), (GOLD, GOLD - 1, GOLD - 1)],
                         ids=["p64m59-zero-bytes", "p64m59-ff-bytes", "p64m59-zero-x-ff", "gold-pm1"])
def test_accumulator_limit_n14(p, wa, wb):
    """n = 14: the contraction (2^14) crosses the int32 run bound (kMatmulRunSteps * 64 = 16320).  All-zero bytes
    (s = -128 on both sides) make every byte product 2^14, the largest; a run of 2^14 would reach exactly 2^31."""
    pkg = load_package()
    n = 14
    ctx = ctx_for(pkg, p)
    ctx.set_option("time_kernels", 1)
    A, B = const_table(pkg, ctx, 2 * n, wa), const_table(pkg, ctx, 2 * n, wb)
    C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
    log = [r for r in ctx.launch_log() if r["kind"] == "matmul"]
    assert [r["kf"] for r in log] == [0, 1]   # the repack, then the matrix-core kernel
    want = (1 << n) * wa * wb * pow(R, -1, p) % p
    c = C.to_evaluations()
    assert np.all(c == np.uint64(want)), (int(c[0]), want, int(np.count_nonzero(c != np.uint64(want))))
    # the identity: the MLE of a constant matrix is the constant; G::new of constant matrices is constant too
    F = ctx.field
    pt = pkg.matrix_multiplication.product_point(F, n, 5)
    assert pkg.matrix_multiplication.product_claim(C, pt) == want
    g = pkg.matrix_multiplication.G.new_from_tables(ctx, n, A, B, pt)
    assert g.hypercube_sum() == want


# ---- the protocol ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P59, 389], ids=pid)
def test_prove_verify_product(p):
    pkg = load_package()
    mm = pkg.matrix_multiplication
    rng = np.random.default_rng(p % 991)
    ctx = ctx_for(pkg, p)
    F = ctx.field
    for n in range(1, 9):
        a = rng.integers(0, p, size=1 << (2 * n), dtype=np.uint64)
        b = rng.integers(0, p, size=1 << (2 * n), dtype=np.uint64)
        A = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, a)
        B = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, b)
        proof = mm.prove_product(ctx, n, A, B, seed_r=1000 + n, seed_pt=2000 + n)
        assert proof.c_1 == proof.claim, n
        assert mm.verify_product(ctx, n, A, B, proof.C, proof), n
        # the transcript is pyref's on G at the same point and challenges (canonical ints)
        if n <= 7:
            ac, bc = F.to_ints(a), F.to_ints(b)
            fa, fb = pyref.g_new(n, ac, bc, F.to_ints(proof.point), p)
            ref = pyref.transcript(fa, fb, F.to_ints(proof.challenges), p)
            assert F.to_int(proof.c_1) == ref["c_1"], n
            assert [F.to_ints(e) for e in proof.evals] == [list(e) for e in ref["evals"]], n
        # one wrong entry of C: the verifier rejects
        c = proof.C.to_evaluations()
        i = int(rng.integers(0, c.size))
        c[i] = (int(c[i]) + 1) % p
        bad = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, c)
        assert not mm.verify_product(ctx, n, A, B, bad, proof), n
        proof_bad = mm.prove_product(ctx, n, A, B, C=bad, seed_r=1000 + n, seed_pt=2000 + n)
        assert proof_bad.c_1 != proof_bad.claim
        assert not mm.verify_product(ctx, n, A, B, bad, proof_bad), n


# ---- plumbing --------------------------------------------------------------------------------------------------------

def expect(pkg, code, fn, *needles):
    with pytest.raises(pkg.SumcheckHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for s in needles:
        assert s in str(ei.value), (s, str(ei.value))


def test_refusals():
    pkg = load_package()
    lib = pkg.load()
    ctx = ctx_for(pkg, GOLD)
    F = ctx.field
    out = ctypes.c_void_p()
    A = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 4, F.from_ints(range(16)))
    B = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 4, F.from_ints(range(16)))
    assert lib.sc_matmul(None, A.h, B.h, 2, ctypes.byref(out)) == 1
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, A.h, B.h, 2, None)))
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, None, B.h, 2, ctypes.byref(out))), "null")
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, A.h, None, 2, ctypes.byref(out))), "null")
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, A.h, B.h, 1, ctypes.byref(out))), "2^(2n)")
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, A.h, B.h, 3, ctypes.byref(out))), "2^(2n)")
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, A.h, B.h, 15, ctypes.byref(out))), "at most 2^14")
    B8 = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 3, F.from_ints(range(8)))
    expect(pkg, 1, lambda: ctx.check(lib.sc_matmul(ctx.h, A.h, B8.h, 2, ctypes.byref(out))), "differ")
    expect(pkg, 1, lambda: ctx.set_option("matmul_path", 3), "matmul_path")
    assert ctx.get_option("matmul_path") == 0
    # a multi-device handle and a sharded context
    m = pkg.Context(pkg.Field(GOLD), devices=[0, 0])
    mA = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: pkg.matrix_multiplication.matmul(m, 2, mA, mA), "multi-device")
    del mA
    m.close()
    sh = pkg.Context(pkg.Field(GOLD))
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    sA = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, F.from_ints(range(16)))
    expect(pkg, 6, lambda: pkg.matrix_multiplication.matmul(sh, 2, sA, sA), "sharded")
    # the context still works
    C = pkg.matrix_multiplication.matmul(ctx, 2, A, B)
    want = exact_words(A.to_evaluations(), B.to_evaluations(), 2, GOLD)
    assert np.array_equal(C.to_evaluations(), want)


@pytest.mark.parametrize("n,path,kinds", [(3, "auto", [3]), (4, "auto", [3]), (4, "mfma", [0, 1]), (5, "auto", [0, 1]),
                                          (6, "valu", [2]), (10, "auto", [0, 1]), (10, "valu", [2])])
def test_launch_log(n, path, kinds):
    pkg = load_package()
    ctx = ctx_for(pkg, GOLD, path)
    ctx.set_option("time_kernels", 1)
    A = pkg.DenseMultilinearExtension.generate(ctx, 1, 2 * n)
    B = pkg.DenseMultilinearExtension.generate(ctx, 2, 2 * n)
    ctx.launch_log()
    pkg.matrix_multiplication.matmul(ctx, n, A, B)
    log = [r for r in ctx.launch_log() if r["kind"] == "matmul"]
    assert [r["kf"] for r in log] == kinds
    names = [pkg._lib.MATMUL_KERNELS[r["kf"]] for r in log]
    if n >= 5 and path == "auto":
        assert "matmul_mfma_kernel" in names
    N = 1 << n
    for r in log:
        assert r["ks"] == n and r["log_in"] == 2 * n and r["ms"] >= 0
        assert r["bytes_read"] >= 8 * N * N and r["bytes_written"] >= 8 * N * N


def test_pool_reuse():
    import torch
    pkg = load_package()
    n = 10
    ctx = ctx_for(pkg, GOLD)
    A = pkg.DenseMultilinearExtension.generate(ctx, 1, 2 * n)
    B = pkg.DenseMultilinearExtension.generate(ctx, 2, 2 * n)
    first = pkg.matrix_multiplication.matmul(ctx, n, A, B).to_evaluations()
    ctx.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    for _ in range(20):
        C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
        del C
    ctx.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    assert free1 >= free0, (free0, free1)
    assert np.array_equal(pkg.matrix_multiplication.matmul(ctx, n, A, B).to_evaluations(), first)
