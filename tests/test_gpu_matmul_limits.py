"""sc_matmul at its design limits: n = 14 on random data (the only size whose contraction takes a second int32 run), n = 14
on patterns where the two runs contribute different, known amounts (a second run that read the wrong K offset gives a wrong
C), the sizes the other tests skip (n = 8, 9, 11 on every path), edge words at large n and the VALU path at n = 13 and 14.
Every product is checked exactly: a full product or sampled entries by exact integer arithmetic, and the identity
f~_C(r1, r2) = c_1 of G::new, which over a large field checks every entry with high probability."""
import numpy as np
import pytest

from conftest import load_package
from test_gpu_matmul import P59, R, check_identity, ctx_for, sample_positions
from util import GOLD, oracle, pid, pyref
from wide_words import WIDE, edge_table, wid

pytestmark = pytest.mark.gpu

P32M5 = 2**32 - 5
RUN_Y = 255 * 64   # y of the first int32 run at n = 14 (kMatmulRunSteps MFMA steps of 64, kernels/matmul.hpp)


# ---- exact references on the host ---------------------------------------------------------------------------------

def _limbs(x):
    """the four 16-bit limbs of uint64 words as float64 (a limb product summed over 2^14 terms stays below 2^46: exact)"""
    x = np.asarray(x, dtype=np.uint64)
    return [((x >> np.uint64(16 * l)) & np.uint64(0xFFFF)).astype(np.float64) for l in range(4)]


def _combine(diag, p):
    """(sum_d 2^(16d) T_d) R^-1 mod p, entrywise, from the seven exact diagonal sums T_d (float64 arrays, < 2^53)"""
    rinv = pow(R, -1, p)
    total = 0
    for d, t in enumerate(diag):
        total = total + (t.astype(np.uint64).astype(object) << (16 * d))
    return np.array([int(v) * rinv % p for v in np.ravel(total)], dtype=np.uint64).reshape(np.shape(diag[0]))


def exact_block(a_rows, b_cols, p):
    """the Montgomery words of a_rows (S x K) times b_cols (K x T), exactly: limb GEMMs in float64"""
    la, lb = _limbs(a_rows), _limbs(b_cols)
    diag = [np.zeros((a_rows.shape[0], b_cols.shape[1])) for _ in range(7)]
    for i in range(4):
        for j in range(4):
            diag[i + j] += la[i] @ lb[j]
    return _combine(diag, p)


def exact_pairs(a_rows, b_cols, p):
    """entry s is the Montgomery word of a_rows[s] . b_cols[s] (both S x K), exactly"""
    la, lb = _limbs(a_rows), _limbs(b_cols)
    diag = [np.zeros(a_rows.shape[0]) for _ in range(7)]
    for i in range(4):
        for j in range(4):
            diag[i + j] += np.einsum("sk,sk->s", la[i], lb[j])
    return _combine(diag, p)


def check_entries(a, b, c, n, p, pos):
    N = 1 << n
    A, B, C = a.reshape(N, N), b.reshape(N, N), c.reshape(N, N)
    rows = np.array([i for i, _ in pos])
    cols = np.array([j for _, j in pos])
    want = exact_pairs(A[rows], B[:, cols].T, p)
    got = C[rows, cols]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (n, p, len(bad), pos[int(bad[0])] if bad.size else None)


def check_sampled(a, b, c, n, p, seed, count=256):
    check_entries(a, b, c, n, p, sample_positions(n, np.random.default_rng(seed), count))


def check_identity_device(pkg, ctx, n, A, B, C, seeds=(21, 22, 23)):
    """f~_C(r1, r2) == c_1 of G::new(A, B, (r1, r2)) built on the device from A and B (sc_matmul_g_new, not the product)"""
    mm = pkg.matrix_multiplication
    for s in seeds:
        pt = mm.product_point(ctx.field, n, s)
        g = mm.G.new_from_tables(ctx, n, A, B, pt)
        assert mm.product_claim(C, pt) == g.hypercube_sum(), (n, s)


def big_edge_table(p, size, rng):
    """edge_table of any size: above 2^24 entries, copies of one 2^24-entry edge table, each rotated by its own offset"""
    m = 1 << 24
    if size <= m:
        return edge_table(p, size, rng)
    base = edge_table(p, m, rng)
    out = np.empty(size, dtype=np.uint64)
    for k in range(size // m):
        out[k * m:(k + 1) * m] = np.roll(base, int(rng.integers(0, m)))
    return out


def test_exact_references_agree_with_pyref():
    """the limb-GEMM references above against pyref's big-integer product (host only; the GPU tests lean on them)"""
    rng = np.random.default_rng(3)
    for p in (GOLD, P59, P32M5, 389):
        for n in (0, 1, 3, 5):
            N = 1 << n
            a = rng.integers(0, p, size=N * N, dtype=np.uint64)
            b = rng.integers(0, p, size=N * N, dtype=np.uint64)
            rinv = pow(R, -1, p)
            C = pyref.matmul([[int(x) for x in a[i * N:(i + 1) * N]] for i in range(N)],
                             [[int(x) for x in b[i * N:(i + 1) * N]] for i in range(N)], p)
            want = np.array([c * rinv % p for row in C for c in row], dtype=np.uint64)
            assert np.array_equal(exact_block(a.reshape(N, N), b.reshape(N, N), p).ravel(), want), (p, n)
            pos = [(i, j) for i in range(N) for j in range(N)]
            got = exact_pairs(a.reshape(N, N)[[i for i, _ in pos]], b.reshape(N, N)[:, [j for _, j in pos]].T, p)
            assert np.array_equal(got, want), (p, n)


# ---- n = 14: two accumulator runs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P59, P32M5], ids=wid)
def test_n14_random_matrix_cores(p):
    pkg = load_package()
    n = 14
    ctx = ctx_for(pkg, p, "mfma")
    A = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A + 140, 2 * n)
    B = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_B + 140, 2 * n)
    C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
    check_identity_device(pkg, ctx, n, A, B, C)
    a, b, c = A.to_evaluations(), B.to_evaluations(), C.to_evaluations()
    check_sampled(a, b, c, n, p, 14)


def _run_pattern(p, where, rng):
    """A and B of zero words (every byte s = -128: the int32 bound's worst case) except 64 columns of A and the mirroring
    64 rows of B, which hold random words: the last 64 (the second run's y) or the first 64 (the first run's y, before 16256
    worst-case ones).  C = A[:, S] B[S, :] exactly, S the 64 special indices."""
    N = 1 << 14
    sl = slice(N - 64, N) if where == "tail" else slice(0, 64)
    a = np.zeros(N * N, dtype=np.uint64)
    b = np.zeros(N * N, dtype=np.uint64)
    a_s = rng.integers(0, p, size=(N, 64), dtype=np.uint64)
    b_s = rng.integers(0, p, size=(64, N), dtype=np.uint64)
    a.reshape(N, N)[:, sl] = a_s
    b.reshape(N, N)[sl, :] = b_s
    return a, b, a_s, b_s


@pytest.mark.parametrize("where,p", [("tail", GOLD), ("tail", P32M5), ("head", P59), ("head", GOLD)],
                         ids=lambda v: v if isinstance(v, str) else wid(v))
def test_n14_run_boundary_patterns(where, p):
    pkg = load_package()
    n, N = 14, 1 << 14
    assert RUN_Y < N < 2 * RUN_Y   # two runs: the first of RUN_Y y, the second of N - RUN_Y = 64
    rng = np.random.default_rng(0xB0 + p % 1000 + (where == "head"))
    a, b, a_s, b_s = _run_pattern(p, where, rng)
    ctx = ctx_for(pkg, p, "mfma")
    ctx.set_option("time_kernels", 1)
    A = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, a)
    B = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, b)
    del a, b
    ctx.launch_log()
    C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
    assert [r["kf"] for r in ctx.launch_log() if r["kind"] == "matmul"] == [0, 1]   # the matrix-core kernel ran
    c = C.to_evaluations().reshape(N, N)
    # whole rows and columns
    rows = [0, 15, 16, 4097, N - 1, int(rng.integers(0, N))]
    cols = [0, 15, 16, 8191, N - 1, int(rng.integers(0, N))]
    bad = np.argwhere(c[rows] != exact_block(a_s[rows], b_s, p))
    assert bad.size == 0, ("rows", [(rows[i], int(j)) for i, j in bad[:4]])
    bad = np.argwhere(c[:, cols] != exact_block(a_s, b_s[:, cols], p))
    assert bad.size == 0, ("cols", [(int(i), cols[j]) for i, j in bad[:4]])
    # thousands of entries
    rows = rng.integers(0, N, 4096)
    cols = rng.integers(0, N, 4096)
    want = exact_pairs(a_s[rows], b_s[:, cols].T, p)
    assert np.array_equal(c[rows, cols], want), int(np.count_nonzero(c[rows, cols] != want))
    del c
    check_identity_device(pkg, ctx, n, A, B, C, seeds=(31, 32))


# ---- sizes no other test checks directly ----------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD, P59, P32M5, 389], ids=wid)
@pytest.mark.parametrize("n", [8, 9, 11])
def test_unchecked_sizes_every_path(n, p):
    pkg = load_package()
    rng = np.random.default_rng(100 * n + p % 97)
    N = 1 << n
    a = rng.integers(0, p, size=N * N, dtype=np.uint64)
    b = rng.integers(0, p, size=N * N, dtype=np.uint64)
    want = exact_block(a.reshape(N, N), b.reshape(N, N), p).ravel() if n <= 9 else None
    for path in ("auto", "mfma", "valu"):
        ctx = ctx_for(pkg, p, path)
        ctx.set_option("time_kernels", 1)
        A = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, a)
        B = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, b)
        ctx.launch_log()
        C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
        kinds = [r["kf"] for r in ctx.launch_log() if r["kind"] == "matmul"]
        assert kinds == ([2] if path == "valu" else [0, 1]), (path, kinds)
        c = C.to_evaluations()
        if want is not None:
            assert np.array_equal(c, want), (n, path, int(np.argmax(c != want)))
        else:
            check_sampled(a, b, c, n, p, n)
            check_identity(pkg, ctx, n, a, b, C, p, 41)
            check_identity(pkg, ctx, n, a, b, C, p, 42)


# ---- edge words at large n ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [GOLD] + WIDE, ids=wid)
@pytest.mark.parametrize("n", [8, 10, 13, 14])
def test_edge_words_large_n(n, p):
    """the words where the field arithmetic carries, on the matrix-core path: the 192-bit epilogue (wide_get) on every
    modulus at sizes up to the two-run one"""
    pkg = load_package()
    rng = np.random.default_rng(1000 * n + p % 991)
    N = 1 << n
    a, b = big_edge_table(p, N * N, rng), big_edge_table(p, N * N, rng)
    ctx = ctx_for(pkg, p, "mfma")
    A = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, a)
    B = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, b)
    C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
    c = C.to_evaluations()
    if n <= 8:
        assert np.array_equal(c, exact_block(a.reshape(N, N), b.reshape(N, N), p).ravel())
    else:
        check_sampled(a, b, c, n, p, n)
    del c
    if n <= 11:
        check_identity(pkg, ctx, n, a, b, C, p, 51)
        check_identity(pkg, ctx, n, a, b, C, p, 52)
    else:
        check_identity_device(pkg, ctx, n, A, B, C, seeds=(51, 52))


# ---- the VALU path at the largest sizes -----------------------------------------------------------------------------

@pytest.mark.parametrize("n,p", [(13, GOLD), (13, P59), (14, GOLD)], ids=lambda v: str(v) if isinstance(v, int) and v < 64 else pid(v))
def test_valu_large(n, p):
    pkg = load_package()
    ctx = ctx_for(pkg, p, "valu")
    ctx.set_option("time_kernels", 1)
    A = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A + 7 * n, 2 * n)
    B = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_B + 7 * n, 2 * n)
    ctx.launch_log()
    C = pkg.matrix_multiplication.matmul(ctx, n, A, B)
    assert [r["kf"] for r in ctx.launch_log() if r["kind"] == "matmul"] == [2]   # matmul_tiled_kernel
    check_identity_device(pkg, ctx, n, A, B, C, seeds=(61, 62))
    check_sampled(A.to_evaluations(), B.to_evaluations(), C.to_evaluations(), n, p, 60 + n)
