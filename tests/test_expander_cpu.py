"""CPU-only: "expander code 1" (DESIGN.md section 9 item 10).  The reference (tests/expander_ref.py) and the package's host
encoder (thaler-study_amd/expander_code.py) against the contract's known answers; the properties the code is built on
(bijections, systematic, linear, the base code's distance); the kernel's own work items (csrc/kernels/expander.hpp, compiled
for the host) against the reference; and the host Verifier(code="expander") against a reference prover over 2^64 - 59."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import expander_ref as ref
import ligero_ref
from conftest import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = 2**64 - 2**32 + 1
P59 = 2**64 - 59
R64 = 2**64
u64p = ctypes.POINTER(ctypes.c_uint64)

# (p, c) -> (E[m], E[2m-1], sha256 over le64 of the canonical codeword) for x[i] = (3 i + 1) mod p
KNOWN = {
    (P59, 4): (7395231923899982794, 3652597681181791053, "4b277083b25a4399569ae6db66e0b15558df5dfdd7e8882698c34b528afb2c01"),
    (P59, 6): (11824905255871736527, 5620255610937501912, "3d392fa5182a9d718bc3794052a122c4a3fce96ece5e0047c060b07ed8f72ea9"),
    (P59, 7): (8122078464881165495, 17614333150964371419, "c45e3f94d1bb64d61518a687d4cbed214d3f4ea1d08cab6c469e364cb3950ba3"),
    (GOLD, 4): (14058706139638006544, 678301629074156362, "eef1afa075f8e55dae34de20a6228917763263665a03c12c2182e5659220347e"),
    (GOLD, 6): (11824910774904634787, 3450943385730609239, "ed77c9c265e82af0220b86e899a6b19da67eec092c8e940b117671b73b018021"),
    (GOLD, 7): (8122090984710658435, 15038129331883664520, "3813cd596ed82981e95197a3c3d6e4c3145bc679091485b9950005d84da98afb"),
    (257, 4): (161, 176, "1e1b9a213b1b99798f4b1f2260b87d4b697aee2c8877cc803e23cb252c1eacc1"),
    (257, 6): (12, 70, "c80512e5d5fc2b61f5855174058a1395462e7cb208654917cb72006d78c9e214"),
    (257, 7): (214, 110, "917cd135a05d5355063172e2b137e8757cdd5373744d24e809ec8db28d1e9a3c"),
}


@pytest.fixture(scope="module")
def xc():
    return load_package().expander_code


@pytest.fixture(scope="module")
def xh(tmp_path_factory):
    out = tmp_path_factory.mktemp("xh") / "libexpander_host.so"
    src = os.path.join(ROOT, "tests", "cpp", "expander_host_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), src])
    lib = ctypes.CDLL(str(out))
    lib.xh_key.argtypes = [ctypes.c_int] * 3
    lib.xh_key.restype = ctypes.c_uint64
    lib.xh_perm.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32]
    lib.xh_perm.restype = ctypes.c_uint32
    lib.xh_coef.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32]
    lib.xh_coef.restype = ctypes.c_uint64
    lib.xh_to_mont.argtypes = [ctypes.c_uint64, ctypes.c_int, u64p, u64p, ctypes.c_size_t]
    lib.xh_levels.argtypes = [ctypes.c_int]
    lib.xh_tile_log.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.xh_encode_rows.argtypes = [ctypes.c_uint64, ctypes.c_int, u64p, u64p, ctypes.c_int, ctypes.c_int, u64p]
    return lib


def mont(p, xs):
    return [int(x) * R64 % p for x in xs]


# ---- the contract's constants ----------------------------------------------------------------------------------------

def test_anchors(xc):
    for m in (ref, xc):
        K = m.key(6, 0, 0)
        assert K == 0xdd4b0ea0580c93d9 and m.key(7, 1, 3) == 0x0abecaa87c3df268
        assert [m.perm(K, 6, i) for i in range(8)] == [9, 49, 27, 10, 11, 40, 0, 35]
        assert m.coef(K, 0, P59) == 9412594181706461107 and m.coef(K, 5, 257) == 128
        assert (m.SEED, m.GOLDEN, m.D_A, m.D_B) == (0x4272616B65646F77, 0x9E3779B97F4A7C15, 8, 16)


@pytest.mark.parametrize("p,c", sorted(KNOWN), ids=lambda v: str(v))
def test_known_answers(pkg, xc, p, c):
    m = 1 << c
    x = [(3 * i + 1) % p for i in range(m)]
    E = ref.encode(x, p)
    assert (E[m], E[2 * m - 1], ref.digest_of(E)) == KNOWN[(p, c)]
    F = pkg.Field(p)
    assert xc.encode(F, mont(p, x)) == mont(p, E)


@pytest.mark.parametrize("p", [P59, GOLD, 2013265921, 257])
def test_host_encoder_equals_the_reference(pkg, xc, p):
    F = pkg.Field(p)
    rng = random.Random(p)
    for c in list(range(0, 10)) + [11]:
        x = [rng.randrange(p) for _ in range(1 << c)]
        assert xc.encode(F, mont(p, x)) == mont(p, ref.encode(x, p)), (p, c)
    with pytest.raises(ValueError):
        xc.encode(F, [0] * 3)
    with pytest.raises(ValueError):
        xc.encode(pkg.Field(5), [0] * 4)


# ---- what the code is built on ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("lm", range(6, 14))
def test_every_permutation_in_use_is_a_bijection(lm):
    for side, deg, b in ((0, ref.D_A, lm), (1, ref.D_B, lm - 1)):
        for t in range(deg):
            K = ref.key(lm, side, t)
            assert sorted(ref.perm(K, b, i) for i in range(1 << b)) == list(range(1 << b)), (lm, side, t)


@pytest.mark.parametrize("p", [P59, 257])
def test_every_input_is_used_exactly_d_times(p):
    for lm in (6, 7, 9):
        A, B = ref.level_maps(lm, p)
        assert all(len(terms) == 4 * ref.D_A for terms in A) and all(len(terms) == ref.D_B for terms in B)
        for gathers, size, deg in ((A, 1 << lm, ref.D_A), (B, 1 << (lm - 1), ref.D_B)):
            used = [0] * size
            for terms in gathers:
                for a, i in terms:
                    assert 1 <= a < p
                    used[i] += 1
            assert used == [deg] * size, (p, lm)


@pytest.mark.parametrize("p", [P59, GOLD, 257])
def test_systematic_and_linear(p):
    rng = random.Random(3)
    for c in (0, 3, 5, 6, 7, 8, 9):
        m = 1 << c
        x, y, a = [rng.randrange(p) for _ in range(m)], [rng.randrange(p) for _ in range(m)], rng.randrange(p)
        Ex, Ey = ref.encode(x, p), ref.encode(y, p)
        assert len(Ex) == 2 * m and Ex[:m] == x
        assert ref.encode([(a * s + t) % p for s, t in zip(x, y)], p) == [(a * s + t) % p for s, t in zip(Ex, Ey)], (p, c)
        assert ref.encode([0] * m, p) == [0] * (2 * m)


def test_layout_is_the_contracts(xc):
    """Enc_m = x || Enc_(m/4)(y) || v: the recursion's pieces sit where the in-place layout says"""
    p = P59
    rng = random.Random(11)
    x = [rng.randrange(p) for _ in range(256)]
    E = ref.encode(x, p)
    A, B = ref.level_maps(8, p)
    y = [sum(a * x[i] for a, i in terms) % p for terms in A]
    assert E[256:256 + 64] == y and E[256:384] == ref.encode(y, p)
    assert E[384:] == [sum(a * E[256 + i] for a, i in terms) % p for terms in B]
    K = ref.base_matrix(16, p)
    y2 = E[256 + 64:256 + 64 + 16]                         # the second level's y, the base code's message
    assert E[256 + 64 + 16:256 + 64 + 32] == [sum(K[j][k] * y2[k] for k in range(16)) % p for j in range(16)]


def test_base_code_distance():
    """m = 2, p = 67: every nonzero message has codeword weight >= 3 = m + 1 (MDS)"""
    p = 67
    for x in itertools.product(range(p), repeat=2):
        if any(x):
            assert sum(1 for v in ref.encode(list(x), p) if v) >= 3, x


# ---- the kernel's code on the host -----------------------------------------------------------------------------------

def test_device_hashes_on_the_host(xh):
    rng = random.Random(5)
    for lm in range(6, 14):
        for side, deg, b in ((0, 8, lm), (1, 16, lm - 1)):
            for t in range(deg):
                K = ref.key(lm, side, t)
                assert xh.xh_key(lm, side, t) == K
                for i in [0, 1, (1 << b) - 1] + [rng.randrange(1 << b) for _ in range(32)]:
                    assert xh.xh_perm(K, b, i) == ref.perm(K, b, i), (lm, side, t, i)
                    for p, gold in ((P59, 0), (257, 0), (2013265921, 0), (GOLD, 0), (GOLD, 1)):
                        assert xh.xh_coef(p, gold, K, i) == ref.coef(K, i, p) * R64 % p
    assert [xh.xh_levels(c) for c in range(14)] == [0] * 6 + [1, 1, 2, 2, 3, 3, 4, 4]
    assert [xh.xh_tile_log(c + 1, n + 1) for c, n in ((0, 0), (5, 8), (5, 13), (10, 12), (11, 11), (13, 20))] == [1, 9, 12, 12, 12, 14]


@pytest.mark.parametrize("p,gold", [(P59, 0), (2**63 + 29, 0), (257, 0), (GOLD, 0), (GOLD, 1)])
def test_to_mont_accepts_an_unreduced_word(xh, p, gold):
    """coef hands to_mont the raw 64-bit hash: words up to 2^64 - 1, not residues"""
    rng = random.Random(9)
    words = [0, 1, p - 1, p, p + 1, 2 * p % R64, R64 - 1, R64 - 2, 2**63, 2**32 - 1, 2**32, 0xFFFFFFFF00000000]
    words += [k * p for k in range(2, 9) if k * p < R64] + [rng.randrange(R64) for _ in range(20000)]
    a = np.array(words, dtype=np.uint64)
    out = np.empty_like(a)
    xh.xh_to_mont(p, gold, a.ctypes.data_as(u64p), out.ctypes.data_as(u64p), a.size)
    assert [int(v) for v in out] == [w * R64 % p for w in words]


@pytest.mark.parametrize("p,gold", [(P59, 0), (257, 0), (GOLD, 1)])
def test_kernel_work_items_on_the_host(xh, p, gold):
    """the kernel's three kinds of work item, run tile by tile on the CPU: one row per tile, several, every recursion depth"""
    rng = random.Random(13)
    inv = np.array([0] + [pow(s, -1, p) * R64 % p for s in range(1, 64)], dtype=np.uint64)
    for n, c in [(0, 0), (3, 0), (5, 5), (13, 5), (8, 6), (9, 7), (12, 8), (10, 9), (10, 10), (12, 11), (13, 12), (13, 13)]:
        table = [rng.randrange(p) for _ in range(1 << n)]
        if (n, c) == (13, 5):
            table = [p - 1] * (1 << n)
        w = np.array(mont(p, table), dtype=np.uint64)
        E = np.zeros(2 << n, dtype=np.uint64)
        xh.xh_encode_rows(p, gold, w.ctypes.data_as(u64p), inv.ctypes.data_as(u64p), n, c, E.ctypes.data_as(u64p))
        want = [v for row in ref.encode_rows(table, c, p) for v in row]
        assert [int(v) for v in E] == mont(p, want), (p, n, c)


# ---- the host verifier -----------------------------------------------------------------------------------------------

def run_protocol(pkg, p, n, c, queries, seed, tamper=None):
    """test_ligero_cpu.run_protocol over the expander code"""
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    rng = random.Random(seed)
    table = [rng.randrange(p) for _ in range(1 << n)]
    prover = ref.RefProver(table, c, p)
    root = prover.root()
    if tamper == "root":
        root = bytes([root[0] ^ 1]) + root[1:]
    v = lp.Verifier(F, n, c, 1, root, queries, code="expander")
    gamma = v.draw_gamma(rng)
    point = [F.rand(rng) for _ in range(n)]
    u_gamma, u_z = prover.combine(ligero_ref.canon(p, point), ligero_ref.canon(p, gamma))
    u_gamma, u_z = mont(p, u_gamma), mont(p, u_z)
    if tamper == "u_z":
        u_z[len(u_z) // 2] = F.add(u_z[len(u_z) // 2], F.one)
    if tamper == "u_gamma":
        u_gamma[0] = F.add(u_gamma[0], F.one)
    v.receive(u_gamma, u_z)
    cols = v.draw_columns(rng)
    openings = [(j, mont(p, vals), lp.ColumnPath(j, sib, F)) for j, vals, sib in prover.open_columns(cols)]
    if tamper == "column":
        j, vals, path = openings[3]
        openings[3] = (j, [F.add(vals[0], F.one)] + vals[1:], path)
    if tamper == "path":
        j, vals, path = openings[5]
        sib = list(path.siblings)
        sib[-1] = bytes(32)
        openings[5] = (j, vals, lp.ColumnPath(j, sib, F))
    value = v.verify(point, openings)
    return value, F.from_int(ligero_ref.mle_eval(table, ligero_ref.canon(p, point), p))


@pytest.mark.parametrize("n,c", [(6, 3), (9, 6), (7, 7), (5, 0)])
def test_verifier_accepts_the_reference_prover(pkg, n, c):
    value, want = run_protocol(pkg, P59, n, c, 16, 100 * n + c)
    assert value == want


@pytest.mark.parametrize("n,c", [(6, 3), (9, 6)])
def test_tampering_is_caught(pkg, n, c):
    lp = pkg.ligero_pcs
    for tamper, err in (("u_z", lp.EvalMismatch), ("u_gamma", lp.ProximityMismatch), ("column", lp.MerkleMismatch),
                        ("path", lp.MerkleMismatch), ("root", lp.MerkleMismatch)):
        with pytest.raises(err):
            run_protocol(pkg, P59, n, c, 16, 31, tamper=tamper)


def test_verifier_arguments(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(P59)
    with pytest.raises(ValueError):
        lp.Verifier(F, 6, 3, 2, bytes(32), 16, code="expander")
    with pytest.raises(ValueError):
        lp.Verifier(F, 6, 3, 1, bytes(32), 16, code="ldpc")
    with pytest.raises(ValueError):
        lp.Verifier(F, 6, 3, 1, bytes(32), 16)              # the default code is Reed-Solomon: 2^64 - 59 has no root of order 16
    assert lp.default_log_cols(28, 1, "expander") == 13 and lp.default_log_cols(9, 1, "expander") == 5
    assert lp.default_log_cols(28, 1) == 13 and lp.default_log_cols(28, 2) == 12
    assert lp.CODES == {"rs": 0, "expander": 1}
