"""CPU checks of the Relaxed PCS (relaxed-pcs/src/lib.rs): the shared SHA-256 compression of kernels/sha256.hpp and the host half of
an opening (kernels/merkle.hpp) compiled with g++ against hashlib, the reference's grid order, the host verifier against paths built here with hashlib, and the built ISA of the
hash kernels.  No GPU needed."""
import ctypes
import hashlib
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_package

CSRC = os.path.join(ROOT, "thaler-study_amd", "csrc")
GOLD = 2**64 - 2**32 + 1
P59 = 2**64 - 59
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    out = tmp_path_factory.mktemp("ph") / "libpcs_host.so"
    src = os.path.join(ROOT, "tests", "cpp", "pcs_host_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), src])
    lib = ctypes.CDLL(str(out))
    lib.ph_leaf.argtypes = [u64p, u32p, ctypes.c_size_t]
    lib.ph_node.argtypes = [u32p, u32p, u32p]
    lib.ph_root.argtypes = [u64p, ctypes.c_int, u32p, ctypes.POINTER(ctypes.c_double)]
    lib.ph_level_offset.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.ph_level_offset.restype = ctypes.c_uint64
    lib.ph_path.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, u64p, u32p, u64p, ctypes.POINTER(ctypes.c_uint8)]
    return lib


def words_to_bytes(w):
    return b"".join(int(x).to_bytes(4, "big") for x in w)


def bytes_to_words(b):
    return np.array([int.from_bytes(b[4 * k:4 * k + 4], "big") for k in range(8)], dtype=np.uint32)


def leaf_hl(v):
    return hashlib.sha256(int(v).to_bytes(8, "little")).digest()


def node_hl(l, r):
    return hashlib.sha256(l + r).digest()


def root_hl(values):
    lev = [leaf_hl(v) for v in values]
    while len(lev) > 1:
        lev = [node_hl(lev[2 * k], lev[2 * k + 1]) for k in range(len(lev) // 2)]
    return lev[0]


def levels_hl(values):
    """every level of the tree, leaves first"""
    levels = [[leaf_hl(v) for v in values]]
    while len(levels[-1]) > 1:
        lev = levels[-1]
        levels.append([node_hl(lev[2 * k], lev[2 * k + 1]) for k in range(len(lev) // 2)])
    return levels


def path_hl(values, i, levels=None):
    """the siblings of leaf i, bottom up (`levels`: levels_hl(values), where a caller opens many leaves of one tree)"""
    levels = levels or levels_hl(values)
    return [lev[(i >> l) ^ 1] for l, lev in enumerate(levels[:-1])]


def edge_values():
    vals = {0, 1, 2, 0xFF, 0x100, 0xFFFFFFFF, 2**32, 2**32 + 1, 0x0123456789ABCDEF, GOLD - 1, P59 - 1, 2**63, 2**64 - 1}
    rng = random.Random(7)
    vals |= {rng.getrandbits(64) for _ in range(40)}
    return sorted(vals)


def test_leaf_digest_is_sha256_of_le64(ph):
    vals = edge_values()
    a = np.array(vals, dtype=np.uint64)
    out = np.zeros(8 * len(vals), dtype=np.uint32)
    ph.ph_leaf(a.ctypes.data_as(u64p), out.ctypes.data_as(u32p), len(vals))
    for k, v in enumerate(vals):
        assert words_to_bytes(out[8 * k:8 * k + 8]) == leaf_hl(v), hex(v)
    # values >= 2^32 catch a swapped word order, values with distinct bytes a missing byte swap
    assert leaf_hl(2**32) != leaf_hl(1)


def test_node_digest_is_sha256_of_the_concatenation(ph):
    rng = random.Random(11)
    for _ in range(50):
        l, r = rng.randbytes(32), rng.randbytes(32)
        out = np.zeros(8, dtype=np.uint32)
        lw, rw = bytes_to_words(l), bytes_to_words(r)
        ph.ph_node(lw.ctypes.data_as(u32p), rw.ctypes.data_as(u32p), out.ctypes.data_as(u32p))
        assert words_to_bytes(out) == node_hl(l, r)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 10])
def test_host_tree_root_matches_hashlib(ph, n):
    rng = random.Random(n)
    vals = np.array([rng.getrandbits(64) for _ in range(1 << n)], dtype=np.uint64)
    root = np.zeros(8, dtype=np.uint32)
    secs = ctypes.c_double()
    ph.ph_root(vals.ctypes.data_as(u64p), n, root.ctypes.data_as(u32p), ctypes.byref(secs))
    assert words_to_bytes(root) == root_hl([int(v) for v in vals])


@pytest.mark.parametrize("log_bottom", range(7))
def test_level_offset_is_the_running_sum_of_the_level_sizes(ph, log_bottom):
    B = 1 << log_bottom
    for l in range(log_bottom + 1):
        assert ph.ph_level_offset(B, l) == sum(B >> k for k in range(l)), l
    assert ph.ph_level_offset(B, log_bottom) == 2 * B - 2


@pytest.mark.parametrize("n,lb", [(0, 0), (1, 1), (3, 3), (4, 4), (5, 4), (7, 4), (9, 4)])
def test_host_opening_matches_hashlib_at_every_leaf(ph, n, lb):
    """merkle_path_host rebuilds the levels below lb from the values; the stored levels lb .. n lie as merkle_level_offset says"""
    rng = random.Random(100 * n + lb)
    values = [rng.getrandbits(64) for _ in range(1 << n)]
    levels = levels_hl(values)
    B, per = 1 << (n - lb), 1 << lb
    stored = np.zeros((2 * B - 1, 8), dtype=np.uint32)
    for l in range(lb, n + 1):
        off = ph.ph_level_offset(B, l - lb)
        for k, d in enumerate(levels[l]):
            stored[off + k] = bytes_to_words(d)
    arr = np.array(values, dtype=np.uint64)
    for i in range(1 << n):
        vals = np.ascontiguousarray(arr[(i >> lb) << lb:((i >> lb) << lb) + per])
        sib = np.zeros((max(1, n - lb), 8), dtype=np.uint32)
        for l in range(lb, n):
            sib[l - lb] = stored[ph.ph_level_offset(B, l - lb) + ((i >> l) ^ 1)]
        leaf = ctypes.c_uint64()
        path = (ctypes.c_uint8 * max(1, 32 * n))()
        ph.ph_path(n, lb, i, vals.ctypes.data_as(u64p), sib.ctypes.data_as(u32p), ctypes.byref(leaf), path)
        assert leaf.value == values[i], i
        assert bytes(path)[:32 * n] == b"".join(path_hl(values, i, levels)), i


@pytest.mark.parametrize("p,m", [(3, 0), (3, 1), (3, 3), (5, 2), (7, 2), (11, 3)])
def test_grid_order_is_the_reference_sort(p, m):
    pkg = load_package()
    F = pkg.Field(p)
    rp = pkg.relaxed_pcs
    pts = rp.all_multidimentional_values(F, m)
    # permutations::permutations over all_values, then res.sort() by canonical value (lib.rs:55-61)
    ref = sorted([list(t) for t in itertools.product(range(p), repeat=m)])
    assert [[F.to_int(v) for v in pt] for pt in pts] == ref
    assert [rp.leaf_index(F, pt) for pt in pts] == list(range(p ** m))


def test_leaf_index_puts_v0_first():
    pkg = load_package()
    F = pkg.Field(5)
    rp = pkg.relaxed_pcs
    assert rp.leaf_index(F, [F.from_int(1), F.from_int(0)]) == 5
    assert rp.leaf_index(F, [F.from_int(0), F.from_int(1)]) == 1


# ---- the host verifier against hashlib -------------------------------------------------------------------------------

def _honest(F, values, i):
    pkg = load_package()
    rp = pkg.relaxed_pcs
    return rp.Path(i, path_hl(values, i), F), root_hl(values)


def test_path_verify_accepts_honest_paths_and_rejects_tampering():
    pkg = load_package()
    F = pkg.Field(389)
    rng = random.Random(3)
    values = [rng.randrange(389) for _ in range(16)]
    for i in range(16):
        path, root = _honest(F, values, i)
        assert path.verify(root, F.from_int(values[i]))
        assert path.verify_canonical(root, values[i])
        # a flipped sibling
        for l in range(4):
            bad = list(path.siblings)
            bad[l] = bytes([bad[l][0] ^ 1]) + bad[l][1:]
            assert not pkg.relaxed_pcs.Path(i, bad, F).verify(root, F.from_int(values[i]))
        # a wrong index bit
        for l in range(4):
            assert not pkg.relaxed_pcs.Path(i ^ (1 << l), path.siblings, F).verify(root, F.from_int(values[i]))
        # a wrong leaf, a wrong root
        assert not path.verify(root, F.from_int((values[i] + 1) % 389))
        assert not path.verify(hashlib.sha256(b"x").digest(), F.from_int(values[i]))
    # a one-leaf tree: the root is the leaf's digest
    p0, r0 = _honest(F, [42], 0)
    assert p0.siblings == [] and r0 == leaf_hl(42) and p0.verify(r0, F.from_int(42))


def _line_instance(p, m, seed):
    """(values of the padded grid, the MLE table, F) of a random m-variate multilinear polynomial over F_p, on the host"""
    pkg = load_package()
    F = pkg.Field(p)
    rng = random.Random(seed)
    table = [rng.randrange(p) for _ in range(1 << m)]
    grid = []
    for pt in itertools.product(range(p), repeat=m):
        acc = 0
        for x in range(1 << m):
            w = 1
            for j in range(m):
                w = w * (pt[j] if (x >> j) & 1 else 1 - pt[j]) % p
            acc = (acc + w * table[x]) % p
        grid.append(acc)
    N = 1
    while N < len(grid):
        N *= 2
    return grid + [0] * (N - len(grid)), table, F


def _restriction(F, table, b, c):
    """the univariate q(t) = W~(b + t (c - b)) as a SparsePolynomial, by interpolation over the integers mod p"""
    pkg = load_package()
    p, m = F.p, len(b)
    bi, ci = [F.to_int(x) for x in b], [F.to_int(x) for x in c]
    xs = list(range(m + 1))
    ys = []
    for t in xs:
        pt = [(bi[j] + t * (ci[j] - bi[j])) % p for j in range(m)]
        acc = 0
        for x in range(1 << m):
            w = 1
            for j in range(m):
                w = w * (pt[j] if (x >> j) & 1 else 1 - pt[j]) % p
            acc = (acc + w * table[x]) % p
        ys.append(acc)
    coeffs = [0] * (m + 1)
    for j in range(m + 1):
        num, den = [1], 1
        for k in range(m + 1):
            if k != j:
                num = [(a - xs[k] * b_) % p for a, b_ in zip([0] + num, num + [0])]
                den = den * (xs[j] - xs[k]) % p
        w = ys[j] * pow(den, -1, p) % p
        coeffs = [(cc + w * nn) % p for cc, nn in zip(coeffs, num)]
    return pkg.sum_check_protocol.SparsePolynomial.from_dense(F, [F.from_int(x) for x in coeffs])


def test_verifier_accepts_an_honest_reply_and_rejects_tampered_ones():
    pkg = load_package()
    rp = pkg.relaxed_pcs
    grid, table, F = _line_instance(5, 2, 1)
    root = root_hl(grid)
    outcomes = set()
    for seed in range(40):
        rng = random.Random(seed)
        v = rp.Verifier(F, 2, 1, root, strict_degree=False)
        b, c = v.random_line(rng)
        q = _restriction(F, table, b, c)
        point = v.challenge_prover(rng)
        i = rp.leaf_index(F, point)
        path = rp.Path(i, path_hl(grid, i), F)
        leaf = F.from_int(grid[i])
        v.commited_univariate(q)
        v.verify_prover_reply(path, leaf)
        strict = rp.Verifier(F, 2, 1, root)
        try:
            strict.commited_univariate(q)
            outcomes.add("exact")
        except rp.DegreeMismatch:
            assert q.degree() < 2
            outcomes.add("lower")
        # tampered leaf, path, univariate, and a path to another leaf
        with pytest.raises(rp.MerkleMismatch):
            v.verify_prover_reply(path, F.from_int((grid[i] + 1) % 5))
        bad = list(path.siblings)
        bad[0] = bytes(32)
        with pytest.raises(rp.MerkleMismatch):
            v.verify_prover_reply(rp.Path(i, bad, F), leaf)
        j = (i + 1) % 25
        with pytest.raises(rp.MerkleMismatch):
            v.verify_prover_reply(rp.Path(j, path_hl(grid, j), F), F.from_int(grid[j]))
        wrong = pkg.sum_check_protocol.SparsePolynomial.from_dense(F, [F.add(cf, F.one) if d == 0 else cf
                                                                       for d, cf in enumerate(_dense(F, q, 3))])
        v.commited_univariate(wrong)
        with pytest.raises(rp.EvalMismatch):
            v.verify_prover_reply(path, leaf)
    assert outcomes == {"exact", "lower"}, outcomes


def _dense(F, q, k):
    out = [0] * k
    for d, c in q.coeffs:
        out[d] = c
    return out


def test_strict_degree_mirrors_the_reference_quirk():
    pkg = load_package()
    rp = pkg.relaxed_pcs
    F = pkg.Field(11)
    SP = pkg.sum_check_protocol.SparsePolynomial
    low = SP.from_dense(F, [F.one, F.one])             # degree 1 against degree * num_vars = 3
    with pytest.raises(rp.DegreeMismatch):
        rp.Verifier(F, 3, 1, bytes(32)).commited_univariate(low)
    rp.Verifier(F, 3, 1, bytes(32), strict_degree=False).commited_univariate(low)
    high = SP.from_dense(F, [F.one] * 5)
    with pytest.raises(rp.DegreeMismatch):
        rp.Verifier(F, 3, 1, bytes(32), strict_degree=False).commited_univariate(high)
    with pytest.raises(rp.NoProverPoly):
        v = rp.Verifier(F, 0, 1, leaf_hl(0))
        v.random_line(random.Random(0))
        v.challenge_prover(random.Random(0))
        v.verify_prover_reply(rp.Path(0, [], F), 0)


# ---- the ISA of the hash kernels -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def isa():
    subprocess.check_call(["make", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    return (open(os.path.join(CSRC, "build", "sumcheck_hip.s")).read(),
            open(os.path.join(CSRC, "build", "resource_usage.txt")).read())


def _body(text, frag):
    m = re.search(r"^(_ZN2sc\S*%s\S*):[^\n]*\n(.*?)\n\.Lfunc_end" % re.escape(frag), text, flags=re.S | re.M)
    assert m, frag
    return m.group(2)


@pytest.mark.parametrize("frag", ["merkle_leaf_kernelINS_14GoldilocksMont", "merkle_leaf_kernelINS_11MontGeneric", "merkle_level_kernel",
                                  "merkle_top_kernel", "merkle_open_kernelINS_14GoldilocksMont", "grid_extend_kernel"])
def test_pcs_kernels_use_no_scratch(isa, frag):
    text, usage = isa
    blocks = [b for b in usage.split("remark: Function Name: ")[1:] if frag in b.split(" ")[0]]
    assert blocks, frag
    for b in blocks:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), b[:400]
    assert "scratch_" not in _body(text, frag)


@pytest.mark.parametrize("frag", ["merkle_leaf_kernelINS_14GoldilocksMont", "merkle_level_kernel", "merkle_top_kernel"])
def test_sha_kernels_rotate_with_alignbit(isa, frag):
    """every rotate is one v_alignbit_b32 (SHA-256 has 6 per round plus 4 per scheduled word: >= 400 per node) and Ch / Maj are
    single bit-select / three-input bit operations"""
    body = _body(isa[0], frag)
    assert body.count("v_alignbit_b32") >= 400, body.count("v_alignbit_b32")
    assert body.count("v_bfi_b32") + body.count("v_bitop3_b32") >= 128
