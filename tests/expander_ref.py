"""A pure-Python restatement of "expander code 1" (thaler-study_amd/csrc/kernels/expander.hpp),
test-local: nothing here imports the package.  Everything is in CANONICAL integers.  What a commitment has above its row code -
the digests, the combinations, the prover - is tests/ligero_ref.py's, under the same names here.

  mix, key, coef, frnd, perm            the hashes that define the two sparse maps of a level
  base_matrix(m, p)                     the Cauchy matrix K[j][k] = 1 / (j + k + 1) of the base code
  encode(x, p)                          Enc_m(x), a list of 2 m values (m a power of two)
  encode_rows(table, c, p)              the codeword matrix of a table's rows of 2^c entries
  known_answer(p, c)                    (E[m], E[2m-1], sha256 hex) of the message x[i] = 3 i + 1
  RefProver                             ligero_ref.RefProver over this code (log_blowup = 1)"""
import hashlib

import ligero_ref
from ligero_ref import column_leaf, combine, eq_weights, root_of, tree_levels   # noqa: F401 (expander_ref.root_of and the rest)

M64 = 2**64 - 1
SEED = 0x4272616B65646F77
GOLDEN = 0x9E3779B97F4A7C15
D_A = 8
D_B = 16
BASE_MAX = 32


def mix(x):
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def key(lm, side, t):
    return mix(SEED + ((lm << 16) | (side << 8) | t))


def coef(K, e, p):
    return mix(K + (e + 1) * GOLDEN) % p or 1


def frnd(K, r, v):
    u = ((v ^ ((K >> (8 * r)) & 0xFFFFFFFF)) * 0x9E3779B1) & 0xFFFFFFFF
    u ^= u >> 15
    u = u * 0x85EBCA77 & 0xFFFFFFFF
    return u ^ (u >> 13)


def perm(K, b, i):
    bl = b >> 1
    bh = b - bl
    lo, hi = i & ((1 << bl) - 1), i >> bl
    for r in range(4):
        if r % 2 == 0:
            hi ^= frnd(K, r, lo) & ((1 << bh) - 1)
        else:
            lo ^= frnd(K, r, hi) & ((1 << bl) - 1)
    return (hi << bl) | lo


def base_matrix(m, p):
    return [[pow(j + k + 1, -1, p) for k in range(m)] for j in range(m)]


_maps = {}


def level_maps(lm, p):
    """the two sparse maps of the level with 2^lm inputs as gather lists: A[q] = [(coefficient, input index)] of y[q] (32 terms),
    B[j] likewise of v[j] (16 terms); cached per (lm, p)"""
    if (lm, p) not in _maps:
        m = 1 << lm
        A = [[] for _ in range(m // 4)]
        for t in range(D_A):
            K = key(lm, 0, t)
            for e in range(m):
                A[e >> 2].append((coef(K, e, p), perm(K, lm, e)))
        B = [[] for _ in range(m // 2)]
        for t in range(D_B):
            K = key(lm, 1, t)
            for j in range(m // 2):
                B[j].append((coef(K, j, p), perm(K, lm - 1, j)))
        _maps[(lm, p)] = (A, B)
    return _maps[(lm, p)]


def encode(x, p):
    m = len(x)
    assert m & (m - 1) == 0 and m >= 1
    x = [int(a) % p for a in x]
    if m <= BASE_MAX:
        assert p > 2 * BASE_MAX - 1
        return x + [sum(pow(j + k + 1, -1, p) * x[k] for k in range(m)) % p for j in range(m)]
    A, B = level_maps(m.bit_length() - 1, p)
    y = [sum(a * x[i] for a, i in terms) % p for terms in A]
    z = encode(y, p)
    v = [sum(a * z[i] for a, i in terms) % p for terms in B]
    return x + z + v


def encode_rows(table, c, p):
    C = 1 << c
    return [encode(table[i:i + C], p) for i in range(0, len(table), C)]


def digest_of(E):
    return hashlib.sha256(b"".join(int(v).to_bytes(8, "little") for v in E)).hexdigest()


def known_answer(p, c):
    m = 1 << c
    E = encode([(3 * i + 1) % p for i in range(m)], p)
    return E[m], E[2 * m - 1], digest_of(E)


class RefProver(ligero_ref.RefProver):
    """the prover of the protocol over this code"""

    def __init__(self, table, c, p):
        super().__init__(table, c, 1, p, E=encode_rows([int(x) for x in table], c, p))
