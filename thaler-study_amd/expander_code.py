"""\"Expander code 1\": the linear-time row code of the Ligero-style commitment for fields without two-adicity (Thaler, "Proofs,
Arguments, and Zero-Knowledge", section 10.5: Ligero with a linear-time code, as in Brakedown).  Pure host code over Montgomery
words; the device encoder is sc_xc_encode_rows (csrc/kernels/expander.hpp states the same contract).

A message x of m = 2^c words encodes to Enc_m(x) of 2 m words, systematic at rate 1/2:

  m <= 32   x || K x with the Cauchy matrix K[j][k] = 1 / (j + k + 1): [I | K] is MDS, distance m + 1; needs p > 63
  m >= 64   y = A x (m/4 words), z = Enc_(m/4)(y) (m/2 words), v = B z (m/2 words); the result is x || z || v

A and B are sums of D_A = 8 and D_B = 16 weighted permutation matrices, permutations and weights hashed from the level:
y[e >> 2] += coef(K, e) x[perm(K, lm, e)] for K = key(lm, 0, t), e < m, and v[j] += coef(K, j) z[perm(K, lm - 1, j)] for
K = key(lm, 1, t), j < m/2 (lm = log2 m).  The relative distance of the recursive code is NOT proved: no security level is
claimed for a commitment over it."""

M64 = 2**64 - 1
SEED = 0x4272616B65646F77
GOLDEN = 0x9E3779B97F4A7C15
D_A = 8
D_B = 16
BASE_MAX = 32          # messages of up to 32 words take the base code
MAX_LOG_COLS = 13      # the device encoder keeps one codeword of 2^14 words in the LDS of a CU
LONG_MAX_LOG_COLS = 23 # sc_xc_encode_rows_long: above 13 the largest levels run through global memory; at 2^24 the tree is 1 GiB
MIN_MODULUS = 64       # the base matrices invert 1 .. 63


def mix(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def key(lm, side, t):
    return mix(SEED + ((lm << 16) | (side << 8) | t))


def coef(K, e, p):
    """the canonical coefficient: the hash mod p, and 1 where that is 0"""
    return mix(K + (e + 1) * GOLDEN) % p or 1


def frnd(K, r, v):
    u = ((v ^ ((K >> (8 * r)) & 0xFFFFFFFF)) * 0x9E3779B1) & 0xFFFFFFFF
    u ^= u >> 15
    u = (u * 0x85EBCA77) & 0xFFFFFFFF
    return u ^ (u >> 13)


def perm(K, b, i):
    """a four-round Feistel network on b bits: a bijection of [0, 2^b) for every K"""
    bl = b >> 1
    bh = b - bl
    lo, hi = i & ((1 << bl) - 1), i >> bl
    for r in range(4):
        if r & 1:
            lo ^= frnd(K, r, hi) & ((1 << bl) - 1)
        else:
            hi ^= frnd(K, r, lo) & ((1 << bh) - 1)
    return (hi << bl) | lo


_gathers = {}


def _level(field, lm):
    """(A, B) of the level with 2^lm inputs as gather lists of (Montgomery coefficient, input index), cached per field and level"""
    k = (field.p, lm)
    if k not in _gathers:
        m = 1 << lm
        A = [[] for _ in range(m // 4)]
        for t in range(D_A):
            K = key(lm, 0, t)
            for e in range(m):
                A[e >> 2].append((field.from_int(coef(K, e, field.p)), perm(K, lm, e)))
        B = [[] for _ in range(m // 2)]
        for t in range(D_B):
            K = key(lm, 1, t)
            for j in range(m // 2):
                B[j].append((field.from_int(coef(K, j, field.p)), perm(K, lm - 1, j)))
        _gathers[k] = (A, B)
    return _gathers[k]


def _base_inverses(field):
    k = (field.p, "inv")
    if k not in _gathers:
        _gathers[k] = [0] + [field.from_int(pow(s, -1, field.p)) for s in range(1, 2 * BASE_MAX)]
    return _gathers[k]


def encode(field, u):
    """Enc(u): 2 len(u) Montgomery words for a message of Montgomery words whose length is a power of two"""
    m = len(u)
    if m < 1 or m & (m - 1):
        raise ValueError("the message must have 2^c words")
    if field.p < MIN_MODULUS:
        raise ValueError("p = %d: the base code inverts 1 .. 63 and needs p > 63" % field.p)
    x = [int(a) for a in u]
    p, rinv = field.p, field._rinv
    if m <= BASE_MAX:
        inv = _base_inverses(field)
        return x + [sum(inv[j + k + 1] * x[k] for k in range(m)) * rinv % p for j in range(m)]
    A, B = _level(field, m.bit_length() - 1)
    y = [sum(a * x[i] for a, i in terms) * rinv % p for terms in A]
    z = encode(field, y)
    v = [sum(a * z[i] for a, i in terms) * rinv % p for terms in B]
    return x + z + v
