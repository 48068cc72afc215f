"""A pure-Python restatement of the Ligero-style commitment's contract (thaler-study_amd/csrc/kernels/ligero.hpp), test-local:
nothing here imports the package.  Everything is in CANONICAL integers; the tests convert to and from Montgomery words at the
boundary (mont / canon below).

  FIELDS, WIDE_NTT, ROOTS               the fields of the tests and their (s, g, w_max)
  two_adic(p), omega(p, log_len)        the root of unity the contract prescribes
  ntt(row, w, p), ntt_rows_np(..)       a radix-2 transform in big integers, and one in numpy (int64 for p < 2^31) over whole matrices
  direct(row, w, p, j)                  the defining sum, one output
  encode(table, c, rho, p)              the codeword matrix E as a list of rows
  column_leaf, tree_levels, path_of     the digests, with hashlib
  combine, eq_weights, mle_eval         linear combinations of rows, the eq weights, the multilinear extension
  RefProver                             the prover of the protocol over all of the above"""
import hashlib

import numpy as np

GOLD = 2**64 - 2**32 + 1
BABYBEAR = 2013265921
FIELDS = [GOLD, BABYBEAR, 65537, 257]
# (s, g, w_max) as the contract lists them
ROOTS = {GOLD: (32, 7, 1753635133440165772), BABYBEAR: (27, 11, 1227303670), 65537: (16, 3, 3), 257: (8, 3, 3)}
# full-width NTT-friendly primes for the generic field (tests/test_gpu_ligero_wide.py): the closest to 2^64 with 2-adicity 18
# (R mod p = 1835007: sums and redc carry out almost always), one with s = 34 > 32, one just above 2^63, one just above 2^32
# (the high limb is 0 or 1) and one just below 2^32.  Not part of FIELDS.
P64S18 = 0xFFFFFFFFFFE40001
P64S34 = 0xFFFFFFFC00000001
P63S16 = 0x8000000000050001
P32HI = 0x100050001
P32LO = 0xFFF00001
WIDE_NTT = [P64S18, P64S34, P63S16, P32HI, P32LO]
ROOTS.update({P64S18: (18, 7, 11880867381004357348), P64S34: (34, 5, 6307343653039168829), P63S16: (16, 3, 3283862531989034960),
              P32HI: (16, 5, 2095801761), P32LO: (20, 17, 2948152962)})
R64 = 2**64


def mont(p, xs):
    return [int(x) * R64 % p for x in xs]


def canon(p, ws):
    rinv = pow(R64, -1, p)
    return [int(w) * rinv % p for w in ws]


def two_adic(p):
    s = 0
    while ((p - 1) >> s) & 1 == 0:
        s += 1
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return s, g, pow(g, (p - 1) >> s, p)


def omega(p, log_len):
    s, _, w_max = two_adic(p)
    assert log_len <= s
    return pow(w_max, 1 << (s - log_len), p)


def direct(row, w, p, j):
    """sum_k row[k] w^(j k)"""
    x = pow(w, j, p)
    acc = 0
    for coeff in reversed(row):
        acc = (acc * x + coeff) % p
    return acc


def ntt(a, w, p):
    """[sum_k a[k] w^(j k) for j < len(a)], len(a) a power of two and w of that order: recursive radix 2"""
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = ntt(a[0::2], w * w % p, p), ntt(a[1::2], w * w % p, p)
    out = [0] * n
    x = 1
    for j in range(n // 2):
        t = x * odd[j] % p
        out[j] = (even[j] + t) % p
        out[j + n // 2] = (even[j] - t) % p
        x = x * w % p
    return out


def ntt_rows_np(rows, w, p):
    """the same transform of every row of a matrix at once: iterative decimation in time over a bit-reversed copy, in numpy
    int64 for p < 2^31 (every product is exact) and in numpy arrays of Python integers above"""
    dtype = np.int64 if p < 2**31 else object
    a = np.array([[int(x) for x in row] for row in rows], dtype=dtype)
    n = a.shape[1]
    log_n = n.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0 for i in range(n)], dtype=np.int64)
    a = a[:, rev]
    h = 1
    while h < n:
        step = pow(w, n // (2 * h), p)
        tw = np.ones(h, dtype=dtype)
        for j in range(1, h):
            tw[j] = tw[j - 1] * step % p
        a = a.reshape(a.shape[0], n // (2 * h), 2, h)
        t = a[:, :, 1, :] * tw % p
        a = np.stack([(a[:, :, 0, :] + t) % p, (a[:, :, 0, :] - t) % p], axis=2).reshape(-1, n)
        h *= 2
    return a


def encode(table, c, rho, p):
    """E as a list of 2^(n-c) rows of L = 2^(c+rho) canonical values"""
    C, L = 1 << c, 1 << (c + rho)
    w = omega(p, c + rho)
    rows = [list(table[i:i + C]) + [0] * (L - C) for i in range(0, len(table), C)]
    return [[int(x) for x in row] for row in ntt_rows_np(rows, w, p)]


def column_leaf(E, j):
    return hashlib.sha256(b"".join(int(row[j]).to_bytes(8, "little") for row in E)).digest()


def tree_levels(leaves):
    lev = [list(leaves)]
    while len(lev[-1]) > 1:
        prev = lev[-1]
        lev.append([hashlib.sha256(prev[2 * k] + prev[2 * k + 1]).digest() for k in range(len(prev) // 2)])
    return lev


def root_of(E):
    return tree_levels([column_leaf(E, j) for j in range(len(E[0]))])[-1][0]


def path_of(levels, j):
    return [levels[l][(j >> l) ^ 1] for l in range(len(levels) - 1)]


def combine(table, c, weights, p):
    """sum_i weights[i] row_i of the table's rows of 2^c entries"""
    C = 1 << c
    return [sum(weights[i] * table[i * C + k] for i in range(len(table) // C)) % p for k in range(C)]


def eq_weights(point, p):
    w = [1]
    for r in point:
        w = [x * (1 - r) % p for x in w] + [x * r % p for x in w]
    return w


def mle_eval(table, point, p):
    """the multilinear extension of the table at `point`, LE"""
    return sum(a * b for a, b in zip(table, eq_weights(point, p))) % p


class RefProver:
    """the prover of the protocol in canonical integers.  E: the codeword matrix, a list of rows, where the row code is not
    Reed-Solomon (tests/expander_ref.py)"""

    def __init__(self, table, c, rho, p, E=None):
        self.table, self.c, self.rho, self.p = [int(x) for x in table], c, rho, p
        self.E = encode(self.table, c, rho, p) if E is None else E
        self.levels = tree_levels([column_leaf(self.E, j) for j in range(1 << (c + rho))])

    def root(self):
        return self.levels[-1][0]

    def combine(self, point, gamma):
        return combine(self.table, self.c, gamma, self.p), combine(self.table, self.c, eq_weights(point[self.c:], self.p), self.p)

    def open_columns(self, indices):
        """[(index, column values, sibling digests)]"""
        return [(j, [row[j] for row in self.E], path_of(self.levels, j)) for j in indices]
