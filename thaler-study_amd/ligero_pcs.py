"""A Ligero-style polynomial commitment on the GPU (Thaler, "Proofs, Arguments, and Zero-Knowledge", section 10.5).

The table of a multilinear polynomial in n variables is a matrix of R = 2^r rows by C = 2^c columns (n = r + c; variables
0..c-1 select the column, c..n-1 the row).  The prover Reed-Solomon-encodes every row (sc_rs_encode_rows: the row as the
coefficients of a polynomial, evaluated at the L = 2^(c + log_blowup) powers of w_L) and commits to the COLUMNS of the codeword
matrix with a SHA-256 Merkle tree (sc_ligero_commit).  An evaluation at z is opened interactively:

  1. the prover sends the root                                   4. the verifier draws `queries` columns in [0, L), with replacement
  2. the verifier sends gamma in F^R                             5. the prover opens each: its R values and its path
  3. the prover sends u_gamma = sum_i gamma_i row_i and          6. per column j the verifier checks the path against the root,
     u_z = sum_i eq(z[c:], i) row_i (C words each)                  Enc(u_gamma)[j] = sum_i gamma_i col_j[i] and Enc(u_z)[j] = sum_i eq_i col_j[i]
                                                                 7. the value is <u_z, eq(z[:c])>

Enc(u)[j] is u, as coefficients, evaluated at w_L^j (Horner).  The verifier is host code (hashlib) and never touches the GPU.

Contract (kernels/ligero.hpp):
  root of unity  s = the 2-adicity of p - 1, g the smallest integer >= 2 with g^((p-1)/2) = -1, w_max = g^((p-1)/2^s),
                 w_L = w_max^(2^(s - c - log_blowup))
  leaf j         SHA-256(le64(canon E[0][j]) || .. || le64(canon E[R-1][j])); nodes SHA-256(left || right); paths bottom up
  limits         c + log_blowup <= 14 and <= s, n + log_blowup <= 29, log_blowup in {1, 2}, one device and one rank
  long rows      rs_encode_rows_long / Prover.commit_long (sc_rs_encode_rows_long, sc_ligero_commit_long; DESIGN.md section 9
                 item 11) lift the first limit to c + log_blowup <= 24 = LONG_MAX_LOG_LEN: above 14 the rows go through a
                 four-step transform in two launches; the encoding, the commitment and the Verifier are the same.
                 opening_bytes and long_log_cols give the size of an opening and the log_cols that makes it smallest.

Field elements are Montgomery words, as everywhere in this package; leaves hash canonical integers.  `queries` is the caller's
parameter: DESIGN.md gives the book's soundness expression for it; no security level is claimed here.

code="expander" (sc_xc_encode_rows, sc_ligero_commit_code) replaces Reed-Solomon by the linear-time
code of expander_code.py - systematic, rate 1/2 (log_blowup = 1), additions and multiplications by constants only - for fields
without two-adicity such as 2^64 - 59: any p > 63, log_cols <= 13.  Everything above the encoder is the same; Enc(u)[j] is then
entry j of expander_code.encode(u).  The distance of that code is not proved.  xc_encode_rows_long and
Prover.commit_long(code="expander") (sc_xc_encode_rows_long, sc_ligero_commit_code_long) serve
log_cols up to expander_code.LONG_MAX_LOG_COLS = 23; the Verifier's host encoding of the two combined rows then costs seconds
at log_cols 14 - 15 and far more above."""
import ctypes
import hashlib

import numpy as np

from . import expander_code
from ._lib import size_t, voidp
from .dense_mle import DenseMultilinearExtension, _u64p, _words
from .relaxed_pcs import Error, EvalMismatch, MerkleMismatch, Path, _draw, node_digest

MAX_LOG_LEN = 14
LONG_MAX_LOG_LEN = 24                  # c + log_blowup of rs_encode_rows_long / Prover.commit_long
CODES = {"rs": 0, "expander": 1}       # SC_CODE_RS, SC_CODE_EXPANDER


def _code_id(code):
    if code not in CODES:
        raise ValueError("code must be one of %s, not %r" % (sorted(CODES), code))
    return CODES[code]


class ProximityMismatch(Error):
    """an opened column does not agree with the encoding of the claimed random combination of the rows"""

    def __init__(self, column, encoded, combined):
        super().__init__("Column %d: Enc(u_gamma) is %d, the combination of the opened column is %d" % (column, encoded, combined))
        self.column, self.encoded, self.combined = column, encoded, combined


# ---- the root of unity -----------------------------------------------------------------------------------------------

def two_adic_root(p):
    """(s, g, w_max) of the modulus p, canonical integers"""
    s = ((p - 1) & -(p - 1)).bit_length() - 1
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return s, g, pow(g, (p - 1) >> s, p)


def root_of_unity(field, log_len):
    """w_L for L = 2^log_len, a Montgomery word"""
    s, _, w_max = two_adic_root(field.p)
    if log_len > s:
        raise ValueError("p = %d has 2-adicity %d: no root of unity of order 2^%d" % (field.p, s, log_len))
    return field.from_int(pow(w_max, 1 << (s - log_len), field.p))


def eq_weights(field, point):
    """eq(point, i) for every i < 2^len(point), LE: bit j of i goes with point[j]"""
    w = [field.one]
    for r in point:
        w = [field.mul(x, field.sub(field.one, r)) for x in w] + [field.mul(x, r) for x in w]
    return w


def default_log_cols(num_vars, log_blowup, code="rs"):
    if code == "expander":
        return min((num_vars + 1) // 2, expander_code.MAX_LOG_COLS)
    return min((num_vars + 1) // 2, MAX_LOG_LEN - log_blowup)


def opening_bytes(num_vars, log_cols, log_blowup, queries):
    """bytes of an opening: `queries` columns of 2^(n - c) words with their paths of c + log_blowup digests, and the two combined
    rows of 2^c words"""
    return queries * (8 * (1 << (num_vars - log_cols)) + 32 * (log_cols + log_blowup)) + 2 * 8 * (1 << log_cols)


def long_log_cols(num_vars, log_blowup, queries, max_log_len=LONG_MAX_LOG_LEN):
    """the log_cols in 0 .. min(num_vars, max_log_len - log_blowup) with the smallest opening (ties: the smaller)"""
    return min(range(min(num_vars, max_log_len - log_blowup) + 1), key=lambda c: (opening_bytes(num_vars, c, log_blowup, queries), c))


# ---- hashing (host) --------------------------------------------------------------------------------------------------

def column_digest(field, values):
    """the leaf of a column: SHA-256 over the 8 little-endian bytes of every canonical value, top row first"""
    return hashlib.sha256(b"".join(field.to_int(v).to_bytes(8, "little") for v in values)).digest()


class ColumnPath(Path):
    """relaxed_pcs.Path over column leaves: the same sibling walk, started from a column's digest"""

    def root_from_column(self, values):
        return self.root_from_digest(column_digest(self.field, values))

    def verify_column(self, root, values):
        return self.index < (1 << len(self.siblings)) and self.root_from_column(values) == bytes(root)


# ---- the device side -------------------------------------------------------------------------------------------------

def _encode_rows(ctx, symbol, poly, *shape):
    """call an encode symbol on `poly`'s table and wrap the handle of the codeword matrix"""
    h = voidp()
    ctx.check(getattr(ctx.lib, symbol)(ctx.h, poly.h, *shape, ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


def rs_encode_rows(ctx, poly, log_cols, log_blowup):
    """sc_rs_encode_rows: the codeword matrix of `poly`'s table, row-major, a device table of 2^(n + log_blowup) words"""
    return _encode_rows(ctx, "sc_rs_encode_rows", poly, log_cols, log_blowup)


def rs_encode_rows_long(ctx, poly, log_cols, log_blowup):
    """sc_rs_encode_rows_long: rs_encode_rows for log_cols + log_blowup up to LONG_MAX_LOG_LEN"""
    return _encode_rows(ctx, "sc_rs_encode_rows_long", poly, log_cols, log_blowup)


def xc_encode_rows(ctx, poly, log_cols):
    """sc_xc_encode_rows: the codeword matrix of `poly`'s table under the expander code, row-major, a device table of 2^(n + 1) words"""
    return _encode_rows(ctx, "sc_xc_encode_rows", poly, log_cols)


def xc_encode_rows_long(ctx, poly, log_cols):
    """sc_xc_encode_rows_long: xc_encode_rows for log_cols up to expander_code.LONG_MAX_LOG_COLS"""
    return _encode_rows(ctx, "sc_xc_encode_rows_long", poly, log_cols)


class Prover:
    """sc_ligero_*: the commitment to a device table (borrowed: kept alive by the prover) and the replies of an opening"""

    def __init__(self, ctx, poly, handle):
        self.ctx, self.field, self.poly, self.h = ctx, ctx.field, poly, handle
        r, c, b = size_t(), size_t(), size_t()
        ctx.check(ctx.lib.sc_ligero_shape(handle, ctypes.byref(r), ctypes.byref(c), ctypes.byref(b)))
        self.log_rows, self.log_cols, self.log_blowup = r.value, c.value, b.value
        self.num_vars = self.log_rows + self.log_cols
        code = ctypes.c_int()
        ctx.check(ctx.lib.sc_ligero_code(handle, ctypes.byref(code)))
        self.code = {v: k for k, v in CODES.items()}[code.value]

    @classmethod
    def _commit(cls, ctx, poly, log_cols, log_blowup, code, long_rows):
        """sc_ligero_commit_code or its _long form, which hand Reed-Solomon to sc_ligero_commit / sc_ligero_commit_long"""
        symbol = "sc_ligero_commit_code_long" if long_rows else "sc_ligero_commit_code"
        h = voidp()
        ctx.check(getattr(ctx.lib, symbol)(ctx.h, poly.h, log_cols, log_blowup, _code_id(code), ctypes.byref(h)))
        return cls(ctx, poly, h)

    @classmethod
    def commit(cls, ctx, poly, log_cols=None, log_blowup=1, code="rs"):
        _code_id(code)
        if log_cols is None:
            log_cols = default_log_cols(poly.num_vars(), log_blowup, code)
        return cls._commit(ctx, poly, log_cols, log_blowup, code, False)

    @classmethod
    def commit_long(cls, ctx, poly, log_cols=None, log_blowup=1, queries=None, code="rs"):
        """sc_ligero_commit_long / sc_ligero_commit_code_long: rows of up to 2^LONG_MAX_LOG_LEN codeword words.  log_cols=None: the
        shape whose opening of `queries` columns is smallest (long_log_cols) - for Reed-Solomon as far as the field's two-adicity
        allows; the expander code has no such bound"""
        _code_id(code)
        if log_cols is None:
            if queries is None:
                raise ValueError("commit_long chooses log_cols from the number of queries: give log_cols or queries")
            s = two_adic_root(ctx.field.p)[0] if code == "rs" else LONG_MAX_LOG_LEN
            log_cols = long_log_cols(poly.num_vars(), log_blowup, queries, min(LONG_MAX_LOG_LEN, s))
        return cls._commit(ctx, poly, log_cols, log_blowup, code, True)

    def root(self):
        buf = (ctypes.c_uint8 * 32)()
        self.ctx.check(self.ctx.lib.sc_ligero_root(self.h, buf))
        return bytes(buf)

    def combine_rows(self, weights):
        """[sum_i w[i] row_i for w in weights]: up to four vectors of 2^log_rows words in one read of the table"""
        count = len(weights)
        w = np.ascontiguousarray(np.array([[int(x) for x in row] for row in weights], dtype=np.uint64).reshape(-1))
        if count and w.size != count << self.log_rows:
            raise ValueError("weight vectors must have 2^log_rows = %d words" % (1 << self.log_rows))
        out = np.zeros(max(1, count << self.log_cols), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.sc_ligero_combine_rows(self.ctx.h, self.h, _u64p(w) if count else None, count, _u64p(out)))
        return [[int(x) for x in out[m << self.log_cols:(m + 1) << self.log_cols]] for m in range(count)]

    def combine(self, point, gamma):
        """(u_gamma, u_z) for the evaluation point and the verifier's gamma; the eq weights of point[c:] are built on the host"""
        if len(point) != self.num_vars:
            raise ValueError("the point has %d coordinates, the polynomial %d variables" % (len(point), self.num_vars))
        u_gamma, u_z = self.combine_rows([list(gamma), eq_weights(self.field, list(point)[self.log_cols:])])
        return u_gamma, u_z

    def open_columns(self, indices):
        """[(index, values, ColumnPath)] for every index, in one call; values are the column's 2^log_rows Montgomery words"""
        idx = _words(indices)
        count, depth, R = idx.size, self.log_cols + self.log_blowup, 1 << self.log_rows
        values = np.zeros(max(1, count * R), dtype=np.uint64)
        paths = (ctypes.c_uint8 * max(1, count * depth * 32))()
        self.ctx.check(self.ctx.lib.sc_ligero_open_columns(self.ctx.h, self.h, _u64p(idx) if count else None, count, _u64p(values), paths))
        raw = bytes(paths)
        out = []
        for q in range(count):
            sib = [raw[(q * depth + l) * 32:(q * depth + l + 1) * 32] for l in range(depth)]
            out.append((int(idx[q]), [int(v) for v in values[q * R:(q + 1) * R]], ColumnPath(int(idx[q]), sib, self.field)))
        return out

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_ligero_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the verifier ----------------------------------------------------------------------------------------------------

class Verifier:
    """The verifier of one opening.  Pure host code: draw_gamma, receive, draw_columns, verify - in that order."""

    def __init__(self, field, num_vars, log_cols, log_blowup, root, queries, code="rs"):
        _code_id(code)
        if not 0 <= log_cols <= num_vars or log_blowup not in (1, 2):
            raise ValueError("log_cols must be in 0..num_vars and log_blowup 1 or 2")
        if code == "expander" and log_blowup != 1:
            raise ValueError("the expander code has rate 1/2: log_blowup must be 1")
        self.code = code
        self.field, self.num_vars, self.log_cols, self.log_blowup = field, num_vars, log_cols, log_blowup
        self.log_rows = num_vars - log_cols
        self.log_len = log_cols + log_blowup
        self.root, self.queries = bytes(root), int(queries)
        self.omega = root_of_unity(field, self.log_len) if code == "rs" else None
        self.enc_gamma = self.enc_z = None      # the expander code: the two whole codewords, encoded once in receive
        self.gamma = None
        self.u_gamma = self.u_z = None
        self.columns = None

    def draw_gamma(self, rng):
        self.gamma = [_draw(self.field, rng) for _ in range(1 << self.log_rows)]
        return list(self.gamma)

    def receive(self, u_gamma, u_z):
        if self.gamma is None:
            raise Error("receive before draw_gamma")
        if len(u_gamma) != 1 << self.log_cols or len(u_z) != 1 << self.log_cols:
            raise Error("the combined rows must have 2^log_cols = %d words" % (1 << self.log_cols))
        self.u_gamma, self.u_z = [int(x) for x in u_gamma], [int(x) for x in u_z]
        if self.code == "expander":
            self.enc_gamma, self.enc_z = expander_code.encode(self.field, self.u_gamma), expander_code.encode(self.field, self.u_z)

    def draw_columns(self, rng):
        """`queries` column indices in [0, L), with replacement; only after the prover is bound to u_gamma and u_z"""
        if self.u_gamma is None:
            raise Error("draw_columns before receive: the columns must be drawn after the prover has sent u_gamma and u_z")
        L = 1 << self.log_len
        self.columns = [rng.randrange(L) if hasattr(rng, "randrange") else self.field.to_int(rng.draw()) % L for _ in range(self.queries)]
        return list(self.columns)

    def _encode_at(self, u, j):
        """Enc(u)[j]: the polynomial with coefficients u at w_L^j (Horner); the expander code: entry j of the whole codeword
        (verify reads the two codewords receive stored instead)"""
        F = self.field
        if self.code == "expander":
            return expander_code.encode(F, u)[j]
        x = F.from_int(pow(F.to_int(self.omega), j, F.p))
        acc = 0
        for coeff in reversed(u):
            acc = F.add(F.mul(acc, x), coeff)
        return acc

    def verify(self, point, openings):
        """check every opening; returns the value of the committed polynomial at `point`"""
        F = self.field
        if self.columns is None:
            raise Error("verify before draw_columns")
        if len(point) != self.num_vars:
            raise Error("the point has %d coordinates, the polynomial %d variables" % (len(point), self.num_vars))
        if len(openings) != len(self.columns):
            raise MerkleMismatch("%d openings for %d drawn columns" % (len(openings), len(self.columns)))
        eq_rows = eq_weights(F, list(point)[self.log_cols:])
        for want, (index, values, path) in zip(self.columns, openings):
            if index != want or path.index != want:
                raise MerkleMismatch("the opening is of column %d, the drawn column is %d" % (index, want))
            if len(values) != 1 << self.log_rows or len(path.siblings) != self.log_len:
                raise MerkleMismatch("an opening of the wrong shape")
            if not ColumnPath(path.index, path.siblings, F).verify_column(self.root, values):
                raise MerkleMismatch("the opening of column %d does not lead to the committed root" % index)
            for u, enc, weights, err in ((self.u_gamma, self.enc_gamma, self.gamma, ProximityMismatch),
                                         (self.u_z, self.enc_z, eq_rows, EvalMismatch)):
                combined = 0
                for wt, v in zip(weights, values):
                    combined = F.add(combined, F.mul(wt, int(v)))
                encoded = enc[index] if enc is not None else self._encode_at(u, index)
                if encoded != combined:
                    if err is ProximityMismatch:
                        raise ProximityMismatch(index, encoded, combined)
                    raise EvalMismatch(combined, encoded)
        value = 0
        for a, b in zip(self.u_z, eq_weights(F, list(point)[:self.log_cols])):
            value = F.add(value, F.mul(a, b))
        return value
