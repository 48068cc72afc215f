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
at log_cols 14 - 15 and far more above.

Folded openings (kernels/rs_fold.hpp states the contract): Prover.fold_begin, FoldVerifier and
open_folded prove the combined row m = u_z + beta u_gamma instead of sending u_gamma and u_z - log_cols rounds of the product
sumcheck over (m, eq(z[:c])) interleaved with log_cols folds of Enc(m) (sc_ligero_fold_*, one rs_fold_kernel launch per round, the kernel at arity one),
the folded layers committed with the same leaf and tree.  The opening no longer grows with 2^log_cols and the verifier does
2 * 2^log_rows + log_cols products per query: fold_opening_bytes and fold_log_cols give its size and the shape that makes it
smallest.  Reed-Solomon commitments with log_cols >= 1 only; the plain opening stays the default.  No security level is claimed.

Staged folded openings: a schedule `arities` = (a_0, .., a_(S-1)), 1 <= a_s <= 3, sum = log_cols,
folds a_s variables between two committed layers - a layer's leaf then holds 2^a_s words and there are S - 1 trees instead of
log_cols - 1 (sc_ligero_fold_begin_staged, one rs_fold_kernel launch per stage).  Prover.fold_begin, FoldVerifier and
fold_opening_bytes take `arities`; fold_shape gives the (log_cols, schedule) of the smallest opening; rs_fold_many is the fold
alone.  arities=None is the binary opening above, unchanged.  The number of queries an arity needs is not analysed.

Openings at a point of the quadratic extension K = F_p[X] / (X^2 - w) (ext_field.QuadExt):
Prover.combine_ext and ExtVerifier open a base-field commitment at z in K^n.  The row weights eq(z[c:]) split into their c0 and c1
words, u_z becomes the pair (u_z0, u_z1) - one sc_ligero_combine_rows call of three weight vectors - and the value is an element of
K.  Both codes; gamma stays in the base field."""
import ctypes
import hashlib

import numpy as np

from . import expander_code
from ._lib import DRAW_FOLD_FN, size_t, u64, voidp
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


def _schedule(log_cols, arities):
    """the schedule as a tuple of ints (None: log_cols ones), checked"""
    if arities is None:
        return (1,) * log_cols
    arities = tuple(int(a) for a in arities)
    if not arities or any(not 1 <= a <= 3 for a in arities) or sum(arities) != log_cols:
        raise ValueError("a schedule is a non-empty list of arities in 1..3 that sum to log_cols = %d, not %r" % (log_cols, arities))
    return arities


def _stage_starts(arities):
    """i_s = a_0 + .. + a_(s-1) for every stage s"""
    starts, i = [], 0
    for a in arities:
        starts.append(i)
        i += a
    return starts


def fold_opening_bytes(num_vars, log_cols, log_blowup, queries, arities=None):
    """bytes of a folded opening: per query 2^a_0 columns of 2^(n - c) words with their paths of c + log_blowup digests and, for
    every stage s >= 1, a leaf of 2^a_s words with a path of c + log_blowup - i_s - a_s digests; once, the S - 1 stage roots, the c
    round polynomials of three words, and v, v_gamma and the final value.  arities=None: every a_s = 1, a pair per layer"""
    if log_cols < 1:
        raise ValueError("a folded opening needs log_cols >= 1")
    arities = _schedule(log_cols, arities)
    l0 = log_cols + log_blowup
    per_query = (1 << arities[0]) * (8 * (1 << (num_vars - log_cols)) + 32 * l0)
    per_query += sum(8 * (1 << a) + 32 * (l0 - i - a) for i, a in list(zip(_stage_starts(arities), arities))[1:])
    return queries * per_query + 32 * (len(arities) - 1) + 24 * log_cols + 24


def fold_log_cols(num_vars, log_blowup, queries, max_log_len=LONG_MAX_LOG_LEN):
    """the log_cols in 1 .. min(num_vars, max_log_len - log_blowup) with the smallest folded opening (ties: the smaller)"""
    return min(range(1, min(num_vars, max_log_len - log_blowup) + 1), key=lambda c: (fold_opening_bytes(num_vars, c, log_blowup, queries), c))


def fold_shape(num_vars, log_blowup, queries, max_arity=3, max_log_len=LONG_MAX_LOG_LEN):
    """(log_cols, arities) of the smallest staged folded opening with arities up to max_arity: the fewest bytes, then the smaller
    log_cols, then the lexicographically smallest schedule.  A dynamic programme over the round index, from the last round back"""
    if not 1 <= max_arity <= 3:
        raise ValueError("max_arity must be 1, 2 or 3")
    best = None
    for c in range(1, min(num_vars, max_log_len - log_blowup) + 1):
        l0 = c + log_blowup
        tail = [0] * (c + 1)                    # tail[i]: the fewest bytes of the stages >= 1 that start at round i or later
        for i in range(c - 1, 0, -1):
            tail[i] = min(queries * (8 * (1 << a) + 32 * (l0 - i - a)) + 32 + tail[i + a] for a in range(1, min(max_arity, c - i) + 1))
        column = 8 * (1 << (num_vars - c)) + 32 * l0
        total, a0 = min((queries * (1 << a) * column + tail[a] + 24 * c + 24, a) for a in range(1, min(max_arity, c) + 1))
        if best is None or total < best[0]:
            arities, i = [a0], a0
            while i < c:                         # the smallest arity that still reaches tail[i], stage by stage
                a = next(a for a in range(1, min(max_arity, c - i) + 1) if queries * (8 * (1 << a) + 32 * (l0 - i - a)) + 32 + tail[i + a] == tail[i])
                arities.append(a)
                i += a
            best = (total, c, tuple(arities))
    return best[1], best[2]


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

    def combine_ext(self, point, gamma, w=None):
        """(u_gamma, u_z0, u_z1) for a point of K^n, K = ext_field.QuadExt(field, w) (elements are (c0, c1) pairs; w=None: the
        smallest non-residue): the row weights eq(point[c:]) in K split into their c0 and c1 words, and since the table is
        base-field, u_z = u_z0 + X u_z1 with u_zk = sum_i weight_k[i] row_i.  ONE sc_ligero_combine_rows call of three vectors"""
        from .ext_field import QuadExt
        if len(point) != self.num_vars:
            raise ValueError("the point has %d coordinates, the polynomial %d variables" % (len(point), self.num_vars))
        K = QuadExt(self.field, w)
        w0, w1 = K.split(K.eq_weights([tuple(z) for z in point][self.log_cols:]))
        u_gamma, u_z0, u_z1 = self.combine_rows([list(gamma), w0, w1])
        return u_gamma, u_z0, u_z1

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

    def fold_begin(self, point, gamma, arities=None):
        """sc_ligero_fold_begin: a folded opening at `point` under the verifier's gamma; its .claims are (v, v_gamma).  With a
        schedule `arities` (sc_ligero_fold_begin_staged) the opening folds a_s variables per committed layer"""
        if len(point) != self.num_vars:
            raise ValueError("the point has %d coordinates, the polynomial %d variables" % (len(point), self.num_vars))
        if len(gamma) != 1 << self.log_rows:
            raise ValueError("gamma must have 2^log_rows = %d words" % (1 << self.log_rows))
        z, g = _words(point), _words(gamma)
        claims = np.zeros(2, dtype=np.uint64)
        h = voidp()
        if arities is None:
            self.ctx.check(self.ctx.lib.sc_ligero_fold_begin(self.ctx.h, self.h, _u64p(z), _u64p(g), _u64p(claims), ctypes.byref(h)))
        else:
            ar = np.ascontiguousarray(np.array([int(a) for a in arities], dtype=np.int32))
            self.ctx.check(self.ctx.lib.sc_ligero_fold_begin_staged(self.ctx.h, self.h, _u64p(z), _u64p(g),
                                                                    ar.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if ar.size else None, ar.size,
                                                                    _u64p(claims), ctypes.byref(h)))
        return FoldOpening(self, h, (int(claims[0]), int(claims[1])), None if arities is None else tuple(int(a) for a in arities))

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_ligero_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rs_fold(ctx, table, alpha):
    """sc_rs_fold: one fold of a codeword of 2^l words (2 <= l <= 24) with alpha, a device table of half the length"""
    h = voidp()
    ctx.check(ctx.lib.sc_rs_fold(ctx.h, table.h, int(alpha), ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


def rs_fold_many(ctx, table, alphas):
    """sc_rs_fold_many: len(alphas) = 1 .. 3 successive folds of a codeword of 2^l words (len(alphas) + 1 <= l <= 24) in one launch,
    a device table of 2^(l - len(alphas)) words"""
    a = _words(alphas)
    h = voidp()
    ctx.check(ctx.lib.sc_rs_fold_many(ctx.h, table.h, _u64p(a) if a.size else None, a.size, ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


class FoldOpening:
    """sc_ligero_fold_*: the prover's side of one folded opening (Prover.fold_begin): .claims, then prove, then query.
    .arities is the schedule the opening was begun with, None for the binary opening"""

    def __init__(self, prover, handle, claims, arities=None):
        self.prover, self.ctx, self.h, self.claims, self.arities = prover, prover.ctx, handle, claims, arities
        self.log_cols, self.log_len = prover.log_cols, prover.log_cols + prover.log_blowup
        self.schedule = _schedule(self.log_cols, arities)

    def prove(self, beta, draw):
        """the log_cols rounds: draw(round, [H(0), H(1), H(2)], root or None) returns alpha_i; the root is that of stage s >= 1 at
        its first round i_s (the binary opening: root_i at every round i >= 1).  Returns (rounds, roots, challenges, final value):
        rounds[i] the three sums, roots[s - 1] the root of stage s = 1 .. S - 1"""
        c, S = self.log_cols, len(self.schedule)
        failure = []

        def cb(_user, i, e, root):
            try:
                return int(draw(i, [int(e[0]), int(e[1]), int(e[2])], ctypes.string_at(root, 32) if root else None))
            except BaseException as exc:   # (an exception must not cross the C frames: the call ends and it is raised again below)
                failure.append(exc)
                return self.ctx.field.p
        evals, challenges = np.zeros(3 * c, dtype=np.uint64), np.zeros(c, dtype=np.uint64)
        roots = (ctypes.c_uint8 * max(1, 32 * (S - 1)))()
        final = u64()
        rc = self.ctx.lib.sc_ligero_fold_prove(self.ctx.h, self.h, int(beta), DRAW_FOLD_FN(cb), None, _u64p(evals), roots, _u64p(challenges),
                                               ctypes.byref(final))
        if failure:
            raise failure[0]
        self.ctx.check(rc)
        raw = bytes(roots)
        return ([[int(x) for x in evals[3 * i:3 * i + 3]] for i in range(c)], [raw[32 * i:32 * i + 32] for i in range(S - 1)],
                [int(x) for x in challenges], int(final.value))

    def query(self, indices):
        """the binary opening: [(q, column q, column q + L / 2, layers)] for every index q < L / 2: the columns as
        Prover.open_columns gives them, layers[i - 1] = ((U_i[j_i], U_i[j_i + M_i / 2]), siblings) for i = 1 .. log_cols - 1.
        With a schedule: [(q, [the 2^a_0 columns q + t L / 2^a_0], stages)] for every q < L / 2^a_0, stages[s - 1] = (the 2^a_s words
        of leaf j_s, siblings) for s = 1 .. S - 1"""
        idx = _words(indices)
        count, l0, ar = idx.size, self.log_len, self.schedule
        depths = [l0 - i - a for i, a in list(zip(_stage_starts(ar), ar))[1:]]
        P, W = sum(depths), sum(1 << a for a in ar[1:])
        pairs = np.zeros(max(1, count * W), dtype=np.uint64)
        paths = (ctypes.c_uint8 * max(1, count * P * 32))()
        self.ctx.check(self.ctx.lib.sc_ligero_fold_query(self.ctx.h, self.h, _u64p(idx) if count else None, count, _u64p(pairs), paths))
        stride, parts = 1 << (l0 - ar[0]), 1 << ar[0]
        cols = self.prover.open_columns([int(q) + t * stride for t in range(parts) for q in idx])
        raw = bytes(paths)
        out = []
        for k in range(count):
            stages, at, word = [], k * P, k * W
            for a, depth in zip(ar[1:], depths):
                words = tuple(int(x) for x in pairs[word:word + (1 << a)])
                stages.append((words, [raw[(at + l) * 32:(at + l + 1) * 32] for l in range(depth)]))
                at += depth
                word += 1 << a
            if self.arities is None:
                out.append((int(idx[k]), cols[k], cols[count + k], stages))
            else:
                out.append((int(idx[k]), [cols[t * count + k] for t in range(parts)], stages))
        return out

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_ligero_fold_destroy(self.ctx.h, self.h)
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


# ---- the verifier of an opening at a point of the quadratic extension ------------------------------------------------

class ExtVerifier(Verifier):
    """The plain Verifier's flow for a point z of K^n, K = ext_field.QuadExt(field, w) (w=None: the smallest non-residue), over
    a base-field commitment: draw_gamma, receive(u_gamma, u_z0, u_z1), draw_columns, verify(point, openings) - which returns the
    value in K, a (c0, c1) pair.  The committed table is base-field, so f(z) = (sum eq.c0 f, sum eq.c1 f): the row weights
    eq(z[c:]) split into two base vectors, and each opened column is checked against both (one EvalMismatch check per
    component).  gamma stays in the base field."""

    def __init__(self, field, num_vars, log_cols, log_blowup, root, queries, code="rs", w=None):
        from .ext_field import QuadExt
        super().__init__(field, num_vars, log_cols, log_blowup, root, queries, code=code)
        self.ext = QuadExt(field, w)
        self.u_z1 = self.enc_z1 = None

    def receive(self, u_gamma, u_z0, u_z1):
        if len(u_z1) != 1 << self.log_cols:
            raise Error("the combined rows must have 2^log_cols = %d words" % (1 << self.log_cols))
        super().receive(u_gamma, u_z0)
        self.u_z1 = [int(x) for x in u_z1]
        if self.code == "expander":
            self.enc_z1 = expander_code.encode(self.field, self.u_z1)

    def verify(self, point, openings):
        """check every opening; returns the value of the committed polynomial at `point`, an element of K"""
        F, K = self.field, self.ext
        if self.columns is None:
            raise Error("verify before draw_columns")
        if len(point) != self.num_vars:
            raise Error("the point has %d coordinates, the polynomial %d variables" % (len(point), self.num_vars))
        if len(openings) != len(self.columns):
            raise MerkleMismatch("%d openings for %d drawn columns" % (len(openings), len(self.columns)))
        point = [tuple(int(x) for x in z) for z in point]
        eq_rows0, eq_rows1 = K.split(K.eq_weights(point[self.log_cols:]))
        for want, (index, values, path) in zip(self.columns, openings):
            if index != want or path.index != want:
                raise MerkleMismatch("the opening is of column %d, the drawn column is %d" % (index, want))
            if len(values) != 1 << self.log_rows or len(path.siblings) != self.log_len:
                raise MerkleMismatch("an opening of the wrong shape")
            if not ColumnPath(path.index, path.siblings, F).verify_column(self.root, values):
                raise MerkleMismatch("the opening of column %d does not lead to the committed root" % index)
            for u, enc, weights, proximity in ((self.u_gamma, self.enc_gamma, self.gamma, True), (self.u_z, self.enc_z, eq_rows0, False),
                                               (self.u_z1, self.enc_z1, eq_rows1, False)):
                combined = 0
                for wt, v in zip(weights, values):
                    combined = F.add(combined, F.mul(wt, int(v)))
                encoded = enc[index] if enc is not None else self._encode_at(u, index)
                if encoded != combined:
                    if proximity:
                        raise ProximityMismatch(index, encoded, combined)
                    raise EvalMismatch(combined, encoded)
        value = K.zero
        for a0, a1, e in zip(self.u_z, self.u_z1, K.eq_weights(point[:self.log_cols])):
            value = K.add(value, K.mul((a0, a1), e))
        return value


# ---- the verifier of a folded opening --------------------------------------------------------------------------------

class FoldMismatch(Error):
    """two opened layers disagree: the fold of a layer's pair is not the next layer's word, or the last fold is not the final value"""

    def __init__(self, query, layer, folded, found):
        super().__init__("Query %d: layer %d folds to %d, the next layer holds %d" % (query, layer, folded, found))
        self.query, self.layer, self.folded, self.found = query, layer, folded, found


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim of the sumcheck"""

    def __init__(self, round_index, claim, total):
        super().__init__("Round %d: H(0) + H(1) is %d, the claim is %d" % (round_index, total, claim))
        self.round, self.claim, self.total = round_index, claim, total


def pair_digest(field, pair):
    """the leaf of a layer: the column leaf of its two words"""
    return column_digest(field, pair)


class FoldVerifier:
    """The verifier of one folded opening.  Pure host code: draw_gamma, receive_claims, draw_beta, round (once per round, in
    order), receive_final, draw_queries, verify - in that order."""

    def __init__(self, field, num_vars, log_cols, log_blowup, root, queries, arities=None):
        if not 1 <= log_cols <= num_vars or log_blowup not in (1, 2):
            raise ValueError("log_cols must be in 1..num_vars (log_cols = 0: the plain opening) and log_blowup 1 or 2")
        self.arities = None if arities is None else _schedule(log_cols, arities)      # None: the binary opening and its tuple shapes
        self.schedule = _schedule(log_cols, arities)
        self.starts = _stage_starts(self.schedule)
        self.field, self.num_vars, self.log_cols, self.log_blowup = field, num_vars, log_cols, log_blowup
        self.log_rows = num_vars - log_cols
        self.log_len = log_cols + log_blowup
        self.root, self.queries = bytes(root), int(queries)
        self.omega = root_of_unity(field, self.log_len)
        self.half = field.inv(field.add(field.one, field.one))
        self.gamma = self.claims = self.beta = self.claim = self.final = self.indices = None
        self.rounds, self.roots, self.alphas = [], [], []

    def draw_gamma(self, rng):
        self.gamma = [_draw(self.field, rng) for _ in range(1 << self.log_rows)]
        return list(self.gamma)

    def receive_claims(self, v, v_gamma):
        if self.gamma is None:
            raise Error("receive_claims before draw_gamma")
        self.claims = (int(v), int(v_gamma))

    def draw_beta(self, rng):
        if self.claims is None:
            raise Error("draw_beta before receive_claims: beta must be drawn after the prover has sent v and v_gamma")
        F = self.field
        self.beta = _draw(F, rng)
        self.claim = F.add(self.claims[0], F.mul(self.beta, self.claims[1]))
        return self.beta

    def _at(self, evals, x):
        """the quadratic through (0, e0), (1, e1), (2, e2) at x"""
        F = self.field
        e0, e1, e2 = evals
        two = F.add(F.one, F.one)
        xm1, xm2 = F.sub(x, F.one), F.sub(x, two)
        l0 = F.mul(F.mul(xm1, xm2), self.half)
        l1 = F.neg(F.mul(x, xm2))
        l2 = F.mul(F.mul(x, xm1), self.half)
        return F.add(F.add(F.mul(e0, l0), F.mul(e1, l1)), F.mul(e2, l2))

    def round(self, i, evals, root, rng):
        """round i's message: the three sums and, where i starts a stage s >= 1 (the binary opening: every i >= 1), the stage's
        root.  Returns alpha_i"""
        F = self.field
        if self.beta is None or i != len(self.rounds) or i >= self.log_cols:
            raise Error("round %d out of order" % i)
        if (root is None) != (i == 0 or i not in self.starts):
            raise Error("round 0 carries no root, every later round one" if self.arities is None else
                        "round %d: a root comes with the first round of every stage after the first, and with no other" % i)
        evals = [int(x) for x in evals]
        total = F.add(evals[0], evals[1])
        if total != self.claim:
            raise RoundMismatch(i, self.claim, total)
        alpha = _draw(F, rng)
        self.claim = self._at(evals, alpha)
        self.rounds.append(evals)
        if root is not None:
            self.roots.append(bytes(root))
        self.alphas.append(alpha)
        return alpha

    def receive_final(self, final):
        if len(self.rounds) != self.log_cols:
            raise Error("receive_final before the last round")
        self.final = int(final)

    def draw_queries(self, rng):
        """`queries` indices in [0, L / 2^a_0), with replacement; only after the prover is bound to every layer and the final value"""
        if self.final is None:
            raise Error("draw_queries before receive_final: the indices must be drawn after the prover has sent every root and the final value")
        half = 1 << (self.log_len - self.schedule[0])
        self.indices = [rng.randrange(half) if hasattr(rng, "randrange") else self.field.to_int(rng.draw()) % half for _ in range(self.queries)]
        return list(self.indices)

    def _fold(self, pair, alpha, layer, j):
        """the fold of layer `layer`'s pair at x = w_(l0 - layer)^j"""
        F = self.field
        L = 1 << self.log_len
        xinv = F.from_int(pow(F.to_int(self.omega), (L - (j << layer)) % L, F.p))
        even = F.mul(F.add(pair[0], pair[1]), self.half)
        odd = F.mul(F.mul(F.sub(pair[0], pair[1]), self.half), xinv)
        return F.add(even, F.mul(alpha, F.sub(odd, even)))

    def verify(self, point, openings):
        """check the last round against the final value and every query's openings; returns v, the value of the committed
        polynomial at `point`"""
        F = self.field
        c, l0 = self.log_cols, self.log_len
        if self.indices is None:
            raise Error("verify before draw_queries")
        if len(point) != self.num_vars:
            raise Error("the point has %d coordinates, the polynomial %d variables" % (len(point), self.num_vars))
        if len(openings) != len(self.indices):
            raise MerkleMismatch("%d openings for %d drawn indices" % (len(openings), len(self.indices)))
        # H_(c-1)(alpha_(c-1)) = final * eq(z_lo, alpha)
        eq = F.one
        for z, a in zip(list(point)[:c], self.alphas):
            za = F.mul(z, a)
            eq = F.mul(eq, F.add(F.sub(F.sub(F.one, z), a), F.add(za, za)))
        if F.mul(self.final, eq) != self.claim:
            raise EvalMismatch(F.mul(self.final, eq), self.claim)
        weights = [F.add(e, F.mul(self.beta, g)) for e, g in zip(eq_weights(F, list(point)[c:]), self.gamma)]
        ar, starts = self.schedule, self.starts
        S = len(ar)
        stride0 = 1 << (l0 - ar[0])
        for k, (want, opening) in enumerate(zip(self.indices, openings)):
            if self.arities is None:
                q, col_lo, col_hi, stages = opening
                cols = [col_lo, col_hi]
            else:
                q, cols, stages = opening
            if q != want or len(stages) != S - 1 or len(cols) != 1 << ar[0]:
                raise MerkleMismatch("the opening is of index %d, the drawn index is %d" % (q, want))
            words = []
            for t, (j, values, path) in enumerate(cols):
                index = want + t * stride0
                if j != index or path.index != index:
                    raise MerkleMismatch("the opening is of column %d, the drawn column is %d" % (j, index))
                if len(values) != 1 << self.log_rows or len(path.siblings) != l0:
                    raise MerkleMismatch("an opening of the wrong shape")
                if not ColumnPath(index, path.siblings, F).verify_column(self.root, values):
                    raise MerkleMismatch("the opening of column %d does not lead to the committed root" % index)
                u = 0
                for wt, val in zip(weights, values):
                    u = F.add(u, F.mul(wt, int(val)))
                words.append(u)                                   # U_0[index]
            for s in range(S):
                i, a = starts[s], ar[s]
                stride = 1 << (l0 - i - a)                        # stage s's words sit at j + t stride, t < 2^a
                j = want % stride
                for l in range(a):                                # a successive folds: the words t and t + 2^(a-1-l) at level l
                    h = 1 << (a - 1 - l)
                    words = [self._fold((words[t], words[t + h]), self.alphas[i + l], i + l, j + t * stride) for t in range(h)]
                folded = words[0]
                if s == S - 1:
                    if folded != self.final:
                        raise FoldMismatch(k, i, folded, self.final)
                    break
                nxt, siblings = stages[s]
                nxt = [int(x) for x in nxt]
                an = ar[s + 1]
                depth = l0 - starts[s + 1] - an
                jn = want % (1 << depth)
                if len(nxt) != 1 << an or len(siblings) != depth or \
                        Path(jn, siblings).root_from_digest(column_digest(F, nxt)) != self.roots[s]:
                    raise MerkleMismatch("query %d: the opening of layer %d does not lead to its root" % (k, starts[s + 1]))
                found = nxt[j >> depth]
                if folded != found:
                    raise FoldMismatch(k, i, folded, found)
                words = nxt
        return self.claims[0]


def open_folded(prover, verifier, point, rng):
    """the whole exchange of a folded opening between a Prover and a FoldVerifier, under the verifier's schedule if it has one;
    returns what verify returns"""
    gamma = verifier.draw_gamma(rng)
    opening = prover.fold_begin(point, gamma, verifier.arities)
    try:
        verifier.receive_claims(*opening.claims)
        beta = verifier.draw_beta(rng)
        _, _, _, final = opening.prove(beta, lambda i, evals, root: verifier.round(i, evals, root, rng))
        verifier.receive_final(final)
        return verifier.verify(point, opening.query(verifier.draw_queries(rng)))
    finally:
        opening.close()
