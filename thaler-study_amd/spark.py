"""SPARK over LogUp: a sparse matrix committed once, and the proof of v = sum_k val_k U[row_k] W[col_k] whose verifier holds the
five roots of the matrix and never reads it (Setty, "Spartan", section 7; with the offline memory check replaced by an indexed
LogUp lookup whose read counts are multiplicities, as in Setty, Thaler and Wahby, "Lasso", section 4; the lookup itself is
logup.py's fraction sum).

csrc/kernels/spark.hpp states the protocol; DESIGN.md section 9 item 18 describes the kernels.  In short, with the list of triples
padded by (0, 0, 0) to N = 2^l entries, the tables row, col, val (l variables), cr[i] = #{k : row_k = i} (a variables) and
cc[j] = #{k : col_k = j} (b variables) committed once, and U, W tables whose extensions the verifier evaluates itself:

  1. P gathers er[k] = U[row_k], ec[k] = W[col_k], commits to both, sends the two roots and v
  2. cubic sumcheck, l rounds of four values over sum_x val(x) er(x) ec(x) = v, ends at r; P sends f_v, f_r, f_c;
     V checks f_v f_r f_c against the last claim
  3. V draws beta, then alpha; per dimension (idx, e, T, cnt) = (row, er, U, cr), (col, ec, W, cc): the fraction sums of
     (1, alpha - idx_k - beta e[k]) and (cnt_i, alpha - i - beta T[i]); V refuses a zero denominator and P_w Q_t != P_t Q_w;
     the w side ends at z with a = 1 and b = alpha - idx~(z) - beta e~(z), the t side at z' with a' = cnt~(z') and
     b' = alpha - id~(z') - beta T~(z')
  4. nine openings: val, er, ec at r; er, row at z_row; ec, col at z_col; cr at z'_row; cc at z'_col

Field elements are Montgomery words, as everywhere in this package.  Nothing beyond the papers' statements is claimed: no
security level, no zero knowledge, no Fiat-Shamir.

  SparseCommitment                       sc_spark_create and the five ligero_pcs.Prover commitments
  gather, denominators, product3_prove   sc_spark_gather, sc_spark_denominators, sc_product3_prove
  table_eq                               sc_table_eq: eq(r, .) as a device table
  Prover, Verifier, prove_eval           the exchange"""
import ctypes

import numpy as np

from . import ligero_pcs, logup
from ._lib import DRAW4_FN, u64, voidp
from .dense_mle import DenseMultilinearExtension, _u64p, _words
from .grand_product import Verifier as _GpVerifier
from .relaxed_pcs import Error, _draw

MAX_LOG = 28           # kSparkMaxLog of csrc/kernels/spark.hpp
TABLES = ("row", "col", "val", "cr", "cc")      # SC_SPARK_ROW .. SC_SPARK_CC
DIMS = ("row", "col")
# (table, point) of the nine openings, in the order they are made
OPENINGS = (("val", "r"), ("er", "r"), ("ec", "r"), ("er", "z_row"), ("row", "z_row"), ("ec", "z_col"), ("col", "z_col"), ("cr", "zt_row"),
            ("cc", "zt_col"))


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial of the triple-product sumcheck is not the running claim (round 0: not v)"""

    def __init__(self, round_index, claim, total):
        super().__init__("Round %d: H(0) + H(1) is %d, the claim is %d" % (round_index, total, claim))
        self.round, self.claim, self.total = round_index, claim, total


class FinalMismatch(Error):
    """f_v f_r f_c is not the last claim of the triple-product sumcheck"""

    def __init__(self, claim, value):
        super().__init__("The last claim is %d, f_v f_r f_c is %d" % (claim, value))
        self.claim, self.value = claim, value


class LookupMismatch(Error):
    """the two fraction sums of a dimension differ, or one of their denominators is 0"""

    def __init__(self, dim, root_w, root_t):
        super().__init__("Dimension %s: the fraction sums are %r and %r" % (dim, root_w, root_t))
        self.dim, self.root_w, self.root_t = dim, root_w, root_t


class NumeratorMismatch(Error):
    """the last claim about the all-ones numerator of a dimension's w side is not 1"""

    def __init__(self, dim, claim):
        super().__init__("Dimension %s: the last claim about the all-ones numerator is %d" % (dim, claim))
        self.dim, self.claim = dim, claim


class InputMismatch(Error):
    """an opened value, or a value the verifier computes itself, is not what the transcript claims.  which: "val", "er", "ec" (the
    finals at r), "den_w row", "den_w col" (alpha - idx~(z) - beta e~(z)), "cr", "cc" (the counts at z'), "u", "w" (alpha - id~(z') -
    beta T~(z') with the verifier's own T~)"""

    def __init__(self, which, claim, value):
        super().__init__("%s: the claim is %d, the value is %d" % (which, claim, value))
        self.which, self.claim, self.value = which, claim, value


def log_len(nnz):
    """l = max(1, ceil(log2 nnz))"""
    return max(1, (int(nnz) - 1).bit_length())


def min_modulus_log(a, b, ell):
    """indices and counts are field words: p must exceed 2^max(l, a, b)"""
    return max(a, b, ell)


# ---- the device side -------------------------------------------------------------------------------------------------

def default_commit(log_blowup=1, code="rs"):
    """commit(table) -> ligero_pcs.Prover with half of the variables in the columns (ligero_pcs.default_log_cols: at least one
    for tables of one variable or more, so that a folded opening exists; at most what one launch encodes)"""
    def commit(table):
        return ligero_pcs.Prover.commit(table.ctx, table, log_cols=ligero_pcs.default_log_cols(table.num_vars(), log_blowup, code),
                                        log_blowup=log_blowup, code=code)
    return commit


def opening_verifier(field, prover, queries=8, folded=False):
    """the verifier of the openings of a ligero_pcs.Prover commitment, from its public shape and root"""
    if folded:
        return ligero_pcs.FoldVerifier(field, prover.num_vars, prover.log_cols, prover.log_blowup, prover.root(), queries)
    return ligero_pcs.Verifier(field, prover.num_vars, prover.log_cols, prover.log_blowup, prover.root(), queries, code=prover.code)


class SparseCommitment:
    """sc_spark_create: the matrix of 2^a x 2^b from rows, cols (integers) and vals (Montgomery words) on the device, and the five
    commitments of the preprocessing.  commit(table) -> ligero_pcs.Prover (default_commit()); commit=False: none (the device object
    alone).  .tables and .pcs are keyed by TABLES"""

    def __init__(self, ctx, a, b, rows, cols, vals, commit=None):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        if not (rows.ndim == cols.ndim == vals.ndim == 1 and rows.size == cols.size == vals.size):
            raise ValueError("rows, cols and vals are three lists of one length")
        self.ctx, self.a, self.b, self.nnz, self.ell = ctx, int(a), int(b), int(rows.size), log_len(max(rows.size, 1))
        self.h, self.tables, self.pcs = voidp(), {}, {}
        u32p = ctypes.POINTER(ctypes.c_uint32)
        ctx.check(ctx.lib.sc_spark_create(ctx.h, self.a, self.b, rows.ctypes.data_as(u32p), cols.ctypes.data_as(u32p), _u64p(vals), rows.size,
                                          ctypes.byref(self.h)))
        try:
            self.commit = default_commit() if commit is None else commit
            if commit is not False:
                for name in TABLES:
                    self.tables[name] = self.table(name)
                    self.pcs[name] = self.commit(self.tables[name])
        except BaseException:
            self.close()
            raise

    def table(self, which):
        """a copy of row, col, val, cr or cc as a device table"""
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_spark_table(self.ctx.h, self.h, TABLES.index(which) if which in TABLES else int(which), ctypes.byref(h)))
        return DenseMultilinearExtension(self.ctx, h)

    def roots(self):
        """{table: root}: what the verifier holds of the matrix"""
        return {name: bytes(self.pcs[name].root()) for name in TABLES}

    def verifiers(self, queries=8, folded=False):
        """{table: the verifier of its openings}, as a verifier that holds the five roots builds them"""
        return {name: opening_verifier(self.ctx.field, self.pcs[name], queries, folded) for name in TABLES}

    def close(self):
        for p in self.pcs.values():
            p.close()
        self.pcs, self.tables = {}, {}
        if self.h and self.ctx.h:
            self.ctx.lib.sc_spark_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gather(ctx, sp, u, w):
    """sc_spark_gather: (er, ec) with er[k] = u[row_k], ec[k] = w[col_k]"""
    er, ec = voidp(), voidp()
    ctx.check(ctx.lib.sc_spark_gather(ctx.h, sp.h, u.h, w.h, ctypes.byref(er), ctypes.byref(ec)))
    return DenseMultilinearExtension(ctx, er), DenseMultilinearExtension(ctx, ec)


def denominators(ctx, sp, dim, t, e, alpha, beta):
    """sc_spark_denominators of dim ("row" / 0, "col" / 1): (den_w, den_t) with den_w[k] = alpha - idx_k - beta e[k] and
    den_t[i] = alpha - i - beta t[i]"""
    dw, dt = voidp(), voidp()
    d = DIMS.index(dim) if dim in DIMS else int(dim)
    ctx.check(ctx.lib.sc_spark_denominators(ctx.h, sp.h, d, t.h, e.h, int(alpha), int(beta), ctypes.byref(dw), ctypes.byref(dt)))
    return DenseMultilinearExtension(ctx, dw), DenseMultilinearExtension(ctx, dt)


def table_eq(ctx, r):
    """sc_table_eq: eq(r, .) as a device table of 2^len(r) words"""
    words = _words(r)
    h = voidp()
    ctx.check(ctx.lib.sc_table_eq(ctx.h, _u64p(words), words.size, ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


def product3_prove(ctx, a, b, c, draw=None, seed_r=0):
    """sc_product3_prove: the cubic sumcheck over sum_x a(x) b(x) c(x).  draw(round, [H(0), H(1), H(2), H(3)]) returns the round's
    challenge; None: the synthetic challenger of sc_prove over seed_r.
    Returns (c1, rounds[n][4], challenges[n], (f_a, f_b, f_c))"""
    n = a.num_vars()
    evals, ch, fin, c1 = np.zeros(4 * max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(3, dtype=np.uint64), u64()
    failure = []

    def cb(_user, j, e):
        try:
            return int(draw(int(j), [int(e[k]) for k in range(4)]))
        except BaseException as exc:      # an exception must not cross the C frames: the call ends, and it is raised again below
            failure.append(exc)
            return ctx.field.p
    rc = ctx.lib.sc_product3_prove(ctx.h, a.h, b.h, c.h, DRAW4_FN(cb) if draw is not None else ctypes.cast(None, DRAW4_FN), None, int(seed_r),
                                   ctypes.byref(c1), _u64p(evals), _u64p(ch), _u64p(fin))
    if failure:
        raise failure[0]
    ctx.check(rc)
    return (int(c1.value), [[int(x) for x in evals[4 * j:4 * j + 4]] for j in range(n)], [int(x) for x in ch[:n]], tuple(int(x) for x in fin))


class Prover:
    """The prover of one evaluation over a SparseCommitment, U and W (device tables of 2^a and 2^b words).  Steps, in the
    protocol's order: gather_commit, sumcheck, lookup_roots(dim, alpha, beta), lookup_prove(dim, side, draw), then the nine
    openings through .pcs (keyed by table name)"""

    def __init__(self, commitment, U, W, commit=None):
        self.ctx, self.sc, self.U, self.W = commitment.ctx, commitment, U, W
        self.commit = commit or commitment.commit
        self.pcs = dict(commitment.pcs)
        self.own, self.er, self.ec, self.trees, self.dens = [], None, None, {}, {}

    def gather_commit(self):
        """step 1, the roots: (root of er, root of ec)"""
        self.er, self.ec = gather(self.ctx, self.sc, self.U, self.W)
        for name, t in (("er", self.er), ("ec", self.ec)):
            self.pcs[name] = self.commit(t)
            self.own.append(self.pcs[name])
        return bytes(self.pcs["er"].root()), bytes(self.pcs["ec"].root())

    def sumcheck(self, receive_claim, draw):
        """step 1's v and step 2: v = H_0(0) + H_0(1) goes to receive_claim(v) before the first round's values go to
        draw(round, four values) -> r_j.  Returns (f_v, f_r, f_c)"""
        sent = []

        def relay(j, e):
            if not sent:
                sent.append(True)
                receive_claim(self.ctx.field.add(e[0], e[1]))
            return draw(j, e)
        _, _, self.r, finals = product3_prove(self.ctx, self.sc.tables["val"], self.er, self.ec, relay)
        return finals

    def lookup_roots(self, dim, alpha, beta):
        """step 3 of one dimension: the denominators and the two trees; returns ((P_w, Q_w), (P_t, Q_t))"""
        T, e, cnt = (self.U, self.er, "cr") if dim == "row" else (self.W, self.ec, "cc")
        self._drop(dim)
        self.dens[dim] = denominators(self.ctx, self.sc, dim, T, e, alpha, beta)
        self.trees[dim] = [logup.FractionTree(self.ctx, self.dens[dim][0]), logup.FractionTree(self.ctx, self.dens[dim][1], self.sc.tables[cnt])]
        return tuple(t.root for t in self.trees[dim])

    def lookup_prove(self, dim, side, draw):
        """the fraction sum of side 0 (w) or 1 (t) of a dimension under draw (logup.prove)"""
        return logup.prove(self.trees[dim][side], draw)

    def _drop(self, dim):
        for t in self.trees.pop(dim, []):
            t.close()
        self.dens.pop(dim, None)

    def close(self):
        for dim in DIMS:
            self._drop(dim)
        for p in self.own:
            p.close()
        self.own, self.er, self.ec = [], None, None


# ---- the verifier ----------------------------------------------------------------------------------------------------

class Verifier:
    """The verifier of one evaluation: pure host code over the verifiers of the openings of the five committed tables
    (pcs_verifiers, keyed by TABLES; only their num_vars is read here) and the callbacks u_eval(point), w_eval(point) = U~, W~.
    receive_commitments, receive_claim, round (l times), receive_finals, draw_lookup, then per dimension receive_roots and the two
    fraction sums (frac[dim][side].challenger), then openings() and finish(values) - in that order."""

    _cubic_at = _GpVerifier._cubic_at

    def __init__(self, field, a, b, ell, pcs_verifiers, u_eval, w_eval):
        if not (1 <= a <= MAX_LOG and 1 <= b <= MAX_LOG and 1 <= ell <= MAX_LOG):
            raise ValueError("a, b and l must be in 1..%d" % MAX_LOG)
        if field.p <= 3 or field.p <= 1 << min_modulus_log(a, b, ell):
            raise ValueError("p = %d: indices and counts of up to 2^%d must be field words, and the cubic through 0, 1, 2, 3 needs 2 and 3 "
                             "invertible" % (field.p, max(a, b, ell)))
        want = {"row": ell, "col": ell, "val": ell, "cr": a, "cc": b}
        for name, n in want.items():
            if pcs_verifiers[name].num_vars != n:
                raise ValueError("the commitment to %s is over %d variables, not %d" % (name, pcs_verifiers[name].num_vars, n))
        self.field, self.a, self.b, self.ell = field, a, b, ell
        self.pcs = dict(pcs_verifiers)
        self.evals = {"row": u_eval, "col": w_eval}
        self.inv2, self.inv6 = field.inv(field.from_int(2)), field.inv(field.from_int(6))
        self.claim = self.v = self.finals = self.alpha = self.beta = None
        self.r, self.frac, self.stage = [], {}, 0

    def receive_commitments(self, pcs_er, pcs_ec):
        """step 1: the verifiers of the openings of er and ec, built over the roots P sent"""
        if self.stage != 0 or pcs_er.num_vars != self.ell or pcs_ec.num_vars != self.ell:
            raise Error("the commitments to er and ec come first and are over l = %d variables" % self.ell)
        self.pcs["er"], self.pcs["ec"] = pcs_er, pcs_ec
        self.stage = 1

    def receive_claim(self, v):
        if self.stage != 1:
            raise Error("v after the roots of er and ec, once")
        self.v = self.claim = int(v)
        self.stage = 2

    def round(self, j, values, rng):
        F = self.field
        if self.stage != 2 or j != len(self.r) or j >= self.ell or len(values) != 4:
            raise Error("round %d out of order" % j)
        total = F.add(int(values[0]), int(values[1]))
        if total != self.claim:
            raise RoundMismatch(j, self.claim, total)
        r = _draw(F, rng)
        self.claim = self._cubic_at(values, r)
        self.r.append(r)
        return r

    def receive_finals(self, f_v, f_r, f_c):
        F = self.field
        if self.stage != 2 or len(self.r) != self.ell:
            raise Error("the finals before the last round")
        value = F.mul(F.mul(int(f_v), int(f_r)), int(f_c))
        if value != self.claim:
            raise FinalMismatch(self.claim, value)
        self.finals = (int(f_v), int(f_r), int(f_c))
        self.stage = 3

    def draw_lookup(self, rng):
        """step 3: beta, then alpha - after the roots of step 1 and the finals.  Returns (alpha, beta)"""
        if self.stage != 3:
            raise Error("alpha and beta are drawn after the finals")
        self.beta = _draw(self.field, rng)
        self.alpha = _draw(self.field, rng)
        self.stage = 4
        return self.alpha, self.beta

    def receive_roots(self, dim, root_w, root_t):
        """Q_w != 0, Q_t != 0 and P_w Q_t = P_t Q_w; then the two fraction sums of the dimension may run"""
        F = self.field
        if self.stage != 4 or dim not in DIMS or dim in self.frac:
            raise Error("the roots of dimension %s out of order" % dim)
        (pw, qw), (pt, qt) = (tuple(int(x) for x in root_w), tuple(int(x) for x in root_t))
        if qw == 0 or qt == 0 or F.mul(pw, qt) != F.mul(pt, qw):
            raise LookupMismatch(dim, (pw, qw), (pt, qt))
        self.frac[dim] = (logup.Verifier(F, self.ell, ones=True), logup.Verifier(F, self.a if dim == "row" else self.b))
        self.frac[dim][0].begin(pw, qw)
        self.frac[dim][1].begin(pt, qt)

    def openings(self):
        """[(table, point name, point)] of the nine openings, in the order of OPENINGS"""
        if self.stage != 4 or len(self.frac) != 2 or any(fv.layer != fv.n for pair in self.frac.values() for fv in pair):
            raise Error("the openings after the fraction sums of both dimensions")
        pts = {"r": list(self.r)}
        for dim in DIMS:
            pts["z_" + dim] = list(self.frac[dim][0].z)
            pts["zt_" + dim] = list(self.frac[dim][1].z)
        return [(table, at, pts[at]) for table, at in OPENINGS]

    def finish(self, opened):
        """opened[(table, point name)] = the nine values the openings' verifiers accepted.  True, or the error of the first check
        that fails: the finals at r, then per dimension the w side and the t side"""
        F = self.field
        for k, name in enumerate(("val", "er", "ec")):
            if int(opened[(name, "r")]) != self.finals[k]:
                raise InputMismatch(name, self.finals[k], int(opened[(name, "r")]))
        for dim in DIMS:
            e, cnt = ("er", "cr") if dim == "row" else ("ec", "cc")
            try:
                _, _, b = self.frac[dim][0].result()
            except logup.NumeratorMismatch as exc:
                raise NumeratorMismatch(dim, exc.claim) from None
            value = F.sub(F.sub(self.alpha, int(opened[(dim, "z_" + dim)])), F.mul(self.beta, int(opened[(e, "z_" + dim)])))
            if value != b:
                raise InputMismatch("den_w " + dim, b, value)
            zt, a_t, b_t = self.frac[dim][1].result()
            if int(opened[(cnt, "zt_" + dim)]) != a_t:
                raise InputMismatch(cnt, a_t, int(opened[(cnt, "zt_" + dim)]))
            value = F.sub(F.sub(self.alpha, logup.range_table_eval(F, zt)), F.mul(self.beta, int(self.evals[dim](zt))))
            if value != b_t:
                raise InputMismatch("u" if dim == "row" else "w", b_t, value)
        self.stage = 5
        return True


def prove_eval(commitment, pcs_verifiers, U, W, u_eval, w_eval, rng, verifier_of=None, commit=None):
    """the whole exchange over a SparseCommitment: pcs_verifiers = the verifiers of the openings of its five tables (built over
    the five roots: commitment.verifiers()), U and W device tables, u_eval and w_eval the verifier's own U~ and W~.
    verifier_of(prover) -> the verifier of the openings of er's and ec's commitments (default: opening_verifier with the number of
    queries and the kind - plain or folded - of the verifier of val).  Openings go through r1cs.open_committed: plain, folded or
    expander code.  Returns v, the value the verifier accepted, or raises the verifier's error"""
    from . import r1cs
    ctx, F = commitment.ctx, commitment.ctx.field
    if verifier_of is None:
        like = pcs_verifiers["val"]
        verifier_of = lambda p: opening_verifier(F, p, like.queries, isinstance(like, ligero_pcs.FoldVerifier))   # noqa: E731
    V = Verifier(F, commitment.a, commitment.b, commitment.ell, pcs_verifiers, u_eval, w_eval)
    P = Prover(commitment, U, W, commit)
    try:
        P.gather_commit()                                                     # 1
        V.receive_commitments(verifier_of(P.pcs["er"]), verifier_of(P.pcs["ec"]))
        V.receive_finals(*P.sumcheck(V.receive_claim, lambda j, e: V.round(j, e, rng)))   # 1 (v), 2
        alpha, beta = V.draw_lookup(rng)                                      # 3
        for dim in DIMS:
            V.receive_roots(dim, *P.lookup_roots(dim, alpha, beta))
            for side in range(2):
                P.lookup_prove(dim, side, V.frac[dim][side].challenger(rng))
        opened = {}
        for table, at, point in V.openings():                                 # 4
            ver = V.pcs[table] if table in TABLES else verifier_of(P.pcs[table])      # er and ec are opened twice: a verifier each
            opened[(table, at)] = r1cs.open_committed(P.pcs[table], ver, point, rng)
        V.finish(opened)
    finally:
        P.close()
    return V.v


def prove_eval_batched(commitment, pcs_verifiers, U, W, u_eval, w_eval, rng, verifier_of=None, commit=None, extra=None, groups=None):
    """prove_eval with batched openings (multiopen.py): after the fraction sums P sends the nine values,
    V runs finish on them as claimed values, and multiopen.prove_claims proves the nine claims - one joint opening per commitment
    shape with several claims (the tables of l variables; more where a or b equals l and the shapes agree), the single opening for
    the rest.  The verifiers are plain ligero_pcs.Verifier objects: a FoldVerifier is refused with a ValueError.
    extra = (provers, verifiers, claims): further commitments and multiopen.Claim's that join the list (r1cs: the witness).
    groups: a list that receives prove_claims' groups.  Returns v, the value the verifier accepted, or raises the verifier's error"""
    from . import multiopen
    ctx, F = commitment.ctx, commitment.ctx.field
    if any(isinstance(v, ligero_pcs.FoldVerifier) for v in pcs_verifiers.values()):
        raise ValueError("batched openings take the plain ligero_pcs.Verifier: a joint folded opening is out of scope")
    if verifier_of is None:
        like = pcs_verifiers["val"]
        verifier_of = lambda p: opening_verifier(F, p, like.queries, False)   # noqa: E731
    V = Verifier(F, commitment.a, commitment.b, commitment.ell, pcs_verifiers, u_eval, w_eval)
    P = Prover(commitment, U, W, commit)
    try:
        P.gather_commit()                                                     # 1
        V.receive_commitments(verifier_of(P.pcs["er"]), verifier_of(P.pcs["ec"]))
        V.receive_finals(*P.sumcheck(V.receive_claim, lambda j, e: V.round(j, e, rng)))   # 1 (v), 2
        alpha, beta = V.draw_lookup(rng)                                      # 3
        for dim in DIMS:
            V.receive_roots(dim, *P.lookup_roots(dim, alpha, beta))
            for side in range(2):
                P.lookup_prove(dim, side, V.frac[dim][side].challenger(rng))
        tables = dict(commitment.tables, er=P.er, ec=P.ec)
        claims = [multiopen.Claim(table, point, tables[table].evaluate(point)) for table, _, point in V.openings()]   # 4: P's nine values
        V.finish({(table, at): c.value for (table, at), c in zip(OPENINGS, claims)})
        provers, verifiers = dict(P.pcs), dict(V.pcs)
        if extra is not None:
            provers.update(extra[0])
            verifiers.update(extra[1])
            claims += [multiopen.Claim(*c) for c in extra[2]]
        multiopen.prove_claims(ctx, provers, verifiers, claims, rng, groups)
    finally:
        P.close()
    return V.v
