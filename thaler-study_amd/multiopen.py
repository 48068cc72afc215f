"""Batched openings: many evaluation claims about Ligero-committed tables, one joint opening per commitment shape.

csrc/kernels/multiopen.hpp states the protocol; DESIGN.md section 9 item 19 describes the kernels.  In short, for a GROUP of T <= 8
commitments of one shape (num_vars n, log_cols c, log_blowup, code) with roots root_t and K <= 16 claims f_(t_k)(r_k) = v_k:

  1. V draws rho; claim k gets the coefficient rho^k
  2. P forms E_t(x) = sum_{k : t_k = t} rho^k eq(r_k, x), one weight table per committed table (sc_table_eq_sum)
  3. sumcheck, n rounds of three values over sum_x sum_t f_t(x) E_t(x) = sum_k rho^k v_k (sc_sumprod_prove), ends at z with claim c
  4. no finals: V computes e_t = E_t(z) itself; what remains is sum_t e_t f_t(z) = c
  5. joint opening: V draws gamma (T vectors of 2^R words); P sends u_gamma = sum_t sum_i gamma[t][i] row_(t,i) and
     u_z = sum_t e_t sum_i eq(z[c:], i) row_(t,i); V checks <u_z, eq(z[:c])> = c, draws ONE list of column indices, P opens those
     columns of every commitment, V checks the T paths and the two combinations per column

Field elements are Montgomery words, as everywhere in this package.  Nothing beyond the statements of the underlying arguments is
claimed: no security level, no zero knowledge, no Fiat-Shamir.  A joint FOLDED opening (one Basefold run over the T codewords) is
out of scope: the batched functions refuse a ligero_pcs.FoldVerifier.

  table_eq_sum, sumprod_prove            sc_table_eq_sum, sc_sumprod_prove
  Claim, group_claims                    a claim (table name, point, value); the claims grouped by commitment shape
  Prover, Verifier                       the two sides of one group's exchange
  prove_claims                           the whole exchange for any list of claims
  batch_opening_bytes                    the size of one group's messages"""
import collections
import ctypes

import numpy as np

from . import expander_code, ligero_pcs
from ._lib import DRAW_FN, u64, voidp
from .dense_mle import DenseMultilinearExtension, _u64p, _words
from .relaxed_pcs import Error, EvalMismatch, _draw
from .relaxed_pcs import MerkleMismatch as _MerkleMismatch

MAX_TABLES = 8         # kSumprodMaxPairs of csrc/kernels/multiopen.hpp
MAX_CLAIMS = 16        # kEqSumMaxCount
MAX_LOG = 28           # kEqSumMaxLog
LO_LOG = 7             # kEqSumLoLog: the low index bits of eq_sum_kernel

ProximityMismatch = ligero_pcs.ProximityMismatch

Claim = collections.namedtuple("Claim", ["table", "point", "value"])
Claim.__doc__ = "the claim table~(point) = value: `table` names a commitment, point and value are Montgomery words"


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial of the combining sumcheck is not the running claim (round 0: not sum_k rho^k v_k)"""

    def __init__(self, round_index, claim, total):
        super().__init__("Round %d: H(0) + H(1) is %d, the claim is %d" % (round_index, total, claim))
        self.round, self.claim, self.total = round_index, claim, total


class FinalMismatch(Error):
    """<u_z, eq(z[:c])> is not the last claim of the combining sumcheck"""

    def __init__(self, claim, value):
        super().__init__("The last claim is %d, <u_z, eq(z[:c])> is %d" % (claim, value))
        self.claim, self.value = claim, value


class MerkleMismatch(_MerkleMismatch):
    """an opened column of the commitment `table` does not lead to its root, or is not the drawn column"""

    def __init__(self, table, message):
        super().__init__("commitment %r: %s" % (table, message))
        self.table = table


class ClaimMismatch(Error):
    """a claim in a group of its own, opened singly: the opened value is not the claimed one"""

    def __init__(self, table, claim, value):
        super().__init__("%s: the claim is %d, the opened value is %d" % (table, claim, value))
        self.table, self.claim, self.value = table, claim, value


def batch_opening_bytes(num_vars, log_cols, log_blowup, queries, T):
    """bytes of one group's messages: the n round polynomials of three words, the two combined rows of 2^c words, and per query
    and commitment a column of 2^(n - c) words with its path of c + log_blowup digests (ligero_pcs.opening_bytes: one opening)"""
    return 8 * (3 * num_vars + 2 * (1 << log_cols)) + queries * T * (8 * (1 << (num_vars - log_cols)) + 32 * (log_cols + log_blowup))


# ---- the device side -------------------------------------------------------------------------------------------------

def table_eq_sum(ctx, points, coeffs):
    """sc_table_eq_sum: sum_k coeffs[k] eq(points[k], .) as a device table of 2^n words; points: 1..16 lists of n words"""
    points = [list(pt) for pt in points]
    count, n = len(points), len(points[0]) if points else 0
    if any(len(pt) != n for pt in points) or len(coeffs) != count:
        raise ValueError("points are lists of one length, with one coefficient each")
    pts = _words([x for pt in points for x in pt])
    cf = _words(coeffs)
    h = voidp()
    ctx.check(ctx.lib.sc_table_eq_sum(ctx.h, _u64p(pts) if pts.size else None, _u64p(cf) if cf.size else None, count, n, ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


def sumprod_prove(ctx, a_tables, b_tables, draw=None, seed_r=0):
    """sc_sumprod_prove: the sumcheck over sum_x sum_t a_t(x) b_t(x) with one sequence of challenges.  draw(round, [H(0), H(1),
    H(2)]) returns the round's challenge; None: the synthetic challenger of sc_prove over seed_r.
    Returns (c1, rounds[n][3], challenges[n], finals_a[T], finals_b[T])"""
    T = len(a_tables)
    if len(b_tables) != T:
        raise ValueError("as many a tables as b tables")
    n = a_tables[0].num_vars() if T else 0
    ha = (voidp * max(T, 1))(*[t.h for t in a_tables])
    hb = (voidp * max(T, 1))(*[t.h for t in b_tables])
    evals, ch, c1 = np.zeros(3 * max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), u64()
    fa, fb = np.zeros(max(T, 1), dtype=np.uint64), np.zeros(max(T, 1), dtype=np.uint64)
    failure = []

    def cb(_user, j, e):
        try:
            return int(draw(int(j), [int(e[k]) for k in range(3)]))
        except BaseException as exc:      # an exception must not cross the C frames: the call ends, and it is raised again below
            failure.append(exc)
            return ctx.field.p
    rc = ctx.lib.sc_sumprod_prove(ctx.h, T, ha, hb, DRAW_FN(cb) if draw is not None else ctypes.cast(None, DRAW_FN), None, int(seed_r),
                                  ctypes.byref(c1), _u64p(evals), _u64p(ch), _u64p(fa), _u64p(fb))
    if failure:
        raise failure[0]
    ctx.check(rc)
    return (int(c1.value), [[int(x) for x in evals[3 * j:3 * j + 3]] for j in range(n)], [int(x) for x in ch[:n]], [int(x) for x in fa[:T]],
            [int(x) for x in fb[:T]])


# ---- claims and groups -----------------------------------------------------------------------------------------------

def group_claims(claims, shapes):
    """The claims grouped by commitment shape, order kept: [(shape, tables, claims)] with shape = shapes[claim.table] (anything
    hashable), tables the group's table names in the order of their first claim, claims in the order given; the groups in the order
    of their first claim.  A group holds at most MAX_TABLES tables and MAX_CLAIMS claims: a claim that would not fit opens a new
    group of the same shape."""
    groups, open_group = [], {}
    for claim in claims:
        claim = Claim(*claim)
        if claim.table not in shapes:
            raise ValueError("no commitment named %r" % (claim.table,))
        shape = shapes[claim.table]
        g = open_group.get(shape)
        if g is None or len(g[2]) == MAX_CLAIMS or (claim.table not in g[1] and len(g[1]) == MAX_TABLES):
            g = (shape, [], [])
            groups.append(g)
            open_group[shape] = g
        if claim.table not in g[1]:
            g[1].append(claim.table)
        g[2].append(claim)
    return groups


def _check_group(tables, claims):
    """the limits of one group, and that every table carries a claim and every claim names a table"""
    tables, claims = list(tables), [Claim(*c) for c in claims]
    if not 1 <= len(tables) <= MAX_TABLES or len(set(tables)) != len(tables):
        raise ValueError("a group is 1..%d different commitments" % MAX_TABLES)
    if not 1 <= len(claims) <= MAX_CLAIMS:
        raise ValueError("a group carries 1..%d claims" % MAX_CLAIMS)
    for c in claims:
        if c.table not in tables:
            raise ValueError("a claim about %r, which is not a commitment of the group" % (c.table,))
    for t in tables:
        if all(c.table != t for c in claims):
            raise ValueError("the commitment %r of the group carries no claim" % (t,))
    return tables, claims


def _powers(field, rho, count):
    out, x = [], field.one
    for _ in range(count):
        out.append(x)
        x = field.mul(x, rho)
    return out


def _free(table):
    if table is not None and table.h and table.ctx.h:
        table.ctx.lib.sc_table_free(table.ctx.h, table.h)
        table.h = None


class Prover:
    """The prover of one group over `provers`, a dict name -> ligero_pcs.Prover (commitments of one shape).  Steps, in the
    protocol's order: begin(claims, rho), sumcheck(draw), combine(gamma), open_columns(indices), close() - which frees the weight
    tables"""

    def __init__(self, ctx, provers):
        self.ctx, self.field, self.provers = ctx, ctx.field, dict(provers)
        self.tables, self.claims, self.weights, self.z, self.e = [], [], [], None, None

    def begin(self, claims, rho, tables=None):
        """steps 1 and 2: the weight tables E_t under V's rho.  tables: the group's commitments in order (default: in the order of
        their first claim); one that carries no claim is an error"""
        claims = [Claim(*c) for c in claims]
        if tables is None:
            tables = list(dict.fromkeys(c.table for c in claims))
        self.tables, self.claims = _check_group(tables, claims)
        shapes = {(p.num_vars, p.log_cols, p.log_blowup, p.code) for p in (self.provers[t] for t in self.tables)}
        if len(shapes) != 1:
            raise ValueError("the commitments of a group have one shape, not %s" % sorted(shapes))
        self.num_vars, self.log_cols = self.provers[self.tables[0]].num_vars, self.provers[self.tables[0]].log_cols
        if any(len(c.point) != self.num_vars for c in self.claims):
            raise ValueError("every point of the group has %d coordinates" % self.num_vars)
        self.close()
        coeff = _powers(self.field, int(rho), len(self.claims))
        for t in self.tables:
            mine = [k for k, c in enumerate(self.claims) if c.table == t]
            self.weights.append(table_eq_sum(self.ctx, [self.claims[k].point for k in mine], [coeff[k] for k in mine]))

    def sumcheck(self, draw):
        """step 3 under draw(round, three values) -> r_j; returns the rounds' values"""
        _, rounds, self.z, _, self.e = sumprod_prove(self.ctx, [self.provers[t].poly for t in self.tables], self.weights, draw)
        return rounds

    def combine(self, gamma):
        """step 5: (u_gamma, u_z) under V's gamma, one vector of 2^R words per commitment: one sc_ligero_combine_rows call of two
        weight vectors per commitment, the results added on the host.  e_t = E_t(z) is the weight table's final of the sumcheck"""
        F = self.field
        if self.z is None or len(gamma) != len(self.tables):
            raise ValueError("combine after sumcheck, with one gamma vector per commitment")
        eq_rows = ligero_pcs.eq_weights(F, self.z[self.log_cols:])
        u_gamma, u_z = [0] * (1 << self.log_cols), [0] * (1 << self.log_cols)
        for t, g, e in zip(self.tables, gamma, self.e):
            ug, uz = self.provers[t].combine_rows([list(g), [F.mul(e, w) for w in eq_rows]])
            u_gamma = [F.add(x, y) for x, y in zip(u_gamma, ug)]
            u_z = [F.add(x, y) for x, y in zip(u_z, uz)]
        return u_gamma, u_z

    def open_columns(self, indices):
        """{table: [(index, values, ColumnPath)]}: the same columns of every commitment"""
        return {t: self.provers[t].open_columns(indices) for t in self.tables}

    def close(self):
        for w in self.weights:
            _free(w)
        self.weights = []


# ---- the verifier ----------------------------------------------------------------------------------------------------

class Verifier:
    """The verifier of one group.  Pure host code: shape = (num_vars, log_cols, log_blowup), roots = {table: root} in the group's
    order.  draw_rho(claims, rng), round(j, evals, rng) n times, draw_gamma, receive, draw_columns, verify - in that order."""

    def __init__(self, field, shape, roots, queries, code="rs"):
        num_vars, log_cols, log_blowup = (int(x) for x in shape)
        if not 1 <= num_vars <= MAX_LOG:
            raise ValueError("num_vars must be in 1..%d" % MAX_LOG)
        if field.p <= 2:
            raise ValueError("the quadratic through 0, 1, 2 needs 2 invertible")
        # (the shape checks of a single opening's verifier: log_cols, log_blowup, the code and its root of unity)
        self._one = ligero_pcs.Verifier(field, num_vars, log_cols, log_blowup, b"\0" * 32, queries, code=code)
        self.field, self.num_vars, self.log_cols, self.log_blowup, self.code = field, num_vars, log_cols, log_blowup, code
        self.log_rows, self.log_len, self.queries = num_vars - log_cols, log_cols + log_blowup, int(queries)
        self.roots = {t: bytes(r) for t, r in dict(roots).items()}
        self.tables = list(self.roots)
        if not 1 <= len(self.tables) <= MAX_TABLES:
            raise ValueError("a group is 1..%d commitments" % MAX_TABLES)
        self.inv2 = field.inv(field.from_int(2))
        self.claims = self.rho = self.claim = self.e = self.gamma = self.u_gamma = self.u_z = self.columns = None
        self.enc_gamma = self.enc_z = None
        self.z = []

    def draw_rho(self, claims, rng):
        """step 1: rho, after the claims are fixed; the running claim becomes sum_k rho^k v_k"""
        F = self.field
        _, claims = _check_group(self.tables, claims)
        if any(len(c.point) != self.num_vars for c in claims):
            raise ValueError("every point of the group has %d coordinates" % self.num_vars)
        if self.rho is not None:
            raise Error("rho is drawn once")
        self.claims = claims
        self.rho = _draw(F, rng)
        self.coeff = _powers(F, self.rho, len(claims))
        self.claim = 0
        for ck, c in zip(self.coeff, claims):
            self.claim = F.add(self.claim, F.mul(ck, int(c.value)))
        return self.rho

    def _quadratic_at(self, e, x):
        F = self.field
        d = [x, F.sub(x, F.one), F.sub(x, F.from_int(2))]
        l0 = F.mul(F.mul(d[1], d[2]), self.inv2)
        l1 = F.neg(F.mul(d[0], d[2]))
        l2 = F.mul(F.mul(d[0], d[1]), self.inv2)
        return F.add(F.add(F.mul(int(e[0]), l0), F.mul(int(e[1]), l1)), F.mul(int(e[2]), l2))

    def round(self, j, evals, rng):
        F = self.field
        if self.rho is None or j != len(self.z) or j >= self.num_vars or len(evals) != 3:
            raise Error("round %d out of order" % j)
        total = F.add(int(evals[0]), int(evals[1]))
        if total != self.claim:
            raise RoundMismatch(j, self.claim, total)
        r = _draw(F, rng)
        self.claim = self._quadratic_at(evals, r)
        self.z.append(r)
        return r

    def _eq_at(self, a, b):
        F = self.field
        out = F.one
        for x, y in zip(a, b):
            xy = F.mul(int(x), int(y))
            out = F.mul(out, F.add(F.sub(F.sub(F.one, int(x)), int(y)), F.add(xy, xy)))
        return out

    def draw_gamma(self, rng):
        """steps 4 and 5: e_t = sum_{k : t_k = t} rho^k eq(r_k, z), then gamma: one vector of 2^R words per commitment"""
        F = self.field
        if len(self.z) != self.num_vars or self.gamma is not None:
            raise Error("gamma is drawn once, after the last round")
        self.e = []
        for t in self.tables:
            e = 0
            for ck, c in zip(self.coeff, self.claims):
                if c.table == t:
                    e = F.add(e, F.mul(ck, self._eq_at(c.point, self.z)))
            self.e.append(e)
        self.gamma = [[_draw(F, rng) for _ in range(1 << self.log_rows)] for _ in self.tables]
        return [list(g) for g in self.gamma]

    def receive(self, u_gamma, u_z):
        """the two combined rows; <u_z, eq(z[:c])> must be the last claim of the sumcheck"""
        F = self.field
        if self.gamma is None or self.u_gamma is not None:
            raise Error("receive after draw_gamma, once")
        if len(u_gamma) != 1 << self.log_cols or len(u_z) != 1 << self.log_cols:
            raise Error("the combined rows must have 2^log_cols = %d words" % (1 << self.log_cols))
        u_gamma, u_z = [int(x) for x in u_gamma], [int(x) for x in u_z]
        value = 0
        for a, b in zip(u_z, ligero_pcs.eq_weights(F, self.z[:self.log_cols])):
            value = F.add(value, F.mul(a, b))
        if value != self.claim:
            raise FinalMismatch(self.claim, value)
        self.u_gamma, self.u_z = u_gamma, u_z
        if self.code == "expander":
            self.enc_gamma, self.enc_z = expander_code.encode(F, u_gamma), expander_code.encode(F, u_z)

    def draw_columns(self, rng):
        """`queries` column indices in [0, L), with replacement, for all the trees; only after the prover is bound to u_gamma and u_z"""
        if self.u_gamma is None:
            raise Error("draw_columns before receive: the columns must be drawn after the prover has sent u_gamma and u_z")
        L = 1 << self.log_len
        self.columns = [rng.randrange(L) if hasattr(rng, "randrange") else self.field.to_int(rng.draw()) % L for _ in range(self.queries)]
        return list(self.columns)

    def verify(self, openings):
        """openings[table] = [(index, values, path)] of the drawn columns (ligero_pcs.Prover.open_columns).  True, or the error of
        the first check that fails: per column the T paths, then the combination under gamma, then the one under e_t eq(z[c:])"""
        F = self.field
        if self.columns is None:
            raise Error("verify before draw_columns")
        for t in self.tables:
            if t not in openings or len(openings[t]) != len(self.columns):
                raise MerkleMismatch(t, "%d openings for %d drawn columns" % (len(openings.get(t, ())), len(self.columns)))
        eq_rows = ligero_pcs.eq_weights(F, self.z[self.log_cols:])
        z_weights = [[F.mul(e, w) for w in eq_rows] for e in self.e]
        for q, want in enumerate(self.columns):
            for t in self.tables:
                index, values, path = openings[t][q]
                if index != want or path.index != want:
                    raise MerkleMismatch(t, "the opening is of column %d, the drawn column is %d" % (index, want))
                if len(values) != 1 << self.log_rows or len(path.siblings) != self.log_len:
                    raise MerkleMismatch(t, "an opening of the wrong shape")
                if not ligero_pcs.ColumnPath(path.index, path.siblings, F).verify_column(self.roots[t], values):
                    raise MerkleMismatch(t, "the opening of column %d does not lead to the committed root" % index)
            for u, enc, weights, proximity in ((self.u_gamma, self.enc_gamma, self.gamma, True), (self.u_z, self.enc_z, z_weights, False)):
                combined = 0
                for t, wt in zip(self.tables, weights):
                    for w, v in zip(wt, openings[t][q][1]):
                        combined = F.add(combined, F.mul(w, int(v)))
                encoded = enc[want] if enc is not None else self._one._encode_at(u, want)
                if encoded != combined:
                    if proximity:
                        raise ProximityMismatch(want, encoded, combined)
                    raise EvalMismatch(combined, encoded)
        return True


# ---- the whole exchange ----------------------------------------------------------------------------------------------

def _shape_of(v):
    return (v.num_vars, v.log_cols, v.log_blowup, v.code)


def prove_claims(ctx, provers, verifiers, claims, rng, groups=None):
    """The whole exchange for any list of claims: provers = {name: ligero_pcs.Prover}, verifiers = {name: ligero_pcs.Verifier}
    (the roots, the shape, `queries` and the code are read from them; shape and code group the claims, and the verifiers of a
    group with several claims must agree in `queries`, else ValueError).  A group with several claims runs
    the protocol above - one joint opening; a group with one claim runs the single opening (r1cs.open_committed) and compares the
    opened value with the claimed one.  True, or the error of the first check that fails.  A ligero_pcs.FoldVerifier is refused:
    a joint folded opening is out of scope.  groups: a list that receives (tables, number of claims) of every group, in order"""
    from . import r1cs
    claims = [Claim(c[0], [int(x) for x in c[1]], int(c[2])) for c in claims]
    for name in dict.fromkeys(c.table for c in claims):
        if name not in provers or name not in verifiers:
            raise ValueError("no commitment named %r" % (name,))
        if isinstance(verifiers[name], ligero_pcs.FoldVerifier):
            raise ValueError("%r has a FoldVerifier: a joint folded opening (one Basefold run over the codewords of a group) is out of scope; "
                             "batched openings take the plain ligero_pcs.Verifier" % (name,))
    shapes = {name: _shape_of(v) for name, v in verifiers.items() if not isinstance(v, ligero_pcs.FoldVerifier)}
    for shape, tables, group in group_claims(claims, shapes):
        if groups is not None:
            groups.append((tuple(tables), len(group)))
        if len(group) == 1:
            c = group[0]
            value = r1cs.open_committed(provers[c.table], verifiers[c.table], c.point, rng)
            if value != c.value:
                raise ClaimMismatch(c.table, c.value, value)
            continue
        num_vars, log_cols, log_blowup, code = shape
        asked = sorted({verifiers[t].queries for t in tables})
        if len(asked) != 1:
            raise ValueError("the verifiers of the group %s ask for different numbers of queries: %s" % (", ".join(map(str, tables)), asked))
        queries = asked[0]
        V = Verifier(ctx.field, (num_vars, log_cols, log_blowup), {t: verifiers[t].root for t in tables}, queries, code)
        P = Prover(ctx, {t: provers[t] for t in tables})
        try:
            P.begin(group, V.draw_rho(group, rng), tables)
            P.sumcheck(lambda j, e: V.round(j, e, rng))
            V.receive(*P.combine(V.draw_gamma(rng)))
            V.verify(P.open_columns(V.draw_columns(rng)))
        finally:
            P.close()
    return True
