"""LogUp lookups: every entry of a committed table w lies in a public table t - the logarithmic-derivative lookup of Haboeck
("Multivariate lookups based on logarithmic derivatives") proved with the fractional sumcheck of Papini and Haboeck ("Improving
logarithmic derivative lookups using GKR"): sum_i 1 / (alpha - w_i) = sum_j mult_j / (alpha - t_j), each side reduced by a binary
tree of fraction additions and one cubic sumcheck per layer to evaluation claims about the input tables, which openings of the
Ligero commitments discharge.

csrc/kernels/fraction.hpp states the protocol; DESIGN.md section 9 item 17 describes the kernels.  In short:

  trees    layer n = (p, q); p_k[x] = p_(k+1)[x] q_(k+1)[x + 2^k] + p_(k+1)[x + 2^k] q_(k+1)[x], q_k[x] = q_(k+1)[x] q_(k+1)[x + 2^k];
           the root (P, Q) = (p_0[0], q_0[0]); PL, PR, QL, QR of layer k = the halves of p_(k+1) and q_(k+1)
  layer k  turns p_k~(z_k) = a_k, q_k~(z_k) = b_k into claims about layer k+1: lambda_k (k >= 1), k rounds of a cubic sumcheck over
           sum_x eq(z_k, x) (PL QR + PR QL + lambda_k QL QR)(x) = a_k + lambda_k b_k, four values H(0..3) per round, variable 0 first;
           then the finals pl, pr, ql, qr, checked as eq(z_k, r) (pl qr + pr ql + lambda_k ql qr) against the running claim (at
           k = 0: pl qr + pr ql = P and ql qr = Q); then rho_k, a_(k+1) = pl + rho_k (pr - pl), b_(k+1) = ql + rho_k (qr - ql),
           z_(k+1) = (r, rho_k)
  end      p~(z_n) = a_n and q~(z_n) = b_n, left to the caller; with an all-ones numerator (p=None) a_n must be 1

Field elements are Montgomery words, as everywhere in this package.  Nothing beyond the papers' statements is claimed: no
security level, no zero knowledge, no Fiat-Shamir.

  FractionTree, prove, Proof             sc_frac_*: the trees and the n layers on the device (small layers and tails on the host)
  Verifier                               pure host code, O(n^2) field operations
  multiplicities, range_indices          sc_lookup_count: mult_j = #{i : idx_i = j}; the indices of a range check
  LookupProver, LookupVerifier, prove_lookup"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import DRAW_FRAC_FN, u64, voidp
from .dense_mle import DenseMultilinearExtension, _u64p
from .grand_product import Verifier as _GpVerifier, _Replay, table_affine
from .relaxed_pcs import Error, _draw

MAX_LOG = 28
TAIL_LOG = 11          # kFrTailLog of csrc/kernels/fraction.hpp: the one-block tail of the trees takes layers of 2^this entries
TREE_LV_MAX = 3        # option "fr_tree_lv" at most
HOST_LOG_MAX = 12      # option "fr_host_log" at most
LOOKUP_LDS_LOG = 13    # kLookupLdsLog: tables of up to 2^this entries are counted in LDS histograms


class RootMismatch(Error):
    """the finals of layer 0 do not add up to the claimed root"""

    def __init__(self, root, value):
        super().__init__("Layer 0: (pl qr + pr ql, ql qr) is %r, the claimed root is %r" % (value, root))
        self.root, self.value = root, value


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim"""

    def __init__(self, layer, round_index, claim, total):
        super().__init__("Layer %d, round %d: H(0) + H(1) is %d, the claim is %d" % (layer, round_index, total, claim))
        self.layer, self.round, self.claim, self.total = layer, round_index, claim, total


class FinalMismatch(Error):
    """eq(z_k, r) (pl qr + pr ql + lambda ql qr) is not the last claim of the layer's sumcheck"""

    def __init__(self, layer, claim, value):
        super().__init__("Layer %d: the last claim is %d, eq(z, r) (pl qr + pr ql + lambda ql qr) is %d" % (layer, claim, value))
        self.layer, self.claim, self.value = layer, claim, value


class NumeratorMismatch(Error):
    """the numerator is all ones, but the last claim about it is not 1"""

    def __init__(self, claim):
        super().__init__("The last claim about the all-ones numerator is %d" % claim)
        self.claim = claim


class InputMismatch(Error):
    """an input table's extension at z_n is not the claim the last layer left"""

    def __init__(self, which, claim, value):
        super().__init__("The last claim about %s is %d, its extension at the point is %d" % (which, claim, value))
        self.which, self.claim, self.value = which, claim, value


class LookupMismatch(Error):
    """the two fraction sums differ, or one of their denominators is 0"""

    def __init__(self, root_w, root_t):
        super().__init__("The fraction sums are %r and %r" % (root_w, root_t))
        self.root_w, self.root_t = root_w, root_t


Proof = collections.namedtuple("Proof", "root rounds finals point claims challenges")
Proof.__doc__ = """root = (P, Q); rounds[k][j] = the four values of round j of layer k; finals[k] = (pl, pr, ql, qr); point = z_n;
claims = (a_n, b_n); challenges = every drawn word as it was drawn: rho_0, then per layer k >= 1 lambda_k, its rounds' challenges, rho_k"""


def n_challenges(n):
    return n * (n - 1) // 2 + 2 * n - 1


# ---- the device side -------------------------------------------------------------------------------------------------

class FractionTree:
    """sc_frac_create: the fraction-sum trees of (p, q) (2^n entries each, 1 <= n <= 28; p=None: all ones), which are kept alive
    and never written"""

    def __init__(self, ctx, q, p=None):
        self.ctx, self.q, self.p = ctx, q, p
        self.h = voidp()
        ctx.check(ctx.lib.sc_frac_create(ctx.h, p.h if p is not None else None, q.h, ctypes.byref(self.h)))
        self.num_vars, self.ones = q.num_vars(), p is None
        out = (u64 * 2)()
        ctx.check(ctx.lib.sc_frac_root(self.h, out))
        self.root = (int(out[0]), int(out[1]))

    def layer(self, k, which):
        """a copy of layer k, 0 <= k < n, of p (which = 0 or "p") or q (1 or "q") as a device table of 2^k words"""
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_frac_layer(self.ctx.h, self.h, int(k), {"p": 0, "q": 1}.get(which, which), ctypes.byref(h)))
        return DenseMultilinearExtension(self.ctx, h)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_frac_destroy(self.ctx.h, self.h)
        self.h = None
        self.q = self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _guarded(ctx, draw):
    """a C callback over draw(layer, round, msg): an exception must not cross the C frames - the call ends (an unreduced word)
    and the exception is raised again by the caller"""
    failure = []

    def cb(_user, layer, j, msg):
        try:
            width = 4 if j <= layer else 0
            return int(draw(int(layer), int(j), [int(msg[k]) for k in range(width)]))
        except BaseException as exc:
            failure.append(exc)
            return ctx.field.p
    return cb, failure


def prove(tree, draw=None, seed_r=0):
    """sc_frac_prove.  draw(layer, round, msg) returns a challenge: round < layer, msg = [H(0), H(1), H(2), H(3)] -> r_round;
    round == layer, msg = [pl, pr, ql, qr] -> rho_layer; round == layer + 1, msg = [] -> lambda of layer + 1.  None: the synthetic
    challenger of sc_prove over seed_r.  Returns a Proof"""
    ctx, n = tree.ctx, tree.num_vars
    n_rounds = n * (n - 1) // 2
    evals, fin = np.zeros(4 * max(n_rounds, 1), dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64)
    ch, point, claims = np.zeros(n_challenges(n), dtype=np.uint64), np.zeros(n, dtype=np.uint64), (u64 * 2)()
    cb, failure = _guarded(ctx, draw) if draw is not None else (None, [])
    rc = ctx.lib.sc_frac_prove(ctx.h, tree.h, DRAW_FRAC_FN(cb) if cb else ctypes.cast(None, DRAW_FRAC_FN), None, int(seed_r), _u64p(evals),
                               _u64p(fin), _u64p(ch), _u64p(point), claims)
    if failure:
        raise failure[0]
    ctx.check(rc)
    rounds, at = [], 0
    for k in range(n):
        rounds.append([[int(x) for x in evals[4 * (at + j):4 * (at + j) + 4]] for j in range(k)])
        at += k
    return Proof(tree.root, rounds, [tuple(int(x) for x in fin[4 * k:4 * k + 4]) for k in range(n)], [int(x) for x in point],
                 (int(claims[0]), int(claims[1])), [int(x) for x in ch])


# ---- the verifier ----------------------------------------------------------------------------------------------------

class Verifier:
    """The verifier of the fraction sum of tables of n variables: pure host code.  begin(P, Q), then per layer k: lam(k, rng) for
    k >= 1, its rounds round(k, j, values, rng) and finals(k, pl, pr, ql, qr, rng), each returning the drawn challenge;
    result() = (z_n, a_n, b_n).  ones: the numerator is all ones, and result() refuses a_n != 1.  verify() runs a whole Proof;
    challenger() is the draw of an interactive prove()."""

    _cubic_at = _GpVerifier._cubic_at

    def __init__(self, field, n, ones=False):
        if not 1 <= n <= MAX_LOG:
            raise ValueError("n must be in 1..%d" % MAX_LOG)
        if field.p <= 3:
            raise ValueError("p = %d: the cubic through 0, 1, 2, 3 needs 2 and 3 invertible" % field.p)
        self.field, self.n, self.ones = field, n, bool(ones)
        self.inv2, self.inv6 = field.inv(field.from_int(2)), field.inv(field.from_int(6))
        self.root = None

    def begin(self, P, Q):
        self.root = (int(P), int(Q))
        self.layer, self.z, self.a, self.b, self.r, self.lam_k, self.claim = 0, [], int(P), int(Q), [], None, None

    def lam(self, layer, rng):
        if self.root is None or layer != self.layer or layer < 1 or layer >= self.n or self.lam_k is not None:
            raise Error("lambda of layer %d out of order" % layer)
        self.lam_k = _draw(self.field, rng)
        self.claim = self.field.add(self.a, self.field.mul(self.lam_k, self.b))
        return self.lam_k

    def round(self, layer, j, values, rng):
        F = self.field
        if self.root is None or layer != self.layer or self.lam_k is None or j != len(self.r) or j >= layer or len(values) != 4:
            raise Error("layer %d, round %d out of order" % (layer, j))
        total = F.add(int(values[0]), int(values[1]))
        if total != self.claim:
            raise RoundMismatch(layer, j, self.claim, total)
        r = _draw(F, rng)
        self.claim = self._cubic_at(values, r)
        self.r.append(r)
        return r

    def finals(self, layer, pl, pr, ql, qr, rng):
        F = self.field
        pl, pr, ql, qr = int(pl), int(pr), int(ql), int(qr)
        if self.root is None or layer != self.layer or len(self.r) != layer or layer >= self.n or (layer > 0 and self.lam_k is None):
            raise Error("finals of layer %d out of order" % layer)
        num, den = F.add(F.mul(pl, qr), F.mul(pr, ql)), F.mul(ql, qr)
        if layer == 0:
            if (num, den) != self.root:
                raise RootMismatch(self.root, (num, den))
        else:
            eq = F.one
            for zi, ri in zip(self.z, self.r):
                zr = F.mul(zi, ri)
                eq = F.mul(eq, F.add(F.sub(F.sub(F.one, zi), ri), F.add(zr, zr)))
            value = F.mul(eq, F.add(num, F.mul(self.lam_k, den)))
            if value != self.claim:
                raise FinalMismatch(layer, self.claim, value)
        rho = _draw(F, rng)
        self.a, self.b = F.add(pl, F.mul(rho, F.sub(pr, pl))), F.add(ql, F.mul(rho, F.sub(qr, ql)))
        self.z, self.r, self.layer, self.lam_k, self.claim = self.r + [rho], [], layer + 1, None, None
        return rho

    def result(self):
        if self.root is None or self.layer != self.n:
            raise Error("result before the last layer")
        if self.ones and self.a != self.field.one:
            raise NumeratorMismatch(self.a)
        return list(self.z), self.a, self.b

    def challenger(self, rng, root=None):
        """draw(layer, round, msg) for prove(): the verifier's checks and draws, message by message.  root: begin(*root) first"""
        if root is not None:
            self.begin(*root)

        def draw(layer, j, msg):
            if j < layer:
                return self.round(layer, j, msg, rng)
            if j == layer:
                return self.finals(layer, msg[0], msg[1], msg[2], msg[3], rng)
            return self.lam(layer + 1, rng)
        return draw

    def verify(self, proof, rng_or_challenges):
        """the whole proof; rng_or_challenges: where the challenges come from - an rng, or the recorded words in the order they
        were drawn.  Returns (z_n, a_n, b_n), or raises the error of the first message that does not fit"""
        rng = rng_or_challenges if hasattr(rng_or_challenges, "draw") or hasattr(rng_or_challenges, "random") else _Replay(rng_or_challenges)
        if len(proof.rounds) != self.n or len(proof.finals) != self.n:
            raise Error("a proof of %d layers for tables of %d variables" % (len(proof.rounds), self.n))
        self.begin(*proof.root)
        for k in range(self.n):
            if len(proof.rounds[k]) != k:
                raise Error("layer %d has %d rounds" % (k, len(proof.rounds[k])))
            if k >= 1:
                self.lam(k, rng)
            for j in range(k):
                self.round(k, j, proof.rounds[k][j], rng)
            self.finals(k, *proof.finals[k], rng)
        return self.result()

    def check_input(self, q_value, p_value=None):
        """the caller's last step: q~(z_n) = q_value against b_n and, unless the numerator is all ones, p~(z_n) = p_value against a_n"""
        _, a, b = self.result()
        if not self.ones:
            if p_value is None:
                raise Error("the numerator's value at the point is missing")
            if int(p_value) != a:
                raise InputMismatch("p", a, int(p_value))
        if int(q_value) != b:
            raise InputMismatch("q", b, int(q_value))
        return True


# ---- the lookup ------------------------------------------------------------------------------------------------------

def multiplicities(ctx, w, t, idx):
    """sc_lookup_count: (mult, mismatches) - mult a device table of t's length with mult_j = #{i : idx_i = j, w_i = t_j} as field
    words, mismatches the number of i with idx_i outside t or w_i != t[idx_i] (they are not counted)"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    if idx.shape != (1 << w.num_vars(),):
        raise ValueError("one index per entry of w")
    h, bad = voidp(), u64()
    ctx.check(ctx.lib.sc_lookup_count(ctx.h, w.h, t.h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(h), ctypes.byref(bad)))
    return DenseMultilinearExtension(ctx, h), int(bad.value)


def range_indices(field, w):
    """the indices of a lookup into the range table t_j = j: idx_i = the integer w_i stands for (2^32 - 1 where it is larger, which
    no table holds).  w: Montgomery words"""
    return np.array([min(field.to_int(x), 0xFFFFFFFF) for x in w], dtype=np.uint32)


def range_table_eval(field, point):
    """t~(point) for t_j = j, j < 2^m: sum_j 2^j point_j (the identity is linear in every bit)"""
    out, weight = 0, field.one
    for x in point:
        out, weight = field.add(out, field.mul(weight, int(x))), field.add(weight, weight)
    return out


def min_modulus_log(n, m):
    """counts are field words: p must exceed 2^max(n, m)"""
    return max(n, m)


class LookupProver:
    """w: a ligero_pcs.Prover commitment to the witness; t: the public device table; idx (u32, one per entry of w) with
    w_i = t[idx_i].  commit_mult(commit) first, then roots(alpha), prove(which, draw)"""

    def __init__(self, pcs_w, t, idx):
        if pcs_w.ctx is not t.ctx:
            raise ValueError("the commitment and the table are of one context")
        self.ctx, self.pcs_w, self.t, self.idx = pcs_w.ctx, pcs_w, t, idx
        self.pcs_mult, self.mult, self.mismatches, self.trees, self.tables = None, None, None, [], []

    def commit_mult(self, commit):
        """step 1, before alpha exists: mult, and commit(mult) -> the prover of its commitment"""
        self.mult, self.mismatches = multiplicities(self.ctx, self.pcs_w.poly, self.t, self.idx)
        self.pcs_mult = commit(self.mult)
        return self.pcs_mult

    def roots(self, alpha):
        """step 3: the trees of (1, alpha - w) and (mult, alpha - t); returns the two roots"""
        F = self.ctx.field
        self._drop_trees()
        self.tables = [table_affine(self.ctx, self.pcs_w.poly, F.neg(F.one), alpha), table_affine(self.ctx, self.t, F.neg(F.one), alpha)]
        self.trees = [FractionTree(self.ctx, self.tables[0]), FractionTree(self.ctx, self.tables[1], self.mult)]
        return tuple(t.root for t in self.trees)

    def prove(self, which, draw):
        return prove(self.trees[which], draw)

    def _drop_trees(self):
        for t in self.trees:
            t.close()
        self.trees, self.tables = [], []

    def close(self):
        self._drop_trees()
        if self.pcs_mult is not None:
            self.pcs_mult.close()
        self.pcs_mult = self.mult = None


class LookupVerifier:
    """over the verifiers of the openings of w's and mult's commitments (ligero_pcs.Verifier or FoldVerifier, built over the
    roots) and table_eval(point) = t~(point), which the verifier computes from the public table (range_table_eval for t_j = j)"""

    def __init__(self, field, pcs_verifier_w, pcs_verifier_mult, table_eval):
        self.field, self.n, self.m = field, pcs_verifier_w.num_vars, pcs_verifier_mult.num_vars
        if field.p <= 1 << min_modulus_log(self.n, self.m):
            raise ValueError("p = %d: a count of up to 2^%d must be a field word" % (field.p, max(self.n, self.m)))
        self.pcs, self.table_eval = (pcs_verifier_w, pcs_verifier_mult), table_eval
        self.frac = (Verifier(field, self.n, ones=True), Verifier(field, self.m))
        self.alpha = None

    def draw_alpha(self, rng):
        self.alpha = _draw(self.field, rng)
        return self.alpha

    def receive_roots(self, root_w, root_t):
        """step 4: Q_w != 0, Q_t != 0 and P_w Q_t = P_t Q_w"""
        F = self.field
        if self.alpha is None:
            raise Error("the roots before alpha")
        (pw, qw), (pt, qt) = (tuple(int(x) for x in root_w), tuple(int(x) for x in root_t))
        if qw == 0 or qt == 0 or F.mul(pw, qt) != F.mul(pt, qw):
            raise LookupMismatch((pw, qw), (pt, qt))
        self.frac[0].begin(pw, qw)
        self.frac[1].begin(pt, qt)

    def opening(self, which):
        """(point, value the commitment must open to): w~(z) = alpha - b_n (which = 0), mult~(z') = a'_m (which = 1)"""
        point, a, b = self.frac[which].result()
        return point, (self.field.sub(self.alpha, b) if which == 0 else a)

    def finish(self, which, opened):
        """steps 5 - 7 of one side, from the value the opening's verifier accepted"""
        F = self.field
        point, expected = self.opening(which)
        if int(opened) != expected:
            raise InputMismatch("w" if which == 0 else "mult", expected, int(opened))
        if which == 1:
            _, _, b = self.frac[1].result()
            value = F.sub(self.alpha, int(self.table_eval(point)))
            if value != b:
                raise InputMismatch("alpha - t", b, value)
        return True


def _default_commit(prover_w, verifier_w):
    """mult committed as w is: the same code and blowup, half of the variables in the columns, the same number of queries"""
    from . import ligero_pcs as lp
    made = []

    def commit(mult):
        m = mult.num_vars()
        made.append(lp.Prover.commit(prover_w.ctx, mult, log_cols=m // 2, log_blowup=prover_w.log_blowup, code=prover_w.code))
        return made[0]

    def verifier(field):
        p = made[0]
        if isinstance(verifier_w, lp.FoldVerifier):
            return lp.FoldVerifier(field, p.num_vars, p.log_cols, p.log_blowup, p.root(), verifier_w.queries)
        return lp.Verifier(field, p.num_vars, p.log_cols, p.log_blowup, p.root(), verifier_w.queries, code=p.code)
    return commit, verifier


def prove_lookup(prover_w, verifier_w, t, idx, rng, table_eval=None, commit=None, verifier_of=None):
    """the whole exchange: prover_w is the ligero_pcs.Prover commitment to w, verifier_w the verifier of its openings, t the public
    device table, idx the u32 indices with w_i = t[idx_i].  table_eval(point) = t~(point) as the verifier computes it (default:
    the table's own evaluate; range_table_eval for a range table).  commit(mult) -> the Prover of mult's commitment and
    verifier_of(field) -> the verifier of its openings (default: committed as w is).  Openings go through r1cs.open_committed:
    plain, folded or expander code.  True, or the verifier's error (LookupMismatch when some w_i is outside t at the drawn alpha)"""
    from . import r1cs
    F = prover_w.ctx.field
    if commit is None:
        commit, verifier_of = _default_commit(prover_w, verifier_w)
    if table_eval is None:
        table_eval = lambda point: t.evaluate(point)   # noqa: E731
    if F.p <= 1 << max(prover_w.num_vars, t.num_vars()):
        raise ValueError("p = %d: a count of up to 2^%d must be a field word" % (F.p, max(prover_w.num_vars, t.num_vars())))
    P = LookupProver(prover_w, t, idx)
    try:
        P.commit_mult(commit)                                                 # 1: before alpha
        V = LookupVerifier(F, verifier_w, verifier_of(F), table_eval)
        V.receive_roots(*P.roots(V.draw_alpha(rng)))                          # 2, 3, 4
        for which in range(2):
            P.prove(which, V.frac[which].challenger(rng))
            point, _ = V.opening(which)
            pcs = (P.pcs_w, P.pcs_mult)[which]
            V.finish(which, r1cs.open_committed(pcs, V.pcs[which], point, rng))   # 5, 6, 7
    finally:
        P.close()
    return True
