"""LogUp's fraction sums with every element in the quadratic extension K = F_p[X] / (X^2 - w), and their first consumer, a lookup
between two Ligero commitments with alpha, lambda, rho and every round challenge in K.

csrc/kernels/ext_fraction.hpp states the protocol - that of logup.py word for word, over K; DESIGN.md section 9 item 22 describes the
kernels.  In short:

  leaves   never stored: q_i = beta + alpha t[i], t a base-field device table of 2^n entries, alpha, beta in K, alpha != 0; the
           numerator p_i a base-field table embedded as (p_i, 0), or all ones (p=None)
  trees    p_k[x] = p_(k+1)[x] q_(k+1)[x + 2^k] + p_(k+1)[x + 2^k] q_(k+1)[x], q_k[x] = q_(k+1)[x] q_(k+1)[x + 2^k] in K; the root
           (P, Q) in K^2
  layer k  lambda_k in K (k >= 1), k rounds of a cubic sumcheck over sum_x eq(z_k, x) (PL QR + PR QL + lambda_k QL QR)(x)
           = a_k + lambda_k b_k, four values of K per round, challenges in K; the finals pl, pr, ql, qr in K, checked as
           eq(z_k, r) (pl qr + pr ql + lambda_k ql qr) (at k = 0: pl qr + pr ql = P and ql qr = Q); then rho_k in K,
           a_(k+1) = pl + rho_k (pr - pl), b_(k+1) = ql + rho_k (qr - ql), z_(k+1) = (r, rho_k)
  end      p~(z_n) = a_n (all ones: a_n = 1) and t~(z_n) = (b_n - beta) / alpha: ext_sumcheck.table_evaluate_ext, or an opening of a
           commitment at the point of K^n

An element of K is a (c0, c1) pair of Montgomery words, as ext_field.QuadExt handles them.  Nothing beyond the papers' statements
is claimed: no security level, no Fiat-Shamir, no zero knowledge, and gamma of the Ligero proximity test stays in the base field.

  ExtFractionTree, prove_ext, Proof         sc_frac_*_ext: the trees and the n layers on the device (small layers and tails on the host)
  Verifier                                  pure host code, O(n^2) operations in K
  range_table_eval                          t~(point) in K for the range table t_j = j
  LookupProver, LookupVerifier, prove_lookup_ext"""
import collections
import ctypes

import numpy as np

from ._lib import DRAW_FRAC_EXT_FN, u64, voidp
from .dense_mle import DenseMultilinearExtension, _u64p
from .ext_field import QuadExt
from .ext_grand_product import Verifier as _GpExtVerifier, _Replay, _draw_ext, _pair, _pairs
from .logup import multiplicities, n_challenges
from .relaxed_pcs import Error

MAX_LOG = 28
TAIL_LOG = 10          # kExtFrTailLog of csrc/kernels/ext_fraction.hpp: the one-block tail of the trees takes layers of 2^this entries


class RootMismatch(Error):
    """the finals of layer 0 do not add up to the claimed root"""

    def __init__(self, root, value):
        super().__init__("Layer 0: (pl qr + pr ql, ql qr) is %r, the claimed root is %r" % (value, root))
        self.root, self.value = root, value


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim"""

    def __init__(self, layer, round_index, claim, total):
        super().__init__("Layer %d, round %d: H(0) + H(1) is %s, the claim is %s" % (layer, round_index, total, claim))
        self.layer, self.round, self.claim, self.total = layer, round_index, claim, total


class FinalMismatch(Error):
    """eq(z_k, r) (pl qr + pr ql + lambda ql qr) is not the last claim of the layer's sumcheck"""

    def __init__(self, layer, claim, value):
        super().__init__("Layer %d: the last claim is %s, eq(z, r) (pl qr + pr ql + lambda ql qr) is %s" % (layer, claim, value))
        self.layer, self.claim, self.value = layer, claim, value


class NumeratorMismatch(Error):
    """the numerator is all ones, but the last claim about it is not 1"""

    def __init__(self, claim):
        super().__init__("The last claim about the all-ones numerator is %s" % (claim,))
        self.claim = claim


class InputMismatch(Error):
    """an input table's extension at z_n is not the claim the last layer left"""

    def __init__(self, which, claim, value):
        super().__init__("The last claim about %s is %s, its extension at the point gives %s" % (which, claim, value))
        self.which, self.claim, self.value = which, claim, value


class LookupMismatch(Error):
    """the two fraction sums differ, or one of their denominators is 0"""

    def __init__(self, root_w, root_t):
        super().__init__("The fraction sums are %r and %r" % (root_w, root_t))
        self.root_w, self.root_t = root_w, root_t


Proof = collections.namedtuple("Proof", "root rounds finals point claims challenges")
Proof.__doc__ = """every element a (c0, c1) pair: root = (P, Q); rounds[k][j] = the four values of round j of layer k; finals[k] =
(pl, pr, ql, qr); point = z_n; claims = (a_n, b_n); challenges = every drawn element as it was drawn: rho_0, then per layer k >= 1
lambda_k, its rounds' challenges, rho_k"""


# ---- the device side -------------------------------------------------------------------------------------------------

class ExtFractionTree:
    """sc_frac_create_ext: the fraction-sum trees over K = QuadExt(field, w) of the leaves (p[i], beta + alpha t[i]).  `t` and `p`
    (2^n base words each, 1 <= n <= 28; p=None: all ones) are kept alive and never written; w is a Montgomery word, alpha and beta
    are (c0, c1) pairs"""

    def __init__(self, ctx, w, p, t, alpha, beta):
        self.ctx, self.p, self.t, self.w = ctx, p, t, int(w)
        self.alpha, self.beta = _pair(alpha), _pair(beta)
        self.h = voidp()
        a, b = (u64 * 2)(*self.alpha), (u64 * 2)(*self.beta)
        ctx.check(ctx.lib.sc_frac_create_ext(ctx.h, self.w, p.h if p is not None else None, t.h, a, b, ctypes.byref(self.h)))
        self.num_vars, self.ones = t.num_vars(), p is None
        out = (u64 * 4)()
        ctx.check(ctx.lib.sc_frac_root_ext(self.h, out))
        self.root = ((int(out[0]), int(out[1])), (int(out[2]), int(out[3])))

    def layer(self, k, which):
        """copies of the two planes of layer k, 0 <= k < n, of p (which = 0 or "p") or q (1 or "q"): (the c0 words, the c1 words),
        device tables of 2^k words each"""
        h0, h1 = voidp(), voidp()
        self.ctx.check(self.ctx.lib.sc_frac_layer_ext(self.ctx.h, self.h, int(k), {"p": 0, "q": 1}.get(which, which), ctypes.byref(h0), ctypes.byref(h1)))
        return DenseMultilinearExtension(self.ctx, h0), DenseMultilinearExtension(self.ctx, h1)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_frac_destroy_ext(self.ctx.h, self.h)
        self.h = None
        self.p = self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prove_ext(tree, draw=None, seed_r=0):
    """sc_frac_prove_ext.  draw(layer, round, msg) returns a challenge, a (c0, c1) pair: round < layer, msg = [H(0), H(1), H(2), H(3)]
    (pairs) -> r_round; round == layer, msg = [pl, pr, ql, qr] -> rho_layer; round == layer + 1, msg = [] -> lambda of layer + 1.
    None: the synthetic challenger over seed_r.  Returns a Proof"""
    ctx, n = tree.ctx, tree.num_vars
    n_rounds = n * (n - 1) // 2
    evals, fin = np.zeros(8 * max(n_rounds, 1), dtype=np.uint64), np.zeros(8 * n, dtype=np.uint64)
    ch, point, claims = np.zeros(2 * n_challenges(n), dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64), (u64 * 4)()
    failure = []

    def cb(_user, layer, j, msg, out):
        try:
            width = 8 if j <= layer else 0
            r = draw(int(layer), int(j), _pairs([int(msg[k]) for k in range(width)]))
            out[0], out[1] = int(r[0]), int(r[1])
        except BaseException as exc:      # an exception must not cross the C frames: the call ends, and it is raised again below
            failure.append(exc)
            out[0] = out[1] = ctx.field.p
    rc = ctx.lib.sc_frac_prove_ext(ctx.h, tree.h, DRAW_FRAC_EXT_FN(cb) if draw is not None else ctypes.cast(None, DRAW_FRAC_EXT_FN), None, int(seed_r),
                                   _u64p(evals), _u64p(fin), _u64p(ch), _u64p(point), claims)
    if failure:
        raise failure[0]
    ctx.check(rc)
    rounds, at = [], 0
    for k in range(n):
        rounds.append([_pairs(evals[8 * (at + j):8 * (at + j) + 8]) for j in range(k)])
        at += k
    return Proof(tree.root, rounds, [tuple(_pairs(fin[8 * k:8 * k + 8])) for k in range(n)], _pairs(point),
                 ((int(claims[0]), int(claims[1])), (int(claims[2]), int(claims[3]))), _pairs(ch))


# ---- the verifier ----------------------------------------------------------------------------------------------------

class Verifier:
    """The verifier of the fraction sum over K = QuadExt(field, w) of tables of n variables: pure host code.  begin(P, Q), then per
    layer k: lam(k, rng) for k >= 1, its rounds round(k, j, values, rng) and finals(k, pl, pr, ql, qr, rng), each returning the drawn
    challenge; result() = (z_n, a_n, b_n).  ones: the numerator is all ones, and result() refuses a_n != 1.  verify() runs a whole
    Proof; challenger() is the draw of an interactive prove_ext()."""

    _cubic_at = _GpExtVerifier._cubic_at    # the cubic through 0 .. 3 in K

    def __init__(self, field, w, n, ones=False):
        if not 1 <= n <= MAX_LOG:
            raise ValueError("n must be in 1..%d" % MAX_LOG)
        if field.p <= 3:
            raise ValueError("p = %d: the cubic through 0, 1, 2, 3 needs 2 and 3 invertible" % field.p)
        self.field, self.ext, self.n, self.ones = field, QuadExt(field, w), n, bool(ones)
        self.inv2, self.inv6 = field.inv(field.from_int(2)), field.inv(field.from_int(6))
        self.root = None

    def begin(self, P, Q):
        self.root = (_pair(P), _pair(Q))
        self.layer, self.z, self.a, self.b, self.r, self.lam_k, self.claim = 0, [], _pair(P), _pair(Q), [], None, None

    def lam(self, layer, rng):
        K = self.ext
        if self.root is None or layer != self.layer or layer < 1 or layer >= self.n or self.lam_k is not None:
            raise Error("lambda of layer %d out of order" % layer)
        self.lam_k = _draw_ext(K, rng)
        self.claim = K.add(self.a, K.mul(self.lam_k, self.b))
        return self.lam_k

    def round(self, layer, j, values, rng):
        K = self.ext
        if self.root is None or layer != self.layer or self.lam_k is None or j != len(self.r) or j >= layer or len(values) != 4:
            raise Error("layer %d, round %d out of order" % (layer, j))
        values = [_pair(v) for v in values]
        total = K.add(values[0], values[1])
        if total != self.claim:
            raise RoundMismatch(layer, j, self.claim, total)
        r = _draw_ext(K, rng)
        self.claim = self._cubic_at(values, r)
        self.r.append(r)
        return r

    def finals(self, layer, pl, pr, ql, qr, rng):
        K = self.ext
        pl, pr, ql, qr = _pair(pl), _pair(pr), _pair(ql), _pair(qr)
        if self.root is None or layer != self.layer or len(self.r) != layer or layer >= self.n or (layer > 0 and self.lam_k is None):
            raise Error("finals of layer %d out of order" % layer)
        num, den = K.add(K.mul(pl, qr), K.mul(pr, ql)), K.mul(ql, qr)
        if layer == 0:
            if (num, den) != self.root:
                raise RootMismatch(self.root, (num, den))
        else:
            eq = K.one
            for zi, ri in zip(self.z, self.r):
                zr = K.mul(zi, ri)
                eq = K.mul(eq, K.add(K.sub(K.sub(K.one, zi), ri), K.add(zr, zr)))
            value = K.mul(eq, K.add(num, K.mul(self.lam_k, den)))
            if value != self.claim:
                raise FinalMismatch(layer, self.claim, value)
        rho = _draw_ext(K, rng)
        self.a, self.b = K.add(pl, K.mul(rho, K.sub(pr, pl))), K.add(ql, K.mul(rho, K.sub(qr, ql)))
        self.z, self.r, self.layer, self.lam_k, self.claim = self.r + [rho], [], layer + 1, None, None
        return rho

    def result(self):
        if self.root is None or self.layer != self.n:
            raise Error("result before the last layer")
        if self.ones and self.a != self.ext.one:
            raise NumeratorMismatch(self.a)
        return list(self.z), self.a, self.b

    def challenger(self, rng, root=None):
        """draw(layer, round, msg) for prove_ext(): the verifier's checks and draws, message by message.  root: begin(*root) first"""
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
        """the whole proof; rng_or_challenges: where the challenges come from - an rng, or the recorded pairs in the order they were
        drawn.  Returns (z_n, a_n, b_n), or raises the error of the first message that does not fit"""
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

    def check_input(self, numerator_value, table_value, alpha, beta):
        """the caller's last step: beta + alpha table_value, table_value = t~(z_n) in K, against b_n and, unless the numerator is all
        ones, numerator_value = p~(z_n) against a_n"""
        K = self.ext
        _, a, b = self.result()
        if not self.ones:
            if numerator_value is None:
                raise Error("the numerator's value at the point is missing")
            if _pair(numerator_value) != a:
                raise InputMismatch("p", a, _pair(numerator_value))
        got = K.add(_pair(beta), K.mul(_pair(alpha), _pair(table_value)))
        if got != b:
            raise InputMismatch("beta + alpha t", b, got)
        return True


# ---- the lookup: every w_i lies in t, alpha in K ---------------------------------------------------------------------------
#
# P commits to mult before alpha exists; V draws alpha_c in K; P builds the trees of (1, alpha_c - w) and (mult, alpha_c - t)
# (alpha = (-1, 0), beta = alpha_c: no table is formed) and proves both fraction sums; V checks Q_w != 0, Q_t != 0 and
# P_w Q_t = P_t Q_w in K, a_n = 1 on the witness side, and turns the final claims into w~(z) = alpha_c - b_n and mult~(z') = a'_m, which
# one opening of each commitment at its point of K^n discharges; t~(z') it computes itself.

def range_table_eval(ext, point):
    """t~(point) in K for t_j = j, j < 2^m: sum_j 2^j point_j (the identity is linear in every bit)"""
    F = ext.field
    out, weight = ext.zero, F.one
    for x in point:
        out, weight = ext.add(out, ext.scale(_pair(x), weight)), F.add(weight, weight)
    return out


class LookupProver:
    """w: a ligero_pcs.Prover commitment to the witness; t: the public device table; idx (u32, one per entry of w) with
    w_i = t[idx_i]; ext_w: w of K, a Montgomery word.  commit_mult(commit) first, then roots(alpha), prove(which, draw)"""

    def __init__(self, pcs_w, t, idx, ext_w):
        if pcs_w.ctx is not t.ctx:
            raise ValueError("the commitment and the table are of one context")
        self.ctx, self.pcs_w, self.t, self.idx, self.w = pcs_w.ctx, pcs_w, t, idx, int(ext_w)
        self.pcs_mult, self.mult, self.mismatches, self.trees = None, None, None, []

    def commit_mult(self, commit):
        """step 1, before alpha exists: mult (sc_lookup_count), and commit(mult) -> the prover of its commitment"""
        self.mult, self.mismatches = multiplicities(self.ctx, self.pcs_w.poly, self.t, self.idx)
        self.pcs_mult = commit(self.mult)
        return self.pcs_mult

    def roots(self, alpha):
        """step 3: the trees of (1, alpha - w) and (mult, alpha - t); returns the two roots"""
        F = self.ctx.field
        self._drop_trees()
        minus_one = (F.neg(F.one), 0)
        self.trees = [ExtFractionTree(self.ctx, self.w, None, self.pcs_w.poly, minus_one, alpha),
                      ExtFractionTree(self.ctx, self.w, self.mult, self.t, minus_one, alpha)]
        return tuple(t.root for t in self.trees)

    def prove(self, which, draw):
        return prove_ext(self.trees[which], draw)

    def _drop_trees(self):
        for t in self.trees:
            t.close()
        self.trees = []

    def close(self):
        self._drop_trees()
        if self.pcs_mult is not None:
            self.pcs_mult.close()
        self.pcs_mult = self.mult = None


class LookupVerifier:
    """over the two ligero_pcs.ExtVerifier of the openings of w's and mult's commitments (built over the roots and the same w) and
    table_eval(point) = t~(point) in K, which the verifier computes from the public table (range_table_eval for t_j = j)"""

    def __init__(self, field, w, pcs_verifier_w, pcs_verifier_mult, table_eval):
        for v in (pcs_verifier_w, pcs_verifier_mult):
            if not hasattr(v, "ext") or v.ext.w != int(w):
                raise ValueError("the verifiers are ligero_pcs.ExtVerifier over the same w")
        self.field, self.ext, self.n, self.m = field, QuadExt(field, w), pcs_verifier_w.num_vars, pcs_verifier_mult.num_vars
        if field.p <= 1 << max(self.n, self.m):
            raise ValueError("p = %d: a count of up to 2^%d must be a field word" % (field.p, max(self.n, self.m)))
        self.pcs, self.table_eval = (pcs_verifier_w, pcs_verifier_mult), table_eval
        self.frac = (Verifier(field, w, self.n, ones=True), Verifier(field, w, self.m))
        self.alpha = None

    def draw_alpha(self, rng):
        self.alpha = _draw_ext(self.ext, rng)
        return self.alpha

    def receive_roots(self, root_w, root_t):
        """step 4: Q_w != 0, Q_t != 0 and P_w Q_t = P_t Q_w, in K"""
        K = self.ext
        if self.alpha is None:
            raise Error("the roots before alpha")
        (pw, qw), (pt, qt) = ((_pair(root_w[0]), _pair(root_w[1])), (_pair(root_t[0]), _pair(root_t[1])))
        if qw == K.zero or qt == K.zero or K.mul(pw, qt) != K.mul(pt, qw):
            raise LookupMismatch((pw, qw), (pt, qt))
        self.frac[0].begin(pw, qw)
        self.frac[1].begin(pt, qt)

    def opening(self, which):
        """(point, value the commitment must open to): w~(z) = alpha - b_n (which = 0), mult~(z') = a'_m (which = 1)"""
        point, a, b = self.frac[which].result()
        return point, (self.ext.sub(self.alpha, b) if which == 0 else a)

    def finish(self, which, opened):
        """steps 5 - 7 of one side, from the value the opening's verifier accepted"""
        K = self.ext
        point, expected = self.opening(which)
        if _pair(opened) != expected:
            raise InputMismatch("w" if which == 0 else "mult", expected, _pair(opened))
        if which == 1:
            _, _, b = self.frac[1].result()
            value = K.sub(self.alpha, _pair(self.table_eval(point)))
            if value != b:
                raise InputMismatch("alpha - t", b, value)
        return True


def _default_mult(prover_w, verifier_w, w):
    """mult committed as w is: the same code and blowup, half of the variables in the columns, the same number of queries"""
    from . import ligero_pcs as lp

    def commit(mult):
        return lp.Prover.commit(prover_w.ctx, mult, log_cols=mult.num_vars() // 2, log_blowup=prover_w.log_blowup, code=prover_w.code)

    def verifier(p):
        return lp.ExtVerifier(prover_w.ctx.field, p.num_vars, p.log_cols, p.log_blowup, p.root(), verifier_w.queries, code=p.code, w=w)
    return commit, verifier


def prove_lookup_ext(prover_w, prover_mult, verifier_w, verifier_mult, table, idx, rng, w, table_eval=None):
    """the whole exchange over K = QuadExt(field, w), w a Montgomery word.  prover_w: the ligero_pcs.Prover commitment to the witness;
    verifier_w: the ligero_pcs.ExtVerifier of its openings over the same w; table: the public device table; idx: the u32 indices
    with w_i = table[idx_i].  The multiplicities do not exist before this call, so their commitment is made here, before alpha is
    drawn: prover_mult(mult) -> the ligero_pcs.Prover of mult's commitment and verifier_mult(that prover) -> the ExtVerifier of its
    openings (both None: committed as w is).  table_eval(point) = t~(point) in K as the verifier computes it (default: the table's own
    extension, ext_sumcheck.table_evaluate_ext; range_table_eval for a range table).  True, or the verifier's error (LookupMismatch
    when some w_i is outside the table at the drawn alpha)"""
    from . import ext_sumcheck
    ctx = prover_w.ctx
    F = ctx.field
    if F.p <= 1 << max(prover_w.num_vars, table.num_vars()):
        raise ValueError("p = %d: a count of up to 2^%d must be a field word" % (F.p, max(prover_w.num_vars, table.num_vars())))
    if prover_mult is None or verifier_mult is None:
        if prover_mult is not None or verifier_mult is not None:
            raise ValueError("prover_mult and verifier_mult come together")
        prover_mult, verifier_mult = _default_mult(prover_w, verifier_w, w)
    if table_eval is None:
        table_eval = lambda point: ext_sumcheck.table_evaluate_ext(ctx, w, table, point)   # noqa: E731
    P = LookupProver(prover_w, table, idx, w)
    try:
        pcs_mult = P.commit_mult(prover_mult)                                          # 1: before alpha
        V = LookupVerifier(F, w, verifier_w, verifier_mult(pcs_mult), table_eval)
        V.receive_roots(*P.roots(V.draw_alpha(rng)))                                   # 2, 3, 4
        for which in range(2):
            P.prove(which, V.frac[which].challenger(rng))
            point, _ = V.opening(which)
            pcs = (P.pcs_w, P.pcs_mult)[which]
            V.finish(which, ext_sumcheck.open_committed_ext(pcs, V.pcs[which], point, rng, w))   # 5, 6, 7
    finally:
        P.close()
    return True
