"""The grand product argument with every element in the quadratic extension K = F_p[X] / (X^2 - w), and its first consumer, a
permutation check between two Ligero-committed tables with gamma and every challenge in K.

csrc/kernels/ext_grand_product.hpp states the protocol - that of grand_product.py word for word, over K; DESIGN.md section 9 item 21
describes the kernels.  In short:

  leaves   V_n[i] = beta + alpha t[i], t a base-field device table of 2^n entries, alpha, beta in K, alpha != 0; never stored
  tree     V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k] in K; P = V_0[0]
  layer k  k rounds of a cubic sumcheck over sum_x eq(z_k, x) L_k(x) R_k(x), four values of K per round, challenges in K; the finals
           l, r' in K, checked as eq(z_k, r) l r'; then rho_k in K, c_(k+1) = l + rho_k (r' - l), z_(k+1) = (r, rho_k)
  end      V_n~(z_n) = c_n, that is t~(z_n) = (c_n - beta) / alpha: ext_sumcheck.table_evaluate_ext, or an opening of a commitment
           to t at the point of K^n

An element of K is a (c0, c1) pair of Montgomery words, as ext_field.QuadExt handles them.  With |K| = p^2 a run's soundness error
is about n^2 / p^2 instead of n^2 / p; nothing else is claimed: no Fiat-Shamir, no zero knowledge, and gamma of the Ligero
proximity test stays in the base field.

  ExtProductTree, prove_ext, Proof          sc_gp_*_ext: the tree and the n layers on the device (small layers and tails on the host)
  Verifier                                  pure host code, O(n^2) operations in K
  PermutationProver, PermutationVerifier, prove_permutation_ext"""
import collections
import ctypes

import numpy as np

from ._lib import DRAW_GP_EXT_FN, u64, voidp
from .dense_mle import DenseMultilinearExtension, _u64p
from .ext_field import QuadExt
from .relaxed_pcs import Error

MAX_LOG = 28
TAIL_LOG = 11          # kExtGpTailLog of csrc/kernels/ext_grand_product.hpp: the one-block tail of the tree takes a layer of 2^this entries


class ProductMismatch(Error):
    """the finals of layer 0 do not multiply to the claimed product"""

    def __init__(self, product, value):
        super().__init__("Layer 0: l r' is %s, the claimed product is %s" % (value, product))
        self.product, self.value = product, value


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim"""

    def __init__(self, layer, round_index, claim, total):
        super().__init__("Layer %d, round %d: H(0) + H(1) is %s, the claim is %s" % (layer, round_index, total, claim))
        self.layer, self.round, self.claim, self.total = layer, round_index, claim, total


class FinalMismatch(Error):
    """eq(z_k, r) l r' is not the last claim of the layer's sumcheck"""

    def __init__(self, layer, claim, value):
        super().__init__("Layer %d: the last claim is %s, eq(z, r) l r' is %s" % (layer, claim, value))
        self.layer, self.claim, self.value = layer, claim, value


class InputMismatch(Error):
    """beta + alpha t~(z_n) is not the claim the last layer left"""

    def __init__(self, claim, value):
        super().__init__("The last claim is %s, the leaves' extension at the point is %s" % (claim, value))
        self.claim, self.value = claim, value


class PermutationMismatch(Error):
    """the two grand products differ"""

    def __init__(self, product_a, product_b):
        super().__init__("The products are %s and %s" % (product_a, product_b))
        self.product_a, self.product_b = product_a, product_b


Proof = collections.namedtuple("Proof", "product rounds finals point claim challenges")
Proof.__doc__ = """every element a (c0, c1) pair: product; rounds[k][j] = the four values of round j of layer k; finals[k] = (l, r');
point = z_n; claim = c_n; challenges = every drawn element in protocol order (per layer its rounds' challenges, then rho)"""


def _pair(x):
    return (int(x[0]), int(x[1]))


def _pairs(words):
    return [(int(words[2 * i]), int(words[2 * i + 1])) for i in range(len(words) // 2)]


# ---- the device side -------------------------------------------------------------------------------------------------

class ExtProductTree:
    """sc_gp_create_ext: the product tree over K = QuadExt(field, w) of the leaves beta + alpha table[i].  `table` (2^n base words,
    1 <= n <= 28) is kept alive and never written; w is a Montgomery word, alpha and beta are (c0, c1) pairs"""

    def __init__(self, ctx, w, table, alpha, beta):
        self.ctx, self.table, self.w = ctx, table, int(w)
        self.alpha, self.beta = _pair(alpha), _pair(beta)
        self.h = voidp()
        a, b = (u64 * 2)(*self.alpha), (u64 * 2)(*self.beta)
        ctx.check(ctx.lib.sc_gp_create_ext(ctx.h, self.w, table.h, a, b, ctypes.byref(self.h)))
        self.num_vars = table.num_vars()
        out = (u64 * 2)()
        ctx.check(ctx.lib.sc_gp_product_ext(self.h, out))
        self.product = (int(out[0]), int(out[1]))

    def layer(self, k):
        """copies of the two planes of V_k, 0 <= k < n: (the c0 words, the c1 words), device tables of 2^k words each"""
        h0, h1 = voidp(), voidp()
        self.ctx.check(self.ctx.lib.sc_gp_layer_ext(self.ctx.h, self.h, int(k), ctypes.byref(h0), ctypes.byref(h1)))
        return DenseMultilinearExtension(self.ctx, h0), DenseMultilinearExtension(self.ctx, h1)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_gp_destroy_ext(self.ctx.h, self.h)
        self.h = None
        self.table = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prove_ext(tree, draw=None, seed_r=0):
    """sc_gp_prove_ext.  draw(layer, round, msg) returns a challenge, a (c0, c1) pair: round < layer, msg = [H(0), H(1), H(2), H(3)]
    (pairs) -> r_round; round == layer, msg = [l, r'] -> rho_layer.  None: the synthetic challenger over seed_r.  Returns a Proof"""
    ctx, n = tree.ctx, tree.num_vars
    n_rounds = n * (n - 1) // 2
    evals, fin = np.zeros(8 * max(n_rounds, 1), dtype=np.uint64), np.zeros(4 * n, dtype=np.uint64)
    ch, point, claim = np.zeros(2 * (n_rounds + n), dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64), (u64 * 2)()
    failure = []

    def cb(_user, layer, j, msg, out):
        try:
            width = 8 if j < layer else 4
            r = draw(int(layer), int(j), _pairs([int(msg[k]) for k in range(width)]))
            out[0], out[1] = int(r[0]), int(r[1])
        except BaseException as exc:      # an exception must not cross the C frames: the call ends, and it is raised again below
            failure.append(exc)
            out[0] = out[1] = ctx.field.p
    rc = ctx.lib.sc_gp_prove_ext(ctx.h, tree.h, DRAW_GP_EXT_FN(cb) if draw is not None else ctypes.cast(None, DRAW_GP_EXT_FN), None, int(seed_r),
                                 _u64p(evals), _u64p(fin), _u64p(ch), _u64p(point), claim)
    if failure:
        raise failure[0]
    ctx.check(rc)
    rounds, at = [], 0
    for k in range(n):
        rounds.append([_pairs(evals[8 * (at + j):8 * (at + j) + 8]) for j in range(k)])
        at += k
    return Proof(tree.product, rounds, [(_pair(fin[4 * k:4 * k + 2]), _pair(fin[4 * k + 2:4 * k + 4])) for k in range(n)], _pairs(point),
                 (int(claim[0]), int(claim[1])), _pairs(ch))


# ---- the verifier ----------------------------------------------------------------------------------------------------

class _Replay:
    """recorded challenges (pairs) served in order where a verifier draws"""

    def __init__(self, elements):
        self.elements, self.at = [_pair(e) for e in elements], 0

    def draw_ext(self):
        if self.at >= len(self.elements):
            raise Error("the recorded challenges ran out")
        self.at += 1
        return self.elements[self.at - 1]


def _draw_ext(K, rng):
    """an element of K: a _Replay's next pair, two draws of a sum_check_protocol.RngF, or K.rand of a random.Random"""
    if hasattr(rng, "draw_ext"):
        return rng.draw_ext()
    return (rng.draw(), rng.draw()) if hasattr(rng, "draw") else K.rand(rng)


class Verifier:
    """The verifier of the grand product over K = QuadExt(field, w) of a table of n variables: pure host code.  begin(product), then
    per layer k its rounds round(k, j, values, rng) and finals(k, l, r', rng), each returning the drawn challenge; result() =
    (z_n, c_n).  verify() runs a whole Proof; challenger() is the draw of an interactive prove_ext()."""

    def __init__(self, field, w, n):
        if not 1 <= n <= MAX_LOG:
            raise ValueError("n must be in 1..%d" % MAX_LOG)
        if field.p <= 3:
            raise ValueError("p = %d: the cubic through 0, 1, 2, 3 needs 2 and 3 invertible" % field.p)
        self.field, self.ext, self.n = field, QuadExt(field, w), n
        self.inv2, self.inv6 = field.inv(field.from_int(2)), field.inv(field.from_int(6))
        self.product = None

    def begin(self, product):
        self.product, self.layer, self.z, self.claim, self.r = _pair(product), 0, [], _pair(product), []

    def _cubic_at(self, e, x):
        """the cubic through (0, e0) .. (3, e3), e_t in K, at x in K"""
        F, K = self.field, self.ext
        d = [K.sub(x, K.from_base(F.from_int(t))) for t in range(4)]
        l0 = K.neg(K.scale(K.mul(K.mul(d[1], d[2]), d[3]), self.inv6))
        l1 = K.scale(K.mul(K.mul(d[0], d[2]), d[3]), self.inv2)
        l2 = K.neg(K.scale(K.mul(K.mul(d[0], d[1]), d[3]), self.inv2))
        l3 = K.scale(K.mul(K.mul(d[0], d[1]), d[2]), self.inv6)
        out = K.zero
        for ek, lk in zip(e, (l0, l1, l2, l3)):
            out = K.add(out, K.mul(_pair(ek), lk))
        return out

    def round(self, layer, j, values, rng):
        K = self.ext
        if self.product is None or layer != self.layer or j != len(self.r) or j >= layer or len(values) != 4:
            raise Error("layer %d, round %d out of order" % (layer, j))
        values = [_pair(v) for v in values]
        total = K.add(values[0], values[1])
        if total != self.claim:
            raise RoundMismatch(layer, j, self.claim, total)
        r = _draw_ext(K, rng)
        self.claim = self._cubic_at(values, r)
        self.r.append(r)
        return r

    def finals(self, layer, l, r, rng):
        K = self.ext
        if self.product is None or layer != self.layer or len(self.r) != layer or layer >= self.n:
            raise Error("finals of layer %d out of order" % layer)
        l, r = _pair(l), _pair(r)
        eq = K.one
        for zi, ri in zip(self.z, self.r):
            zr = K.mul(zi, ri)
            eq = K.mul(eq, K.add(K.sub(K.sub(K.one, zi), ri), K.add(zr, zr)))
        value = K.mul(eq, K.mul(l, r))
        if value != self.claim:
            if layer == 0:
                raise ProductMismatch(self.claim, value)
            raise FinalMismatch(layer, self.claim, value)
        rho = _draw_ext(K, rng)
        self.claim = K.add(l, K.mul(rho, K.sub(r, l)))
        self.z, self.r, self.layer = self.r + [rho], [], layer + 1
        return rho

    def result(self):
        if self.product is None or self.layer != self.n:
            raise Error("result before the last layer")
        return list(self.z), self.claim

    def challenger(self, rng, product=None):
        """draw(layer, round, msg) for prove_ext(): the verifier's checks and draws, message by message.  product: begin(product) first"""
        if product is not None:
            self.begin(product)

        def draw(layer, j, msg):
            return self.round(layer, j, msg, rng) if j < layer else self.finals(layer, msg[0], msg[1], rng)
        return draw

    def verify(self, proof, rng_or_challenges):
        """the whole proof; rng_or_challenges: where the challenges come from - an rng, or the recorded pairs in protocol order.
        Returns (z_n, c_n), or raises the error of the first message that does not fit"""
        rng = rng_or_challenges if hasattr(rng_or_challenges, "draw") or hasattr(rng_or_challenges, "random") else _Replay(rng_or_challenges)
        if len(proof.rounds) != self.n or len(proof.finals) != self.n:
            raise Error("a proof of %d layers for a table of %d variables" % (len(proof.rounds), self.n))
        self.begin(proof.product)
        for k in range(self.n):
            if len(proof.rounds[k]) != k:
                raise Error("layer %d has %d rounds" % (k, len(proof.rounds[k])))
            for j in range(k):
                self.round(k, j, proof.rounds[k][j], rng)
            self.finals(k, proof.finals[k][0], proof.finals[k][1], rng)
        return self.result()

    def check_input(self, value, alpha, beta):
        """the caller's last step: beta + alpha value, value = t~(z_n) in K, against c_n"""
        K = self.ext
        _, claim = self.result()
        got = K.add(_pair(beta), K.mul(_pair(alpha), _pair(value)))
        if got != claim:
            raise InputMismatch(claim, got)
        return True


# ---- the consumer: b is a permutation of a, gamma in K ---------------------------------------------------------------------
#
# V draws gamma in K; P builds the trees of gamma - a and gamma - b (alpha = (-1, 0), beta = gamma: no table is formed) and runs two
# grand products; V checks that the products are equal in K, turns each final claim c into a~(z) = gamma - c and obtains a~(z_a),
# b~(z_b) from one opening of each commitment at its point of K^n.

class PermutationProver:
    """over two ligero_pcs.Prover commitments to tables of 2^n entries of one context"""

    def __init__(self, pcs_a, pcs_b, w):
        if pcs_a.ctx is not pcs_b.ctx or pcs_a.num_vars != pcs_b.num_vars:
            raise ValueError("two commitments of one context to tables of one length")
        self.ctx, self.pcs, self.w, self.trees = pcs_a.ctx, (pcs_a, pcs_b), int(w), []

    def products(self, gamma):
        """the trees of gamma - a and gamma - b; returns the two products"""
        F = self.ctx.field
        self.close()
        self.trees = [ExtProductTree(self.ctx, self.w, pcs.poly, (F.neg(F.one), 0), gamma) for pcs in self.pcs]
        return tuple(t.product for t in self.trees)

    def prove(self, which, draw):
        return prove_ext(self.trees[which], draw)

    def close(self):
        for t in self.trees:
            t.close()
        self.trees = []


class PermutationVerifier:
    """over the two ligero_pcs.ExtVerifier of the commitments' openings (built over the roots and the same w)"""

    def __init__(self, field, w, pcs_verifier_a, pcs_verifier_b):
        if pcs_verifier_a.num_vars != pcs_verifier_b.num_vars:
            raise ValueError("two commitments to tables of one length")
        for v in (pcs_verifier_a, pcs_verifier_b):
            if not hasattr(v, "ext") or v.ext.w != int(w):
                raise ValueError("the verifiers are ligero_pcs.ExtVerifier over the same w")
        self.field, self.ext, self.n, self.pcs = field, QuadExt(field, w), pcs_verifier_a.num_vars, (pcs_verifier_a, pcs_verifier_b)
        self.gp = (Verifier(field, w, self.n), Verifier(field, w, self.n))
        self.gamma = None

    def draw_gamma(self, rng):
        self.gamma = _draw_ext(self.ext, rng)
        return self.gamma

    def receive_products(self, product_a, product_b):
        if self.gamma is None:
            raise Error("the products before gamma")
        if _pair(product_a) != _pair(product_b):
            raise PermutationMismatch(_pair(product_a), _pair(product_b))
        for v, product in zip(self.gp, (product_a, product_b)):
            v.begin(product)

    def opening(self, which):
        """(point, value the commitment must open to): a~(z) = gamma - c"""
        point, claim = self.gp[which].result()
        return point, self.ext.sub(self.gamma, claim)

    def finish(self, which, opened):
        _, expected = self.opening(which)
        if _pair(opened) != expected:
            raise InputMismatch(expected, _pair(opened))
        return True


def prove_permutation_ext(prover_a, prover_b, verifier_a, verifier_b, rng, w):
    """the whole exchange: prover_a, prover_b are ligero_pcs.Prover commitments to a and b, verifier_a, verifier_b the
    ligero_pcs.ExtVerifier of their openings over the same w (a Montgomery word).  True, or the verifier's error
    (PermutationMismatch when the multisets differ at the drawn gamma)"""
    from . import ext_sumcheck
    P = PermutationProver(prover_a, prover_b, w)
    V = PermutationVerifier(prover_a.ctx.field, w, verifier_a, verifier_b)
    try:
        V.receive_products(*P.products(V.draw_gamma(rng)))
        for which in range(2):
            P.prove(which, V.gp[which].challenger(rng))
            point, _ = V.opening(which)
            V.finish(which, ext_sumcheck.open_committed_ext(P.pcs[which], V.pcs[which], point, rng, w))
    finally:
        P.close()
    return True
