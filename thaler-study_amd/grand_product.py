"""The grand product argument: the product of the 2^n entries of a device table is P, reduced to one evaluation claim about the
table's multilinear extension (Thaler, "Proofs, Arguments, and Zero-Knowledge", section 4.6: GKR specialised to a binary tree of
multiplication gates; Spartan section 7) - and its first consumer, a permutation check between two Ligero-committed tables.

csrc/kernels/grand_product.hpp states the protocol; DESIGN.md section 9 item 16 describes the kernels.  In short:

  tree     V_n = t, V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k], x < 2^k; P = V_0[0]; L_k, R_k = the two halves of V_(k+1)
  layer k  turns V_k~(z_k) = c_k into a claim about V_(k+1): k rounds of a cubic sumcheck over sum_x eq(z_k, x) L_k(x) R_k(x),
           four values H(0..3) per round, variable 0 first; then the finals l = L~(r), r' = R~(r), checked as eq(z_k, r) l r'
           against the running claim; then rho_k, c_(k+1) = l + rho_k (r' - l), z_(k+1) = (r, rho_k).  z_0 = (), c_0 = P
  end      t~(z_n) = c_n, left to the caller: DenseMultilinearExtension.evaluate, or an opening of a commitment to t

Field elements are Montgomery words, as everywhere in this package.  Nothing beyond the book's statement is claimed: no security
level, no zero knowledge, no Fiat-Shamir.

  ProductTree, prove, Proof     sc_gp_*: the tree and the n layers on the device (the small layers and tails on the host)
  Verifier                      pure host code, O(n^2) field operations
  table_affine                  sc_table_affine: alpha t + beta
  PermutationProver, PermutationVerifier, prove_permutation"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import DRAW_GP_FN, u64, voidp
from .dense_mle import DenseMultilinearExtension, _u64p
from .relaxed_pcs import Error, _draw

MAX_LOG = 28
TAIL_LOG = 12          # kGpTailLog of csrc/kernels/grand_product.hpp: the one-block tail of the tree takes a layer of 2^this words
HOST_LOG_MAX = 12      # option "gp_host_log" at most


class ProductMismatch(Error):
    """the finals of layer 0 do not multiply to the claimed product"""

    def __init__(self, product, value):
        super().__init__("Layer 0: l r' is %d, the claimed product is %d" % (value, product))
        self.product, self.value = product, value


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim"""

    def __init__(self, layer, round_index, claim, total):
        super().__init__("Layer %d, round %d: H(0) + H(1) is %d, the claim is %d" % (layer, round_index, total, claim))
        self.layer, self.round, self.claim, self.total = layer, round_index, claim, total


class FinalMismatch(Error):
    """eq(z_k, r) l r' is not the last claim of the layer's sumcheck"""

    def __init__(self, layer, claim, value):
        super().__init__("Layer %d: the last claim is %d, eq(z, r) l r' is %d" % (layer, claim, value))
        self.layer, self.claim, self.value = layer, claim, value


class InputMismatch(Error):
    """the table's extension at z_n is not the claim the last layer left"""

    def __init__(self, claim, value):
        super().__init__("The last claim is %d, the table's extension at the point is %d" % (claim, value))
        self.claim, self.value = claim, value


class PermutationMismatch(Error):
    """the two grand products differ"""

    def __init__(self, product_a, product_b):
        super().__init__("The products are %d and %d" % (product_a, product_b))
        self.product_a, self.product_b = product_a, product_b


Proof = collections.namedtuple("Proof", "product rounds finals point claim challenges")
Proof.__doc__ = """product; rounds[k][j] = the four values of round j of layer k; finals[k] = (l, r'); point = z_n; claim = c_n;
challenges = every drawn word in protocol order (per layer its rounds' challenges, then rho)"""


# ---- the device side -------------------------------------------------------------------------------------------------

def table_affine(ctx, t, alpha, beta):
    """sc_table_affine: the table alpha t[i] + beta"""
    h = voidp()
    ctx.check(ctx.lib.sc_table_affine(ctx.h, t.h, int(alpha), int(beta), ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


class ProductTree:
    """sc_gp_create: the product tree of `table` (2^n entries, 1 <= n <= 28), which is kept alive and never written"""

    def __init__(self, ctx, table):
        self.ctx, self.table = ctx, table
        self.h = voidp()
        ctx.check(ctx.lib.sc_gp_create(ctx.h, table.h, ctypes.byref(self.h)))
        self.num_vars = table.num_vars()
        out = u64()
        ctx.check(ctx.lib.sc_gp_product(self.h, ctypes.byref(out)))
        self.product = int(out.value)

    def layer(self, k):
        """a copy of V_k, 0 <= k < n, as a device table of 2^k words"""
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_gp_layer(self.ctx.h, self.h, int(k), ctypes.byref(h)))
        return DenseMultilinearExtension(self.ctx, h)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_gp_destroy(self.ctx.h, self.h)
        self.h = None
        self.table = None

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
            width = 4 if j < layer else 2
            return int(draw(int(layer), int(j), [int(msg[k]) for k in range(width)]))
        except BaseException as exc:
            failure.append(exc)
            return ctx.field.p
    return cb, failure


def prove(tree, draw=None, seed_r=0):
    """sc_gp_prove.  draw(layer, round, msg) returns a challenge: round < layer, msg = [H(0), H(1), H(2), H(3)] -> r_round;
    round == layer, msg = [l, r'] -> rho_layer.  None: the synthetic challenger of sc_prove over seed_r.  Returns a Proof"""
    ctx, n = tree.ctx, tree.num_vars
    n_rounds = n * (n - 1) // 2
    evals, fin = np.zeros(4 * max(n_rounds, 1), dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64)
    ch, point, claim = np.zeros(n_rounds + n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), u64()
    cb, failure = _guarded(ctx, draw) if draw is not None else (None, [])
    rc = ctx.lib.sc_gp_prove(ctx.h, tree.h, DRAW_GP_FN(cb) if cb else ctypes.cast(None, DRAW_GP_FN), None, int(seed_r), _u64p(evals), _u64p(fin),
                             _u64p(ch), _u64p(point), ctypes.byref(claim))
    if failure:
        raise failure[0]
    ctx.check(rc)
    rounds, at = [], 0
    for k in range(n):
        rounds.append([[int(x) for x in evals[4 * (at + j):4 * (at + j) + 4]] for j in range(k)])
        at += k
    return Proof(tree.product, rounds, [(int(fin[2 * k]), int(fin[2 * k + 1])) for k in range(n)], [int(x) for x in point], int(claim.value),
                 [int(x) for x in ch])


# ---- the verifier ----------------------------------------------------------------------------------------------------

class _Replay:
    """recorded challenges served in order where a verifier draws"""

    def __init__(self, words):
        self.words, self.at = [int(w) for w in words], 0

    def draw(self):
        if self.at >= len(self.words):
            raise Error("the recorded challenges ran out")
        self.at += 1
        return self.words[self.at - 1]


class Verifier:
    """The verifier of the grand product of a table of n variables: pure host code.  begin(product), then per layer k its rounds
    round(k, j, values, rng) and finals(k, l, r', rng), each returning the drawn challenge; result() = (z_n, c_n).  verify()
    runs a whole Proof; challenger() is the draw of an interactive prove()."""

    def __init__(self, field, n):
        if not 1 <= n <= MAX_LOG:
            raise ValueError("n must be in 1..%d" % MAX_LOG)
        if field.p <= 3:
            raise ValueError("p = %d: the cubic through 0, 1, 2, 3 needs 2 and 3 invertible" % field.p)
        self.field, self.n = field, n
        self.inv2, self.inv6 = field.inv(field.from_int(2)), field.inv(field.from_int(6))
        self.product = None

    def begin(self, product):
        self.product, self.layer, self.z, self.claim, self.r = int(product), 0, [], int(product), []

    def _cubic_at(self, e, x):
        """the cubic through (0, e0) .. (3, e3) at x"""
        F = self.field
        pts = [0, F.one, F.from_int(2), F.from_int(3)]
        d = [F.sub(x, t) for t in pts]
        l0 = F.neg(F.mul(F.mul(F.mul(d[1], d[2]), d[3]), self.inv6))
        l1 = F.mul(F.mul(F.mul(d[0], d[2]), d[3]), self.inv2)
        l2 = F.neg(F.mul(F.mul(F.mul(d[0], d[1]), d[3]), self.inv2))
        l3 = F.mul(F.mul(F.mul(d[0], d[1]), d[2]), self.inv6)
        out = 0
        for ek, lk in zip(e, (l0, l1, l2, l3)):
            out = F.add(out, F.mul(int(ek), lk))
        return out

    def round(self, layer, j, values, rng):
        F = self.field
        if self.product is None or layer != self.layer or j != len(self.r) or j >= layer or len(values) != 4:
            raise Error("layer %d, round %d out of order" % (layer, j))
        total = F.add(int(values[0]), int(values[1]))
        if total != self.claim:
            raise RoundMismatch(layer, j, self.claim, total)
        r = _draw(F, rng)
        self.claim = self._cubic_at(values, r)
        self.r.append(r)
        return r

    def finals(self, layer, l, r, rng):
        F = self.field
        if self.product is None or layer != self.layer or len(self.r) != layer or layer >= self.n:
            raise Error("finals of layer %d out of order" % layer)
        eq = F.one
        for zi, ri in zip(self.z, self.r):
            zr = F.mul(zi, ri)
            eq = F.mul(eq, F.add(F.sub(F.sub(F.one, zi), ri), F.add(zr, zr)))
        value = F.mul(eq, F.mul(int(l), int(r)))
        if value != self.claim:
            if layer == 0:
                raise ProductMismatch(self.claim, value)
            raise FinalMismatch(layer, self.claim, value)
        rho = _draw(F, rng)
        self.claim = F.add(int(l), F.mul(rho, F.sub(int(r), int(l))))
        self.z, self.r, self.layer = self.r + [rho], [], layer + 1
        return rho

    def result(self):
        if self.product is None or self.layer != self.n:
            raise Error("result before the last layer")
        return list(self.z), self.claim

    def challenger(self, rng, product=None):
        """draw(layer, round, msg) for prove(): the verifier's checks and draws, message by message.  product: begin(product) first"""
        if product is not None:
            self.begin(product)

        def draw(layer, j, msg):
            return self.round(layer, j, msg, rng) if j < layer else self.finals(layer, msg[0], msg[1], rng)
        return draw

    def verify(self, proof, rng_or_challenges):
        """the whole proof; rng_or_challenges: where the challenges come from - an rng, or the recorded words in protocol order.
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

    def check_input(self, value):
        """the caller's last step: t~(z_n) = value against c_n"""
        _, claim = self.result()
        if int(value) != claim:
            raise InputMismatch(claim, int(value))
        return True


# ---- the consumer: b is a permutation of a -----------------------------------------------------------------------------
#
# V draws gamma; P forms gamma - a and gamma - b, builds two trees and runs two grand products; V checks that the products are
# equal, turns each final claim c into a~(z) = gamma - c (sum_x eq(z, x) = 1) and obtains a~(z_a), b~(z_b) from one opening each.

class PermutationProver:
    """over two ligero_pcs.Prover commitments to tables of 2^n entries of one context"""

    def __init__(self, pcs_a, pcs_b):
        if pcs_a.ctx is not pcs_b.ctx or pcs_a.num_vars != pcs_b.num_vars:
            raise ValueError("two commitments of one context to tables of one length")
        self.ctx, self.pcs, self.trees = pcs_a.ctx, (pcs_a, pcs_b), []

    def products(self, gamma):
        """the trees of gamma - a and gamma - b; returns the two products"""
        F = self.ctx.field
        self.close()
        self.trees = [ProductTree(self.ctx, table_affine(self.ctx, pcs.poly, F.neg(F.one), gamma)) for pcs in self.pcs]
        return tuple(t.product for t in self.trees)

    def prove(self, which, draw):
        return prove(self.trees[which], draw)

    def close(self):
        for t in self.trees:
            t.close()
        self.trees = []


class PermutationVerifier:
    """over the two verifiers of the commitments' openings (ligero_pcs.Verifier or FoldVerifier, built over the roots)"""

    def __init__(self, field, pcs_verifier_a, pcs_verifier_b):
        if pcs_verifier_a.num_vars != pcs_verifier_b.num_vars:
            raise ValueError("two commitments to tables of one length")
        self.field, self.n, self.pcs = field, pcs_verifier_a.num_vars, (pcs_verifier_a, pcs_verifier_b)
        self.gp = (Verifier(field, self.n), Verifier(field, self.n))
        self.gamma = None

    def draw_gamma(self, rng):
        self.gamma = _draw(self.field, rng)
        return self.gamma

    def receive_products(self, product_a, product_b):
        if self.gamma is None:
            raise Error("the products before gamma")
        if int(product_a) != int(product_b):
            raise PermutationMismatch(int(product_a), int(product_b))
        for v, product in zip(self.gp, (product_a, product_b)):
            v.begin(product)

    def opening(self, which):
        """(point, value the commitment must open to): a~(z) = gamma - c"""
        point, claim = self.gp[which].result()
        return point, self.field.sub(self.gamma, claim)

    def finish(self, which, opened):
        _, expected = self.opening(which)
        if int(opened) != expected:
            raise InputMismatch(expected, int(opened))
        return True


def prove_permutation(prover_a, prover_b, verifier_a, verifier_b, rng):
    """the whole exchange: prover_a, prover_b are ligero_pcs.Prover commitments to a and b, verifier_a, verifier_b the verifiers
    of their openings.  True, or the verifier's error (PermutationMismatch when the multisets differ at the drawn gamma)"""
    from . import r1cs
    P = PermutationProver(prover_a, prover_b)
    V = PermutationVerifier(prover_a.ctx.field, verifier_a, verifier_b)
    try:
        V.receive_products(*P.products(V.draw_gamma(rng)))
        for which in range(2):
            P.prove(which, V.gp[which].challenger(rng))
            point, _ = V.opening(which)
            V.finish(which, r1cs.open_committed(P.pcs[which], V.pcs[which], point, rng))
    finally:
        P.close()
    return True
