"""The sum-of-products sumcheck with challenges from the quadratic extension K = F_p[X] / (X^2 - w), and an inner-product argument
over two Ligero commitments built on it (csrc/kernels/ext_sumprod.hpp states the conventions).

The tables stay base-field Montgomery words.  The challenges, the round values and the finals are elements of K: (c0, c1) pairs of
Montgomery words, as ext_field.QuadExt handles them.  With |K| = p^2 the soundness error of a run is about 2 n / p^2 instead of
2 n / p; nothing else is claimed: no Fiat-Shamir, no zero knowledge, and gamma of the proximity test stays in the base field.

  sumprod_prove_ext, table_evaluate_ext  sc_sumprod_prove_ext, sc_table_evaluate_ext
  Verifier                               the host verifier of the sumcheck: round checks, then the final check
  prove_inner_product                    c = sum a b claimed, the sumcheck, the two finals discharged by two openings at the
                                         point of K^n (ligero_pcs.Prover.combine_ext / ExtVerifier)"""
import ctypes

import numpy as np

from ._lib import DRAW_EXT_FN, u64, voidp
from .dense_mle import _u64p, _words
from .ext_field import QuadExt
from .relaxed_pcs import Error

MAX_TABLES = 8         # kSumprodMaxPairs of csrc/kernels/multiopen.hpp
MAX_LOG = 28           # kGpMaxLog


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim (round 0: not the claimed sum)"""

    def __init__(self, round_index, claim, total):
        super().__init__("Round %d: H(0) + H(1) is %s, the claim is %s" % (round_index, total, claim))
        self.round, self.claim, self.total = round_index, claim, total


class FinalMismatch(Error):
    """sum_t fa_t fb_t is not the last claim of the sumcheck"""

    def __init__(self, claim, value):
        super().__init__("The last claim is %s, the product of the finals is %s" % (claim, value))
        self.claim, self.value = claim, value


# ---- the device side -------------------------------------------------------------------------------------------------

def _pairs(words):
    return [(int(words[2 * i]), int(words[2 * i + 1])) for i in range(len(words) // 2)]


def sumprod_prove_ext(ctx, w, a_tables, b_tables, draw=None, seed_r=0):
    """sc_sumprod_prove_ext: the sumcheck over sum_x sum_t a_t(x) b_t(x) with one sequence of challenges from K.  draw(round,
    [H(0), H(1), H(2)]) - three (c0, c1) pairs - returns the round's challenge, a pair; None: the synthetic challenger over seed_r.
    Returns (c1, rounds[n][3], challenges[n], finals_a[T], finals_b[T]), every element a (c0, c1) pair"""
    T = len(a_tables)
    if len(b_tables) != T:
        raise ValueError("as many a tables as b tables")
    n = a_tables[0].num_vars() if T else 0
    ha = (voidp * max(T, 1))(*[t.h for t in a_tables])
    hb = (voidp * max(T, 1))(*[t.h for t in b_tables])
    evals, ch, c1 = np.zeros(6 * max(n, 1), dtype=np.uint64), np.zeros(2 * max(n, 1), dtype=np.uint64), (u64 * 2)()
    fa, fb = np.zeros(2 * max(T, 1), dtype=np.uint64), np.zeros(2 * max(T, 1), dtype=np.uint64)
    failure = []

    def cb(_user, j, e, out):
        try:
            r = draw(int(j), _pairs([int(e[k]) for k in range(6)]))
            out[0], out[1] = int(r[0]), int(r[1])
        except BaseException as exc:      # an exception must not cross the C frames: the call ends, and it is raised again below
            failure.append(exc)
            out[0] = out[1] = ctx.field.p
    rc = ctx.lib.sc_sumprod_prove_ext(ctx.h, int(w), T, ha, hb, DRAW_EXT_FN(cb) if draw is not None else ctypes.cast(None, DRAW_EXT_FN), None,
                                      int(seed_r), c1, _u64p(evals), _u64p(ch), _u64p(fa), _u64p(fb))
    if failure:
        raise failure[0]
    ctx.check(rc)
    return ((int(c1[0]), int(c1[1])), [_pairs(evals[6 * j:6 * j + 6]) for j in range(n)], _pairs(ch[:2 * n]), _pairs(fa[:2 * T]), _pairs(fb[:2 * T]))


def table_evaluate_ext(ctx, w, table, point):
    """sc_table_evaluate_ext: the multilinear extension of a base-field device table at a point of K^n (a list of (c0, c1) pairs,
    coordinate 0 first), a (c0, c1) pair"""
    pt = _words([x for z in point for x in z])
    out = (u64 * 2)()
    ctx.check(ctx.lib.sc_table_evaluate_ext(ctx.h, int(w), table.h, _u64p(pt) if pt.size else None, len(point), out))
    return (int(out[0]), int(out[1]))


# ---- the verifier ----------------------------------------------------------------------------------------------------

class Verifier:
    """The host verifier of the sumcheck over K = QuadExt(field, w): claim(c), round(j, evals, rng) n times, final(finals_a,
    finals_b) - in that order.  .z is the point the challenges form, .claim the running claim"""

    def __init__(self, field, w, num_vars):
        if not 1 <= num_vars <= MAX_LOG:
            raise ValueError("num_vars must be in 1..%d" % MAX_LOG)
        self.field, self.ext, self.num_vars = field, QuadExt(field, w), int(num_vars)
        self.inv2 = field.inv(field.from_int(2))
        self.claim, self.z = None, []

    def start(self, claim):
        """the claimed sum, an element of K (a base word c is (c, 0))"""
        if self.claim is not None:
            raise Error("the claim is set once")
        self.claim = (int(claim[0]), int(claim[1]))

    def quadratic_at(self, e, x):
        """the quadratic through (0, e[0]), (1, e[1]), (2, e[2]) at x in K"""
        F, K = self.field, self.ext
        d = [x, K.sub(x, K.one), K.sub(x, K.from_base(F.from_int(2)))]
        l0 = K.scale(K.mul(d[1], d[2]), self.inv2)
        l1 = K.neg(K.mul(d[0], d[2]))
        l2 = K.scale(K.mul(d[0], d[1]), self.inv2)
        return K.add(K.add(K.mul(e[0], l0), K.mul(e[1], l1)), K.mul(e[2], l2))

    def round(self, j, evals, rng):
        K = self.ext
        if self.claim is None or j != len(self.z) or j >= self.num_vars or len(evals) != 3:
            raise Error("round %d out of order" % j)
        evals = [(int(e[0]), int(e[1])) for e in evals]
        total = K.add(evals[0], evals[1])
        if total != self.claim:
            raise RoundMismatch(j, self.claim, total)
        r = K.rand(rng) if not hasattr(rng, "draw") else (rng.draw(), rng.draw())
        self.claim = self.quadratic_at(evals, r)
        self.z.append(r)
        return r

    def final(self, finals_a, finals_b):
        """the last check: claim = sum_t fa_t fb_t.  Whoever calls this owes the finals' own proofs (openings at .z)"""
        K = self.ext
        if len(self.z) != self.num_vars:
            raise Error("the final check comes after the last round")
        if len(finals_a) != len(finals_b) or not finals_a:
            raise Error("as many finals of a as of b, at least one")
        value = K.zero
        for fa, fb in zip(finals_a, finals_b):
            value = K.add(value, K.mul((int(fa[0]), int(fa[1])), (int(fb[0]), int(fb[1]))))
        if value != self.claim:
            raise FinalMismatch(self.claim, value)
        return True


# ---- an inner-product claim, end to end --------------------------------------------------------------------------------

def open_committed_ext(pcs_prover, pcs_verifier, point, rng, w=None):
    """one opening of a base-field commitment at a point of K^n between a ligero_pcs.Prover and a ligero_pcs.ExtVerifier; returns
    the value the verifier accepts, an element of K"""
    gamma = pcs_verifier.draw_gamma(rng)
    pcs_verifier.receive(*pcs_prover.combine_ext(point, gamma, w))
    return pcs_verifier.verify(point, pcs_prover.open_columns(pcs_verifier.draw_columns(rng)))


def prove_inner_product(ctx, w, prover_a, prover_b, verifier_a, verifier_b, rng):
    """c = sum_x a(x) b(x) for two committed tables (ligero_pcs.Prover; the verifiers are ligero_pcs.ExtVerifier over the same w):
    the prover claims c, the sumcheck runs at T = 1 with challenges from K, and the two finals it ends in are discharged by two
    openings at the point of K^n.  Returns c (a Montgomery word), or raises the failing check's error"""
    from . import ligero_pcs
    for v in (verifier_a, verifier_b):
        if not isinstance(v, ligero_pcs.ExtVerifier) or v.ext.w != int(w):
            raise ValueError("the verifiers are ligero_pcs.ExtVerifier over the same w")
    n = prover_a.num_vars
    if prover_b.num_vars != n or verifier_a.num_vars != n or verifier_b.num_vars != n:
        raise ValueError("both tables have the same number of variables")
    V = Verifier(ctx.field, w, n)
    claimed = []

    def draw(j, evals):
        if j == 0:                        # the claim is the prover's first message: H_0(0) + H_0(1), a base word
            claimed.append(V.ext.add(evals[0], evals[1]))
            if claimed[0][1] != 0:
                raise RoundMismatch(0, (claimed[0][0], 0), claimed[0])
            V.start(claimed[0])
        return V.round(j, evals, rng)
    c1, _, z, fa, fb = sumprod_prove_ext(ctx, w, [prover_a.poly], [prover_b.poly], draw)
    if c1 != claimed[0]:
        raise RoundMismatch(0, claimed[0], c1)
    # the finals are claims about the committed tables: the openings give the values the verifier trusts
    va = open_committed_ext(prover_a, verifier_a, z, rng, w)
    vb = open_committed_ext(prover_b, verifier_b, z, rng, w)
    V.final([va], [vb])
    return c1[0]
