"""Python mirror of the reference crate `matrix-multiplication` (src/lib.rs):
`G` = f_A(r1, z) * f_B(z, r2) as two device tables (:12-15), `G::new` (:77-92), the
`SumCheckPolynomial` impl (:95-147) and `interpolate_quadratic_poly` (:17-60)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import u64, u64p, voidp
from .dense_mle import DenseMultilinearExtension, _u64p, _words
from .sum_check_protocol import SparsePolynomial, SumCheckPolynomial


def interpolate_quadratic_poly(field, points):
    """:17-60 - generic three-point Lagrange form, like the reference"""
    polys = []
    for i in range(3):
        (xi, yi), (xj, _), (xk, _) = points[i], points[(i + 1) % 3], points[(i + 2) % 3]
        den = field.mul(field.sub(xi, xj), field.sub(xi, xk))
        coeffs = [(0, field.mul(xj, xk)), (1, field.sub(field.neg(xj), xk)), (2, field.one)]
        coeffs = [(d, field.div(field.mul(c, yi), den)) for d, c in coeffs]
        polys.append(SparsePolynomial.from_coefficients_vec(field, coeffs))
    return polys[0] + polys[1] + polys[2]


def _round_poly_from_evals(ctx, e):
    """the three sums -> the round polynomial as triangle_counting::G and W hand it out: coefficients through
    sc_interpolate_quadratic, then `DensePolynomial -> SparsePolynomial` (`p.into()`,
    triangle-counting/src/lib.rs:129-131, gkr-protocol/src/round_polynomial.rs:87-89): non-zero terms only"""
    ev = (u64 * 3)(*[int(x) for x in e])
    c = (u64 * 3)()
    ctx.check(ctx.lib.sc_interpolate_quadratic(ctx.field.ref(), ev, c))
    return SparsePolynomial.from_dense(ctx.field, [int(c[d]) for d in range(3)])


def _round_poly_lagrange(ctx, e):
    """the three sums -> the round polynomial as matrix_multiplication::G hands it out (:124-130): the sum of three
    Lagrange terms, which in arkworks' canonical form can carry an explicit zero constant term (e.g. H(0) = H(2) = 0)
    - the same values as sc_interpolate_quadratic's, and on the wire the reference's bytes"""
    f = ctx.field
    poly = interpolate_quadratic_poly(f, [(f.zero, int(e[0])), (f.one, int(e[1])), (f.two, int(e[2]))])
    return poly


class _NativeProver:
    """sc_prover: the fused fold + round-sum engine behind Prover::round"""

    def __init__(self, g):
        self.ctx = g.ctx
        self._g = g  # keeps the borrowed tables alive
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_prover_create(self.ctx.h, g.f_a.h, g.f_b.h, ctypes.byref(h)))
        self.h = h
        self.last_evals = None

    def c1(self):
        out = u64()
        self.ctx.check(self.ctx.lib.sc_prover_c1(self.h, ctypes.byref(out)))
        return int(out.value)

    def round_evals(self, r_prev, j):
        e = (u64 * 3)()
        self.ctx.check(self.ctx.lib.sc_prover_round(self.h, int(r_prev), j, e))
        self.last_evals = [int(x) for x in e]
        return self.last_evals

    def round(self, r_prev, j):
        return _round_poly_lagrange(self.ctx, self.round_evals(r_prev, j))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.sc_prover_destroy(self.h)
                self.h = None
        except Exception:
            pass


class G(SumCheckPolynomial):
    """:12-15"""

    def __init__(self, f_a, f_b):
        self.f_a, self.f_b = f_a, f_b
        self.ctx = f_a.ctx
        self.field = self.ctx.field

    @classmethod
    def new(cls, ctx, n, a, b, point):
        """:77-92 - a, b: the 2^n x 2^n matrices flattened row-major (Montgomery words)"""
        A = DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, a)
        B = DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, b)
        pt = _words(point)
        if pt.size != 2 * n:
            raise ValueError("point must have 2n entries")
        ha, hb = voidp(), voidp()
        ctx.check(ctx.lib.sc_matmul_g_new(ctx.h, A.h, B.h, n, _u64p(pt), ctypes.byref(ha), ctypes.byref(hb)))
        f_a, f_b = DenseMultilinearExtension(ctx, ha), DenseMultilinearExtension(ctx, hb)
        assert f_a.num_vars() == n and f_b.num_vars() == n                 # :88-89
        return cls(f_a, f_b)

    @classmethod
    def new_from_tables(cls, ctx, n, A, B, point):
        """G::new on matrices that already live in HBM (2^(2n)-entry device tables)"""
        pt = _words(point)
        ha, hb = voidp(), voidp()
        ctx.check(ctx.lib.sc_matmul_g_new(ctx.h, A.h, B.h, n, _u64p(pt), ctypes.byref(ha), ctypes.byref(hb)))
        return cls(DenseMultilinearExtension(ctx, ha), DenseMultilinearExtension(ctx, hb))

    def clone(self):
        """#[derive(Clone)] :11 - tables are never written by the prover, so share them"""
        return G(self.f_a, self.f_b)

    # ---- SumCheckPolynomial (:95-147) ---------------------------------------------------
    def evaluate(self, point):
        pt = _words(point)
        if pt.size != self.num_vars():
            return None
        out = u64()
        self.ctx.check(self.ctx.lib.sc_prod2_evaluate(self.ctx.h, self.f_a.h, self.f_b.h, _u64p(pt), pt.size,
                                                     ctypes.byref(out)))
        return int(out.value)

    def fix_variables(self, partial_point):
        return G(self.f_a.fix_variables(partial_point), self.f_b.fix_variables(partial_point))

    def round_evals(self):
        e = (u64 * 3)()
        self.ctx.check(self.ctx.lib.sc_prod2_round_sums(self.ctx.h, self.f_a.h, self.f_b.h, e))
        return [int(x) for x in e]

    def to_univariate(self):
        return _round_poly_lagrange(self.ctx, self.round_evals())

    def fold_and_univariate(self, r):
        """fix_variables(&[r]) + to_univariate in one pass over HBM"""
        rr = (u64 * 1)(int(r))
        ha, hb = voidp(), voidp()
        e = (u64 * 3)()
        self.ctx.check(self.ctx.lib.sc_prod2_fold_and_sums(self.ctx.h, self.f_a.h, self.f_b.h, rr,
                                                          ctypes.byref(ha), ctypes.byref(hb), e))
        g = G(DenseMultilinearExtension(self.ctx, ha), DenseMultilinearExtension(self.ctx, hb))
        return g, _round_poly_lagrange(self.ctx, [int(x) for x in e])

    def num_vars(self):
        return self.f_a.num_vars() + self._log_world()

    def to_evaluations(self):
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_prod2_to_evaluations(self.ctx.h, self.f_a.h, self.f_b.h, ctypes.byref(h)))
        return DenseMultilinearExtension(self.ctx, h).to_evaluations()

    # ---- provided-method overrides: keep Prover::new / round on the device ---------------
    def hypercube_sum(self, field=None):
        out = u64()
        self.ctx.check(self.ctx.lib.sc_prod2_sum(self.ctx.h, self.f_a.h, self.f_b.h, ctypes.byref(out)))
        return int(out.value)

    def native_prover(self):
        return _NativeProver(self)

    def _log_world(self):
        _, world = self.ctx.rank_world()
        return world.bit_length() - 1


def prove(ctx, g, seed_r, draw=None):
    """sc_prove: the whole loop of benches/mm_benchmark.rs:88-96 in one native call.
    Returns (c_1, evals[n][3], challenges[n])."""
    buf = getattr(g, "_prove_buf", None)
    if buf is None:  # output buffers and their ctypes views are built once per G (a benchmark loop
        n = g.num_vars()  # proves the same G many times; this keeps the wrapper out of its timing)
        ev = np.zeros(3 * max(n, 1), dtype=np.uint64)
        ch = np.zeros(max(n, 1), dtype=np.uint64)
        c1 = u64()
        buf = g._prove_buf = (n, ev, ch, c1, _u64p(ev), _u64p(ch), ctypes.byref(c1), ctypes.cast(None, _lib.DRAW_FN))
    n, ev, ch, c1, p_ev, p_ch, p_c1, no_draw = buf
    cb = _lib.DRAW_FN(draw) if draw is not None else no_draw
    ctx.check(ctx.lib.sc_prove(ctx.h, g.f_a.h, g.f_b.h, cb, None, seed_r, p_c1, p_ev, p_ch))
    return int(c1.value), ev[: 3 * n].reshape(n, 3).copy(), ch[:n].copy()


def _batch_seeds(seed_r, count):
    """seed_r of prove_batch: None -> _SEED_R + i for instance i, an int -> the same seed for every instance, a sequence ->
    one seed per instance"""
    if seed_r is None:
        return [(_SEED_R + i) & _MASK64 for i in range(count)]
    if isinstance(seed_r, (int, np.integer)):
        return [int(seed_r) & _MASK64] * count
    seeds = [int(x) for x in seed_r]
    if len(seeds) != count:
        raise ValueError("seed_r has %d entries for %d instances" % (len(seeds), count))
    return [x & _MASK64 for x in seeds]


def prove_batch(ctx, gs, seed_r=None, draw=None):
    """sc_prove_batch: B independent proofs of G_i = f_a * f_b, all with the same num_vars, proved together (one launch per
    pass for the whole batch).  Instance i gets exactly what prove(ctx, gs[i], seed_r[i], ...) gives it alone.
    seed_r: None (instance i uses _SEED_R + i), one int for all, or one per instance.  draw(instance, round, evals) -> the
    challenge (called round by round, within a round in instance order); None: the synthetic challenger.
    Returns [(c_1, evals[n][3], challenges[n])] per instance."""
    gs = list(gs)
    if not gs:
        raise ValueError("prove_batch needs at least one instance")
    for g in gs:
        if not isinstance(g, G):
            raise TypeError("prove_batch takes matrix_multiplication.G instances, not %s" % type(g).__name__)
        if g.ctx is not ctx:
            raise ValueError("every instance must live on the context the batch runs on")
    if draw is not None and not callable(draw):
        raise TypeError("draw must be callable (instance, round, evals) -> challenge")
    seeds = _batch_seeds(seed_r, len(gs))
    n = gs[0].num_vars()
    if any(g.num_vars() != n for g in gs):
        raise ValueError("every instance of a batch must have the same num_vars")
    B = len(gs)
    ta = (voidp * B)(*[g.f_a.h for g in gs])
    tb = (voidp * B)(*[g.f_b.h for g in gs])
    sd = np.array(seeds, dtype=np.uint64)
    c1 = np.zeros(B, dtype=np.uint64)
    ev = np.zeros(3 * max(n, 1) * B, dtype=np.uint64)
    ch = np.zeros(max(n, 1) * B, dtype=np.uint64)
    if draw is None:
        cb = ctypes.cast(None, _lib.DRAW_BATCH_FN)
    else:
        cb = _lib.DRAW_BATCH_FN(lambda _user, i, j, e: int(draw(int(i), int(j), [int(e[0]), int(e[1]), int(e[2])])))
    ctx.check(ctx.lib.sc_prove_batch(ctx.h, B, ta, tb, cb, None, _u64p(sd), _u64p(c1), _u64p(ev), _u64p(ch)))
    ev = ev[: 3 * n * B].reshape(B, n, 3)
    ch = ch[: n * B].reshape(B, n)
    return [(int(c1[i]), ev[i].copy(), ch[i].copy()) for i in range(B)]


# ---- the product itself and the MatMult protocol around it (the reference's tests: `randomized_test`, `matrix_test_from_book`) ----

_MASK64 = 2**64 - 1
_SEED_R = 0xC7C7000000000003   # synthetic.SEED_R: the default challenger of sc_prove
SEED_PT = 0xD8D8000000000004   # default seed of the point (r1, r2)


def _splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def product_point(field, n, seed_pt=SEED_PT):
    """the point (r1, r2) as 2n Montgomery words, drawn in this order: r1 (the row point of A and C) first, then r2
    (the column point of B and C); entry i is splitmix64(seed_pt + i + 1) mod p"""
    return [field.from_int(_splitmix64((seed_pt + i + 1) & _MASK64) % field.p) for i in range(2 * n)]


def _as_matrix(ctx, n, M):
    if isinstance(M, DenseMultilinearExtension):
        return M
    return DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * n, M)


def matmul(ctx, n, A, B):
    """C = A * B (sc_matmul) for 2^n x 2^n matrices flattened row-major: device tables or host arrays of Montgomery
    words; returns C as a device table"""
    A, B = _as_matrix(ctx, n, A), _as_matrix(ctx, n, B)
    h = voidp()
    ctx.check(ctx.lib.sc_matmul(ctx.h, A.h, B.h, n, ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


def product_claim(C, point):
    """f~_C(r1, r2): C's index is (row << n) | col and its variables are LE, so the column point r2 comes first"""
    n = len(point) // 2
    return C.evaluate(list(point[n:]) + list(point[:n]))


class ProductProof:
    """the prover's side of MatMult: C, the point (r1, r2), the claim f~_C(r1, r2), c_1 and the sumcheck transcript over
    G(z) = f~_A(r1, z) f~_B(z, r2) (evals[j] = g_j(0), g_j(1), g_j(2); challenges[j] = r_j)"""

    def __init__(self, C, point, claim, c_1, evals, challenges):
        self.C, self.point, self.claim, self.c_1 = C, list(point), claim, c_1
        self.evals, self.challenges = evals, challenges


def prove_product(ctx, n, A, B, C=None, seed_r=_SEED_R, draw=None, point=None, seed_pt=SEED_PT):
    """MatMult, prover side: C on the device if not given (sc_matmul), the point (product_point order unless given),
    claim = f~_C(r1, r2) (sc_table_evaluate), G::new on the device tables and the sumcheck (sc_prove)"""
    A, B = _as_matrix(ctx, n, A), _as_matrix(ctx, n, B)
    C = matmul(ctx, n, A, B) if C is None else _as_matrix(ctx, n, C)
    pt = product_point(ctx.field, n, seed_pt) if point is None else [int(x) for x in point]
    claim = product_claim(C, pt)
    g = G.new_from_tables(ctx, n, A, B, pt)
    c_1, evals, challenges = prove(ctx, g, seed_r, draw)
    return ProductProof(C, pt, claim, c_1, evals, challenges)


def prove_products(ctx, n, pairs, Cs=None, seed_r=None, draw=None, points=None, seed_pt=SEED_PT):
    """MatMult, prover side, for many products of 2^n x 2^n matrices: per pair (A, B) what prove_product does - C (sc_matmul
    unless Cs gives it), the point (product_point order unless points gives one per pair), the claim f~_C(r1, r2), G::new -
    with the sumchecks of all pairs proved together (prove_batch; seed_r and draw as there).  Returns one ProductProof per
    pair, each accepted by verify_product as it stands."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 14:
        raise ValueError("n must be an int in 0..14 (2^n x 2^n matrices)")
    n = int(n)
    pairs = list(pairs)
    if not pairs:
        raise ValueError("prove_products needs at least one (A, B) pair")
    if any(not isinstance(pr, (tuple, list)) or len(pr) != 2 for pr in pairs):
        raise TypeError("pairs must be (A, B) tuples")
    if Cs is not None:
        Cs = list(Cs)
        if len(Cs) != len(pairs):
            raise ValueError("Cs has %d entries for %d pairs" % (len(Cs), len(pairs)))
    if points is not None:
        points = [[int(x) for x in pt] for pt in points]
        if len(points) != len(pairs) or any(len(pt) != 2 * n for pt in points):
            raise ValueError("points must hold one point of 2n = %d words per pair" % (2 * n))
    if draw is not None and not callable(draw):
        raise TypeError("draw must be callable (instance, round, evals) -> challenge")
    seeds = _batch_seeds(seed_r, len(pairs))
    Cm, pts, claims, gs = [], [], [], []
    for i, (A, B) in enumerate(pairs):
        A, B = _as_matrix(ctx, n, A), _as_matrix(ctx, n, B)
        C = matmul(ctx, n, A, B) if Cs is None or Cs[i] is None else _as_matrix(ctx, n, Cs[i])
        pt = product_point(ctx.field, n, seed_pt) if points is None else points[i]
        Cm.append(C)
        pts.append(pt)
        claims.append(product_claim(C, pt))
        gs.append(G.new_from_tables(ctx, n, A, B, pt))
    out = prove_batch(ctx, gs, seeds, draw)
    return [ProductProof(Cm[i], pts[i], claims[i], *out[i]) for i in range(len(pairs))]


def verify_transcript(field, n, claim, c_1, evals, challenges, oracle):
    """the host verifier of MatMult over a transcript: c_1 must equal the claim, then sum_check_protocol.Verifier (strict)
    round by round with the transcript's challenges, and g_n(r_n) == oracle(r) at the end (also for n = 1, where the
    reference's Verifier never reaches its final branch).  oracle(point) -> G(point).  Returns True / False."""
    from .sum_check_protocol import Error, Verifier

    if int(c_1) != int(claim) or len(evals) != n or len(challenges) < n:
        return False

    class _G:   # oracle access for the verifier's final round
        def evaluate(self, r):
            return oracle(r)

    class _Script:
        def __init__(self):
            self.j = 0

        def draw(self):
            r = int(challenges[self.j])
            self.j += 1
            return r

    v = Verifier.new(n, _G(), field, strict=True)
    v.set_c_1(int(c_1))
    rng, polys = _Script(), []
    try:
        for j in range(n):
            e = [int(x) for x in evals[j]]
            poly = interpolate_quadratic_poly(field, [(field.zero, e[0]), (field.one, e[1]), (field.two, e[2])])
            polys.append(poly)
            res = v.round(poly, rng)
            if res.is_final() and not res.value:
                return False
    except Error:
        return False
    if n == 1:
        r = [int(challenges[0])]
        return polys[0].evaluate(r[0]) == oracle(r)
    return True


def verify_product(ctx, n, A, B, C, proof):
    """MatMult, verifier side: the claim is recomputed from C (the product under test), then verify_transcript with
    G.evaluate on the device tables as the oracle.  A C with a wrong entry changes f~_C(r1, r2) and is rejected."""
    A, B, C = _as_matrix(ctx, n, A), _as_matrix(ctx, n, B), _as_matrix(ctx, n, C)
    claim = product_claim(C, proof.point)
    if claim != proof.claim:
        return False
    g = G.new_from_tables(ctx, n, A, B, proof.point)
    return verify_transcript(ctx.field, n, claim, proof.c_1, proof.evals, proof.challenges, g.evaluate)
