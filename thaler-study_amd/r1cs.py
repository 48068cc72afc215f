"""An argument for rank-1 constraint satisfiability, (A z) o (B z) = C z, with a committed witness (Thaler, "Proofs, Arguments,
and Zero-Knowledge", section 8.4: Spartan's two sumchecks; the witness half of z committed by ligero_pcs).

csrc/kernels/r1cs.hpp states the protocol; DESIGN.md section 9 item 15 describes the kernels.  In short, with A, B, C of
2^s x 2^m and z = (x, w), x = (1, io_1, .., io_k, 0, ..) public and w committed (m - 1 variables each):

  1. P sends the root of w                          6. sumcheck 2: sc_prove(T, z), m rounds, claim rho . (v_A, v_B, v_C), ends at r_y
  2. V draws tau in F^s                             7. V computes T~(r_y) from the instance (R1CS.bind_eval), O(nnz + 2^s + 2^m)
  3. sumcheck 1, cubic: sum_x eq(tau, x)            8. V computes x~(r_y[:m-1]) from the public inputs
     (Az(x) Bz(x) - Cz(x)) = 0, s rounds of four    9. V obtains w~(r_y[:m-1]) from one opening of the commitment (the plain
     values, ends at r_x; P sends v_A, v_B, v_C        Verifier, or a folded opening when it is a FoldVerifier)
  4. V draws rho_A, rho_B, rho_C                   10. V checks T~(r_y) z~(r_y) against the last claim
  5. P builds T[y] = sum_k rho_k sum_i eq(r_x, i) M_k[i][y]

Field elements are Montgomery words, as everywhere in this package.  Verifier reads the instance in step 7; SublinearVerifier
holds the five roots of DeviceR1CS.commit_instance in its place and takes T~(r_y) from the SPARK exchange of spark.py (DESIGN.md
section 9 item 18).  Nothing beyond the book's statement of each part is claimed: no security level, no zero knowledge, no
Fiat-Shamir.

  R1CS              the instance on the host: is_satisfied, mul, bind_eval
  DeviceR1CS        sc_r1cs_*: mul (A z, B z, C z), bind_rows (T) and row_weights on the device; commit_instance
  zerocheck_prove   sc_zerocheck_prove: the cubic sumcheck over any three tables
  Prover, Verifier, prove_and_verify; synthetic_instance
  SublinearVerifier, prove_and_verify_sublinear"""
import ctypes
import random

import numpy as np

from . import _lib, ligero_pcs
from ._lib import DRAW4_FN, DRAW_FN, u64, u64p, voidp
from .dense_mle import DenseMultilinearExtension, _u64p, _words
from .ligero_pcs import EvalMismatch, FoldMismatch, MerkleMismatch, ProximityMismatch, eq_weights  # noqa: F401 (passed through)
from .relaxed_pcs import Error, _draw

SPMV_BLOCK_ENTRIES = 2048      # kSpmvBlockEntries of csrc/kernels/r1cs.hpp: the run of entries one block of the sparse product owns
MAX_LOG = 26


class RoundMismatch(Error):
    """H(0) + H(1) of a round polynomial is not the running claim; phase 1 = the cubic sumcheck, 2 = the product sumcheck"""

    def __init__(self, phase, round_index, claim, total):
        super().__init__("Sumcheck %d, round %d: H(0) + H(1) is %d, the claim is %d" % (phase, round_index, total, claim))
        self.phase, self.round, self.claim, self.total = phase, round_index, claim, total


class FinalMismatch(Error):
    """the last claim of a sumcheck is not what the verifier computes at the bound point"""

    def __init__(self, phase, claim, value):
        super().__init__("Sumcheck %d: the last claim is %d, the polynomial at the bound point is %d" % (phase, claim, value))
        self.phase, self.claim, self.value = phase, claim, value


# ---- the instance ----------------------------------------------------------------------------------------------------

class R1CS:
    """A, B, C in F^(2^s x 2^m) as lists of (row, col, val) triples, val a Montgomery word; equal (row, col) add.  Pure host code."""

    def __init__(self, field, s, m, A, B, C):
        if not 1 <= s <= MAX_LOG or not 2 <= m <= MAX_LOG:
            raise ValueError("s must be in 1..%d and m in 2..%d" % (MAX_LOG, MAX_LOG))
        self.field, self.s, self.m = field, s, m
        self.matrices = tuple([(int(i), int(j), int(v)) for i, j, v in M] for M in (A, B, C))
        for M in self.matrices:
            for i, j, v in M:
                if not (0 <= i < 1 << s and 0 <= j < 1 << m and 0 <= v < field.p):
                    raise ValueError("the triple (%d, %d, %d) is outside 2^%d x 2^%d, or not a word below p" % (i, j, v, s, m))

    def mul(self, z):
        """(A z, B z, C z), lists of 2^s words"""
        F = self.field
        out = []
        for M in self.matrices:
            y = [0] * (1 << self.s)
            for i, j, v in M:
                y[i] = F.add(y[i], F.mul(v, int(z[j])))
            out.append(y)
        return tuple(out)

    def is_satisfied(self, z):
        F = self.field
        az, bz, cz = self.mul(z)
        return all(F.mul(a, b) == c for a, b, c in zip(az, bz, cz))

    def bind_eval(self, rx, ry, rho):
        """T~(r_y) = sum_k rho_k sum_{(i, j, v) in M_k} eq(r_x, i) v eq(r_y, j)"""
        F = self.field
        ex, ey = eq_weights(F, list(rx)), eq_weights(F, list(ry))
        total = 0
        for M, rk in zip(self.matrices, rho):
            t = 0
            for i, j, v in M:
                t = F.add(t, F.mul(F.mul(ex[i], v), ey[j]))
            total = F.add(total, F.mul(int(rk), t))
        return total

    def assignment(self, io, w):
        """z = (1, io_1, .., io_k, 0, .. | w)"""
        half = 1 << (self.m - 1)
        if len(io) + 1 > half or len(w) != half:
            raise ValueError("the public half holds 1 and at most %d inputs, the witness %d words" % (half - 1, half))
        return [self.field.one] + [int(x) for x in io] + [0] * (half - 1 - len(io)) + [int(x) for x in w]


def synthetic_instance(field, s, m, seed, row_nnz=3):
    """(R1CS, io, w) of a satisfied instance: z random with z[0] = 1 (no public input beyond it); A and B have row_nnz random
    entries per row; C has one entry per row, at column 0, with the value (A z)_i (B z)_i - column 0 of C is the dense constant
    column"""
    rng = random.Random(seed)
    n_rows, n_cols = 1 << s, 1 << m
    half = n_cols // 2
    z = [field.one] + [0] * (half - 1) + [field.rand(rng) for _ in range(half)]
    A = [(i, rng.randrange(n_cols), field.rand(rng)) for i in range(n_rows) for _ in range(row_nnz)]
    B = [(i, rng.randrange(n_cols), field.rand(rng)) for i in range(n_rows) for _ in range(row_nnz)]
    probe = R1CS(field, s, m, A, B, [])
    az, bz, _ = probe.mul(z)
    C = [(i, 0, field.mul(az[i], bz[i])) for i in range(n_rows)]      # times z[0] = 1
    return R1CS(field, s, m, A, B, C), [], z[half:]


# ---- the device side -------------------------------------------------------------------------------------------------

class DeviceR1CS:
    """sc_r1cs_*: the instance's images on the device"""

    def __init__(self, ctx, r1cs):
        self.ctx, self.r1cs, self.s, self.m = ctx, r1cs, r1cs.s, r1cs.m
        arrays = []
        for M in r1cs.matrices:
            arrays.append((np.ascontiguousarray(np.array([t[0] for t in M], dtype=np.uint32)),
                           np.ascontiguousarray(np.array([t[1] for t in M], dtype=np.uint32)),
                           np.ascontiguousarray(np.array([t[2] for t in M], dtype=np.uint64))))
        self.h = voidp()
        ctx.check(self.create(ctx, r1cs.s, r1cs.m, arrays, self.h))

    @classmethod
    def from_arrays(cls, ctx, s, m, arrays):
        """the handle over three (row uint32, col uint32, val uint64) numpy triples, with no host instance behind it (.r1cs is
        None): instances too large for lists of triples"""
        self = cls.__new__(cls)
        self.ctx, self.r1cs, self.s, self.m = ctx, None, s, m
        self.h = voidp()
        ctx.check(cls.create(ctx, s, m, [tuple(np.ascontiguousarray(a) for a in t) for t in arrays], self.h))
        return self

    @staticmethod
    def create(ctx, s, m, arrays, handle):
        """sc_r1cs_create over three (row, col, val) numpy triples; returns the status"""
        u32p = ctypes.POINTER(ctypes.c_uint32)
        rows = (u32p * 3)(*[a[0].ctypes.data_as(u32p) for a in arrays])
        cols = (u32p * 3)(*[a[1].ctypes.data_as(u32p) for a in arrays])
        vals = (u64p * 3)(*[a[2].ctypes.data_as(u64p) for a in arrays])
        nnz = (ctypes.c_size_t * 3)(*[a[0].size for a in arrays])
        return ctx.lib.sc_r1cs_create(ctx.h, s, m, rows, cols, vals, nnz, ctypes.byref(handle))

    def mul(self, z):
        """(A z, B z, C z) as device tables; z a device table of 2^m words"""
        out = [voidp(), voidp(), voidp()]
        self.ctx.check(self.ctx.lib.sc_r1cs_mul(self.ctx.h, self.h, z.h, *[ctypes.byref(h) for h in out]))
        return tuple(DenseMultilinearExtension(self.ctx, h) for h in out)

    def bind_rows(self, rx, rho):
        """T[y] = sum_k rho_k sum_i eq(r_x, i) M_k[i][y] as a device table of 2^m words"""
        r, w = _words(rx), _words(rho)
        if r.size != self.s or w.size != 3:
            raise ValueError("r_x has s = %d words and rho three" % self.s)
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_r1cs_bind_rows(self.ctx.h, self.h, _u64p(r), _u64p(w), ctypes.byref(h)))
        return DenseMultilinearExtension(self.ctx, h)

    def row_weights(self, rx, rho):
        """sc_r1cs_row_weights: (rho_A eq(r_x, .), rho_B eq(r_x, .), rho_C eq(r_x, .), 0) as a device table of 2^(s+2) words - the
        row weights of the combined matrix of commit_instance"""
        r, w = _words(rx), _words(rho)
        if r.size != self.s or w.size != 3:
            raise ValueError("r_x has s = %d words and rho three" % self.s)
        h = voidp()
        self.ctx.check(self.ctx.lib.sc_r1cs_row_weights(self.ctx.h, self.h, _u64p(r), _u64p(w), ctypes.byref(h)))
        return DenseMultilinearExtension(self.ctx, h)

    def commit_instance(self, **commit_kwargs):
        """the spark.SparseCommitment of the one combined matrix of 2^(s+2) x 2^m: row k 2^s + i holds entry (i, j) of matrix k (the
        layout of bind_rows' transposed image).  commit_kwargs go to spark.default_commit (log_blowup, code)"""
        from . import spark
        if self.r1cs is None:
            raise ValueError("commit_instance needs the host instance")
        rows, cols, vals = [], [], []
        for k, M in enumerate(self.r1cs.matrices):
            rows += [(k << self.s) + i for i, _, _ in M]
            cols += [j for _, j, _ in M]
            vals += [v for _, _, v in M]
        return spark.SparseCommitment(self.ctx, self.s + 2, self.m, rows, cols, vals, commit=spark.default_commit(**commit_kwargs))

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_r1cs_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _guarded(ctx, draw, width):
    """a C callback over draw(round, evals): an exception must not cross the C frames - the call ends (an unreduced word) and the
    exception is raised again by the caller"""
    failure = []

    def cb(_user, j, e):
        try:
            return int(draw(int(j), [int(e[k]) for k in range(width)]))
        except BaseException as exc:
            failure.append(exc)
            return ctx.field.p
    return cb, failure


def zerocheck_prove(ctx, a, b, c, tau, draw=None, seed_r=0):
    """sc_zerocheck_prove: the cubic sumcheck over sum_x eq(tau, x) (a(x) b(x) - c(x)).  draw(round, [H(0), H(1), H(2), H(3)])
    returns the round's challenge; None: the synthetic challenger of sc_prove over seed_r.
    Returns (c1, rounds[s][4], challenges[s], (v_a, v_b, v_c))"""
    s = a.num_vars()
    t = _words(tau)
    if t.size != s:
        raise ValueError("tau has %d words, the tables %d variables" % (t.size, s))
    evals, ch, fin, c1 = np.zeros(4 * max(s, 1), dtype=np.uint64), np.zeros(max(s, 1), dtype=np.uint64), np.zeros(3, dtype=np.uint64), u64()
    cb, failure = _guarded(ctx, draw, 4) if draw is not None else (None, [])
    rc = ctx.lib.sc_zerocheck_prove(ctx.h, a.h, b.h, c.h, _u64p(t) if s else None, DRAW4_FN(cb) if cb else ctypes.cast(None, DRAW4_FN), None,
                                    int(seed_r), ctypes.byref(c1), _u64p(evals), _u64p(ch), _u64p(fin))
    if failure:
        raise failure[0]
    ctx.check(rc)
    return (int(c1.value), [[int(x) for x in evals[4 * j:4 * j + 4]] for j in range(s)], [int(x) for x in ch[:s]],
            tuple(int(x) for x in fin))


def _product_prove(ctx, a, b, draw):
    """sc_prove(a, b) under draw(round, [H(0), H(1), H(2)]); returns (c1, rounds[n][3], challenges[n])"""
    n = a.num_vars()
    evals, ch, c1 = np.zeros(3 * max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), u64()
    cb, failure = _guarded(ctx, draw, 3)
    rc = ctx.lib.sc_prove(ctx.h, a.h, b.h, DRAW_FN(cb), None, 0, ctypes.byref(c1), _u64p(evals), _u64p(ch))
    if failure:
        raise failure[0]
    ctx.check(rc)
    return int(c1.value), [[int(x) for x in evals[3 * j:3 * j + 3]] for j in range(n)], [int(x) for x in ch[:n]]


class Prover:
    """The prover of the argument over a DeviceR1CS.  Steps, in the protocol's order: root, sumcheck1, bind, sumcheck2, then the
    opening of w at r_y[:m-1] through .pcs (a ligero_pcs.Prover).  commit_kwargs go to ligero_pcs.Prover.commit - or, with
    long_rows=True, to commit_long"""

    def __init__(self, ctx, device_r1cs, io, w, long_rows=False, **commit_kwargs):
        self.ctx, self.field, self.dev = ctx, ctx.field, device_r1cs
        self.s, self.m = device_r1cs.s, device_r1cs.m
        z = device_r1cs.r1cs.assignment(io, w)
        self.z = DenseMultilinearExtension.from_evaluations_vec(ctx, self.m, np.array(z, dtype=np.uint64))
        self.w = DenseMultilinearExtension.from_evaluations_vec(ctx, self.m - 1, np.array([int(x) for x in w], dtype=np.uint64))
        commit = ligero_pcs.Prover.commit_long if long_rows else ligero_pcs.Prover.commit
        self.pcs = commit(ctx, self.w, **commit_kwargs)            # step 1
        self.rx = self.ry = self.T = None

    def root(self):
        return self.pcs.root()

    def sumcheck1(self, tau, draw):
        """step 3: draw(round, four values) -> r_j.  Returns (v_A, v_B, v_C)"""
        az, bz, cz = self.dev.mul(self.z)
        _, _, self.rx, finals = zerocheck_prove(self.ctx, az, bz, cz, tau, draw)
        return finals

    def bind(self, rho):
        """step 5"""
        self.T = self.dev.bind_rows(self.rx, rho)

    def sumcheck2(self, draw):
        """step 6: draw(round, three values) -> r_j"""
        _, _, self.ry = _product_prove(self.ctx, self.T, self.z, draw)

    def close(self):
        self.pcs.close()


class Verifier:
    """The verifier of the argument: pure host code over the instance, the public inputs, the root and the verifier of the
    commitment's opening (a ligero_pcs.Verifier or FoldVerifier over m - 1 variables, built by the caller with that root).
    draw_tau, round1 (s times), receive_finals, draw_rho, round2 (m times), point, finish - in that order."""

    def __init__(self, r1cs, io, root, pcs_verifier):
        F = self.field = r1cs.field
        if bytes(root) != pcs_verifier.root or pcs_verifier.num_vars != r1cs.m - 1:
            raise ValueError("the opening's verifier must be over the committed root and m - 1 = %d variables" % (r1cs.m - 1))
        if F.p <= 3:
            raise ValueError("p = %d: the cubic through 0, 1, 2, 3 needs 2 and 3 invertible" % F.p)
        self.r1cs, self.io, self.root, self.pcs = r1cs, [int(x) for x in io], bytes(root), pcs_verifier
        self.s, self.m = r1cs.s, r1cs.m
        self.inv2, self.inv6 = F.inv(F.from_int(2)), F.inv(F.from_int(6))
        self.tau = self.claim = self.rho = None
        self.rx, self.ry = [], []
        self.phase = 0

    def draw_tau(self, rng):
        self.tau = [_draw(self.field, rng) for _ in range(self.s)]
        self.claim, self.phase = 0, 1
        return list(self.tau)

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

    def _quadratic_at(self, e, x):
        F = self.field
        d = [x, F.sub(x, F.one), F.sub(x, F.from_int(2))]
        l0 = F.mul(F.mul(d[1], d[2]), self.inv2)
        l1 = F.neg(F.mul(d[0], d[2]))
        l2 = F.mul(F.mul(d[0], d[1]), self.inv2)
        return F.add(F.add(F.mul(int(e[0]), l0), F.mul(int(e[1]), l1)), F.mul(int(e[2]), l2))

    def round1(self, j, evals, rng):
        F = self.field
        if self.phase != 1 or j != len(self.rx) or j >= self.s or len(evals) != 4:
            raise Error("sumcheck 1: round %d out of order" % j)
        total = F.add(int(evals[0]), int(evals[1]))
        if total != self.claim:
            raise RoundMismatch(1, j, self.claim, total)
        r = _draw(F, rng)
        self.claim = self._cubic_at(evals, r)
        self.rx.append(r)
        return r

    def receive_finals(self, v_a, v_b, v_c):
        F = self.field
        if self.phase != 1 or len(self.rx) != self.s:
            raise Error("receive_finals before the last round of sumcheck 1")
        eq = F.one
        for t, r in zip(self.tau, self.rx):
            tr = F.mul(t, r)
            eq = F.mul(eq, F.add(F.sub(F.sub(F.one, t), r), F.add(tr, tr)))
        value = F.mul(eq, F.sub(F.mul(int(v_a), int(v_b)), int(v_c)))
        if value != self.claim:
            raise FinalMismatch(1, self.claim, value)
        self.finals = (int(v_a), int(v_b), int(v_c))
        self.phase = 2

    def draw_rho(self, rng):
        F = self.field
        if self.phase != 2 or self.rho is not None:
            raise Error("draw_rho before receive_finals: rho must be drawn after the prover has sent v_A, v_B, v_C")
        self.rho = [_draw(F, rng) for _ in range(3)]
        self.claim = 0
        for rk, vk in zip(self.rho, self.finals):
            self.claim = F.add(self.claim, F.mul(rk, vk))
        return list(self.rho)

    def round2(self, j, evals, rng):
        F = self.field
        if self.rho is None or j != len(self.ry) or j >= self.m or len(evals) != 3:
            raise Error("sumcheck 2: round %d out of order" % j)
        total = F.add(int(evals[0]), int(evals[1]))
        if total != self.claim:
            raise RoundMismatch(2, j, self.claim, total)
        r = _draw(F, rng)
        self.claim = self._quadratic_at(evals, r)
        self.ry.append(r)
        return r

    def point(self):
        """where the commitment is opened: r_y[:m-1]"""
        if len(self.ry) != self.m:
            raise Error("point before the last round of sumcheck 2")
        return list(self.ry[:self.m - 1])

    def finish(self, w_value):
        """steps 7, 8 and 10 with w~(r_y[:m-1]) = w_value, the value the opening's verifier returned"""
        F = self.field
        pt = self.point()
        ey = eq_weights(F, pt)
        x_value = ey[0]                                               # the constant 1 at index 0
        for k, v in enumerate(self.io):
            x_value = F.add(x_value, F.mul(v, ey[k + 1]))
        top = self.ry[self.m - 1]
        z_value = F.add(F.mul(F.sub(F.one, top), x_value), F.mul(top, int(w_value)))
        value = F.mul(self.r1cs.bind_eval(self.rx, self.ry, self.rho), z_value)
        if value != self.claim:
            raise FinalMismatch(2, self.claim, value)
        return True


def open_committed(pcs_prover, pcs_verifier, point, rng):
    """step 9: one opening of the commitment at `point` - folded when the verifier is a FoldVerifier, else the plain one;
    returns the value the opening's verifier accepts"""
    if isinstance(pcs_verifier, ligero_pcs.FoldVerifier):
        return ligero_pcs.open_folded(pcs_prover, pcs_verifier, point, rng)
    gamma = pcs_verifier.draw_gamma(rng)
    pcs_verifier.receive(*pcs_prover.combine(point, gamma))
    return pcs_verifier.verify(point, pcs_prover.open_columns(pcs_verifier.draw_columns(rng)))


def prove_and_verify(prover, verifier, rng):
    """the whole exchange between a Prover (anything with its steps) and a Verifier; True, or the verifier's error"""
    tau = verifier.draw_tau(rng)
    finals = prover.sumcheck1(tau, lambda j, e: verifier.round1(j, e, rng))
    verifier.receive_finals(*finals)
    prover.bind(verifier.draw_rho(rng))
    prover.sumcheck2(lambda j, e: verifier.round2(j, e, rng))
    w_value = open_committed(prover.pcs, verifier.pcs, verifier.point(), rng)
    return verifier.finish(w_value)


# ---- the verifier that does not read the instance (spark.py) --------------------------------

class SublinearVerifier(Verifier):
    """Verifier's steps without the matrices: it holds s, m, the public inputs, the witness root with the verifier of its opening,
    and instance_verifiers, the verifiers of the openings of the five tables of DeviceR1CS.commit_instance (built over its five
    roots, keyed by spark.TABLES).  Step 7, T~(r_y), comes from the SPARK exchange over the combined matrix with
    U = row_weights(r_x, rho) and W = eq(r_y, .), whose extensions are u_eval and w_eval below."""

    def __init__(self, field, s, m, io, root, pcs_verifier, instance_verifiers):
        F = self.field = field
        if not 1 <= s <= MAX_LOG or not 2 <= m <= MAX_LOG:
            raise ValueError("s must be in 1..%d and m in 2..%d" % (MAX_LOG, MAX_LOG))
        if bytes(root) != pcs_verifier.root or pcs_verifier.num_vars != m - 1:
            raise ValueError("the opening's verifier must be over the committed root and m - 1 = %d variables" % (m - 1))
        if F.p <= 3:
            raise ValueError("p = %d: the cubic through 0, 1, 2, 3 needs 2 and 3 invertible" % F.p)
        self.r1cs, self.io, self.root, self.pcs = None, [int(x) for x in io], bytes(root), pcs_verifier
        self.instance_pcs = dict(instance_verifiers)
        self.s, self.m = s, m
        self.inv2, self.inv6 = F.inv(F.from_int(2)), F.inv(F.from_int(6))
        self.tau = self.claim = self.rho = None
        self.rx, self.ry = [], []
        self.phase = 0

    def _eq_at(self, a, b):
        F = self.field
        out = F.one
        for x, y in zip(a, b):
            xy = F.mul(int(x), int(y))
            out = F.mul(out, F.add(F.sub(F.sub(F.one, int(x)), int(y)), F.add(xy, xy)))
        return out

    def u_eval(self, z):
        """U~(z) for U = (rho_A eq(r_x, .), rho_B eq(r_x, .), rho_C eq(r_x, .), 0): eq(r_x, z[:s]) (rho_A (1 - z_s)(1 - z_(s+1)) +
        rho_B z_s (1 - z_(s+1)) + rho_C (1 - z_s) z_(s+1))"""
        F = self.field
        lo, hi = int(z[self.s]), int(z[self.s + 1])
        nlo, nhi = F.sub(F.one, lo), F.sub(F.one, hi)
        sel = F.add(F.add(F.mul(self.rho[0], F.mul(nlo, nhi)), F.mul(self.rho[1], F.mul(lo, nhi))), F.mul(self.rho[2], F.mul(nlo, hi)))
        return F.mul(self._eq_at(self.rx, z[:self.s]), sel)

    def w_eval(self, z):
        """W~(z) for W = eq(r_y, .)"""
        return self._eq_at(self.ry, z)

    def finish(self, w_value, t_value):
        """steps 8 and 10 with w~(r_y[:m-1]) = w_value from the opening and T~(r_y) = t_value from the SPARK exchange"""
        F = self.field
        pt = self.point()
        ey = eq_weights(F, pt)
        x_value = ey[0]                                               # the constant 1 at index 0
        for k, v in enumerate(self.io):
            x_value = F.add(x_value, F.mul(v, ey[k + 1]))
        top = self.ry[self.m - 1]
        z_value = F.add(F.mul(F.sub(F.one, top), x_value), F.mul(top, int(w_value)))
        value = F.mul(int(t_value), z_value)
        if value != self.claim:
            raise FinalMismatch(2, self.claim, value)
        return True


def prove_and_verify_sublinear(prover, instance, verifier, rng):
    """the whole exchange between a Prover, the spark.SparseCommitment of its instance (DeviceR1CS.commit_instance) and a
    SublinearVerifier; True, or the verifier's error (spark's errors among them)"""
    from . import spark
    tau = verifier.draw_tau(rng)
    finals = prover.sumcheck1(tau, lambda j, e: verifier.round1(j, e, rng))
    verifier.receive_finals(*finals)
    rho = verifier.draw_rho(rng)
    prover.bind(rho)
    prover.sumcheck2(lambda j, e: verifier.round2(j, e, rng))
    U, W = prover.dev.row_weights(prover.rx, rho), spark.table_eq(prover.ctx, prover.ry)
    t_value = spark.prove_eval(instance, verifier.instance_pcs, U, W, verifier.u_eval, verifier.w_eval, rng)
    w_value = open_committed(prover.pcs, verifier.pcs, verifier.point(), rng)
    return verifier.finish(w_value, t_value)


def prove_and_verify_sublinear_batched(prover, instance, verifier, rng, groups=None):
    """prove_and_verify_sublinear with batched openings (multiopen.py): P sends w~(r_y[:m-1]) next to
    the nine values of the SPARK exchange, and the witness claim joins that exchange's list of claims (spark.prove_eval_batched) -
    one joint opening per commitment shape, the witness's commitment among them where its shape agrees.  The accepted value is
    M~(r_x, r_y) exactly as in prove_and_verify_sublinear.  A FoldVerifier is refused with a ValueError: a joint folded opening is
    out of scope.  groups: a list that receives multiopen.prove_claims' groups.  True, or the verifier's error"""
    from . import multiopen, spark
    if isinstance(verifier.pcs, ligero_pcs.FoldVerifier) or any(isinstance(v, ligero_pcs.FoldVerifier) for v in verifier.instance_pcs.values()):
        raise ValueError("batched openings take the plain ligero_pcs.Verifier: a joint folded opening is out of scope")
    tau = verifier.draw_tau(rng)
    finals = prover.sumcheck1(tau, lambda j, e: verifier.round1(j, e, rng))
    verifier.receive_finals(*finals)
    rho = verifier.draw_rho(rng)
    prover.bind(rho)
    prover.sumcheck2(lambda j, e: verifier.round2(j, e, rng))
    U, W = prover.dev.row_weights(prover.rx, rho), spark.table_eq(prover.ctx, prover.ry)
    point = verifier.point()
    w_value = prover.pcs.poly.evaluate(point)
    extra = ({"w": prover.pcs}, {"w": verifier.pcs}, [multiopen.Claim("w", point, w_value)])
    t_value = spark.prove_eval_batched(instance, verifier.instance_pcs, U, W, verifier.u_eval, verifier.w_eval, rng, extra=extra, groups=groups)
    return verifier.finish(w_value, t_value)
