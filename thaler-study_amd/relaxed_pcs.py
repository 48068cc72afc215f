"""relaxed-pcs/src/lib.rs on the GPU: the Relaxed polynomial commitment.

The prover evaluates W~ at every point of F^m (sc_table_extend_grid) and commits to those values with a Merkle tree
(sc_merkle_commit); the verifier picks a random line, receives the univariate restriction of W~ to it (restrict_poly) and checks
it at one random point of the line against a Merkle opening.  The verifier is host code (hashlib) and never touches the GPU.

Contract (kernels/pcs.hpp for the leaf order, kernels/sha256.hpp for the hashing):
  leaf order   all_multidimentional_values(m) (:46-63): the p^m points sorted by canonical value, v_0 the most significant
               digit; point (v_0, .., v_{m-1}) is leaf o = sum_j v_j p^(m-1-j); its value is the LE MLE at it (point[0] binds
               index bit 0 of the table); values are zero-padded to a power of two
  hashing      leaf digest SHA-256(le64(canonical value)); node digest SHA-256(left || right).  The reference's own test hashes
               with Pedersen over JubJub; this project uses SHA-256 (a deliberate deviation).  Meant to equal arkworks'
               MerkleTree with Sha256 as both hashes and IdentityDigestConverter, which is not pinned here
  limits       p > m (restrict_poly) and p^m <= 2^28

Field elements are Montgomery words, as everywhere in this package; Merkle leaves are canonical integers."""
import ctypes
import hashlib
import itertools

import numpy as np

from ._lib import size_t, voidp
from .dense_mle import DenseMultilinearExtension, _u64p
from .gkr_protocol import restrict_poly


class Error(Exception):
    """relaxed_pcs::Error (:20-41)"""


class EvalMismatch(Error):
    def __init__(self, leaf, evaluation):
        super().__init__("Evaluation does not match leaf %s %s" % (leaf, evaluation))
        self.leaf, self.evaluation = leaf, evaluation


class NoProverPoly(Error):
    def __init__(self):
        super().__init__("Prover not commited a polynomial")


class PolyEvalDimMismatch(Error):
    def __init__(self):
        super().__init__("Poly evaluation dimention mismatch")


class DegreeMismatch(Error):
    def __init__(self, degree, expected):
        super().__init__("Prover claim degree mismatch: %d, expected %d" % (degree, expected))
        self.degree, self.expected = degree, expected


class MerkleMismatch(Error):
    """the opening does not lead to the committed root, or opens another leaf than the challenge point's"""


# ---- grid order ------------------------------------------------------------------------------------------------------

def all_multidimentional_values(field, m):
    """IF::all_multidimentional_values (:55-61): every point of F^m as a list of Montgomery words, sorted by canonical value
    with v_0 the most significant digit (itertools.product over 0..p-1 is that order)"""
    values = [field.from_int(x) for x in range(field.p)]
    return [list(t) for t in itertools.product(values, repeat=m)]


def leaf_index(field, point):
    """the position of `point` (Montgomery words) in all_multidimentional_values: sum_j v_j p^(m-1-j)"""
    o = 0
    for v in point:
        o = o * field.p + field.to_int(v)
    return o


def extend_grid(ctx, poly):
    """sc_table_extend_grid: W~ at every point of F^m in leaf order, zero-padded to a power of two (a device table)"""
    h = voidp()
    ctx.check(ctx.lib.sc_table_extend_grid(ctx.h, poly.h, poly.num_vars(), ctypes.byref(h)))
    return DenseMultilinearExtension(ctx, h)


# ---- hashing (host) --------------------------------------------------------------------------------------------------

def leaf_digest(canonical):
    return hashlib.sha256(int(canonical).to_bytes(8, "little")).digest()


def node_digest(left, right):
    return hashlib.sha256(bytes(left) + bytes(right)).digest()


class Path:
    """merkle_tree::Path: the opened leaf's index and its sibling digests, bottom up"""

    def __init__(self, index, siblings, field=None):
        self.index, self.siblings, self.field = int(index), [bytes(s) for s in siblings], field

    def root_from_digest(self, h):
        """the sibling walk from the leaf's digest `h` up to the root it leads to"""
        for level, s in enumerate(self.siblings):
            h = node_digest(h, s) if (self.index >> level) & 1 == 0 else node_digest(s, h)
        return h

    def root_from(self, canonical):
        return self.root_from_digest(leaf_digest(canonical))

    def verify_canonical(self, root, canonical):
        return self.index < (1 << len(self.siblings)) and self.root_from(canonical) == bytes(root)

    def verify(self, root, leaf):
        """Path::verify with the leaf as a field element (Montgomery word): True if the path leads to `root`"""
        return self.verify_canonical(root, self.field.to_int(leaf))


# ---- the commitment of any table -------------------------------------------------------------------------------------

class MerkleTree:
    """sc_merkle_*: the SHA-256 Merkle tree over the 2^n entries of a device table (borrowed: kept alive by the tree)"""

    def __init__(self, ctx, table):
        self.ctx, self.table = ctx, table
        h = voidp()
        ctx.check(ctx.lib.sc_merkle_commit(ctx.h, table.h, ctypes.byref(h)))
        self.h = h
        d = ctypes.c_size_t()
        ctx.check(ctx.lib.sc_merkle_depth(self.h, ctypes.byref(d)))
        self.depth = d.value

    def root(self):
        buf = (ctypes.c_uint8 * 32)()
        self.ctx.check(self.ctx.lib.sc_merkle_root(self.h, buf))
        return bytes(buf)

    def open(self, indices):
        """[(Path, canonical leaf)] for every index, in one call"""
        idx = np.ascontiguousarray(np.array([int(i) for i in indices], dtype=np.uint64))
        count = idx.size
        leaves = np.zeros(max(count, 1), dtype=np.uint64)
        paths = (ctypes.c_uint8 * max(1, count * self.depth * 32))()
        self.ctx.check(self.ctx.lib.sc_merkle_open(self.ctx.h, self.h, _u64p(idx) if count else None, count, _u64p(leaves), paths))
        raw = bytes(paths)
        out = []
        for q in range(count):
            sib = [raw[(q * self.depth + l) * 32:(q * self.depth + l + 1) * 32] for l in range(self.depth)]
            out.append((Path(int(idx[q]), sib, self.ctx.field), int(leaves[q])))
        return out

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.sc_merkle_tree_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merkle_commit(ctx, table):
    return MerkleTree(ctx, table)


# ---- the protocol ----------------------------------------------------------------------------------------------------

def _draw(field, rng):
    """F::rand(rng): a sum_check_protocol.RngF (rng.draw()) or a random.Random"""
    return rng.draw() if hasattr(rng, "draw") else field.rand(rng)


class Prover:
    """Prover (:152-214).  new() extends the grid and commits on the device; the grid table and the tree stay there."""

    def __init__(self, ctx, poly, grid, tree):
        self.ctx, self.field, self.poly, self.grid, self.tree = ctx, ctx.field, poly, grid, tree
        self.num_vars = poly.num_vars()

    @classmethod
    def new(cls, ctx, poly):
        grid = extend_grid(ctx, poly)
        return cls(ctx, poly, grid, MerkleTree(ctx, grid))

    def merkle_root(self):
        return self.tree.root()

    def poly_restriction_to_line(self, b, c):
        """restrict_poly(b, c, poly) (:201-204) on the device: a SparsePolynomial"""
        return restrict_poly(b, c, self.poly)

    def challenge(self, point):
        """(Path, value) of the leaf at `point` (:206-213); value is a Montgomery word"""
        if len(point) != self.num_vars:
            raise PolyEvalDimMismatch()
        [(path, canonical)] = self.tree.open([leaf_index(self.field, point)])
        return path, self.field.from_int(canonical)


class Verifier:
    """Verifier (:65-149).  Pure host code.

    Degree quirk: the reference's commited_univariate (:108-114) rejects unless the restriction's degree equals
    degree * num_vars EXACTLY, while an honest restriction has a lower degree whenever its top coefficient vanishes (for p = 11,
    m = 8 that is more than half of random instances).  strict_degree=True (the default) mirrors that and raises
    DegreeMismatch; strict_degree=False accepts any degree up to the bound.

    verify_prover_reply raises MerkleMismatch when the path does not lead to the root, where the reference drops
    Path::verify's boolean (`path.verify(..)?`, :129-134), and when the path opens another leaf than the challenge point's."""

    def __init__(self, field, num_vars, degree, merkle_root, strict_degree=True):
        self.field, self.num_vars = field, num_vars
        self.degree = degree * num_vars
        self.merkle_root, self.strict_degree = bytes(merkle_root), strict_degree
        self.x = 0
        self.challenge_point = []
        self.line = None
        self.prover_univariate = None

    def random_line(self, rng):
        b = [_draw(self.field, rng) for _ in range(self.num_vars)]
        c = [_draw(self.field, rng) for _ in range(self.num_vars)]
        self.line = (b, c)
        return b, c

    def commited_univariate(self, p):
        d = p.degree()
        if d != self.degree if self.strict_degree else d > self.degree:
            raise DegreeMismatch(d, self.degree)
        self.prover_univariate = p

    def challenge_prover(self, rng):
        """x at random; the point l(x) = b + x (c - b) of the line (gkr-protocol `line`)"""
        F = self.field
        self.x = _draw(F, rng)
        b, c = self.line
        self.challenge_point = [F.add(bi, F.mul(self.x, F.sub(ci, bi))) for bi, ci in zip(b, c)]
        return list(self.challenge_point)

    def verify_prover_reply(self, path, leaf):
        if not path.verify_canonical(self.merkle_root, self.field.to_int(leaf)):
            raise MerkleMismatch("the opening does not lead to the committed root")
        if path.index != leaf_index(self.field, self.challenge_point):
            raise MerkleMismatch("the opening is of leaf %d, the challenge point is leaf %d"
                                 % (path.index, leaf_index(self.field, self.challenge_point)))
        if self.prover_univariate is None:
            raise NoProverPoly()
        ev = self.prover_univariate.evaluate(self.x)
        if int(leaf) != ev:
            raise EvalMismatch(int(leaf), ev)
