"""The quadratic extension K = F_p[X] / (X^2 - w) over pairs of Montgomery words (csrc/kernels/ext_sumprod.hpp states the
conventions): an element is a tuple (c0, c1), meaning c0 + c1 X; w is a quadratic non-residue of F_p, a Montgomery word.

  nonresidue(p)                          the smallest canonical integer >= 2 that is no square mod p
  QuadExt(field, w)                      add, sub, neg, mul, inv, from_base, scale, eq_weights(point)"""


def nonresidue(p):
    """the smallest integer g >= 2 with g^((p-1)/2) = p - 1 (7 for Goldilocks, 2 for 2^64 - 59, 3 for 2^61 - 1, 2^32 + 15 and 257)"""
    if p < 3 or p % 2 == 0:
        raise ValueError("the modulus must be an odd prime")
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
        if g >= p:
            raise ValueError("no non-residue below p = %d: not a prime" % p)
    return g


class QuadExt:
    """K over `field` (a field.Field); w: a Montgomery word, default the smallest non-residue.  A residue is refused."""

    def __init__(self, field, w=None):
        self.field = field
        self.w = field.from_int(nonresidue(field.p)) if w is None else int(w)
        if not 0 <= self.w < field.p or pow(field.to_int(self.w), (field.p - 1) // 2, field.p) != field.p - 1:
            raise ValueError("w must be a Montgomery word of a quadratic non-residue")
        self.zero, self.one, self.x = (0, 0), (field.one, 0), (0, field.one)

    def from_base(self, a):
        return (int(a), 0)

    def add(self, a, b):
        F = self.field
        return (F.add(a[0], b[0]), F.add(a[1], b[1]))

    def sub(self, a, b):
        F = self.field
        return (F.sub(a[0], b[0]), F.sub(a[1], b[1]))

    def neg(self, a):
        F = self.field
        return (F.neg(a[0]), F.neg(a[1]))

    def scale(self, a, s):
        """a times the base word s"""
        F = self.field
        return (F.mul(a[0], s), F.mul(a[1], s))

    def mul(self, a, b):
        """three base products, as the kernels form it"""
        F = self.field
        s00, s11, sm = F.mul(a[0], b[0]), F.mul(a[1], b[1]), F.mul(F.add(a[0], a[1]), F.add(b[0], b[1]))
        return (F.add(s00, F.mul(self.w, s11)), F.sub(F.sub(sm, s00), s11))

    def inv(self, a):
        """(c0 - c1 X) / (c0^2 - w c1^2): the norm is zero only for a = 0"""
        F = self.field
        norm = F.sub(F.mul(a[0], a[0]), F.mul(self.w, F.mul(a[1], a[1])))
        if norm == 0:
            raise ZeroDivisionError("inverse of zero")
        ninv = F.inv(norm)
        return (F.mul(a[0], ninv), F.neg(F.mul(a[1], ninv)))

    def rand(self, rng):
        return (self.field.rand(rng), self.field.rand(rng))

    def eq_weights(self, point):
        """eq(point, i) in K for every i < 2^len(point), LE: bit j of i goes with point[j]"""
        w = [self.one]
        for r in point:
            nr = self.sub(self.one, r)
            w = [self.mul(x, nr) for x in w] + [self.mul(x, r) for x in w]
        return w

    def split(self, values):
        """the c0 words and the c1 words of a list of elements"""
        return [v[0] for v in values], [v[1] for v in values]
