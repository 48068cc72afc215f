"""A pure-Python restatement of the sum-of-products sumcheck with challenges from K = F_p[X] / (X^2 - w)
(thaler-study_amd/csrc/kernels/ext_sumprod.hpp), test-local: nothing here imports the package.  Everything is in CANONICAL integers;
an element of K is a pair (c0, c1).  Products are plain schoolbook products - four base multiplications - so nothing here shares the
kernels' Karatsuba formula.

  nonresidue, kmul, kadd, ksub, kinv     K itself
  round_message, fold, quadratic_at      one round over the pairs (a_t, b_t)
  sumcheck                               the whole prover: (c1, rounds, challenges, finals_a, finals_b)
  eq_weights, mle_eval                   eq(z, .) in K and a base table's extension at z in K^n
  synthetic_draw                         the engine's synthetic challenger over seed_r"""

M64 = 2**64 - 1


def nonresidue(p):
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return g


def kadd(a, b, p):
    return ((a[0] + b[0]) % p, (a[1] + b[1]) % p)


def ksub(a, b, p):
    return ((a[0] - b[0]) % p, (a[1] - b[1]) % p)


def kmul(a, b, p, w):
    return ((a[0] * b[0] + w * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def kinv(a, p, w):
    n = pow((a[0] * a[0] - w * a[1] * a[1]) % p, -1, p)
    return (a[0] * n % p, -a[1] * n % p)


def lift(table):
    return [(int(x), 0) for x in table]


def round_message(As, Bs, p, w):
    """H(0), H(1), H(2) in K over the pairs of tables of K elements"""
    msg = [(0, 0)] * 3
    for a, b in zip(As, Bs):
        for i in range(len(a) // 2):
            a0, a1, b0, b1 = a[2 * i], a[2 * i + 1], b[2 * i], b[2 * i + 1]
            a2, b2 = ksub(kadd(a1, a1, p), a0, p), ksub(kadd(b1, b1, p), b0, p)
            msg = [kadd(msg[0], kmul(a0, b0, p, w), p), kadd(msg[1], kmul(a1, b1, p, w), p), kadd(msg[2], kmul(a2, b2, p, w), p)]
    return msg


def fold(u, r, p, w):
    return [kadd(u[2 * i], kmul(r, ksub(u[2 * i + 1], u[2 * i], p), p, w), p) for i in range(len(u) // 2)]


def quadratic_at(msg, x, p, w):
    """the quadratic through (0, msg[0]), (1, msg[1]), (2, msg[2]) at x in K"""
    inv2 = pow(2, -1, p)
    xm1, xm2 = ksub(x, (1, 0), p), ksub(x, (2, 0), p)
    l0 = kmul(kmul(xm1, xm2, p, w), (inv2, 0), p, w)
    l1 = ksub((0, 0), kmul(x, xm2, p, w), p)
    l2 = kmul(kmul(x, xm1, p, w), (inv2, 0), p, w)
    out = (0, 0)
    for m, l in zip(msg, (l0, l1, l2)):
        out = kadd(out, kmul(m, l, p, w), p)
    return out


def sumcheck(a_tables, b_tables, p, w, draw):
    """a_tables, b_tables: T base tables each (canonical integers); draw(j, msg) -> r_j in K.
    Returns (c1, rounds, challenges, finals_a, finals_b), every element a pair"""
    As, Bs = [lift(t) for t in a_tables], [lift(t) for t in b_tables]
    rounds, rs, c1, j = [], [], None, 0
    while len(As[0]) > 1:
        msg = round_message(As, Bs, p, w)
        if j == 0:
            c1 = kadd(msg[0], msg[1], p)
        r = draw(j, msg)
        r = (int(r[0]) % p, int(r[1]) % p)
        rounds.append(msg)
        rs.append(r)
        As, Bs = [fold(a, r, p, w) for a in As], [fold(b, r, p, w) for b in Bs]
        j += 1
    return c1, rounds, rs, [a[0] for a in As], [b[0] for b in Bs]


def eq_weights(point, p, w):
    out = [(1, 0)]
    for r in point:
        nr = ksub((1, 0), r, p)
        out = [kmul(x, nr, p, w) for x in out] + [kmul(x, r, p, w) for x in out]
    return out


def mle_eval(table, point, p, w):
    """the multilinear extension of a base table at a point of K^n, LE, from the eq weights"""
    c0 = c1 = 0
    for x, e in zip(table, eq_weights(point, p, w)):
        c0 += int(x) * e[0]
        c1 += int(x) * e[1]
    return (c0 % p, c1 % p)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def synthetic_draw(p, seed_r):
    """r_j = (splitmix64(seed_r + 2 j + 1) mod p, splitmix64(seed_r + 2 j + 2) mod p), canonical"""
    return lambda j, msg: (splitmix64((seed_r + 2 * j + 1) & M64) % p, splitmix64((seed_r + 2 * j + 2) & M64) % p)
