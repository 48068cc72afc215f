"""A pure-Python restatement of the R1CS argument's contract (thaler-study_amd/csrc/kernels/r1cs.hpp), test-local: nothing here
imports the package.  Everything is in CANONICAL integers; the tests convert to and from Montgomery words at the boundary
(ligero_ref.mont / canon).

  dense(M, s, m), dense_mul, sparse_mul     the products, from the dense definition and over the triples
  eq_table(point, p), fold(t, r, p)         eq(point, i) for every i, LE; one fold of a table, variable 0
  cubic_round(E, A, B, C, p)                H(0..3) of one round, straight from the definition
  zerocheck(a, b, c, tau, challenges, p)    all rounds under fixed challenges: (c1, rounds, finals)
  product_round(a, b, p)                    H(0..2) of the product sumcheck
  bind_rows(mats, s, m, rx, rho, p)         T[y] = sum_k rho_k sum_i eq(r_x, i) M_k[i][y], from the dense definition
  bind_eval_dense(..)                       T~(r_y) from the dense definition
  RefProver                                 the prover of the protocol over all of the above, with a commitment from ligero_ref"""
import ligero_ref


def dense(M, s, m, p):
    """the 2^s x 2^m matrix of a list of (row, col, val) triples; equal (row, col) add"""
    D = [[0] * (1 << m) for _ in range(1 << s)]
    for i, j, v in M:
        D[i][j] = (D[i][j] + v) % p
    return D


def dense_mul(D, z, p):
    return [sum(a * b for a, b in zip(row, z)) % p for row in D]


def sparse_mul(M, s, z, p):
    y = [0] * (1 << s)
    for i, j, v in M:
        y[i] = (y[i] + v * z[j]) % p
    return y


def eq_table(point, p):
    w = [1]
    for r in point:
        w = [x * (1 - r) % p for x in w] + [x * r % p for x in w]
    return w


def fold(t, r, p):
    return [(t[2 * i] + r * (t[2 * i + 1] - t[2 * i])) % p for i in range(len(t) // 2)]


def cubic_round(E, A, B, C, p):
    """H(t) = sum_i e_i(t) (a_i(t) b_i(t) - c_i(t)) at t = 0, 1, 2, 3, with u_i(t) = u[2i] + t (u[2i+1] - u[2i])"""
    out = []
    for t in range(4):
        h = 0
        for i in range(len(E) // 2):
            e, a, b, c = (u[2 * i] + t * (u[2 * i + 1] - u[2 * i]) for u in (E, A, B, C))
            h += e * (a * b - c)
        out.append(h % p)
    return out


def zerocheck(a, b, c, tau, challenges, p):
    """the cubic sumcheck under fixed challenges: (c1, rounds[s][4], (A_s[0], B_s[0], C_s[0]))"""
    E, A, B, C = eq_table(tau, p), list(a), list(b), list(c)
    rounds = []
    for r in challenges:
        rounds.append(cubic_round(E, A, B, C, p))
        E, A, B, C = (fold(u, r, p) for u in (E, A, B, C))
    return (rounds[0][0] + rounds[0][1]) % p, rounds, (A[0], B[0], C[0])


def cubic_at(e, x, p):
    """the cubic through (0, e0) .. (3, e3) at x (Lagrange)"""
    total = 0
    for k in range(4):
        num, den = 1, 1
        for l in range(4):
            if l != k:
                num = num * (x - l) % p
                den = den * (k - l) % p
        total += e[k] * num * pow(den, -1, p)
    return total % p


def quadratic_at(e, x, p):
    total = 0
    for k in range(3):
        num, den = 1, 1
        for l in range(3):
            if l != k:
                num = num * (x - l) % p
                den = den * (k - l) % p
        total += e[k] * num * pow(den, -1, p)
    return total % p


def product_round(a, b, p):
    out = []
    for t in range(3):
        out.append(sum((a[2 * i] + t * (a[2 * i + 1] - a[2 * i])) * (b[2 * i] + t * (b[2 * i + 1] - b[2 * i])) for i in range(len(a) // 2)) % p)
    return out


def bind_rows(mats, s, m, rx, rho, p):
    ex = eq_table(rx, p)
    T = [0] * (1 << m)
    for M, rk in zip(mats, rho):
        D = dense(M, s, m, p)
        for y in range(1 << m):
            T[y] = (T[y] + rk * sum(ex[i] * D[i][y] for i in range(1 << s))) % p
    return T


def bind_rows_sparse(mats, s, m, rx, rho, p):
    """the same T over the triples (the GPU tests' sizes are out of the dense definition's reach)"""
    ex = eq_table(rx, p)
    T = [0] * (1 << m)
    for M, rk in zip(mats, rho):
        for i, j, v in M:
            T[j] = (T[j] + rk * ex[i] * v) % p
    return T


def bind_eval_dense(mats, s, m, rx, ry, rho, p):
    return ligero_ref.mle_eval(bind_rows(mats, s, m, rx, rho, p), ry, p)


def assignment(io, w, m):
    half = 1 << (m - 1)
    return [1] + list(io) + [0] * (half - 1 - len(io)) + list(w)


class RefProver:
    """the prover of the protocol in canonical integers; pcs = a ligero_ref.RefProver (or expander_ref.RefProver) over w"""

    def __init__(self, mats, s, m, io, w, p, pcs):
        self.mats, self.s, self.m, self.p, self.pcs = mats, s, m, p, pcs
        self.z = assignment(io, w, m)
        self.w = list(w)

    def sumcheck1(self, tau, draw):
        """draw(round, four values) -> r_j; returns (v_A, v_B, v_C)"""
        p = self.p
        E = eq_table(tau, p)
        A, B, C = (sparse_mul(M, self.s, self.z, p) for M in self.mats)
        self.rx = []
        for j in range(self.s):
            r = draw(j, cubic_round(E, A, B, C, p))
            E, A, B, C = (fold(u, r, p) for u in (E, A, B, C))
            self.rx.append(r)
        return A[0], B[0], C[0]

    def bind(self, rho):
        self.T = bind_rows(self.mats, self.s, self.m, self.rx, rho, self.p)

    def sumcheck2(self, draw):
        p = self.p
        a, b = list(self.T), list(self.z)
        self.ry = []
        for j in range(self.m):
            r = draw(j, product_round(a, b, p))
            a, b = fold(a, r, p), fold(b, r, p)
            self.ry.append(r)
