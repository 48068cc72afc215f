"""A pure-Python restatement of the LogUp contract (thaler-study_amd/csrc/kernels/fraction.hpp), test-local: nothing here
imports the package or reads csrc/.  Everything is in CANONICAL integers; the tests convert to and from Montgomery words at the
boundary (mont / canon).

  tree(p_table, q_table, p)       ([p_0, .., p_n], [q_0, .., q_n]): the fraction-sum tree by halves; p_table None = all ones
  eq_table, eq_point, mle_eval    eq and the multilinear extension by their definitions
  fold, layer_round, cubic_at     one fold (variable 0), H(0..3) of one round straight from the definition, the cubic's value
  prove(pt, qt, p, draw)          the layer prover under draw(layer, round, msg) -> challenge: a dict of every message
  verify(n, p, proof, draw, ones) the verifier: (point, a, b), or Reject(kind, layer, round)
  multiplicities(w, t, idx)       (mult, mismatches)
  range_eval(point, p)            the extension of t_j = j by its definition's closed form, sum_j 2^j point_j"""


def mont(x, p):
    return x * (1 << 64) % p


def canon(w, p):
    return w * pow(1 << 64, -1, p) % p


def mont_list(xs, p):
    R = (1 << 64) % p
    return [int(x) * R % p for x in xs]


def canon_list(ws, p):
    rinv = pow(1 << 64, -1, p)
    return [int(w) * rinv % p for w in ws]


def tree(pt, qt, p):
    P, Q = [list(pt) if pt is not None else [1 % p] * len(qt)], [list(qt)]
    while len(Q[0]) > 1:
        tp, tq = P[0], Q[0]
        half = len(tq) // 2
        P.insert(0, [(tp[x] * tq[x + half] + tp[x + half] * tq[x]) % p for x in range(half)])
        Q.insert(0, [tq[x] * tq[x + half] % p for x in range(half)])
    return P, Q


def eq_table(point, p):
    """eq(point, i) for every i, LE: bit j of i goes with point[j]"""
    w = [1]
    for r in point:
        w = [x * (1 - r) % p for x in w] + [x * r % p for x in w]
    return w


def eq_point(a, b, p):
    out = 1
    for x, y in zip(a, b):
        out = out * (x * y + (1 - x) * (1 - y)) % p
    return out


def mle_eval(t, point, p):
    """sum_i t[i] eq(point, i), by the definition"""
    return sum(x * w for x, w in zip(t, eq_table(point, p))) % p


def fold(t, r, p):
    return [(t[2 * i] + r * (t[2 * i + 1] - t[2 * i])) % p for i in range(len(t) // 2)]


def layer_round(E, PL, PR, QL, QR, lam, p):
    """H(t) = sum_i e_i(t) (pl_i(t) qr_i(t) + pr_i(t) ql_i(t) + lam ql_i(t) qr_i(t)) at t = 0, 1, 2, 3, with
    u_i(t) = u[2i] + t (u[2i+1] - u[2i])"""
    out = [0, 0, 0, 0]
    for i in range(len(E) // 2):
        for t in range(4):
            e, pl, pr, ql, qr = (u[2 * i] + t * (u[2 * i + 1] - u[2 * i]) for u in (E, PL, PR, QL, QR))
            out[t] += e * (pl * qr + pr * ql + lam * ql * qr)
    return [h % p for h in out]


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


def n_challenges(n):
    """rho_0, then per layer k >= 1: lambda_k, k rounds, rho_k"""
    return n * (n - 1) // 2 + 2 * n - 1


def prove(pt, qt, p, draw, layers=None):
    """every message of the prover under draw(layer, round, msg): root, rounds[k][j][4], finals[k] = (pl, pr, ql, qr), challenges (as
    drawn: rho_0, then per layer lambda_k, r_0 .., rho_k), lambdas[k], point = z_n, claims = (a_n, b_n).  draw(k, k + 1, []) is the
    lambda of layer k + 1"""
    P, Q = layers or tree(pt, qt, p)
    n = len(Q) - 1
    z, a, b, lam = [], P[0][0], Q[0][0], 0
    rounds, finals, challenges, lambdas = [], [], [], [None]
    for k in range(n):
        half = 1 << k
        E = eq_table(z, p)
        PL, PR, QL, QR = P[k + 1][:half], P[k + 1][half:], Q[k + 1][:half], Q[k + 1][half:]
        rs, msgs = [], []
        for j in range(k):
            msg = layer_round(E, PL, PR, QL, QR, lam, p)
            r = draw(k, j, msg)
            E, PL, PR, QL, QR = (fold(u, r, p) for u in (E, PL, PR, QL, QR))
            rs.append(r)
            msgs.append(msg)
        fin = (PL[0], PR[0], QL[0], QR[0])
        rho = draw(k, k, list(fin))
        a, b = (fin[0] + rho * (fin[1] - fin[0])) % p, (fin[2] + rho * (fin[3] - fin[2])) % p
        z = rs + [rho]
        rounds.append(msgs)
        finals.append(fin)
        challenges += rs + [rho]
        if k + 1 < n:
            lam = draw(k, k + 1, [])
            lambdas.append(lam)
            challenges.append(lam)
    return {"root": (P[0][0], Q[0][0]), "rounds": rounds, "finals": finals, "challenges": challenges, "lambdas": lambdas, "point": z,
            "claims": (a, b)}


class Reject(Exception):
    def __init__(self, kind, layer=None, round_index=None):
        super().__init__("%s at layer %s round %s" % (kind, layer, round_index))
        self.kind, self.layer, self.round = kind, layer, round_index


def verify(n, p, proof, draw, ones=False):
    """the verifier over a prove() dict under draw(layer, round, msg); returns (point, a, b).  Reject kinds: "root" (layer 0's
    finals), "round", "final", "numerator" (ones: a_n != 1)"""
    z, (a, b), lam = [], (proof["root"][0] % p, proof["root"][1] % p), 0
    for k in range(n):
        claim = (a + lam * b) % p
        rs = []
        for j in range(k):
            msg = proof["rounds"][k][j]
            if (msg[0] + msg[1]) % p != claim:
                raise Reject("round", k, j)
            r = draw(k, j, msg)
            claim = cubic_at(msg, r, p)
            rs.append(r)
        pl, pr, ql, qr = proof["finals"][k]
        if k == 0:
            if ((pl * qr + pr * ql) % p, ql * qr % p) != (a, b):
                raise Reject("root", 0)
        elif eq_point(z, rs, p) * (pl * qr + pr * ql + lam * ql * qr) % p != claim:
            raise Reject("final", k)
        rho = draw(k, k, [pl, pr, ql, qr])
        a, b = (pl + rho * (pr - pl)) % p, (ql + rho * (qr - ql)) % p
        z = rs + [rho]
        if k + 1 < n:
            lam = draw(k, k + 1, [])
    if ones and a != 1 % p:
        raise Reject("numerator")
    return z, a, b


def multiplicities(w, t, idx):
    """(mult, mismatches): mult_j = #{i : idx_i = j and w_i = t_j}; every other i is a mismatch and is not counted"""
    mult, bad = [0] * len(t), 0
    for wi, j in zip(w, idx):
        if 0 <= j < len(t) and t[j] == wi:
            mult[j] += 1
        else:
            bad += 1
    return mult, bad


def range_eval(point, p):
    return sum(x << j for j, x in enumerate(point)) % p
