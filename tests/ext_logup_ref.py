"""A pure-Python restatement of LogUp's fraction sums over K = F_p[X] / (X^2 - w)
(thaler-study_amd/csrc/kernels/ext_fraction.hpp), test-local: nothing here imports the package or reads csrc/.  Everything is in
CANONICAL integers; an element of K is a pair (c0, c1).  Products are ext_ref's plain schoolbook products - four base
multiplications - so nothing here shares the kernels' Karatsuba formula, their base x K leaf products, their affine leaf fold or
their stepped lambda qr(t).

  leaves(pt, t, alpha, beta, p, w)      (p_n, q_n): p_n[i] = (pt[i], 0) or (1, 0) (pt None), q_n[i] = beta + alpha t[i]
  tree(p_n, q_n, p, w)                  ([p_0, .., p_n], [q_0, .., q_n]): the fraction-sum tree by halves
  layer_round, kmle                     H(0..3) of one round straight from the definition; an extension table's extension at a point
  prove(pt, t, alpha, beta, p, w, draw) the layer prover under draw(layer, round, msg) -> challenge in K: a dict of every message
  verify(n, p, w, proof, draw, ones)    the verifier: (point, a, b), or Reject(kind, layer, round)
  synthetic_draw(p, seed_r)             the engine's synthetic challenger
  range_eval(point, p)                  the extension in K of t_j = j: sum_j 2^j point_j"""
import ext_ref as X
from ext_gp_ref import cubic_at, eq_point
from ext_ref import kadd, kmul, ksub


def leaves(pt, t, alpha, beta, p, w):
    q = [kadd(beta, kmul(alpha, (int(x) % p, 0), p, w), p) for x in t]
    num = [(int(x) % p, 0) for x in pt] if pt is not None else [(1 % p, 0)] * len(q)
    return num, q


def tree(top_p, top_q, p, w):
    P, Q = [list(top_p)], [list(top_q)]
    while len(Q[0]) > 1:
        tp, tq = P[0], Q[0]
        half = len(tq) // 2
        P.insert(0, [kadd(kmul(tp[x], tq[x + half], p, w), kmul(tp[x + half], tq[x], p, w), p) for x in range(half)])
        Q.insert(0, [kmul(tq[x], tq[x + half], p, w) for x in range(half)])
    return P, Q


def layer_round(E, PL, PR, QL, QR, lam, p, w):
    """H(t) = sum_i e_i(t) (pl_i(t) qr_i(t) + pr_i(t) ql_i(t) + lam ql_i(t) qr_i(t)) in K at t = 0, 1, 2, 3, with
    u_i(t) = u[2i] + t (u[2i+1] - u[2i])"""
    out = [(0, 0)] * 4
    for i in range(len(E) // 2):
        for t in range(4):
            e, pl, pr, ql, qr = (kadd(u[2 * i], kmul((t, 0), ksub(u[2 * i + 1], u[2 * i], p), p, w), p) for u in (E, PL, PR, QL, QR))
            inner = kadd(kadd(kmul(pl, qr, p, w), kmul(pr, ql, p, w), p), kmul(lam, kmul(ql, qr, p, w), p, w), p)
            out[t] = kadd(out[t], kmul(e, inner, p, w), p)
    return out


def kmle(table, point, p, w):
    """sum_i table[i] eq(point, i) for a table of elements of K"""
    out = (0, 0)
    for e, v in zip(X.eq_weights(point, p, w), table):
        out = kadd(out, kmul(e, v, p, w), p)
    return out


def n_challenges(n):
    """rho_0, then per layer k >= 1: lambda_k, k rounds, rho_k"""
    return n * (n - 1) // 2 + 2 * n - 1


def _elem(r, p):
    return (int(r[0]) % p, int(r[1]) % p)


def prove(pt, t, alpha, beta, p, w, draw, layers=None):
    """every message of the prover under draw(layer, round, msg): root = (P, Q), rounds[k][j][4], finals[k] = (pl, pr, ql, qr),
    challenges (as drawn: rho_0, then per layer lambda_k, r_0 .., rho_k), lambdas[k], point = z_n, claims = (a_n, b_n) - every element
    a pair.  draw(k, k + 1, []) is the lambda of layer k + 1"""
    P, Q = layers or tree(*leaves(pt, t, alpha, beta, p, w), p, w)
    n = len(Q) - 1
    z, a, b, lam = [], P[0][0], Q[0][0], (0, 0)
    rounds, finals, challenges, lambdas = [], [], [], [None]
    for k in range(n):
        half = 1 << k
        E = X.eq_weights(z, p, w)
        PL, PR, QL, QR = P[k + 1][:half], P[k + 1][half:], Q[k + 1][:half], Q[k + 1][half:]
        rs, msgs = [], []
        for j in range(k):
            msg = layer_round(E, PL, PR, QL, QR, lam, p, w)
            r = _elem(draw(k, j, msg), p)
            E, PL, PR, QL, QR = (X.fold(u, r, p, w) for u in (E, PL, PR, QL, QR))
            rs.append(r)
            msgs.append(msg)
        fin = (PL[0], PR[0], QL[0], QR[0])
        rho = _elem(draw(k, k, list(fin)), p)
        a = kadd(fin[0], kmul(rho, ksub(fin[1], fin[0], p), p, w), p)
        b = kadd(fin[2], kmul(rho, ksub(fin[3], fin[2], p), p, w), p)
        z = rs + [rho]
        rounds.append(msgs)
        finals.append(fin)
        challenges += rs + [rho]
        if k + 1 < n:
            lam = _elem(draw(k, k + 1, []), p)
            lambdas.append(lam)
            challenges.append(lam)
    return {"root": (P[0][0], Q[0][0]), "rounds": rounds, "finals": finals, "challenges": challenges, "lambdas": lambdas, "point": z,
            "claims": (a, b)}


class Reject(Exception):
    def __init__(self, kind, layer=None, round_index=None):
        super().__init__("%s at layer %s round %s" % (kind, layer, round_index))
        self.kind, self.layer, self.round = kind, layer, round_index


def verify(n, p, w, proof, draw, ones=False):
    """the verifier over a prove() dict under draw(layer, round, msg); returns (point, a, b).  Reject kinds: "root" (layer 0's
    finals), "round", "final", "numerator" (ones: a_n != 1)"""
    z, (a, b), lam = [], proof["root"], (0, 0)
    for k in range(n):
        claim = kadd(a, kmul(lam, b, p, w), p)
        rs = []
        for j in range(k):
            msg = proof["rounds"][k][j]
            if kadd(msg[0], msg[1], p) != claim:
                raise Reject("round", k, j)
            r = draw(k, j, msg)
            claim = cubic_at(msg, r, p, w)
            rs.append(r)
        pl, pr, ql, qr = proof["finals"][k]
        num, den = kadd(kmul(pl, qr, p, w), kmul(pr, ql, p, w), p), kmul(ql, qr, p, w)
        if k == 0:
            if (num, den) != (a, b):
                raise Reject("root", 0)
        elif kmul(eq_point(z, rs, p, w), kadd(num, kmul(lam, den, p, w), p), p, w) != claim:
            raise Reject("final", k)
        rho = draw(k, k, [pl, pr, ql, qr])
        a, b = kadd(pl, kmul(rho, ksub(pr, pl, p), p, w), p), kadd(ql, kmul(rho, ksub(qr, ql, p), p, w), p)
        z = rs + [rho]
        if k + 1 < n:
            lam = draw(k, k + 1, [])
    if ones and a != (1 % p, 0):
        raise Reject("numerator")
    return z, a, b


def synthetic_draw(p, seed_r):
    """draw number d = 0, 1, .. in the order drawn is (splitmix64(seed_r + 2 d + 1) mod p, splitmix64(seed_r + 2 d + 2) mod p)"""
    count = [0]

    def draw(layer, j, msg):
        d = count[0]
        count[0] += 1
        return (X.splitmix64((seed_r + 2 * d + 1) & X.M64) % p, X.splitmix64((seed_r + 2 * d + 2) & X.M64) % p)
    return draw


def range_eval(point, p):
    return (sum(x[0] << j for j, x in enumerate(point)) % p, sum(x[1] << j for j, x in enumerate(point)) % p)
