"""A pure-Python restatement of the grand product argument over K = F_p[X] / (X^2 - w)
(thaler-study_amd/csrc/kernels/ext_grand_product.hpp), test-local: nothing here imports the package or reads csrc/.  Everything is in
CANONICAL integers; an element of K is a pair (c0, c1).  Products are ext_ref's plain schoolbook products - four base
multiplications - so nothing here shares the kernels' Karatsuba formula, their affine leaf fold or their doubling eq table.

  leaves(t, alpha, beta, p, w)          V_n[i] = beta + alpha t[i]
  tree(V_n, p, w)                       [V_0, .., V_n], V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k]
  layer_round, cubic_at, eq_point       H(0..3) of one round straight from the definition, the cubic's value, eq of two points
  prove(t, alpha, beta, p, w, draw)     the layer prover under draw(layer, round, msg) -> challenge in K: a dict of every message
  verify(n, p, w, proof, draw)          the verifier: (point, claim), or Reject(kind, layer, round)
  synthetic_draw(p, seed_r)             the engine's synthetic challenger"""
import ext_ref as X
from ext_ref import kadd, kmul, ksub


def leaves(t, alpha, beta, p, w):
    return [kadd(beta, kmul(alpha, (int(x) % p, 0), p, w), p) for x in t]


def tree(top, p, w):
    layers = [list(top)]
    while len(layers[0]) > 1:
        cur = layers[0]
        half = len(cur) // 2
        layers.insert(0, [kmul(cur[x], cur[x + half], p, w) for x in range(half)])
    return layers


def eq_point(a, b, p, w):
    out = (1, 0)
    for x, y in zip(a, b):
        xy = kmul(x, y, p, w)
        out = kmul(out, kadd(ksub(ksub((1, 0), x, p), y, p), kadd(xy, xy, p), p), p, w)
    return out


def layer_round(E, L, R, p, w):
    """H(t) = sum_i e_i(t) l_i(t) r_i(t) in K at t = 0, 1, 2, 3, with u_i(t) = u[2i] + t (u[2i+1] - u[2i])"""
    out = [(0, 0)] * 4
    for i in range(len(E) // 2):
        for t in range(4):
            at = [kadd(u[2 * i], kmul((t, 0), ksub(u[2 * i + 1], u[2 * i], p), p, w), p) for u in (E, L, R)]
            out[t] = kadd(out[t], kmul(at[0], kmul(at[1], at[2], p, w), p, w), p)
    return out


def cubic_at(e, x, p, w):
    """the cubic through (0, e0) .. (3, e3), e_k in K, at x in K (Lagrange)"""
    total = (0, 0)
    for k in range(4):
        num, den = (1, 0), 1
        for l in range(4):
            if l != k:
                num = kmul(num, ksub(x, (l, 0), p), p, w)
                den = den * (k - l) % p
        total = kadd(total, kmul(e[k], kmul(num, (pow(den, -1, p), 0), p, w), p, w), p)
    return total


def prove(t, alpha, beta, p, w, draw, layers=None):
    """every message of the prover under draw(layer, round, msg): product, rounds[k][j][4], finals[k] = (l, r'), challenges (protocol
    order), point = z_n, claim = c_n - every element a pair"""
    V = layers or tree(leaves(t, alpha, beta, p, w), p, w)
    n = len(V) - 1
    z, claim = [], V[0][0]
    rounds, finals, challenges = [], [], []
    for k in range(n):
        half = 1 << k
        E, L, R = X.eq_weights(z, p, w), V[k + 1][:half], V[k + 1][half:]
        rs, msgs = [], []
        for j in range(k):
            msg = layer_round(E, L, R, p, w)
            r = draw(k, j, msg)
            r = (int(r[0]) % p, int(r[1]) % p)
            E, L, R = (X.fold(u, r, p, w) for u in (E, L, R))
            rs.append(r)
            msgs.append(msg)
        l, r2 = L[0], R[0]
        rho = draw(k, k, [l, r2])
        rho = (int(rho[0]) % p, int(rho[1]) % p)
        claim = kadd(l, kmul(rho, ksub(r2, l, p), p, w), p)
        z = rs + [rho]
        rounds.append(msgs)
        finals.append((l, r2))
        challenges += rs + [rho]
    return {"product": V[0][0], "rounds": rounds, "finals": finals, "challenges": challenges, "point": z, "claim": claim}


class Reject(Exception):
    def __init__(self, kind, layer, round_index=None):
        super().__init__("%s at layer %s round %s" % (kind, layer, round_index))
        self.kind, self.layer, self.round = kind, layer, round_index


def verify(n, p, w, proof, draw):
    """the verifier over a prove() dict under draw(layer, round, msg); returns (point, claim).  Reject kinds: "product" (layer 0's
    finals), "round", "final" """
    z, claim = [], proof["product"]
    for k in range(n):
        rs = []
        for j in range(k):
            msg = proof["rounds"][k][j]
            if kadd(msg[0], msg[1], p) != claim:
                raise Reject("round", k, j)
            r = draw(k, j, msg)
            claim = cubic_at(msg, r, p, w)
            rs.append(r)
        l, r2 = proof["finals"][k]
        if kmul(eq_point(z, rs, p, w), kmul(l, r2, p, w), p, w) != claim:
            raise Reject("product" if k == 0 else "final", k)
        rho = draw(k, k, [l, r2])
        claim = kadd(l, kmul(rho, ksub(r2, l, p), p, w), p)
        z = rs + [rho]
    return z, claim


def n_challenges(n):
    return n * (n + 1) // 2


def synthetic_draw(p, seed_r):
    """draw number d = 0, 1, .. in protocol order is (splitmix64(seed_r + 2 d + 1) mod p, splitmix64(seed_r + 2 d + 2) mod p), canonical"""
    count = [0]

    def draw(layer, j, msg):
        d = count[0]
        count[0] += 1
        return (X.splitmix64((seed_r + 2 * d + 1) & X.M64) % p, X.splitmix64((seed_r + 2 * d + 2) & X.M64) % p)
    return draw
