"""A pure-Python restatement of the grand product argument's contract (thaler-study_amd/csrc/kernels/grand_product.hpp),
test-local: nothing here imports the package or reads csrc/.  Everything is in CANONICAL integers; the tests convert to and from
Montgomery words at the boundary (mont / canon).

  tree(t, p)                      [V_0, .., V_n], V_n = t, V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k]: the tree by halves
  eq_table, eq_point, mle_eval    eq and the multilinear extension by their definitions
  fold, layer_round, cubic_at     one fold (variable 0), H(0..3) of one round straight from the definition, the cubic's value
  prove(t, p, draw)               the layer prover under draw(layer, round, msg) -> challenge: a dict of every message
  verify(n, p, proof, draw)       the verifier: (point, claim), or Reject(kind, layer, round)
  affine(t, alpha, beta, p)"""


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


def tree(t, p):
    layers = [list(t)]
    while len(layers[0]) > 1:
        top = layers[0]
        half = len(top) // 2
        layers.insert(0, [top[x] * top[x + half] % p for x in range(half)])
    return layers


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


def layer_round(E, L, R, p):
    """H(t) = sum_i e_i(t) l_i(t) r_i(t) at t = 0, 1, 2, 3, with u_i(t) = u[2i] + t (u[2i+1] - u[2i])"""
    out = [0, 0, 0, 0]
    for i in range(len(E) // 2):
        e0, l0, r0 = E[2 * i], L[2 * i], R[2 * i]
        de, dl, dr = E[2 * i + 1] - e0, L[2 * i + 1] - l0, R[2 * i + 1] - r0
        for t in range(4):
            out[t] += (e0 + t * de) * (l0 + t * dl) * (r0 + t * dr)
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


def affine(t, alpha, beta, p):
    return [(alpha * x + beta) % p for x in t]


def prove(t, p, draw, layers=None):
    """every message of the prover under draw(layer, round, msg): product, rounds[k][j][4], finals[k] = (l, r'), challenges (protocol
    order), point = z_n, claim = c_n"""
    V = layers or tree(t, p)
    n = len(V) - 1
    z, claim = [], V[0][0]
    rounds, finals, challenges = [], [], []
    for k in range(n):
        half = 1 << k
        E, L, R = eq_table(z, p), V[k + 1][:half], V[k + 1][half:]
        rs, msgs = [], []
        for j in range(k):
            msg = layer_round(E, L, R, p)
            r = draw(k, j, msg)
            E, L, R = (fold(u, r, p) for u in (E, L, R))
            rs.append(r)
            msgs.append(msg)
        l, r2 = L[0], R[0]
        rho = draw(k, k, [l, r2])
        claim = (l + rho * (r2 - l)) % p
        z = rs + [rho]
        rounds.append(msgs)
        finals.append((l, r2))
        challenges += rs + [rho]
    return {"product": V[0][0], "rounds": rounds, "finals": finals, "challenges": challenges, "point": z, "claim": claim}


class Reject(Exception):
    def __init__(self, kind, layer, round_index=None):
        super().__init__("%s at layer %s round %s" % (kind, layer, round_index))
        self.kind, self.layer, self.round = kind, layer, round_index


def verify(n, p, proof, draw):
    """the verifier over a prove() dict under draw(layer, round, msg); returns (point, claim).  Reject kinds: "product" (layer 0's
    finals), "round", "final" """
    z, claim = [], proof["product"] % p
    for k in range(n):
        rs = []
        for j in range(k):
            msg = proof["rounds"][k][j]
            if (msg[0] + msg[1]) % p != claim:
                raise Reject("round", k, j)
            r = draw(k, j, msg)
            claim = cubic_at(msg, r, p)
            rs.append(r)
        l, r2 = proof["finals"][k]
        if eq_point(z, rs, p) * l * r2 % p != claim:
            raise Reject("product" if k == 0 else "final", k)
        rho = draw(k, k, [l, r2])
        claim = (l + rho * (r2 - l)) % p
        z = rs + [rho]
    return z, claim
