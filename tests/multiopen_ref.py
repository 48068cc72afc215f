"""A pure-Python restatement of the batched-opening protocol (thaler-study_amd/csrc/kernels/multiopen.hpp), test-local: nothing here
imports the package.  Everything is in CANONICAL integers over tests/ligero_ref.py (and tests/expander_ref.py for the expander code);
the tests convert to and from Montgomery words at the boundary.

  powers, weight_tables, eq_at           rho^k, E_t = sum_{k : t_k = t} rho^k eq(r_k, .), eq(a, b)
  round_message, fold, quadratic_at      one round of the sumcheck over sum_t f_t E_t
  RefProver                              steps 1-5 over one ligero_ref.RefProver per table
  exchange                               the whole exchange against a verifier reached through send(tag, *args)
  serialise                              the prover's messages as bytes"""
import expander_ref
import ligero_ref as lref

GOLD = lref.GOLD
P64 = 2**64 - 59


def powers(rho, count, p):
    return [pow(rho, k, p) for k in range(count)]


def eq_at(a, b, p):
    out = 1
    for x, y in zip(a, b):
        out = out * ((1 - x) * (1 - y) + x * y) % p
    return out


def weight_tables(names, claims, rho, p):
    """{name: E_t}: claims = [(name, point, value)], claim k weighted by rho^k"""
    coeff = powers(rho, len(claims), p)
    n = len(claims[0][1])
    out = {name: [0] * (1 << n) for name in names}
    for ck, (name, point, _) in zip(coeff, claims):
        eq = lref.eq_weights(point, p)
        out[name] = [(a + ck * b) % p for a, b in zip(out[name], eq)]
    return out


def round_message(fs, es, p):
    """H(0), H(1), H(2) over the pairs (f_t, E_t)"""
    msg = [0, 0, 0]
    for f, e in zip(fs, es):
        for i in range(len(f) // 2):
            f0, f1, e0, e1 = f[2 * i], f[2 * i + 1], e[2 * i], e[2 * i + 1]
            msg[0] += f0 * e0
            msg[1] += f1 * e1
            msg[2] += (2 * f1 - f0) * (2 * e1 - e0)
    return [x % p for x in msg]


def fold(u, r, p):
    return [(u[2 * i] + r * (u[2 * i + 1] - u[2 * i])) % p for i in range(len(u) // 2)]


def quadratic_at(msg, x, p):
    """the quadratic through (0, msg[0]), (1, msg[1]), (2, msg[2]) at x"""
    inv2 = pow(2, -1, p)
    l0 = (x - 1) * (x - 2) % p * inv2 % p
    l1 = -x * (x - 2) % p
    l2 = x * (x - 1) % p * inv2 % p
    return (msg[0] * l0 + msg[1] * l1 + msg[2] * l2) % p


def sumcheck(fs, es, p, draw):
    """(rounds, challenges, finals_f, finals_e): draw(j, msg) -> r_j"""
    fs, es = [list(f) for f in fs], [list(e) for e in es]
    rounds, rs = [], []
    j = 0
    while len(fs[0]) > 1:
        msg = round_message(fs, es, p)
        r = draw(j, msg)
        rounds.append(msg)
        rs.append(r)
        fs, es = [fold(f, r, p) for f in fs], [fold(e, r, p) for e in es]
        j += 1
    return rounds, rs, [f[0] for f in fs], [e[0] for e in es]


class RefProver:
    """the prover of one group: tables = {name: table of 2^n canonical values} (the order is the group's), all committed with
    log_cols = c, blow-up 1 and the code `code` ("rs" or "expander")"""

    def __init__(self, tables, c, p, code="rs"):
        self.names, self.tables, self.c, self.p, self.code = list(tables), {k: [int(x) for x in v] for k, v in tables.items()}, c, p, code
        self.n = len(next(iter(self.tables.values()))).bit_length() - 1
        make = (lambda t: expander_ref.RefProver(t, c, p)) if code == "expander" else (lambda t: lref.RefProver(t, c, 1, p))
        self.pcs = {name: make(self.tables[name]) for name in self.names}

    def roots(self):
        return {name: self.pcs[name].root() for name in self.names}

    def begin(self, claims, rho):
        self.claims = [(name, [int(x) for x in point], int(value)) for name, point, value in claims]
        self.weights = weight_tables(self.names, self.claims, rho, self.p)

    def sumcheck(self, draw):
        rounds, self.z, self.finals, self.e = sumcheck([self.tables[t] for t in self.names], [self.weights[t] for t in self.names], self.p, draw)
        return rounds

    def combine(self, gamma):
        p, C = self.p, 1 << self.c
        eq_rows = lref.eq_weights(self.z[self.c:], p)
        u_gamma, u_z = [0] * C, [0] * C
        for t, g, e in zip(self.names, gamma, self.e):
            ug = lref.combine(self.tables[t], self.c, g, p)
            uz = lref.combine(self.tables[t], self.c, [e * w % p for w in eq_rows], p)
            u_gamma = [(a + b) % p for a, b in zip(u_gamma, ug)]
            u_z = [(a + b) % p for a, b in zip(u_z, uz)]
        return u_gamma, u_z

    def open_columns(self, indices):
        return {t: self.pcs[t].open_columns(indices) for t in self.names}


def exchange(prover, claims, send):
    """steps 1-5 against a verifier reached through send(tag, *args) -> its reply: "claims" -> rho, "round" -> r_j, "gamma" ->
    T vectors, "rows" -> None, "columns" -> the indices, "open" -> its verdict.  Returns the transcript"""
    rho = send("claims", claims)
    prover.begin(claims, rho)
    rounds = prover.sumcheck(lambda j, msg: send("round", j, msg))
    gamma = send("gamma")
    u_gamma, u_z = prover.combine(gamma)
    send("rows", u_gamma, u_z)
    indices = send("columns")
    openings = prover.open_columns(indices)
    verdict = send("open", openings)
    return {"rho": rho, "rounds": rounds, "z": list(prover.z), "e": list(prover.e), "finals": list(prover.finals), "gamma": gamma,
            "u_gamma": u_gamma, "u_z": u_z, "indices": indices, "openings": openings, "verdict": verdict}


def serialise(out):
    """the prover's messages of one exchange, as they would go over a wire: every round's three words, the two combined rows,
    and per query and commitment the column's words and its path's digests"""
    words = [x for msg in out["rounds"] for x in msg] + list(out["u_gamma"]) + list(out["u_z"])
    blob = b"".join(int(x).to_bytes(8, "little") for x in words)
    for q in range(len(out["indices"])):
        for t in out["openings"]:
            _, col, path = out["openings"][t][q]
            blob += b"".join(int(x).to_bytes(8, "little") for x in col) + b"".join(path)
    return blob
