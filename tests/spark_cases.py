"""Shared by tests/test_spark_cpu.py and tests/test_gpu_spark.py: the cases of the SPARK tests in canonical integers, the choice of
an alpha outside the keys, and the reference prover (tests/spark_ref.py) driven by the package's host Verifier."""
import random

import spark_ref as ref

GOLD = 2**64 - 2**32 + 1
P64 = 2**64 - 59
P61 = 2**61 - 1


def edge_or_random(p, rng, share=0.3):
    edge = [0, 1, p - 1, p - 2, (p - 1) // 2, 2**64 % p, (2**32 - 1) % p]
    return rng.choice(edge) if rng.random() < share else rng.randrange(p)


def case(p, a, b, nnz, seed):
    """(triples, U, W): nnz triples of a 2^a x 2^b matrix with one (row, col) pair repeated (where nnz >= 2) and edge words among
    the values; U, W tables of edge and random words"""
    rng = random.Random(seed)
    triples = [(rng.randrange(1 << a), rng.randrange(1 << b), edge_or_random(p, rng)) for _ in range(nnz)]
    if nnz >= 2:
        triples[-1] = (triples[0][0], triples[0][1], rng.randrange(1, p))
    U = [edge_or_random(p, rng) for _ in range(1 << a)]
    W = [edge_or_random(p, rng) for _ in range(1 << b)]
    return triples, U, W


def keys(triples, U, W, beta, p, er=None, ec=None):
    """every idx_k + beta e[k] and i + beta T[i] of both dimensions: the alphas with a zero denominator"""
    _, rows, cols, _ = ref.pad(triples)
    er = [U[i] for i in rows] if er is None else er
    ec = [W[j] for j in cols] if ec is None else ec
    out = set()
    for idx, e, T in ((rows, er, U), (cols, ec, W)):
        out |= {(i + beta * x) % p for i, x in zip(idx, e)} | {(i + beta * x) % p for i, x in enumerate(T)}
    return out


def sums(triples, U, W, alpha, beta, p, a, b, er=None, ec=None, cr=None, cc=None):
    """{dim: (sum_k 1 / den_w[k], sum_i cnt_i / den_t[i])} by the definition; alpha outside keys()"""
    _, rows, cols, _ = ref.pad(triples)
    er = [U[i] for i in rows] if er is None else er
    ec = [W[j] for j in cols] if ec is None else ec
    cr = ref.counts(rows, a) if cr is None else cr
    cc = ref.counts(cols, b) if cc is None else cc
    out = {}
    for dim, idx, e, T, cnt in (("row", rows, er, U, cr), ("col", cols, ec, W, cc)):
        den_w, den_t = ref.denominators(idx, e, T, alpha, beta, p)
        out[dim] = (sum(pow(x, -1, p) for x in den_w) % p, sum(c * pow(x, -1, p) for c, x in zip(cnt, den_t)) % p)
    return out


def alpha_outside(triples, U, W, beta, p, a, b, rng, dishonest):
    """alpha with no zero denominator.  Over p = 257 a random alpha hits one of the up to 2 (2^l + 2^a + 2^b) keys with a
    probability that is not small, so it is drawn again until it is outside them: every denominator is then invertible and the
    claim the test checks is the papers'.  Where the prover's tables are dishonest it is also drawn again until the two sums of
    the changed dimension differ (over a small field they coincide at up to 2^l + 2^a of the p values of alpha)"""
    used = keys(triples, U, W, beta, p, dishonest.get("er"), dishonest.get("ec"))
    while True:
        alpha = rng.randrange(4, p)
        if alpha in used:
            continue
        s = sums(triples, U, W, alpha, beta, p, a, b, **dishonest)
        wrong = [dim for dim, tables in (("row", ("er", "cr")), ("col", ("ec", "cc"))) if any(t in dishonest for t in tables)]
        if all(s[dim][0] != s[dim][1] for dim in wrong):
            return alpha


class Opening:
    """stands where the verifier of a commitment's openings stands in spark.Verifier: only num_vars is read on the CPU"""

    def __init__(self, num_vars):
        self.num_vars = num_vars


class Draws:
    """the rng of the package's verifier: canonical words >= 4 from a random.Random (a changed H(2) or H(3) goes unnoticed exactly
    when the round's challenge is another interpolation point), or the words forced ahead; draw() returns Montgomery words"""

    def __init__(self, p, seed):
        self.p, self.rng, self.forced = p, random.Random(seed), []

    def draw(self):
        c = self.forced.pop(0) if self.forced else self.rng.randrange(4, self.p)
        return ref.mont(c, self.p)


def drive(pkg, p, a, b, triples, U, W, seed, tamper=None, dishonest=None, u_eval=None, w_eval=None, before_finish=None):
    """the reference prover under the package's spark.Verifier.  tamper(tag, args) -> args changes one message on its way
    (canonical integers); dishonest: the prover's own er, ec, cr or cc.  Returns (v as a Montgomery word, the reference's dict)"""
    sp, F = pkg.spark, pkg.Field(p)
    dishonest = dishonest or {}
    ell = ref.log_len(len(triples))
    draws = Draws(p, seed)
    point_of = lambda z: ref.canon_list(z, p)   # noqa: E731
    u_eval = u_eval or (lambda z: ref.mont(ref.mle_eval(U, point_of(z), p), p))
    w_eval = w_eval or (lambda z: ref.mont(ref.mle_eval(W, point_of(z), p), p))
    sizes = {"row": ell, "col": ell, "val": ell, "cr": a, "cc": b}
    V = sp.Verifier(F, a, b, ell, {name: Opening(n) for name, n in sizes.items()}, u_eval, w_eval)
    V.receive_commitments(Opening(ell), Opening(ell))
    opened, challengers, state = {}, {}, {}

    def send(tag, *args):
        if tamper:
            args = tamper(tag, args)
        if tag == "v":
            return V.receive_claim(ref.mont(args[0], p))
        if tag == "round":
            return ref.canon(V.round(args[0], ref.mont_list(args[1], p), draws), p)
        if tag == "finals":
            return V.receive_finals(*ref.mont_list(args[0], p))
        if tag == "beta":
            beta = draws.rng.randrange(4, p)
            state["alpha"] = alpha_outside(triples, U, W, beta, p, a, b, draws.rng, dishonest)
            draws.forced += [beta, state["alpha"]]
            assert V.draw_lookup(draws) == (ref.mont(state["alpha"], p), ref.mont(beta, p))
            return beta
        if tag == "alpha":
            return state["alpha"]
        if tag == "roots":
            return V.receive_roots(args[0], *[tuple(ref.mont_list(r, p)) for r in args[1:]])
        if tag == "frac":
            dim, side, k, j, msg = args
            if (dim, side) not in challengers:
                challengers[(dim, side)] = V.frac[dim][side].challenger(draws)
            return ref.canon(challengers[(dim, side)](k, j, ref.mont_list(msg, p)), p)
        assert tag == "open"
        table, at, point, value = args
        state.setdefault("points", {})[(table, at)] = ref.mont_list(point, p)
        opened[(table, at)] = ref.mont(value, p)

    out = ref.exchange(p, a, b, triples, U, W, send, **dishonest)
    assert [(t, at) for t, at, _ in V.openings()] == list(ref.OPENINGS)
    for table, at, point in V.openings():
        assert point == state["points"][(table, at)], (table, at)
    if before_finish:
        before_finish(V)
    assert V.finish(opened) is True
    return V.v, out
