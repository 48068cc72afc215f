"""A pure-Python restatement of the staged folded opening's contract (thaler-study_amd/csrc/kernels/rs_fold.hpp, the section on
schedules) over ligero_fold_ref, test-local: nothing here imports the package.  Everything is in CANONICAL integers.

  starts(arities)                   i_s, the first round of every stage
  fold_many(U, alphas, p)           len(alphas) successive folds of ligero_fold_ref.fold - the definition of a stage's fold
  fold_leaf(words, alphas, ...)     the same fold of ONE leaf: word j of the result from the 2^a words U[j + t M / 2^a] alone
  stage_leaf, stage_levels          the leaf of a stage (its 2^a words as a column) and the tree over a stage's layer
  RefStagedProver                   every message of the opening under a schedule; .messages collects them for message_bytes
  message_bytes(messages)           the bytes of an opening, counted message by message
  opening_bytes, best_shape         the size formula written out, and the smallest opening by brute force over every schedule"""
import hashlib

import ligero_fold_ref as fref
import ligero_ref as ref


def starts(arities):
    out, i = [], 0
    for a in arities:
        out.append(i)
        i += a
    return out


def fold_many(U, alphas, p):
    for alpha in alphas:
        U = fref.fold(U, alpha, p)
    return U


def fold_leaf(words, alphas, p, log_m, j):
    """word j of fold_many(U, alphas) from words[t] = U[j + t M / 2^a], M = 2^log_m, a = len(alphas): level l folds the words t and
    t + 2^(a-1-l) at x = w_(log_m - l)^(j + t M / 2^a)"""
    a = len(alphas)
    stride = (1 << log_m) >> a
    inv2 = pow(2, -1, p)
    words = list(words)
    for l, alpha in enumerate(alphas):
        w = ref.omega(p, log_m - l)
        h = 1 << (a - 1 - l)
        nxt = []
        for t in range(h):
            xinv = pow(w, -(j + t * stride), p)
            even = (words[t] + words[t + h]) * inv2 % p
            odd = (words[t] - words[t + h]) * inv2 * xinv % p
            nxt.append((even + alpha * (odd - even)) % p)
        words = nxt
    return words[0]


def stage_leaf(words):
    return hashlib.sha256(b"".join(int(w).to_bytes(8, "little") for w in words)).digest()


def stage_leaves(U, a):
    n = len(U) >> a
    return [stage_leaf([U[j + t * n] for t in range(1 << a)]) for j in range(n)]


def stage_levels(U, a):
    return ref.tree_levels(stage_leaves(U, a))


class RefStagedProver:
    """the prover of a staged folded opening over a ligero_ref.RefProver's commitment.  corrupt(s, U) -> U, if given, replaces the
    layer of stage s >= 1 before it is committed (a prover that folds wrongly but hashes what it holds)"""

    def __init__(self, table, c, rho, p, arities, corrupt=None, commitment=None):
        assert c >= 1 and sum(arities) == c and all(1 <= a <= 3 for a in arities)
        self.table, self.c, self.rho, self.p = [int(x) for x in table], c, rho, p
        self.arities, self.starts = tuple(arities), starts(arities)
        self.commitment = commitment or ref.RefProver(self.table, c, rho, p)
        self.corrupt = corrupt
        self.messages = []

    def root(self):
        return self.commitment.root()

    def begin(self, point, gamma):
        p, c = self.p, self.c
        self.z_lo = [int(x) for x in point[:c]]
        self.u_gamma, self.u_z = self.commitment.combine([int(x) for x in point], [int(x) for x in gamma])
        eq = ref.eq_weights(self.z_lo, p)
        v = sum(a * b for a, b in zip(self.u_z, eq)) % p
        v_gamma = sum(a * b for a, b in zip(self.u_gamma, eq)) % p
        self.messages.append(("claims", (v, v_gamma)))
        return v, v_gamma

    def prove(self, beta, draw):
        """draw(i, [H(0), H(1), H(2)], root or None) -> alpha_i, the root at the first round of every stage s >= 1.  Returns
        (rounds, roots, challenges, final)"""
        p, c, rho = self.p, self.c, self.rho
        m = [(a + beta * b) % p for a, b in zip(self.u_z, self.u_gamma)]
        eq = ref.eq_weights(self.z_lo, p)
        U = ref.encode(m, c, rho, p)[0]
        self.layers, self.levels = [U], [None]
        rounds, roots, alphas = [], [], []
        for s, a in enumerate(self.arities):
            stage = []
            for k in range(a):
                i = self.starts[s] + k
                sums = fref.round_sums(m, eq, p)
                root = self.levels[s][-1][0] if s and k == 0 else None
                rounds.append(sums)
                self.messages.append(("round", sums))
                if root is not None:
                    roots.append(root)
                    self.messages.append(("root", root))
                alpha = int(draw(i, sums, root))
                alphas.append(alpha)
                stage.append(alpha)
                m, eq = fref.fix_variables(m, [alpha], p), fref.fix_variables(eq, [alpha], p)
            U = fold_many(U, stage, p)
            if s + 1 < len(self.arities):
                if self.corrupt:
                    U = self.corrupt(s + 1, U)
                self.layers.append(U)
                self.levels.append(stage_levels(U, self.arities[s + 1]))
        assert self.corrupt or U == [m[0]] * (1 << rho), "U_c is 2^rho equal words"
        self.messages.append(("final", U[0]))
        return rounds, roots, alphas, U[0]

    def query(self, indices):
        """[(q, [the 2^a_0 columns q + t L / 2^a_0], stages)], a column as RefProver.open_columns gives it, stages[s - 1] =
        (the 2^a_s words of leaf j_s, siblings)"""
        l0 = self.c + self.rho
        a0 = self.arities[0]
        out = []
        for q in indices:
            cols = self.commitment.open_columns([q + t * (1 << (l0 - a0)) for t in range(1 << a0)])
            stages = []
            for s in range(1, len(self.arities)):
                U, a = self.layers[s], self.arities[s]
                n = len(U) >> a
                j = q % n
                stages.append((tuple(U[j + t * n] for t in range(1 << a)), ref.path_of(self.levels[s], j)))
            out.append((q, list(cols), stages))
            self.messages.append(("query", (cols, stages)))
        return out


def message_bytes(messages):
    """8 bytes a word, 32 a digest; indices are the verifier's and cost nothing"""
    total = 0
    for kind, body in messages:
        if kind == "claims":
            total += 16
        elif kind == "round":
            total += 8 * len(body)
        elif kind == "root":
            total += 32
        elif kind == "final":
            total += 8
        else:
            cols, stages = body
            for _, values, siblings in cols:
                total += 8 * len(values) + 32 * len(siblings)
            for words, siblings in stages:
                total += 8 * len(words) + 32 * len(siblings)
    return total


def opening_bytes(n, c, rho, queries, arities):
    """the size formula, term by term"""
    l0 = c + rho
    per_query = (1 << arities[0]) * (8 * (1 << (n - c)) + 32 * l0)
    for i, a in list(zip(starts(arities), arities))[1:]:
        per_query += 8 * (1 << a) + 32 * (l0 - i - a)
    return queries * per_query + 32 * (len(arities) - 1) + 24 * c + 24


def schedules(c, max_arity=3):
    """every schedule of c rounds, in lexicographic order"""
    if c == 0:
        yield ()
        return
    for a in range(1, min(max_arity, c) + 1):
        for rest in schedules(c - a, max_arity):
            yield (a,) + rest


def best_shape(n, rho, queries, max_arity=3, max_log_len=24):
    """(bytes, c, arities) of the smallest opening: every c and every schedule tried"""
    return min((opening_bytes(n, c, rho, queries, ar), c, ar) for c in range(1, min(n, max_log_len - rho) + 1) for ar in schedules(c, max_arity))

