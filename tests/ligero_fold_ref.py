"""A pure-Python restatement of the folded opening's contract (thaler-study_amd/csrc/kernels/rs_fold.hpp) over ligero_ref,
test-local: nothing here imports the package.  Everything is in CANONICAL integers.

  fold(U, alpha, p)            one fold of a codeword in the contract's order
  fix_variables(m, rs, p)      the LE fix of a table's low variables
  round_sums(a, b, p)          (H(0), H(1), H(2)) of the product sumcheck's round over the tables a and b
  pair_leaf, layer_levels      the leaf of a layer (its two words as a column) and the tree over a layer
  RefFoldProver                every message of steps 3 - 9; .messages collects them for message_bytes
  message_bytes(messages)      the bytes of an opening, counted message by message"""
import hashlib

import ligero_ref as ref


def fold(U, alpha, p):
    """U' of len(U) / 2 words: U'[j] = even + alpha (odd - even), even = (U[j] + U[j + M/2]) / 2, odd = (U[j] - U[j + M/2]) / (2 x),
    x = w_M^j"""
    M = len(U)
    w = ref.omega(p, M.bit_length() - 1)
    inv2, winv = pow(2, -1, p), pow(w, M - 1, p)
    out, xinv = [], 1
    for j in range(M // 2):
        a, b = U[j], U[j + M // 2]
        even = (a + b) * inv2 % p
        odd = (a - b) * inv2 * xinv % p
        out.append((even + alpha * (odd - even)) % p)
        xinv = xinv * winv % p
    return out


def fix_variables(m, rs, p):
    for r in rs:
        m = [(m[2 * b] + r * (m[2 * b + 1] - m[2 * b])) % p for b in range(len(m) // 2)]
    return m


def round_sums(a, b, p):
    out = []
    for t in (0, 1, 2):
        out.append(sum((a[2 * k] + t * (a[2 * k + 1] - a[2 * k])) * (b[2 * k] + t * (b[2 * k + 1] - b[2 * k])) for k in range(len(a) // 2)) % p)
    return out


def pair_leaf(lo, hi):
    return hashlib.sha256(int(lo).to_bytes(8, "little") + int(hi).to_bytes(8, "little")).digest()


def layer_levels(U):
    half = len(U) // 2
    return ref.tree_levels([pair_leaf(U[j], U[j + half]) for j in range(half)])


class RefFoldProver:
    """the prover of a folded opening over a ligero_ref.RefProver's commitment.  corrupt(i, U_i) -> U_i, if given, replaces a
    layer before it is committed (a prover that folds wrongly but hashes what it holds)"""

    def __init__(self, table, c, rho, p, corrupt=None):
        assert c >= 1
        self.table, self.c, self.rho, self.p = [int(x) for x in table], c, rho, p
        self.commitment = ref.RefProver(self.table, c, rho, p)
        self.corrupt = corrupt
        self.messages = []

    def root(self):
        return self.commitment.root()

    def begin(self, point, gamma):
        """step 3: (v, v_gamma)"""
        p, c = self.p, self.c
        self.z_lo = [int(x) for x in point[:c]]
        self.u_gamma, self.u_z = self.commitment.combine([int(x) for x in point], [int(x) for x in gamma])
        eq = ref.eq_weights(self.z_lo, p)
        v = sum(a * b for a, b in zip(self.u_z, eq)) % p
        v_gamma = sum(a * b for a, b in zip(self.u_gamma, eq)) % p
        self.messages.append(("claims", (v, v_gamma)))
        return v, v_gamma

    def prove(self, beta, draw):
        """steps 5 - 7: draw(i, [H(0), H(1), H(2)], root_i or None) -> alpha_i.  Returns (rounds, roots, challenges, final)"""
        p, c, rho = self.p, self.c, self.rho
        m = [(a + beta * b) % p for a, b in zip(self.u_z, self.u_gamma)]
        eq = ref.eq_weights(self.z_lo, p)
        U = ref.encode(m, c, rho, p)[0]
        self.layers, self.levels = [U], [None]
        rounds, roots, alphas = [], [], []
        for i in range(c):
            sums = round_sums(m, eq, p)
            root = self.levels[i][-1][0] if i else None
            rounds.append(sums)
            self.messages.append(("round", sums))
            if i:
                roots.append(root)
                self.messages.append(("root", root))
            alpha = int(draw(i, sums, root))
            alphas.append(alpha)
            m, eq = fix_variables(m, [alpha], p), fix_variables(eq, [alpha], p)
            U = fold(U, alpha, p)
            if i + 1 < c:
                if self.corrupt:
                    U = self.corrupt(i + 1, U)
                self.layers.append(U)
                self.levels.append(layer_levels(U))
        assert self.corrupt or U == [m[0]] * (1 << rho), "U_c is 2^rho equal words"
        self.messages.append(("final", U[0]))
        return rounds, roots, alphas, U[0]

    def query(self, indices):
        """step 9: [(q, column q, column q + L / 2, layers)], a column as RefProver.open_columns gives it, layers[i - 1] =
        ((U_i[j_i], U_i[j_i + M_i / 2]), siblings)"""
        l0 = self.c + self.rho
        half = 1 << (l0 - 1)
        out = []
        for q in indices:
            col_lo, col_hi = self.commitment.open_columns([q, q + half])
            layers = []
            for i in range(1, self.c):
                U, h = self.layers[i], len(self.layers[i]) // 2
                j = q % h
                layers.append(((U[j], U[j + h]), ref.path_of(self.levels[i], j)))
            out.append((q, col_lo, col_hi, layers))
            self.messages.append(("query", (col_lo, col_hi, layers)))
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
            col_lo, col_hi, layers = body
            for _, values, siblings in (col_lo, col_hi):
                total += 8 * len(values) + 32 * len(siblings)
            for pair, siblings in layers:
                total += 8 * len(pair) + 32 * len(siblings)
    return total
