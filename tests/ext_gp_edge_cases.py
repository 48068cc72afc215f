"""Inputs shared by tests/test_ext_gp_edge_words_cpu.py and tests/test_gpu_ext_gp_edge_words.py: the grand product over
K = F_p[X] / (X^2 - w) (ext_gp_tree_kernel, ext_gp_tree_tail_kernel, ext_gp_pass_kernel, ext_eq_table_kernel of
kernels/ext_grand_product.hpp and their host twins) on the words of tests/wide_words.py in BOTH planes, for every modulus.  Nothing here
imports the package or touches a GPU.

All tables, alpha, beta and challenges are RAW (Montgomery) words, an element of K a pair (c0, c1) of them; tests/ext_gp_ref.py takes
canonical integers (ext_edge_cases.canon_list / canon_pairs).  one = 2^64 mod p is the Montgomery one, mm(a, b) = a b / 2^64 the
Montgomery product.

The ABI takes a base table t and the leaf map alpha, beta only, yet chosen words reach the planes:

  the leaves     alpha = (one, +-one), beta = (0, d): the raw planes of V_n are c0 = t, c1 = d +- t; a leaf is zero only where t = 0 and
                 d = 0, so with d != 0 an octet table keeps its zero words.  leaf_maps(p) is a greedy choice among these maps under which
                 the two components of the entries (c0[i], c1[i]) meet every class of wide_words.classes_present(p).  Mirrored,
                 alpha = (one, one), beta = (d, 0): c1 = t.
  layer n - q    beta = 1 - alpha c for a base word c and the upper 1 - 2^-q of t constant at c: every leaf there is 1 and
                 V_(n-q)[x] = 1 + alpha (t[x] - c), x < 2^(n-q), raw planes (one + mm(a0, s), mm(a1, s)) with s = t - c.
                 alpha = (0, one) puts s word for word into c1; alpha = (one, one) with s = u - one puts u into c0; and one entry
                 (lo, hi) is reached with a0 = (lo - one) / s, a1 = hi / s for a fixed s != 0 (solve_alpha).
  the eq table   E of layer k is built from the challenges of layer k - 1: the layer before the one whose launches receive the chosen
                 words draws both components of every challenge from seeded residues outside {0, one}, so E has no zero entry there.

  names_of(p), gp_input(p, n, name)      the named inputs, each a GpInput
  entry_inputs(p)                        `planes-entry`: one proof at n = 5 per pair of diff_classes(p)
  gp_reference(p, n, name)               the reference transcript of one input, computed once and never changed
  tables_at, table_classes               E, L, R as the reference's own tree and fold hold them at a launch, and the classes they meet
  const_transcript                       the closed form of the transcript over a constant table"""
import collections
import functools

import numpy as np

import ext_gp_ref as ref
import ext_ref as xref
from ext_edge_cases import canon_list, canon_pairs, cycle_pairs, edge_pairs, mont_list
from layered_edge_cases import BLOCK, MODULI, WAVE, carry_table   # noqa: F401  (MODULI, BLOCK, WAVE: for the tests)
from wide_words import classes_of, classes_present, diff_classes, edge_table, edge_words, octet_table

R64 = 1 << 64
TAIL_LOG = 11            # kExtGpTailLog: the one-block tail of the tree over K
ENTRY_N = 5              # the size of the planes-entry proofs

# cover = (layer, round): the launch of that round of that layer is the one the chosen words are meant for - it reads the tables
# E, L, R of the layer folded by the challenges of the rounds before it.  plane: "c0", "c1", "both", "entry" or None - where the
# chosen words are.  depth: the layer n - depth holds them (0: the leaves).  injected: how many low words of t carry them.
GpInput = collections.namedtuple("GpInput", "table alpha beta challenges cover plane depth injected")


def one_of(p):
    return R64 % p


def mm(a, b, p):
    """the Montgomery product of two raw words"""
    return int(a) * int(b) * pow(R64, -1, p) % p


def _freeze(t):
    t = np.asarray(t, dtype=np.uint64)
    t.setflags(write=False)
    return t


def _words(xs):
    return np.array([int(x) for x in xs], dtype=object).astype(np.uint64)


# ---- the leaf maps -------------------------------------------------------------------------------------------------------------

def shifts(p):
    one = one_of(p)
    out = []
    for d in (1, 2, p - 1, p - 2, one, p - one, (p + 1) // 2, (p - 2**32) % p, 2**32 % p, 2**64 - p):
        if 0 < d < p and d not in out:
            out.append(d)
    return out


def entry_classes(p, table, sign, d):
    """the classes the two components (t, d +- t) of the leaves of `table` meet under alpha = (one, sign one), beta = (0, d)"""
    out = set()
    for x in table:
        out |= classes_of(p, int(x), (d + sign * int(x)) % p)
    return out


@functools.lru_cache(maxsize=None)
def leaf_maps(p):
    """[(sign, d)]: greedily, the map that meets most of the classes still missing over octet_table(p, 2048, default_rng(1)), until
    every class of classes_present(p) is met across the components (or no map adds one)"""
    probe = octet_table(p, 2048, np.random.default_rng(1))
    met = {(s, d): entry_classes(p, probe, s, d) for s in (1, -1) for d in shifts(p)}
    missing, out = set(classes_present(p)), []
    while missing:
        best = max(met, key=lambda k: len(met[k] & missing))
        if not met[best] & missing:
            break
        out.append(best)
        missing -= met[best]
    return out


# ---- the challenges --------------------------------------------------------------------------------------------------------------

def _residue_pair(p, rng):
    """both components seeded residues outside {0, one}"""
    out = []
    while len(out) < 2:
        x = int(rng.integers(2, p, dtype=np.uint64))
        if x != one_of(p):
            out.append(x)
    return tuple(out)


def challenge_index(k, j):
    """where round j of layer k (j = k: its rho) stands in protocol order"""
    return k * (k + 1) // 2 + j


def _challenges(p, n, rng, special):
    """n (n + 1) / 2 raw pairs in protocol order.  special = {layer: its first challenges}: such a layer goes on with the degenerate
    cycle (six pairs) and then with pairs of edge words; every other layer draws seeded residues outside {0, one}"""
    out = []
    for k in range(n):
        if k in special:
            got = [tuple(c) for c in special[k]][:k + 1]
            got += cycle_pairs(p, min(6, k + 1 - len(got)))
            got += edge_pairs(p, k + 1 - len(got), rng)
        else:
            got = [_residue_pair(p, rng) for _ in range(k + 1)]
        out += [(int(a), int(b)) for a, b in got]
    assert len(out) == ref.n_challenges(n)
    return out


# ---- the injection into layer n - depth ----------------------------------------------------------------------------------------

def base_word(p):
    """c: the word the upper part of an injected table is constant at"""
    return 0x0123456789ABCDEF % (p - 1) + 1


def unit_map(p, alpha):
    """beta = 1 - alpha c"""
    c = base_word(p)
    return ((one_of(p) - mm(alpha[0], c, p)) % p, -mm(alpha[1], c, p) % p)


def inject(p, n, depth, u, plane):
    """(t, alpha, beta): the table of 2^n words whose layer n - depth holds the 2^(n-depth) raw words u in `plane` (c1: beside
    c0 = one; c0: beside c1 = u - one)"""
    one, c = one_of(p), base_word(p)
    assert len(u) == 1 << (n - depth) and depth >= 1
    t = np.full(1 << n, c, dtype=np.uint64)
    if plane == "c1":
        alpha = (0, one)
        t[:len(u)] = _words((int(x) + c) % p for x in u)
    else:
        alpha = (one, one)
        t[:len(u)] = _words((int(x) - one + c) % p for x in u)
    return t, alpha, unit_map(p, alpha)


def solve_alpha(p, lo, hi, s):
    """alpha with (one + mm(a0, s), mm(a1, s)) = (lo, hi)"""
    k = R64 * pow(s, -1, p) % p
    return ((lo - one_of(p)) * k % p, hi * k % p)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------

FIXED = ("leaf-c1", "leaf-perm", "leaf-deep-even", "leaf-deep-odd", "leaf-carry", "planes-c0", "planes-c1", "planes2-c0", "planes2-c1",
         "planes-carry-c0", "planes-carry-c1", "edge", "const")
TREE_ONLY = ("planes3-c0", "planes3-c1")      # the seven-eighths-unit table: too large for a reference transcript, its tree is compared


def leaf_entry_names(p):
    return tuple("leaf-entry-%d" % i for i in range(len(leaf_maps(p))))


def names_of(p):
    return leaf_entry_names(p) + FIXED


def _seed(p, n, name):
    return [p % 1000003, n] + [ord(c) for c in name]


def _zero_leaf(p, t, alpha, beta):
    return any((beta[0] + mm(alpha[0], x, p)) % p == 0 and (beta[1] + mm(alpha[1], x, p)) % p == 0 for x in set(int(x) for x in t))


@functools.lru_cache(maxsize=None)
def gp_input(p, n, name):
    """One named input at n >= 4 variables.
    leaf-entry-i      an octet table under leaf_maps(p)[i]; layer n - 1 takes the degenerate cycle, then edge pairs
    leaf-c1           the mirrored map alpha = (one, one), beta = (1, 0): c1 = t
    leaf-perm         the permutation check's map alpha = (p - one, 0), beta = gamma, gamma's components edge words
    leaf-deep-even    octet_table(shift = 1) under alpha = (one, one), beta = (0, 1); round 0 of layer n - 1 takes (0, 0) - odd:
    leaf-deep-odd     (one, 0) - and the leaf-in fold hands the even or the odd leaves to the accumulate of round 1 and to round 2
    leaf-carry        carry_table under alpha = (one, one), beta = 0; round 0 of layer n - 1 takes (one, 0): ext_gp_fold_leaf leaves
                      sums inside [p, 2^64) in both planes and the difference of the next round borrows against them
    planes-c0, -c1    an octet table in one plane of layer n - 1 (inject, depth 1); layer n - 2 reads it
    planes2-c0, -c1   the same in layer n - 2 (depth 2); layer n - 3 reads it.  planes3-*: depth 3, for the tree alone
    planes-carry-c*   carry_table in one plane of layer n - 1; round 0 of layer n - 2 takes (one, 0): the planes-in ext_fold
    edge              an edge table; every component of alpha, beta and every challenge from edge_words(p)
    const             every word p - 1 under alpha = (one, one), beta = 0: both planes of the leaves constant at p - 1"""
    assert n >= 4
    size, one = 1 << n, one_of(p)
    rng = np.random.default_rng(_seed(p, n, name))
    top = n - 1
    if name.startswith("leaf-entry-"):
        sign, d = leaf_maps(p)[int(name.rsplit("-", 1)[1])]
        out = (octet_table(p, size, rng), (one, one if sign > 0 else p - one), (0, d), _challenges(p, n, rng, {top: []}), (top, 0), "c0", 0)
    elif name == "leaf-c1":
        out = (octet_table(p, size, rng), (one, one), (1, 0), _challenges(p, n, rng, {top: []}), (top, 0), "c1", 0)
    elif name == "leaf-perm":
        out = (octet_table(p, size, rng), (p - one, 0), (p - 2, (p - 1) // 2), _challenges(p, n, rng, {top: []}), (top, 0), None, 0)
    elif name.startswith("leaf-deep"):
        r0 = (0, 0) if name.endswith("even") else (one, 0)
        out = (octet_table(p, size, rng, shift=1), (one, one), (0, 1), _challenges(p, n, rng, {top: [r0]}), (top, 1), "c0", 0)
    elif name == "leaf-carry":
        out = (carry_table(p, size, rng), (one, one), (0, 0), _challenges(p, n, rng, {top: [(one, 0)]}), (top, 1), "both", 0)
    elif name.startswith("planes"):
        plane = name[-2:]
        depth = 1 if name.startswith(("planes-c", "planes-carry")) else int(name[6])
        reader = n - depth - 1
        if "carry" in name:
            u, first, cover = carry_table(p, size >> depth, rng), [(one, 0)], (reader, 1)
        else:
            u, first, cover = octet_table(p, size >> depth, rng), [], (reader, 0)
        t, alpha, beta = inject(p, n, depth, u, plane)
        out = (t, alpha, beta, _challenges(p, n, rng, {reader: first}), cover, plane, depth)
    elif name == "edge":
        e = edge_words(p)
        for _ in range(64):
            t = edge_table(p, size, rng)
            alpha, beta = [tuple(e[int(i)] for i in rng.integers(0, len(e), size=2)) for _ in range(2)]
            if alpha != (0, 0) and not _zero_leaf(p, t, alpha, beta):
                break
        else:
            raise AssertionError("no edge input without a zero leaf")
        out = (t, alpha, beta, edge_pairs(p, ref.n_challenges(n), rng), (top, 0), None, 0)
    elif name == "const":
        return const_input(p, n)
    else:
        raise KeyError(name)
    return GpInput(_freeze(out[0]), *out[1:], injected=size >> out[6])


@functools.lru_cache(maxsize=None)
def const_input(p, n):
    """the constant input at any n >= 1: seeded residues as challenges, pairs of edge words in the last layer"""
    rng = np.random.default_rng(_seed(p, n, "const"))
    return GpInput(_freeze(np.full(1 << n, p - 1, dtype=np.uint64)), (one_of(p), one_of(p)), (0, 0), _challenges(p, n, rng, {n - 1: []}),
                   (n - 1, 0), "both", 0, 1 << n)


def entry_pairs(p):
    """the pairs of diff_classes(p) but (0, 0): as an entry that pair is the zero of K, which no tree with a product other than 0
    holds; its class, diff_zero, is met by the pair (x, x)"""
    return [pair for pair in diff_classes(p) if pair != (0, 0)]


@functools.lru_cache(maxsize=None)
def entry_inputs(p):
    """`planes-entry`: one input at n = ENTRY_N per pair (lo, hi) of entry_pairs(p).  The even entries of layer n - 1 are (lo, hi)
    - t = s + c there with s = 3 and alpha solved for the pair - and the odd ones images of seeded residues; layer n - 2 reads it"""
    n, s, c = ENTRY_N, 3, base_word(p)
    out = []
    for k, (lo, hi) in enumerate(entry_pairs(p)):
        rng = np.random.default_rng(_seed(p, n, "planes-entry") + [k])
        alpha = solve_alpha(p, lo, hi, s)
        assert alpha != (0, 0)
        beta = unit_map(p, alpha)
        for _ in range(64):
            t = np.full(1 << n, c, dtype=np.uint64)
            t[:1 << (n - 1)] = rng.integers(1, p, size=1 << (n - 1), dtype=np.uint64)
            t[0:1 << (n - 1):2] = (s + c) % p
            if not _zero_leaf(p, t, alpha, beta):
                break
        else:
            raise AssertionError("no table without a zero leaf", lo, hi)
        out.append(GpInput(_freeze(t), alpha, beta, _challenges(p, n, rng, {n - 2: []}), (n - 2, 0), "entry", 1, 1 << (n - 1)))
    return out


# ---- the references, one per (modulus, size, input): computed once, shared, never changed ----------------------------------------

Reference = collections.namedtuple("Reference", "input table alpha beta challenges out")


def _reference(p, inp, prove=True):
    """the canonical table, alpha, beta and challenges of an input and tests/ext_gp_ref.py's transcript under them"""
    t, alpha, beta = canon_list(inp.table, p), tuple(canon_list(inp.alpha, p)), tuple(canon_list(inp.beta, p))
    cc = canon_pairs(inp.challenges, p)
    out = ref.prove(t, alpha, beta, p, xref.nonresidue(p), lambda k, j, msg, it=iter(cc): next(it)) if prove else None
    return Reference(inp, t, alpha, beta, cc, out)


@functools.lru_cache(maxsize=None)
def gp_reference(p, n, name):
    return _reference(p, gp_input(p, n, name))


@functools.lru_cache(maxsize=None)
def entry_references(p):
    return [_reference(p, inp) for inp in entry_inputs(p)]


@functools.lru_cache(maxsize=None)
def tree_reference(p, n, name):
    """(input, canonical alpha, beta, the reference's tree layers [V_0 .. V_n]) - no transcript"""
    r = _reference(p, gp_input(p, n, name), prove=False)
    w = xref.nonresidue(p)
    return r.input, r.alpha, r.beta, ref.tree(ref.leaves(r.table, r.alpha, r.beta, p, w), p, w)


# ---- what a launch reads: from the reference's own tree and fold ---------------------------------------------------------------

def tables_at(p, inp, layer=None, rnd=None):
    """{"E": (c0, c1), "L": .., "R": ..}: the raw planes of the three tables of `layer` after the reference's fold by the challenges of
    its rounds before `rnd` (default: the input's cover): what the launch of that round accumulates"""
    w = xref.nonresidue(p)
    layer, rnd = inp.cover if layer is None else (layer, rnd)
    cc = canon_pairs(inp.challenges, p)
    V = ref.tree(ref.leaves(canon_list(inp.table, p), tuple(canon_list(inp.alpha, p)), tuple(canon_list(inp.beta, p)), p, w), p, w)
    z = cc[challenge_index(layer - 1, 0):challenge_index(layer - 1, layer)] if layer else []
    half = 1 << layer
    tabs = {"E": xref.eq_weights(z, p, w), "L": V[layer + 1][:half], "R": V[layer + 1][half:]}
    for r in cc[challenge_index(layer, 0):challenge_index(layer, rnd)]:
        tabs = {k: xref.fold(u, r, p, w) for k, u in tabs.items()}
    return {k: (mont_list([x[0] for x in u], p), mont_list([x[1] for x in u], p)) for k, u in tabs.items()}


def table_classes(p, planes):
    """{"c0": .., "c1": .., "entry": ..}: the classes met by the neighbours (2 i, 2 i + 1) of each plane and by the two components of
    an entry"""
    c0, c1 = planes
    out = {"c0": set(), "c1": set(), "entry": set()}
    for i in range(len(c0) // 2):
        out["c0"] |= classes_of(p, c0[2 * i], c0[2 * i + 1])
        out["c1"] |= classes_of(p, c1[2 * i], c1[2 * i + 1])
    for x, y in zip(c0, c1):
        out["entry"] |= classes_of(p, x, y)
    return out


# ---- the closed form over a constant table ---------------------------------------------------------------------------------------

def const_transcript(p, w, n, v, cc):
    """the prove() dict, canonical, of a table whose leaves are all v in K under the canonical challenges cc (protocol order).  Every
    V_k is constant at v_k = v^(2^(n-k)), so L = R = v_(k+1) stay constant under every fold: the finals are l = r' = v_(k+1), and with
    E folded by r_0 .. r_(j-1) the message of round j is H_j(t) = v_(k+1)^2 P_j ((1 - z_j) + t (2 z_j - 1)), P_j = prod_(i<j) eq1(z_i, r_i),
    eq1(z, r) = (1 - z)(1 - r) + z r: the sum of eq over the variables still free is 1"""
    kmul, kadd, ksub = xref.kmul, xref.kadd, xref.ksub
    vs = [v]
    for _ in range(n):
        vs.insert(0, kmul(vs[0], vs[0], p, w))
    z, claim, rounds, finals = [], vs[0], [], []
    for k in range(n):
        at = challenge_index(k, 0)
        rs, rho = cc[at:at + k], cc[at + k]
        sq, P, msgs = kmul(vs[k + 1], vs[k + 1], p, w), (1, 0), []
        for j in range(k):
            lo, slope = ksub((1, 0), z[j], p), ksub(kadd(z[j], z[j], p), (1, 0), p)
            msgs.append([kmul(kmul(sq, P, p, w), kadd(lo, kmul((t, 0), slope, p, w), p), p, w) for t in range(4)])
            P = kmul(P, kadd(kmul(lo, ksub((1, 0), rs[j], p), p, w), kmul(z[j], rs[j], p, w), p), p, w)
        rounds.append(msgs)
        finals.append((vs[k + 1], vs[k + 1]))
        claim = vs[k + 1]                       # l + rho (r' - l)
        z = list(rs) + [rho]
    return {"product": vs[0], "rounds": rounds, "finals": finals, "challenges": list(cc), "point": z, "claim": claim}
