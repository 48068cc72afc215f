"""Inputs shared by tests/test_ext_edge_words_cpu.py and tests/test_gpu_ext_edge_words.py: the extension-field sumcheck
(ext_sumprod_pass_kernel, ext_fold_kernel, ext_host_rounds, ext_host_evaluate of kernels/ext_sumprod.hpp) on the words of
tests/wide_words.py in BOTH planes, for every modulus.  Nothing here imports the package or touches a GPU.

All tables and challenges are RAW (Montgomery) words, a challenge a pair (c0, c1) of them; tests/ext_ref.py takes canonical
integers, converted with canon_pairs / canon_list.

The prover's ABI takes base tables only, yet the planes of its first extension table can be chosen word for word: a base table
folded by X = (0, one) is c0[i] = u[2 i], c1[i] = u[2 i + 1] - u[2 i] (ext_fold_base with r0 = 0 multiplies by nothing and with
r1 = one by the Montgomery one), so inject(p, E0, E1) - u[2 i] = E0[i], u[2 i + 1] = E0[i] + E1[i] - under the first challenge X
puts E0 and E1 into the launch of round 1, whose accumulate sees them and whose output the extension-in fold of round 2 reads.

  inject(p, E0, E1)                      the base table above
  cross_planes(p, size, rng, ..)         two planes whose ENTRIES (c0[i], c1[i]) sit on the corners of wide_words.classes_of
  ext_inputs(p, n, T)                    {name: (a tables, b tables, n challenge pairs)} for the names of NAMES (names_of(p))
  ext_reference(p, n, T, name)           the reference transcript of one input, computed once and never changed
  const_transcript(p, w, n, T, e)        the closed form of the transcript over constant planes
  planes_at, plane_classes               the planes the reference's own fold holds at a round, and the classes they meet"""
import functools

import numpy as np

import ext_ref as ref
from layered_edge_cases import MODULI, carry_table
from util import GOLD
from wide_words import classes_of, degenerate_challenges, diff_classes, edge_table, edge_words, octet_table, select_challenges

R64 = 1 << 64
NAMES = ("planes", "planes-deep-even", "planes-deep-odd", "late-x", "carry-base", "carry-planes", "edge", "const")
GOLD_ONLY = ("const-down",)              # a = b = DOWN_WORD in both planes: over Goldilocks alone
DOWN_WORD = 0xFFFF000000000000           # its square is a multiple of 2^96
# the round whose launch receives the chosen planes: the one the coverage is checked at
COVER_ROUND = {"planes": 1, "planes-deep-even": 2, "planes-deep-odd": 2}


def names_of(p):
    return NAMES + (GOLD_ONLY if p == GOLD else ())


def one_of(p):
    return R64 % p


def x_of(p):
    """X itself as a raw pair"""
    return (0, one_of(p))


def canon_list(ws, p):
    rinv = pow(R64, -1, p)
    return [int(x) * rinv % p for x in ws]


def mont_list(xs, p):
    return [int(x) * R64 % p for x in xs]


def canon_pairs(pairs, p):
    return [tuple(canon_list(e, p)) for e in pairs]


def _freeze(arrays):
    for t in arrays:
        t.setflags(write=False)
    return arrays


def inject(p, E0, E1):
    """the base table of 2 len(E0) raw words that X folds into the planes E0, E1: u[2 i] = E0[i], u[2 i + 1] = E0[i] + E1[i] mod p"""
    e0 = np.array([int(x) for x in E0], dtype=object)
    e1 = np.array([int(x) for x in E1], dtype=object)
    u = np.empty(2 * len(e0), dtype=np.uint64)
    u[0::2] = e0.astype(np.uint64)
    u[1::2] = ((e0 + e1) % p).astype(np.uint64)
    return u


def cross_planes(p, size, rng, share=0.5, shift=0):
    """two planes (E0, E1) of `size` >= 4 raw words in which about `share` of the aligned quads of entries (at seeded positions;
    every quad when there are fewer than four) are built from the pairs (lo, hi) of diff_classes(p), taken in turn from a seeded
    start, and the rest are uniform residues.  Built quads alternate between two kinds.
      entry: (E0[i], E1[i]) = (lo, hi) on all four entries - the operand sums x0 + x1, y0 + y1 of ext_accumulate at s = 0, 1 add
             the two components of one entry.
      diff:  entries 4 q + 1 and 4 q + 3 are their left neighbours plus (lo, hi), component by component - the fold's difference
             d = u1 - u0 is then (lo, hi) itself, and ext_mul adds d0 + d1.
    shift = k > 0: as octet_table - the entries with the same k low index bits are, in order, planes built as above"""
    if shift > 0 and size >= 4 << shift:
        E0, E1 = np.empty((size >> shift, 1 << shift), dtype=np.uint64), np.empty((size >> shift, 1 << shift), dtype=np.uint64)
        for low in range(1 << shift):
            E0[:, low], E1[:, low] = cross_planes(p, size >> shift, rng, share)
        return E0.reshape(size), E1.reshape(size)
    pairs = diff_classes(p)
    E0, E1 = rng.integers(0, p, size=size, dtype=np.uint64), rng.integers(0, p, size=size, dtype=np.uint64)
    n_quads = size // 4
    built = range(n_quads) if n_quads < 4 else np.sort(rng.permutation(n_quads)[:max(1, int(round(n_quads * share)))])
    j = m = int(rng.integers(0, len(pairs)))          # one place in the list per kind: each kind walks the whole list
    for k, q in enumerate(built):
        if k % 2 == 0:
            for i in range(4 * q, 4 * q + 4):
                E0[i], E1[i] = pairs[j % len(pairs)]
                j += 1
        else:
            for i in (4 * q, 4 * q + 2):
                lo, hi = pairs[m % len(pairs)]
                E0[i + 1], E1[i + 1] = (int(E0[i]) + lo) % p, (int(E1[i]) + hi) % p
                m += 1
    return E0, E1


def cycle_pairs(p, k):
    """k raw challenge pairs: c0 walks the degenerate cycle of wide_words.degenerate_challenges, c1 the same list one ahead"""
    cyc = degenerate_challenges(p, k + 1)
    return [(cyc[j], cyc[j + 1]) for j in range(k)]


def edge_pairs(p, k, rng):
    e = edge_words(p)
    return [(e[int(rng.integers(0, len(e)))], e[int(rng.integers(0, len(e)))]) for _ in range(k)]


def _aliased(a, b):
    """with three or more pairs, pair 2 reads pair 1's b table as its a table and pair 0's a table as its b table"""
    if len(a) >= 3:
        a[2], b[2] = b[1], a[0]
    return a, b


def _plane_tables(p, half, T, rng, shift):
    """(a, b): T pairs of base tables of 2 * half words - the tables of an even pair inject two independent octet planes each,
    those of an odd pair a cross table each"""
    def table(t):
        if t % 2 == 0:
            return inject(p, octet_table(p, half, rng, shift=shift), octet_table(p, half, rng, shift=shift))
        return inject(p, *cross_planes(p, half, rng, shift=shift))
    return _aliased([table(t) for t in range(T)], [table(t) for t in range(T)])


@functools.lru_cache(maxsize=None)
def ext_inputs(p, n, T):
    """{name: (a tables, b tables, challenges)}: T pairs of base tables of 2^n raw words, n >= 4, and n raw challenge pairs.
    planes            r_0 = X over injected planes: pair 0 two independent octet planes per table, pair 1 cross tables; r_1 and
                      later from edge_words(p) in both components.  The launch of round 1 accumulates the planes, that of round
                      2 differences them.
    planes-deep-even  the same planes with shift = 1, r_0 = X, r_1 = (0, 0): the launch of round 2 hands on the even entries of
    planes-deep-odd   both planes - r_1 = (one, 0): the odd ones, as u0 + (d0, d1) - and accumulates them, that of round 3
                      differences them; then cycle_pairs.
    late-x            octet base tables (shift = 2) under (0, 0), (one, 0), then r_2 = X: the extension-in fold receives a c1 plane
                      of zeros and leaves differences of octet words in it; then cycle_pairs.
    carry-base        layered_edge_cases.carry_table under r_0 = (one, 0): the add(u0, r0 d) of ext_fold_base; then cycle_pairs.
    carry-planes      two carry tables injected, r_0 = X, r_1 = (one, 0): both adds of ext_fold; then cycle_pairs.
    edge              edge tables under challenges whose components are all drawn from edge_words(p).
    const             both planes constant at p - 1 (base words p - 1, p - 2 in turn), ONE array as every a_t and b_t, r_0 = X and
                      then edge words: const_transcript is its whole transcript.
    const-down        (Goldilocks) the same with DOWN_WORD in both planes"""
    assert n >= 4
    size, half = 1 << n, 1 << (n - 1)
    one, X = one_of(p), x_of(p)
    out = {}
    for k, name in enumerate(names_of(p)):
        rng = np.random.default_rng([p % 1000003, n, T, k])
        if name == "planes":
            a, b = _plane_tables(p, half, T, rng, 0)
            ch = [X] + edge_pairs(p, n - 1, rng)
        elif name.startswith("planes-deep"):
            a, b = _plane_tables(p, half, T, rng, 1)
            ch = [X, (0, 0) if name.endswith("even") else (one, 0)] + cycle_pairs(p, n - 2)
        elif name == "late-x":
            a, b = _aliased([octet_table(p, size, rng, shift=2) for _ in range(T)], [octet_table(p, size, rng, shift=2) for _ in range(T)])
            ch = [(r, 0) for r in select_challenges(p, 2)] + [X] + cycle_pairs(p, n - 3)
        elif name == "carry-base":
            a, b = _aliased([carry_table(p, size, rng) for _ in range(T)], [carry_table(p, size, rng) for _ in range(T)])
            ch = [(one, 0)] + cycle_pairs(p, n - 1)
        elif name == "carry-planes":
            a, b = _aliased([inject(p, carry_table(p, half, rng), carry_table(p, half, rng)) for _ in range(T)],
                            [inject(p, carry_table(p, half, rng), carry_table(p, half, rng)) for _ in range(T)])
            ch = [X, (one, 0)] + cycle_pairs(p, n - 2)
        elif name == "edge":
            a, b = _aliased([edge_table(p, size, rng) for _ in range(T)], [edge_table(p, size, rng) for _ in range(T)])
            ch = edge_pairs(p, n, rng)
        else:
            a, b, ch = const_input(p, n, T, name)
        assert len(a) == len(b) == T and len(ch) == n
        _freeze(a + b)
        out[name] = (a, b, [(int(r0), int(r1)) for r0, r1 in ch])
    return out


def const_word(p, name):
    """the raw word both planes of a constant input hold"""
    return {"const": p - 1, "const-down": DOWN_WORD}[name]


@functools.lru_cache(maxsize=None)
def const_input(p, n, T, name):
    """(a tables, b tables, challenges) of the constant inputs, at any n >= 1: ONE array - inject of two planes constant at
    const_word(p, name), written out - as every a_t and b_t; r_0 = X, then seeded edge words"""
    e = const_word(p, name)
    arr = np.empty(1 << n, dtype=np.uint64)
    arr[0::2], arr[1::2] = e, 2 * e % p
    rng = np.random.default_rng([p % 1000003, n, T, len(name)])
    return _freeze([arr]) * T, [arr] * T, [x_of(p)] + edge_pairs(p, n - 1, rng)


@functools.lru_cache(maxsize=None)
def ext_reference(p, n, T, name):
    """(a tables, b tables, canonical challenges, tests/ext_ref.py's transcript (canonical)) of one input: computed once, shared"""
    a, b, ch = ext_inputs(p, n, T)[name]
    cc = canon_pairs(ch, p)
    canon = {id(t): canon_list(t, p) for t in a + b}
    out = ref.sumcheck([canon[id(t)] for t in a], [canon[id(t)] for t in b], p, ref.nonresidue(p), lambda j, msg: cc[j])
    return a, b, cc, out


def const_transcript(p, w, n, T, e):
    """(c1, rounds, finals_a, finals_b), canonical, of the sumcheck over T pairs (a_t, b_t) that are all ONE base table of 2^n words
    whose planes under r_0 = X are constant at e = (e0, e1) in K (canonical): base words e0, e0 + e1 in turn.  Constant planes stay
    constant under every fold, u0 + r (u1 - u0) = e, and a(2) = 2 e - e = e, so every value of a round over 2^m entries, m < n, is
    T 2^(m-1) e^2; round 0 is over the base words: T 2^(n-1) u^2 for u = e0, e0 + e1, 2 (e0 + e1) - e0.  Needs r_0 = X; the later
    challenges do not enter"""
    e = (int(e[0]) % p, int(e[1]) % p)
    u0, u1 = e[0], (e[0] + e[1]) % p
    rounds = [[(T * 2**(n - 1) * u * u % p, 0) for u in (u0, u1, (2 * u1 - u0) % p)]]
    sq = ref.kmul(e, e, p, w)
    for j in range(1, n):
        k = T * 2**(n - j - 1)
        rounds.append([(k * sq[0] % p, k * sq[1] % p)] * 3)
    return ref.kadd(rounds[0][0], rounds[0][1], p), rounds, [e] * T, [e] * T


def planes_at(p, w, table, challenges, rnd):
    """the raw planes (c0, c1) of one raw base table after the reference's own fold by challenges[0 .. rnd): what the launch of
    round `rnd` reads (rnd = 1: what it forms and accumulates)"""
    u = ref.lift(canon_list(table, p))
    for r in canon_pairs(challenges[:rnd], p):
        u = ref.fold(u, r, p, w)
    return mont_list([x[0] for x in u], p), mont_list([x[1] for x in u], p)


def plane_classes(p, w, tables, challenges, rnd):
    """{"c0": .., "c1": .., "entry": ..}: the classes of wide_words.classes_of met in the planes of `tables` at round `rnd` (planes_at)
    by (c0[2 i], c0[2 i + 1]), by (c1[2 i], c1[2 i + 1]) - the neighbours a fold differences and a(2) is formed from - and by
    the two components (c0[i], c1[i]) of one entry"""
    out = {"c0": set(), "c1": set(), "entry": set()}
    for t in tables:
        c0, c1 = planes_at(p, w, t, challenges, rnd)
        for i in range(len(c0) // 2):
            out["c0"] |= classes_of(p, c0[2 * i], c0[2 * i + 1])
            out["c1"] |= classes_of(p, c1[2 * i], c1[2 * i + 1])
        for x, y in zip(c0, c1):
            out["entry"] |= classes_of(p, x, y)
    return out


def diff_sum_classes(p, w, tables, challenges, rnd):
    """the classes met by the two components (d0, d1) of the differences u[2 i + 1] - u[2 i] of the planes at round `rnd`: the
    operands of ext_mul's y0 + y1 in the fold of that round's planes"""
    out = set()
    for t in tables:
        c0, c1 = planes_at(p, w, t, challenges, rnd)
        for i in range(len(c0) // 2):
            out |= classes_of(p, (c0[2 * i + 1] - c0[2 * i]) % p, (c1[2 * i + 1] - c1[2 * i]) % p)
    return out
