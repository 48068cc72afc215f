"""What tests/test_gpu_ligero_fold_limits.py and tests/test_ligero_fold_limits_cpu.py share: the fields, the four shapes whose
schedules launch every rs_fold_kernel<F, A, AN>, and the worst-case inputs of a folded opening - all RAW (Montgomery) words,
as the device takes them; a reference gets ligero_ref.canon of them.  Nothing here imports the package."""
import random

import numpy as np

import ligero_ref as ref
import wide_words

GOLD, BABYBEAR, P64S18 = ref.GOLD, ref.BABYBEAR, ref.P64S18
FIELDS = [GOLD, BABYBEAR] + ref.WIDE_NTT
IDS = {GOLD: "gold", BABYBEAR: "babybear", ref.P64S18: "p64s18", ref.P64S34: "p64s34", ref.P63S16: "p63s16", ref.P32HI: "p32hi",
       ref.P32LO: "p32lo"}
# (n, c, rho, schedule): l0 = 8; l0 = 11, the last length on the single table, rho = 2; l0 = 12, the first on the twist tables;
# l0 = 13, rho = 2.  Every stage after the first folds a layer of 2^(l0 - i_s) words with the tables of length 2^l0 (shift = i_s)
SHAPES = [(9, 7, 1, (2, 2, 3)), (11, 9, 2, (2, 3, 1, 1, 2)), (12, 11, 1, (3, 3, 2, 2, 1)), (13, 11, 2, (1, 3, 1, 2, 2, 2))]
BINARY_SHAPES = [SHAPES[0], SHAPES[2]]          # also opened without a schedule: rs_fold_kernel<F, 1, 1 / 0>, recorded as rs_fold
VERIFIER_SHAPES = [SHAPES[1], SHAPES[2]]        # l0 = 11 and l0 = 12
RANDOM_SHAPE = SHAPES[2]
ALL_PAIRS = {(a, an) for a in (1, 2, 3) for an in (0, 1, 2, 3)}
FOLD_LOGS = (4, 9, 11, 12, 13)                  # sc_rs_fold / sc_rs_fold_many alone: one block, several, and around the table switch


def fid(v):
    return "".join(str(a) for a in v) if isinstance(v, tuple) else IDS.get(v, str(v))


def launched_pairs(arities):
    """(A, AN) of every rs_fold_many launch of an opening under the schedule: AN is the next stage's arity, 0 after the last"""
    return [(a, arities[s + 1] if s + 1 < len(arities) else 0) for s, a in enumerate(arities)]


def edge_inputs(p, n, c, rho, arities):
    """the worst-case inputs of the opening of SHAPES[k]: the table puts the pairs of wide_words.diff_classes on (k, k + C/2) of
    its rows, the point and gamma are edge words, the alphas wide_words.degenerate_challenges.  By shape: gamma all zero at the
    second; every coordinate of the point one of the words 0, 1, p - 1 at the third; beta = p - 1 at the first two, 0 at the others"""
    k = SHAPES.index((n, c, rho, arities))
    rng = np.random.default_rng([p, n, c])
    rows = 1 << (n - c)
    table = wide_words.half_stride_table(p, rows, c, rng)
    point = wide_words.edge_table(p, n, rng, share=1.0)
    gamma = wide_words.edge_table(p, rows, rng)
    if k == 1:
        gamma = np.zeros(rows, dtype=np.uint64)
    if k == 2:
        point = np.array([(0, 1, p - 1)[int(x)] for x in rng.integers(0, 3, size=n)], dtype=np.uint64)
    return {"table": table, "point": [int(x) for x in point], "gamma": [int(x) for x in gamma], "beta": p - 1 if k < 2 else 0,
            "alphas": wide_words.degenerate_challenges(p, c)}


def random_inputs(p, n, c, rho, arities):
    """uniform residues for everything"""
    rng = np.random.default_rng([p, n, c, 1])
    draw = lambda size: rng.integers(0, p, size=size, dtype=np.uint64)      # noqa: E731
    return {"table": draw(1 << n), "point": [int(x) for x in draw(n)], "gamma": [int(x) for x in draw(1 << (n - c))],
            "beta": int(draw(1)[0]), "alphas": [int(x) for x in draw(c)]}


def queries_of(c, rho, arities, seed, count=4):
    """both ends of [0, L / 2^a_0) and `count` seeded indices"""
    top = 1 << (c + rho - (arities[0] if arities else 1))
    rng = random.Random(seed)
    return [0, top - 1] + [rng.randrange(top) for _ in range(count)]


def fold_table(p, log_m):
    """one codeword-length row of raw words with the pairs of diff_classes(p) on (j, j + M/2), the pairs a fold takes the sum and
    the difference of"""
    return wide_words.half_stride_table(p, 1, log_m, np.random.default_rng([p, log_m, 2]))


def fold_alpha_sets(p, log_m, count):
    """raw challenge words for `count` folds in one launch: two sets off wide_words.degenerate_challenges - between them 0, the
    field's one, p - 1, 1, p - 2 and (p + 1) / 2 - then one of uniform residues"""
    cyc = wide_words.degenerate_challenges(p, 6)
    rng = random.Random("%d %d %d" % (p, log_m, count))
    return [cyc[:count], cyc[3:3 + count], [rng.randrange(p) for _ in range(count)]]


class ScriptedDraws:
    """in place of a random.Random: randrange(p) hands out the given canonical values in order - what a host verifier then
    draws as gamma, beta and the alphas - and every other range (the query indices) comes from a seeded generator"""

    def __init__(self, p, values, seed):
        self.p, self.values, self.rng = p, [int(x) for x in values], random.Random(seed)

    def randrange(self, *args):
        if args == (self.p,) and self.values:
            return self.values.pop(0)
        return self.rng.randrange(*args)
