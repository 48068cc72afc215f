"""check_levels: one codeword row of "expander code 1" checked from the codeword alone (tests/expander_ref.py states the code).

Every intermediate of the recursion survives in the codeword: the systematic part of z = Enc_(m/4)(y) is y, so at the level with
m = 2^lm inputs at offset o of the row, y sits at [o + m, o + m + m/4) and must equal A x for the x at [o, o + m); z is
[o + m, o + 3m/2) and v at [o + 3m/2, o + 2m) must equal B z; below the last level the base block must equal K x; and the first
2^c words must be the message.  Nothing is encoded: an output costs its 32 (A) or 16 (B) gathered products, so single outputs of
rows of 2^24 words can be checked.

The maps are linear, so the words may be the canonical values or any fixed nonzero multiple of them - the Montgomery words a
device table holds, as they come: a c R = sum a_i (x_i R) mod p exactly when c = sum a_i x_i.  `message` and `codeword` are lists
or numpy arrays of integers below p."""
import random

import numpy as np

import expander_ref as ref

EDGE = 4          # sampled positions: the first and the last EDGE outputs of a map ..
SAMPLES = 256     # .. and this many random ones


def down_output(p, x, o, lm, q):
    """y[q] of the level with 2^lm inputs at x[o:]"""
    acc = 0
    for t in range(ref.D_A):
        K = ref.key(lm, 0, t)
        for e in range(4 * q, 4 * q + 4):
            acc += ref.coef(K, e, p) * int(x[o + ref.perm(K, lm, e)])
    return acc % p


def up_output(p, x, o, lm, j):
    """v[j] of the level with 2^lm inputs at x[o:]: z is at o + 2^lm"""
    z = o + (1 << lm)
    acc = 0
    for t in range(ref.D_B):
        K = ref.key(lm, 1, t)
        acc += ref.coef(K, j, p) * int(x[z + ref.perm(K, lm - 1, j)])
    return acc % p


def _outputs(count, rng):
    if rng is None or count <= 2 * EDGE + SAMPLES:
        return range(count)
    return sorted(set(range(EDGE)) | set(range(count - EDGE, count)) | {rng.randrange(count) for _ in range(SAMPLES)})


def check_levels(p, message, codeword, c, positions=None):
    """raises AssertionError naming the first place where `codeword` (2^(c+1) words) is not the encoding of `message` (2^c words).
    positions=None: every output of every map; a seed or a random.Random: per level and map the first 4 outputs, the last 4 and
    256 random ones (a map with no more outputs than that: all).  The base block and the systematic part are always whole."""
    m = 1 << c
    assert len(message) == m and len(codeword) == 2 * m, (len(message), len(codeword), c)
    rng = None if positions is None else positions if isinstance(positions, random.Random) else random.Random(positions)
    same = np.array_equal(np.asarray(codeword[:m], dtype=np.uint64), np.asarray(message, dtype=np.uint64))
    assert same, "the systematic part is not the message"
    o, lm = 0, c
    while (1 << lm) > ref.BASE_MAX:
        for q in _outputs(1 << (lm - 2), rng):
            assert int(codeword[o + (1 << lm) + q]) == down_output(p, codeword, o, lm, q), ("down", lm, o, q)
        for j in _outputs(1 << (lm - 1), rng):
            assert int(codeword[o + 3 * (1 << lm) // 2 + j]) == up_output(p, codeword, o, lm, j), ("up", lm, o, j)
        o += 1 << lm
        lm -= 2
    mb = 1 << lm
    x = [int(codeword[o + k]) for k in range(mb)]
    for j in range(mb):
        want = sum(pow(j + k + 1, -1, p) * x[k] for k in range(mb)) % p
        assert int(codeword[o + mb + j]) == want, ("base", lm, o, j)
