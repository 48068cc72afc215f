"""Words and moduli for testing the generic field at full word width (tests/test_oracle_wide_moduli.py,
tests/test_gpu_wide_moduli.py, tests/test_gpu_ligero_wide.py)."""
import numpy as np

from util import pid

# full-width generic moduli (all prime): p > 2^63 at the top and just above 2^63, a Mersenne prime, and two moduli around
# 2^32 - one whose high half is 0 or 1, one whose residues fit 32 bits while their products fill 64
WIDE = [2**64 - 59, 2**63 + 29, 2**61 - 1, 2**32 + 15, 2**32 - 5]
_WIDE_IDS = {2**64 - 59: "p64m59", 2**63 + 29: "p63p29", 2**61 - 1: "p61m1", 2**32 + 15: "p32p15", 2**32 - 5: "p32m5"}


def wid(p):
    return _WIDE_IDS.get(p) or pid(p)


def edge_words(p):
    """the raw (Montgomery) words at which the carries of the field arithmetic happen, each below p: 0, 1, p-1, p-2, (p-1)/2,
    R mod p (the Montgomery one), 2^32-1, 2^32, 2^32+1, 2^63 and 0xFFFFFFFF00000000"""
    cand = [0, 1, p - 1, p - 2, (p - 1) // 2, 2**64 % p, 2**32 - 1, 2**32, 2**32 + 1, 2**63, 0xFFFFFFFF00000000]
    out = []
    for w in cand:
        if w < p and w not in out:
            out.append(w)
    return out


def edge_table(p, size, rng, share=0.5):
    """`size` raw words: edge words in about `share` of the entries (at seeded positions), uniform residues in the rest"""
    e = np.array(edge_words(p), dtype=np.uint64)
    t = rng.integers(0, p, size=size, dtype=np.uint64)
    pick = rng.random(size) < share
    t[pick] = e[rng.integers(0, e.size, size=int(pick.sum()))]
    return t


# ---- words chosen by the DIFFERENCE and the SUM of neighbouring entries (tests/test_gpu_pass_edge_words.py) ---------------
# The passes take hi - lo of table entries at strides 1, 2 and 4 (extend_quads, the three-round extension, the one-challenge
# fold) and hand on lo + r (hi - lo); the branches of the device's sub / sub4 / sub2 / add that correct a borrow or a carry
# depend on where that difference or sum lands, not on the words themselves.

_M64 = 2**64 - 1
_LOW = 0xFFFFFFFF

DIFF_CLASSES = ("no_borrow", "borrow_low_ones", "borrow_low_zero", "diff_zero", "diff_minus_one",
                "sum_p", "sum_p_plus_1", "sum_2_64", "sum_p_to_2_64", "sum_carry")


def classes_of(p, lo, hi):
    """the corners the pair of raw words (lo, hi) sits on, as a set of names from DIFF_CLASSES.
    Of hi - lo mod 2^64: no borrow; a borrow with low limb 0xFFFFFFFF (GoldilocksMont::sub4 / sub2: d0 += bw carries, so
    d1 stays); a borrow with low limb 0; difference 0; difference p - 1.
    Of hi + lo: equal to p; to p + 1; to 2^64 (the carry goes out and leaves 0); inside (p + 1, 2^64) (GoldilocksMont::add:
    only the second carry is set); above 2^64 (MontGeneric::add: the carry out of a + b)"""
    lo, hi = int(lo), int(hi)
    d, s = (hi - lo) & _M64, hi + lo
    out = set()
    if hi > lo:
        out.add("no_borrow")
    if hi < lo and d & _LOW == _LOW:
        out.add("borrow_low_ones")
    if hi < lo and d & _LOW == 0:
        out.add("borrow_low_zero")
    if hi == lo:
        out.add("diff_zero")
    if (hi - lo) % p == p - 1:
        out.add("diff_minus_one")
    if s == p:
        out.add("sum_p")
    if s == p + 1:
        out.add("sum_p_plus_1")
    if s == 2**64:
        out.add("sum_2_64")
    if p + 1 < s < 2**64:
        out.add("sum_p_to_2_64")
    if s > 2**64:
        out.add("sum_carry")
    return out


def diff_classes(p):
    """raw-word pairs (lo, hi), both below p, whose difference hi - lo or sum hi + lo lands on each corner of classes_of that
    exists for this p (a pair is listed where both its words are below p, each pair once)"""
    r = 2**64 % p
    x = min(p - 2, 0x123456789ABCDEF0 % p)
    top = 0xFFFFFFFF00000000                 # at most 20 pairs: 15 built octets of octet_table carry them all
    cand = [
        # hi - lo: no borrow
        (0, 1), (5, 2**32 + 6),
        # a borrow that leaves the low limb 0xFFFFFFFF: lo - hi = 1 mod 2^32
        (x + 1, x), (1, 0), (2**32 + 6, 5), (2**63, 2**63 - 1),
        # a borrow that leaves the low limb 0: lo - hi a multiple of 2^32
        (2**32, 0), (2**63 + 7, 7),
        # difference 0, difference p - 1
        (0, 0), (x, x), (0, p - 1),
        # hi + lo = p, = p + 1
        (1, p - 1), ((p - 1) // 2, (p + 1) // 2), (r, p - r), (2, p - 1),
        # hi + lo = 2^64, inside (p + 1, 2^64), above 2^64
        (2**63, 2**63), (2**64 - (p - 1), p - 1), (top, 2**32 - 1), (p - 1, min(p - 1, _M64 - (p - 1))), (p - 2, p - 1),
    ]
    out = []
    for lo, hi in cand:
        if 0 <= lo < p and 0 <= hi < p and (lo, hi) not in out:
            out.append((lo, hi))
    return out


def classes_present(p):
    """the classes that exist for p: those at least one pair of diff_classes(p) sits on"""
    out = set()
    for lo, hi in diff_classes(p):
        out |= classes_of(p, lo, hi)
    return out


def octet_table(p, size, rng, share=0.5, shift=0):
    """`size` raw words in which about `share` of the aligned groups of eight entries (at seeded positions; every group when
    there are fewer than four) are built from the pairs of diff_classes(p) and the rest are uniform residues.  The k-th built
    octet takes one stride s of 1, 2, 4 (k mod 3) and puts four pairs, taken from the list in turn, on its four (i, i + s):
    t[i] = lo, t[i + s] = hi - so every 3 * ceil(len(pairs) / 4) built octets in a row carry every pair at every stride, and
    the differences t[i + s] - t[i] that extend_quads and the three-round extension take meet every class there is.
    Tables below eight entries are filled pair by pair at stride 1.
    shift = k > 0 moves the octets up by k index bits: the entries with the same k low index bits l are, in order, a table
    built as above (one per l), so the strides of the patterns are 2^k, 2^(k+1), 2^(k+2) and a fold by k challenges that are
    each 0 or one (it keeps the entries with one value of l) leaves such a table: the patterns then reach the extension step
    of a pass with k pending challenges.  Needs size >= 2^(k+3), else the table is the unshifted one."""
    if shift > 0 and size >= 8 << shift:
        t = np.empty((size >> (3 + shift), 8, 1 << shift), dtype=np.uint64)
        for low in range(1 << shift):
            t[:, :, low] = octet_table(p, size >> shift, rng, share).reshape(-1, 8)
        return t.reshape(size)
    pairs = diff_classes(p)
    t = rng.integers(0, p, size=size, dtype=np.uint64)
    if size < 8:
        for i in range(size // 2):
            t[2 * i], t[2 * i + 1] = pairs[int(rng.integers(0, len(pairs)))]
        if size == 1:
            t[0] = pairs[int(rng.integers(0, len(pairs)))][1]
        return t
    n_oct = size // 8
    n_built = n_oct if n_oct < 4 else max(1, int(round(n_oct * share)))
    built = np.sort(rng.permutation(n_oct)[:n_built])
    start = int(rng.integers(0, len(pairs)))
    for k, o in enumerate(built):
        s = (1, 2, 4)[k % 3]
        lows = [i for i in range(8) if not i & s]
        for j, i in enumerate(lows):
            lo, hi = pairs[(start + 4 * (k // 3) + j) % len(pairs)]
            t[8 * o + i], t[8 * o + i + s] = lo, hi
    return t


def stride_classes(p, t, s):
    """the classes met by the differences t[i + s] - t[i] inside the aligned octets of t (i without bit s)"""
    t = [int(x) for x in t]
    out = set()
    for i in range(len(t)):
        if not (i & 7) & s and (i & 7) + s < 8 and i + s < len(t):
            out |= classes_of(p, t[i], t[i + s])
    return out


def half_stride_table(p, rows, c, rng):
    """`rows` rows of 2^c raw words for the Reed-Solomon encoder (tests/test_gpu_ligero_wide.py).  Its first executed level, at
    the position whose twiddle is the field's one, takes t[k] + t[k + C/2] and t[k] - t[k + C/2] of the raw words of a row, k <
    C/2 = 2^(c-1) (with c = 1 those are the outputs themselves).  Each row's pairs (k, k + C/2) take the pairs of
    diff_classes(p) in turn, going on from row to row from a seeded start: t[k] = hi, t[k + C/2] = lo.  rows * C/2 >=
    len(diff_classes(p)) pairs carry them all; positions past the list's end hold uniform residues (c = 0: every position)."""
    C = 1 << c
    t = rng.integers(0, p, size=(rows, C), dtype=np.uint64)
    pairs = diff_classes(p)
    start, h = int(rng.integers(0, len(pairs))), C // 2
    for i in range(rows):
        for k in range(min(h, max(0, len(pairs) - i * h))):
            lo, hi = pairs[(start + i * h + k) % len(pairs)]
            t[i, k], t[i, k + h] = hi, lo
    return t.reshape(rows * C)


def half_stride_classes(p, t, c):
    """the classes met by the pairs (lo, hi) = (t[k + C/2], t[k]), k < C/2, of every row of 2^c words of t"""
    C = 1 << c
    t = [int(x) for x in t]
    out = set()
    for row in range(0, len(t), C):
        for k in range(C // 2):
            out |= classes_of(p, t[row + k + C // 2], t[row + k])
    return out


def degenerate_challenges(p, n):
    """n raw challenge words cycling through 0, R mod p (the field's one), p-1, 1, p-2 and (p+1)/2: with r = 0 a fold hands
    the even entries on unchanged and with r = one the odd entries, which carries the patterns of octet_table through a
    pass with pending challenges into its extension step"""
    cyc = [0, 2**64 % p, p - 1, 1, p - 2, (p + 1) // 2]
    return [cyc[j % len(cyc)] for j in range(n)]


def select_challenges(p, k):
    """k raw challenge words, each 0 or the field's one (0, one, one, 0, 0, ...): a fold by them keeps one entry of every
    aligned 2^k - with octet_table(shift=k) a table of octets"""
    one = 2**64 % p
    return [(0, one, one, 0)[j % 4] for j in range(k)]
