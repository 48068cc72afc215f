"""Words and moduli for testing the generic field at full word width (tests/test_oracle_wide_moduli.py,
tests/test_gpu_wide_moduli.py)."""
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
