"""CPU-only: expander-code rows longer than the LDS of a CU (csrc/kernels/expander_long.hpp).  The
plan - which levels run through global memory, where, and the inner code - compiled for the host
(tests/cpp/xc_long_host_harness.cpp) for every c; a replay of the launches with the kernels' own work items on a two-row,
row-strided array against tests/expander_ref.py bit for bit; check_levels (tests/expander_long_ref.py), the checker the GPU
tests use on rows too long to encode in Python, against the reference: it accepts every codeword and rejects every single-word
corruption; and the Python surface that needs no GPU."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import expander_long_ref as xl_ref
import expander_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = 2**64 - 2**32 + 1
P59 = 2**64 - 59
R64 = 2**64
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def xl(tmp_path_factory):
    out = tmp_path_factory.mktemp("xl") / "libxc_long_host.so"
    src = os.path.join(ROOT, "tests", "cpp", "xc_long_host_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), src])
    lib = ctypes.CDLL(str(out))
    lib.xl_plan.argtypes = [ctypes.c_int, ip, u32p, ip, u32p]
    lib.xl_encode_rows.argtypes = [ctypes.c_uint64, ctypes.c_int, u64p, u64p, ctypes.c_int, ctypes.c_int, u64p]
    return lib


def plan(xl, c):
    """([(lm, offset)] of the global levels, (lm_i, offset_i))"""
    cap = xl.xl_max_levels()
    lm, off = (ctypes.c_int * cap)(), (ctypes.c_uint32 * cap)()
    lm_i, off_i = ctypes.c_int(), ctypes.c_uint32()
    levels = xl.xl_plan(c, lm, off, ctypes.byref(lm_i), ctypes.byref(off_i))
    assert 0 <= levels <= cap
    return [(lm[k], off[k]) for k in range(levels)], (lm_i.value, off_i.value)


def test_the_plan(xl):
    for c in range(0, 24):
        levels, (lm_i, off_i) = plan(xl, c)
        if c <= 13:
            assert levels == [] and (lm_i, off_i) == (c, 0)
            continue
        assert [lm for lm, _ in levels] == list(range(c, 13, -2))                 # descending by 2, all above 13
        assert lm_i == levels[-1][0] - 2 and lm_i in (12, 13)
        # the in-place layout: Enc_(m/4)(y) starts where y does, at o + m
        o = 0
        for lm, off in levels:
            assert off == o
            o += 1 << lm
        assert off_i == o and off_i + (2 << lm_i) <= 2 << c
    assert len(plan(xl, 23)[0]) == xl.xl_max_levels() == 5


@pytest.mark.parametrize("c", [14, 15])
@pytest.mark.parametrize("p,gold", [(P59, 0), (GOLD, 1)], ids=["p59", "gold"])
def test_host_replay_equals_the_reference(xl, p, gold, c):
    """two rows: every item of the second lands one row stride further"""
    n = c + 1
    rng = random.Random(100 * c + gold)
    table = [rng.randrange(p) for _ in range(1 << n)]
    inv = np.array([0] + [pow(s, -1, p) * R64 % p for s in range(1, 64)], dtype=np.uint64)
    w = np.array([x * R64 % p for x in table], dtype=np.uint64)
    E = np.zeros(2 << n, dtype=np.uint64)
    xl.xl_encode_rows(p, gold, w.ctypes.data_as(u64p), inv.ctypes.data_as(u64p), n, c, E.ctypes.data_as(u64p))
    want = np.array([v * R64 % p for row in ref.encode_rows(table, c, p) for v in row], dtype=np.uint64)
    assert np.array_equal(E, want), (p, c, int(np.flatnonzero(E != want)[0]))
    # and the checker agrees, on the Montgomery words as they are
    for i in (0, 1):
        xl_ref.check_levels(p, w[i << c:(i + 1) << c], E[i << (c + 1):(i + 1) << (c + 1)], c, positions=c)


@pytest.mark.parametrize("p", [P59, 257], ids=["p59", "p257"])
def test_check_levels_accepts_the_reference(p):
    rng = random.Random(p)
    for c in range(6, 11):
        x = [rng.randrange(p) for _ in range(1 << c)]
        E = ref.encode(x, p)
        xl_ref.check_levels(p, x, E, c)
        xl_ref.check_levels(p, x, E, c, positions=1)
        xl_ref.check_levels(p, [v * R64 % p for v in x], [v * R64 % p for v in E], c)          # any fixed multiple: the maps are linear


@pytest.mark.parametrize("p", [P59, 257], ids=["p59", "p257"])
def test_check_levels_rejects_every_single_word_corruption(p):
    c = 6
    rng = random.Random(c)
    x = [rng.randrange(p) for _ in range(1 << c)]
    E = ref.encode(x, p)
    for i in range(2 << c):
        bad = list(E)
        bad[i] = (bad[i] + 1 + rng.randrange(p - 1)) % p
        with pytest.raises(AssertionError):
            xl_ref.check_levels(p, x, bad, c)
    with pytest.raises(AssertionError):
        xl_ref.check_levels(p, x[:-1] + [(x[-1] + 1) % p], E, c)


def test_the_python_surface(pkg):
    lp = pkg.ligero_pcs
    assert pkg.expander_code.LONG_MAX_LOG_COLS == 23 and pkg.expander_code.MAX_LOG_COLS == 13
    assert lp.long_log_cols(28, 1, 128, 24) == 17
    assert lp.default_log_cols(28, 1, "expander") == 13                                         # unchanged
    assert pkg._lib.KIND_NAMES[23] == "xc_long"
    with pytest.raises(ValueError):
        lp.Prover.commit_long(None, None, 14, 1, code="ldpc")
    with pytest.raises(ValueError):
        lp.Prover.commit_long(None, None, code="expander")                                      # neither log_cols nor queries
    assert callable(lp.xc_encode_rows_long)
