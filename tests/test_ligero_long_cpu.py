"""CPU-only: the long-row Reed-Solomon encoder (csrc/kernels/ligero_long.hpp).  The split, the index
maps and the twist of the two kernels, compiled for the host (tests/cpp/rs_long_host_harness.cpp): the split's bounds, every
map a bijection on a row, the blocks of the in-place step disjoint, and a replay of both steps - the kernel's own maps and twist
around a plain radix-2 transform - against tests/ligero_ref.py bit for bit, and from 2^19 words up to the limit 2^24 against the
compiled textbook encoder of tests/rs_plain.py; and the opening-size helpers of ligero_pcs."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import ligero_ref as ref
import rs_plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = ref.GOLD
u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def rl(tmp_path_factory):
    out = tmp_path_factory.mktemp("rl") / "librs_long_host.so"
    src = os.path.join(ROOT, "tests", "cpp", "rs_long_host_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), src])
    lib = ctypes.CDLL(str(out))
    ip = ctypes.POINTER(ctypes.c_int)
    lib.rl_split.argtypes = [ctypes.c_int, ip, ip, ip]
    lib.rl_blocks.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.rl_blocks.restype = ctypes.c_uint64
    lib.rl_map_block.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, u64p]
    lib.rl_encode.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, u64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64p]
    return lib


def split(rl, log_len):
    a, b, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rl.rl_split(log_len, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t))
    return a.value, b.value, t.value


def block_map(rl, which, log_len, rho, blk):
    _, _, tile_log = split(rl, log_len)
    out = np.zeros(1 << (tile_log - rho if which in (0, 3) else tile_log), dtype=np.uint64)
    rl.rl_map_block(which, log_len, rho, blk, out.ctypes.data_as(u64p))
    return out


def test_the_split(rl):
    for log_len in range(15, 25):
        a, b, tile_log = split(rl, log_len)
        assert a + b == log_len and a <= 14 and b <= 14, (log_len, a, b)
        assert all(rho <= a for rho in (1, 2)), (log_len, a)                          # step 0 runs a - rho >= 0 levels of its own
        assert max(a, b) <= tile_log <= 14                                            # a tile holds whole transforms
        assert rl.rl_blocks(log_len, log_len + 3) == 8 << (log_len - tile_log)


def covers(addresses, start, stop):
    """the addresses are [start, stop), each once: as many as the range has, all inside it, none missing"""
    if addresses.size != stop - start or int(addresses.min()) < start or int(addresses.max()) >= stop:
        return False
    seen = np.zeros(stop - start, dtype=bool)
    seen[(addresses - np.uint64(start)).astype(np.int64)] = True
    return bool(seen.all())


@pytest.mark.parametrize("log_len", range(15, 25))
def test_the_maps_cover_a_row_exactly_once(rl, log_len):
    """every length the encoder serves - each has its own split (a, b) from (8, 7) to (12, 12) - at rho = 1 and 2.  From 2^21
    words on only the second matrix row, which still carries the row offset"""
    a, b, tile_log = split(rl, log_len)
    per_row = rl.rl_blocks(log_len, log_len)
    for rho in (1, 2):
        c = log_len - rho
        for row in ((0, 1) if log_len < 21 else (1,)):       # the second matrix row: everything moves by one row
            blocks = range(row * per_row, (row + 1) * per_row)
            src = np.concatenate([block_map(rl, 0, log_len, rho, blk) for blk in blocks])
            assert covers(src, row << c, (row + 1) << c)
            dst = np.concatenate([block_map(rl, 1, log_len, rho, blk) for blk in blocks])
            assert covers(dst, row << log_len, (row + 1) << log_len)
            per_block = [block_map(rl, 2, log_len, rho, blk) for blk in blocks]
            assert covers(np.concatenate(per_block), row << log_len, (row + 1) << log_len)
            # (a bijection on the row from blocks of 2^tile_log items each: the sets of distinct blocks are disjoint)
            assert all(np.unique(m).size == 1 << tile_log for m in per_block)
        # inside the tile: step 0 fills every 2^rho-th position once, step 1 every position once, in and out
        pos0 = block_map(rl, 3, log_len, rho, 1)
        assert np.array_equal(np.sort(pos0), np.arange(0, 1 << tile_log, 1 << rho, dtype=np.uint64))
        for which in (4, 5):
            assert np.array_equal(np.sort(block_map(rl, which, log_len, rho, 1)), np.arange(1 << tile_log, dtype=np.uint64))
        # the twist exponent of T[j1 + L1 k2] is j1 k2
        for blk in (0, per_row - 1, per_row, 2 * per_row - 1):
            addr = block_map(rl, 1, log_len, rho, blk) % np.uint64(1 << log_len)
            j1, k2 = addr % np.uint64(1 << a), addr >> np.uint64(a)
            assert np.array_equal(block_map(rl, 6, log_len, rho, blk), j1 * k2)
            assert int((j1 * k2).max()) < 1 << log_len                    # inside the two twist tables


REPLAY = ([(GOLD, 1, log_len, rho, r) for log_len in (15, 16, 17) for rho in (1, 2) for r in (0, 1)]
          + [(ref.P64S18, 0, 15, 1, 0), (ref.P64S18, 0, 18, 1, 0), (65537, 0, 16, 1, 0)])
# .. and the lengths only the compiled reference follows: raw uniform words in (both sides are linear in them), one row
LONG_REPLAY = ([(GOLD, 1, log_len, 1, 0) for log_len in range(19, 25)] + [(GOLD, 1, 21, 2, 0), (GOLD, 1, 23, 2, 0)]
               + [(ref.P64S34, 0, 21, 1, 0), (ref.P64S34, 0, 24, 1, 0)])


@pytest.mark.parametrize("p,gold,log_len,rho,r", REPLAY + LONG_REPLAY, ids=lambda v: str(v))
def test_host_replay_equals_the_reference(rl, p, gold, log_len, rho, r):
    c = log_len - rho
    n = r + c
    omega = ref.omega(p, log_len) * ref.R64 % p
    if (p, gold, log_len, rho, r) in LONG_REPLAY:
        w = np.random.default_rng([p % 1000, log_len, rho]).integers(0, p, size=1 << n, dtype=np.uint64)
        E = np.zeros(1 << (n + rho), dtype=np.uint64)
        rl.rl_encode(p, gold, omega, w.ctypes.data_as(u64p), n, c, rho, E.ctypes.data_as(u64p))
        want = rs_plain.encode(p, w, c, rho)
        assert np.array_equal(E, want), (p, log_len, rho, r, int(np.flatnonzero(E != want)[0]))
        return
    rng = random.Random(100 * log_len + 10 * rho + r)
    table = [rng.randrange(p) for _ in range(1 << n)]
    w = np.array(ref.mont(p, table), dtype=np.uint64)
    E = np.zeros(1 << (n + rho), dtype=np.uint64)
    rl.rl_encode(p, gold, omega, w.ctypes.data_as(u64p), n, c, rho, E.ctypes.data_as(u64p))
    want = np.array(ref.mont(p, [x for row in ref.encode(table, c, rho, p) for x in row]), dtype=np.uint64)
    assert np.array_equal(E, want), (p, log_len, rho, r, int(np.flatnonzero(E != want)[0]))


def test_opening_size(pkg):
    lp = pkg.ligero_pcs
    assert lp.LONG_MAX_LOG_LEN == 24 and lp.MAX_LOG_LEN == 14
    assert lp.opening_bytes(28, 16, 1, 64) == 3180544
    assert [lp.long_log_cols(28, 1, t) for t in (64, 128, 256)] == [16, 17, 17]
    assert lp.long_log_cols(10, 1, 64) <= 10
    assert lp.long_log_cols(28, 2, 256, max_log_len=16) == 14
    # the smallest by exhaustion, ties to the smaller c
    for n, rho, t in ((28, 1, 64), (20, 2, 100), (5, 1, 1)):
        sizes = [lp.opening_bytes(n, c, rho, t) for c in range(min(n, 24 - rho) + 1)]
        assert lp.long_log_cols(n, rho, t) == sizes.index(min(sizes))
