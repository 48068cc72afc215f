"""CPU-only: the plain compiled reference (tests/rs_plain.py, tests/cpp/rs_plain_ref.cpp) pinned to the Python references it
stands in for at long lengths: its encoding against ligero_ref.encode at every shape up to 2^13 words over every field of the
tests, at 2^20 and 2^24 words against its own defining sum (another routine of the same file: Horner instead of butterflies), and
its fold against ligero_fold_ref.fold."""
import random

import numpy as np
import pytest

import ligero_fold_ref as fref
import ligero_ref as ref
import rs_plain

FIELDS = ref.FIELDS + ref.WIDE_NTT


def pid(p):
    return "p%x" % p


@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_encode_equals_the_python_reference(p):
    s = ref.ROOTS[p][0]
    rng = random.Random(p)
    shapes = [(c, rho) for rho in (1, 2) for c in range(0, 14 - rho) if c + rho <= min(13, s)]
    assert shapes
    for c, rho in shapes:
        r = 1 if c + rho < 12 else 0                  # two rows where that is cheap: the second row's offset
        table = [rng.randrange(p) for _ in range(1 << (r + c))]
        got = rs_plain.encode(p, table, c, rho)
        want = [x for row in ref.encode(table, c, rho, p) for x in row]
        assert [int(x) for x in got] == want, (p, c, rho)


@pytest.mark.parametrize("log_len", [20, 24])
@pytest.mark.parametrize("p", [ref.GOLD, ref.P64S34], ids=pid)
def test_long_encodings_equal_the_defining_sum(p, log_len):
    c, rho = log_len - 1, 1
    L = 1 << log_len
    row = np.random.default_rng([p % 1000, log_len]).integers(0, p, size=1 << c, dtype=np.uint64)
    E = rs_plain.encode(p, row, c, rho)
    assert E.size == L
    rng = random.Random(log_len)
    for j in [0, 1, L // 2, L - 1] + [rng.randrange(L) for _ in range(12)]:
        assert int(E[j]) == rs_plain.eval_at(p, row, log_len, j), (p, log_len, j)


@pytest.mark.parametrize("p", FIELDS, ids=pid)
def test_fold_equals_the_python_reference(p):
    s = ref.ROOTS[p][0]
    rng = random.Random(p + 1)
    for log_m in range(2, min(12, s) + 1):
        U = [rng.randrange(p) for _ in range(1 << log_m)]
        for alpha in (0, 1, p - 1, rng.randrange(p)):
            assert [int(x) for x in rs_plain.fold(p, U, alpha)] == fref.fold(U, alpha, p), (p, log_m, alpha)
