"""CPU-only checks of sc_matmul (the C = A * B of the MatMult protocol): the symbol is exported and declared, the int32 run
bound of kernels/matmul.hpp holds on the worst byte pattern at the largest size, and the host verifier of
matrix_multiplication accepts pyref-made transcripts and rejects tampered ones."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_package
from util import GOLD, pyref

MATMUL_HPP = os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "matmul.hpp")


def matmul_constant(name):
    m = re.search(r"constexpr int %s = ([0-9]+|kMatmulRunSteps \* kMatmulStepK);" % name, open(MATMUL_HPP).read())
    assert m, name
    if m.group(1).isdigit():
        return int(m.group(1))
    return matmul_constant("kMatmulRunSteps") * matmul_constant("kMatmulStepK")


def test_library_exports_sc_matmul():
    pkg = load_package()
    pkg.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    assert re.search(r" T sc_matmul$", out, flags=re.M)
    assert "sc_matmul" in pkg._lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()
    assert re.search(r"int sc_matmul\(sc_ctx\* ctx, const sc_table\* A, const sc_table\* B, size_t n, sc_table\*\* C\);", header)
    assert re.search(r"#define SC_KIND_MATMUL 15\b", header)
    assert pkg._lib.KIND_NAMES[15] == "matmul"
    rust = open(os.path.join(ROOT, "rust", "sumcheck-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn sc_matmul\(", rust)


def test_accumulator_run_bound_fits_int32_at_n14():
    step = matmul_constant("kMatmulStepK")
    run_steps = matmul_constant("kMatmulRunSteps")
    run = run_steps * step
    assert matmul_constant("kMatmulMaxRunK") == run
    # worst pattern: all-zero bytes, s = 0 ^ 0x80 = -128 on both sides; the middle diagonal has 8 byte pairs
    worst_per_y = 8 * (-128) * (-128)
    assert worst_per_y * run <= 2**31 - 1
    # the most negative per-y sum stays far inside too
    assert 8 * (-128) * 127 * run >= -(2**31)
    # at n = 14 the contraction needs more than one run, and one step more per run would overflow on that pattern
    K = 1 << 14
    assert K > run and (K + step - 1) // step > run_steps
    assert worst_per_y * (run + step) > 2**31 - 1
    # every run of the n = 14 contraction is within the bound
    runs = [min(run, K - s) for s in range(0, K, run)]
    assert sum(runs) == K and all(worst_per_y * r <= 2**31 - 1 for r in runs)


def _transcript(p, n, seed):
    """a pyref MatMult transcript in Montgomery words: (field, claim, c_1, evals, challenges, oracle)"""
    import random
    pkg = load_package()
    F = pkg.Field(p)
    rng = random.Random(seed)
    N = 1 << n
    A = [rng.randrange(p) for _ in range(N * N)]
    B = [rng.randrange(p) for _ in range(N * N)]
    pt = [rng.randrange(p) for _ in range(2 * n)]
    C = [x for row in pyref.matmul([A[i * N:(i + 1) * N] for i in range(N)], [B[i * N:(i + 1) * N] for i in range(N)], p) for x in row]
    claim = pyref.mle_evaluate(C, pt[n:] + pt[:n], p)
    fa, fb = pyref.g_new(n, A, B, pt, p)
    ch = [rng.randrange(p) for _ in range(n)]
    ref = pyref.transcript(fa, fb, ch, p)
    assert ref["c_1"] == claim   # the MatMult identity, in pyref alone
    evals = [[F.from_int(x) for x in e] for e in ref["evals"]]

    def oracle(r):
        return F.from_int(pyref.g_evaluate(fa, fb, [F.to_int(x) for x in r], p))

    return F, F.from_int(claim), F.from_int(ref["c_1"]), evals, [F.from_int(x) for x in ch], oracle


@pytest.mark.parametrize("p", [GOLD, 2**64 - 59, 389])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_verify_transcript(p, n):
    mm = load_package().matrix_multiplication
    F, claim, c_1, evals, ch, oracle = _transcript(p, n, 100 * n + p % 7)
    assert mm.verify_transcript(F, n, claim, c_1, evals, ch, oracle)
    # a tampered claim
    assert not mm.verify_transcript(F, n, F.add(claim, F.one), c_1, evals, ch, oracle)
    # a tampered round: every round, each of the three values
    for j in range(n):
        for t in range(3):
            bad = [list(e) for e in evals]
            bad[j][t] = F.add(bad[j][t], F.one)
            assert not mm.verify_transcript(F, n, claim, c_1, bad, ch, oracle), (j, t)
    # rounds replayed against another first challenge (round 2 no longer matches g_1(r_1); the honest g_n matches G at
    # any last challenge, so only an earlier one shows)
    if n >= 2:
        other = list(ch)
        other[0] = F.add(other[0], F.one)
        assert not mm.verify_transcript(F, n, claim, c_1, evals, other, oracle)


def test_product_point_order():
    pkg = load_package()
    mm = pkg.matrix_multiplication
    F = pkg.Field(GOLD)
    pt = mm.product_point(F, 3, 7)
    assert len(pt) == 6 and pt == [F.from_int(pyref.splitmix64(7 + i + 1) % GOLD) for i in range(6)]
