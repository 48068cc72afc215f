"""The four-round first pass on the int8 matrix cores (kernels/gram.hpp: gram_pass_kernel) with full partials: an int32
accumulator of the kernel takes 2^16 rows (|s s'| <= 2^14), launch_gram_pass cuts the rows into partials of at most that many,
and at the headline shape every partial holds exactly 2^16 rows.  These cases put extreme bytes into full partials, over
Goldilocks and two moduli above 2^63, and check from the launch log that the partials really were full - a change of geometry
fails here instead of quietly testing a smaller partial."""
import os
import re

import numpy as np
import pytest

from conftest import load_package
from util import GOLD, oracle, pid, pyref

pytestmark = pytest.mark.gpu

P59 = 2**64 - 59
P63 = 2**63 + 29

GRAM_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thaler-study_amd", "csrc", "kernels", "gram.hpp")
FULL_PARTIAL_ROWS = 1 << 16          # 2^16 rows of signed products of at most 2^14 stay below 2^31
GRAM_ROWS_PER_STEP = 64              # K = 4: a row is 2^4 entries of 8 bytes, a step 8 KiB of each table


def gram_constant(name):
    m = re.search(r"constexpr int %s = (?:1 << )?(\d+);" % name, open(GRAM_HPP).read())
    assert m, name
    return int(m.group(1)) if "1 << " not in m.group(0) else 1 << int(m.group(1))


def gram_geometry(ctx, n):
    """(grid, n_partials, steps per partial) of the last gram launch: the grid from bytes_written = grid * kGramRowWords * 8,
    the rest by launch_gram_pass's rule with that grid as the block count"""
    recs = [r for r in ctx.launch_log() if r["kind"] == "gram_pass"]
    assert len(recs) == 1, recs
    row_bytes = gram_constant("kGramRowWords") * 8
    assert recs[0]["bytes_written"] % row_bytes == 0
    grid = recs[0]["bytes_written"] // row_bytes
    max_steps = gram_constant("kGramMaxRows") // GRAM_ROWS_PER_STEP
    n_steps = (1 << n) // (gram_constant("kGramTabBytes") // 8)
    n_partials = min(grid, n_steps // gram_constant("kGramStages"))
    while n_steps // n_partials > max_steps:
        n_partials *= 2
    spp = n_steps // n_partials
    assert n_partials * spp == n_steps
    return grid, n_partials, spp, max_steps


def byte_pattern(p, kind, n, seed):
    size = 1 << n
    ff, x80, x7f = p - 1, 0x8080808080808080 % p, 0x7F7F7F7F7F7F7F7F % p
    row = np.arange(size, dtype=np.int64) >> 4
    if kind == "ff":
        return np.full(size, ff, dtype=np.uint64), np.full(size, ff, dtype=np.uint64)
    if kind == "zero_ff":
        return np.zeros(size, dtype=np.uint64), np.full(size, ff, dtype=np.uint64)
    if kind == "x80":
        return np.full(size, x80, dtype=np.uint64), np.full(size, x80, dtype=np.uint64)
    if kind == "x7f":
        return np.full(size, x7f, dtype=np.uint64), np.full(size, x7f, dtype=np.uint64)
    if kind == "alt_rows":
        return (np.where(row % 2 == 0, ff, 0).astype(np.uint64), np.where(row % 3 == 0, 0, ff).astype(np.uint64))
    rng = np.random.default_rng(seed)
    words = np.array([ff, 0, x80, x7f], dtype=np.uint64)
    return words[rng.integers(0, 4, size, dtype=np.uint8)], words[rng.integers(0, 4, size, dtype=np.uint8)]


GRAM_KINDS = ["ff", "zero_ff", "x80", "x7f", "alt_rows", "mix"]


@pytest.mark.parametrize("kind", GRAM_KINDS)
@pytest.mark.parametrize("p", [GOLD, P59, P63], ids=pid)
@pytest.mark.parametrize("n,max_blocks,grid", [(20, 1, 1), (21, 1, 1), (22, 2, 2)])
def test_gram_full_partials(p, kind, n, max_blocks, grid):
    """one block and one partial of exactly 2^16 rows (n = 20); one block walking two full partials, which it adds mod p
    (n = 21); two blocks of two full partials each (n = 22) - each extreme byte pattern, transcript and final evaluation
    against the oracle"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    ctx.set_option("first_pass_vars", 4)
    ctx.set_option("max_blocks", max_blocks)
    ctx.set_option("time_kernels", 1)
    ha, hb = byte_pattern(p, kind, n, seed=n)
    a = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, ha)
    b = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, hb)
    g = pkg.matrix_multiplication.G(a, b)
    ctx.launch_log(reset=True)
    c1, evals, ch = pkg.matrix_multiplication.prove(ctx, g, pyref.SEED_R)
    got_grid, n_partials, spp, max_steps = gram_geometry(ctx, n)
    assert (got_grid, n_partials) == (grid, 1 << (n - 20)), (got_grid, n_partials)
    assert spp == max_steps and spp * GRAM_ROWS_PER_STEP == FULL_PARTIAL_ROWS, (spp, max_steps)
    ref = oracle(p).prove(ha, hb, ch)
    assert ref["status"] == 0
    assert c1 == ref["c_1"], (p, kind, n)
    assert np.array_equal(evals, ref["evals"]), (p, kind, n)
    assert g.evaluate([int(x) for x in ch]) == ref["final_eval"], (p, kind, n)
    del g, a, b
    ctx.close()


@pytest.mark.parametrize("kind", ["ff", "mix"])
@pytest.mark.parametrize("p", [GOLD, P59], ids=pid)
def test_gram_full_partials_headline_shape(p, kind):
    """n = 28 with the default options: 256 partials of exactly 2^16 rows, against the oracle's multithreaded prover (as
    bench.py checks the headline), and the final evaluation against the oracle's last round polynomial at the last
    challenge"""
    pkg = load_package()
    n = 28
    o = oracle(p)
    ctx = pkg.Context(pkg.Field(p))
    ctx.set_option("time_kernels", 1)
    ha, hb = byte_pattern(p, kind, n, seed=28)
    a = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, ha)
    b = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, hb)
    g = pkg.matrix_multiplication.G(a, b)
    ctx.launch_log(reset=True)
    c1, evals, ch = pkg.matrix_multiplication.prove(ctx, g, pyref.SEED_R)
    _, n_partials, spp, max_steps = gram_geometry(ctx, n)
    assert n_partials == 256 and spp == max_steps and spp * GRAM_ROWS_PER_STEP == FULL_PARTIAL_ROWS, (n_partials, spp)
    final = g.evaluate([int(x) for x in ch])
    del g, a, b
    ctx.close()
    c1_ref, ev_ref = o.prover_run_mt(ha, hb, ch)
    assert c1 == c1_ref and np.array_equal(evals, ev_ref), (p, kind)
    assert final == o.poly2_eval(o.interpolate(ev_ref[-1]), int(ch[-1])), (p, kind)
