"""wfold_pass_kernel's clock-aligned write slots (kernels/grid_pass.hpp, WfSlots; options "wfold_slot_period" / "wfold_slot_width" /
"wfold_slot_stagger"): when the folded tables are stored must never change what is stored.  Transcripts bit for bit against the
CPU oracle with host_tail_log = 0, so that every later round is served from the stored folded tables, at the smallest shapes at
which the held-back stores can go wrong - one tile and seven idle waves, two tiles, two and eight tiles per wave, uneven shares -
and under the settings that take every way out of the wave's registers: no slots at all, a slot that never opens (every store
leaves at the deadline or behind the loop), one that is always open, slots that flicker from boundary to boundary, and the
aligned write-back requests alone (width 0); each with the XCDs' slots aligned and staggered.  Before every setting the blocks
that will take the folded tables are filled with another proof's words, so that a store that never left is a wrong transcript
(checked against two wrong builds: without the store behind the loop every case that launches the pass fails, 14 of 16; without
the deadline store every case in which a wave takes a second tile fails, 10 of 16)."""
import numpy as np
import pytest

from conftest import load_package
from util import GOLD, challenges, oracle, pid, pyref

pytestmark = pytest.mark.gpu

P59 = 2**64 - 59
BASE = {"first_pass_vars": 4, "wfold_min_log": 12, "wfold_always": 1, "host_tail_log": 0}
# (period, width) in ticks of 10 ns
NEVER, ALWAYS, FLICKER, REQUESTS = (1 << 24, 1), (800, 800), (5, 2), (800, 0)
SETTINGS = [(0, 0, 0)] + [(p_, w_, s_) for (p_, w_) in (NEVER, ALWAYS, FLICKER, REQUESTS) for s_ in (0, 1)]

_refs = {}


def reference(p, n):
    if (p, n) not in _refs:
        o = oracle(p)
        ha, hb = o.generate(pyref.SEED_A, n), o.generate(pyref.SEED_B, n)
        ref = o.prove(ha, hb, challenges(o, n))
        assert ref["status"] == 0
        _refs[(p, n)] = (ha, hb, ref)
    return _refs[(p, n)]


def walk(pkg, ctx, a, b, n):
    """one proof both ways (whole, then round by round): c_1, the round polynomials, the final evaluation, the launches"""
    g = pkg.matrix_multiplication.G(a, b)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log(reset=True)
    c1, evals, ch = pkg.matrix_multiplication.prove(ctx, g, pyref.SEED_R)
    log = [(r["kind"], r["kf"], r["ks"], r["log_in"]) for r in ctx.launch_log(reset=True)]
    ctx.set_option("time_kernels", 0)
    final = g.evaluate([int(x) for x in ch])
    # round by round: rounds 4..8 out of the pass's cells, everything behind them out of the tables it stored
    pr = g.native_prover()
    rounds = [pr.round_evals(int(ch[j - 1]) if j else ctx.field.one, j) for j in range(n)]
    c1_rounds = pr.c1()
    del pr, g
    return c1, np.array(evals, copy=True), final, c1_rounds, rounds, log


def run_settings(pkg, p, n, opts, wfold_launches):
    ha, hb, ref = reference(p, n)
    ctx = pkg.Context(pkg.Field(p))
    for k, v in dict(BASE, **opts).items():
        ctx.set_option(k, v)
    a = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, ha)
    b = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, hb)
    # A store that never leaves must show.  The folded tables of a proof go to pool blocks, and the pool hands the blocks of the
    # last proof of this shape out again in the same order: left alone, every setting would find the right words of the run before
    # it already in place.  So in front of every setting the same context proves OTHER tables of the same shape without slots,
    # the same two ways, and leaves their folded words in those blocks (tools/wfbench.hip clears its outputs for the same reason)
    da = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A ^ 0x5A5A5A5A, n)
    db = pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_B ^ 0x5A5A5A5A, n)
    transcripts = []
    for period, width, stagger in SETTINGS:
        ctx.set_option("wfold_slot_period", 0)
        d_c1, d_evals, _, _, _, d_log = walk(pkg, ctx, da, db, n)
        assert d_c1 != ref["c_1"] and not np.array_equal(d_evals[n - 1], ref["evals"][n - 1])   # (other words, down to the last round)
        ctx.set_option("wfold_slot_period", period)
        ctx.set_option("wfold_slot_width", width)
        ctx.set_option("wfold_slot_stagger", stagger)
        assert (ctx.get_option("wfold_slot_period"), ctx.get_option("wfold_slot_width"), ctx.get_option("wfold_slot_stagger")) == (period, width, stagger)
        what = (p, n, opts, period, width, stagger)
        c1, evals, final, c1_rounds, rounds, log = walk(pkg, ctx, a, b, n)
        assert log == d_log and [r[1:] for r in log if r[0] == "wfold_pass"] == wfold_launches, (log, d_log, what)
        assert c1 == ref["c_1"] and c1_rounds == ref["c_1"], what
        assert np.array_equal(evals, ref["evals"]), what
        assert final == ref["final_eval"], what
        for j in range(n):
            assert rounds[j] == [int(x) for x in ref["evals"][j]], (what, j)
        transcripts.append(evals)
    for t in transcripts[1:]:   # (stagger on and off, and every setting against none: the same words)
        assert np.array_equal(t, transcripts[0])
    del a, b, da, db
    ctx.close()


@pytest.mark.parametrize("p", [GOLD, P59], ids=pid)
@pytest.mark.parametrize("n,opts,wfold_launches", [
    (12, {}, [(4, 5, 12)]),                    # one tile: one wave works, seven hold nothing
    # n = 13 under these options: the planner gives the first pass five rounds, so no (4, 5) launch exists on two tiles (the
    # proof runs through the grid passes; kept, because a setting must not disturb them either) - the two tiles come in the
    # five-challenge form, below
    (13, {}, []),
    (16, {"max_blocks": 1}, [(4, 5, 16)]),     # two tiles per wave: the second tile's boundaries and its deadline
    (18, {"max_blocks": 1}, [(4, 5, 18)]),     # eight tiles per wave
    (18, {"max_blocks": 3}, [(4, 5, 18)])])    # uneven shares: 22 / 21 / 21 tiles per block
def test_slots_store_what_the_kernel_without_them_stores(p, n, opts, wfold_launches):
    run_settings(load_package(), p, n, opts, wfold_launches)


@pytest.mark.parametrize("p", [GOLD, P59], ids=pid)
@pytest.mark.parametrize("n,opts,wfold_launches", [
    (13, {"wfold5_min_log": 12}, [(5, 4, 13)]),                                  # two tiles, one block each
    (18, {"max_blocks": 1, "wfold5_min_log": 12}, [(4, 5, 18), (5, 5, 14)]),    # (5, 5) behind the (4, 5) pass on four tiles
    (20, {"max_blocks": 1, "wfold5_min_log": 12}, [(4, 5, 20), (5, 4, 16)])])   # ... (5, 4) on sixteen: two per wave, 8 VGPRs held
def test_slots_in_the_five_challenge_form(p, n, opts, wfold_launches):
    run_settings(load_package(), p, n, opts, wfold_launches)
