"""sc_prove_batch at its design limits: batch sizes up to kBatchMaxCount (few blocks per instance, one block per 2^20-entry
table near the top), the refusal above it, every schedule option the single-proof planner honours (the batch runs each of
its passes through one batched kernel, whatever kind the planner chose), state carried across calls on one context, n = 0,
and MatMult end to end at the largest sizes.  Every instance must equal its own sc_prove word for word; the launch log
shows which path the batch took."""
import ctypes

import numpy as np
import pytest

from conftest import load_package
from test_gpu_prove_batch import P64, _raw, assert_same, fid, seeds, singles_of
from util import GOLD, challenges, oracle, pyref

pytestmark = pytest.mark.gpu

MAX_COUNT = 1024   # kBatchMaxCount (engine/abi_batch.inc)
MAX_LOG = 20       # kBatchMaxLog

_ctxs = {}


def ctx_of(pkg, p):
    if p not in _ctxs:
        _ctxs[p] = pkg.Context(pkg.Field(p))
    return _ctxs[p]


def distinct_instances(pkg, ctx, n, B, seed):
    """B instances with pairwise different (a, b) pairs from k + k device tables, k = ceil(sqrt(B)) (32 + 32 tables at
    B = 1024: 512 MiB at n = 20); instance i is (a[i % k], b[i // k]).  Returns (gs, seeds of a, seeds of b)."""
    mm = pkg.matrix_multiplication
    k = 1
    while k * k < B:
        k += 1
    sa = [seed + 7919 * t + n for t in range(k)]
    sb = [seed + 1 + 7919 * t + n for t in range(k)]
    ta = [pkg.DenseMultilinearExtension.generate(ctx, s, n) for s in sa]
    tb = [pkg.DenseMultilinearExtension.generate(ctx, s, n) for s in sb]
    gs = [mm.G(ta[i % k], tb[i // k]) for i in range(B)]
    return gs, [sa[i % k] for i in range(B)], [sb[i // k] for i in range(B)]


def batch_log(ctx, fn):
    ctx.set_option("time_kernels", 1)
    try:
        ctx.launch_log(reset=True)
        out = fn()
        log = ctx.launch_log(reset=True)
    finally:
        ctx.set_option("time_kernels", 0)
    return out, [(r["kind"], r["kf"], r["ks"], r["log_in"]) for r in log]


def launch_plan(pkg, n, **opts):
    return [(s["action"], s["kf"], s["ks"], s["log_in"]) for s in pkg.schedule.plan_proof(n, **opts) if s["action"] != "host_tail"]


def batchable(pkg, n, **opts):
    """batch_plan_ok (engine/abi_batch.inc) on the plan sc_plan_proof shows: 1 <= n <= 20, the mailbox, and passes of
    kf <= 5 / 1 <= ks <= 5 on whole tables up to the host tail"""
    if not 1 <= n <= MAX_LOG or not opts.get("use_mailbox", 1):
        return False
    for s in pkg.schedule.plan_proof(n, **opts):
        if s["action"] == "host_tail":
            return True
        if s["action"] in ("rank_pass", "gather") or s["kf"] > 5 or not 1 <= s["ks"] <= 5 or s["log_in"] < s["kf"] + s["ks"]:
            return False
    return True


def assert_batched(pkg, log, n, B, **opts):
    plan = launch_plan(pkg, n, **opts)
    assert len(plan) >= 1
    assert log == [("batch_pass", kf, ks, log_in) for _, kf, ks, log_in in plan], (n, B, opts, log, plan)


# ---- batch sizes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [128, 129, 256, 257, 1000, 1024])
@pytest.mark.parametrize("n", [4, 11, 12, 16, 17, 20])
@pytest.mark.parametrize("p", [GOLD, P64], ids=fid)
def test_batch_sizes(p, n, B):
    """at these counts an instance gets a handful of blocks of the resident grid (near B = 1024 one or two; at n = 20 one
    block may walk a whole 2^20-entry table), the instance's finish adds that few rows, and the prefetch form turns on at
    smaller tables than in any single proof; n = 11 / 12 and 16 / 17 sit on both sides of a hand-over to the host"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    mm = pkg.matrix_multiplication
    gs, sa, sb = distinct_instances(pkg, ctx, n, B, 0x51 * B)
    sd = seeds(B, 0xABC + n)
    out, log = batch_log(ctx, lambda: mm.prove_batch(ctx, gs, sd))
    assert_batched(pkg, log, n, B)
    assert_same(out, singles_of(pkg, ctx, gs, sd), "n=%d B=%d" % (n, B))
    o = oracle(p)
    for i in (0, 1, B // 2, B - 2, B - 1):
        c1, ev, ch = out[i]
        assert np.array_equal(ch, challenges(o, n, sd[i])), i
        ref = o.prove(o.generate(sa[i], n), o.generate(sb[i], n), ch)
        assert ref["status"] == 0 and c1 == ref["c_1"] and np.array_equal(ev, ref["evals"]), i


def test_count_above_the_limit_is_refused():
    pkg = load_package()
    ctx = ctx_of(pkg, GOLD)
    mm = pkg.matrix_multiplication
    t = [pkg.DenseMultilinearExtension.generate(ctx, 0xC0 + i, 6) for i in range(2)]
    ctx.set_option("time_kernels", 1)
    try:
        ctx.launch_log(reset=True)
        assert _raw(pkg, ctx, [t[0]] * (MAX_COUNT + 1), [t[1]] * (MAX_COUNT + 1)) == 1   # SC_ERR_ARG
        assert "at most 1024" in ctx.lib.sc_last_error(ctx.h).decode()
        assert ctx.launch_log(reset=True) == []
    finally:
        ctx.set_option("time_kernels", 0)
    with pytest.raises(pkg.SumcheckHipError) as ei:
        mm.prove_batch(ctx, [mm.G(t[0], t[1])] * (MAX_COUNT + 1), 5)
    assert ei.value.code == 1
    # the context still works, at the limit itself too
    gs = [mm.G(t[i % 2], t[(i // 2) % 2]) for i in range(MAX_COUNT)]
    sd = seeds(MAX_COUNT, 5)
    assert_same(mm.prove_batch(ctx, gs, sd), singles_of(pkg, ctx, gs, sd))


# ---- schedule options -------------------------------------------------------------------------------------------------

OPTION_SETS = [{}, {"grid_pass": 0}, {"vars_per_pass": 1}, {"first_pass_vars": 2}, {"grid_max_vars": 3}, {"grid_log": 8},
               {"first_pass_vars": 3, "grid_max_vars": 4}, {"first_pass_vars": 4}, {"gram_log": 0}, {"gram_log": 19, "grid_log": 12},
               {"host_tail_log": 0}, {"host_tail_log": 4}, {"host_tail_log": 8, "grid_max_vars": 3},
               {"first_pass_vars": 1}, {"grid_max_vars": 1}, {"grid_max_vars": 2}, {"grid_max_vars": 4}, {"gram_log": 14},
               {"first_pass_vars": 4, "wfold_min_log": 12, "wfold_always": 1}, {"use_mailbox": 0}]
# The batch waits on the mailbox once per pass: without it (use_mailbox = 0) the instances go one after another through
# sc_prove.  Every other set plans passes of kf <= 5 / ks <= 5 at every n here (asserted below against the plan), so the
# batch serves them - including the pass_kernel, gram and wfold passes of the single-proof plan.
FALLS_BACK = [{"use_mailbox": 0}]


@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda d: ",".join("%s=%d" % kv for kv in d.items()) or "default")
def test_schedule_options(opts, B):
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(GOLD))
    mm = pkg.matrix_multiplication
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        for n in (1, 3, 5, 8, 12, 14, 16, 18, 20):
            assert batchable(pkg, n, **opts) == (opts not in FALLS_BACK), (n, opts)
            gs, _, _ = distinct_instances(pkg, ctx, n, B, 0x0F7 + n)
            sd = seeds(B, 0x0F7)
            out, log = batch_log(ctx, lambda: mm.prove_batch(ctx, gs, sd))
            if opts in FALLS_BACK:
                assert log == launch_plan(pkg, n, **opts) * B, (n, opts)
            else:
                assert_batched(pkg, log, n, B, **opts)
            assert_same(out, singles_of(pkg, ctx, gs, sd), "n=%d B=%d %r" % (n, B, opts))
            del gs
    finally:
        ctx.close()


# ---- state across calls on one context --------------------------------------------------------------------------------

def test_pinned_memory_grows_and_shrinks():
    """counts and hand-over sizes that grow and shrink from call to call: the pinned batch memory is reallocated
    (batch_reserve) and the smaller batches after a larger one run in it"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(P64))
    mm = pkg.matrix_multiplication
    try:
        for B, n in [(3, 12), (300, 16), (5, 20), (1024, 12), (2, 17), (700, 20), (1, 4), (129, 11), (1024, 17), (8, 20)]:
            gs, _, _ = distinct_instances(pkg, ctx, n, B, 0x9A + B)
            sd = seeds(B, B + n)
            assert_same(mm.prove_batch(ctx, gs, sd), singles_of(pkg, ctx, gs, sd), "B=%d n=%d" % (B, n))
            del gs
    finally:
        ctx.close()


@pytest.mark.parametrize("p", [GOLD, P64], ids=fid)
def test_batch_between_rounds_of_a_prover(p):
    """a round-by-round prover (sc_prover) on the same context, with a batch between two of its rounds before and after
    it hands over to the host: its rounds still equal the oracle's"""
    pkg = load_package()
    ctx = ctx_of(pkg, p)
    mm = pkg.matrix_multiplication
    F, o = ctx.field, oracle(p)
    n = 17
    plan = pkg.schedule.plan_proof(n)
    assert plan[-1]["action"] == "host_tail"
    j_host = n - plan[-1]["ks"]   # the first round the host serves
    assert 2 < j_host < n - 1
    sa, sb = pyref.SEED_A + 3, pyref.SEED_B + 3
    g = mm.G(pkg.DenseMultilinearExtension.generate(ctx, sa, n), pkg.DenseMultilinearExtension.generate(ctx, sb, n))
    ch = challenges(o, n, 0x77)
    ref = o.prove(o.generate(sa, n), o.generate(sb, n), ch)
    pr = g.native_prover()
    assert pr.c1() == ref["c_1"]
    for j in range(n):
        if j in (1, j_host + 1, n - 1):
            B, nb = (64, 20) if j != n - 1 else (1024, 16)
            gs, _, _ = distinct_instances(pkg, ctx, nb, B, 0x100 + j)
            sd = seeds(B, j)
            assert_same(mm.prove_batch(ctx, gs, sd), singles_of(pkg, ctx, gs, sd), "between rounds, j=%d" % j)
            del gs
        e = pr.round_evals(F.one if j == 0 else int(ch[j - 1]), j)
        assert e == [int(x) for x in ref["evals"][j]], j


def test_unreduced_draw_late_in_a_large_batch():
    """B = 1024, n = 20: draw returns p (unreduced) for a late instance in a round after the hand-over to the host; the call
    fails with SC_ERR_ARG, the next batch is right, and ten failures lose no device memory"""
    import torch
    pkg = load_package()
    ctx = ctx_of(pkg, GOLD)
    F = ctx.field
    mm = pkg.matrix_multiplication
    n, B = 20, MAX_COUNT
    plan = pkg.schedule.plan_proof(n)
    assert plan[-1]["action"] == "host_tail"
    bad_round = n - 1
    assert bad_round >= n - plan[-1]["ks"]   # the host serves that round
    gs, _, _ = distinct_instances(pkg, ctx, n, B, 0xD7)
    small, _, _ = distinct_instances(pkg, ctx, 12, 64, 0xD8)
    sd_small = seeds(64, 3)
    want_small = singles_of(pkg, ctx, small, sd_small)

    def draw(i, j, e):
        if i == B - 3 and j == bad_round:
            return F.p
        return F.from_int(pyref.splitmix64((1000 * i + j) % 2**64) % F.p)

    free0 = None
    for rep in range(10):
        with pytest.raises(pkg.SumcheckHipError) as ei:
            mm.prove_batch(ctx, gs, None, draw)
        assert ei.value.code == 1 and "unreduced" in str(ei.value), str(ei.value)
        assert_same(mm.prove_batch(ctx, small, sd_small), want_small, "after failure %d" % rep)
        ctx.synchronize()
        if rep == 0:
            free0, _ = torch.cuda.mem_get_info(0)
    ctx.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    assert free1 >= free0, (free0, free1)
    # and a whole batch of that size is right afterwards
    sd = seeds(B, 11)
    some = list(range(0, B, 97)) + [B - 3, B - 1]
    out = mm.prove_batch(ctx, gs, sd)
    assert_same([out[i] for i in some], singles_of(pkg, ctx, [gs[i] for i in some], [sd[i] for i in some]))


def test_single_entry_instances():
    """n = 0: the batch takes the sequential path; whatever sc_prove does with a one-entry table, the batch does too"""
    pkg = load_package()
    ctx = ctx_of(pkg, GOLD)
    F = ctx.field
    mm = pkg.matrix_multiplication
    gs = [mm.G(pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, F.from_ints([3 + i])),
               pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 0, F.from_ints([5 + 2 * i]))) for i in range(4)]
    sd = seeds(4, 9)
    try:
        single = singles_of(pkg, ctx, gs, sd)
    except pkg.SumcheckHipError as e:
        with pytest.raises(pkg.SumcheckHipError) as ei:
            mm.prove_batch(ctx, gs, sd)
        assert ei.value.code == e.code
        return
    out, log = batch_log(ctx, lambda: mm.prove_batch(ctx, gs, sd))
    assert all(kind != "batch_pass" for kind, *_ in log)
    assert_same(out, single, "n=0")
    for i, (c1, ev, ch) in enumerate(out):
        assert c1 == F.from_int((3 + i) * (5 + 2 * i)) and ev.size == 0 and ch.size == 0, i


# ---- MatMult end to end -----------------------------------------------------------------------------------------------

def _only_one_rejected(pkg, ctx, n, pairs, k, seed_r=None):
    mm = pkg.matrix_multiplication
    proofs = mm.prove_products(ctx, n, pairs, seed_r=seed_r)
    for i, ((A, B), pf) in enumerate(zip(pairs, proofs)):
        assert pf.c_1 == pf.claim, i
        assert mm.verify_product(ctx, n, A, B, pf.C, pf), i
    bad = proofs[k].C.to_evaluations()
    bad[(5 << n) | 3] = (int(bad[(5 << n) | 3]) + 1) % ctx.field.p
    Cs = [pf.C for pf in proofs]
    Cs[k] = bad
    del bad
    again = mm.prove_products(ctx, n, pairs, Cs=Cs, seed_r=seed_r)
    for i, ((A, B), pf) in enumerate(zip(pairs, again)):
        assert mm.verify_product(ctx, n, A, B, Cs[i], pf) == (i != k), i
        assert (pf.c_1 == pf.claim) == (i != k), i


@pytest.mark.parametrize("p", [GOLD, P64], ids=fid)
def test_prove_products_n14(p):
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))   # (its own: the product's scratch goes back with it)
    n = 14
    try:
        pairs = [(pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_A + 20 + i, 2 * n),
                  pkg.DenseMultilinearExtension.generate(ctx, pyref.SEED_B + 20 + i, 2 * n)) for i in range(2)]
        _only_one_rejected(pkg, ctx, n, pairs, 1)
        del pairs
    finally:
        ctx.close()


def test_prove_products_many_pairs():
    pkg = load_package()
    ctx = ctx_of(pkg, P64)
    n, k = 10, 16
    ta = [pkg.DenseMultilinearExtension.generate(ctx, 0xAA00 + t, 2 * n) for t in range(k)]
    tb = [pkg.DenseMultilinearExtension.generate(ctx, 0xBB00 + t, 2 * n) for t in range(k)]
    pairs = [(ta[i % k], tb[i // k]) for i in range(k * k)]
    _only_one_rejected(pkg, ctx, n, pairs, 200, seed_r=seeds(k * k, 0x1234))
