"""Every form of the product prover's passes on worst-case words, for every kind of field.

The device arithmetic of csrc/field.hpp is a second implementation (hand-scheduled sub4 / sub2 / acc_mac / acc3_mac beside the
plain C of the host branch, which tests/test_field_host.py pins), and its correcting branches are rare on uniform residues: a
Goldilocks sum that lands in [p, 2^64), or a borrow that leaves a low limb of 0xFFFFFFFF, is one case in 2^32.  Here every launch
meets them: the tables are wide_words.octet_table (aligned octets whose differences at strides 1, 2, 4 - the ones extend_quads,
the three-round extension and the one-challenge fold take - sit on every corner of wide_words.classes_of) with
wide_words.degenerate_challenges (r = 0 / one hand the even / odd entries on, so the patterns reach the extension step of a
pass that folds first), wide_words.edge_table with edge challenges, and all p-1 against all p-1.  One more input carries the
octets through a pass with MORE than one pending challenge: a fold by the cycle 0, one, p-1, 1 mixes the entries, so the extension
step of pass_kernel<3, 2>, <4, 2> or wfold_pass_kernel<4, 5> would see ordinary residues; octet_table(shift = kf) with
select_challenges (kf challenges that are each 0 or one) puts the octets where the row's second launch, after its fold, extends.
tests/test_oracle_wide_moduli.py pins the C oracle on these inputs against big integers; every check here is bit for bit
against that oracle.

ROWS lists one schedule per form of pass_kernel / wfold_pass_kernel / wgrid_pass_kernel at the smallest size where the form
exists (or walks more than one tile); each row asserts that the launch log is the planner's plan and that the (kind, kf, ks) it
exists for were launched, so a planner change that routes round a kernel fails here.  The launch log does not say which FORM of
a (kf, ks) ran; the rule is launch_pass_t's (engine/launch.inc) and the rows pin its inputs:
  - (3, 2) pipelined: option pipe32 = 1, whole tiles, log_in >= pipe32_log (row f: 13 >= 11) - every field; pipe32 = 0: staged.
  - (4, 2) LDS-DMA: option fold_dma = 1 AND Goldilocks.  The form is unreachable for the generic field (MontGeneric's constants
    do not leave it the registers): on the five generic moduli row g runs the staged pass_kernel<4, 2> under both values of
    fold_dma - form_of says so by name and the test asserts the name it expects for the field.
  - NT: rows a-d and g-k run again with nt_load_log = nt_store_log = 8: every pass on a table of >= 2^8 entries is then the
    NT = 1 (kf = 0) or NT = 3 instantiation of pass_kernel, NT = true of wfold_pass_kernel / the streaming loads of the rest."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_package
from test_gpu_wide_moduli import edge_challenges
from util import GOLD, oracle, verifier_identities
from wide_words import WIDE, degenerate_challenges, edge_table, octet_table, select_challenges, wid

pytestmark = pytest.mark.gpu

MODULI = WIDE + [GOLD]
P63 = 2**63 + 29

_H = {"first_pass_vars": 4, "wfold_min_log": 12, "wfold5_min_log": 12, "wfold_always": 1}
_J = {"first_pass_vars": 4, "wfold_min_log": 12, "wfold5_min_log": 12, "grid_log": 4, "host_tail_log": 0}
_NT = {"nt_load_log": 8, "nt_store_log": 8}
_STAGED = {"grid_pass": 0, "host_tail_log": 0}

# row: (n, options, the (kind, kf, ks) the row exists for)
ROWS = {
    "a": (13, dict(_STAGED, vars_per_pass=1), [("pass", 0, 1), ("pass", 1, 1)]),
    "b": (13, dict(_STAGED, first_pass_vars=1), [("pass", 0, 1), ("pass", 1, 2)]),
    "c": (13, dict(_STAGED, first_pass_vars=2), [("pass", 0, 2), ("pass", 2, 2), ("pass", 2, 1)]),
    "d": (14, dict(_STAGED, first_pass_vars=3), [("pass", 0, 3), ("pass", 3, 2), ("pass", 2, 1)]),
    "e": (4, dict(_STAGED, first_pass_vars=3), [("pass", 0, 3), ("pass", 3, 1)]),             # pass(3, 1): its only size
    "f": (13, {"gram_log": 0, "first_pass_vars": 3, "grid_log": 7, "pipe32_log": 11}, [("pass", 0, 3), ("pass", 3, 2), ("grid_pass", 2, 3)]),
    "g": (14, {"first_pass_vars": 4, "grid_log": 8}, [("gram_pass", 0, 4), ("pass", 4, 2), ("grid_pass", 2, 4)]),
    "h": (16, _H, [("gram_pass", 0, 4), ("wfold_pass", 4, 5), ("grid_pass", 5, 4)]),         # one block
    "i": (17, dict(_H, host_tail_log=0), [("wfold_pass", 4, 5), ("wfold_pass", 5, 4)]),
    "j": (18, _J, [("wfold_pass", 4, 5), ("wfold_pass", 5, 5)]),
    "k": (19, _J, [("wfold_pass", 4, 5), ("wfold_pass", 5, 3), ("pass", 3, 2)]),
    "l": (20, dict(_H, max_blocks=3), [("wfold_pass", 4, 5)]),                              # many tiles per block
    "m": (16, {"host_tail_log": 0}, [("grid_pass", 0, 4), ("grid_pass", 4, 4)]),             # the device alone, wgrid
}


def _cases():
    out = []
    for row, (n, opts, named) in ROWS.items():
        variants = [("", {})]
        if row == "f":
            variants = [("pipe32=1", {"pipe32": 1}), ("pipe32=0", {"pipe32": 0})]
        if row == "g":
            variants = [("fold_dma=1", {"fold_dma": 1}), ("fold_dma=0", {"fold_dma": 0})]
        if row in "abcdghijk":
            variants = variants + [((name + ",nt").lstrip(","), dict(extra, **_NT)) for name, extra in variants]
        for name, extra in variants:
            out.append(pytest.param(row, n, dict(opts, **extra), named, id=row + ("-" + name if name else "")))
    return out


def form_of(p, kf, ks, log_in, get):
    """the form of pass_kernel<kf, ks> that launch_pass_t takes, from the field and the context's options (get = ctx.get_option)"""
    if (kf, ks) == (4, 2) and p == GOLD and get("fold_dma"):
        return "lds_dma"
    if (kf, ks) == (3, 2) and get("pipe32") and log_in >= get("pipe32_log") and log_in >= 11:      # (whole tiles: 2^(log_in - 5) runs, a multiple of 64)
        return "pipelined"
    return "staged"


def plan_keys(pkg):
    return [k for k, _ in pkg._lib.ScPlanOptions._fields_ if k != "struct_size"]


def plan_str(plan):
    return " ".join("%s(%d,%d)@%d" % (s["action"], s["kf"], s["ks"], s["log_in"]) for s in plan)


@functools.lru_cache(maxsize=8)
def inputs(p, n):
    """the three inputs of a (modulus, size) with the oracle's transcript, computed once and shared by the rows of that size:
    [(name, a, b, challenges, ref)]"""
    o = oracle(p)
    rng = np.random.default_rng([p % 1000003, n])
    size = 1 << n
    ins = [("octet", octet_table(p, size, rng), octet_table(p, size, rng), degenerate_challenges(p, n)),
           ("edge", edge_table(p, size, rng), edge_table(p, size, rng), edge_challenges(p, n, rng)),
           ("pm1", np.full(size, p - 1, dtype=np.uint64), np.full(size, p - 1, dtype=np.uint64), [p - 1 - (j % 3) for j in range(n)])]
    out = []
    for name, a, b, ch in ins:
        ch = np.array(ch, dtype=np.uint64)
        ref = o.prove(a, b, ch)
        assert ref["status"] == 0, (p, n, name)
        for arr in (a, b, ch):
            arr.setflags(write=False)
        out.append((name, a, b, ch, ref))
    return out


@functools.lru_cache(maxsize=8)
def deep_input(p, n, kf):
    """octet tables whose octets sit kf index bits up, kf challenges of 0 / one and then the degenerate cycle: the fold by the
    first kf challenges leaves octet tables for the extension step of a pass with kf pending challenges"""
    rng = np.random.default_rng([p % 1000003, n, kf])
    a, b = octet_table(p, 1 << n, rng, shift=kf), octet_table(p, 1 << n, rng, shift=kf)
    ch = np.array((select_challenges(p, kf) + degenerate_challenges(p, n))[:n], dtype=np.uint64)
    ref = oracle(p).prove(a, b, ch)
    assert ref["status"] == 0, (p, n, kf)
    for arr in (a, b, ch):
        arr.setflags(write=False)
    return ("deep%d" % kf, a, b, ch, ref)


def run_inputs(pkg, ctx, p, n, kf, log_plan=None):
    """the three inputs and the deep one through prove_and_check; every input runs, the failures are reported together (which
    input and which round went wrong first is what tells a wrong fold from a wrong extension)"""
    failures = []
    for inp in inputs(p, n) + [deep_input(p, n, kf)]:
        try:
            prove_and_check(pkg, ctx, p, n, inp, log_plan=log_plan, rounds=inp[0] == "octet" or inp[0].startswith("deep"))
        except AssertionError as e:
            failures.append(str(e).split("\n")[0])
    assert not failures, failures


def prove_and_check(pkg, ctx, p, n, inp, log_plan=None, rounds=False):
    """one input through sc_prove on ctx: c_1, every evals[j] and g.evaluate(ch) bit for bit the oracle's, every word below p,
    the verifier's identities; log_plan: the launches must be exactly these (kind, kf, ks, log_in); rounds: also round by round
    through the native prover, which reads the launches' cached cells"""
    name, ta, tb, ch, ref = inp
    tag = (wid(p), n, name)
    F = ctx.field
    a = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, ta)
    b = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, tb)
    g = pkg.matrix_multiplication.G(a, b)
    it = iter(ch)
    if log_plan is not None:
        ctx.launch_log(reset=True)
    c1, evals, chn = pkg.matrix_multiplication.prove(ctx, g, 0, draw=lambda _u, _j, _e: int(next(it)))
    if log_plan is not None:
        log = [(r["kind"], r["kf"], r["ks"], r["log_in"]) for r in ctx.launch_log(reset=True)]
        assert log == log_plan, (tag, log)
    assert np.array_equal(chn, ch), tag
    assert c1 == ref["c_1"], (tag, "c_1")
    for j in range(n):
        assert [int(x) for x in evals[j]] == [int(x) for x in ref["evals"][j]], (tag, j)
    final = g.evaluate([int(x) for x in ch])
    assert final == ref["final_eval"], tag
    assert c1 < p and final < p and int(evals.max()) < p, tag
    assert verifier_identities(F, c1, evals, ch, final) is None, tag
    if rounds:
        pr = g.native_prover()
        assert pr.c1() == ref["c_1"], tag
        for j in range(n):
            e = pr.round_evals(int(ch[j - 1]) if j else F.one, j)
            assert e == [int(x) for x in ref["evals"][j]] and max(e) < p, (tag, j)
        del pr
    del g, a, b


@pytest.mark.parametrize("row,n,opts,named", _cases())
@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_pass_forms_on_edge_words(p, row, n, opts, named):
    pkg = load_package()
    plan = pkg.schedule.plan_proof(n, **{k: v for k, v in opts.items() if k in plan_keys(pkg)})
    steps = [(s["action"], s["kf"], s["ks"], s["log_in"]) for s in plan if s["action"] != "host_tail"]
    assert not any(s["sharded"] for s in plan)
    for form in named:
        assert form in [s[:3] for s in steps], (row, form, plan_str(plan))
    ctx = pkg.Context(pkg.Field(p))
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
            assert ctx.get_option(k) == v
        # the forms the log cannot tell apart, by name (see the module docstring)
        if row == "f":
            assert form_of(p, 3, 2, 13, ctx.get_option) == ("pipelined" if opts["pipe32"] else "staged")
        if row == "g":   # the LDS-DMA form is Goldilocks only: the generic field runs the staged <4, 2> whatever fold_dma says
            assert form_of(p, 4, 2, 14, ctx.get_option) == ("lds_dma" if p == GOLD and opts["fold_dma"] else "staged")
        if row == "d":
            assert form_of(p, 3, 2, 14, ctx.get_option) == "staged"      # pipe32_log is 20 by default
        ctx.set_option("time_kernels", 1)
        run_inputs(pkg, ctx, p, n, plan[1]["kf"], log_plan=steps)
    finally:
        ctx.close()


# rows h and k on the shards of a multi-device handle (entries of device 0): the shards' cells are added by the host.  n: the
# smallest at which the plan of the handle still has a sharded wfold_pass (shards of 2^12 entries for row h, where the first
# pass of so small a shard is a grid pass; 2^16 for row k, whose second wfold pass needs 2^12 folded entries)
@pytest.mark.parametrize("row,devs,n,want", [
    ("h", 2, 13, "grid_pass(0,4)@12 wfold_pass(4,5)@12 grid_pass(5,3)@8 host_tail(3,1)@3"),
    ("h", 8, 15, "grid_pass(0,4)@12 wfold_pass(4,5)@12 grid_pass(5,3)@8 host_tail(3,3)@3"),
    ("k", 2, 17, "gram_pass(0,4)@16 wfold_pass(4,5)@16 wfold_pass(5,4)@12 grid_pass(4,3)@7 host_tail(3,1)@3"),
    ("k", 8, 19, "gram_pass(0,4)@16 wfold_pass(4,5)@16 wfold_pass(5,4)@12 grid_pass(4,3)@7 host_tail(3,3)@3")],
    ids=["h-2", "h-8", "k-2", "k-8"])
@pytest.mark.parametrize("p", [GOLD, P63], ids=wid)
def test_wfold_rows_on_a_handle(p, row, devs, n, want):
    pkg = load_package()
    opts = ROWS[row][1]
    popts = {k: v for k, v in opts.items() if k in plan_keys(pkg)}
    plan = pkg.schedule.plan_proof(n, devs, "local", **popts)
    assert plan_str(plan) == want and all(s["sharded"] for s in plan), plan_str(plan)
    smaller = pkg.schedule.plan_proof(n - 1, devs, "local", **popts)
    assert not any(s["action"] == "wfold_pass" for s in smaller), plan_str(smaller)
    ctx = pkg.Context(pkg.Field(p), devices=[0] * devs)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        run_inputs(pkg, ctx, p, n, plan[1]["kf"])
    finally:
        ctx.close()


def fold_and_sums(pkg, g, r):
    """sc_prod2_fold_and_sums: (G folded by r, the three round sums of the folded G)"""
    ctx = g.ctx
    rr = (ctypes.c_uint64 * 1)(int(r))
    ha, hb = ctypes.c_void_p(), ctypes.c_void_p()
    e = (ctypes.c_uint64 * 3)()
    ctx.check(ctx.lib.sc_prod2_fold_and_sums(ctx.h, g.f_a.h, g.f_b.h, rr, ctypes.byref(ha), ctypes.byref(hb), e))
    DM = pkg.DenseMultilinearExtension
    return pkg.matrix_multiplication.G(DM(ctx, ha), DM(ctx, hb)), [int(x) for x in e]


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_trait_calls_on_octet_tables(p):
    """test_gpu_parity.py::test_trait_methods_vs_oracle on octet tables: sc_prod2_sum, round_sums, fold_and_sums (every r of
    degenerate_challenges), evaluate and to_evaluations against the oracle"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    o = oracle(p)
    DM = pkg.DenseMultilinearExtension
    rng = np.random.default_rng(p % 1039)
    for n in (1, 6, 13):
        oa, ob = octet_table(p, 1 << n, rng), octet_table(p, 1 << n, rng)
        a, b = DM.from_evaluations_vec(ctx, n, oa), DM.from_evaluations_vec(ctx, n, ob)
        g = pkg.matrix_multiplication.G(a, b)
        assert g.num_vars() == n
        assert np.array_equal(g.to_evaluations(), o.to_evaluations(oa, ob)), n
        assert g.hypercube_sum() == o.c1(oa, ob), n
        e = o.round_evals(oa, ob)
        assert g.round_evals() == [int(x) for x in e] and int(max(e)) < p, n
        dense = [0, 0, 0]
        for d, c in g.to_univariate().coeffs:
            dense[d] = c
        assert dense == [int(x) for x in o.interpolate(e)], n
        for r in degenerate_challenges(p, 6):
            fa, fb = o.fix_variables(oa, [r]), o.fix_variables(ob, [r])
            g2 = g.fix_variables([r])
            assert np.array_equal(g2.f_a.to_evaluations(), fa) and np.array_equal(g2.f_b.to_evaluations(), fb), (n, r)
            if n >= 2:
                g3, sums = fold_and_sums(pkg, g, r)
                assert np.array_equal(g3.f_a.to_evaluations(), fa) and np.array_equal(g3.f_b.to_evaluations(), fb), (n, r)
                assert sums == [int(x) for x in o.round_evals(fa, fb)] and max(sums) < p, (n, r)
                del g3
            del g2
        for pt in (degenerate_challenges(p, n), edge_challenges(p, n, rng)):
            got = g.evaluate(pt)
            assert got == o.g_evaluate(oa, ob, pt) and got < p, n
        assert g.evaluate(degenerate_challenges(p, n)[:-1]) is None
        assert np.array_equal(a.to_evaluations(), oa) and np.array_equal(b.to_evaluations(), ob)      # inputs never modified
        del g, a, b
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_fold_identities_on_octet_tables(p):
    """no oracle: folding by 0 keeps the even entries, folding by the field's one keeps the odd entries, and
    sc_prod2_fold_and_sums with those r folds the same way and returns the round sums of the tables so folded"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    DM = pkg.DenseMultilinearExtension
    n = 13
    rng = np.random.default_rng(p % 1049)
    oa, ob = octet_table(p, 1 << n, rng), octet_table(p, 1 << n, rng)
    a, b = DM.from_evaluations_vec(ctx, n, oa), DM.from_evaluations_vec(ctx, n, ob)
    g = pkg.matrix_multiplication.G(a, b)
    assert F.one == 2**64 % p
    for r, first in ((0, 0), (F.one, 1)):
        ha, hb = np.ascontiguousarray(oa[first::2]), np.ascontiguousarray(ob[first::2])
        assert np.array_equal(a.fix_variables([r]).to_evaluations(), ha), r
        assert np.array_equal(b.fix_variables([r]).to_evaluations(), hb), r
        g3, sums = fold_and_sums(pkg, g, r)
        assert np.array_equal(g3.f_a.to_evaluations(), ha) and np.array_equal(g3.f_b.to_evaluations(), hb), r
        halved = pkg.matrix_multiplication.G(DM.from_evaluations_vec(ctx, n - 1, ha), DM.from_evaluations_vec(ctx, n - 1, hb))
        assert sums == halved.round_evals() == g3.round_evals(), r
        del g3, halved
    del g, a, b
    ctx.close()
