"""Staged folded openings (sc_rs_fold_many, sc_ligero_fold_begin_staged; csrc/kernels/rs_fold.hpp):
one launch that folds up to three variables against repeated sc_rs_fold, bit for bit, at every length from one thread to
several blocks, on both field templates and on worst-case words; whole transcripts under a schedule against
tests/ligero_fold_staged_ref.py under fixed challenges; the whole protocol with the host FoldVerifier, honest and tampered; an
explicit all-ones schedule against the binary opening; the refusals, the launch log and the pool's books.

A reference commitment is built once per (field, shape) and shared by the tests that need it."""
import ctypes
import gc
import random

import numpy as np
import pytest

import ligero_fold_staged_ref as sref
import ligero_ref as ref
import wide_words
from ligero_common import context_cache, expect, mont_np
from test_gpu_sharded import Loopback

pytestmark = pytest.mark.gpu

GOLD, BABYBEAR, P64S18 = ref.GOLD, ref.BABYBEAR, ref.P64S18
IDS = {GOLD: "gold", BABYBEAR: "babybear", P64S18: "p64s18", 65537: "p65537", 257: "p257"}
CPU_SHAPES = [(3, 3, 1, (3,)), (5, 1, 1, (1,)), (6, 3, 1, (1, 2)), (6, 3, 1, (2, 1)), (7, 2, 2, (2,)), (8, 6, 1, (1, 3, 2)), (8, 7, 1, (3, 3, 1))]
SHAPES = CPU_SHAPES + [(10, 8, 1, (1, 3, 3, 1)), (16, 15, 1, (1, 3, 3, 3, 3, 2))]

ctx_of, _close_contexts = context_cache()
_commitments = {}


def teardown_module(module):
    _commitments.clear()
    _close_contexts(module)


def _id(v):
    return "".join(str(a) for a in v) if isinstance(v, tuple) else IDS.get(v, str(v))


# ---- 1. one launch, bit for bit --------------------------------------------------------------------------------------

def many_equals_repeated(pkg, p, words, alpha_sets):
    """sc_rs_fold_many of the RAW words against len(alphas) calls of sc_rs_fold"""
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    log_m = len(words).bit_length() - 1
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, log_m, words)
    for alphas in alpha_sets:
        alphas = [F.from_int(a) for a in alphas]
        got = lp.rs_fold_many(ctx, t, alphas).to_evaluations()
        want = t
        for a in alphas:
            want = lp.rs_fold(ctx, want, a)
        want = want.to_evaluations()
        assert got.size == len(words) >> len(alphas)
        assert np.array_equal(got, want), (p, log_m, alphas, int(np.flatnonzero(got != want)[0]))


def random_words(p, log_m):
    rng = random.Random("%d %d staged" % (p, log_m))
    return mont_np(p, [rng.randrange(p) for _ in range(1 << log_m)])


def alpha_sets(p, log_m, rng):
    """for every count that fits: one set from {0, 1, p - 1, random} in turn and one all random"""
    corner = [0, 1, p - 1, rng.randrange(p)]
    out = []
    for count in (1, 2, 3):
        if count + 1 <= log_m:
            out.append([corner[(log_m + count + k) % 4] for k in range(count)])
            out.append([rng.randrange(p) for _ in range(count)])
    return out


@pytest.mark.parametrize("log_m", range(2, 15))
def test_goldilocks_many_equals_repeated_folds(pkg, log_m):
    many_equals_repeated(pkg, GOLD, random_words(GOLD, log_m), alpha_sets(GOLD, log_m, random.Random(log_m)))


@pytest.mark.parametrize("p,log_m", [(p, l) for p in (BABYBEAR, 65537) for l in (4, 7, 13, 16)] + [(257, l) for l in range(4, 9)], ids=_id)
def test_generic_many_equals_repeated_folds(pkg, p, log_m):
    many_equals_repeated(pkg, p, random_words(p, log_m), alpha_sets(p, log_m, random.Random(p + log_m)))


def test_full_width_generic_field_on_worst_case_words(pkg):
    p, log_m = P64S18, 18                                       # 18 = s: the longest codeword this field has
    words = wide_words.edge_table(p, 1 << log_m, np.random.default_rng(18))
    many_equals_repeated(pkg, p, words, [[p - 1], [0, p - 1], [p - 1, random.Random(18).randrange(p), 1]])


def test_long_many_equals_repeated_folds(pkg):
    """2^22 words, three variables: the grid-stride loop runs"""
    ctx = ctx_of(pkg, GOLD)
    words = pkg.DenseMultilinearExtension.generate(ctx, 62, 22).to_evaluations()
    rng = random.Random(22)
    many_equals_repeated(pkg, GOLD, words, [[rng.randrange(GOLD) for _ in range(3)]])


# ---- 2. transcripts --------------------------------------------------------------------------------------------------

def reference_prover(p, n, c, rho, arities):
    """(table, a fresh RefStagedProver over the shared commitment of (p, n, c, rho))"""
    key = (p, n, c, rho)
    if key not in _commitments:
        rng = random.Random("%d %d %d %d" % key)
        table = [rng.randrange(p) for _ in range(1 << n)]
        _commitments[key] = (table, ref.RefProver(table, c, rho, p))
    table, commitment = _commitments[key]
    return table, sref.RefStagedProver(table, c, rho, p, arities, commitment=commitment)


def device_prover(pkg, p, n, c, rho):
    ctx = ctx_of(pkg, p)
    key = (p, n, c, rho)
    if key not in _commitments:
        reference_prover(p, n, c, rho, (1,) * c)
    poly = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, mont_np(p, _commitments[key][0]))
    return pkg.ligero_pcs.Prover.commit_long(ctx, poly, c, rho)


@pytest.mark.parametrize("n,c,rho,arities", SHAPES, ids=_id)
@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_staged_transcript_equals_the_reference(pkg, p, n, c, rho, arities):
    F = pkg.Field(p)
    rng = random.Random(n * 100 + c)
    _, want = reference_prover(p, n, c, rho, arities)
    prover = device_prover(pkg, p, n, c, rho)
    assert prover.root() == want.root()
    point = [rng.randrange(p) for _ in range(n)]
    gamma = [rng.randrange(p) for _ in range(1 << (n - c))]
    beta = rng.randrange(p)
    alphas = [rng.randrange(p) for _ in range(c)]
    top = 1 << (c + rho - arities[0])
    queries = [0, top - 1] + [rng.randrange(top) for _ in range(4)]
    opening = prover.fold_begin(ref.mont(p, point), ref.mont(p, gamma), arities)
    assert list(opening.claims) == ref.mont(p, want.begin(point, gamma))
    seen = []
    rounds, roots, challenges, final = opening.prove(F.from_int(beta), lambda i, e, root: seen.append((i, e, root)) or F.from_int(alphas[i]))
    w_rounds, w_roots, _, w_final = want.prove(beta, lambda i, e, root: alphas[i])
    assert rounds == [ref.mont(p, e) for e in w_rounds]
    assert roots == w_roots and len(roots) == len(arities) - 1
    assert challenges == ref.mont(p, alphas) and final == ref.mont(p, [w_final])[0]
    starts = sref.starts(arities)
    assert seen == [(i, rounds[i], roots[starts.index(i) - 1] if i and i in starts else None) for i in range(c)]    # what `draw` is shown
    got = opening.query(queries)
    for (q, cols, stages), (wq, w_cols, w_stages) in zip(got, want.query(queries)):
        assert q == wq and len(cols) == 1 << arities[0]
        for (j, vals, path), (wj, w_vals, w_sib) in zip(cols, w_cols):
            assert j == wj and vals == ref.mont(p, w_vals) and path.siblings == w_sib
        assert [(list(words), sib) for words, sib in stages] == [(ref.mont(p, words), sib) for words, sib in w_stages]
    opening.close()
    prover.close()


# ---- 3. the whole protocol -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,c,rho,arities", SHAPES, ids=_id)
@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_open_folded_with_a_schedule_is_accepted_with_the_value(pkg, p, n, c, rho, arities):
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    rng = random.Random(n + c)
    prover = device_prover(pkg, p, n, c, rho)
    point = [F.rand(rng) for _ in range(n)]
    v = lp.FoldVerifier(F, n, c, rho, prover.root(), 12, arities=arities)
    assert lp.open_folded(prover, v, point, rng) == prover.poly.evaluate(point)
    assert len(v.roots) == len(arities) - 1
    prover.close()


def test_the_limit_shape(pkg):
    """(n, c, rho) = (24, 23, 1) under (1, 3, 3, 3, 3, 3, 3, 3, 1): codewords of 2^24 words, two rows, eight trees"""
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, GOLD), pkg.Field(GOLD)
    rng = random.Random(24)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 11, 24)
    prover = lp.Prover.commit_long(ctx, poly, 23, 1)
    point = [F.rand(rng) for _ in range(24)]
    v = lp.FoldVerifier(F, 24, 23, 1, prover.root(), 4, arities=(1, 3, 3, 3, 3, 3, 3, 3, 1))
    assert lp.open_folded(prover, v, point, rng) == poly.evaluate(point)
    assert len(v.roots) == 8
    prover.close()


def test_an_explicit_all_ones_schedule_is_the_binary_opening(pkg):
    p, n, c, rho = GOLD, 16, 15, 1
    F = pkg.Field(p)
    rng = random.Random(161)
    prover = device_prover(pkg, p, n, c, rho)
    point, gamma = [F.rand(rng) for _ in range(n)], [F.rand(rng), F.rand(rng)]
    beta, alphas = F.rand(rng), [F.rand(rng) for _ in range(c)]
    queries = [0, (1 << c) - 1, 12345]
    out = []
    for arities in (None, (1,) * c):
        opening = prover.fold_begin(point, gamma, arities)
        seen = []
        proved = opening.prove(beta, lambda i, e, root: seen.append((i, e, root)) or alphas[i])
        out.append((opening.claims, proved, seen, opening.query(queries)))
        opening.close()
    (claims0, proved0, seen0, q0), (claims1, proved1, seen1, q1) = out
    assert claims0 == claims1 and proved0 == proved1 and seen0 == seen1          # sums, roots, challenges, final value
    for (q, lo, hi, layers), (qs, cols, stages) in zip(q0, q1):
        assert q == qs and layers == stages
        for (j, vals, path), (js, vals_s, path_s) in zip((lo, hi), cols):
            assert (j, vals, path.siblings) == (js, vals_s, path_s.siblings)
    prover.close()


def test_tampered_device_messages_are_refused(pkg):
    """the tamper cases of tests/test_ligero_fold_staged_cpu.py, once, on the device prover's messages"""
    lp, rp = pkg.ligero_pcs, pkg.relaxed_pcs
    p, n, c, rho, arities = GOLD, 8, 6, 1, (1, 3, 2)
    F = pkg.Field(p)
    prover = device_prover(pkg, p, n, c, rho)
    top = 1 << (c + rho - arities[0])

    def exchange(tamper):
        rng = random.Random(5)
        v = lp.FoldVerifier(F, n, c, rho, prover.root(), 8, arities=arities)
        point = [F.rand(rng) for _ in range(n)]
        opening = prover.fold_begin(point, v.draw_gamma(rng), arities)
        try:
            claims = list(opening.claims)
            if tamper in ("v", "v_gamma"):
                k = tamper == "v_gamma"
                claims[k] = F.add(claims[k], F.one)
            v.receive_claims(*claims)

            def draw(i, e, root):
                if (tamper == "round" and i == c - 1) or (tamper == "round0" and i == 0):
                    e[2 if tamper == "round" else 0] = F.add(e[2 if tamper == "round" else 0], F.one)
                if tamper == "root" and i == 4:
                    root = bytes([root[0] ^ 1]) + root[1:]
                if tamper == "stray_root" and i == 2:
                    root = bytes(32)
                return v.round(i, e, root, rng)

            final = opening.prove(v.draw_beta(rng), draw)[3]
            v.receive_final(F.add(final, F.one) if tamper == "final" else final)
            indices = v.draw_queries(rng)
            asked = list(indices)
            if tamper == "index":
                asked[2] = (asked[2] + 1) % top
            openings = opening.query(asked)
            q, cols, stages = openings[2]
            if tamper == "index":
                openings[2] = (indices[2], cols, stages)
            if tamper == "word":
                words, sib = stages[0]
                openings[2] = (q, cols, [(words[:5] + (F.add(words[5], F.one),) + words[6:], sib)] + stages[1:])
            if tamper == "path":
                words, sib = stages[-1]
                openings[2] = (q, cols, stages[:-1] + [(words, [bytes(32)] + sib[1:])])
            if tamper == "column":
                j, vals, path = cols[1]
                openings[2] = (q, [cols[0], (j, vals[:-1] + [F.add(vals[-1], F.one)], path)], stages)
            return v.verify(point, openings), prover.poly.evaluate(point)
        finally:
            opening.close()

    value, want = exchange(None)
    assert value == want
    for tamper, err in (("v", lp.RoundMismatch), ("v_gamma", lp.RoundMismatch), ("round0", lp.RoundMismatch), ("round", lp.EvalMismatch),
                        ("root", lp.MerkleMismatch), ("final", lp.EvalMismatch), ("word", lp.MerkleMismatch), ("path", lp.MerkleMismatch),
                        ("column", lp.MerkleMismatch), ("index", lp.MerkleMismatch), ("stray_root", rp.Error)):
        with pytest.raises(err):
            exchange(tamper)
    prover.close()


# ---- 4. refusals, the launch log, the pool's books -------------------------------------------------------------------

def begin_staged_raw(lp, lib, ctx_h, prover_h, z, gm, arities, stages=None):
    """the return code of sc_ligero_fold_begin_staged called with a raw schedule (None: a null pointer) and whether a handle came out"""
    h, claims = ctypes.c_void_p(), np.zeros(2, dtype=np.uint64)
    ar = None if arities is None else (ctypes.c_int32 * max(1, len(arities)))(*arities)
    rc = lib.sc_ligero_fold_begin_staged(ctx_h, prover_h, lp._u64p(z), lp._u64p(gm), ar, len(arities or ()) if stages is None else stages,
                                         lp._u64p(claims), ctypes.byref(h))
    return rc, bool(h.value)


def test_refusals(pkg):
    lp = pkg.ligero_pcs
    g, G = ctx_of(pkg, GOLD), pkg.Field(GOLD)
    rng = random.Random(3)
    poly = pkg.DenseMultilinearExtension.generate(g, 9, 6)
    point, gamma = [G.rand(rng) for _ in range(6)], [G.rand(rng) for _ in range(8)]
    prover = lp.Prover.commit(g, poly, 3, 1)
    z, gm = lp._words(point), lp._words(gamma)
    # the schedule: null, empty, an entry outside 1 .. 3, a sum other than c
    assert begin_staged_raw(lp, g.lib, g.h, prover.h, z, gm, None, stages=2) == (1, False)
    assert "schedule" in g.lib.sc_last_error(g.h).decode()
    assert begin_staged_raw(lp, g.lib, g.h, prover.h, z, gm, [3], stages=0) == (1, False)
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma, ()), "schedule")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma, (0, 3)), "1 .. 3")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma, (4,)), "1 .. 3")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma, (-1, 3, 1)), "1 .. 3")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma, (1, 1)), "log_cols is 3")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma, (2, 2)), "log_cols is 3")
    # the plain-opening shape, the other code, another context's commitment, null pointers, unreduced words
    flat = lp.Prover.commit(g, poly, 0, 1)
    expect(pkg, 1, lambda: flat.fold_begin(point, [G.rand(rng) for _ in range(64)], (1,)), "plain opening")
    flat.close()
    xc = lp.Prover.commit(g, poly, 3, 1, code="expander")
    expect(pkg, 6, lambda: xc.fold_begin(point, gamma, (1, 2)), "expander")
    xc.close()
    other = pkg.Context(G)
    assert begin_staged_raw(lp, other.lib, other.h, prover.h, z, gm, [1, 2]) == (1, False)
    assert "another context" in other.lib.sc_last_error(other.h).decode()
    other.close()
    assert begin_staged_raw(lp, g.lib, g.h, None, z, gm, [1, 2]) == (1, False)
    expect(pkg, 1, lambda: prover.fold_begin([GOLD] + point[1:], gamma, (1, 2)), "not reduced")
    expect(pkg, 1, lambda: prover.fold_begin(point, gamma[:-1] + [GOLD], (1, 2)), "not reduced")
    # the order of the calls, a refused prove, the indices
    opening = prover.fold_begin(point, gamma, (2, 1))
    expect(pkg, 5, lambda: opening.query([1]), "sc_ligero_fold_prove")
    expect(pkg, 1, lambda: opening.prove(GOLD, lambda i, e, root: 1), "beta")
    expect(pkg, 1, lambda: opening.prove(1, lambda i, e, root: GOLD if i == 1 else 1), "unreduced")
    with pytest.raises(ZeroDivisionError):
        opening.prove(1, lambda i, e, root: 1 // (2 - i))       # an exception in `draw` ends the call and comes back
    shown = []
    opening.prove(1, lambda i, e, root: shown.append(root is not None) or G.from_int(i + 2))     # (a refused prove leaves the opening where it was)
    assert shown == [False, False, True]
    expect(pkg, 5, lambda: opening.prove(1, lambda i, e, root: 1), "already")
    expect(pkg, 1, lambda: opening.query([3, 4]), "L / 4")       # L / 2^a_0 = 4
    assert len(opening.query([3])) == 1
    opening.close()
    prover.close()
    # sc_rs_fold_many: null pointers, the count, too short, unreduced, longer than the field's roots reach, longer than 2^24
    h = ctypes.c_void_p()
    one = lp._words([1])
    assert g.lib.sc_rs_fold_many(g.h, None, lp._u64p(one), 1, ctypes.byref(h)) == 1 and g.lib.sc_rs_fold_many(g.h, poly.h, lp._u64p(one), 1, None) == 1
    assert g.lib.sc_rs_fold_many(g.h, poly.h, None, 1, ctypes.byref(h)) == 1 and not h.value
    expect(pkg, 1, lambda: lp.rs_fold_many(g, poly, []), "1 .. 3")
    expect(pkg, 1, lambda: lp.rs_fold_many(g, poly, [1, 1, 1, 1]), "1 .. 3")
    expect(pkg, 1, lambda: lp.rs_fold_many(g, poly, [1, GOLD]), "not reduced")
    tiny = pkg.DenseMultilinearExtension.from_evaluations_vec(g, 3, G.from_ints(range(8)))
    expect(pkg, 1, lambda: lp.rs_fold_many(g, tiny, [1, 1, 1]), "at least 16")
    assert len(lp.rs_fold_many(g, tiny, [1, 1])) == 2
    f = ctx_of(pkg, 257)
    expect(pkg, 6, lambda: lp.rs_fold_many(f, pkg.DenseMultilinearExtension.generate(f, 1, 9), [1, 1]), "2-adicity 8", "257")
    expect(pkg, 6, lambda: lp.rs_fold_many(g, pkg.DenseMultilinearExtension.generate(g, 1, 25), [1]), "2^24")
    assert len(lp.rs_fold_many(g, poly, [1, 2, 3])) == 8          # the context still works


def test_sharded_and_multi_device_are_refused(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    g = ctx_of(pkg, GOLD)
    poly = pkg.DenseMultilinearExtension.generate(g, 9, 4)
    prover = lp.Prover.commit(g, poly, 2, 1)
    words = F.from_ints(range(16))
    z = lp._words(words[:4])
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, words)
    expect(pkg, 6, lambda: lp.rs_fold_many(m, mt, [1, 1]), "multi-device")
    assert begin_staged_raw(lp, m.lib, m.h, prover.h, z, z, [2]) == (6, False)
    del mt
    m.close()
    sh = pkg.Context(F)
    ar, ag = Loopback(2).collectives(0)
    sh.comm_init_host(0, 2, ar, ag)
    st = pkg.DenseMultilinearExtension.from_evaluations_vec(sh, 4, words)
    expect(pkg, 6, lambda: lp.rs_fold_many(sh, st, [1, 1]), "sharded")
    assert begin_staged_raw(lp, sh.lib, sh.h, prover.h, z, z, [2]) == (6, False)
    prover.close()


def test_launch_log(pkg):
    """(16, 15, 1) under (1, 3, 3, 3, 3, 2): one rs_fold_many launch and one tree per stage, the leaves hashed in the fold"""
    p, n, c, rho, arities = GOLD, 16, 15, 1, (1, 3, 3, 3, 3, 2)
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    rng = random.Random(16)
    prover = device_prover(pkg, p, n, c, rho)
    opening = prover.fold_begin([F.rand(rng) for _ in range(n)], [F.rand(rng), F.rand(rng)], arities)
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    opening.prove(F.rand(rng), lambda i, e, root: F.from_int(i + 3))
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    folds = [x for x in log if x["kind"] == "rs_fold_many"]
    assert len(folds) == len(arities) and not [x for x in log if x["kind"] == "rs_fold"]
    for s, (i, x) in enumerate(zip(sref.starts(arities), folds)):
        M = 1 << (c + rho - i)
        a, an = arities[s], arities[s + 1] if s + 1 < len(arities) else 0
        assert (x["kf"], x["ks"], x["log_in"]) == (a, c + rho - i, n), (s, x)
        assert (x["bytes_read"], x["bytes_written"]) == (8 * M, (8 * M >> a) + (32 * (M >> (a + an)) if an else 0)), (s, x)
    assert not [x for x in log if x["kind"] == "ligero" and x["kf"] == 0]
    # every tree ends in the top kernel: one merkle_finish per stage after the first
    assert [x["kf"] for x in log if x["kind"] == "merkle"].count(2) == len(arities) - 1
    # a query batch: one gather launch per stage after the first
    ctx.set_option("time_kernels", 1)
    ctx.launch_log()
    opening.query([0, 5, 77])
    log = ctx.launch_log()
    ctx.set_option("time_kernels", 0)
    assert len([x for x in log if x["kind"] == "ligero" and x["kf"] == 2]) == len(arities) - 1 + 1    # and the column opening's own
    opening.close()
    prover.close()


@pytest.mark.parametrize("p", [GOLD, BABYBEAR], ids=_id)
def test_pool_balance(pkg, p):
    lp = pkg.ligero_pcs
    ctx, F = ctx_of(pkg, p), pkg.Field(p)
    n, c, arities = 14, 12, (1, 3, 3, 3, 2)
    poly = pkg.DenseMultilinearExtension.generate(ctx, 3, n)

    def workload(refused):
        rng = random.Random(8)
        prover = lp.Prover.commit(ctx, poly, c, 1)
        point = [F.rand(rng) for _ in range(n)]
        if refused:
            expect(pkg, 1, lambda: prover.fold_begin(point, [p] * 4, arities))
            expect(pkg, 1, lambda: prover.fold_begin(point, [1] * 4, (1, 3, 3, 3, 3)))
            opening = prover.fold_begin(point, [F.rand(rng) for _ in range(4)], arities)
            expect(pkg, 1, lambda: opening.prove(1, lambda i, e, root: p if i == 5 else 1), "unreduced")      # refused half-way
            expect(pkg, 5, lambda: opening.query([0]))
            opening.close()
            expect(pkg, 1, lambda: lp.rs_fold_many(ctx, poly, [1, p]))
        else:
            v = lp.FoldVerifier(F, n, c, 1, prover.root(), 4, arities=arities)
            assert lp.open_folded(prover, v, point, rng) == poly.evaluate(point)
            folded = lp.rs_fold_many(ctx, poly, [1, 2, 3])
            del folded
        prover.close()

    workload(False)                         # (the tables of this length are workspace of the context, made here)
    gc.collect()
    books = ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")
    for refused in (False, True):
        workload(refused)
        gc.collect()
        assert (ctx.get_option("stat_pool_live_blocks"), ctx.get_option("stat_pool_live_words")) == books, refused
    assert len(lp.rs_fold_many(ctx, poly, [1, 1, 1])) == 1 << (n - 3)
