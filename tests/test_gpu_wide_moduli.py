"""The generic-field build (MontGeneric) of every kernel family at full word width.  With the toy moduli every residue is below
2^21: the high half of each word is zero, the upper limbs of the 160-bit accumulator never carry and the carry-out branches of
add / redc never run.  Here the tables and challenges mix uniform residues with the words where those carries happen
(util.edge_words: 0, 1, p-1, p-2, (p-1)/2, R mod p, 2^32 +- 1, 2^32, 2^63, 0xFFFFFFFF00000000 - each where it is below p), over
the moduli of util.WIDE (p > 2^63 down to p < 2^32, tests/test_oracle_wide_moduli.py pins the oracle on them) and Goldilocks,
and every check is bit for bit against the C oracle or pyref: the triangle prover (engine, trait path, the three matrix-square
paths, the one-call prover, sharded), the GKR W prover (dense shapes, wiring-built layers dense against sparse, colliding
wiring, the protocol, the device-resident circuit, sharded), the table calls on a context and on a two-entry handle, and the
sharded product prover whose cells cross the ranks as 32-bit limbs."""
import random
import threading

import numpy as np
import pytest

from conftest import load_package
from test_gpu_gkr import make_circuit, random_circuit
from test_gpu_gkr_circuit import edge_circuit, ks_of, np_layers, prove_and_check
from test_gpu_gkr_protocol import compare, run_protocol
from test_gpu_sharded import Loopback, run_virtual_ranks
from test_host_protocols import gkr_draw_count
from util import GOLD, challenges, oracle, pyref
from wide_words import WIDE, edge_table, wid

pytestmark = pytest.mark.gpu

MODULI = WIDE + [GOLD]


def edge_challenges(p, n, rng):
    """n raw challenge words: p-1 and p-2 first, then edge words and uniform residues"""
    ch = edge_table(p, n, rng)
    ch[:2] = [p - 1, p - 2][:n]
    return [int(x) for x in ch]


def canon(F, words):
    return [F.to_int(w) for w in words]


def run_threads(world, body):
    errors = []

    def wrapped(rank):
        try:
            body(rank)
        except Exception as e:  # pragma: no cover
            import traceback
            traceback.print_exc()
            errors.append(e)

    threads = [threading.Thread(target=wrapped, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors


# ---- triangle ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_triangle_engine_and_trait_path(p):
    """k = 1..4 on field-valued tables of edge words: the engine round by round, the generic fix_variables -> round_evals
    path, and fix_variables across the x/y/z boundaries (test_gpu_triangle.py::test_vs_oracle on 0/1 tables)"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    o = oracle(p)
    rng = np.random.default_rng(p % 997)
    for k in (1, 2, 3, 4):
        ev = edge_table(p, 1 << (2 * k), rng)
        t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * k, ev)
        g = pkg.triangle_counting.G(t, t, t, k)
        ch = edge_challenges(p, 3 * k, rng)
        ref = o.tri_prove(ev, k, ch)
        assert ref["status"] == 0
        eng = g.native_prover()
        assert eng.c1() == ref["c_1"], k
        for j in range(3 * k):
            assert eng.round_evals(ch[j - 1] if j else F.one, j) == [int(x) for x in ref["evals"][j]], (k, j)
        assert g.evaluate(ch) == ref["final_eval"]
        cur = g
        assert cur.hypercube_sum(F) == ref["c_1"]
        if k <= 3:
            assert np.array_equal(cur.to_evaluations(), o.tri_to_evaluations(ev, ev, ev, k))
        for j in range(3 * k):
            if j:
                cur = cur.fix_variables([ch[j - 1]])
            assert cur.round_evals() == [int(x) for x in ref["evals"][j]], (k, j)
        for kk in sorted({1, k, k + 1, 2 * k, 2 * k + 1, 3 * k - 1} - {3 * k}):
            g2 = g.fix_variables(ch[:kk])
            assert g2.num_vars() == 3 * k - kk and g2.evaluate(ch[kk:]) == ref["final_eval"], (k, kk)
        del eng, g, t
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_triangle_matrix_square_paths(p):
    """the square of the adjacency matrix at k = 6 and 7: a directed 0/1 table (words 0 and R mod p) on the int8 matrix cores,
    a table of edge words on the tiled field kernel, a 0/1 table with one p-1 entry that has to fall back to the tiled kernel;
    engine, final evaluation and the one-call triangle_counting.prove"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    o = oracle(p)
    rng = np.random.default_rng(p % 991)
    for k, kind in [(6, "directed"), (7, "directed"), (6, "field"), (7, "field"), (6, "almost01")]:
        n = 1 << k
        if kind == "field":
            ev = edge_table(p, n * n, rng)
        else:
            ev = np.where(rng.random(n * n) < 0.4, F.one, 0).astype(np.uint64)
            if kind == "almost01":
                ev[rng.integers(0, n * n)] = p - 1
        t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * k, ev)
        g = pkg.triangle_counting.G(t, t, t, k)
        ch = edge_challenges(p, 3 * k, rng)
        ref = o.tri_prove(ev, k, ch)
        assert ref["status"] == 0
        eng = g.native_prover()
        assert eng.c1() == ref["c_1"], (k, kind)
        for j in range(3 * k):
            assert eng.round_evals(ch[j - 1] if j else F.one, j) == [int(x) for x in ref["evals"][j]], (k, kind, j)
        assert g.evaluate(ch) == ref["final_eval"], (k, kind)
        it = iter(ch)
        c1, evals, _ = pkg.triangle_counting.prove(ctx, g, 0, draw=lambda _u, _j, _e: int(next(it)))
        assert c1 == ref["c_1"] and np.array_equal(evals, ref["evals"]), (k, kind)
        del eng, g, t
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_triangle_sharded_host(p):
    """the triangle engine on two ranks over host collectives, tables of edge words"""
    pkg = load_package()
    o = oracle(p)
    world = 2
    rng = np.random.default_rng(p % 983)
    for k in (3, 6):
        flat = edge_table(p, 1 << (2 * k), rng)
        ch = edge_challenges(p, 3 * k, rng)
        ref = o.tri_prove(flat, k, ch)
        lb = Loopback(world)
        results = [None] * world

        def body(rank):
            ctx = pkg.Context(pkg.Field(p))
            try:
                ar, ag = lb.collectives(rank)
                ctx.comm_init_host(rank, world, ar, ag)
                n_loc = flat.size // world
                shard = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 2 * k - 1, flat[rank * n_loc:(rank + 1) * n_loc])
                g = pkg.triangle_counting.G(shard, shard, shard, k)
                eng = pkg.triangle_counting._NativeTriProver(g)
                got = [eng.c1()]
                for j in range(3 * k):
                    got.append(eng.round_evals(ch[j - 1] if j else ctx.field.one, j))
                results[rank] = got
                del eng, g, shard
            except Exception:
                lb.barrier.abort()
                raise
            finally:
                ctx.close()

        run_threads(world, body)
        for got in results:
            assert got[0] == ref["c_1"], k
            assert got[1:] == [[int(x) for x in e] for e in ref["evals"]], k


# ---- GKR W ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_w_general_shapes(p):
    """dense add / mul / W tables of edge words at every (kb, kc) split of test_gpu_gkr.py::test_w_prover_general_shapes,
    against pyref.w_transcript; and the tail of the transcript from a W with variables already fixed"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    gp = pkg.gkr_protocol
    DM = pkg.DenseMultilinearExtension
    rng = np.random.default_rng(p % 1013)
    for kb, kc in [(1, 1), (3, 5), (5, 2), (0, 4), (4, 0), (1, 6), (6, 1), (2, 2)]:
        n = kb + kc
        add, mul = edge_table(p, 1 << n, rng), edge_table(p, 1 << n, rng)
        wb, wc = edge_table(p, 1 << kb, rng), edge_table(p, 1 << kc, rng)
        ch = edge_challenges(p, n, rng)
        ref = pyref.w_transcript(canon(F, add), canon(F, mul), canon(F, wb), canon(F, wc), canon(F, ch), p)
        w = gp.W(DM.from_evaluations_vec(ctx, n, add), DM.from_evaluations_vec(ctx, n, mul),
                 DM.from_evaluations_vec(ctx, kb, wb), DM.from_evaluations_vec(ctx, kc, wc))
        eng = w.native_prover()
        assert F.to_int(eng.c1()) == ref["c_1"], (kb, kc)
        for j in range(n):
            e = eng.round_evals(ch[j - 1] if j else F.one, j)
            assert canon(F, e) == ref["evals"][j], (kb, kc, j)
        assert F.to_int(w.evaluate(ch)) == ref["final_eval"], (kb, kc)
        for t in sorted({1, kb, min(kb + 1, n - 1)} - {0, n}):
            eng2 = w.fix_variables(ch[:t]).native_prover()
            for j in range(n - t):
                e = eng2.round_evals(ch[t + j - 1] if j else F.one, j)
                assert canon(F, e) == ref["evals"][t + j], (kb, kc, t, j)
        del eng, w
    ctx.close()


def edge_inputs(F, p, n, rng):
    """n canonical ints whose Montgomery words are edge words or uniform residues"""
    return canon(F, edge_table(p, n, rng))


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_w_random_circuits_dense_sparse_oracle(p):
    """wiring-built layers: the dense prover (wiring scatter), the per-gate sparse prover and the oracle's wiring tables and
    transcript agree round by round on edge-word inputs and points"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    o = oracle(p)
    gp = pkg.gkr_protocol
    rng = random.Random(p % 97)
    nrng = np.random.default_rng(p % 89)
    for ks in ([1, 1], [2, 3], [3, 2], [4, 4], [6, 5], [5, 6]):
        layers = random_circuit(rng, ks)
        circuit = make_circuit(pkg, layers, 1 << ks[-1])
        evaluation = circuit.evaluate(F, [int(x) for x in edge_table(p, 1 << ks[-1], nrng)])
        k_i, k_next = ks[0], ks[1]
        r_i = edge_challenges(p, k_i, nrng)
        w = gp.start_round_w(ctx, circuit, evaluation, 0, r_i)
        oadd, omul = o.wiring_fixed(layers[0], k_next, r_i)
        assert np.array_equal(w.add_i.to_evaluations(), oadd) and np.array_equal(w.mul_i.to_evaluations(), omul), ks
        ow = np.array(evaluation[1], dtype=np.uint64)
        ch = edge_challenges(p, 2 * k_next, nrng)
        ref = o.w_prove(oadd, omul, ow, ow, ch)
        assert ref["status"] == 0
        dense, sparse = w.native_prover(), gp.SparseLayerProver(ctx, circuit, evaluation, 0, r_i)
        assert dense.c1() == sparse.c1() == ref["c_1"], ks
        for j in range(2 * k_next):
            rp = ch[j - 1] if j else F.one
            e = [int(x) for x in ref["evals"][j]]
            assert dense.round_evals(rp, j) == e and sparse.round_evals(rp, j) == e, (ks, j)
        assert w.evaluate(ch) == ref["final_eval"], ks
        del dense, sparse, w
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_w_wiring_collisions_wrap(p):
    """2^7 gates wired to two (b, c) slots, with r_i made of p-1, p-2 and other edge words: the eq weights of the gates are
    large residues, and the compare-and-swap modular add of the wiring scatter (atomic_add_mod) wraps many times"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    o = oracle(p)
    gp = pkg.gkr_protocol
    nrng = np.random.default_rng(p % 83)
    k_i, k_next = 7, 2
    layers = [[(("add" if a % 3 else "mul"), a % 2, 1) for a in range(1 << k_i)]]
    circuit = make_circuit(pkg, layers, 1 << k_next)
    for r_i in ([p - 1] * k_i, [p - 2, p - 1] * 3 + [p - 1], edge_challenges(p, k_i, nrng)):
        add_d, mul_d = gp.wiring(ctx, circuit, 0, r_i)
        oadd, omul = o.wiring_fixed(layers[0], k_next, r_i)
        assert np.array_equal(add_d.to_evaluations(), oadd) and np.array_equal(mul_d.to_evaluations(), omul), r_i
        evaluation = circuit.evaluate(F, [int(x) for x in edge_table(p, 1 << k_next, nrng)])
        ow = np.array(evaluation[1], dtype=np.uint64)
        ch = edge_challenges(p, 2 * k_next, nrng)
        ref = o.w_prove(oadd, omul, ow, ow, ch)
        dense = gp.start_round_w(ctx, circuit, evaluation, 0, r_i).native_prover()
        sparse = gp.SparseLayerProver(ctx, circuit, evaluation, 0, r_i)
        assert dense.c1() == sparse.c1() == ref["c_1"]
        for j in range(2 * k_next):
            rp = ch[j - 1] if j else F.one
            e = [int(x) for x in ref["evals"][j]]
            assert dense.round_evals(rp, j) == e and sparse.round_evals(rp, j) == e, j
        del dense, sparse, add_d, mul_d
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_gkr_protocol_end_to_end(p):
    """the whole GKR protocol through the host Prover / Verifier mirrors, dense and sparse layer provers, against
    pyref.gkr_transcript message by message; inputs and draws are edge words"""
    pkg = load_package()
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    rng = random.Random(p % 1000)
    nrng = np.random.default_rng(p % 79)
    for ks in ([1, 2, 3, 2], [2, 3, 4, 4, 3], [1, 1, 1, 1]):
        layers = random_circuit(rng, ks)
        num_inputs = 1 << ks[-1]
        inputs = edge_inputs(F, p, num_inputs, nrng)
        draws = edge_inputs(F, p, gkr_draw_count(layers, num_inputs), nrng)
        ref = pyref.gkr_transcript(layers, num_inputs, inputs, draws, p)
        assert ref["check_input"]
        for sparse in (False, True):
            rec, _ = run_protocol(pkg, ctx, layers, num_inputs, inputs, draws, sparse)
            compare(rec, ref)
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_device_circuit_evaluate_and_prove(p):
    """DeviceCircuit.evaluate (circuit_layer_kernel) against pyref.circuit_evaluate, and prove_circuit against
    pyref.gkr_transcript, on the edge_circuit shapes with edge-word inputs and draws"""
    pkg = load_package()
    gp = pkg.gkr_protocol
    ctx = pkg.Context(pkg.Field(p))
    F = ctx.field
    rng = random.Random(p % 10007)
    nrng = np.random.default_rng(p % 73)
    for ks in ([1, 2, 3, 2], [3, 5, 4], [0, 4, 6, 6]):
        layers = edge_circuit(rng, ks)
        inputs = edge_inputs(F, p, 1 << ks[-1], nrng)
        want = pyref.circuit_evaluate(layers, inputs, p)
        k = ks_of(layers, 1 << ks[-1])
        dc = gp.DeviceCircuit.from_arrays(ctx, k, np_layers(layers))
        vals = dc.evaluate(F.from_ints(inputs))
        assert [F.to_ints(v.to_evaluations()) for v in vals] == want[:len(layers)], ks
        del vals, dc
        if ks[0] > 0:
            draws = edge_inputs(F, p, gkr_draw_count(layers, 1 << ks[-1]), nrng)
            prove_and_check(pkg, ctx, layers, 1 << ks[-1], inputs, draws, p)
    ctx.close()


@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_w_prover_sharded_host(p):
    """the dense W prover on two ranks over host collectives (rows of add_i / mul_i by rank) beside the replicated sparse
    prover, on edge-word inputs and points"""
    pkg = load_package()
    o = oracle(p)
    gp = pkg.gkr_protocol
    DM = pkg.DenseMultilinearExtension
    F0 = pkg.Field(p)
    world = 2
    rng = random.Random(p % 77)
    nrng = np.random.default_rng(p % 71)
    for ks in ([3, 3], [5, 4], [6, 7]):
        layers = random_circuit(rng, ks)
        circuit = make_circuit(pkg, layers, 1 << ks[-1])
        evaluation = circuit.evaluate(F0, [int(x) for x in edge_table(p, 1 << ks[-1], nrng)])
        k_next = ks[1]
        r_i = edge_challenges(p, ks[0], nrng)
        oadd, omul = o.wiring_fixed(layers[0], k_next, r_i)
        ow = np.array(evaluation[1], dtype=np.uint64)
        ch = edge_challenges(p, 2 * k_next, nrng)
        ref = o.w_prove(oadd, omul, ow, ow, ch)
        lb = Loopback(world)
        results = [None] * world

        def body(rank):
            ctx = pkg.Context(pkg.Field(p))
            try:
                ar, ag = lb.collectives(rank)
                ctx.comm_init_host(rank, world, ar, ag)
                n_loc = oadd.size // world
                add_t = DM.from_evaluations_vec(ctx, 2 * k_next - 1, oadd[rank * n_loc:(rank + 1) * n_loc])
                mul_t = DM.from_evaluations_vec(ctx, 2 * k_next - 1, omul[rank * n_loc:(rank + 1) * n_loc])
                w_t = DM.from_evaluations_vec(ctx, k_next, ow)
                eng = gp.W(add_t, mul_t, w_t, w_t).native_prover()
                seng = gp.SparseLayerProver(ctx, circuit, evaluation, 0, r_i)
                got = [(eng.c1(), seng.c1())]
                for j in range(2 * k_next):
                    rp = ch[j - 1] if j else ctx.field.one
                    got.append((eng.round_evals(rp, j), seng.round_evals(rp, j)))
                results[rank] = got
                del eng, seng, add_t, mul_t, w_t
            except Exception:
                lb.barrier.abort()
                raise
            finally:
                ctx.close()

        run_threads(world, body)
        for got in results:
            assert got[0] == (ref["c_1"], ref["c_1"]), ks
            for j in range(2 * k_next):
                e = [int(x) for x in ref["evals"][j]]
                assert got[1 + j] == (e, e), (ks, j)


# ---- table calls --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["context", "handle2"])
@pytest.mark.parametrize("p", MODULI, ids=wid)
def test_table_calls(p, devices):
    """fix_variables (LE and BE), evaluate (LE and BE), evaluate_many, relabel and G::new on tables and points of edge words,
    on a one-device context and on a handle of two entries"""
    pkg = load_package()
    o = oracle(p)
    DM = pkg.DenseMultilinearExtension
    ctx = pkg.Context(pkg.Field(p), devices=devices) if devices else pkg.Context(pkg.Field(p))
    rng = np.random.default_rng(p % 67)
    for n in (8, 12, 17):
        ot = edge_table(p, 1 << n, rng)
        t = DM.from_evaluations_vec(ctx, n, ot)
        assert np.array_equal(t.to_evaluations(), ot)
        pt = np.array(edge_challenges(p, n, rng), dtype=np.uint64)
        for k in (1, 2, n // 2, n - 1, n):
            for order in (pkg.ORDER_LE, pkg.ORDER_BE):
                got = t.fix_variables([int(x) for x in pt[:k]], order=order).to_evaluations()
                assert np.array_equal(got, o.fix_variables(ot, pt[:k], order)), (n, k, order)
        assert t.evaluate([int(x) for x in pt]) == o.evaluate(ot, pt), n
        assert t.evaluate([int(x) for x in pt], order=pkg.ORDER_BE) == o.vsbw(ot, pt), n
        pts = edge_table(p, 5 * n, rng).reshape(5, n)
        pts[0] = p - 1
        assert t.evaluate_many(pts) == [o.evaluate(ot, pts[j].copy()) for j in range(5)], n
        assert t.evaluate_many(pts, pkg.ORDER_BE) == [o.vsbw(ot, pts[j].copy()) for j in range(5)], n
        for a, b, k in ((0, n // 2, n // 2), (1, n - 3, 2)):
            assert np.array_equal(t.relabel(a, b, k).to_evaluations(), o.relabel(ot, a, b, k)), (n, a, b, k)
        h = n // 2
        A, B = edge_table(p, 1 << (2 * h), rng), edge_table(p, 1 << (2 * h), rng)
        point = np.array(edge_challenges(p, 2 * h, rng), dtype=np.uint64)
        G = pkg.matrix_multiplication.G.new_from_tables(ctx, h, DM.from_evaluations_vec(ctx, 2 * h, A),
                                                        DM.from_evaluations_vec(ctx, 2 * h, B), point)
        fa, fb = o.g_new(h, A, B, point)
        assert np.array_equal(G.f_a.to_evaluations(), fa) and np.array_equal(G.f_b.to_evaluations(), fb), h
        del G, t
    ctx.close()


# ---- the sharded product prover -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,transport", [(2, "host"), (4, "host"), (2, "peer")])
@pytest.mark.parametrize("p", [2**63 + 29, 2**32 + 15], ids=wid)
def test_sharded_product_prover(p, world, transport):
    """virtual ranks (threads) proving the synthetic instance: the cells of every sharded pass cross the ranks as 32-bit limbs
    (split_limbs / sum_limb_rows / recombine_limbs, or the peer inboxes), and with these moduli the high limb of a residue is
    not zero - every rank's transcript against the oracle, from the one-round passes to the matrix-core first pass"""
    pkg = load_package()
    o = oracle(p)
    g = world.bit_length() - 1
    for n, tail_log, vpp in [(g + 3, 0, 2), (12, 0, 3), (15, 12, 2), (17 + g, 5, 4)]:
        oa, ob = o.generate(pyref.SEED_A, n), o.generate(pyref.SEED_B, n)
        ref = o.prove(oa, ob, challenges(o, n))
        results, _ = run_virtual_ranks(pkg, p, n, world, tail_log, vpp, transport=transport)
        for rank, (c1, evals, chn, final, e0, s0) in enumerate(results):
            assert c1 == ref["c_1"] and s0 == ref["c_1"], (n, rank)
            assert np.array_equal(evals, ref["evals"]), (n, rank)
            assert final == ref["final_eval"], (n, rank)
