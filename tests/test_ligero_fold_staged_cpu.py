"""CPU-only: the staged folded opening's reference (tests/ligero_fold_staged_ref.py) against the definition it rests on (a stage's
fold is successive single folds, and word j of it needs the 2^a words of leaf j alone), the package's host FoldVerifier with a
schedule (thaler-study_amd/ligero_pcs.py) against the reference prover - honest transcripts are accepted with the right value,
every tampered message is refused with its own error, an all-ones schedule gives the binary opening's messages - the size
helpers and fold_shape against counted bytes and brute force, and the per-item code of rs_fold_kernel, compiled for the
host (tests/cpp/rs_fold_host_harness.cpp), against the reference bit for bit."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import ligero_fold_ref as fref
import ligero_fold_staged_ref as sref
import ligero_ref as ref
import wide_words
from conftest import ROOT

GOLD = ref.GOLD
# (n, c, rho, schedule): R = 1 in one stage; no trees; both orders of (1, 2); two blow-up bits; three stages; arity 3 first
SHAPES = [(3, 3, 1, (3,)), (5, 1, 1, (1,)), (6, 3, 1, (1, 2)), (6, 3, 1, (2, 1)), (7, 2, 2, (2,)), (8, 6, 1, (1, 3, 2)), (8, 7, 1, (3, 3, 1))]


def _sid(v):
    return "".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("p", [GOLD, ref.BABYBEAR, 257])
def test_a_stage_is_successive_folds_and_needs_its_leaf_alone(p):
    rng = random.Random(p + 1)
    for log_m in range(2, 8):
        M = 1 << log_m
        U = [rng.randrange(p) for _ in range(M)]
        for a in range(1, min(3, log_m - 1) + 1):
            alphas = [(0, 1, p - 1)[(a + log_m + k) % 3] if k == 1 else rng.randrange(p) for k in range(a)]
            want = sref.fold_many(U, alphas, p)
            assert len(want) == M >> a
            got = [sref.fold_leaf([U[j + t * (M >> a)] for t in range(1 << a)], alphas, p, log_m, j) for j in range(M >> a)]
            assert got == want, (p, log_m, a)
    # a codeword folds to the codeword of the fixed message, whatever the grouping
    m = [rng.randrange(p) for _ in range(32)]
    alphas = [rng.randrange(p) for _ in range(5)]
    U = ref.encode(m, 5, 1, p)[0]
    for ar in ((3, 2), (2, 3), (1, 3, 1)):
        V, i = U, 0
        for a in ar:
            V, i = sref.fold_many(V, alphas[i:i + a], p), i + a
        assert V == [ref.mle_eval(m, alphas, p)] * 2


def run_staged_protocol(pkg, p, n, c, rho, arities, queries, seed, tamper=None, table=None, rng=None):
    """the reference prover against the package's FoldVerifier under a schedule; `tamper` names the message to corrupt.  `table`
    (canonical values) and `rng` (what draws for the verifier) replace the seeded ones (tests/test_ligero_fold_limits_cpu.py).
    Returns (value, expected, reference prover)"""
    lp = pkg.ligero_pcs
    F = pkg.Field(p)
    rng = rng or random.Random(seed)
    if table is None:
        table = [rng.randrange(p) for _ in range(1 << n)]
    corrupt = None
    if tamper == "layer":
        corrupt = lambda s, U: [(x + k % 2) % p for k, x in enumerate(U)] if s == 1 else U   # noqa: E731 (wrong odd words of stage 1's layer, hashed as they are: the final value does not depend on them)
    prover = sref.RefStagedProver(table, c, rho, p, arities, corrupt=corrupt)
    v = lp.FoldVerifier(F, n, c, rho, prover.root(), queries, arities=arities)
    gamma = v.draw_gamma(rng)
    point = [F.rand(rng) for _ in range(n)]
    claims = ref.mont(p, prover.begin(ref.canon(p, point), ref.canon(p, gamma)))
    if tamper == "v":
        claims[0] = F.add(claims[0], F.one)
    if tamper == "v_gamma":
        claims[1] = F.add(claims[1], F.one)
    v.receive_claims(*claims)
    beta = v.draw_beta(rng)
    starts = sref.starts(arities)
    stray = next((i for i in range(1, c) if i not in starts), None)       # a round that starts no stage

    def draw(i, sums, root):
        sums = ref.mont(p, sums)
        if tamper == "round" and i == c - 1:
            sums[2] = F.add(sums[2], F.one)       # the last round's H(2): only the final check sees it
        if tamper == "round0" and i == 0:
            sums[0] = F.add(sums[0], F.one)
        if tamper == "root" and len(starts) > 1 and i == starts[1]:
            root = bytes([root[0] ^ 1]) + root[1:]
        if tamper == "stray_root" and i == stray:
            root = bytes(32)
        if tamper == "no_root" and len(starts) > 1 and i == starts[1]:
            root = None
        return F.to_int(v.round(i, sums, root, rng))

    _, roots, _, final = prover.prove(F.to_int(beta), draw)
    assert len(roots) == len(arities) - 1
    final = F.from_int(final)
    if tamper == "final":
        final = F.add(final, F.one)
    v.receive_final(final)
    indices = v.draw_queries(rng)
    assert all(q < 1 << (c + rho - arities[0]) for q in indices)
    asked = list(indices)
    if tamper == "index":
        asked[2] = (asked[2] + 1) % (1 << (c + rho - arities[0]))
    openings = []
    for q, cols, stages in prover.query(asked):
        cols = [(j, ref.mont(p, vals), lp.ColumnPath(j, sib, F)) for j, vals, sib in cols]
        openings.append((q, cols, [(tuple(ref.mont(p, words)), list(sib)) for words, sib in stages]))
    if tamper == "index":
        q, cols, stages = openings[2]
        openings[2] = (indices[2], cols, stages)               # answered for another index, labelled as the drawn one
    if tamper == "word":
        q, cols, stages = openings[1]
        words, sib = stages[-1]
        openings[1] = (q, cols, stages[:-1] + [(words[:-1] + (F.add(words[-1], F.one),), sib)])
    if tamper == "path":
        q, cols, stages = openings[3]
        words, sib = stages[0]
        openings[3] = (q, cols, [(words, sib[:-1] + [bytes(32)])] + stages[1:])
    if tamper == "column":
        q, cols, stages = openings[0]
        j, vals, path = cols[-1]
        openings[0] = (q, cols[:-1] + [(j, [F.add(vals[0], F.one)] + vals[1:], path)], stages)
    value = v.verify(point, openings)
    return value, F.from_int(ref.mle_eval(table, ref.canon(p, point), p)), prover


@pytest.mark.parametrize("p", [GOLD, 257])
@pytest.mark.parametrize("n,c,rho,arities", SHAPES, ids=_sid)
def test_fold_verifier_accepts_the_staged_reference_prover(pkg, p, n, c, rho, arities):
    value, want, _ = run_staged_protocol(pkg, p, n, c, rho, arities, 8, 10 * n + c)
    assert value == want


@pytest.mark.parametrize("p", [GOLD, 257])
def test_staged_tampering_is_caught(pkg, p):
    lp, rp = pkg.ligero_pcs, pkg.relaxed_pcs
    cases = (("v", lp.RoundMismatch), ("v_gamma", lp.RoundMismatch), ("round0", lp.RoundMismatch), ("round", lp.EvalMismatch),
             ("final", lp.EvalMismatch), ("root", lp.MerkleMismatch), ("word", lp.MerkleMismatch), ("path", lp.MerkleMismatch),
             ("column", lp.MerkleMismatch), ("index", lp.MerkleMismatch), ("stray_root", rp.Error), ("no_root", rp.Error),
             ("layer", lp.FoldMismatch))
    for tamper, err in cases:
        with pytest.raises(err) as ei:
            run_staged_protocol(pkg, p, 8, 6, 1, (1, 3, 2), 8, 31, tamper=tamper)
        assert type(ei.value) is err, (tamper, ei.value)
    # arity 3 first: eight columns per query; and one stage (no trees): the claims, the round and the columns still bind
    for tamper, err in (("column", lp.MerkleMismatch), ("index", lp.MerkleMismatch), ("layer", lp.FoldMismatch), ("word", lp.MerkleMismatch)):
        with pytest.raises(err):
            run_staged_protocol(pkg, p, 8, 7, 1, (3, 3, 1), 8, 33, tamper=tamper)
    for tamper, err in (("v", lp.RoundMismatch), ("round", lp.EvalMismatch), ("final", lp.EvalMismatch), ("column", lp.MerkleMismatch)):
        with pytest.raises(err):
            run_staged_protocol(pkg, p, 3, 3, 1, (3,), 8, 32, tamper=tamper)


def test_schedules_are_checked(pkg):
    lp = pkg.ligero_pcs
    F = pkg.Field(GOLD)
    for bad in ((), (1, 1), (4, 2), (0, 3, 3), (3, 3, 1)):
        with pytest.raises(ValueError):
            lp.FoldVerifier(F, 8, 6, 1, bytes(32), 4, arities=bad)
        with pytest.raises(ValueError):
            lp.fold_opening_bytes(8, 6, 1, 4, arities=bad)
    assert lp.FoldVerifier(F, 8, 6, 1, bytes(32), 4).arities is None
    assert lp.FoldVerifier(F, 8, 6, 1, bytes(32), 4, arities=[3, 3]).arities == (3, 3)


@pytest.mark.parametrize("p", [GOLD, 257])
def test_an_all_ones_schedule_gives_the_binary_openings_messages(pkg, p):
    lp = pkg.ligero_pcs
    n, c, rho = 6, 3, 1
    rng = random.Random(p + 2)
    table = [rng.randrange(p) for _ in range(1 << n)]
    point, gamma = [rng.randrange(p) for _ in range(n)], [rng.randrange(p) for _ in range(1 << (n - c))]
    beta, alphas = rng.randrange(p), [rng.randrange(p) for _ in range(c)]
    old = fref.RefFoldProver(table, c, rho, p)
    new = sref.RefStagedProver(table, c, rho, p, (1,) * c, commitment=old.commitment)
    assert new.begin(point, gamma) == old.begin(point, gamma)
    seen_old, seen_new = [], []
    assert new.prove(beta, lambda i, e, root: seen_new.append((i, e, root)) or alphas[i]) == \
        old.prove(beta, lambda i, e, root: seen_old.append((i, e, root)) or alphas[i])
    assert seen_new == seen_old
    queries = [0, 7, 3, 5]
    for (q, cols, stages), (wq, lo, hi, layers) in zip(new.query(queries), old.query(queries)):
        assert (q, cols, stages) == (wq, [lo, hi], layers)
    assert sref.message_bytes(new.messages) == fref.message_bytes(old.messages) == lp.fold_opening_bytes(n, c, rho, 4) == \
        lp.fold_opening_bytes(n, c, rho, 4, arities=(1, 1, 1))
    # and the verifier with that schedule accepts them
    value, want, _ = run_staged_protocol(pkg, p, n, c, rho, (1, 1, 1), 8, 5)
    assert value == want


@pytest.mark.parametrize("n,c,rho,arities", SHAPES, ids=_sid)
def test_fold_opening_bytes_counts_the_staged_reference_messages(pkg, n, c, rho, arities):
    lp = pkg.ligero_pcs
    _, _, prover = run_staged_protocol(pkg, GOLD, n, c, rho, arities, 5, 77)
    assert sref.message_bytes(prover.messages) == lp.fold_opening_bytes(n, c, rho, 5, arities=arities) == sref.opening_bytes(n, c, rho, 5, arities)


def test_staged_size_helpers(pkg):
    lp = pkg.ligero_pcs
    table = {28: (23, (1, 3, 3, 3, 3, 3, 3, 3, 1), 641856), 24: (19, (1, 3, 3, 3, 3, 3, 3), 488096), 20: (16, (1, 3, 3, 3, 3, 3), 356920)}
    for n, (c, arities, size) in table.items():
        assert lp.fold_opening_bytes(n, c, 1, 128, arities=arities) == size
        assert lp.fold_shape(n, 1, 128) == (c, arities)
        assert size < lp.fold_opening_bytes(n, lp.fold_log_cols(n, 1, 128), 1, 128)
    assert lp.fold_opening_bytes(28, 22, 1, 128, arities=(1,) * 22) == lp.fold_opening_bytes(28, 22, 1, 128) == 1309896
    assert lp.fold_shape(12, 1, 16) == (8, (1, 3, 3, 1)) and lp.fold_opening_bytes(12, 8, 1, 16, arities=(1, 3, 3, 1)) == 20024
    # arity 1 alone is the binary opening's shape
    for n in (12, 20, 28):
        c = lp.fold_log_cols(n, 1, 128)
        assert lp.fold_shape(n, 1, 128, max_arity=1) == (c, (1,) * c)
    with pytest.raises(ValueError):
        lp.fold_shape(12, 1, 16, max_arity=4)


@pytest.mark.parametrize("rho", [1, 2])
def test_fold_shape_equals_brute_force(pkg, rho):
    lp = pkg.ligero_pcs
    for n in range(1, 13):
        for queries in (1, 16, 128):
            for max_arity in (1, 2, 3):
                size, c, arities = sref.best_shape(n, rho, queries, max_arity)
                assert lp.fold_shape(n, rho, queries, max_arity) == (c, arities), (n, rho, queries, max_arity)
                assert lp.fold_opening_bytes(n, c, rho, queries, arities=arities) == size
    # the limit on the codeword's length holds
    assert lp.fold_shape(12, rho, 16, max_log_len=6) == sref.best_shape(12, rho, 16, 3, max_log_len=6)[1:]


# ---- the kernel's per-item code on the host --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rfm(tmp_path_factory):
    out = tmp_path_factory.mktemp("rfm") / "librs_fold_many_host.so"
    src = os.path.join(ROOT, "tests", "cpp", "rs_fold_host_harness.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(out), src])
    lib = ctypes.CDLL(str(out))
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.rfm_fold.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u64p, ctypes.c_int, ctypes.c_int, u64p, u64p,
                             ctypes.POINTER(ctypes.c_uint8)]
    lib.rfm_fold.restype = None
    return lib


def host_stage(rfm, p, log_len0, shift, alphas, an, words):
    """rs_fold_kernel<F, len(alphas), an>'s items over the RAW words of a layer of 2^(log_len0 - shift) words: (folded
    canonical words, leaf digests)"""
    a, M = len(alphas), len(words)
    u = np.ascontiguousarray(words, dtype=np.uint64)
    al = np.array(ref.mont(p, alphas), dtype=np.uint64)
    out = np.zeros(M >> a, dtype=np.uint64)
    leaves = (M >> (a + an)) if an else 0
    dig = (ctypes.c_uint8 * max(1, 32 * leaves))()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    rfm.rfm_fold(p, int(p == GOLD), ref.mont(p, [ref.omega(p, log_len0)])[0], log_len0, shift, al.ctypes.data_as(u64p), a, an,
                 u.ctypes.data_as(u64p), out.ctypes.data_as(u64p), dig)
    raw = bytes(dig)
    return ref.canon(p, out), [raw[32 * j:32 * j + 32] for j in range(leaves)]


@pytest.mark.parametrize("p", [GOLD, ref.BABYBEAR, ref.P64S18])
def test_host_item_equals_successive_reference_folds(rfm, p):
    rng, nrng = random.Random(p + 7), np.random.default_rng(p % 1000)
    for a in (1, 2, 3):
        for log_m in range(a + 1, 11):
            words = wide_words.edge_table(p, 1 << log_m, nrng)
            U = ref.canon(p, words)
            alphas = [(0, 1, p - 1, rng.randrange(p))[(log_m + k) % 4] for k in range(a)]
            want = sref.fold_many(U, alphas, p)
            for an in range(0, min(3, log_m - a) + 1):
                got, leaves = host_stage(rfm, p, log_m, 0, alphas, an, words)
                assert got == want, (p, a, an, log_m)
                assert leaves == (sref.stage_leaves(want, an) if an else []), (p, a, an, log_m)


@pytest.mark.parametrize("p", [GOLD, ref.P64S18])
def test_host_item_serves_every_stage_from_the_layer_0_tables(rfm, p):
    """a layer of 2^(l0 - shift) words folds with the tables of length 2^l0, on both sides of the twist tables' boundary"""
    rng, nrng = random.Random(p + 8), np.random.default_rng(8)
    for log_len0 in (11, 12, 13):
        for shift in (1, 3, log_len0 - 6, log_len0 - 4):
            for a, an in ((1, 3), (2, 2), (3, 0), (3, 1), (3, 3)):
                if a + an > log_len0 - shift or a + 1 > log_len0 - shift:
                    continue
                words = wide_words.edge_table(p, 1 << (log_len0 - shift), nrng)
                alphas = [rng.randrange(p) for _ in range(a)]
                want = sref.fold_many(ref.canon(p, words), alphas, p)
                got, leaves = host_stage(rfm, p, log_len0, shift, alphas, an, words)
                assert got == want, (p, log_len0, shift, a, an)
                assert leaves == (sref.stage_leaves(want, an) if an else []), (p, log_len0, shift, a, an)


def test_stage_leaf_is_the_column_leaf_of_its_words():
    assert sref.stage_leaf((3, 5)) == fref.pair_leaf(3, 5)
    assert sref.stage_leaf((3, 5, 7, 9)) == ref.column_leaf([[3], [5], [7], [9]], 0)
    U = list(range(16))
    assert sref.stage_leaves(U, 3) == [ref.column_leaf([U[0:2], U[2:4], U[4:6], U[6:8], U[8:10], U[10:12], U[12:14], U[14:16]], j) for j in (0, 1)]
