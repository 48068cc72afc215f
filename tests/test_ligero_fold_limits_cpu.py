"""CPU-only, with tests/test_gpu_ligero_fold_limits.py: that the inputs of that file cover what it says they cover - its four
shapes launch all twelve rs_fold_kernel<F, A, AN>, its fold tables carry every add / sub corner class that exists for the
field, its challenges contain 0, the field's one and p - 1 - and, on those same inputs, the two host-side pieces the GPU file
leans on: the package's FoldVerifier over full-width fields (accepted with the value, tampering refused) and the per-item code of
rs_fold_kernel compiled for the host, for every (A, AN), against tests/ligero_fold_staged_ref.py."""
import pytest

import ligero_fold_staged_ref as sref
import ligero_ref as ref
import wide_words
from ligero_fold_limits_cases import (ALL_PAIRS, FIELDS, FOLD_LOGS, P64S18, SHAPES, ScriptedDraws, edge_inputs, fid, fold_alpha_sets,
                                      fold_table, launched_pairs)
from test_ligero_fold_staged_cpu import host_stage, rfm, run_staged_protocol  # noqa: F401 (rfm: the fixture that builds the harness)


# ---- 1. what the inputs cover ----------------------------------------------------------------------------------------

def test_the_shapes_launch_every_instantiation():
    assert {pair for _, _, _, arities in SHAPES for pair in launched_pairs(arities)} == ALL_PAIRS
    for n, c, rho, arities in SHAPES:
        assert sum(arities) == c <= n and all(c + rho <= ref.ROOTS[p][0] for p in FIELDS)


@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_the_fold_tables_carry_every_class_of_the_field(p):
    pairs, present = wide_words.diff_classes(p), wide_words.classes_present(p)
    assert present and present <= set(wide_words.DIFF_CLASSES)
    checked = 0
    for log_m in FOLD_LOGS:
        table = fold_table(p, log_m)
        assert table.size == 1 << log_m and int(table.max()) < p
        if 1 << (log_m - 1) >= len(pairs):
            assert wide_words.half_stride_classes(p, table, log_m) == present, log_m
            checked += 1
    assert checked == len(FOLD_LOGS) - 1          # every length but 2^4
    # the tables of the transcripts: 2^(n-c) rows of 2^c words, the pairs going on from row to row
    for n, c, rho, arities in SHAPES:
        assert wide_words.half_stride_classes(p, edge_inputs(p, n, c, rho, arities)["table"], c) == present, (n, c)


@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_the_challenges_contain_zero_one_and_minus_one(p):
    for _, c, _, _ in SHAPES:
        assert {0, ref.R64 % p, p - 1} <= set(wide_words.degenerate_challenges(p, c))
    for count in (1, 2, 3):
        sets = fold_alpha_sets(p, 9, count)
        assert all(len(s) == count and max(s) < p for s in sets)
    assert {0, ref.R64 % p, p - 1} <= {a for s in fold_alpha_sets(p, 9, 3) for a in s}


# ---- 2. the host verifier over full-width fields ---------------------------------------------------------------------

def edge_protocol(pkg, p, shape, tamper=None):
    """run_staged_protocol on the worst-case inputs of the GPU file: the table as it is, gamma, the point, beta and the alphas
    through the verifier's own draws"""
    n, c, rho, arities = shape
    x = edge_inputs(p, n, c, rho, arities)
    table = ref.canon(p, x["table"])
    draws = ScriptedDraws(p, ref.canon(p, x["gamma"] + x["point"] + [x["beta"]] + x["alphas"]), n)
    value, want, prover = run_staged_protocol(pkg, p, n, c, rho, arities, 8, None, tamper=tamper, table=table, rng=draws)
    assert not draws.values                       # every scripted word was drawn: the verifier saw exactly these inputs
    return value, want, table, x


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: fid(s[3]))
@pytest.mark.parametrize("p", FIELDS, ids=fid)
def test_fold_verifier_accepts_the_reference_prover_on_worst_case_words(pkg, p, shape):
    value, want, table, x = edge_protocol(pkg, p, shape)
    assert value == want == ref.mont(p, [ref.mle_eval(table, ref.canon(p, x["point"]), p)])[0]


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=lambda s: fid(s[3]))
def test_tampering_is_caught_over_a_full_width_field(pkg, shape):
    lp = pkg.ligero_pcs
    for tamper, err in (("layer", lp.FoldMismatch), ("word", lp.MerkleMismatch)):
        with pytest.raises(err) as ei:
            edge_protocol(pkg, P64S18, shape, tamper=tamper)
        assert type(ei.value) is err, (tamper, ei.value)


# ---- 3. the kernel's per-item code on the host, on the fold tables ---------------------------------------------------

@pytest.mark.parametrize("p", ref.WIDE_NTT, ids=fid)
def test_host_item_on_the_fold_tables(rfm, p):  # noqa: F811
    ran = set()
    for log_m in FOLD_LOGS:
        words = fold_table(p, log_m)
        U = ref.canon(p, words)
        for a in (1, 2, 3):
            for alphas in fold_alpha_sets(p, log_m, a)[::2]:          # the first degenerate set and the uniform one
                alphas = ref.canon(p, alphas)
                want = sref.fold_many(U, alphas, p)
                for an in range(0, min(3, log_m - a) + 1):
                    got, leaves = host_stage(rfm, p, log_m, 0, alphas, an, words)
                    assert got == want, (p, log_m, a, an)
                    assert leaves == (sref.stage_leaves(want, an) if an else []), (p, log_m, a, an)
                    ran.add((a, an))
    assert ran == ALL_PAIRS
