"""The Reed-Solomon form of the Ligero-style commitment over full-width NTT-friendly fields (ligero_ref.WIDE_NTT): five primes
from just below 2^32 to 0xffffffffffe40001, all served by the generic field template, whose residues fill 64 bits - the carry
out of MontGeneric::add and redc, the high limbs in the host's twiddle chain and the s > 32 shifts of the root derivation, none
of which tests/test_gpu_ligero.py's fields (Goldilocks with its own template, and three primes below 2^31) can reach.

Everything is bit for bit against tests/ligero_ref.py.  The bodies of test_gpu_ligero.py's tests are the checks; this file
calls them at the wide primes (sections 1, 3-6) and adds what they lack: tables built to put every corner of add / sub in
front of the encoder's first level (section 2) and the LDS refusal on a field whose 2-adicity would allow the shape (section 7)."""
import numpy as np
import pytest

import ligero_ref as ref
import test_gpu_ligero as base
import wide_words as ww

pytestmark = pytest.mark.gpu

GOLD = ref.GOLD
P64S18, P64S34, P63S16, P32HI, P32LO = ref.WIDE_NTT
IDS = {GOLD: "gold", P64S18: "p64s18", P64S34: "p64s34", P63S16: "p63s16", P32HI: "p32hi", P32LO: "p32lo"}


def _id(v):
    return IDS.get(v, str(v))


def teardown_module(module):
    base.teardown_module(module)        # the contexts base.ctx_of made for this file


# ---- 1. the encoding on uniform residues -----------------------------------------------------------------------------

def _encode_cases():
    return [(p, log_len, rho) for p in ref.WIDE_NTT for log_len in range(1, min(14, ref.ROOTS[p][0]) + 1) for rho in (1, 2)
            if log_len - rho >= 0]


@pytest.mark.parametrize("p,log_len,rho", _encode_cases(), ids=_id)
def test_encode_equals_the_reference(pkg, p, log_len, rho):
    """every c + rho from 1 to 14, rows 1, 2 and 8 (and 32 at c = 0): every radix remainder, both load widths, one and several
    rows per block"""
    base.test_encode_equals_the_reference(pkg, p, log_len, rho)


# ---- 2. the encoding on words chosen by their sums and differences ---------------------------------------------------

def _edge_cases():
    # c = 1: the outputs E[i][0] and E[i][L/2] are the raw sums and differences; c = 6: one radix-16 pass and a radix-4 one;
    # the field's largest c: L = 2^14, the dynamic-LDS shape.  r: enough rows for every pair of diff_classes at c = 1, several
    # rows per block at c = 6, two blocks at the largest
    return [(p, c, r) for p in ref.WIDE_NTT + [GOLD] for c, r in ((1, 5), (6, 2), (min(14, ref.ROOTS[p][0]) - 1, 1))]


@pytest.mark.parametrize("p,c,r", _edge_cases(), ids=_id)
def test_encode_of_edge_words(pkg, p, c, r):
    """raw tables: the pairs of wide_words.diff_classes at the stride of the first level (every class that exists for p, checked
    before the launch), edge words only, every word p - 1, and 0 / p - 1 alternating.  For a modulus just above 2^63 two uniform
    residues practically never sum past 2^64, so there these tables are the only ones that make MontGeneric::add carry out"""
    ctx = base.ctx_of(pkg, p)
    rho, size = 1, 1 << (r + c)
    rng = np.random.default_rng(100 * c + r)
    half = ww.half_stride_table(p, 1 << r, c, rng)
    assert ww.half_stride_classes(p, half, c) >= ww.classes_present(p)
    tables = [("half_stride", half), ("edge", ww.edge_table(p, size, rng, share=1.0)),
              ("p-1", np.full(size, p - 1, dtype=np.uint64)), ("0/p-1", np.array([0, p - 1] * (size // 2), dtype=np.uint64))]
    for name, words in tables:
        assert words.dtype == np.uint64 and words.size == size and int(words.max()) < p
        t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, r + c, words)
        got = pkg.ligero_pcs.rs_encode_rows(ctx, t, c, rho).to_evaluations()
        assert got.size == size << rho
        want = base.mont_np(p, base.flat(ref.encode(ref.canon(p, words), c, rho, p)))
        assert np.array_equal(got, want), (name, int(np.flatnonzero(got != want)[0]))
        if c == 1:
            # the raw sums and differences themselves, without the reference
            hi, lo = words[0::2].astype(object), words[1::2].astype(object)
            E = got.reshape(-1, 4)
            assert [int(x) for x in E[:, 0]] == list((hi + lo) % p) and [int(x) for x in E[:, 2]] == list((hi - lo) % p), name


# ---- 3. the root -----------------------------------------------------------------------------------------------------

# rows on both sides of 8 (one hash block with its padding; data blocks and a padding block), L below, at and above the 512
# nodes the one-block tree kernel takes
ROOT_SHAPES = [(r, log_len) for r, log_len in base.ROOT_SHAPES if r in (0, 2, 3, 6)]


@pytest.mark.parametrize("r,log_len", ROOT_SHAPES)
@pytest.mark.parametrize("p", [P64S18, P63S16, P32HI], ids=_id)
def test_root_equals_hashlib_over_the_reference_encoding(pkg, p, r, log_len):
    base.test_root_equals_hashlib_over_the_reference_encoding(pkg, p, r, log_len)


# ---- 4. row combinations ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,c", [(5, 4), (12, 1)])
@pytest.mark.parametrize("p", ref.WIDE_NTT, ids=_id)
def test_combine_equals_the_reference(pkg, p, r, c):
    base.test_combine_equals_the_reference(pkg, p, r, c)


@pytest.mark.parametrize("p", ref.WIDE_NTT, ids=_id)
def test_combine_of_worst_case_words(pkg, p):
    base.test_combine_of_worst_case_words(pkg, p)


# ---- 5. openings -----------------------------------------------------------------------------------------------------

def test_open_every_column(pkg):
    base.test_open_every_column(pkg, P64S18)


# ---- 6. the protocol -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p,n,c,rho", [(P64S34, 10, 5, 1), (P64S18, 12, 7, 2), (P32HI, 8, 4, 1)], ids=_id)
def test_protocol(pkg, p, n, c, rho):
    base.test_protocol(pkg, p, n, c, rho)


# ---- 7. the LDS limit on a field whose 2-adicity is above it ---------------------------------------------------------

def test_the_lds_limit_is_refused_as_such(pkg):
    """0x8000000000050001 has s = 16: c + rho = 14 is served, 15 and 16 have a root of unity and are refused for the LDS"""
    lp = pkg.ligero_pcs
    p = P63S16
    assert ref.ROOTS[p][0] == 16
    ctx = base.ctx_of(pkg, p)
    rng = np.random.default_rng(7)
    words = rng.integers(0, p, size=1 << 14, dtype=np.uint64)
    t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 14, words)
    for c, rho in ((13, 1), (12, 2)):
        got = lp.rs_encode_rows(ctx, t, c, rho).to_evaluations()
        want = base.mont_np(p, base.flat(ref.encode(ref.canon(p, words), c, rho, p)))
        assert np.array_equal(got, want), (c, rho)
    for c, rho in ((14, 1), (13, 2), (14, 2)):
        for fn in (lambda: lp.rs_encode_rows(ctx, t, c, rho), lambda: lp.Prover.commit(ctx, t, c, rho)):
            with pytest.raises(pkg.SumcheckHipError) as ei:
                fn()
            assert ei.value.code == 6 and "LDS" in str(ei.value) and "2-adicity" not in str(ei.value), str(ei.value)
    assert len(lp.rs_encode_rows(ctx, t, 2, 1)) == 1 << 15                   # the context still works
