"""What the eight row-code entry points refuse (sc_rs_encode_rows, sc_ligero_commit, sc_xc_encode_rows, sc_ligero_commit_code and
their _long forms), pinned whole: the return code, every character of sc_last_error and a null *out.  The expected texts are
written out from the format strings of the engine, so that a change of a check, of its place in the order of the checks or of the
name a call reports under shows here.  Every case but the last two is refused before any launch.

(The refusal of n + log_blowup > 29 needs a table of 2 GiB and is not here.)"""
import ctypes
import random

import numpy as np
import pytest

import expander_ref
import ligero_ref

pytestmark = pytest.mark.gpu

GOLD = ligero_ref.GOLD
P59 = 2**64 - 59
BIG = (GOLD, P59)
SENTINEL = 0xDEAD0

# a path: (symbol, code or None); the four-argument forms take no log_blowup, the _code forms a code
RS_SHORT = [("sc_rs_encode_rows", None), ("sc_ligero_commit", None), ("sc_ligero_commit_code", 0)]
RS_LONG = [("sc_rs_encode_rows_long", None), ("sc_ligero_commit_long", None), ("sc_ligero_commit_code_long", 0)]
XC_SHORT = [("sc_xc_encode_rows", None), ("sc_ligero_commit_code", 1)]
XC_LONG = [("sc_xc_encode_rows_long", None), ("sc_ligero_commit_code_long", 1)]
XC_COMMITS = [XC_SHORT[1], XC_LONG[1]]
EVERY = RS_SHORT + RS_LONG + XC_SHORT + XC_LONG

_ctx = {}
_tables = {}


def ctx_of(pkg, p):
    if p not in _ctx:
        _ctx[p] = pkg.Context(pkg.Field(p))
    return _ctx[p]


def table_of(pkg, p, n):
    if (p, n) not in _tables:
        _tables[(p, n)] = pkg.DenseMultilinearExtension.generate(ctx_of(pkg, p), 7, n)
    return _tables[(p, n)]


def teardown_module(module):
    _tables.clear()
    for ctx in _ctx.values():
        ctx.close()
    _ctx.clear()


def name_of(path):
    """the name a path reports under: the _code forms with SC_CODE_RS delegate to the plain commit"""
    sym, code = path
    return sym.replace("_commit_code", "_commit") if code == 0 else sym


def call(lib, path, ctx_h, t_h, log_cols, log_blowup, out):
    sym, code = path
    if "_xc_" in sym:
        return getattr(lib, sym)(ctx_h, t_h, log_cols, out)
    if code is None:
        return getattr(lib, sym)(ctx_h, t_h, log_cols, log_blowup, out)
    return getattr(lib, sym)(ctx_h, t_h, log_cols, log_blowup, code, out)


def refused(ctx, path, t, log_cols, log_blowup, rc, text):
    h = ctypes.c_void_p(SENTINEL)
    got = call(ctx.lib, path, ctx.h, t.h if t is not None else None, log_cols, log_blowup, ctypes.byref(h))
    assert (got, ctx.lib.sc_last_error(ctx.h).decode(), h.value) == (rc, text, None), (path, log_cols, log_blowup)


# ---- the texts, from the engine's format strings ---------------------------------------------------------------------

def t_table(name):
    return "%s: table is null or not 2^k long" % name


def t_multi(name):
    return "%s: runs on a context of one device and one rank (this one is a multi-device handle)" % name


def t_blowup(name, rho):
    return "%s: log_blowup is %d, not 1 or 2" % (name, rho)


def t_rate(name, rho):
    return "%s: the expander code has rate 1/2: log_blowup is %d, not 1" % (name, rho)


def t_cols(name, c, n):
    return "%s: log_cols = %d exceeds the table's %d variables" % (name, c, n)


def t_rs_lds(name, c, rho):
    return "%s: a codeword of 2^(%d+%d) words does not fit the LDS of a CU (at most 2^14)" % (name, c, rho)


def t_rs_long(name, c, rho):
    return ("%s: a codeword of 2^(%d+%d) words is longer than 2^24 (there the stored tree is 1 GiB and a tile's strided segments 32 bytes)"
            % (name, c, rho))


def t_xc_lds(name, c):
    return "%s: a codeword of 2^(%d+1) words does not fit the LDS of a CU (at most 2^14)" % (name, c)


def t_xc_long(name, c):
    return "%s: a codeword of 2^(%d+1) words is longer than 2^24 (there the stored tree is 1 GiB)" % (name, c)


def t_adicity(name, p, s, c, rho):
    return "%s: p = %d has 2-adicity %d: no root of unity of order 2^(%d+%d)" % (name, p, s, c, rho)


def t_small_p(name, p):
    return "%s: p = %d: the base code inverts 1 .. 63 and needs p > 63" % (name, p)


def t_code(sym, code):
    return "%s: code %d is neither SC_CODE_RS nor SC_CODE_EXPANDER" % (sym, code)


# ---- the cases -------------------------------------------------------------------------------------------------------

def test_null_arguments(pkg):
    for p in BIG:
        ctx, t = ctx_of(pkg, p), table_of(pkg, p, 3)
        refused(ctx, RS_SHORT[0], t, 1, 0, 1, t_blowup("sc_rs_encode_rows", 0))      # a message to find unchanged below
        before = ctx.lib.sc_last_error(ctx.h).decode()
        for path in EVERY:
            h = ctypes.c_void_p(SENTINEL)
            assert call(ctx.lib, path, None, t.h, 1, 1, ctypes.byref(h)) == 1, path  # no context
            assert call(ctx.lib, path, ctx.h, t.h, 1, 1, None) == 1, path            # nowhere to put the result
            assert call(ctx.lib, path, None, None, 1, 1, None) == 1, path
            assert ctx.lib.sc_last_error(ctx.h).decode() == before, path            # neither leaves a message
        for path in EVERY:
            refused(ctx, path, None, 1, 1, 1, t_table(name_of(path)))


def test_log_blowup_out_of_range(pkg):
    for p in BIG:
        ctx, t = ctx_of(pkg, p), table_of(pkg, p, 3)
        for path in RS_SHORT + RS_LONG:
            for rho in (0, 3):
                refused(ctx, path, t, 1, rho, 1, t_blowup(name_of(path), rho))
        for path in XC_COMMITS:
            for rho in (0, 2):
                refused(ctx, path, t, 1, rho, 1, t_rate(path[0], rho))


def test_log_cols_above_the_table(pkg):
    for p in BIG:
        ctx, t = ctx_of(pkg, p), table_of(pkg, p, 3)
        for path in EVERY:
            refused(ctx, path, t, 4, 1, 1, t_cols(name_of(path), 4, 3))


def test_the_short_limit(pkg):
    for p in BIG:
        ctx, t = ctx_of(pkg, p), table_of(pkg, p, 15)
        for path in RS_SHORT:
            for c, rho in ((14, 1), (13, 2)):
                refused(ctx, path, t, c, rho, 6, t_rs_lds(name_of(path), c, rho))
        for path in XC_SHORT:
            refused(ctx, path, t, 14, 1, 6, t_xc_lds(path[0], 14))


def test_the_long_limit(pkg):
    ctx = ctx_of(pkg, GOLD)
    for n, c, rho in ((23, 23, 2), (24, 24, 1)):
        for path in RS_LONG:
            refused(ctx, path, table_of(pkg, GOLD, n), c, rho, 6, t_rs_long(name_of(path), c, rho))
    for path in XC_LONG:
        refused(ctx, path, table_of(pkg, GOLD, 24), 24, 1, 6, t_xc_long(path[0], 24))


def test_two_adicity(pkg):
    ctx, t = ctx_of(pkg, 257), table_of(pkg, 257, 9)
    for path in RS_SHORT:
        for c, rho in ((8, 1), (7, 2)):
            refused(ctx, path, t, c, rho, 6, t_adicity(name_of(path), 257, 8, c, rho))
    ctx, t = ctx_of(pkg, 65537), table_of(pkg, 65537, 16)
    for path in RS_LONG:
        for c, rho in ((16, 1), (15, 2)):
            refused(ctx, path, t, c, rho, 6, t_adicity(name_of(path), 65537, 16, c, rho))
    # c + rho = 16 = s is served
    h = ctypes.c_void_p()
    assert ctx.lib.sc_ligero_commit_long(ctx.h, t.h, 15, 1, ctypes.byref(h)) == 0 and h.value
    prover = pkg.ligero_pcs.Prover(ctx, t, h)
    assert (prover.log_rows, prover.log_cols, prover.log_blowup, prover.code) == (1, 15, 1, "rs")
    prover.close()


def test_a_field_too_small_for_the_base_code(pkg):
    ctx, t = ctx_of(pkg, 5), table_of(pkg, 5, 4)
    for path in XC_SHORT + XC_LONG:
        refused(ctx, path, t, 2, 1, 6, t_small_p(path[0], 5))


def test_unknown_codes(pkg):
    for p in BIG:
        ctx, t = ctx_of(pkg, p), table_of(pkg, p, 3)
        for sym in ("sc_ligero_commit_code", "sc_ligero_commit_code_long"):
            for code in (2, -1):
                refused(ctx, (sym, code), t, 1, 1, 1, t_code(sym, code))
                refused(ctx, (sym, code), None, 9, 7, 1, t_code(sym, code))          # before every other check
            # SC_CODE_RS reports under the name of the plain commit
            refused(ctx, (sym, 0), t, 1, 3, 1, t_blowup(sym.replace("_commit_code", "_commit"), 3))


def test_order_of_the_checks(pkg):
    for p in BIG:
        ctx = ctx_of(pkg, p)
        # the expander commit: the limit before the rate
        refused(ctx, XC_COMMITS[0], table_of(pkg, p, 15), 14, 2, 6, t_xc_lds("sc_ligero_commit_code", 14))
        # Reed-Solomon: log_blowup before log_cols
        for path in RS_SHORT + RS_LONG:
            refused(ctx, path, table_of(pkg, p, 3), 4, 3, 1, t_blowup(name_of(path), 3))
        # the expander code: log_cols against the table before log_cols against the limit
        for path in XC_SHORT:
            refused(ctx, path, table_of(pkg, p, 15), 16, 1, 1, t_cols(path[0], 16, 15))
    ctx = ctx_of(pkg, GOLD)
    refused(ctx, XC_COMMITS[1], table_of(pkg, GOLD, 24), 24, 2, 6, t_xc_long("sc_ligero_commit_code_long", 24))
    for path in XC_LONG:
        refused(ctx, path, table_of(pkg, GOLD, 24), 25, 1, 1, t_cols(path[0], 25, 24))


def test_order_of_the_checks_on_a_multi_device_handle(pkg):
    F = pkg.Field(GOLD)
    m = pkg.Context(F, devices=[0, 0])
    mt = pkg.DenseMultilinearExtension.from_evaluations_vec(m, 4, F.from_ints(range(16)))
    for path in RS_SHORT + RS_LONG:
        refused(m, path, mt, 2, 3, 6, t_multi(name_of(path)))
    for path in XC_SHORT + XC_LONG:
        refused(m, path, mt, 2, 2, 6, t_multi(path[0]))
    for path in EVERY:
        refused(m, path, None, 2, 1, 6, t_multi(name_of(path)))                      # before the table is looked at
    del mt
    m.close()


def test_every_context_still_encodes(pkg):
    """last in the file: after all the refusals above each context encodes a table of 16 words, bit for bit"""
    lp = pkg.ligero_pcs
    rng = random.Random(16)
    for p in (GOLD, P59, 257, 65537, 5):
        ctx = ctx_of(pkg, p)
        table = [rng.randrange(p) for _ in range(16)]
        t = pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, 4, np.array(ligero_ref.mont(p, table), dtype=np.uint64))
        c = min(2, ligero_ref.two_adic(p)[0] - 1)
        for encode in (lp.rs_encode_rows, lp.rs_encode_rows_long):
            want = [x for row in ligero_ref.encode(table, c, 1, p) for x in row]
            assert [int(x) for x in encode(ctx, t, c, 1).to_evaluations()] == ligero_ref.mont(p, want), (p, c)
        if p > 63:
            for encode in (lp.xc_encode_rows, lp.xc_encode_rows_long):
                want = [x for row in expander_ref.encode_rows(table, 2, p) for x in row]
                assert [int(x) for x in encode(ctx, t, 2).to_evaluations()] == ligero_ref.mont(p, want), p
