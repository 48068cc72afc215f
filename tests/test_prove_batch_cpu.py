"""CPU-only checks of sc_prove_batch (a batch of independent product sumchecks, one launch per pass for the whole batch): the
header declares it and SC_KIND_BATCH_PASS, the ctypes stub and the Rust declaration agree with it, the kernel is in the code
object, and the Python wrappers refuse bad arguments before they touch a device."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, load_package

HEADER = open(os.path.join(ROOT, "include", "sumcheck_hip.h")).read()


def test_header_declares_sc_prove_batch():
    assert re.search(r"#define SC_KIND_BATCH_PASS 16\b", HEADER)
    assert re.search(r"typedef uint64_t \(\*sc_draw_batch_fn\)\(void\* user, size_t instance, size_t round, const uint64_t evals\[3\]\);",
                     HEADER)
    flat = re.sub(r"\s+", " ", HEADER)
    assert ("int sc_prove_batch(sc_ctx* ctx, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_batch_fn draw, "
            "void* user, const uint64_t* seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges);") in flat
    assert re.search(r"#define SC_ABI_VERSION 6\b", HEADER)


def test_ctypes_signature_matches_header():
    pkg = load_package()
    lib = pkg._lib
    res, args = lib.SIGNATURES["sc_prove_batch"]
    assert res is ctypes.c_int
    assert args == [lib.voidp, lib.size_t, ctypes.POINTER(lib.voidp), ctypes.POINTER(lib.voidp), lib.DRAW_BATCH_FN, lib.voidp,
                    lib.u64p, lib.u64p, lib.u64p, lib.u64p]
    assert lib.DRAW_BATCH_FN._restype_ is lib.u64
    assert list(lib.DRAW_BATCH_FN._argtypes_) == [lib.voidp, lib.size_t, lib.size_t, lib.u64p]
    assert lib.KIND_NAMES[16] == "batch_pass"
    rust = open(os.path.join(ROOT, "rust", "sumcheck-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn sc_prove_batch\(", rust)
    assert re.search(r"pub type sc_draw_batch_fn = Option<unsafe extern \"C\" fn\(user: \*mut c_void, instance: usize, round: usize, "
                     r"evals: \*const u64\) -> u64>;", rust)


def test_library_exports_sc_prove_batch():
    pkg = load_package()
    pkg.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    assert re.search(r" T sc_prove_batch$", out, flags=re.M)
    assert b"batch_pass_kernel" in open(pkg._lib.LIB_PATH, "rb").read()


class _Untouchable:
    """a context whose every attribute access fails: a wrapper that validates first never reaches it"""

    def __getattr__(self, name):
        raise AssertionError("the device context was touched (%s)" % name)


def _fake_g(mm, ctx, n):
    g = mm.G.__new__(mm.G)
    g.ctx = ctx
    g.field = None
    g.num_vars = lambda: n
    g.f_a = g.f_b = None
    return g


def test_prove_batch_validates_before_the_device():
    mm = load_package().matrix_multiplication
    ctx = _Untouchable()
    with pytest.raises(ValueError):
        mm.prove_batch(ctx, [])
    with pytest.raises(TypeError):
        mm.prove_batch(ctx, [object()])
    with pytest.raises(ValueError):   # an instance of another context
        mm.prove_batch(ctx, [_fake_g(mm, ctx, 3), _fake_g(mm, _Untouchable(), 3)])
    with pytest.raises(ValueError):   # sizes differ
        mm.prove_batch(ctx, [_fake_g(mm, ctx, 3), _fake_g(mm, ctx, 4)])
    with pytest.raises(ValueError):   # one seed per instance
        mm.prove_batch(ctx, [_fake_g(mm, ctx, 3)] * 2, seed_r=[1, 2, 3])
    with pytest.raises(TypeError):
        mm.prove_batch(ctx, [_fake_g(mm, ctx, 3)], draw=5)


def test_prove_products_validates_before_the_device():
    mm = load_package().matrix_multiplication
    ctx = _Untouchable()
    A = [0] * 16
    with pytest.raises(ValueError):
        mm.prove_products(ctx, 2, [])
    with pytest.raises(ValueError):
        mm.prove_products(ctx, 15, [(A, A)])
    with pytest.raises(ValueError):
        mm.prove_products(ctx, -1, [(A, A)])
    with pytest.raises(TypeError):
        mm.prove_products(ctx, 2, [(A, A, A)])
    with pytest.raises(ValueError):
        mm.prove_products(ctx, 2, [(A, A)], Cs=[A, A])
    with pytest.raises(ValueError):
        mm.prove_products(ctx, 2, [(A, A)], points=[[1, 2, 3]])
    with pytest.raises(ValueError):
        mm.prove_products(ctx, 2, [(A, A)] * 2, seed_r=[1])
    with pytest.raises(TypeError):
        mm.prove_products(ctx, 2, [(A, A)], draw="no")


def test_batch_seeds():
    mm = load_package().matrix_multiplication
    assert mm._batch_seeds(None, 3) == [mm._SEED_R, mm._SEED_R + 1, mm._SEED_R + 2]
    assert mm._batch_seeds(7, 2) == [7, 7]
    assert mm._batch_seeds([1, 2**64 + 3], 2) == [1, 3]
