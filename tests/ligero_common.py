"""What the GPU tests of the Ligero-style commitment share, whatever the row code (tests/test_gpu_ligero.py,
tests/test_gpu_expander.py and the files built on them): contexts, the one way a refusal is checked, and tables."""
import numpy as np
import pytest

import ligero_ref


def context_cache():
    """(ctx_of, teardown_module) over a cache of their own: one ordinary context per field for the whole of a test file, closed by
    the file's teardown_module.  A file that borrows another's ctx_of calls that file's teardown_module from its own"""
    cache = {}

    def ctx_of(pkg, p):
        if p not in cache:
            cache[p] = pkg.Context(pkg.Field(p))
        return cache[p]

    def teardown_module(module):
        for ctx in cache.values():
            ctx.close()
        cache.clear()

    return ctx_of, teardown_module


def expect(pkg, code, fn, *needles):
    with pytest.raises(pkg.SumcheckHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for s in needles:
        assert s in str(ei.value), (s, str(ei.value))


def mont_np(p, canon):
    """canonical integers -> Montgomery words, uint64"""
    if p < 2**31:
        return ((np.asarray(canon, dtype=np.int64) % p) * (ligero_ref.R64 % p) % p).astype(np.uint64)
    return (np.array([int(x) for x in canon], dtype=object) * ligero_ref.R64 % p).astype(np.uint64)


def upload(pkg, ctx, p, canon):
    n = len(canon).bit_length() - 1
    return pkg.DenseMultilinearExtension.from_evaluations_vec(ctx, n, mont_np(p, canon))


def flat(E):
    return [x for row in E for x in row]
