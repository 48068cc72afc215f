"""CPU-only: the transcript layout of sc_gkr_prove_circuit as the Python binding sizes it, and DeviceCircuit.from_arrays'
checks, which run before any native call."""
import random

import numpy as np
import pytest

from conftest import load_package
from test_gpu_gkr import random_circuit
from test_host_protocols import BOOK, THREE, gkr_draw_count
from util import pyref


def ks_of(layers, num_inputs):
    return [(len(l) - 1).bit_length() for l in layers] + [(num_inputs - 1).bit_length()]


CASES = [(BOOK, 4), (THREE, 8)]
_rng = random.Random(7)
for _ks in ([1, 2, 3, 2], [2, 3, 4, 4, 3], [3, 5, 4], [1, 1, 1, 1], [0, 2, 1]):
    CASES.append((random_circuit(_rng, _ks), 1 << _ks[-1]))


@pytest.mark.parametrize("layers,num_inputs", CASES, ids=["book", "three_layer", "r1232", "r23443", "r354", "r1111", "r021"])
def test_transcript_sizes_match_the_oracle_layout(layers, num_inputs):
    gp = load_package().gkr_protocol
    p = 389
    k = ks_of(layers, num_inputs)
    sz = gp.transcript_sizes(k)
    assert sz["draws"] == gkr_draw_count(layers, num_inputs)
    rng = random.Random(len(layers))
    inputs = [rng.randrange(p) for _ in range(num_inputs)]
    draws = [rng.randrange(p) for _ in range(sz["draws"])]
    ref = pyref.gkr_transcript(layers, num_inputs, inputs, draws, p)
    assert sz["outputs"] == len(ref["circuit_outputs"])
    assert sz["c1"] == len(ref["layers"])
    assert sz["evals"] == 3 * sum(len(l["evals"]) for l in ref["layers"])
    assert sz["q"] == sum(l["num_vars"] // 2 + 1 for l in ref["layers"])          # dense, k + 1 coefficients per layer
    assert sz["draws"] == len(ref["r_0"]) + sum(len(l["challenges"]) + 1 for l in ref["layers"])


def _arrays(k, rng):
    out = []
    for i in range(len(k) - 1):
        n, n_next = 1 << k[i], 1 << k[i + 1]
        out.append((np.array([rng.randrange(2) for _ in range(n)], dtype=np.int32),
                    np.array([rng.randrange(n_next) for _ in range(n)], dtype=np.uint32),
                    np.array([rng.randrange(n_next) for _ in range(n)], dtype=np.uint32)))
    return out


def test_from_arrays_rejects_bad_arrays_before_any_native_call():
    """ctx=None: anything that reached the library would fail with an AttributeError, not these errors"""
    gp = load_package().gkr_protocol
    rng = random.Random(3)
    k = [2, 3, 2]
    good = _arrays(k, rng)
    t, a, b = good[1]
    bad_cases = [
        (TypeError, [good[0], (t.astype(np.int64), a, b)]),                    # types of the wrong dtype
        (TypeError, [good[0], (t, a.astype(np.int32), b)]),                    # in0 signed
        (TypeError, [good[0], (t, a, b.astype(np.uint64))]),                   # in1 too wide
        (TypeError, [good[0], (t, a, list(b))]),                               # not a numpy array
        (TypeError, [good[0], (t, a, b.reshape(2, 4))]),                       # not 1-D
        (ValueError, [good[0], (t[:-1], a, b)]),                               # one gate short
        (ValueError, [good[0], (t, a, np.concatenate([b, b]))]),               # twice as long
        (ValueError, [good[0]]),                                               # a layer missing for k
        (ValueError, [good[0], (t, a)]),                                       # not a triple
    ]
    for exc, layers in bad_cases:
        with pytest.raises(exc):
            gp.DeviceCircuit.from_arrays(None, k, layers)
    with pytest.raises(ValueError):
        gp.DeviceCircuit.from_arrays(None, [2, -1, 2], good)
