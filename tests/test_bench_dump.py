"""bench.py --dump-outputs: the file format (CPU: the writer itself, exact round trip, seeded sample, size bound), the --steps
check, and on the GPU the dump of the last timed step - the same files from run to run and the oracle's transcript."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from util import GOLD, challenges, oracle, pyref


@pytest.fixture()
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def words(path, name):
    """the u64 words of one dumped output (limb pairs back to integers)"""
    a = np.load(os.path.join(path, name + ".npy"))
    assert a.dtype == np.float64 and a.shape[-1] == 2
    assert np.all(a >= 0) and np.all(a < 2.0**32) and np.all(a == np.floor(a))
    return a[..., 0].astype(np.uint64) | (a[..., 1].astype(np.uint64) << np.uint64(32))


def test_dump_round_trip_and_sample(bench, tmp_path):
    rng = np.random.default_rng(1)
    big = rng.integers(0, 2**64, size=bench.DUMP_SAMPLE_WORDS * 3, dtype=np.uint64)
    evals = np.array([[0, 1, 2**64 - 1], [2**32, 2**32 - 1, 2**63]], dtype=np.uint64)
    bench.LAST_OUTPUTS.update(c_1=np.array(2**64 - 2**32, dtype=np.uint64), round_evals=evals, table=big)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d))
    assert sorted(os.listdir(tmp_path / "a")) == ["c_1.npy", "round_evals.npy", "table.npy", "table_index.npy"]
    assert int(words(tmp_path / "a", "c_1")) == 2**64 - 2**32
    assert np.array_equal(words(tmp_path / "a", "round_evals"), evals)
    idx = np.load(tmp_path / "a" / "table_index.npy").astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE_WORDS and np.all(np.diff(idx) > 0)
    assert np.array_equal(words(tmp_path / "a", "table"), big[idx])
    for f in os.listdir(tmp_path / "a"):          # the sample is fixed: two dumps are the same files
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES


def test_dump_refuses_more_than_the_bound(bench, tmp_path):
    for k in range(40):      # 40 sampled outputs of 2^18 words: 40 x 6 MiB > 64 MiB
        bench.LAST_OUTPUTS["t%d" % k] = np.zeros(bench.DUMP_SAMPLE_WORDS + 1, dtype=np.uint64)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "x"))
    assert not (tmp_path / "x").exists()


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_steps_must_be_a_real_count(flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + flags, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--steps must be >= 1" in out.stderr, out.stderr[-1000:]


def _run(args, dump):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([l for l in out.stdout.splitlines() if l.startswith("{")]) == 1, out.stdout


@pytest.mark.gpu
def test_dump_of_the_prover_is_the_oracle_transcript(tmp_path):
    n = 18
    args = ["--num-vars", str(n), "--steps", "3", "--warmup", "1", "--cpu-num-vars", "0"]
    for d in ("a", "b"):
        _run(args, tmp_path / d)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["c_1.npy", "challenges.npy", "round_evals.npy"]
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    o = oracle(GOLD)
    ch = words(tmp_path / "a", "challenges")
    assert np.array_equal(ch, challenges(o, n))
    ref = o.prove(o.generate(pyref.SEED_A, n), o.generate(pyref.SEED_B, n), ch)
    assert ref["status"] == 0
    assert int(words(tmp_path / "a", "c_1")) == ref["c_1"]
    assert np.array_equal(words(tmp_path / "a", "round_evals"), np.asarray(ref["evals"], dtype=np.uint64).reshape(n, 3))


@pytest.mark.gpu
def test_dump_of_the_mle_workload_samples_large_tables(tmp_path):
    n = 20
    _run(["--workload", "mle", "--num-vars", str(n), "--steps", "2", "--warmup", "1"], tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["evaluate_be.npy", "evaluate_le.npy", "fix_variables_k1.npy", "fix_variables_k10.npy",
                                            "fix_variables_k1_index.npy", "fix_variables_k3.npy"]
    o = oracle(GOLD)
    t = o.generate(pyref.SEED_A, n)
    pt = np.array([o.challenge(pyref.SEED_PT, j) for j in range(n)], dtype=np.uint64)
    assert int(words(tmp_path, "evaluate_le")) == o.evaluate(t, pt)
    idx = np.load(tmp_path / "fix_variables_k1_index.npy").astype(np.int64)
    assert np.array_equal(words(tmp_path, "fix_variables_k1"), o.fix_variables(t, pt[:1])[idx])
    assert np.array_equal(words(tmp_path, "fix_variables_k3"), o.fix_variables(t, pt[:3]))
    assert np.array_equal(words(tmp_path, "fix_variables_k10"), o.fix_variables(t, pt[:10]))
