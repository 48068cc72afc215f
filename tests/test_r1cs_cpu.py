"""CPU-only: the R1CS argument's reference (tests/r1cs_ref.py) against the dense definitions, the package's host Verifier
(thaler-study_amd/r1cs.py) against the reference prover - honest runs are accepted, every single tampered message is refused
with its own error - the host instance (R1CS, synthetic_instance) against the reference, and the SC_HD code of the sparse product
and the cubic pass, compiled for the host and run stand-alone (tests/cpp/r1cs_host_harness.cpp)."""
import os
import random
import re
import subprocess

import pytest

import expander_ref
import ligero_ref as lref
import r1cs_ref as ref
from conftest import ROOT

GOLD = lref.GOLD
P64 = 2**64 - 59
FIELDS = [(GOLD, "rs"), (P64, "expander"), (257, "rs")]
SHAPES = [(1, 2), (3, 3), (6, 5), (5, 8)]
QUERIES = 8


def instance(p, s, m, seed):
    """a satisfied instance in canonical integers: (mats, io, w); every row of A reads a witness column first, C has one entry
    per row at column 0"""
    rng = random.Random(seed)
    half = 1 << (m - 1)
    io = [rng.randrange(p)] if half >= 2 else []
    w = [rng.randrange(p) for _ in range(half)]
    z = ref.assignment(io, w, m)
    A = [(i, half + rng.randrange(half) if k == 0 else rng.randrange(2 * half), rng.randrange(1, p)) for i in range(1 << s) for k in range(3)]
    B = [(i, rng.randrange(2 * half), rng.randrange(1, p)) for i in range(1 << s) for _ in range(3)]
    az, bz = ref.sparse_mul(A, s, z, p), ref.sparse_mul(B, s, z, p)
    C = [(i, 0, az[i] * bz[i] % p) for i in range(1 << s)]
    return (A, B, C), io, w


class MontPcs:
    """a ligero_ref.RefProver behind the interface of ligero_pcs.Prover (Montgomery words, ColumnPath)"""

    def __init__(self, pkg, ref_prover, p, tamper=None):
        self.lp, self.F, self.ref, self.p, self.tamper = pkg.ligero_pcs, pkg.Field(p), ref_prover, p, tamper

    def combine(self, point, gamma):
        u_gamma, u_z = self.ref.combine(lref.canon(self.p, point), lref.canon(self.p, gamma))
        return lref.mont(self.p, u_gamma), lref.mont(self.p, u_z)

    def open_columns(self, indices):
        out = [(j, lref.mont(self.p, vals), self.lp.ColumnPath(j, sib, self.F)) for j, vals, sib in self.ref.open_columns(indices)]
        if self.tamper == "column":
            j, vals, path = out[1]
            out[1] = (j, [self.F.add(vals[0], self.F.one)] + vals[1:], path)
        return out


class MontProver:
    """r1cs_ref.RefProver behind the interface of r1cs.Prover; `tamper` names the one message it corrupts"""

    def __init__(self, pkg, p, code, s, m, mats, io, w, tamper=None):
        self.p, self.F, self.tamper, self.s = p, pkg.Field(p), tamper, s
        c = m // 2
        pcs = expander_ref.RefProver(w, c, p) if code == "expander" else lref.RefProver(w, c, 1, p)
        self.log_cols = c
        self.ref = ref.RefProver(mats, s, m, io, w, p, pcs)
        self.pcs = MontPcs(pkg, pcs, p, tamper)

    def root(self):
        return self.ref.pcs.root()

    def _draw(self, draw, name_round, k):
        """the verifier's draw behind a tamper of value k of the named round"""
        def d(j, e):
            e = lref.mont(self.p, e)
            if k is not None and j == name_round:
                e[k] = self.F.add(e[k], self.F.one)
            return lref.canon(self.p, [draw(j, e)])[0]
        return d

    def sumcheck1(self, tau, draw):
        k = int(self.tamper[4:]) if self.tamper and self.tamper.startswith("sc1_") else None
        fin = lref.mont(self.p, self.ref.sumcheck1(lref.canon(self.p, tau), self._draw(draw, 0, k)))
        if self.tamper == "v_A":
            fin[0] = self.F.add(fin[0], self.F.one)
        return tuple(fin)

    def bind(self, rho):
        self.ref.bind(lref.canon(self.p, rho))

    def sumcheck2(self, draw):
        self.ref.sumcheck2(self._draw(draw, 0, 2 if self.tamper == "sc2" else None))


def run(pkg, p, code, s, m, seed, tamper=None):
    rp = pkg.r1cs
    F = pkg.Field(p)
    mats, io, w = instance(p, s, m, seed)
    if tamper == "w":
        col = mats[0][0][1] - (1 << (m - 1))              # a witness word the first constraint reads
        w = list(w)
        w[col] = (w[col] + 1) % p
    R = rp.R1CS(F, s, m, *[[(i, j, v * lref.R64 % p) for i, j, v in M] for M in mats])
    prover = MontProver(pkg, p, code, s, m, mats, io, w, tamper)
    root = prover.root()
    pv = pkg.ligero_pcs.Verifier(F, m - 1, prover.log_cols, 1, root, QUERIES, code=code)
    verifier = rp.Verifier(R, lref.mont(p, io), root, pv)
    rng = random.Random(seed + 1)
    if tamper != "opened":
        return rp.prove_and_verify(prover, verifier, rng)
    # the same exchange by hand, with the opened value off by one
    finals = prover.sumcheck1(verifier.draw_tau(rng), lambda j, e: verifier.round1(j, e, rng))
    verifier.receive_finals(*finals)
    prover.bind(verifier.draw_rho(rng))
    prover.sumcheck2(lambda j, e: verifier.round2(j, e, rng))
    value = rp.open_committed(prover.pcs, pv, verifier.point(), rng)
    return verifier.finish(F.add(value, F.one))


@pytest.mark.parametrize("p,code", FIELDS, ids=["gold", "p64m59", "p257"])
@pytest.mark.parametrize("s,m", SHAPES)
def test_verifier_accepts_the_reference_prover(pkg, p, code, s, m):
    assert run(pkg, p, code, s, m, 1000 * s + m) is True


@pytest.mark.parametrize("p,code", FIELDS, ids=["gold", "p64m59", "p257"])
@pytest.mark.parametrize("s,m", SHAPES)
def test_every_single_tamper_is_refused_with_its_own_error(pkg, p, code, s, m):
    rp, lp = pkg.r1cs, pkg.ligero_pcs
    seed = 77 * s + m

    def refused(tamper, err, **attrs):
        with pytest.raises(err) as ei:
            run(pkg, p, code, s, m, seed, tamper)
        for k, v in attrs.items():
            assert getattr(ei.value, k) == v, (tamper, k, getattr(ei.value, k))

    refused("w", rp.RoundMismatch, phase=1, round=0)             # c1 != 0
    refused("sc1_0", rp.RoundMismatch, phase=1, round=0)
    refused("sc1_1", rp.RoundMismatch, phase=1, round=0)
    for k in (2, 3):                                             # H(2), H(3) only move the next claim
        if s > 1:
            refused("sc1_%d" % k, rp.RoundMismatch, phase=1, round=1)
        else:
            refused("sc1_%d" % k, rp.FinalMismatch, phase=1)
    refused("v_A", rp.FinalMismatch, phase=1)
    refused("sc2", rp.RoundMismatch, phase=2, round=1)
    refused("opened", rp.FinalMismatch, phase=2)
    refused("column", lp.MerkleMismatch)


@pytest.mark.parametrize("p", [GOLD, P64, 257], ids=["gold", "p64m59", "p257"])
def test_reference_sparse_products_are_the_dense_ones(p):
    rng = random.Random(p)
    s, m = 3, 4
    M = [(rng.randrange(1 << s), rng.randrange(1 << m), rng.randrange(p)) for _ in range(40)] + [(2, 5, 7), (2, 5, p - 3)]
    z = [rng.randrange(p) for _ in range(1 << m)]
    assert ref.sparse_mul(M, s, z, p) == ref.dense_mul(ref.dense(M, s, m, p), z, p)
    rx0, rho0 = [rng.randrange(p) for _ in range(s)], [rng.randrange(p) for _ in range(3)]
    assert ref.bind_rows_sparse((M, M[:7], []), s, m, rx0, rho0, p) == ref.bind_rows((M, M[:7], []), s, m, rx0, rho0, p)
    # a cubic round's H(0) + H(1) is the sum of the summand over the cube, and the cubic through its values is the next round's sum
    a, b, c = ([rng.randrange(p) for _ in range(1 << s)] for _ in range(3))
    tau, ch = [rng.randrange(p) for _ in range(s)], [rng.randrange(p) for _ in range(s)]
    E = ref.eq_table(tau, p)
    c1, rounds, finals = ref.zerocheck(a, b, c, tau, ch, p)
    assert c1 == sum(e * (x * y - t) for e, x, y, t in zip(E, a, b, c)) % p
    claim = c1
    for e4, r in zip(rounds, ch):
        assert (e4[0] + e4[1]) % p == claim
        claim = ref.cubic_at(e4, r, p)
    assert claim == lref.mle_eval(E, ch, p) * (finals[0] * finals[1] - finals[2]) % p
    assert finals == tuple(lref.mle_eval(t, ch, p) for t in (a, b, c))


@pytest.mark.parametrize("p", [GOLD, P64, 257], ids=["gold", "p64m59", "p257"])
def test_host_instance_against_the_dense_definition(pkg, p):
    rp, F = pkg.r1cs, pkg.Field(p)
    rng = random.Random(p + 5)
    s, m = 3, 4
    mats, io, w = instance(p, s, m, 9)
    mats = tuple(M + [(M[0][0], M[0][1], 5)] for M in mats[:2]) + (mats[2],)      # a duplicated (row, col)
    io, w = [], w                                                                   # (A and B changed: not satisfied any more)
    R = rp.R1CS(F, s, m, *[[(i, j, v * lref.R64 % p) for i, j, v in M] for M in mats])
    z = [rng.randrange(p) for _ in range(1 << m)]
    got = R.mul(lref.mont(p, z))
    for M, y in zip(mats, got):
        assert lref.canon(p, y) == ref.dense_mul(ref.dense(M, s, m, p), z, p)
    rx, ry, rho = ([rng.randrange(p) for _ in range(n)] for n in (s, m, 3))
    assert F.to_int(R.bind_eval(lref.mont(p, rx), lref.mont(p, ry), lref.mont(p, rho))) == ref.bind_eval_dense(mats, s, m, rx, ry, rho, p)
    with pytest.raises(ValueError):
        rp.R1CS(F, s, m, [(1 << s, 0, 1)], [], [])
    with pytest.raises(ValueError):
        rp.R1CS(F, s, m, [(0, 0, p)], [], [])


@pytest.mark.parametrize("p", [GOLD, P64], ids=["gold", "p64m59"])
def test_synthetic_instance_is_satisfied_and_has_a_dense_constant_column(pkg, p):
    rp, F = pkg.r1cs, pkg.Field(p)
    s, m = 5, 6
    R, io, w = rp.synthetic_instance(F, s, m, 3)
    z = R.assignment(io, w)
    assert z[0] == F.one and R.is_satisfied(z)
    assert sum(1 for i, j, v in R.matrices[2] if j == 0) == 1 << s == len(R.matrices[2])
    assert len(R.matrices[0]) == len(R.matrices[1]) == 3 << s
    z[-1] = F.add(z[-1], F.one)
    mats = [[(i, j, F.to_int(v)) for i, j, v in M] for M in R.matrices]
    assert R.is_satisfied(z) == all(a * b % p == c for a, b, c in zip(*(ref.sparse_mul(M, s, lref.canon(p, z), p) for M in mats)))


def test_block_run_constant_is_the_headers(pkg):
    text = open(os.path.join(ROOT, "thaler-study_amd", "csrc", "kernels", "r1cs.hpp")).read()
    run = int(re.search(r"constexpr int kSpmvRun = (\d+);", text).group(1))
    threads = int(re.search(r"constexpr int kSpmvThreads = (\d+);", text).group(1))
    assert pkg.r1cs.SPMV_BLOCK_ENTRIES == run * threads


def test_kernel_items_on_the_host(tmp_path):
    """tests/cpp/r1cs_host_harness.cpp, built and run stand-alone: the segment reduction and the image construction against a
    naive loop, the cubic item against its definition, both fields"""
    exe = tmp_path / "r1cs_host_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "r1cs_host_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "r1cs host harness ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
