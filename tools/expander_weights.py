"""A probe of the minimum codeword weight of "expander code 1"  on the CPU: NOT a distance bound.

The relative distance of the recursive code is not proved.  This tool encodes low-weight messages - where a sparse-graph code
is weakest - and records the lightest codeword it meets, as a fraction of L = 2 m:

  every weight-1 message (m of them; by linearity the weight does not depend on the nonzero value);
  --samples random messages of each weight 2 .. 8 (random positions, random nonzero values);
  c = 6 .. 13, over p = 257 and p = 2^64 - 59.

The encoder is a numpy restatement of the contract (gathers over index and coefficient arrays built from
thaler-study_amd/expander_code.py's hashes; int64 arithmetic for p = 257, Python integers in object arrays above); it is
checked against expander_code.encode on a random message per (p, c) before it is used.

  python tools/expander_weights.py [--samples 3000] [--cmin 6] [--cmax 13] [--out profiles/expander_weights.md]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (257, 2**64 - 59)


def load_package_module(name):
    """thaler-study_amd/<name>.py alone, without the package (no library needed)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "thaler-study_amd", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


xc = load_package_module("expander_code")


class Level:
    """the two maps of one level as arrays: y = sum over 32 terms of ca[:, k] * x[ia[:, k]], v likewise over 16"""

    def __init__(self, lm, p):
        m = 1 << lm
        dtype = np.int64 if p < 2**31 else object
        self.ia = np.empty((m // 4, 4 * xc.D_A), dtype=np.int64)
        self.ca = np.empty((m // 4, 4 * xc.D_A), dtype=dtype)
        for t in range(xc.D_A):
            K = xc.key(lm, 0, t)
            for e in range(m):
                self.ia[e >> 2, 4 * t + (e & 3)] = xc.perm(K, lm, e)
                self.ca[e >> 2, 4 * t + (e & 3)] = xc.coef(K, e, p)
        self.ib = np.empty((m // 2, xc.D_B), dtype=np.int64)
        self.cb = np.empty((m // 2, xc.D_B), dtype=dtype)
        for t in range(xc.D_B):
            K = xc.key(lm, 1, t)
            for j in range(m // 2):
                self.ib[j, t] = xc.perm(K, lm - 1, j)
                self.cb[j, t] = xc.coef(K, j, p)


class Encoder:
    """Enc over canonical values, a batch of messages at once: X of shape (batch, m) -> (batch, 2 m)"""

    def __init__(self, p):
        self.p = p
        self.dtype = np.int64 if p < 2**31 else object
        self.levels = {}
        self.base = {}

    def encode(self, X):
        p, m = self.p, X.shape[1]
        if m <= xc.BASE_MAX:
            if m not in self.base:
                self.base[m] = np.array([[pow(j + k + 1, -1, p) for j in range(m)] for k in range(m)], dtype=self.dtype)
            return np.concatenate([X, X.dot(self.base[m]) % p], axis=1)
        lm = m.bit_length() - 1
        if lm not in self.levels:
            self.levels[lm] = Level(lm, p)
        lv = self.levels[lm]
        Y = (X[:, lv.ia] * lv.ca).sum(axis=2) % p
        Z = self.encode(Y)
        V = (Z[:, lv.ib] * lv.cb).sum(axis=2) % p
        return np.concatenate([X, Z, V], axis=1)


class _CanonField:
    """expander_code.encode takes Montgomery words of a field object; with R = 1 they are the canonical values"""

    def __init__(self, p):
        self.p, self._rinv = p, 1

    def from_int(self, x):
        return int(x) % self.p


def probe(p, c, samples, rng):
    """{weight: (lightest codeword weight, messages tried)} for message weights 1 .. 8"""
    m = 1 << c
    enc = Encoder(p)
    check = [int(v) for v in rng.integers(0, min(p, 2**63), size=m)]
    got = enc.encode(np.array([check], dtype=enc.dtype))[0]
    assert [int(v) for v in got] == xc.encode(_CanonField(p), check), "the numpy encoder disagrees with expander_code.encode"
    out = {}
    batch = 256 if p < 2**31 else 64
    # weight 1: every position, value 1
    light = 2 * m
    for i0 in range(0, m, batch):
        X = np.zeros((min(batch, m - i0), m), dtype=enc.dtype)
        for k in range(X.shape[0]):
            X[k, i0 + k] = 1
        light = min(light, int((enc.encode(X) != 0).sum(axis=1).min()))
    out[1] = (light, m)
    for w in range(2, 9):
        light = 2 * m
        for i0 in range(0, samples, batch):
            X = np.zeros((min(batch, samples - i0), m), dtype=enc.dtype)
            for k in range(X.shape[0]):
                for pos in rng.choice(m, size=w, replace=False):
                    X[k, pos] = int(rng.integers(1, min(p, 2**63)))
            light = min(light, int((enc.encode(X) != 0).sum(axis=1).min()))
        out[w] = (light, samples)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=3000, help="random messages per weight 2 .. 8")
    ap.add_argument("--cmin", type=int, default=6)
    ap.add_argument("--cmax", type=int, default=13)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expander_weights.md"))
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    lines = ["# Expander code 1: lightest codewords met by a low-weight probe", "",
             "Written by `python tools/expander_weights.py --samples %d --seed %d`.  For each field and message length m = 2^c: every "
             "weight-1 message and %d random messages of each weight 2 .. 8; the entry is the lightest codeword met, as a fraction of "
             "L = 2 m (in brackets: its weight).  **A sanity check, not a bound**: the relative distance of the code is not proved, "
             "and a probe of low-weight messages cannot prove it." % (args.samples, args.seed, args.samples), "",
             "| p | c | L | w = 1 | w = 2 | w = 3 | w = 4 | w = 5 | w = 6 | w = 7 | w = 8 | minimum |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    overall = {}
    for p in FIELDS:
        for c in range(args.cmin, args.cmax + 1):
            t0 = time.perf_counter()
            res = probe(p, c, args.samples, rng)
            L = 2 << c
            low = min(v[0] for v in res.values())
            overall[p] = min(overall.get(p, 1.0), low / L)
            lines.append("| %d | %d | %d | %s | %.3f |" % (p, c, L, " | ".join("%.3f (%d)" % (res[w][0] / L, res[w][0]) for w in range(1, 9)), low / L))
            print("p = %d c = %d: minimum %.3f of L (%d) in %.0f s" % (p, c, low / L, low, time.perf_counter() - t0), file=sys.stderr)
    lines += ["", "Minimum over every shape: " + ", ".join("%.3f of L over p = %d" % (v, p) for p, v in overall.items()) + ".", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
