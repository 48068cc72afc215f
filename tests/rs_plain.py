"""The plain compiled reference of the Reed-Solomon rows and their folds (tests/cpp/rs_plain_ref.cpp: textbook code, 128-bit
products, nothing of the package's sources), for the lengths Python big integers cannot follow.  Compiled with g++ on first use
into a temporary directory; the handle is kept for the process.  Nothing here imports the package.

The data words go in and come out as uint64 arrays in whatever scaling they have - the operations are linear, so the raw
Montgomery words of a device table give the Montgomery words of the result - while roots of unity (ligero_ref.omega) and alphas
are CANONICAL.

  encode(p, words, c, rho)         E of ligero.hpp's contract, flat, row-major
  eval_at(p, row, log_len, j)      sum_k row[k] w_L^(j k), L = 2^log_len
  fold(p, U, alpha)                one fold of rs_fold.hpp's step 6
  fold_many(p, U, alphas)          len(alphas) successive folds"""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import ligero_ref as ref

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "rs_plain_ref.cpp")
u64p = ctypes.POINTER(ctypes.c_uint64)
_lib = []


def lib():
    if not _lib:
        build = tempfile.mkdtemp(prefix="rs_plain_")
        atexit.register(shutil.rmtree, build, ignore_errors=True)
        out = os.path.join(build, "librs_plain_ref.so")
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, SOURCE])
        h = ctypes.CDLL(out)
        h.pr_encode.argtypes = [ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, u64p]
        h.pr_encode.restype = None
        h.pr_eval_at.argtypes = [ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_uint64, ctypes.c_uint64]
        h.pr_eval_at.restype = ctypes.c_uint64
        h.pr_fold.argtypes = [ctypes.c_uint64, ctypes.c_uint64, u64p, ctypes.c_uint64, ctypes.c_uint64, u64p]
        h.pr_fold.restype = None
        _lib.append(h)
    return _lib[0]


def _words(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def encode(p, words, c, rho):
    """the codeword matrix of the 2^n words (rows of 2^c), flat: 2^(n + rho) words"""
    w = _words(words)
    n = w.size.bit_length() - 1
    assert w.size == 1 << n and 0 <= c <= n
    out = np.empty(w.size << rho, dtype=np.uint64)
    lib().pr_encode(p, ref.omega(p, c + rho), w.ctypes.data_as(u64p), n, c, rho, out.ctypes.data_as(u64p))
    return out


def eval_at(p, row, log_len, j):
    w = _words(row)
    return int(lib().pr_eval_at(p, ref.omega(p, log_len), w.ctypes.data_as(u64p), w.size, j))


def fold(p, U, alpha, omega_m=None):
    """the fold of the M words of U by the canonical alpha; omega_m: the canonical root of order M (ligero_ref.omega's)"""
    u = _words(U)
    log_m = u.size.bit_length() - 1
    assert u.size == 1 << log_m and log_m >= 1 and 0 <= int(alpha) < p
    out = np.empty(u.size // 2, dtype=np.uint64)
    lib().pr_fold(p, ref.omega(p, log_m) if omega_m is None else omega_m, u.ctypes.data_as(u64p), u.size, int(alpha), out.ctypes.data_as(u64p))
    return out


def fold_many(p, U, alphas):
    for alpha in alphas:
        U = fold(p, U, alpha)
    return U
