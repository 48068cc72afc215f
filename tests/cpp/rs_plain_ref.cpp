// A plain compiled reference of the Reed-Solomon row code and of the fold of a folded opening, for lengths at which
// tests/ligero_ref.py (Python big integers) cannot run: textbook code that includes nothing of thaler-study_amd/csrc and shares
// no arithmetic with it.  Every product is (unsigned __int128) a * b % p; sums and differences go through 128 bits as well.
//
// Everything is linear in the data, so the data words may be in any fixed scaling - the tests hand in the raw Montgomery words
// of a device table and get the Montgomery words of the result - while the roots of unity and alpha are CANONICAL.
//
//   pr_encode(p, omega_L, in, n, c, rho, out)   ligero.hpp's contract: E[i][j] = sum_k in[i][k] omega_L^(j k), natural order
//   pr_eval_at(p, omega_L, row, C, j)           the same sum for one j, by Horner
//   pr_fold(p, omega_M, U, M, alpha, out)       step 6 of rs_fold.hpp's header
#include <cstddef>
#include <cstdint>
#include <vector>

typedef uint64_t u64;
typedef unsigned __int128 u128;

namespace {

u64 mul(u64 a, u64 b, u64 p) { return (u64)((u128)a * b % p); }
u64 add(u64 a, u64 b, u64 p) { return (u64)(((u128)a + b) % p); }
u64 sub(u64 a, u64 b, u64 p) { return (u64)(((u128)a + p - b) % p); }

u64 pow_mod(u64 x, u64 e, u64 p) {
  u64 r = 1 % p;
  for (; e; e >>= 1, x = mul(x, x, p))
    if (e & 1) r = mul(r, x, p);
  return r;
}

size_t bit_reverse(size_t x, int bits) {
  size_t r = 0;
  for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1) << (bits - 1 - i);
  return r;
}

// x[j] <- sum_k x[k] w^(j k), len = 2^log_len words, w of order len: bit-reverse, then decimation in time.  pw[k] = w^k, k < len / 2
void transform(u64* x, int log_len, const std::vector<u64>& pw, u64 p) {
  const size_t len = (size_t)1 << log_len;
  for (size_t k = 0; k < len; ++k) {
    const size_t r = bit_reverse(k, log_len);
    if (k < r) {
      const u64 t = x[k];
      x[k] = x[r];
      x[r] = t;
    }
  }
  for (size_t h = 1; h < len; h *= 2) {
    const size_t stride = len / (2 * h);       // w_(2h) = w^stride
    for (size_t base = 0; base < len; base += 2 * h)
      for (size_t j = 0; j < h; ++j) {
        const u64 a = x[base + j], b = mul(x[base + j + h], pw[j * stride], p);
        x[base + j] = add(a, b, p);
        x[base + j + h] = sub(a, b, p);
      }
  }
}

}  // namespace

extern "C" {

// in: 2^n words, 2^(n-c) rows of 2^c; out: 2^(n+rho) words, the rows of L = 2^(c+rho); omega_L canonical, of order L
void pr_encode(u64 p, u64 omega_L, const u64* in, int n, int c, int rho, u64* out) {
  const size_t C = (size_t)1 << c, L = (size_t)1 << (c + rho), rows = (size_t)1 << (n - c);
  std::vector<u64> pw(L / 2 ? L / 2 : 1);
  pw[0] = 1 % p;
  for (size_t k = 1; k < L / 2; ++k) pw[k] = mul(pw[k - 1], omega_L, p);
  for (size_t i = 0; i < rows; ++i) {
    u64* row = out + i * L;
    for (size_t k = 0; k < L; ++k) row[k] = k < C ? in[i * C + k] % p : 0;
    transform(row, c + rho, pw, p);
  }
}

// sum_k row[k] omega_L^(j k), k < C
u64 pr_eval_at(u64 p, u64 omega_L, const u64* row, u64 C, u64 j) {
  const u64 x = pow_mod(omega_L, j, p);
  u64 acc = 0;
  for (u64 k = C; k-- > 0;) acc = add(mul(acc, x, p), row[k] % p, p);
  return acc;
}

// out[j] = even + alpha (odd - even), even = (U[j] + U[j + M/2]) / 2, odd = (U[j] - U[j + M/2]) / (2 omega_M^j), j < M / 2;
// omega_M (of order M) and alpha canonical
void pr_fold(u64 p, u64 omega_M, const u64* U, u64 M, u64 alpha, u64* out) {
  const u64 inv2 = pow_mod(2 % p, p - 2, p), winv = pow_mod(omega_M, p - 2, p);
  u64 xinv = 1 % p;                            // omega_M^(-j)
  for (u64 j = 0; j < M / 2; ++j, xinv = mul(xinv, winv, p)) {
    const u64 a = U[j] % p, b = U[j + M / 2] % p;
    const u64 even = mul(add(a, b, p), inv2, p);
    const u64 odd = mul(mul(sub(a, b, p), inv2, p), xinv, p);
    out[j] = add(even, mul(alpha % p, sub(odd, even, p), p), p);
  }
}
}
