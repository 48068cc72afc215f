// Host build of the per-item code of thaler-study_amd/csrc/kernels/rs_fold.hpp (what rs_fold_kernel runs for every j < M / 4: the
// exponent of 1 / x, its table look-up on either side of the twist tables' boundary, the two folds and the leaf digest), compiled
// for the CPU, so that a whole fold is checked against tests/ligero_fold_ref.py without a GPU.  As a shared library it serves
// tests/test_ligero_fold_cpu.py; as a program (it has a main) it checks the same items against the fold's defining formula,
// with every table allocated at its exact size: that is the build that runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/merkle.hpp"
#include "../../thaler-study_amd/csrc/kernels/rs_fold.hpp"
using namespace sc;

namespace {

template <class F>
u64 power(const F& f, u64 x, u64 e) {
  u64 r = f.one();
  for (; e; e >>= 1, x = f.mul(x, x))
    if (e & 1) r = f.mul(r, x);
  return r;
}

// the tables of layer-0 length 2^log_len0 as the context builds them: lo (and hi from 2^kRsFoldTwistMinLog on)
template <class F>
void fold_tables(const F& f, u64 omega0, int log_len0, std::vector<u64>* lo, std::vector<u64>* hi) {
  if (log_len0 >= kRsFoldTwistMinLog) {
    const size_t n_lo = (size_t)1 << kRsTwistLoLog, n_hi = (size_t)1 << (log_len0 - kRsTwistLoLog);
    lo->assign(n_lo, f.one());
    hi->assign(n_hi, f.one());
    for (size_t i = 1; i < n_lo; ++i) (*lo)[i] = f.mul((*lo)[i - 1], omega0);
    const u64 step = f.mul((*lo)[n_lo - 1], omega0);
    for (size_t i = 1; i < n_hi; ++i) (*hi)[i] = f.mul((*hi)[i - 1], step);
  } else {
    const size_t half = ((size_t)1 << log_len0) / 2;
    lo->assign(half, f.one());
    hi->clear();
    for (size_t i = 1; i < half; ++i) (*lo)[i] = f.mul((*lo)[i - 1], omega0);
  }
}

// one launch of rs_fold_kernel, item by item: U has 2^(log_len0 - shift) words; leaves (may be null) gets 8 words per item
template <class F>
void fold_layer(const F& f, u64 omega0, int log_len0, int shift, u64 alpha, const u64* U, u64* out, u32* leaves) {
  std::vector<u64> lo, hi;
  fold_tables(f, omega0, log_len0, &lo, &hi);
  const u64 half = power(f, f.add(f.one(), f.one()), f.modulus() - 2);
  RsFoldArgs a;
  a.c1 = f.mul(half, alpha);
  a.c0 = f.sub(half, a.c1);
  const u64 w4 = power(f, omega0, (u64)1 << (log_len0 - 2));
  a.inv_w4 = f.sub(0, w4);
  a.lo = lo.data();
  a.hi = hi.empty() ? nullptr : hi.data();
  a.log_len0 = log_len0;
  a.shift = shift;
  const u32 quarter = 1u << (log_len0 - shift - 2);
  for (u32 j = 0; j < quarter; ++j) {
    const u64 u[4] = {U[j], U[j + quarter], U[j + 2 * quarter], U[j + 3 * quarter]};
    u64 o[2];
    rs_fold_item(f, a, j, u, o);
    out[j] = o[0];
    out[j + quarter] = o[1];
    if (leaves) rs_fold_leaf(f, o, *reinterpret_cast<u32(*)[8]>(leaves + 8 * (size_t)j));
  }
}

// the defining formula, every power from scratch
template <class F>
u64 fold_direct(const F& f, u64 omega_m, u64 alpha, const u64* U, u32 M, u32 j) {
  const u64 half = power(f, f.add(f.one(), f.one()), f.modulus() - 2);
  const u64 xinv = power(f, power(f, omega_m, j), f.modulus() - 2);
  const u64 even = f.mul(f.add(U[j], U[j + M / 2]), half), odd = f.mul(f.mul(f.sub(U[j], U[j + M / 2]), half), xinv);
  return f.add(even, f.mul(alpha, f.sub(odd, even)));
}

template <class F>
int self_check(const F& f, u64 w_max_canonical, int s, const char* name) {
  int bad = 0;
  const u64 p = f.modulus(), w_max = f.to_mont(w_max_canonical);
  for (int log_len0 = 2; log_len0 <= 13 && log_len0 <= s; ++log_len0) {
    const u64 omega0 = power(f, w_max, (u64)1 << (s - log_len0));
    for (int shift = 0; log_len0 - shift >= 2; shift += (log_len0 > 8 ? 3 : 1)) {
      const u32 M = 1u << (log_len0 - shift);
      std::vector<u64> U(M), out(M / 2);
      std::vector<u32> leaves(8 * (size_t)(M / 4));
      for (u32 k = 0; k < M; ++k) U[k] = (k % 3 == 0) ? p - 1 : (k % 3 == 1 ? 0 : f.to_mont(splitmix64(k + 17 * log_len0) % p));
      const u64 alphas[3] = {0, p - 1, f.to_mont(splitmix64(99 + shift) % p)};
      for (u64 alpha : alphas) {
        fold_layer(f, omega0, log_len0, shift, alpha, U.data(), out.data(), leaves.data());
        const u64 omega_m = power(f, omega0, (u64)1 << shift);
        for (u32 j = 0; j < M / 2; ++j)
          if (out[j] != fold_direct(f, omega_m, alpha, U.data(), M, j)) ++bad;
      }
    }
  }
  printf("%s: %s\n", name, bad ? "MISMATCH" : "ok");
  return bad;
}

}  // namespace

extern "C" {
// gold != 0: GoldilocksMont (p ignored), else MontGeneric of p.  omega0: w_l0, Montgomery; U: 2^(log_len0 - shift) Montgomery words;
// out: half as many; leaves: null, or 32 bytes per item in the ABI's byte order
void rf_fold(u64 p, int gold, u64 omega0, int log_len0, int shift, u64 alpha, const u64* U, u64* out, uint8_t* leaves) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  const size_t items = (size_t)1 << (log_len0 - shift - 2);
  std::vector<u32> words(leaves ? 8 * items : 0);
  if (gold) fold_layer(GoldilocksMont(fp), omega0, log_len0, shift, alpha, U, out, leaves ? words.data() : nullptr);
  else fold_layer(MontGeneric(fp), omega0, log_len0, shift, alpha, U, out, leaves ? words.data() : nullptr);
  for (size_t j = 0; leaves && j < items; ++j) put_digest(leaves + 32 * j, &words[8 * j]);
}
u32 rf_exp(int log_len0, int shift, u32 j) { return rs_fold_exp(log_len0, shift, j); }
}

int main() {
  FieldParams fp;
  field_params_from_modulus(GoldilocksMont::P, &fp);
  int bad = self_check(GoldilocksMont(fp), 1753635133440165772ull, 32, "Goldilocks");
  field_params_from_modulus(0xFFFFFFFFFFE40001ull, &fp);
  bad += self_check(MontGeneric(fp), 11880867381004357348ull, 18, "0xffffffffffe40001");
  field_params_from_modulus(257, &fp);
  bad += self_check(MontGeneric(fp), 3, 8, "257");
  return bad ? 1 : 0;
}
