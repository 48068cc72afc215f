// Host build of the fold's per-item code and constants of thaler-study_amd/csrc/kernels/rs_fold.hpp (what rs_fold_kernel<F, A, AN> runs
// for every output leaf: the exponent of 1 / x, its table look-up on either side of the twist tables' boundary, the 2^AN output
// words one after the other, each A successive folds of 2^A input words, and the leaf digest fed word by word; and
// rs_fold_constants, which the engine calls for every launch), compiled for the CPU, so that a whole stage is checked against
// tests/ligero_fold_ref.py and tests/ligero_fold_staged_ref.py without a GPU.  As a shared library it serves
// tests/test_ligero_fold_cpu.py and tests/test_ligero_fold_staged_cpu.py; as a program (it has a main) it checks the same items
// against A successive applications of the fold's defining formula, with every table allocated at its exact size: that is the
// build that runs under -fsanitize=address,undefined.
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

// the kernel arguments: the engine's constants (rs_fold_constants) on half, zeta and eta derived from w_l0 by plain powers
template <class F>
RsFoldArgs fold_args(const F& f, u64 omega0, int log_len0, int shift, const u64* alphas, int a, int an, const std::vector<u64>& lo,
                     const std::vector<u64>& hi) {
  RsFoldArgs k = {};
  const int log_m = log_len0 - shift;
  const u64 half = power(f, f.add(f.one(), f.one()), f.modulus() - 2);
  const u64 w_m = power(f, omega0, (u64)1 << shift);
  const u64 zeta = power(f, power(f, w_m, (u64)1 << (log_m - a)), f.modulus() - 2);
  const int w = rs_fold_item_log(an);
  const u64 eta = power(f, power(f, w_m, (u64)1 << (log_m - a - w)), f.modulus() - 2);
  rs_fold_constants(f, half, zeta, eta, alphas, a, w, &k);
  k.lo = lo.data();
  k.hi = hi.empty() ? nullptr : hi.data();
  k.log_len0 = log_len0;
  k.shift = shift;
  return k;
}

// one launch of rs_fold_kernel<F, A, AN>, item by item: U has 2^(log_len0 - shift) words, out 2^A times fewer and at least two;
// leaves (AN >= 1) gets 8 words per item
template <int A, int AN, class F>
void fold_stage_as(const F& f, const RsFoldArgs& k, int log_m, const u64* U, u64* out, u32* leaves) {
  const u32 items = 1u << (log_m - A - rs_fold_item_log(AN));
  for (u32 j = 0; j < items; ++j) {
    u32 d[8];
    rs_fold_item<A, AN>(f, k, j, items, U, out, d);
    if (AN > 0) memcpy(leaves + 8 * (size_t)j, d, sizeof d);
  }
}

template <class F>
void fold_stage(const F& f, u64 omega0, int log_len0, int shift, const u64* alphas, int a, int an, const u64* U, u64* out, u32* leaves) {
  std::vector<u64> lo, hi;
  fold_tables(f, omega0, log_len0, &lo, &hi);
  const RsFoldArgs k = fold_args(f, omega0, log_len0, shift, alphas, a, an, lo, hi);
  const int log_m = log_len0 - shift;
#define RFM_CASE(A, AN) \
  if (a == A && an == AN) return fold_stage_as<A, AN>(f, k, log_m, U, out, leaves)
  RFM_CASE(1, 0); RFM_CASE(1, 1); RFM_CASE(1, 2); RFM_CASE(1, 3);
  RFM_CASE(2, 0); RFM_CASE(2, 1); RFM_CASE(2, 2); RFM_CASE(2, 3);
  RFM_CASE(3, 0); RFM_CASE(3, 1); RFM_CASE(3, 2); RFM_CASE(3, 3);
#undef RFM_CASE
}

// the defining formula of one fold, every power from scratch
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
      const int log_m = log_len0 - shift;
      const u32 M = 1u << log_m;
      std::vector<u64> U(M);
      for (u32 k = 0; k < M; ++k) U[k] = (k % 3 == 0) ? p - 1 : (k % 3 == 1 ? 0 : f.to_mont(splitmix64(k + 17 * log_len0) % p));
      // every challenge at every level: a single fold meets 0 and p - 1 too
      const u64 any = f.to_mont(splitmix64(99 + shift) % p), ring[5] = {any, p - 1, 0, any, p - 1};
      for (int rot = 0; rot < 3; ++rot)
      for (int a = 1; a <= 3 && a + 1 <= log_m; ++a) {
        const u64* alphas = ring + rot;
        // `a` single folds, one after the other
        std::vector<u64> want(U);
        u64 omega_m = power(f, omega0, (u64)1 << shift);
        for (int l = 0; l < a; ++l, omega_m = f.mul(omega_m, omega_m)) {
          const u32 len = M >> l;
          std::vector<u64> next(len / 2);
          for (u32 j = 0; j < len / 2; ++j) next[j] = fold_direct(f, omega_m, alphas[l], want.data(), len, j);
          want.swap(next);
        }
        for (int an = 0; an <= 3 && a + an <= log_m; ++an) {
          std::vector<u64> out(M >> a);
          std::vector<u32> leaves(an ? 8 * (size_t)(M >> (a + an)) : 0);
          fold_stage(f, omega0, log_len0, shift, alphas, a, an, U.data(), out.data(), leaves.data());
          if (out != want) ++bad;
        }
      }
    }
  }
  printf("%s: %s\n", name, bad ? "MISMATCH" : "ok");
  return bad;
}

}  // namespace

extern "C" {
// gold != 0: GoldilocksMont (p ignored), else MontGeneric of p.  omega0: w_l0, Montgomery; alphas: a Montgomery words; U:
// 2^(log_len0 - shift) Montgomery words; out: 2^a times fewer; leaves (an >= 1): 32 bytes per leaf of 2^an words, in the ABI's byte order
void rfm_fold(u64 p, int gold, u64 omega0, int log_len0, int shift, const u64* alphas, int a, int an, const u64* U, u64* out,
              uint8_t* leaves) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  const size_t items = an ? (size_t)1 << (log_len0 - shift - a - an) : 0;
  std::vector<u32> words(8 * items);
  if (gold) fold_stage(GoldilocksMont(fp), omega0, log_len0, shift, alphas, a, an, U, out, words.data());
  else fold_stage(MontGeneric(fp), omega0, log_len0, shift, alphas, a, an, U, out, words.data());
  for (size_t j = 0; j < items; ++j) put_digest(leaves + 32 * j, &words[8 * j]);
}
// one fold with alpha, the binary opening's: out has half as many words; leaves: null, or 32 bytes per pair of out
void rf_fold(u64 p, int gold, u64 omega0, int log_len0, int shift, u64 alpha, const u64* U, u64* out, uint8_t* leaves) {
  rfm_fold(p, gold, omega0, log_len0, shift, &alpha, 1, leaves ? 1 : 0, U, out, leaves);
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
