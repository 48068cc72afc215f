// Host build of the plan of thaler-study_amd/csrc/kernels/expander_long.hpp and a replay of its launches with the work items the
// kernels run, compiled for the CPU: the copy, every global level's down items on the row-strided array E, the inner code of
// every row through an image of its own (what xc_long_inner_kernel does in LDS), every global level's up items.  Checked
// against tests/expander_ref.py without a GPU.  With XC_LONG_HARNESS_MAIN it is a program that replays two shapes on both field
// types and compares with the whole recursion run in place on E (for a sanitizer build).
#include <cstdio>
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/expander_long.hpp"
using namespace sc;

namespace {

// xc_sweeps over an image of one codeword of 2^(c+1) words, work items in order (the barriers become the loop ends)
template <class F>
void sweeps(const F& f, u64* tile, const u64* inv, int c) {
  const int log_len = c + 1, levels = xc_levels(c);
  u32 o = 0;
  for (int l = 0; l < levels; ++l) {
    const int lm = c - 2 * l;
    for (u32 it = 0; it < 1u << (lm - 2); ++it) xc_down_item(f, tile, log_len, o, lm, it);
    o += 1u << lm;
  }
  const int log_mb = c - 2 * levels;
  for (u32 it = 0; it < 1u << log_mb; ++it) xc_base_item(f, tile, inv, log_len, o, log_mb, it);
  for (int l = levels - 1; l >= 0; --l) {
    const int lm = c - 2 * l;
    o -= 1u << lm;
    for (u32 it = 0; it < 1u << (lm - 1); ++it) xc_up_item(f, tile, log_len, o, lm, it);
  }
}

// the launches of xc_encode_long_impl, one after the other; item numbers are the kernels' global thread indices
template <class F>
void encode_long(const F& f, const u64* w, const u64* inv, int n, int c, u64* E) {
  const XcLongPlan pl = xc_long_plan(c);
  const int log_len = c + 1, r = n - c;
  for (u64 e = 0; e < (u64)1 << n; ++e) E[((e >> c) << log_len) + (e & (((u64)1 << c) - 1))] = w[e];
  for (int k = 0; k < pl.levels; ++k)
    for (u32 it = 0; it < 1u << (r + pl.lm[k] - 2); ++it) xc_down_item(f, E, log_len, pl.off[k], pl.lm[k], it);
  const size_t m = (size_t)1 << pl.lm_i;
  std::vector<u64> tile(2 * m);
  for (u64 i = 0; i < (u64)1 << r; ++i) {
    u64* row = E + (i << log_len) + pl.off_i;
    for (size_t e = 0; e < m; ++e) tile[e] = row[e];
    sweeps(f, tile.data(), inv, pl.lm_i);
    for (size_t e = 0; e < m; ++e) row[m + e] = tile[m + e];
  }
  for (int k = pl.levels - 1; k >= 0; --k)
    for (u32 it = 0; it < 1u << (r + pl.lm[k] - 1); ++it) xc_up_item(f, E, log_len, pl.off[k], pl.lm[k], it);
}

}  // namespace

extern "C" {
// lm and off have room for kXcLongMaxLevels entries; returns the number of global levels
int xl_plan(int c, int* lm, u32* off, int* lm_i, u32* off_i) {
  const XcLongPlan pl = xc_long_plan(c);
  for (int k = 0; k < pl.levels; ++k) {
    lm[k] = pl.lm[k];
    off[k] = pl.off[k];
  }
  *lm_i = pl.lm_i;
  *off_i = pl.off_i;
  return pl.levels;
}
int xl_max_levels() { return kXcLongMaxLevels; }
// gold != 0: GoldilocksMont (p ignored), else MontGeneric of p.  w: 2^n Montgomery words; inv: the 64 words of inverses
// (Montgomery); E: 2^(n+1) words
void xl_encode_rows(u64 p, int gold, const u64* w, const u64* inv, int n, int c, u64* E) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  if (gold) encode_long(GoldilocksMont(fp), w, inv, n, c, E);
  else encode_long(MontGeneric(fp), w, inv, n, c, E);
}
}

#if defined(XC_LONG_HARNESS_MAIN)
namespace {
template <class F>
u64 power(const F& f, u64 x, u64 e) {
  u64 r = f.one();
  for (; e; e >>= 1, x = f.mul(x, x))
    if (e & 1) r = f.mul(r, x);
  return r;
}
template <class F>
int run(const F& f, u64 p, int n, int c) {
  std::vector<u64> inv(kXcInvWords, 0), w((size_t)1 << n), E((size_t)2 << n), whole((size_t)2 << n);
  u64 s = f.one();
  for (int i = 1; i < kXcInvWords; ++i, s = f.add(s, f.one())) inv[i] = power(f, s, p - 2);
  u64 x = 0x1234567;
  for (auto& v : w) v = (x = xc_mix(x + kXcGolden)) % p;
  encode_long(f, w.data(), inv.data(), n, c, E.data());
  // the whole recursion in place on the rows, as xc_encode_rows_kernel would run it on an image that large
  for (u64 i = 0; i < (u64)1 << (n - c); ++i) {
    u64* row = whole.data() + (i << (c + 1));
    for (size_t e = 0; e < (size_t)1 << c; ++e) row[e] = w[(i << c) + e];
    sweeps(f, row, inv.data(), c);
  }
  const int bad = E != whole;
  std::printf("n = %d c = %d p = %llu: %s\n", n, c, (unsigned long long)p, bad ? "DIFFERENT" : "equal");
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (int c : {14, 15}) {
    FieldParams fp;
    field_params_from_modulus(GoldilocksMont::P, &fp);
    bad |= run(GoldilocksMont(fp), GoldilocksMont::P, c + 1, c);
    const u64 p59 = 0xFFFFFFFFFFFFFFC5ull;
    field_params_from_modulus(p59, &fp);
    bad |= run(MontGeneric(fp), p59, c + 1, c);
  }
  return bad;
}
#endif
