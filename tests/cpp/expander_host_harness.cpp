// Host build of the hashes and the work items of thaler-study_amd/csrc/kernels/expander.hpp (the code xc_encode_rows_kernel
// runs, compiled for the CPU) so that they are checked against tests/expander_ref.py without a GPU, and of to_mont on
// unreduced 64-bit words for both field types.
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/expander.hpp"
using namespace sc;

namespace {
// the kernel's steps over one tile of 2^tile_log codeword words, work items in order (the barriers become the loop ends)
template <class F>
void encode_tile(const F& f, u64* tile, const u64* inv, int c, int tile_log) {
  const int log_len = c + 1, log_rows = tile_log - log_len, levels = xc_levels(c);
  u32 o = 0;
  for (int l = 0; l < levels; ++l) {
    const int lm = c - 2 * l;
    for (u32 it = 0; it < 1u << (log_rows + lm - 2); ++it) xc_down_item(f, tile, log_len, o, lm, it);
    o += 1u << lm;
  }
  const int log_mb = c - 2 * levels;
  for (u32 it = 0; it < 1u << (log_rows + log_mb); ++it) xc_base_item(f, tile, inv, log_len, o, log_mb, it);
  for (int l = levels - 1; l >= 0; --l) {
    const int lm = c - 2 * l;
    o -= 1u << lm;
    for (u32 it = 0; it < 1u << (log_rows + lm - 1); ++it) xc_up_item(f, tile, log_len, o, lm, it);
  }
}
}  // namespace

extern "C" {
u64 xh_key(int lm, int side, int t) { return xc_key(lm, side, t); }
u32 xh_perm(u64 K, int b, u32 i) { return xc_perm(K, b, i); }
// gold != 0: GoldilocksMont (p ignored), else MontGeneric of p
u64 xh_coef(u64 p, int gold, u64 K, u32 e) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  return gold ? xc_coef(GoldilocksMont(fp), K, e) : xc_coef(MontGeneric(fp), K, e);
}
void xh_to_mont(u64 p, int gold, const u64* words, u64* out, size_t count) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  const GoldilocksMont g(fp);
  const MontGeneric m(fp);
  for (size_t i = 0; i < count; ++i) out[i] = gold ? g.to_mont(words[i]) : m.to_mont(words[i]);
}
int xh_levels(int c) { return xc_levels(c); }
int xh_tile_log(int log_len, int log_total) { return xc_tile_log(log_len, log_total); }
// E (2^(n+1) Montgomery words) = the encoding of the 2^(n-c) rows of w, tile by tile as the kernel's blocks take them; inv = the
// 64 words of inverses (Montgomery)
void xh_encode_rows(u64 p, int gold, const u64* w, const u64* inv, int n, int c, u64* E) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  const int tile_log = xc_tile_log(c + 1, n + 1), log_len = c + 1;
  const u32 in_words = 1u << (tile_log - 1), cmask = (1u << c) - 1;
  std::vector<u64> tile((size_t)1 << tile_log);
  for (u64 b = 0; b < (u64)1 << (n + 1 - tile_log); ++b) {
    for (u32 e = 0; e < in_words; ++e) tile[((e >> c) << log_len) + (e & cmask)] = w[b * in_words + e];
    if (gold) encode_tile(GoldilocksMont(fp), tile.data(), inv, c, tile_log);
    else encode_tile(MontGeneric(fp), tile.data(), inv, c, tile_log);
    for (size_t e = 0; e < tile.size(); ++e) E[(b << tile_log) + e] = tile[e];
  }
}
}
