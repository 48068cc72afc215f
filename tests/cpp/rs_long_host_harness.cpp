// Host build of the split, the index maps and the twist of thaler-study_amd/csrc/kernels/ligero_long.hpp (the code
// rs_long_column_kernel and rs_long_row_kernel run, compiled for the CPU), and a replay of both steps block by block with a
// plain radix-2 transform per tile row in place of rs_radix_pass, so that they are checked against tests/ligero_ref.py
// without a GPU.
#include <vector>

#include "../../thaler-study_amd/csrc/kernels/ligero_long.hpp"
using namespace sc;

namespace {

template <class F>
u64 power(const F& f, u64 x, u64 e) {
  u64 r = f.one();
  for (; e; e >>= 1, x = f.mul(x, x))
    if (e & 1) r = f.mul(r, x);
  return r;
}

// every transform of 2^len_log words in the tile, in place: input bit-reversed, output natural, w of order 2^len_log
template <class F>
void dit_rows(const F& f, u64* tile, int tile_log, int len_log, u64 w) {
  const u32 len = 1u << len_log;
  for (u32 t = 0; t < 1u << (tile_log - len_log); ++t) {
    u64* x = tile + (size_t)t * len;
    for (u32 h = 1; h < len; h *= 2) {
      const u64 step = power(f, w, len / (2 * h));
      for (u32 base = 0; base < len; base += 2 * h) {
        u64 tw = f.one();
        for (u32 j = 0; j < h; ++j, tw = f.mul(tw, step)) {
          const u64 a = x[base + j], b = f.mul(x[base + j + h], tw);
          x[base + j] = f.add(a, b);
          x[base + j + h] = f.sub(a, b);
        }
      }
    }
  }
}

// both steps over the whole matrix; omega = w_L (Montgomery).  Step 0 places every coefficient once, at the first of the 2^rho
// positions the kernel duplicates it to, and runs ALL a levels over the zero fill: what the duplication stands for.
template <class F>
void encode_long(const F& f, u64 omega, const u64* w, int n, int c, int rho, u64* E) {
  const int log_len = c + rho;
  const RsLongSplit sp = rs_long_split(log_len);
  const u64 blocks = rs_long_blocks(sp, n + rho);
  const u64 w_a = power(f, omega, (u64)1 << sp.b), w_b = power(f, omega, (u64)1 << sp.a);
  // the twist tables as the context builds them
  const size_t n_lo = (size_t)1 << kRsTwistLoLog, n_hi = (size_t)1 << (log_len - kRsTwistLoLog);
  std::vector<u64> lo(n_lo), hi(n_hi);
  lo[0] = hi[0] = f.one();
  for (size_t i = 1; i < n_lo; ++i) lo[i] = f.mul(lo[i - 1], omega);
  const u64 step = f.mul(lo[n_lo - 1], omega);
  for (size_t i = 1; i < n_hi; ++i) hi[i] = f.mul(hi[i - 1], step);
  std::vector<u64> tile((size_t)1 << sp.tile_log);
  for (u64 blk = 0; blk < blocks; ++blk) {
    std::fill(tile.begin(), tile.end(), 0);
    for (u32 e = 0; e < 1u << (sp.tile_log - rho); ++e) tile[rs_long_pos0(sp, rho, e)] = w[rs_long_src0(sp, c, blk, e)];
    dit_rows(f, tile.data(), sp.tile_log, sp.a, w_a);
    for (u32 o = 0; o < 1u << sp.tile_log; ++o) {
      const u32 ex = rs_long_twist_exp(sp, blk, o);
      E[rs_long_dst0(sp, blk, o)] = f.mul(tile[o], f.mul(lo[ex & (n_lo - 1)], hi[ex >> kRsTwistLoLog]));
    }
  }
  for (u64 blk = 0; blk < blocks; ++blk) {
    for (u32 e = 0; e < 1u << sp.tile_log; ++e) tile[rs_long_pos1(sp, e, true)] = E[rs_long_addr1(sp, blk, e)];
    dit_rows(f, tile.data(), sp.tile_log, sp.b, w_b);
    for (u32 e = 0; e < 1u << sp.tile_log; ++e) E[rs_long_addr1(sp, blk, e)] = tile[rs_long_pos1(sp, e, false)];
  }
}

}  // namespace

extern "C" {
void rl_split(int log_len, int* a, int* b, int* tile_log) {
  const RsLongSplit sp = rs_long_split(log_len);
  *a = sp.a;
  *b = sp.b;
  *tile_log = sp.tile_log;
}
u64 rl_blocks(int log_len, int log_total) { return rs_long_blocks(rs_long_split(log_len), log_total); }
// the addresses of one block's items, in item order.  which = 0: step 0's source words of w (2^(tile_log - rho) items), 1: step
// 0's words of E (2^tile_log), 2: step 1's words of E (2^tile_log), 3: step 0's tile positions (2^(tile_log - rho)), 4 / 5: step
// 1's tile positions on the way in / out (2^tile_log), 6: step 0's twist exponents (2^tile_log)
void rl_map_block(int which, int log_len, int rho, u64 blk, u64* out) {
  const RsLongSplit sp = rs_long_split(log_len);
  const u32 count = 1u << (which == 0 || which == 3 ? sp.tile_log - rho : sp.tile_log);
  for (u32 e = 0; e < count; ++e)
    out[e] = which == 0   ? rs_long_src0(sp, log_len - rho, blk, e)
             : which == 1 ? rs_long_dst0(sp, blk, e)
             : which == 2 ? rs_long_addr1(sp, blk, e)
             : which == 3 ? rs_long_pos0(sp, rho, e)
             : which == 6 ? rs_long_twist_exp(sp, blk, e)
                          : rs_long_pos1(sp, e, which == 4);
}
// gold != 0: GoldilocksMont (p ignored), else MontGeneric of p.  omega: w_L, Montgomery; w: 2^n Montgomery words; E: 2^(n+rho)
void rl_encode(u64 p, int gold, u64 omega, const u64* w, int n, int c, int rho, u64* E) {
  FieldParams fp;
  field_params_from_modulus(gold ? GoldilocksMont::P : p, &fp);
  if (gold) encode_long(GoldilocksMont(fp), omega, w, n, c, rho, E);
  else encode_long(MontGeneric(fp), omega, w, n, c, rho, E);
}
}
