// "Expander code 1": a linear-time, systematic, rate-1/2 code in Spielman's recursive shape (Thaler, "Proofs, Arguments, and
// Zero-Knowledge", section 10.5: Ligero with a linear-time code, as in Brakedown; the reference has no such crate), the row
// code of the Ligero-style commitment for fields WITHOUT two-adicity.  Only additions and multiplications by constants: any
// prime p > 63 is served, 2^64 - 59 included.
//
// Contract   All arithmetic in F_p on canonical integers (the device holds Montgomery words).  A message x of m = 2^c words
//            encodes to Enc_m(x) of L = 2 m words:
//              M64 = 2^64 - 1; SEED = 0x4272616B65646F77; GOLDEN = 0x9E3779B97F4A7C15; D_A = 8; D_B = 16
//              mix(x)          x &= M64; x ^= x>>30; x = x 0xBF58476D1CE4E5B9 & M64; x ^= x>>27; x = x 0x94D049BB133111EB & M64; x ^= x>>31
//              key(lm,side,t)  mix(SEED + ((lm<<16) | (side<<8) | t))
//              coef(K,e)       mix(K + (e+1) GOLDEN) mod p, and 1 where that is 0
//              frnd(K,r,v)     u = ((v ^ ((K >> 8r) & 0xFFFFFFFF)) 0x9E3779B1) mod 2^32; u ^= u>>15; u = u 0x85EBCA77 mod 2^32; u ^= u>>13
//              perm(K,b,i)     bl = b>>1, bh = b - bl; lo = i & (2^bl - 1); hi = i >> bl; r = 0..3: r even: hi ^= frnd(K,r,lo) & (2^bh - 1),
//                              r odd: lo ^= frnd(K,r,hi) & (2^bl - 1); result (hi << bl) | lo - a four-round Feistel network, a bijection
//              m <= 32 (base)  x || K x, K[j][k] = (j + k + 1)^-1: a Cauchy matrix, so [I | K] is MDS, distance m + 1
//              m >= 64         y[e>>2] += coef(K,e) x[perm(K,lm,e)]    t < D_A, K = key(lm,0,t), e < m     (y of m/4 words)
//                              z = Enc_(m/4)(y)                                                           (m/2 words)
//                              v[j] += coef(K,j) z[perm(K,lm-1,j)]     t < D_B, K = key(lm,1,t), j < m/2   (m/2 words)
//                              result x || z || v
//            Both maps are sums of weighted permutation matrices (every input of A used D_A times, of B D_B times): they are
//            defined by gathers alone - nothing is stored, nothing is scattered.  The relative distance of the recursive
//            code is NOT proved; the base code's distance is exact.
// Layout     In place, Enc_m at [o, o + 2m): x at o; y at o + m and z = Enc_(m/4)(y) over it at [o + m, o + 3m/2); v at o + 3m/2.
// Limits     c <= 13 (one codeword, 128 KiB, in the LDS of a CU; expander_long.hpp serves c up to 23); n + 1 <= 29; p > 63; one
//            device, one rank.
//
// xc_encode_rows_kernel: a block owns 2^tile_log codeword words in LDS - one row, or several when L < 2^12.  A "down" sweep
// writes each level's y behind its input (32 gathered products per output, accumulated unreduced), one dense product with the
// base matrix follows, then an "up" sweep writes each level's v (16 products per output); a barrier after every step,
// 2 levels + 1 in all.  K[j][k] depends on j + k alone, so the base matrices of every m <= 32 are one table of the 63 inverses
// 1/1 .. 1/63 (Montgomery), built by the host once per context and copied to LDS.  Permutations and coefficients are
// generated on the fly: frnd is 32-bit arithmetic, coef one mix and one Montgomery product with R^2 (to_mont takes the
// unreduced 64-bit hash on both field types: its product with R^2 mod p is below p 2^64, which is all redc asks).
// The gathers are random 8-byte LDS reads and conflict; that is the code, not the layout.  Writes are consecutive.
#pragma once
#include "../field.hpp"
#include "row_code.hpp"

namespace sc {

constexpr int kXcMaxLogCols = 13;    // c at most: L = 2^14 words in LDS
constexpr int kXcMaxThreads = 1024;
constexpr int kXcDegA = 8, kXcDegB = 16;
constexpr int kXcBaseLog = 5;        // messages of up to 2^5 words take the base code
constexpr int kXcInvWords = 64;      // the table of inverses: entry s = 1/s, s = 1 .. 63 (entry 0 unused)
constexpr u64 kXcSeed = 0x4272616B65646F77ull;
constexpr u64 kXcGolden = 0x9E3779B97F4A7C15ull;

inline int xc_tile_log(int log_len, int log_total) { return row_tile_log(log_len, log_total); }   // the host harness's name for it
SC_HD int xc_levels(int c) { return c > kXcBaseLog ? (c - kXcBaseLog + 1) / 2 : 0; }
inline int xc_threads(int tile_log) {
  const int t = 1 << (tile_log > 2 ? tile_log - 2 : 0);
  return t < 64 ? 64 : (t > kXcMaxThreads ? kXcMaxThreads : t);
}
SC_HD size_t xc_lds_words(int tile_log) { return ((size_t)1 << tile_log) + kXcInvWords; }

SC_HD u64 xc_mix(u64 x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
SC_HD u64 xc_key(int lm, int side, int t) { return xc_mix(kXcSeed + (((u64)lm << 16) | ((u64)side << 8) | (u64)t)); }
SC_HD u32 xc_frnd(u64 K, int r, u32 v) {
  u32 u = (v ^ (u32)(K >> (8 * r))) * 0x9E3779B1u;
  u ^= u >> 15;
  u *= 0x85EBCA77u;
  return u ^ (u >> 13);
}
SC_HD u32 xc_perm(u64 K, int b, u32 i) {
  const int bl = b >> 1, bh = b - bl;
  const u32 ml = (1u << bl) - 1, mh = (1u << bh) - 1;
  u32 lo = i & ml, hi = i >> bl;
  hi ^= xc_frnd(K, 0, lo) & mh;
  lo ^= xc_frnd(K, 1, hi) & ml;
  hi ^= xc_frnd(K, 2, lo) & mh;
  lo ^= xc_frnd(K, 3, hi) & ml;
  return (hi << bl) | lo;
}
// coef(K, e) as a Montgomery word
template <class F>
SC_HD u64 xc_coef(const F& f, u64 K, u32 e) {
  const u64 w = f.to_mont(xc_mix(K + (u64)(e + 1) * kXcGolden));
  return w ? w : f.one();
}

// The three kinds of work item, on a tile of whole codeword rows of 2^log_len words (the kernel's LDS image; host code in the
// tests replays them).  `it` numbers the outputs of a step over the rows of the tile: row = it >> (log2 of outputs per row).
// down, level with 2^lm inputs at offset o of its row: y[q] = sum over t < D_A and the four e = 4 q + s of
// coef(K_t, e) x[perm(K_t, lm, e)], written at o + 2^lm + q
template <class F>
SC_HD void xc_down_item(const F& f, u64* tile, int log_len, u32 o, int lm, u32 it) {
  const int log_out = lm - 2;
  const u32 q = it & ((1u << log_out) - 1);
  u64* x = tile + ((size_t)(it >> log_out) << log_len) + o;
  typename F::Acc acc;
  f.acc_zero(acc);
#pragma unroll 1
  for (int t = 0; t < kXcDegA; ++t) {
    const u64 K = xc_key(lm, 0, t);
#pragma unroll
    for (u32 s = 0; s < 4; ++s) f.acc_mac(acc, x[xc_perm(K, lm, 4 * q + s)], xc_coef(f, K, 4 * q + s));
  }
  x[(1u << lm) + q] = f.acc_get(acc);
}
// base: the message of 2^log_mb <= 32 words at o, (K x)[j] written at o + 2^log_mb + j; inv[s] = 1/s
template <class F>
SC_HD void xc_base_item(const F& f, u64* tile, const u64* inv, int log_len, u32 o, int log_mb, u32 it) {
  const u32 mb = 1u << log_mb, j = it & (mb - 1);
  u64* x = tile + ((size_t)(it >> log_mb) << log_len) + o;
  typename F::Acc acc;
  f.acc_zero(acc);
  for (u32 k = 0; k < mb; ++k) f.acc_mac(acc, x[k], inv[j + k + 1]);
  x[mb + j] = f.acc_get(acc);
}
// up, level with 2^lm inputs at o: v[j] = sum over t < D_B of coef(K_t, j) z[perm(K_t, lm - 1, j)], z at o + 2^lm, v at
// o + 3 2^lm / 2
template <class F>
SC_HD void xc_up_item(const F& f, u64* tile, int log_len, u32 o, int lm, u32 it) {
  const int log_out = lm - 1;
  const u32 j = it & ((1u << log_out) - 1);
  u64* z = tile + ((size_t)(it >> log_out) << log_len) + o + (1u << lm);
  typename F::Acc acc;
  f.acc_zero(acc);
#pragma unroll 1
  for (int t = 0; t < kXcDegB; ++t) {
    const u64 K = xc_key(lm, 1, t);
    f.acc_mac(acc, z[xc_perm(K, lm - 1, j)], xc_coef(f, K, j));
  }
  z[(1u << log_out) + j] = f.acc_get(acc);
}

}  // namespace sc

#if defined(__HIPCC__)
namespace sc {

// The sweeps over an LDS image of 2^log_rows codeword rows of 2^(c+1) words whose messages are in place: every level's down step,
// the base product, every level's up step, a barrier behind each.  The caller's barrier stands between its loads and this.
template <class F>
__device__ __forceinline__ void xc_sweeps(const F& f, u64* lds, const u64* kinv, int c, int log_rows) {
  const int log_len = c + 1;
  const int levels = xc_levels(c);
  u32 o = 0;
  for (int l = 0; l < levels; ++l) {
    const int lm = c - 2 * l;
    const u32 items = 1u << (log_rows + lm - 2);
    for (u32 it = threadIdx.x; it < items; it += blockDim.x) xc_down_item(f, lds, log_len, o, lm, it);
    __syncthreads();
    o += 1u << lm;
  }
  {
    const int log_mb = c - 2 * levels;
    const u32 items = 1u << (log_rows + log_mb);
    for (u32 it = threadIdx.x; it < items; it += blockDim.x) xc_base_item(f, lds, kinv, log_len, o, log_mb, it);
    __syncthreads();
  }
  for (int l = levels - 1; l >= 0; --l) {
    const int lm = c - 2 * l;
    o -= 1u << lm;
    const u32 items = 1u << (log_rows + lm - 1);
    for (u32 it = threadIdx.x; it < items; it += blockDim.x) xc_up_item(f, lds, log_len, o, lm, it);
    __syncthreads();
  }
}

// One block encodes 2^(tile_log - c - 1) consecutive rows: their messages are one contiguous run of w, their codewords one
// contiguous run of E.  inv: the kXcInvWords inverses.  vec: both runs are 16-byte aligned and a row is at least two words.
template <class F>
__global__ __launch_bounds__(kXcMaxThreads) void xc_encode_rows_kernel(F f, const u64* __restrict__ w, u64* __restrict__ E,
                                                                       const u64* __restrict__ inv, int c, int tile_log, int vec) {
  extern __shared__ __attribute__((aligned(16))) u64 xc_lds[];
  u64* lds = xc_lds;
  u64* kinv = xc_lds + ((size_t)1 << tile_log);
  const int log_len = c + 1, log_rows = tile_log - log_len;
  const u32 in_words = 1u << (tile_log - 1), cmask = (1u << c) - 1;
  const u64* src = w + (u64)blockIdx.x * in_words;
  u64* dst = E + ((u64)blockIdx.x << tile_log);
  // in: word k of local row q -> q L + k
  if (vec) {
    for (u32 q = threadIdx.x; q < in_words / 2; q += blockDim.x) {
      const u32 e = 2 * q;
      *reinterpret_cast<ull2*>(lds + ((e >> c) << log_len) + (e & cmask)) = *reinterpret_cast<const ull2*>(src + e);
    }
  } else {
    for (u32 e = threadIdx.x; e < in_words; e += blockDim.x) lds[((e >> c) << log_len) + (e & cmask)] = src[e];
  }
  if (threadIdx.x < (u32)kXcInvWords) kinv[threadIdx.x] = inv[threadIdx.x];
  __syncthreads();
  xc_sweeps(f, lds, kinv, c, log_rows);
  // out: the whole tile, one coalesced run
  const u32 out_words = 1u << tile_log;
  if (vec) {
    for (u32 q = threadIdx.x; q < out_words / 2; q += blockDim.x) *reinterpret_cast<ull2*>(dst + 2 * q) = *reinterpret_cast<const ull2*>(lds + 2 * q);
  } else {
    for (u32 e = threadIdx.x; e < out_words; e += blockDim.x) dst[e] = lds[e];
  }
}

}  // namespace sc
#endif
