// Reed-Solomon rows longer than the LDS of a CU (ligero.hpp's contract, codeword lengths 2^15 .. 2^24): a four-step transform
// through HBM, two launches and no scratch buffer.
//
// Split      l = c + rho = a + b, L1 = 2^a, L2 = 2^b, a = ceil(l / 2) (rs_long_split; a, b <= 14).  With k = k2 + L2 k1 and
//            j = j1 + L1 j2, w_L^L2 = w_L1 and w_L^L1 = w_L2:
//              E[j1 + L1 j2] = sum_{k2 < L2} w_L2^(j2 k2) ( w_L^(j1 k2) sum_{k1 < L1 / 2^rho} w_L1^(j1 k1) w[k2 + L2 k1] )
// Step 0     (rs_long_column_kernel) for every k2 the inner sum: what rs_encode_rows_kernel does for a row - L1 / 2^rho
//            coefficients, here at stride L2 in w, placed bit-reversed with the 2^rho-fold duplication, a - rho levels with the
//            table of length 2^a - then the twist w_L^(j1 k2) on the way out, T[j1 + L1 k2] into E.  A block takes the
//            2^(14-a) adjacent k2 of one tile: it reads segments of that many adjacent words and writes one run of 2^14.
// Step 1     (rs_long_row_kernel) in place on E: for every j1 the length-L2 transform over k2 (all b levels, the table of length
//            2^b).  A block takes 2^(14-b) adjacent j1: it reads T[j1 + L1 k2] for every k2 - segments of 2^(14-b) words at
//            stride L1 - and writes the same addresses back, so no block reads what another writes.
// Twist      w_L^e, e = j1 k2 < L, from two tables of the context: lo[i] = w_L^i, i < 2^12, and hi[i] = w_L^(2^12 i),
//            i < 2^(l-12): two loads and a product per word, 2^12 + 2^(l-12) host products per length.
// Traffic    step 0 reads 8 2^n and writes 8 2^(n+rho) bytes, step 1 reads and writes 8 2^(n+rho): 8 2^n (1 + 3 2^rho) against
//            the floor 8 2^n (1 + 2^rho) of a transform that keeps a row on chip.
//
// The butterflies are rs_radix_pass over the padded rs_slot image, with log_len = a or b: a tile holds 2^(14-a) or 2^(14-b)
// transforms one after the other, as a tile of rs_encode_rows_kernel holds several short rows.  The index maps below are plain
// functions of (block, item) that compile for the host, where tests/cpp/rs_long_host_harness.cpp replays both steps.
#pragma once
#include "../field.hpp"

namespace sc {

constexpr int kRsLongMaxLog = 24;       // c + rho at most: the stored tree is 64 L bytes (1 GiB), the strided segments 32 bytes
constexpr int kRsLongTileLog = 14;      // a block's tile: kRsMaxLog, the most rs_radix_pass takes
constexpr int kRsTwistLoLog = 12;       // the twist's low table: w_L^i, i < 2^12

struct RsLongSplit {
  int a, b;        // L1 = 2^a (step 0's transforms), L2 = 2^b (step 1's)
  int tile_log;    // words of a block's tile
};

SC_HD RsLongSplit rs_long_split(int log_len) {
  RsLongSplit sp;
  sp.a = (log_len + 1) / 2;
  sp.b = log_len - sp.a;
  sp.tile_log = kRsLongTileLog;
  return sp;
}

SC_HD u32 rs_bitrev(u32 x, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  return bits ? __brev(x) >> (32 - bits) : 0u;
#else
  u32 r = 0;
  for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
#endif
}

// blocks of either step: 2^(l - tile_log) per matrix row, row-major
SC_HD u64 rs_long_blocks(const RsLongSplit& sp, int log_total) { return (u64)1 << (log_total - sp.tile_log); }

// Step 0, item e < 2^(tile_log - rho) of block blk: the tile's transform t = e mod 2^(tile_log - a) is k2 = g 2^(tile_log-a) + t
// of matrix row i (blk = i 2^(l - tile_log) + g), its coefficient k1 = e >> (tile_log - a).  Adjacent items are adjacent words.
SC_HD u64 rs_long_src0(const RsLongSplit& sp, int c, u64 blk, u32 e) {
  const int per_row = sp.a + sp.b - sp.tile_log, tlog = sp.tile_log - sp.a;
  const u64 i = blk >> per_row, g = blk & (((u64)1 << per_row) - 1);
  const u32 t = e & ((1u << tlog) - 1), k1 = e >> tlog;
  return (i << c) + (g << tlog) + t + ((u64)k1 << sp.b);
}
// .. and the first of the 2^rho tile positions it fills
SC_HD u32 rs_long_pos0(const RsLongSplit& sp, int rho, u32 e) {
  const int tlog = sp.tile_log - sp.a;
  const u32 t = e & ((1u << tlog) - 1), k1 = e >> tlog;
  return (t << sp.a) + (rs_bitrev(k1, sp.a - rho) << rho);
}
// Step 0, tile word o (transform o >> a, output j1 = o mod L1): its place in E - T[j1 + L1 k2], one run per block - and the
// exponent j1 k2 of its twist
SC_HD u64 rs_long_dst0(const RsLongSplit& sp, u64 blk, u32 o) { return (blk << sp.tile_log) + o; }
SC_HD u32 rs_long_twist_exp(const RsLongSplit& sp, u64 blk, u32 o) {
  const int per_row = sp.a + sp.b - sp.tile_log, tlog = sp.tile_log - sp.a;
  const u32 g = (u32)(blk & (((u64)1 << per_row) - 1));
  const u32 k2 = (g << tlog) + (o >> sp.a), j1 = o & ((1u << sp.a) - 1);
  return j1 * k2;
}
// Step 1, item e < 2^tile_log of block blk: the tile's transform u = e mod 2^(tile_log - b) is j1 = g 2^(tile_log-b) + u of
// matrix row i, q = e >> (tile_log - b) its input k2 on the way in and its output j2 on the way out: the same word of E
SC_HD u64 rs_long_addr1(const RsLongSplit& sp, u64 blk, u32 e) {
  const int per_row = sp.a + sp.b - sp.tile_log, ulog = sp.tile_log - sp.b;
  const u64 i = blk >> per_row, g = blk & (((u64)1 << per_row) - 1);
  const u32 u = e & ((1u << ulog) - 1), q = e >> ulog;
  return (i << (sp.a + sp.b)) + (g << ulog) + u + ((u64)q << sp.a);
}
// .. and its tile position: input k2 bit-reversed, output j2 in natural order
SC_HD u32 rs_long_pos1(const RsLongSplit& sp, u32 e, bool in) {
  const int ulog = sp.tile_log - sp.b;
  const u32 u = e & ((1u << ulog) - 1), q = e >> ulog;
  return (u << sp.b) + (in ? rs_bitrev(q, sp.b) : q);
}

}  // namespace sc

#if defined(__HIPCC__)
#include "ligero.hpp"
namespace sc {

static_assert(kRsLongTileLog == kRsMaxLog, "a tile is the LDS image of rs_encode_rows_kernel");

// `left` levels from half-size 2^hlog over every transform of the tile, four at a time; a barrier behind every pass
template <class F>
__device__ __forceinline__ void rs_levels(const F& f, u64* __restrict__ lds, const u64* __restrict__ tw, const RsRoots& roots, int hlog,
                                          int left, int log_len, int tile_log) {
  for (; left >= 4; left -= 4, hlog += 4) {
    rs_radix_pass<F, 4>(f, lds, tw, roots, hlog, log_len, tile_log);
    __syncthreads();
  }
  if (left == 3) rs_radix_pass<F, 3>(f, lds, tw, roots, hlog, log_len, tile_log);
  else if (left == 2) rs_radix_pass<F, 2>(f, lds, tw, roots, hlog, log_len, tile_log);
  else if (left == 1) rs_radix_pass<F, 1>(f, lds, tw, roots, hlog, log_len, tile_log);
  if (left) __syncthreads();
}

// Step 0.  tw: the powers of w_L1; lo, hi: the twist tables of w_L.  vec: w and E are 16-byte aligned (items come in even pairs
// of adjacent words: a tile holds at least four transforms).
template <class F>
__global__ __launch_bounds__(rs_max_threads<F>()) void rs_long_column_kernel(F f, const u64* __restrict__ w, u64* __restrict__ E,
                                                                             const u64* __restrict__ tw, RsRoots roots,
                                                                             const u64* __restrict__ lo, const u64* __restrict__ hi, int c,
                                                                             int rho, int vec) {
  extern __shared__ __attribute__((aligned(16))) u64 rs_lds[];
  u64* lds = rs_lds;
  const RsLongSplit sp = rs_long_split(c + rho);
  const u64 blk = blockIdx.x;
  const u32 in_words = 1u << (sp.tile_log - rho), out_words = 1u << sp.tile_log;
  auto place = [&](u32 e, u64 x) {
    const u32 pos = rs_long_pos0(sp, rho, e);
    for (int t = 0; t < (1 << rho); ++t) lds[rs_slot(pos + t)] = x;
  };
  if (vec) {
    for (u32 q = threadIdx.x; q < in_words / 2; q += blockDim.x) {
      const ull2 x = *reinterpret_cast<const ull2*>(w + rs_long_src0(sp, c, blk, 2 * q));
      place(2 * q, x.x);
      place(2 * q + 1, x.y);
    }
  } else {
    for (u32 e = threadIdx.x; e < in_words; e += blockDim.x) place(e, w[rs_long_src0(sp, c, blk, e)]);
  }
  __syncthreads();
  rs_levels(f, lds, tw, roots, rho, sp.a - rho, sp.a, sp.tile_log);
  auto twisted = [&](u32 o, u64 x) {
    const u32 ex = rs_long_twist_exp(sp, blk, o);
    return f.mul(x, f.mul(lo[ex & ((1u << kRsTwistLoLog) - 1)], hi[ex >> kRsTwistLoLog]));
  };
  if (vec) {
    for (u32 q = threadIdx.x; q < out_words / 2; q += blockDim.x) {
      ull2 x = *reinterpret_cast<const ull2*>(lds + rs_slot(2 * q));
      x.x = twisted(2 * q, x.x);
      x.y = twisted(2 * q + 1, x.y);
      *reinterpret_cast<ull2*>(E + rs_long_dst0(sp, blk, 2 * q)) = x;
    }
  } else {
    for (u32 o = threadIdx.x; o < out_words; o += blockDim.x) E[rs_long_dst0(sp, blk, o)] = twisted(o, lds[rs_slot(o)]);
  }
}

// Step 1, in place on E.  tw: the powers of w_L2.
template <class F>
__global__ __launch_bounds__(rs_max_threads<F>()) void rs_long_row_kernel(F f, u64* __restrict__ E, const u64* __restrict__ tw, RsRoots roots,
                                                                          int log_len, int vec) {
  extern __shared__ __attribute__((aligned(16))) u64 rs_lds[];
  u64* lds = rs_lds;
  const RsLongSplit sp = rs_long_split(log_len);
  const u64 blk = blockIdx.x;
  const u32 words = 1u << sp.tile_log;
  if (vec) {
    for (u32 q = threadIdx.x; q < words / 2; q += blockDim.x) {
      const ull2 x = *reinterpret_cast<const ull2*>(E + rs_long_addr1(sp, blk, 2 * q));
      lds[rs_slot(rs_long_pos1(sp, 2 * q, true))] = x.x;
      lds[rs_slot(rs_long_pos1(sp, 2 * q + 1, true))] = x.y;
    }
  } else {
    for (u32 e = threadIdx.x; e < words; e += blockDim.x) lds[rs_slot(rs_long_pos1(sp, e, true))] = E[rs_long_addr1(sp, blk, e)];
  }
  __syncthreads();
  rs_levels(f, lds, tw, roots, 0, sp.b, sp.b, sp.tile_log);
  if (vec) {
    for (u32 q = threadIdx.x; q < words / 2; q += blockDim.x) {
      ull2 x;
      x.x = lds[rs_slot(rs_long_pos1(sp, 2 * q, false))];
      x.y = lds[rs_slot(rs_long_pos1(sp, 2 * q + 1, false))];
      *reinterpret_cast<ull2*>(E + rs_long_addr1(sp, blk, 2 * q)) = x;
    }
  } else {
    for (u32 e = threadIdx.x; e < words; e += blockDim.x) E[rs_long_addr1(sp, blk, e)] = lds[rs_slot(rs_long_pos1(sp, e, false))];
  }
}

}  // namespace sc
#endif
