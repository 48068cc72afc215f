// Expander-code rows longer than the LDS of a CU (expander.hpp's contract and layout, unchanged: messages of 2^14 .. 2^23 words,
// codewords of 2^15 .. 2^24): the levels too large for LDS run as plain launches over E in global memory, the recursion below
// them in LDS as before.
//
// Levels     Enc_m lives in place at [o, o + 2m) of its row: x at o, y and then z = Enc_(m/4)(y) at o + m, v at o + 3m/2.  For
//            c > 13 the levels lm = c, c - 2, .. with lm > 13 are GLOBAL (xc_long_plan: at most five, offsets o_0 = 0,
//            o_(k+1) = o_k + 2^lm_k); the first lm <= 13 - 12 or 13 - is the INNER code, at the offset behind the last global one.
// Launches   copy    (xc_long_copy_kernel)   w[i C + k] -> E[i L + k], the systematic part
//            down    (xc_long_down_kernel)   one per global level, largest first: y[q] at o + 2^lm + q, one output per thread
//            inner   (xc_long_inner_kernel)  one block per row: the message of 2^lm_i words at o_i into LDS, xc_sweeps, the
//                                            2^lm_i check words back behind it
//            up      (xc_long_up_kernel)     one per global level, smallest first: v[j] at o + 3 2^lm / 2 + j
//            A launch reads one region of a row and writes a disjoint one of the same row, so the kernel boundaries are the
//            only synchronisation: no hand-off between blocks, no atomics.
// Items      xc_down_item and xc_up_item themselves: "a tile of whole codeword rows of 2^log_len words" is E with
//            log_len = c + 1, `it` the launch's global thread index (at most 2^27 items: n + 1 <= 29).  Threads are numbered
//            row-major, so the chip works through one row after the other and the region a level gathers from - 8 2^lm bytes,
//            1 MiB at lm = 17 - is what the caches hold meanwhile.
// Traffic    copy 16 2^n bytes; a global level reads 8 R 2^lm and writes 8 R 2^(lm-2) on the way down, reads and writes
//            8 R 2^(lm-1) on the way up; the inner launch reads and writes 8 R 2^lm_i.  At c = 17 that is 39.5 2^n bytes
//            against the 24 2^n of a launch that keeps a row on chip.
#pragma once
#include "expander.hpp"

namespace sc {

constexpr int kXcLongMaxLogCols = 23;   // c at most: L = 2^24, where the stored tree is 64 L bytes = 1 GiB (as kRsLongMaxLog)
constexpr int kXcLongMaxLevels = (kXcLongMaxLogCols - kXcMaxLogCols + 1) / 2;

struct XcLongPlan {
  int levels;                    // global levels; 0 for c <= kXcMaxLogCols
  int lm[kXcLongMaxLevels];      // their log2 message lengths, descending by 2, all above kXcMaxLogCols
  u32 off[kXcLongMaxLevels];     // their offsets in the row
  int lm_i;                      // the inner code: log2 of its message length ..
  u32 off_i;                     // .. and its offset
};

SC_HD XcLongPlan xc_long_plan(int c) {
  XcLongPlan pl = {};
  int lm = c;
  u32 o = 0;
  for (; lm > kXcMaxLogCols; o += 1u << lm, lm -= 2) {
    pl.lm[pl.levels] = lm;
    pl.off[pl.levels++] = o;
  }
  pl.lm_i = lm;
  pl.off_i = o;
  return pl;
}

}  // namespace sc

#if defined(__HIPCC__)
namespace sc {

// pairs of words: C >= 2^14 and E, w 16-byte aligned (hipMalloc'ed tables)
__global__ __launch_bounds__(kBlock) void xc_long_copy_kernel(const u64* __restrict__ w, u64* __restrict__ E, int c, u64 pairs) {
  const u64 q = (u64)blockIdx.x * kBlock + threadIdx.x;
  if (q >= pairs) return;
  const u64 e = 2 * q, row = e >> c, k = e & (((u64)1 << c) - 1);
  *reinterpret_cast<ull2*>(E + (row << (c + 1)) + k) = *reinterpret_cast<const ull2*>(w + e);
}

// the grids of the two level kernels are exact: R 2^(lm-2) and R 2^(lm-1) items are multiples of kBlock for lm > 13
template <class F>
__global__ __launch_bounds__(kBlock) void xc_long_down_kernel(F f, u64* E, int log_len, u32 o, int lm) {
  xc_down_item(f, E, log_len, o, lm, blockIdx.x * (u32)kBlock + threadIdx.x);
}

template <class F>
__global__ __launch_bounds__(kBlock) void xc_long_up_kernel(F f, u64* E, int log_len, u32 o, int lm) {
  xc_up_item(f, E, log_len, o, lm, blockIdx.x * (u32)kBlock + threadIdx.x);
}

// Block i: the message at E[i L + o] (2^lm_i words, 16-byte aligned) through xc_sweeps; its check words go back behind it.
template <class F>
__global__ __launch_bounds__(kXcMaxThreads) void xc_long_inner_kernel(F f, u64* E, const u64* __restrict__ inv, int log_len, u32 o,
                                                                      int lm_i) {
  extern __shared__ __attribute__((aligned(16))) u64 xc_lds[];
  u64* lds = xc_lds;
  u64* kinv = xc_lds + ((size_t)2 << lm_i);
  u64* row = E + ((u64)blockIdx.x << log_len) + o;
  const u32 m = 1u << lm_i;
  for (u32 q = threadIdx.x; q < m / 2; q += blockDim.x) *reinterpret_cast<ull2*>(lds + 2 * q) = *reinterpret_cast<const ull2*>(row + 2 * q);
  if (threadIdx.x < (u32)kXcInvWords) kinv[threadIdx.x] = inv[threadIdx.x];
  __syncthreads();
  xc_sweeps(f, lds, kinv, lm_i, 0);
  for (u32 q = threadIdx.x; q < m / 2; q += blockDim.x) *reinterpret_cast<ull2*>(row + m + 2 * q) = *reinterpret_cast<const ull2*>(lds + m + 2 * q);
}

}  // namespace sc
#endif
