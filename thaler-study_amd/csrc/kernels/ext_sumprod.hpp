// Part of kernels.hpp (included there, in order, after multiopen.hpp): the sum-of-products sumcheck of multiopen.hpp with its
// challenges drawn from a quadratic extension of the field.  The tables stay base-field words; the challenges, the round values
// and the folded tables live in the extension.  The work per element is in SC_HD and plain inline functions, which compile without
// hipcc: tests/cpp/ext_host_harness.cpp replays them.
//
// THE FIELD  K = F_p[X] / (X^2 - w), |K| = p^2.  w is a quadratic non-residue of F_p, passed by the caller as a Montgomery word; the
// engine checks w^((p-1)/2) = p - 1 on the host before any launch.  Any odd p a context accepts will do (non-residues: 7 for
// Goldilocks, 2 for 2^64 - 59, 3 for 2^61 - 1, 2^32 + 15 and 257).  An element is two Montgomery words (c0, c1), meaning c0 + c1 X;
// it crosses the ABI as two consecutive words.  A product is three base multiplications, Karatsuba style (ext_mul):
//     s00 = x0 y0,  s11 = x1 y1,  sm = (x0 + x1)(y0 + y1);   x y = (s00 + w s11,  sm - s00 - s11)
// and one more by the constant w.
//
// THE LAYOUT  Inside the engine an extension table of 2^m entries is two PLANES of 2^m words in one pool block: all c0 words, then
// all c1 words.  Every load and store of the pass then has the shape of sumprod_pass_kernel's (a lane reads and writes 16
// contiguous bytes, a wave 1 KiB), and a base-field table is simply a c0 plane with no c1.  The layout never crosses the ABI.
//
// THE PROTOCOL  The sumcheck of multiopen.hpp, step 3, over sum_x sum_t a_t(x) b_t(x), n rounds, variable 0 first, with r_j in K.
// Round 0 is over base-field tables and no challenge is drawn yet: it is sumprod_pass_kernel<F, T, false>, its three words the c0
// of H(0..2), every c1 = 0.  A round's message is H(0).c0, H(0).c1, H(1).c0, H(1).c1, H(2).c0, H(2).c1.
//
// THE PASS  ext_sumprod_pass_kernel<F, T, BASE_IN>: one launch per round j >= 1.  A thread takes a unit of four consecutive entries
// of each of the 2T tables.  BASE_IN (round 1): it reads base words exactly as the FOLD form of sumprod_pass_kernel does and folds
// them by r in K into two extension entries, c0 = u0 + r.c0 (u1 - u0), c1 = r.c1 (u1 - u0) (ext_fold_base: two base
// multiplications per folded entry).  Otherwise it reads both planes and folds with one K-product per folded entry (ext_fold).
// Both store both planes.  For s = 0, 1, 2, with a(2) = 2 a_1 - a_0 componentwise, it adds the three Karatsuba partial products of
// a(s) b(s) into lazy accumulators: nine per thread, shared across t (ext_accumulate).  The loop over t is sequential, so register
// use does not grow with T.  A thread adds at most T 2^(kGpMaxLog - 2) / kBlock = 2^21 products to an accumulator (one block, n = 28,
// round 1), far below kAccMaxTerms.
//
// NINE SUMS, SIX WORDS  The map from the nine sums (S00, S11, Sm per s) to the words of H(s) = (S00 + w S11, Sm - S00 - S11) is
// linear, so it commutes with the sum over blocks.  Every block applies it to ITS nine block sums (reduce_cells<F, 9>, then six
// threads form one word each: ext_cells_to_words) and the launch leaves through finish_pass<F, 6> as it is: finish_pass publishes the
// cells it is given, so a map in the last block would have to live inside it, and it is shared by every prover.  The price is one
// multiplication by w in three threads of every block; the last block sums six rows of partials instead of nine.
//
// THE FOLD-ONLY KERNEL  ext_fold_kernel<F, BASE_IN>: the same two folds over one table, nothing accumulated - sc_table_evaluate_ext.
//
// THE HOST FINISH  ext_host_rounds: the rounds over host copies of the planes with the same folds, accumulate and nine-to-six map;
// the engine runs all rounds of tables of at most 2^gp_host_log entries there (from base words: the first fold is ext_fold_base),
// and the tail of larger ones from what its last launch wrote.  The transcript is the same wherever the hand-over falls: every
// function returns reduced words, and a reduced word is unique.
//
// BYTE MODEL of the launch records (include/sumcheck_hip.h, kind 38).  SC_KIND_SUMPROD_EXT_PASS: kf = 1 for base tables in, 2 for
// extension tables in; ks = T (0: the fold-only kernel, one table); log_in = m for 2^m entries per input table.  Reads
// 2 T * 8 * 2^m (kf = 1) or 2 T * 16 * 2^m (kf = 2), writes 2 T * 16 * 2^(m-1); fold-only: the same with 2 T replaced by 1.
#pragma once
#include <stddef.h>

#include "../field.hpp"
#include "multiopen.hpp"   // kSumprodMaxPairs, sp_host_sums

namespace sc {

// ---- the work per element ------------------------------------------------------------------------------------------------

// x y in K, Karatsuba style
template <class F>
SC_HD void ext_mul(const F& f, u64 w, const u64 (&x)[2], const u64 (&y)[2], u64 (&o)[2]) {
  const u64 s00 = f.mul(x[0], y[0]), s11 = f.mul(x[1], y[1]), sm = f.mul(f.add(x[0], x[1]), f.add(y[0], y[1]));
  o[0] = f.add(s00, f.mul(w, s11));
  o[1] = f.sub(f.sub(sm, s00), s11);
}

// two base words folded by r in K: u0 + r (u1 - u0)
template <class F>
SC_HD void ext_fold_base(const F& f, const u64 (&r)[2], u64 u0, u64 u1, u64 (&o)[2]) {
  const u64 d = f.sub(u1, u0);
  o[0] = f.add(u0, f.mul(r[0], d));
  o[1] = f.mul(r[1], d);
}

// two extension entries folded by r in K
template <class F>
SC_HD void ext_fold(const F& f, u64 w, const u64 (&r)[2], const u64 (&u0)[2], const u64 (&u1)[2], u64 (&o)[2]) {
  const u64 d[2] = {f.sub(u1[0], u0[0]), f.sub(u1[1], u0[1])};
  u64 m[2];
  ext_mul(f, w, r, d, m);
  o[0] = f.add(u0[0], m[0]);
  o[1] = f.add(u0[1], m[1]);
}

// One item of the pass: the pair of adjacent entries a[0], a[1] and b[0], b[1] of one index ([entry][component]) -> the partial
// products of a(s) b(s), s = 0, 1, 2: acc[3 s] += c0 c0, acc[3 s + 1] += c1 c1, acc[3 s + 2] += (c0 + c1)(c0 + c1)
template <class F>
SC_HD void ext_accumulate(const F& f, typename F::Acc (&acc)[9], const u64 (&a)[2][2], const u64 (&b)[2][2]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int s = 0; s < 3; ++s) {
    u64 x[2], y[2];
    for (int c = 0; c < 2; ++c) {
      x[c] = s == 0 ? a[0][c] : s == 1 ? a[1][c] : f.add(a[1][c], f.sub(a[1][c], a[0][c]));
      y[c] = s == 0 ? b[0][c] : s == 1 ? b[1][c] : f.add(b[1][c], f.sub(b[1][c], b[0][c]));
    }
    f.acc_mac(acc[3 * s], x[0], y[0]);
    f.acc_mac(acc[3 * s + 1], x[1], y[1]);
    f.acc_mac(acc[3 * s + 2], f.add(x[0], x[1]), f.add(y[0], y[1]));
  }
}

// word k < 6 of the message from the nine sums: H(s).c0 = S00 + w S11 (k = 2 s), H(s).c1 = Sm - S00 - S11 (k = 2 s + 1)
template <class F>
SC_HD u64 ext_cells_to_word(const F& f, u64 w, const u64* cells, int k) {
  const u64* c = cells + 3 * (k >> 1);
  return (k & 1) ? f.sub(f.sub(c[2], c[0]), c[1]) : f.add(c[0], f.mul(w, c[1]));
}

// ---- the host finish ---------------------------------------------------------------------------------------------------

// A host table is two planes: pl[2 q] the c0 words, pl[2 q + 1] the c1 words of table q, q < 2 count (a_0 .., b_0 ..).

// the six words of a round over `count` pairs of host tables of 2 n_units entries
template <class F>
inline void ext_host_sums(const F& f, u64 w, size_t count, u64* const* pl, size_t n_units, u64 (&out)[6]) {
  typename F::Acc acc[9];
  for (int s = 0; s < 9; ++s) f.acc_zero(acc[s]);
  for (size_t t = 0; t < count; ++t) {
    const u64 *a0 = pl[2 * t], *a1 = pl[2 * t + 1], *b0 = pl[2 * (count + t)], *b1 = pl[2 * (count + t) + 1];
    for (size_t i = 0; i < n_units; ++i) {
      const u64 ai[2][2] = {{a0[2 * i], a1[2 * i]}, {a0[2 * i + 1], a1[2 * i + 1]}};
      const u64 bi[2][2] = {{b0[2 * i], b1[2 * i]}, {b0[2 * i + 1], b1[2 * i + 1]}};
      ext_accumulate(f, acc, ai, bi);
    }
  }
  u64 cells[9];
  for (int s = 0; s < 9; ++s) cells[s] = f.acc_get(acc[s]);
  for (int k = 0; k < 6; ++k) out[k] = ext_cells_to_word(f, w, cells, k);
}

// one table of 2 n_out entries folded in place by r; base: the c1 plane is not read (the entries are base words)
template <class F>
inline void ext_host_fold(const F& f, u64 w, const u64 (&r)[2], u64* c0, u64* c1, size_t n_out, bool base) {
  for (size_t i = 0; i < n_out; ++i) {
    u64 o[2];
    if (base) {
      ext_fold_base(f, r, c0[2 * i], c0[2 * i + 1], o);
    } else {
      const u64 u0[2] = {c0[2 * i], c1[2 * i]}, u1[2] = {c0[2 * i + 1], c1[2 * i + 1]};
      ext_fold(f, w, r, u0, u1, o);
    }
    c0[i] = o[0];
    c1[i] = o[1];
  }
}

// The rounds first .. first + log_len - 1 over the host planes pl[.] of 2 count tables of 2^log_len entries each (folded in place;
// on return pl[2 q][0], pl[2 q + 1][0] are the finals).  base_in: the tables are base words - the c1 planes hold zeros and the first
// fold is the base fold.  `given`: the six words of round `first`, when the device has already formed them, else null.
// next(round, msg, c) receives a round's six words and returns false to end the call - or sets the challenge c[0..1].
// challenges[2 (first ..)] receive what next() drew.  Returns false when next() did.
template <class F, class Next>
inline bool ext_host_rounds(const F& f, u64 w, size_t count, u64* const* pl, int log_len, size_t first, bool base_in, const u64* given,
                            u64* challenges, Next&& next) {
  for (int j = 0; j < log_len; ++j) {
    const size_t n_units = (size_t)1 << (log_len - j - 1);
    u64 msg[6];
    if (j == 0 && given) {
      for (int s = 0; s < 6; ++s) msg[s] = given[s];
    } else {
      ext_host_sums(f, w, count, pl, n_units, msg);
    }
    u64 c[2] = {0, 0};
    if (!next(first + (size_t)j, msg, c)) return false;
    challenges[2 * (first + (size_t)j)] = c[0];
    challenges[2 * (first + (size_t)j) + 1] = c[1];
    for (size_t q = 0; q < 2 * count; ++q) ext_host_fold(f, w, c, pl[2 * q], pl[2 * q + 1], n_units, base_in && j == 0);
  }
  return true;
}

// one table of 2^log_len entries folded by point[0 .. log_len) in place: its multilinear extension at the point ends in c0[0], c1[0]
template <class F>
inline void ext_host_evaluate(const F& f, u64 w, u64* c0, u64* c1, int log_len, const u64* point, bool base_in) {
  for (int j = 0; j < log_len; ++j) {
    const u64 r[2] = {point[2 * j], point[2 * j + 1]};
    ext_host_fold(f, w, r, c0, c1, (size_t)1 << (log_len - j - 1), base_in && j == 0);
  }
}

#if defined(__HIPCC__)

static_assert(((u64)kSumprodMaxPairs << (kGpMaxLog - 2)) / kBlock <= GoldilocksMont::kAccMaxTerms &&
                  ((u64)kSumprodMaxPairs << (kGpMaxLog - 2)) / kBlock <= MontGeneric::kAccMaxTerms,
              "the products one thread of ext_sumprod_pass_kernel adds to a lazy accumulator (one block, the largest table)");

// a unit: entries 4 i .. 4 i + 3 of one table (BASE_IN: base words at `in`; else planes at in, in + 4 n_units) folded by r into
// entries 2 i, 2 i + 1 of the planes at out, out + 2 n_units; p[entry][component] receives them
template <class F, bool BASE_IN>
__device__ __forceinline__ void ext_fold_unit(const F& f, u64 w, const u64 (&r)[2], const u64* __restrict__ in, u64* __restrict__ out,
                                              size_t n_units, size_t i, u64 (&p)[2][2]) {
  const ull2* src = reinterpret_cast<const ull2*>(in) + 2 * i;
  const ull2 lo = src[0], hi = src[1];
  if constexpr (BASE_IN) {
    ext_fold_base(f, r, lo.x, lo.y, p[0]);
    ext_fold_base(f, r, hi.x, hi.y, p[1]);
  } else {
    const ull2* src1 = reinterpret_cast<const ull2*>(in + 4 * n_units) + 2 * i;
    const ull2 lo1 = src1[0], hi1 = src1[1];
    const u64 u[4][2] = {{lo.x, lo1.x}, {lo.y, lo1.y}, {hi.x, hi1.x}, {hi.y, hi1.y}};
    ext_fold(f, w, r, u[0], u[1], p[0]);
    ext_fold(f, w, r, u[2], u[3], p[1]);
  }
  reinterpret_cast<ull2*>(out)[i] = ull2{p[0][0], p[1][0]};
  reinterpret_cast<ull2*>(out + 2 * n_units)[i] = ull2{p[0][1], p[1][1]};
}

// One round j >= 1 of the sumcheck over sum_t a_t b_t with challenges in K.  The tables have 4 n_units entries (BASE_IN: base
// words; else two planes of 4 n_units words); unit i folds entries 4i .. 4i+3 of each by r = (r0, r1) into entries 2i, 2i+1 of the
// planes at ao[.] / bo[.] (2 n_units words each) and adds them to the nine sums.  Six words leave: H(0..2) of the round.
template <class F, int T, bool BASE_IN>
__global__ void __launch_bounds__(kBlock) ext_sumprod_pass_kernel(F f, SpTables tb, u64 w, u64 r0, u64 r1, size_t n_units, PassOut out) {
  __shared__ u64 lds[(kBlock / kWave) * 9];
  __shared__ u64 cells[9];
  __shared__ int lds_flag;
  const u64 r[2] = {r0, r1};
  typename F::Acc acc[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) f.acc_zero(acc[s]);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      u64 p[2][2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k) ext_fold_unit<F, BASE_IN>(f, w, r, k ? tb.b[t] : tb.a[t], k ? tb.bo[t] : tb.ao[t], n_units, i, p[k]);
      ext_accumulate(f, acc, p[0], p[1]);
    }
  }
  const u64 mine = reduce_cells<F, 9>(f, acc, lds);
  if (threadIdx.x < 9) cells[threadIdx.x] = mine;
  __syncthreads();
  const u64 word = threadIdx.x < 6 ? ext_cells_to_word(f, w, cells, (int)threadIdx.x) : 0;
  finish_pass<F, 6>(f, out, word, &lds_flag);
}

// The fold alone, one table: 4 n_units entries in, 2 n_units out (both planes).
template <class F, bool BASE_IN>
__global__ void __launch_bounds__(kBlock) ext_fold_kernel(F f, const u64* __restrict__ in, u64* __restrict__ out, u64 w, u64 r0, u64 r1,
                                                          size_t n_units) {
  const u64 r[2] = {r0, r1};
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 p[2][2];
    ext_fold_unit<F, BASE_IN>(f, w, r, in, out, n_units, i, p);
  }
}

#endif   // __HIPCC__

}  // namespace sc
