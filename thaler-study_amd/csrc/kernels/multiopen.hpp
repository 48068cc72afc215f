// Part of kernels.hpp (included there, in order, after spark.hpp): batched openings - many evaluation claims about committed
// tables of one shape, one joint Ligero opening.  Two kernels: a weighted sum of eq tables, and the quadratic sumcheck pass over a
// sum of products of table pairs with shared challenges.  The work per element is in SC_HD and plain inline functions, which
// compile without hipcc: tests/cpp/multiopen_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract; the reduction of many evaluation claims to one by a sumcheck - Thaler, "Proofs, Arguments, and
// Zero-Knowledge", section 4.5.2 generalised to several polynomials, as in Chiesa, Forbes and Spooner's and HyperPlonk's batch
// openings - over the Ligero commitment of kernels/ligero.hpp, which is linear)
//
//   All tables are LE tables of Montgomery words, variable 0 first, as everywhere in the ABI.
//
//   A group is T commitments, 1 <= T <= 8, to tables f_0 .. f_(T-1) of n variables, all of one shape: the same log_rows = R,
//   log_cols = c, log_blowup and the same code (Reed-Solomon or expander), with roots root_t.  The K claims, 1 <= K <= 16, are
//   f_(t_k)(r_k) = v_k with r_k in F^n.  A table may carry several claims and a (table, point) pair may repeat; a table of the
//   group with no claim is an error.
//
//    1. Combining challenge.  V draws rho; claim k gets the coefficient rho^k.
//    2. Weight tables.  P forms one weight table per committed table: E_t(x) = sum_{k : t_k = t} rho^k eq(r_k, x), 2^n words.
//    3. Sumcheck, n rounds over sum_x sum_t f_t(x) E_t(x) = sum_k rho^k v_k, variable 0 first.  Before round j all 2T tables have
//       2^(n-j) entries; with u_i(s) = u[2i] + s (u[2i+1] - u[2i]) the message is H_j(s) = sum_t sum_i f_(t,i)(s) E_(t,i)(s) at
//       s = 0, 1, 2.  V checks H_j(0) + H_j(1) against the running claim and draws r_j; the new claim is the quadratic through the
//       three values at r_j; all tables fold by r_j.  After round n-1 the point is z = (r_0 .. r_(n-1)) and the claim is c.
//    4. No finals are sent.  V computes e_t = E_t(z) = sum_{k : t_k = t} rho^k eq(r_k, z) itself, in O(K n).  What remains is the
//       claim sum_t e_t f_t(z) = c.
//    5. Joint opening.  V draws gamma, T 2^R words.  P sends u_gamma = sum_t sum_i gamma[t][i] row_(t,i) and
//       u_z = sum_t e_t sum_i eq(z[c:], i) row_(t,i), 2^c words each.  V checks <u_z, eq(z[:c], .)> = c: the sumcheck's last check.
//       V then draws `queries` column indices - after u_gamma and u_z; one list serves all T trees.  For every index j P opens
//       column j of every commitment (2^R words and a path each); V checks the T paths against the T roots,
//       Enc(u_gamma)[j] = sum_t sum_i gamma[t][i] col_t[j][i] and Enc(u_z)[j] = sum_t e_t sum_i eq(z[c:], i) col_t[j][i].
//
//   Nothing beyond the statements of the underlying arguments is claimed: no security level, no zero knowledge, no Fiat-Shamir.
//   A joint FOLDED opening (one Basefold run over the T codewords) is not part of this.
//
// THE EQ SUM  eq_sum_kernel<F>: out[x] = sum_{k < count} coeffs[k] eq(points[k], x), count <= kEqSumMaxCount, at one multiply-add per
// entry and point (eq_table_kernel pays n multiplications per entry and point).  The index splits into lo = min(n, kEqSumLoLog)
// low bits and n - lo high bits.  A block builds the `count` low tables eq(points[k][:lo], .) in LDS once (eq_sum_low).  Then it
// takes kBlock high indices at a time: thread t forms the `count` high factors coeffs[k] eq(points[k][lo:], h) of ITS high index
// (eq_sum_high: n - lo multiplications each, amortised over 2^lo entries) into LDS, and after a barrier the block writes the
// kBlock x 2^lo entries: an item is a pair of adjacent entries of one high index, items in index order over the threads, so a
// wave's store is 64 x 16 contiguous bytes - with lo = kEqSumLoLog exactly one high index per wave instruction, whose factors are
// an LDS broadcast.  An entry is sum_k factor_k low_k[x_lo] through one lazy accumulator (eq_sum_entry).  n <= lo: one high
// index, the factors are the coefficients.  No atomics.  LDS: kEqSumMaxCount (2^kEqSumLoLog + kBlock) words = 48 KiB.
//
// THE SUM-OF-PRODUCTS PASS  sumprod_pass_kernel<F, T, FOLD>: one launch per round over the T pairs (a_t, b_t), the challenges
// SHARED by all pairs - this is one sumcheck over sum_t a_t b_t, not sc_prove_batch, whose instances are independent proofs with
// their own transcripts.  With FOLD a thread reads four consecutive entries of each of the 2T tables (two 16-byte loads per
// table), folds them by the previous challenge (zc_fold4 of kernels/r1cs.hpp), stores the two folded entries and adds the pair's
// a(s) b(s), s = 0, 1, 2, into three lazy accumulators shared across t (sp_accumulate); round 0 reads pairs and stores nothing.
// The loop over t is sequential in a thread, so register use does not grow with T.  The sums leave through reduce_cells<F, 3> /
// finish_pass<F, 3>.  Inputs are never written: the folded tables live in pool blocks the call owns.
//
// THE HOST FINISH  sp_host_rounds: the rounds over host copies of the 2T tables with the same fold and accumulate; the engine runs
// all rounds of tables of at most 2^gp_host_log entries there, and the tail of larger ones from what its last launch wrote.
//
// BYTE MODEL of the launch records (include/sumcheck_hip.h, kinds 36 and 37).  SC_KIND_EQ_SUM: log_in = n; reads the count (n + 1)
// words of points and coefficients, writes 8 * 2^n.  SC_KIND_SUMPROD_PASS: kf = 1 when the launch folded, ks = T, log_in = m for
// 2^m input entries per table; reads 2 T * 8 * 2^m and, with FOLD, writes 2 T * 8 * 2^(m-1).
#pragma once
#include <stddef.h>

#include "../field.hpp"
#include "grand_product.hpp"   // gp_host_fold, kGpMaxLog
#include "r1cs.hpp"            // zc_fold4

namespace sc {

constexpr int kEqSumMaxCount = 16;   // points per call
constexpr int kEqSumLoLog = 7;       // low bits: 2^7 entries = 64 lanes x one 16-byte pair, one high index per wave instruction
constexpr int kEqSumMaxLog = 28;     // n at most
constexpr int kSumprodMaxPairs = 8;  // T at most

// ---- the work per element ------------------------------------------------------------------------------------------------

// eq(point[:lo], x), x < 2^lo: prod_j (bit_j(x) ? point[j] : 1 - point[j])
template <class F>
SC_HD u64 eq_sum_low(const F& f, const u64* __restrict__ point, int lo, unsigned x) {
  u64 v = f.one();
  for (int j = 0; j < lo; ++j) v = f.mul(v, ((x >> j) & 1u) ? point[j] : f.sub(f.one(), point[j]));
  return v;
}

// coeff eq(point[lo:n], h), h < 2^(n-lo)
template <class F>
SC_HD u64 eq_sum_high(const F& f, const u64* __restrict__ point, int lo, int n, size_t h, u64 coeff) {
  u64 v = coeff;
  for (int j = lo; j < n; ++j) v = f.mul(v, ((h >> (j - lo)) & 1u) ? point[j] : f.sub(f.one(), point[j]));
  return v;
}

// One entry: sum_k fac[k fac_stride] low[k low_stride], k < count
template <class F>
SC_HD u64 eq_sum_entry(const F& f, int count, const u64* fac, size_t fac_stride, const u64* low, size_t low_stride) {
  typename F::Acc acc;
  f.acc_zero(acc);
  for (int k = 0; k < count; ++k) f.acc_mac(acc, fac[(size_t)k * fac_stride], low[(size_t)k * low_stride]);
  return f.acc_get(acc);
}

// One item of the sum-of-products pass: the pairs (a, b)[0..1] of one index i -> H(0..2) += a_i(s) b_i(s)
template <class F>
SC_HD void sp_accumulate(const F& f, typename F::Acc (&acc)[3], const u64 (&a)[2], const u64 (&b)[2]) {
  f.acc_mac(acc[0], a[0], b[0]);
  f.acc_mac(acc[1], a[1], b[1]);
  f.acc_mac(acc[2], f.add(a[1], f.sub(a[1], a[0])), f.add(b[1], f.sub(b[1], b[0])));
}

// ---- the host finish ---------------------------------------------------------------------------------------------------

// H(0..2) of a round over `count` pairs of host tables of 2 n_units entries
template <class F>
inline void sp_host_sums(const F& f, size_t count, u64* const* a, u64* const* b, size_t n_units, u64 (&out)[3]) {
  typename F::Acc acc[3];
  for (int s = 0; s < 3; ++s) f.acc_zero(acc[s]);
  for (size_t t = 0; t < count; ++t)
    for (size_t i = 0; i < n_units; ++i) {
      const u64 ai[2] = {a[t][2 * i], a[t][2 * i + 1]}, bi[2] = {b[t][2 * i], b[t][2 * i + 1]};
      sp_accumulate(f, acc, ai, bi);
    }
  for (int s = 0; s < 3; ++s) out[s] = f.acc_get(acc[s]);
}

// The rounds first .. first + log_len - 1 over host tables a[t], b[t], t < count, of 2^log_len entries each (folded in place; on
// return a[t][0] and b[t][0] are the finals).  `given`: H(0..2) of round `first`, when the device has already formed it, else
// null.  next(round, msg, &c) receives a round's three values and returns false to end the call - or sets the challenge c.
// challenges[first ..] receive what next() drew.  Returns false when next() did.
template <class F, class Next>
inline bool sp_host_rounds(const F& f, size_t count, u64* const* a, u64* const* b, int log_len, size_t first, const u64* given, u64* challenges,
                           Next&& next) {
  for (int j = 0; j < log_len; ++j) {
    const size_t n_units = (size_t)1 << (log_len - j - 1);
    u64 msg[3];
    if (j == 0 && given) {
      for (int s = 0; s < 3; ++s) msg[s] = given[s];
    } else {
      sp_host_sums(f, count, a, b, n_units, msg);
    }
    u64 c = 0;
    if (!next(first + (size_t)j, msg, &c)) return false;
    challenges[first + (size_t)j] = c;
    for (size_t t = 0; t < count; ++t) {
      gp_host_fold(f, c, a[t], n_units);
      gp_host_fold(f, c, b[t], n_units);
    }
  }
  return true;
}

#if defined(__HIPCC__)

// out[x] = sum_k coeffs[k] eq(points[k], x), x < 2^n.  pc: `count` rows of n words (the points), then `count` words (the
// coefficients).  1 <= count <= kEqSumMaxCount, 1 <= n <= kEqSumMaxLog.  Every block walks whole chunks of kBlock high indices, so
// the barriers are met by all its threads.
template <class F>
__global__ void __launch_bounds__(kBlock) eq_sum_kernel(F f, const u64* __restrict__ pc, int count, int n, u64* __restrict__ out) {
  __shared__ u64 low[kEqSumMaxCount << kEqSumLoLog];
  __shared__ u64 fac[kEqSumMaxCount * kBlock];
  const int lo = n < kEqSumLoLog ? n : kEqSumLoLog;
  const u64* const coeffs = pc + (size_t)count * n;
  for (int e = threadIdx.x; e < (count << lo); e += kBlock) {
    const int k = e >> lo;
    const unsigned x = (unsigned)e & ((1u << lo) - 1u);
    low[(k << kEqSumLoLog) + x] = eq_sum_low(f, pc + (size_t)k * n, lo, x);
  }
  const size_t n_high = (size_t)1 << (n - lo);
  const size_t n_chunks = (n_high + kBlock - 1) / kBlock;
  const int log_pairs = lo - 1;   // pairs of adjacent entries per high index
  for (size_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const size_t h0 = chunk * kBlock;
    const int in_chunk = (int)((n_high - h0 < (size_t)kBlock) ? n_high - h0 : (size_t)kBlock);
    __syncthreads();   // the low tables are complete; the previous chunk's factors have been read
    if ((int)threadIdx.x < in_chunk)
      for (int k = 0; k < count; ++k) fac[k * kBlock + threadIdx.x] = eq_sum_high(f, pc + (size_t)k * n, lo, n, h0 + threadIdx.x, coeffs[k]);
    __syncthreads();
    const int items = in_chunk << log_pairs;
    for (int item = threadIdx.x; item < items; item += kBlock) {
      const int hl = item >> log_pairs, q = item & ((1 << log_pairs) - 1);
      const u64 v0 = eq_sum_entry(f, count, fac + hl, kBlock, low + 2 * q, (size_t)1 << kEqSumLoLog);
      const u64 v1 = eq_sum_entry(f, count, fac + hl, kBlock, low + 2 * q + 1, (size_t)1 << kEqSumLoLog);
      *reinterpret_cast<ull2*>(out + ((h0 + (size_t)hl) << lo) + 2 * q) = ull2{v0, v1};
    }
  }
}

// One round of the sumcheck over sum_t a_t b_t.  FOLD: the tables have 4 n_units entries; unit i folds entries 4i .. 4i+3 of each
// by r into entries 2i, 2i+1 of ao[.] / bo[.] and adds them to H(0..2).  Otherwise: 2 n_units entries, nothing stored.
struct SpTables {
  const u64* a[kSumprodMaxPairs];
  const u64* b[kSumprodMaxPairs];
  u64* ao[kSumprodMaxPairs];
  u64* bo[kSumprodMaxPairs];
};
template <class F, int T, bool FOLD>
__global__ void __launch_bounds__(kBlock) sumprod_pass_kernel(F f, SpTables tb, u64 r, size_t n_units, PassOut out) {
  __shared__ u64 lds[(kBlock / kWave) * 3];
  __shared__ int lds_flag;
  typename F::Acc acc[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) f.acc_zero(acc[s]);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      u64 p[2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const u64* const in = k ? tb.b[t] : tb.a[t];
        if constexpr (FOLD) {
          const ull2* src = reinterpret_cast<const ull2*>(in) + 2 * i;
          const ull2 lo = src[0], hi = src[1];
          const u64 u[4] = {lo.x, lo.y, hi.x, hi.y};
          zc_fold4(f, r, u, p[k]);
          reinterpret_cast<ull2*>(k ? tb.bo[t] : tb.ao[t])[i] = ull2{p[k][0], p[k][1]};
        } else {
          const ull2 x = reinterpret_cast<const ull2*>(in)[i];
          p[k][0] = x.x;
          p[k][1] = x.y;
        }
      }
      sp_accumulate(f, acc, p[0], p[1]);
    }
  }
  const u64 mine = reduce_cells<F, 3>(f, acc, lds);
  finish_pass<F, 3>(f, out, mine, &lds_flag);
}

#endif   // __HIPCC__

}  // namespace sc
