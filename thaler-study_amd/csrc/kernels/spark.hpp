// Part of kernels.hpp (included there, in order, after fraction.hpp): SPARK over LogUp - a committed sparse matrix and the proof of
// sum_k val_k U[row_k] W[col_k]: the gather of both dimensions, the (index, value) tuples of the two indexed lookups, and the
// preprocessing that turns the u32 indices into field-word tables and counts.  The work per element is in SC_HD and plain inline
// functions, which compile without hipcc: tests/cpp/spark_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract; Setty, "Spartan", section 7: SPARK; Setty, Thaler and Wahby, "Lasso", section 4: the memory check
// replaced by a lookup whose read counts are multiplicities; Haboeck, "Multivariate lookups based on logarithmic derivatives" and
// Papini and Haboeck, "Improving logarithmic derivative lookups using GKR": the fraction sum, kernels/fraction.hpp)
//
//   All tables are LE tables of Montgomery words, variable 0 first, as everywhere in the ABI.
//
//   Objects.  M in F^(2^a x 2^b) is a list of nnz >= 1 triples (row_k, col_k, val_k); equal (row, col) pairs are allowed and add.
//   The list is padded with (0, 0, 0) to N = 2^l entries, l = max(1, ceil(log2 nnz)).  Tables of l variables: row and col (the
//   indices as field words) and val.  cr[i] = #{k < N : row_k = i} has a variables, cc[j] = #{k < N : col_k = j} has b; the
//   padding counts in cr[0] and cc[0].
//
//   Preprocessing, once per matrix and honest: five Ligero commitments, to row, col, val, cr and cc.  The counts depend on the
//   matrix alone, so they are committed with it and not once per proof.
//
//   Claim.  U (2^a words) and W (2^b words) are tables whose extensions the verifier evaluates itself, through callbacks
//   u_eval(point) and w_eval(point).  The claim is v = sum_{k < N} val_k U[row_k] W[col_k].  With U = eq(r_x, .) and
//   W = eq(r_y, .) this is M~(r_x, r_y).
//
//   Exchange.
//    1. P gathers er[k] = U[row_k] and ec[k] = W[col_k], commits to both, and sends the two roots and v.
//    2. A cubic sumcheck of l rounds over sum_x val(x) er(x) ec(x) = v, variable 0 first.  Before round j the tables have
//       2^(l-j) entries; with u_i(t) = u[2i] + t (u[2i+1] - u[2i]) the message is H_j(t) = sum_i val_i(t) er_i(t) ec_i(t) at
//       t = 0, 1, 2, 3.  V checks H_j(0) + H_j(1) against the running claim (v at first) and draws r_j; the new claim is the cubic
//       through the four values at r_j; the three tables fold by r_j (kernels/grand_product.hpp: the same checks, interpolation
//       and folds).  P sends the finals (f_v, f_r, f_c), the tables' extensions at r; V checks f_v f_r f_c against the last claim.
//    3. V draws beta, then alpha - after the roots of step 1.  Then for each dimension d in {row, col}, with
//       (idx, e, T, cnt) = (row, er, U, cr) or (col, ec, W, cc):
//        - P forms den_w[k] = alpha - idx_k - beta e[k], k < N, and den_t[i] = alpha - i - beta T[i], i < 2^a (2^b).
//        - P builds the fraction trees of (1, den_w) and of (cnt, den_t) and sends the roots (P_w, Q_w), (P_t, Q_t).
//        - V refuses Q_w = 0 or Q_t = 0, and refuses P_w Q_t != P_t Q_w.
//        - Both fraction sums run under V's draws (kernels/fraction.hpp, unchanged).
//        - The w side ends at z with a_l = 1 and b_l = alpha - idx~(z) - beta e~(z).
//        - The t side ends at z' with a' = cnt~(z') and b' = alpha - id~(z') - beta T~(z'); id~(z') = sum_j 2^j z'_j and T~ is
//          the verifier's callback.
//    4. Nine single openings, each plain, folded or of the expander code: val at r; er at r and z_row; ec at r and z_col; row at
//       z_row; col at z_col; cr at z'_row; cc at z'_col.  The values at r must be the finals; those at z and z' must satisfy the
//       two identities of step 3.
//
//   Limits and refusals.  1 <= l, a, b <= 28.  p > 3 (interpolation on {0, 1, 2, 3}) and p > 2^max(l, a, b): counts and indices
//   must be field words.  One device and one rank.  Nothing beyond the papers' statements is claimed: no security level, no zero
//   knowledge, no Fiat-Shamir.
//
// THE GATHER  spark_gather_kernel<F>: both dimensions in one launch.  A thread owns four consecutive k: one 16-byte load of row
// (u32) and one of col, eight 8-byte gathers from U and W, two 16-byte lane-contiguous stores to each of er and ec.  N = 2 is
// smaller than a thread's unit: thread 0 takes the one pair with 8-byte index loads and one store per table.  The indices were
// validated when the matrix was made (sc_spark_create), so every gather is inside its table.
//
// THE TUPLES  spark_tuple_kernel<F, IOTA>: out[i] = alpha - key_i - beta v[i]; key comes from a u32 stream, or with IOTA is the
// index i itself; the integer is turned into a Montgomery word in the kernel (spark_key_word).  Four entries per thread, every
// access 16 bytes wide; tables of two entries take the same tail.
//
// THE PREPROCESSING  spark_index_kernel<F, LDS>, one launch per dimension: a thread takes four indices (one 16-byte load),
// stores their Montgomery words (two 16-byte stores) and adds one to the u32 counter of each - a thread whose four indices are
// equal adds four at once, and a wave whose lanes all hold that one index adds once (spark_count4: the padding, and a dense
// column of an R1CS instance, are long runs of one index).  Integer atomics only.  LDS
// (at most 2^kLookupLdsLog counters): every block keeps a private histogram and flushes its nonzero counters with one global
// add each, as lookup_count_kernel does; else the adds go to global memory.  lookup_mont_kernel<F> (kernels/fraction.hpp,
// unchanged) turns the counts into Montgomery words.
//
// THE TRIPLE PRODUCT has no kernel of its own: gp_pass_kernel<F, FOLD> forms e l r over three arbitrary tables, so the sumcheck of
// step 2 runs on it with E := val (engine/abi_spark.inc, sc_product3_prove; SC_KIND_PRODUCT_PASS records).
//
// BYTE MODEL of the launch records (include/sumcheck_hip.h, kinds 33 .. 35).  SC_KIND_SPARK_INDEX: kf = 0 the index launch of one
// dimension (ks = 1 with LDS histograms; log_in = l; reads 4 * 2^l, writes 8 * 2^l + 4 * 2^m for 2^m counters), kf = 1 the
// conversion of its counts (log_in = m; reads 4 * 2^m, writes 8 * 2^m).  SC_KIND_SPARK_GATHER: log_in = l; reads 8 * 2^l of
// indices plus the gathered 16 * 2^l, writes 16 * 2^l.  SC_KIND_SPARK_TUPLE: kf = 1 with IOTA, log_in = n for 2^n entries;
// reads 8 * 2^n (12 * 2^n with a key stream), writes 8 * 2^n.
#pragma once
#include <stddef.h>

#include "../field.hpp"
#include "fraction.hpp"   // kLookupLdsLog

namespace sc {

constexpr int kSparkMaxLog = 28;   // l, a and b at most

// ---- the work per element ------------------------------------------------------------------------------------------------

// l = max(1, ceil(log2 nnz)), nnz >= 1
inline int spark_log_len(size_t nnz) {
  int l = 1;
  while (((size_t)1 << l) < nnz) ++l;
  return l;
}

// The first triple outside 2^a x 2^b or with a value that is not a word below p; nnz when there is none
inline size_t spark_first_bad(const u32* row, const u32* col, const u64* val, size_t nnz, int a, int b, u64 p) {
  const u64 n_rows = (u64)1 << a, n_cols = (u64)1 << b;
  for (size_t k = 0; k < nnz; ++k)
    if (row[k] >= n_rows || col[k] >= n_cols || val[k] >= p) return k;
  return nnz;
}

// The list padded with (0, 0, 0) to n entries, n >= nnz
inline void spark_pad(const u32* row, const u32* col, const u64* val, size_t nnz, size_t n, u32* prow, u32* pcol, u64* pval) {
  for (size_t k = 0; k < n; ++k) {
    prow[k] = k < nnz ? row[k] : 0;
    pcol[k] = k < nnz ? col[k] : 0;
    pval[k] = k < nnz ? val[k] : 0;
  }
}

// The Montgomery word of an index or a count (below p: the callers refuse p <= 2^max(l, a, b))
template <class F>
SC_HD u64 spark_key_word(const F& f, u32 key) {
  return f.to_mont((u64)key);
}

// S entries of the gather: out[s] = table[idx[s]]
template <int S>
SC_HD void spark_gather_item(const u64* __restrict__ table, const u32 (&idx)[S], u64 (&out)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) out[s] = table[idx[s]];
}

// One tuple: alpha - key - beta v, key an integer below p
template <class F>
SC_HD u64 spark_tuple_item(const F& f, u64 alpha, u64 beta, u32 key, u64 v) {
  return f.sub(f.sub(alpha, spark_key_word(f, key)), f.mul(beta, v));
}

#if defined(__HIPCC__)

// er[k] = U[row[k]], ec[k] = W[col[k]], k < n; n = 2 or a multiple of four
template <class F>
__global__ void __launch_bounds__(kBlock) spark_gather_kernel(const u32* __restrict__ row, const u32* __restrict__ col, const u64* __restrict__ U,
                                                              const u64* __restrict__ W, size_t n, u64* __restrict__ er, u64* __restrict__ ec) {
  const size_t n_units = n / 4;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    const uint4 rr = reinterpret_cast<const uint4*>(row)[i];
    const uint4 cc = reinterpret_cast<const uint4*>(col)[i];
    const u32 ri[4] = {rr.x, rr.y, rr.z, rr.w}, ci[4] = {cc.x, cc.y, cc.z, cc.w};
    u64 u[4], w[4];
    spark_gather_item<4>(U, ri, u);
    spark_gather_item<4>(W, ci, w);
    ull2* const eo = reinterpret_cast<ull2*>(er) + 2 * i;
    ull2* const co = reinterpret_cast<ull2*>(ec) + 2 * i;
    eo[0] = ull2{u[0], u[1]};
    eo[1] = ull2{u[2], u[3]};
    co[0] = ull2{w[0], w[1]};
    co[1] = ull2{w[2], w[3]};
  }
  if (n == 2 && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint2 rr = *reinterpret_cast<const uint2*>(row);
    const uint2 cc = *reinterpret_cast<const uint2*>(col);
    const u32 ri[2] = {rr.x, rr.y}, ci[2] = {cc.x, cc.y};
    u64 u[2], w[2];
    spark_gather_item<2>(U, ri, u);
    spark_gather_item<2>(W, ci, w);
    *reinterpret_cast<ull2*>(er) = ull2{u[0], u[1]};
    *reinterpret_cast<ull2*>(ec) = ull2{w[0], w[1]};
  }
}

// out[i] = alpha - key_i - beta v[i], i < n; key_i = key[i], or with IOTA i itself (key is not read).  n = 2 or a multiple of four
template <class F, bool IOTA>
__global__ void __launch_bounds__(kBlock) spark_tuple_kernel(F f, const u32* __restrict__ key, const u64* __restrict__ v, u64 alpha, u64 beta, size_t n,
                                                             u64* __restrict__ out) {
  const size_t n_units = n / 4;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u32 k[4];
    if constexpr (IOTA) {
#pragma unroll
      for (int s = 0; s < 4; ++s) k[s] = (u32)(4 * i) + (u32)s;
    } else {
      const uint4 kk = reinterpret_cast<const uint4*>(key)[i];
      k[0] = kk.x; k[1] = kk.y; k[2] = kk.z; k[3] = kk.w;
    }
    const ull2* const src = reinterpret_cast<const ull2*>(v) + 2 * i;
    const ull2 lo = src[0], hi = src[1];
    ull2* const dst = reinterpret_cast<ull2*>(out) + 2 * i;
    dst[0] = ull2{spark_tuple_item(f, alpha, beta, k[0], lo.x), spark_tuple_item(f, alpha, beta, k[1], lo.y)};
    dst[1] = ull2{spark_tuple_item(f, alpha, beta, k[2], hi.x), spark_tuple_item(f, alpha, beta, k[3], hi.y)};
  }
  if (n == 2 && blockIdx.x == 0 && threadIdx.x == 0) {
    u32 k[2] = {0, 1};
    if constexpr (!IOTA) {
      const uint2 kk = *reinterpret_cast<const uint2*>(key);
      k[0] = kk.x; k[1] = kk.y;
    }
    const ull2 x = *reinterpret_cast<const ull2*>(v);
    *reinterpret_cast<ull2*>(out) = ull2{spark_tuple_item(f, alpha, beta, k[0], x.x), spark_tuple_item(f, alpha, beta, k[1], x.y)};
  }
}

// The counts of one thread's four indices, with the runs of one index merged: the padding and a dense column are long runs of
// one index, and 2^24 adds that meet on one counter of global memory take a third of a second.  A wave whose active lanes all
// hold four copies of one index adds once, from its first active lane; a thread whose four are equal adds four at once.
// Every index is below m_len (a counter outside the histogram is never touched).
__device__ __forceinline__ void spark_count4(u32* __restrict__ counters, const u32 (&jv)[4], u32 m_len) {
  const bool four = jv[0] == jv[1] && jv[1] == jv[2] && jv[2] == jv[3];
  const unsigned long long active = __ballot(1);
  const int first = __ffsll((long long)active) - 1;
  const u32 lead = (u32)__shfl((int)jv[0], first);
  if (__ballot(four && jv[0] == lead) == active) {
    if ((int)__lane_id() == first && lead < m_len) atomicAdd(&counters[lead], 4u * (u32)__popcll(active));
    return;
  }
  if (four) {
    if (jv[0] < m_len) atomicAdd(&counters[jv[0]], 4u);
    return;
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (jv[s] < m_len) atomicAdd(&counters[jv[s]], 1u);
}

// One dimension of the preprocessing: words[k] = the Montgomery word of idx[k] and counts[idx[k]] += 1, k < n; n = 2 or a multiple of
// four; every idx[k] < 2^log_m (validated by the caller); counts: 2^log_m u32 counters, zeroed by the caller.  LDS: log_m <= kLookupLdsLog
template <class F, bool LDS>
__global__ void __launch_bounds__(kBlock) spark_index_kernel(F f, const u32* __restrict__ idx, size_t n, int log_m, u64* __restrict__ words,
                                                             u32* __restrict__ counts) {
  __shared__ u32 hist[LDS ? (1 << kLookupLdsLog) : 1];
  const u32 m_len = (u32)1 << log_m;
  if constexpr (LDS) {
    for (u32 j = threadIdx.x; j < m_len; j += kBlock) hist[j] = 0;
    __syncthreads();
  }
  const size_t n_units = n / 4;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    const uint4 jj = reinterpret_cast<const uint4*>(idx)[i];
    const u32 jv[4] = {jj.x, jj.y, jj.z, jj.w};
    ull2* const dst = reinterpret_cast<ull2*>(words) + 2 * i;
    dst[0] = ull2{spark_key_word(f, jv[0]), spark_key_word(f, jv[1])};
    dst[1] = ull2{spark_key_word(f, jv[2]), spark_key_word(f, jv[3])};
    spark_count4(LDS ? hist : counts, jv, m_len);
  }
  if (n == 2 && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint2 jj = *reinterpret_cast<const uint2*>(idx);
    const u32 jv[2] = {jj.x, jj.y};
    *reinterpret_cast<ull2*>(words) = ull2{spark_key_word(f, jv[0]), spark_key_word(f, jv[1])};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (jv[s] < m_len) {
        if constexpr (LDS) atomicAdd(&hist[jv[s]], 1u);
        else atomicAdd(&counts[jv[s]], 1u);
      }
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (u32 j = threadIdx.x; j < m_len; j += kBlock) {
      const u32 c = hist[j];
      if (c) atomicAdd(&counts[j], c);
    }
  }
}

#endif   // __HIPCC__

}  // namespace sc
