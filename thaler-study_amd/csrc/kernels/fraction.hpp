// Part of kernels.hpp (included there, in order, after grand_product.hpp): LogUp lookups - the fraction-sum tree of two tables,
// the five-table cubic sumcheck pass of one tree layer (three tables where the numerator is all ones), the multiplicity
// histogram of a lookup, and the host code that finishes the small layers and the tails of the large ones.  The host parts
// (SC_HD and plain inline functions) compile without hipcc: tests/cpp/fr_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract; Haboeck, "Multivariate lookups based on logarithmic derivatives"; Papini and Haboeck, "Improving
// logarithmic derivative lookups using GKR": the fractional sumcheck)
//
//   All tables are LE tables of Montgomery words, variable 0 first, as everywhere in the ABI.
//
//   Fraction sum.  The inputs are p and q, 2^n entries each, 1 <= n <= 28; layer n is (p, q).  For k = n-1 .. 0 and x < 2^k
//     p_k[x] = p_(k+1)[x] q_(k+1)[x + 2^k] + p_(k+1)[x + 2^k] q_(k+1)[x]        q_k[x] = q_(k+1)[x] q_(k+1)[x + 2^k]:
//   the tree splits by halves, as the product tree does, so PL_k, PR_k, QL_k, QR_k - the two halves of p_(k+1) and of q_(k+1) -
//   are contiguous tables of k variables and nothing is deinterleaved.  The root (P, Q) = (p_0[0], q_0[0]) satisfies
//   P / Q = sum_i p_i / q_i whenever no q_i is 0.
//
//   Layer k = 0 .. n-1 turns the claims p_k~(z_k) = a_k and q_k~(z_k) = b_k into claims about layer k+1; z_0 = (),
//   (a_0, b_0) = (P, Q).
//    - Rounds, k >= 1.  V draws lambda_k.  A sumcheck of k rounds over
//        sum_{x in {0,1}^k} eq(z_k, x) (PL QR + PR QL + lambda_k QL QR)(x) = a_k + lambda_k b_k,
//      variable 0 first.  Before round j the tables have 2^(k-j) entries; with u_i(t) = u[2i] + t (u[2i+1] - u[2i]) the message is
//      H_j(t) = sum_i e_i(t) (pl_i(t) qr_i(t) + pr_i(t) ql_i(t) + lambda_k ql_i(t) qr_i(t)) at t = 0, 1, 2, 3.  V checks
//      H_j(0) + H_j(1) against the running claim and draws r_j; the new claim is the cubic through the four values at r_j; all five
//      tables fold by r_j (kernels/grand_product.hpp: the same checks, interpolation and folds).
//    - Finals.  P sends pl, pr, ql, qr, the four tables' extensions at r.  V checks
//      eq(z_k, r) (pl qr + pr ql + lambda_k ql qr) against the running claim.  At k = 0 there are no rounds and no lambda: V
//      checks pl qr + pr ql = P and ql qr = Q.
//    - Combining step.  V draws rho_k; a_(k+1) = pl + rho_k (pr - pl), b_(k+1) = ql + rho_k (qr - ql), z_(k+1) = (r, rho_k).
//   After layer n-1 the claims p~(z_n) = a_n and q~(z_n) = b_n are the caller's.
//
//   All-ones numerator.  p == NULL means p = 1 everywhere, the witness side of every lookup.  The constant table folds to
//   itself, so for the whole of layer n-1 PL = PR = 1: the pass reads E, QL, QR only and forms e (ql + qr + lambda ql qr), the
//   finals are pl = pr = 1, and the verifier checks a_n = 1.  The top launch of the tree reads one table instead of two.
//
//   Lookup.  The witness w (2^n entries, committed), the public table t (2^m entries) and idx with w_i = t[idx_i].
//    1. P computes mult_j = #{i : idx_i = j} and commits to it, before alpha exists.       2. V draws alpha.
//    3. P proves the fraction sums of (1, alpha - w) and (mult, alpha - t).
//    4. V refuses unless Q_w != 0, Q_t != 0 and P_w Q_t = P_t Q_w.
//    5. On the w side V checks a_n = 1 and b_n = alpha - w~(z) from one opening of w's commitment.
//    6. On the t side V checks a'_m = mult~(z') from one opening of mult's commitment,
//    7. and b'_m = alpha - t~(z'), which V computes from the public table; for the range table t_j = j,
//       t~(z') = sum_j 2^j z'_j.
//   Counts are field words, so the lookup layer (not the fraction sum) refuses p <= 2^max(n, m); the fraction sum refuses
//   p <= 3 only (interpolation on {0, 1, 2, 3}).  Nothing beyond the papers' statements is claimed: no security level, no zero
//   knowledge, no Fiat-Shamir.
//
// THE TREES are two pool blocks in heap layout: layer k of p (of q) occupies words [2^k, 2^(k+1)) of its block, k = 0 .. n-1
// (word 0 is unused); layer n is the caller's p and q, borrowed and never written.
//   fr_tree_kernel<F, LV, ONES>, LV = 1, 2, 3: one launch reads layer m of both tables once (ONES: of q alone, m = n) and writes
//   layers m-1 .. m-LV of both.  A thread owns two adjacent indices x, x+1 of layer m-LV: 2^LV 16-byte loads per table at a
//   distance of 2^(m-LV) words, each lane-contiguous across the wave, three products per node (fr_tree_item: the numerator's two
//   in the lazy accumulator, reduced once), and every intermediate layer stored with 16-byte lane-contiguous stores.  No LDS, no
//   atomics.  m - LV >= 1.  It holds twice the words of gp_tree_kernel per level; LV = 3 still compiles without scratch.
//   fr_tree_tail_kernel<F, ONES>: one block takes a layer of at most 2^kFrTailLog entries of both tables (32 KiB of LDS) down to
//   the root through LDS, one barrier per level, and stores every layer.
//   Schedule: from layer n, LV = min(option fr_tree_lv, layers left above kFrTailLog), then the tail kernel.
//
// THE CUBIC PASS  fr_pass_kernel<F, FOLD, ONES>: one launch per round over E, QL, QR, PL, PR (ONES: E, QL, QR).  The unit of work
// is gp_pass_kernel's: with FOLD a thread reads four consecutive entries of each table (two 16-byte loads), folds them by the
// previous challenge (zc_fold4), stores the two folded entries and adds the four values of its pair into four lazy accumulators
// (fr_accumulate / fr_accumulate_ones); round 0 reads pairs and stores nothing.  The sums leave through reduce_cells<F, 4> /
// finish_pass<F, 4>.  Inputs are never written: the first launch of a layer reads its tables straight from the trees.
//
// THE COUNT  lookup_count_kernel<LDS>: a thread takes two adjacent i; idx[i] < 2^m and w[i] == t[idx[i]] are checked, a failure
// adds one to the mismatch counter and is not counted, otherwise one is added to the u32 counter of idx[i].  Integer atomics only.
// LDS (2^m counters fit in 32 KiB, m <= kLookupLdsLog): every block keeps a private histogram in LDS and flushes its nonzero
// counters with one global add each; else the adds go to global memory.  lookup_mont_kernel<F> turns counts into Montgomery words.
//
// THE HOST FINISH  fr_host_rounds: the rounds of a layer over host copies of the tables with the same fold and accumulate; the
// engine runs the layers of at most 2^fr_host_log entries there entirely, and the tail of every larger layer from the tables its
// last launch wrote.
//
// BYTE MODEL of the launch records (include/sumcheck_hip.h, kinds 30 .. 32).  SC_KIND_FRACTION_TREE from layer m: kf = LV (0: the
// tail), ks = tables read (1 with ONES at m = n, else 2); 8 ks 2^m bytes read, 2 * 8 (2^m - 2^(m-LV)) written (the tail:
// 2 * 8 (2^m - 1)).  SC_KIND_FRACTION_PASS: kf = 1 if it folded, ks = tables (3 or 5), log_in = log2 of the tables read;
// 8 ks 2^log_in read, 8 ks 2^(log_in - 1) written with kf = 1.  SC_KIND_LOOKUP_COUNT: kf = 0 the count (ks = 1 with LDS
// histograms; log_in = n; reads 12 * 2^n bytes - w, idx - plus the gathered 8 * 2^n of t, writes 4 * 2^m), kf = 1 the
// conversion (log_in = m; reads 4 * 2^m, writes 8 * 2^m).
#pragma once
#include <vector>

#include "../field.hpp"
#include "grand_product.hpp"   // gp_host_fold, gp_host_eq
#include "r1cs.hpp"            // zc_fold4

namespace sc {

constexpr int kFrMaxLog = 28;      // n at most
constexpr int kFrTailLog = 11;     // the tail kernel takes layers of at most 2^this entries: two tables in 32 KiB of LDS
constexpr int kFrTreeLvMax = 3;    // layers per launch at most (no scratch, no spills: DESIGN.md section 9 item 17)
constexpr int kFrTreeLv = 3;       // layers per launch above the tail, the default of option "fr_tree_lv"
constexpr int kFrHostLogMax = 12;  // option "fr_host_log" at most
constexpr int kLookupLdsLog = 13;  // 2^this u32 counters are 32 KiB of LDS

// One index x of layer m - LV of both tables: pin[j], qin[j] = layer m at x + j 2^(m-LV), j < 2^LV (ONES: pin is not read, it is
// all ones).  pout, qout are the little heaps above x as in gp_tree_item: [h + j], j < h, is layer m-d at x + j 2^(m-LV) for
// h = 2^(LV-d), d = 1 .. LV ([0] is not written); [1] is layer m-LV at x.
template <class F, int LV, bool ONES = false>
SC_HD void fr_tree_item(const F& f, const u64 (&pin)[1 << LV], const u64 (&qin)[1 << LV], u64 (&pout)[1 << LV], u64 (&qout)[1 << LV]) {
  constexpr int H = 1 << (LV - 1);
#pragma unroll
  for (int j = 0; j < H; ++j) {
    if constexpr (ONES) {
      pout[H + j] = f.add(qin[j + H], qin[j]);
    } else {
      typename F::Acc a;
      f.acc_zero(a);
      f.acc_mac(a, pin[j], qin[j + H]);
      f.acc_mac(a, pin[j + H], qin[j]);
      pout[H + j] = f.acc_get(a);
    }
    qout[H + j] = f.mul(qin[j], qin[j + H]);
  }
#pragma unroll
  for (int h = H / 2; h >= 1; h /= 2) {
#pragma unroll
    for (int j = 0; j < h; ++j) {
      typename F::Acc a;
      f.acc_zero(a);
      f.acc_mac(a, pout[2 * h + j], qout[3 * h + j]);
      f.acc_mac(a, pout[3 * h + j], qout[2 * h + j]);
      pout[h + j] = f.acc_get(a);
      qout[h + j] = f.mul(qout[2 * h + j], qout[3 * h + j]);
    }
  }
}

// One item of the cubic pass: the pairs of one index i -> H(t) += e(t) (pl(t) qr(t) + ql(t) (pr(t) + lambda qr(t))), t = 0 .. 3.
// lambda qr(t) is linear in t: it is stepped by its difference like the other terms.
template <class F>
SC_HD void fr_accumulate(const F& f, typename F::Acc (&acc)[4], u64 lambda, const u64 (&e)[2], const u64 (&pl)[2], const u64 (&pr)[2],
                         const u64 (&ql)[2], const u64 (&qr)[2]) {
  const u64 m0 = f.mul(lambda, qr[0]), m1 = f.mul(lambda, qr[1]);
  const u64 s0 = f.add(pr[0], m0), s1 = f.add(pr[1], m1);   // s(t) = pr(t) + lambda qr(t)
  const u64 de = f.sub(e[1], e[0]), dpl = f.sub(pl[1], pl[0]), dql = f.sub(ql[1], ql[0]), dqr = f.sub(qr[1], qr[0]), ds = f.sub(s1, s0);
  u64 et = e[0], plt = pl[0], qlt = ql[0], qrt = qr[0], st = s0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      et = e[1]; plt = pl[1]; qlt = ql[1]; qrt = qr[1]; st = s1;
    } else if (t > 1) {
      et = f.add(et, de); plt = f.add(plt, dpl); qlt = f.add(qlt, dql); qrt = f.add(qrt, dqr); st = f.add(st, ds);
    }
    typename F::Acc a;
    f.acc_zero(a);
    f.acc_mac(a, plt, qrt);
    f.acc_mac(a, qlt, st);
    f.acc_mac(acc[t], et, f.acc_get(a));
  }
}

// The same with pl = pr = 1: H(t) += e(t) (ql(t) + qr(t) + lambda ql(t) qr(t)) = e(t) (qr(t) + ql(t) (1 + lambda qr(t)))
template <class F>
SC_HD void fr_accumulate_ones(const F& f, typename F::Acc (&acc)[4], u64 lambda, const u64 (&e)[2], const u64 (&ql)[2], const u64 (&qr)[2]) {
  const u64 s0 = f.add(f.one(), f.mul(lambda, qr[0])), s1 = f.add(f.one(), f.mul(lambda, qr[1]));   // s(t) = 1 + lambda qr(t)
  const u64 de = f.sub(e[1], e[0]), dql = f.sub(ql[1], ql[0]), dqr = f.sub(qr[1], qr[0]), ds = f.sub(s1, s0);
  u64 et = e[0], qlt = ql[0], qrt = qr[0], st = s0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      et = e[1]; qlt = ql[1]; qrt = qr[1]; st = s1;
    } else if (t > 1) {
      et = f.add(et, de); qlt = f.add(qlt, dql); qrt = f.add(qrt, dqr); st = f.add(st, ds);
    }
    f.acc_mac(acc[t], et, f.add(qrt, f.mul(qlt, st)));
  }
}

// ---- the host finish ---------------------------------------------------------------------------------------------------

// The order of the tables everywhere below and in the pass kernel: with ONES the first three alone
enum { kFrE = 0, kFrQL = 1, kFrQR = 2, kFrPL = 3, kFrPR = 4 };

// H(0..3) of a round over host tables tb[0 .. n_tables) of 2 n_units entries; n_tables = 5, or 3 (pl = pr = 1)
template <class F>
inline void fr_host_sums(const F& f, u64* const* tb, int n_tables, u64 lambda, size_t n_units, u64 (&out)[4]) {
  typename F::Acc acc[4];
  for (int t = 0; t < 4; ++t) f.acc_zero(acc[t]);
  for (size_t i = 0; i < n_units; ++i) {
    u64 u[5][2];
    for (int k = 0; k < n_tables; ++k) {
      u[k][0] = tb[k][2 * i];
      u[k][1] = tb[k][2 * i + 1];
    }
    if (n_tables == 3) fr_accumulate_ones(f, acc, lambda, u[kFrE], u[kFrQL], u[kFrQR]);
    else fr_accumulate(f, acc, lambda, u[kFrE], u[kFrPL], u[kFrPR], u[kFrQL], u[kFrQR]);
  }
  for (int t = 0; t < 4; ++t) out[t] = f.acc_get(acc[t]);
}

// The rounds first .. first + log_len - 1 of a layer over host tables tb[0 .. n_tables) of 2^log_len entries each (folded in
// place; on return tb[k][0], k >= 1, are the finals).  `given`: H(0..3) of round `first`, when the device has already formed
// it, else null.  next(round, msg, &c) receives a round's four values and returns false to end the call - or sets the challenge
// c.  challenges[first ..] receive what next() drew.  Returns false when next() did.
template <class F, class Next>
inline bool fr_host_rounds(const F& f, u64* const* tb, int n_tables, u64 lambda, int log_len, size_t first, const u64* given, u64* challenges,
                           Next&& next) {
  for (int j = 0; j < log_len; ++j) {
    const size_t n_units = (size_t)1 << (log_len - j - 1);
    u64 msg[4];
    if (j == 0 && given) {
      for (int t = 0; t < 4; ++t) msg[t] = given[t];
    } else {
      fr_host_sums(f, tb, n_tables, lambda, n_units, msg);
    }
    u64 c = 0;
    if (!next(first + (size_t)j, msg, &c)) return false;
    challenges[first + (size_t)j] = c;
    for (int k = 1; k < n_tables; ++k) gp_host_fold(f, c, tb[k], n_units);
    if (n_units > 1) gp_host_fold(f, c, tb[kFrE], n_units);   // (nobody reads the last E)
  }
  return true;
}

#if defined(__HIPCC__)

// Layers m-1 .. m-LV of both tables from layer m = (psrc, qsrc) (2^m words each; ONES: psrc is not read); ptree, qtree: the heaps
// (layer k at word 2^k).  n_units = 2^(m-LV-1) threads' worth of work: unit i owns the indices 2i, 2i+1 of layer m - LV.
// log_low = m - LV >= 1.
template <class F, int LV, bool ONES>
__global__ void __launch_bounds__(kBlock) fr_tree_kernel(F f, const u64* __restrict__ psrc, const u64* __restrict__ qsrc, u64* __restrict__ ptree,
                                                         u64* __restrict__ qtree, int log_low, size_t n_units) {
  constexpr int W = 1 << LV;
  const size_t dist = (size_t)1 << log_low;   // words between a unit's loads
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 pa[W], pb[W], qa[W], qb[W], opa[W], opb[W], oqa[W], oqb[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const ull2 y = *reinterpret_cast<const ull2*>(qsrc + (size_t)j * dist + 2 * i);
      qa[j] = y.x;
      qb[j] = y.y;
      if constexpr (!ONES) {
        const ull2 x = *reinterpret_cast<const ull2*>(psrc + (size_t)j * dist + 2 * i);
        pa[j] = x.x;
        pb[j] = x.y;
      } else {
        pa[j] = pb[j] = 0;   // (not read)
      }
    }
    fr_tree_item<F, LV, ONES>(f, pa, qa, opa, oqa);
    fr_tree_item<F, LV, ONES>(f, pb, qb, opb, oqb);
#pragma unroll
    for (int h = W / 2; h >= 1; h /= 2) {
      // layer log_low + log2 h: 2^log_low h words at word 2^log_low h of each heap
      u64* const pl = ptree + (size_t)h * dist;
      u64* const ql = qtree + (size_t)h * dist;
#pragma unroll
      for (int j = 0; j < h; ++j) {
        *reinterpret_cast<ull2*>(pl + (size_t)j * dist + 2 * i) = ull2{opa[h + j], opb[h + j]};
        *reinterpret_cast<ull2*>(ql + (size_t)j * dist + 2 * i) = ull2{oqa[h + j], oqb[h + j]};
      }
    }
  }
}

// Layers m-1 .. 0 of both tables from layer m (2^m words each, 1 <= m <= kFrTailLog; ONES: psrc is all ones and not read): one block
template <class F, bool ONES>
__global__ void __launch_bounds__(kBlock) fr_tree_tail_kernel(F f, const u64* __restrict__ psrc, const u64* __restrict__ qsrc, u64* __restrict__ ptree,
                                                              u64* __restrict__ qtree, int m) {
  __shared__ u64 vp[1 << kFrTailLog];
  __shared__ u64 vq[1 << kFrTailLog];
  const int n = 1 << m;
  for (int x = threadIdx.x; x < n; x += kBlock) {
    vp[x] = ONES ? f.one() : psrc[x];
    vq[x] = qsrc[x];
  }
  __syncthreads();
  for (int k = m - 1; k >= 0; --k) {
    const int half = 1 << k;
    // thread x reads [x] and [x + half] of both tables and writes [x]: nobody else touches either this level
    for (int x = threadIdx.x; x < half; x += kBlock) {
      const u64 pin[2] = {vp[x], vp[x + half]}, qin[2] = {vq[x], vq[x + half]};
      u64 po[2], qo[2];
      fr_tree_item<F, 1>(f, pin, qin, po, qo);
      vp[x] = po[1];
      vq[x] = qo[1];
      ptree[half + x] = po[1];
      qtree[half + x] = qo[1];
    }
    __syncthreads();
  }
}

// One round of the cubic sumcheck over tables in the order kFrE .. kFrPR (ONES: the first three).  FOLD: the tables have
// 4 n_units entries; unit i folds entries 4i .. 4i+3 of each by r into entries 2i, 2i+1 of out[.] and adds them to H(0..3).
// Otherwise: 2 n_units entries, nothing stored.
struct FrTables {
  const u64* in[5];
  u64* out[5];
};
template <class F, bool FOLD, bool ONES>
__global__ void __launch_bounds__(kBlock) fr_pass_kernel(F f, FrTables tb, u64 r, u64 lambda, size_t n_units, PassOut out) {
  constexpr int NT = ONES ? 3 : 5;
  __shared__ u64 lds[(kBlock / kWave) * 4];
  __shared__ int lds_flag;
  typename F::Acc acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) f.acc_zero(acc[s]);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 p[NT][2];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      if constexpr (FOLD) {
        const ull2* src = reinterpret_cast<const ull2*>(tb.in[k]) + 2 * i;
        const ull2 lo = src[0], hi = src[1];
        const u64 u[4] = {lo.x, lo.y, hi.x, hi.y};
        zc_fold4(f, r, u, p[k]);
        reinterpret_cast<ull2*>(tb.out[k])[i] = ull2{p[k][0], p[k][1]};
      } else {
        const ull2 x = reinterpret_cast<const ull2*>(tb.in[k])[i];
        p[k][0] = x.x;
        p[k][1] = x.y;
      }
    }
    if constexpr (ONES) fr_accumulate_ones(f, acc, lambda, p[kFrE], p[kFrQL], p[kFrQR]);
    else fr_accumulate(f, acc, lambda, p[kFrE], p[kFrPL], p[kFrPR], p[kFrQL], p[kFrQR]);
  }
  const u64 mine = reduce_cells<F, 4>(f, acc, lds);
  finish_pass<F, 4>(f, out, mine, &lds_flag);
}

// The multiplicities of a lookup: n_pairs pairs of (w[i], idx[i]); counts: 2^log_m u32 counters and *mismatches, zeroed by the
// caller.  LDS: log_m <= kLookupLdsLog.  The words of w and t are compared as they are (Montgomery words below p are unique).
template <bool LDS>
__global__ void __launch_bounds__(kBlock) lookup_count_kernel(const u64* __restrict__ w, const u64* __restrict__ t, const u32* __restrict__ idx,
                                                              size_t n_pairs, int log_m, u32* __restrict__ counts, u32* __restrict__ mismatches) {
  __shared__ u32 hist[LDS ? (1 << kLookupLdsLog) : 1];
  const u32 m_len = (u32)1 << log_m;
  if constexpr (LDS) {
    for (u32 j = threadIdx.x; j < m_len; j += kBlock) hist[j] = 0;
    __syncthreads();
  }
  u32 bad = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_pairs; i += (size_t)gridDim.x * kBlock) {
    const ull2 ww = reinterpret_cast<const ull2*>(w)[i];
    const uint2 jj = reinterpret_cast<const uint2*>(idx)[i];
    const u64 wv[2] = {ww.x, ww.y};
    const u32 jv[2] = {jj.x, jj.y};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (jv[s] < m_len && t[jv[s]] == wv[s]) {   // (t is read only at an index inside it)
        if constexpr (LDS) atomicAdd(&hist[jv[s]], 1u);
        else atomicAdd(&counts[jv[s]], 1u);
      } else {
        bad += 1;
      }
    }
  }
  if (bad) atomicAdd(mismatches, bad);
  if constexpr (LDS) {
    __syncthreads();
    for (u32 j = threadIdx.x; j < m_len; j += kBlock) {
      const u32 c = hist[j];
      if (c) atomicAdd(&counts[j], c);
    }
  }
}

// out[j] = the Montgomery word of counts[j], j < n (counts are below p: the caller refuses p <= 2^max(n, m))
template <class F>
__global__ void __launch_bounds__(kBlock) lookup_mont_kernel(F f, const u32* __restrict__ counts, size_t n, u64* __restrict__ out) {
  for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (size_t)gridDim.x * kBlock) out[j] = f.to_mont((u64)counts[j]);
}

#endif   // __HIPCC__

}  // namespace sc
