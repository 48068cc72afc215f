// Part of kernels.hpp (included there, in order, after ext_grand_product.hpp): the fraction sums of fraction.hpp (LogUp) with
// every element in the quadratic extension K = F_p[X] / (X^2 - w) of ext_sumprod.hpp - the fraction-sum trees over K, the
// five-table cubic sumcheck pass of one tree layer over extension tables (three tables where the numerator is all ones), and the
// host code that finishes the small layers and the tails of the large ones.  The eq table of a point of K^k is
// ext_grand_product.hpp's.  The work per element is in SC_HD and plain inline functions, which compile without hipcc:
// tests/cpp/ext_fr_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract: that of fraction.hpp word for word, every element in K)
//
//   An element of K is two Montgomery words (c0, c1), meaning c0 + c1 X; it crosses the ABI as two consecutive words.
//
//   Leaves.  They are NEVER STORED.  The denominator is q_i = beta + alpha t[i] for a base-field table t of 2^n entries,
//   1 <= n <= 28, and alpha, beta in K, alpha != 0 (ext_gp_leaf, formed in registers wherever layer n is read).  The numerator p is
//   a base-field table embedded as (p_i, 0), or NULL: all ones.  Both sides of a lookup have this form: (1, alpha_c - w_i) is p
//   NULL, alpha = (-1, 0), beta = alpha_c; (mult_j, alpha_c - t_j) is p = mult with the same alpha and beta.
//
//   Tree.  For k = n-1 .. 0 and x < 2^k
//     p_k[x] = p_(k+1)[x] q_(k+1)[x + 2^k] + p_(k+1)[x + 2^k] q_(k+1)[x]        q_k[x] = q_(k+1)[x] q_(k+1)[x + 2^k]
//   in K; the root is (P, Q) in K^2.  At layer n-1 the numerator's products are base x K, two base multiplications each; with all
//   ones p_(n-1)[x] = q[x] + q[x + 2^(n-1)].  PL_k, PR_k, QL_k, QR_k are the halves of p_(k+1) and q_(k+1).
//
//   Layer k = 0 .. n-1 turns the claims p_k~(z_k) = a_k, q_k~(z_k) = b_k, z_k in K^k, into claims about layer k+1; z_0 = (),
//   (a_0, b_0) = (P, Q).
//    - Rounds, k >= 1.  V draws lambda_k in K.  A sumcheck of k rounds over
//        sum_{x in {0,1}^k} eq(z_k, x) (PL QR + PR QL + lambda_k QL QR)(x) = a_k + lambda_k b_k,
//      variable 0 first.  Before round j the tables have 2^(k-j) entries of K; with u_i(t) = u[2i] + t (u[2i+1] - u[2i]) the message
//      is H_j(t) = sum_i e_i(t) (pl_i(t) qr_i(t) + pr_i(t) ql_i(t) + lambda_k ql_i(t) qr_i(t)) in K at t = 0, 1, 2, 3: eight words
//      H(0).c0, H(0).c1, .., H(3).c0, H(3).c1.  V checks H_j(0) + H_j(1) against the running claim and draws r_j in K; the new claim
//      is the cubic through the four values at r_j; all five tables fold by r_j.
//    - Finals.  P sends pl, pr, ql, qr in K, eight words.  V checks eq(z_k, r) (pl qr + pr ql + lambda_k ql qr) against the running
//      claim.  At k = 0 there are no rounds and no lambda: V checks pl qr + pr ql = P and ql qr = Q.
//    - Combining step.  V draws rho_k in K; a_(k+1) = pl + rho_k (pr - pl), b_(k+1) = ql + rho_k (qr - ql), z_(k+1) = (r, rho_k).
//   After layer n-1 the caller's claims are p~(z_n) = a_n (a_n = 1 for all ones) and t~(z_n) = (b_n - beta) alpha^-1 at z_n in K^n:
//   each is checked with sc_table_evaluate_ext or with an opening of a commitment at the extension point.
//
//   Fields with p <= 3 are refused, w must be a quadratic non-residue (the engine checks both on the host).  Tuple denominators
//   (SPARK) need extension-valued leaves and are not covered.  Nothing beyond the papers' statements is claimed: no zero knowledge,
//   no Fiat-Shamir.
//
// THE LAYOUT  An extension table of 2^m entries is two planes of 2^m words, all c0 words then all c1 words, as in ext_sumprod.hpp.
// THE TREE is one pool block of four heaps of 2^n words each, in the order p.c0, p.c1, q.c0, q.c1: layer k of heap h occupies words
// h 2^n + [2^k, 2^(k+1)), k < n.  Every load and store keeps the shape of fr_tree_kernel and fr_pass_kernel: a lane reads and writes
// 16 contiguous bytes, a wave 1 KiB.
//   ext_fr_tree_kernel<F, LV, LEAF_IN, ONES>, LV = 1, 2, 3: the schedule and access pattern of fr_tree_kernel, per plane.  With
//   LEAF_IN (the first launch) it reads the base words of t, and of p unless ONES, and forms the leaves; otherwise it reads the four
//   planes of layer m.  It stores all four planes of the layers m-1 .. m-LV.  ONES only with LEAF_IN.
//   ext_fr_tree_tail_kernel<F, LEAF_IN, ONES>: one block takes a layer of at most 2^kExtFrTailLog entries down to the root through
//   LDS (four planes: 32 KiB), one barrier per level, and stores every layer.  LEAF_IN where n <= kExtFrTailLog.
//   Schedule: from layer n, LV = min(fr_tree_lv, layers left above kExtFrTailLog), then the tail kernel.
//
// THE CUBIC PASS  ext_fr_pass_kernel<F, FOLD, LEAF_IN, ONES>: one launch per round over E, QL, QR, PL, PR (the order kFrE ..
// kFrPR of fraction.hpp; ONES: E, QL, QR).  E is always two planes.  In layer n-1 only (LEAF_IN), in round 0 (no fold, nothing
// stored) and in round 1 (FOLD), QL and QR are the halves of t as base words with the leaf map applied in registers - the fold is
// ext_gp_fold_leaf with r alpha formed once per thread - and PL, PR are the halves of p as base words, folded by ext_fold_base; with
// ONES they are not read and stay 1 through the whole layer.  Everywhere else the tables are two planes, read straight from the tree
// or from the folded tables of the round before, and fold by ext_fold.  With FOLD a thread reads four consecutive entries of each
// table, folds them by the previous challenge and stores the two folded entries of both planes; the P pair is folded and stored
// before the Q pair is loaded.
//
// ACCUMULATION (ext_fr_accumulate / ext_fr_accumulate_ones)  Per t = 0 .. 3: m = pl(t) qr(t) + ql(t) (pr(t) + lambda qr(t)) in K -
// lambda qr(t) is linear in t and is stepped by its difference, as fr_accumulate does; ONES: m = qr(t) + ql(t) (1 + lambda qr(t)).
// Then e(t) m goes into the twelve lazy accumulators exactly as in ext_gp_accumulate (ext_gp_mac_cells), and the twelve block sums
// leave as there: two reduce_cells<F, 6>, ext_gp_cells_to_word, finish_pass<F, 8>.  A thread adds at most
// 2^(kFrMaxLog - 2) / kBlock products to an accumulator (one block, layer 27, round 0), far below kAccMaxTerms.
//
// THE HOST FINISH  ext_fr_host_rounds over host planes of the five (three) tables with the same fold, accumulate and map, the eq
// table by ext_gp_host_eq.  The engine runs the layers of at most 2^fr_host_log entries there entirely, from one copy of the bottom
// of the four heaps, and the tail of every larger layer from what its last launch wrote; where layer n falls into the host part, or
// no launch of layer n-1 folded, the leaves are formed on the host.  Every function returns reduced words and a reduced word is
// unique, so the transcript is the same wherever the hand-over falls.
//
// BYTE MODEL of the launch records (include/sumcheck_hip.h, kinds 42, 43; the eq table is kind 41)
//   SC_KIND_EXT_FRACTION_TREE, from layer m = log_in: kf = LV (0: the tail kernel), ks = the planes or base tables read: 1 (LEAF_IN,
//   ONES), 2 (LEAF_IN), else 4.  Reads 8 ks 2^m; writes 32 (2^m - 2^(m-LV)), the tail 32 (2^m - 1).
//   SC_KIND_EXT_FRACTION_PASS, log_in = m for 2^m entries per input table: kf = 1 if it folded, ks = the words per entry of L and R
//   it read: 2 (LEAF_IN, ONES: t), 4 (LEAF_IN: t and p; or planes with ONES), 8 (four tables of two planes).  Reads 16 2^m for E plus
//   8 ks 2^m; writes 16 nt 2^(m-1) with kf = 1 - 80 2^(m-1) with five tables, 48 2^(m-1) with three (ONES) - else 0.
#pragma once
#include <stddef.h>

#include <vector>

#include "../field.hpp"
#include "ext_grand_product.hpp"   // ExtGpLeaf, ext_gp_leaf, ext_gp_fold_leaf, ext_gp_mac_cells, ext_gp_cells_to_word, ext_gp_host_eq
#include "ext_sumprod.hpp"         // ext_mul, ext_fold, ext_fold_base, ext_host_fold
#include "fraction.hpp"            // kFrMaxLog, kFrTailLog, kFrE .. kFrPR

namespace sc {

constexpr int kExtFrTailLog = kFrTailLog - 1;   // the tail kernel takes a layer of at most 2^this entries of K (four planes: 32 KiB of LDS)

// lambda next to the leaf map, as a kernel argument
struct ExtFrLambda {
  u64 v[2];
};

// ---- the work per element ------------------------------------------------------------------------------------------------

// one node: (pa, qa) + (pb, qb) as fractions, in K
template <class F>
SC_HD void ext_fr_node(const F& f, u64 w, const u64 (&pa)[2], const u64 (&qa)[2], const u64 (&pb)[2], const u64 (&qb)[2], u64 (&po)[2], u64 (&qo)[2]) {
  u64 x[2], y[2];
  ext_mul(f, w, pa, qb, x);
  ext_mul(f, w, pb, qa, y);
  po[0] = f.add(x[0], y[0]);
  po[1] = f.add(x[1], y[1]);
  ext_mul(f, w, qa, qb, qo);
}

// One index x of layer m - LV of both tables: pin[j], qin[j] = layer m at x + j 2^(m-LV), j < 2^LV ([entry][component]).  LEAF_IN:
// qin are leaves (formed by the caller) and pin[j][0] is a base word - pin[j][1] is not read; ONES (with LEAF_IN): pin is not
// read, it is all ones.  pout, qout are the little heaps above x as in fr_tree_item: [h + j], j < h, is layer m-d at
// x + j 2^(m-LV) for h = 2^(LV-d), d = 1 .. LV ([0] is not written); [1] is layer m-LV at x.
template <class F, int LV, bool LEAF_IN, bool ONES>
SC_HD void ext_fr_tree_item(const F& f, u64 w, const u64 (&pin)[1 << LV][2], const u64 (&qin)[1 << LV][2], u64 (&pout)[1 << LV][2],
                            u64 (&qout)[1 << LV][2]) {
  static_assert(LEAF_IN || !ONES, "the numerator is all ones at the leaves only");
  constexpr int H = 1 << (LV - 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < H; ++j) {
    if constexpr (ONES) {
      pout[H + j][0] = f.add(qin[j][0], qin[j + H][0]);
      pout[H + j][1] = f.add(qin[j][1], qin[j + H][1]);
      ext_mul(f, w, qin[j], qin[j + H], qout[H + j]);
    } else if constexpr (LEAF_IN) {
      for (int c = 0; c < 2; ++c) {   // base x K: two base multiplications per component
        typename F::Acc a;
        f.acc_zero(a);
        f.acc_mac(a, pin[j][0], qin[j + H][c]);
        f.acc_mac(a, pin[j + H][0], qin[j][c]);
        pout[H + j][c] = f.acc_get(a);
      }
      ext_mul(f, w, qin[j], qin[j + H], qout[H + j]);
    } else {
      ext_fr_node(f, w, pin[j], qin[j], pin[j + H], qin[j + H], pout[H + j], qout[H + j]);
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int h = H / 2; h >= 1; h /= 2) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < h; ++j) ext_fr_node(f, w, pout[2 * h + j], qout[2 * h + j], pout[3 * h + j], qout[3 * h + j], pout[h + j], qout[h + j]);
  }
}

// One item of the cubic pass: the pairs of one index i ([entry][component]) -> the partial products of
// e_i(t) (pl_i(t) qr_i(t) + ql_i(t) (pr_i(t) + lambda qr_i(t))), t = 0 .. 3.  s(t) = pr(t) + lambda qr(t) is linear in t.
template <class F>
SC_HD void ext_fr_accumulate(const F& f, u64 w, typename F::Acc (&acc)[2][6], const u64 (&lambda)[2], const u64 (&e)[2][2], const u64 (&pl)[2][2],
                             const u64 (&pr)[2][2], const u64 (&ql)[2][2], const u64 (&qr)[2][2]) {
  u64 s[2][2], de[2], dpl[2], dql[2], dqr[2], ds[2], et[2], plt[2], qlt[2], qrt[2], st[2];
  for (int h = 0; h < 2; ++h) {
    u64 lq[2];
    ext_mul(f, w, lambda, qr[h], lq);
    s[h][0] = f.add(pr[h][0], lq[0]);
    s[h][1] = f.add(pr[h][1], lq[1]);
  }
  for (int c = 0; c < 2; ++c) {
    de[c] = f.sub(e[1][c], e[0][c]);
    dpl[c] = f.sub(pl[1][c], pl[0][c]);
    dql[c] = f.sub(ql[1][c], ql[0][c]);
    dqr[c] = f.sub(qr[1][c], qr[0][c]);
    ds[c] = f.sub(s[1][c], s[0][c]);
    et[c] = e[0][c];
    plt[c] = pl[0][c];
    qlt[c] = ql[0][c];
    qrt[c] = qr[0][c];
    st[c] = s[0][c];
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      for (int c = 0; c < 2; ++c) {
        et[c] = e[1][c];
        plt[c] = pl[1][c];
        qlt[c] = ql[1][c];
        qrt[c] = qr[1][c];
        st[c] = s[1][c];
      }
    } else if (t > 1) {
      for (int c = 0; c < 2; ++c) {
        et[c] = f.add(et[c], de[c]);
        plt[c] = f.add(plt[c], dpl[c]);
        qlt[c] = f.add(qlt[c], dql[c]);
        qrt[c] = f.add(qrt[c], dqr[c]);
        st[c] = f.add(st[c], ds[c]);
      }
    }
    u64 x[2], y[2];
    ext_mul(f, w, plt, qrt, x);
    ext_mul(f, w, qlt, st, y);
    const u64 m[2] = {f.add(x[0], y[0]), f.add(x[1], y[1])};
    ext_gp_mac_cells(f, acc, t, et, m);
  }
}

// The same with pl = pr = 1: e(t) (qr(t) + ql(t) (1 + lambda qr(t)))
template <class F>
SC_HD void ext_fr_accumulate_ones(const F& f, u64 w, typename F::Acc (&acc)[2][6], const u64 (&lambda)[2], const u64 (&e)[2][2], const u64 (&ql)[2][2],
                                  const u64 (&qr)[2][2]) {
  u64 s[2][2], de[2], dql[2], dqr[2], ds[2], et[2], qlt[2], qrt[2], st[2];
  for (int h = 0; h < 2; ++h) {
    u64 lq[2];
    ext_mul(f, w, lambda, qr[h], lq);
    s[h][0] = f.add(f.one(), lq[0]);
    s[h][1] = lq[1];
  }
  for (int c = 0; c < 2; ++c) {
    de[c] = f.sub(e[1][c], e[0][c]);
    dql[c] = f.sub(ql[1][c], ql[0][c]);
    dqr[c] = f.sub(qr[1][c], qr[0][c]);
    ds[c] = f.sub(s[1][c], s[0][c]);
    et[c] = e[0][c];
    qlt[c] = ql[0][c];
    qrt[c] = qr[0][c];
    st[c] = s[0][c];
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      for (int c = 0; c < 2; ++c) {
        et[c] = e[1][c];
        qlt[c] = ql[1][c];
        qrt[c] = qr[1][c];
        st[c] = s[1][c];
      }
    } else if (t > 1) {
      for (int c = 0; c < 2; ++c) {
        et[c] = f.add(et[c], de[c]);
        qlt[c] = f.add(qlt[c], dql[c]);
        qrt[c] = f.add(qrt[c], dqr[c]);
        st[c] = f.add(st[c], ds[c]);
      }
    }
    u64 y[2];
    ext_mul(f, w, qlt, st, y);
    const u64 m[2] = {f.add(qrt[0], y[0]), f.add(qrt[1], y[1])};
    ext_gp_mac_cells(f, acc, t, et, m);
  }
}

// ---- the host finish ---------------------------------------------------------------------------------------------------

// A host table is two planes: pl[2 q] the c0 words, pl[2 q + 1] the c1 words of table q = kFrE .. kFrPR (n_tables = 3: E, QL, QR).

// the eight words of a round over host tables of 2 n_units entries
template <class F>
inline void ext_fr_host_sums(const F& f, u64 w, u64* const* pl, int n_tables, const u64 (&lambda)[2], size_t n_units, u64 (&out)[8]) {
  typename F::Acc acc[2][6];
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < 6; ++s) f.acc_zero(acc[h][s]);
  for (size_t i = 0; i < n_units; ++i) {
    u64 u[5][2][2];
    for (int q = 0; q < n_tables; ++q)
      for (int h = 0; h < 2; ++h)
        for (int c = 0; c < 2; ++c) u[q][h][c] = pl[2 * q + c][2 * i + h];
    if (n_tables == 3) ext_fr_accumulate_ones(f, w, acc, lambda, u[kFrE], u[kFrQL], u[kFrQR]);
    else ext_fr_accumulate(f, w, acc, lambda, u[kFrE], u[kFrPL], u[kFrPR], u[kFrQL], u[kFrQR]);
  }
  u64 cells[12];
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < 6; ++s) cells[6 * h + s] = f.acc_get(acc[h][s]);
  for (int k = 0; k < 8; ++k) out[k] = ext_gp_cells_to_word(f, w, cells, k);
}

// The rounds first .. first + log_len - 1 of a layer over the host planes pl[0 .. 2 n_tables) of 2^log_len entries each (folded in
// place; on return pl[2 q][0], pl[2 q + 1][0], q >= 1, are the finals).  `given`: the eight words of round `first`, when the device
// has already formed them, else null.  next(round, msg, c) receives a round's eight words and returns false to end the call - or
// sets the challenge c[0..1].  challenges[2 (first ..)] receive what next() drew.  Returns false when next() did.
template <class F, class Next>
inline bool ext_fr_host_rounds(const F& f, u64 w, u64* const* pl, int n_tables, const u64 (&lambda)[2], int log_len, size_t first, const u64* given,
                               u64* challenges, Next&& next) {
  for (int j = 0; j < log_len; ++j) {
    const size_t n_units = (size_t)1 << (log_len - j - 1);
    u64 msg[8];
    if (j == 0 && given) {
      for (int s = 0; s < 8; ++s) msg[s] = given[s];
    } else {
      ext_fr_host_sums(f, w, pl, n_tables, lambda, n_units, msg);
    }
    u64 c[2] = {0, 0};
    if (!next(first + (size_t)j, msg, c)) return false;
    challenges[2 * (first + (size_t)j)] = c[0];
    challenges[2 * (first + (size_t)j) + 1] = c[1];
    for (int q = n_units > 1 ? 0 : 1; q < n_tables; ++q) ext_host_fold(f, w, c, pl[2 * q], pl[2 * q + 1], n_units, false);   // (nobody reads the last E)
  }
  return true;
}

#if defined(__HIPCC__)

static_assert((((u64)1 << (kFrMaxLog - 2)) / kBlock) <= GoldilocksMont::kAccMaxTerms && (((u64)1 << (kFrMaxLog - 2)) / kBlock) <= MontGeneric::kAccMaxTerms,
              "the products one thread of ext_fr_pass_kernel adds to a lazy accumulator (one block, layer 27, round 0)");
static_assert(kExtFrTailLog == 10 && 4 * sizeof(u64) << kExtFrTailLog <= 32 * 1024, "the tail kernel's four planes in LDS");

// Layers m-1 .. m-LV from layer m.  LEAF_IN: qsrc = t and psrc = p (not read with ONES), 2^m base words each, the leaves formed
// here; else the planes of layer m at psrc, psrc + src_stride and qsrc, qsrc + src_stride.  tree: the four heaps (heap h at
// tree + h heap, p.c0, p.c1, q.c0, q.c1; layer k at word 2^k of its heap).  n_units = 2^(m-LV-1) threads' worth of work: unit i owns
// the indices 2i, 2i+1 of layer m - LV.  log_low = m - LV >= 1.
template <class F, int LV, bool LEAF_IN, bool ONES>
__global__ void __launch_bounds__(kBlock) ext_fr_tree_kernel(F f, ExtGpLeaf lf, const u64* __restrict__ psrc, const u64* __restrict__ qsrc,
                                                             size_t src_stride, u64* __restrict__ tree, size_t heap, int log_low, size_t n_units) {
  constexpr int W = 1 << LV;
  const size_t dist = (size_t)1 << log_low;   // words between a unit's loads
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 pa[W][2], pb[W][2], qa[W][2], qb[W][2], opa[W][2], opb[W][2], oqa[W][2], oqb[W][2];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const ull2 y = *reinterpret_cast<const ull2*>(qsrc + (size_t)j * dist + 2 * i);
      if constexpr (LEAF_IN) {
        ext_gp_leaf(f, lf.alpha, lf.beta, y.x, qa[j]);
        ext_gp_leaf(f, lf.alpha, lf.beta, y.y, qb[j]);
        pa[j][1] = pb[j][1] = 0;   // (not read)
        if constexpr (!ONES) {
          const ull2 x = *reinterpret_cast<const ull2*>(psrc + (size_t)j * dist + 2 * i);
          pa[j][0] = x.x;
          pb[j][0] = x.y;
        } else {
          pa[j][0] = pb[j][0] = 0;   // (not read)
        }
      } else {
        const ull2 y1 = *reinterpret_cast<const ull2*>(qsrc + src_stride + (size_t)j * dist + 2 * i);
        const ull2 x = *reinterpret_cast<const ull2*>(psrc + (size_t)j * dist + 2 * i);
        const ull2 x1 = *reinterpret_cast<const ull2*>(psrc + src_stride + (size_t)j * dist + 2 * i);
        qa[j][0] = y.x;
        qa[j][1] = y1.x;
        qb[j][0] = y.y;
        qb[j][1] = y1.y;
        pa[j][0] = x.x;
        pa[j][1] = x1.x;
        pb[j][0] = x.y;
        pb[j][1] = x1.y;
      }
    }
    ext_fr_tree_item<F, LV, LEAF_IN, ONES>(f, lf.w, pa, qa, opa, oqa);
    ext_fr_tree_item<F, LV, LEAF_IN, ONES>(f, lf.w, pb, qb, opb, oqb);
#pragma unroll
    for (int h = W / 2; h >= 1; h /= 2) {
      // layer log_low + log2 h: 2^log_low h entries at word 2^log_low h of each heap
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u64* const pl = tree + (size_t)c * heap + (size_t)h * dist;
        u64* const ql = tree + (size_t)(2 + c) * heap + (size_t)h * dist;
#pragma unroll
        for (int j = 0; j < h; ++j) {
          *reinterpret_cast<ull2*>(pl + (size_t)j * dist + 2 * i) = ull2{opa[h + j][c], opb[h + j][c]};
          *reinterpret_cast<ull2*>(ql + (size_t)j * dist + 2 * i) = ull2{oqa[h + j][c], oqb[h + j][c]};
        }
      }
    }
  }
}

// Layers m-1 .. 0 from layer m (1 <= m <= kExtFrTailLog; psrc, qsrc, src_stride as in ext_fr_tree_kernel): one block.  The leaves'
// numerators enter as (p, 0) or (1, 0) and every level is the product in K: the field identities are exact, so the words are those
// of the base x K form.
template <class F, bool LEAF_IN, bool ONES>
__global__ void __launch_bounds__(kBlock) ext_fr_tree_tail_kernel(F f, ExtGpLeaf lf, const u64* __restrict__ psrc, const u64* __restrict__ qsrc,
                                                                  size_t src_stride, u64* __restrict__ tree, size_t heap, int m) {
  __shared__ u64 v[4][1 << kExtFrTailLog];   // p.c0, p.c1, q.c0, q.c1
  const int n = 1 << m;
  for (int x = threadIdx.x; x < n; x += kBlock) {
    if constexpr (LEAF_IN) {
      u64 o[2];
      ext_gp_leaf(f, lf.alpha, lf.beta, qsrc[x], o);
      v[0][x] = ONES ? f.one() : psrc[x];
      v[1][x] = 0;
      v[2][x] = o[0];
      v[3][x] = o[1];
    } else {
      v[0][x] = psrc[x];
      v[1][x] = psrc[src_stride + x];
      v[2][x] = qsrc[x];
      v[3][x] = qsrc[src_stride + x];
    }
  }
  __syncthreads();
  for (int k = m - 1; k >= 0; --k) {
    const int half = 1 << k;
    // thread x reads entries x and x + half and writes entry x: nobody else touches either this level
    for (int x = threadIdx.x; x < half; x += kBlock) {
      const u64 pa[2] = {v[0][x], v[1][x]}, pb[2] = {v[0][x + half], v[1][x + half]};
      const u64 qa[2] = {v[2][x], v[3][x]}, qb[2] = {v[2][x + half], v[3][x + half]};
      u64 po[2], qo[2];
      ext_fr_node(f, lf.w, pa, qa, pb, qb, po, qo);
      const u64 o[4] = {po[0], po[1], qo[0], qo[1]};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        v[h][x] = o[h];
        tree[(size_t)h * heap + half + x] = o[h];
      }
    }
    __syncthreads();
  }
}

// One round of the cubic sumcheck over the tables kFrE .. kFrPR (ONES: the first three) of K: table q is the planes at in[q] and
// in[q] + stride[q] - but with LEAF_IN in[1 .. 4] are base words (the halves of t, then of p) and the leaves are formed here.
// FOLD: the tables have 4 n_units entries; unit i folds entries 4i .. 4i+3 of each by r = (r0, r1) into entries 2i, 2i+1 of the
// planes at out[.] and out[.] + 2 n_units, and adds them to the twelve sums.  Otherwise: 2 n_units entries, nothing stored.  Eight
// words leave.
struct ExtFrTables {
  const u64* in[5];
  size_t stride[5];
  u64* out[5];
};

// table q of unit i into p[entry][component]; KIND: 0 two planes, 1 base words under the leaf map (t), 2 base words embedded (p)
template <class F, bool FOLD, int KIND>
__device__ __forceinline__ void ext_fr_load(const F& f, const ExtGpLeaf& lf, const u64 (&r)[2], const u64 (&ra)[2], const u64* __restrict__ in, size_t stride,
                                            u64* __restrict__ out, size_t n_units, size_t i, u64 (&p)[2][2]) {
  if constexpr (FOLD) {
    const ull2* src = reinterpret_cast<const ull2*>(in) + 2 * i;
    const ull2 lo = src[0], hi = src[1];
    if constexpr (KIND == 1) {
      ext_gp_fold_leaf(f, lf.alpha, lf.beta, ra, lo.x, lo.y, p[0]);
      ext_gp_fold_leaf(f, lf.alpha, lf.beta, ra, hi.x, hi.y, p[1]);
    } else if constexpr (KIND == 2) {
      ext_fold_base(f, r, lo.x, lo.y, p[0]);
      ext_fold_base(f, r, hi.x, hi.y, p[1]);
    } else {
      const ull2* src1 = reinterpret_cast<const ull2*>(in + stride) + 2 * i;
      const ull2 lo1 = src1[0], hi1 = src1[1];
      const u64 u[4][2] = {{lo.x, lo1.x}, {lo.y, lo1.y}, {hi.x, hi1.x}, {hi.y, hi1.y}};
      ext_fold(f, lf.w, r, u[0], u[1], p[0]);
      ext_fold(f, lf.w, r, u[2], u[3], p[1]);
    }
    reinterpret_cast<ull2*>(out)[i] = ull2{p[0][0], p[1][0]};
    reinterpret_cast<ull2*>(out + 2 * n_units)[i] = ull2{p[0][1], p[1][1]};
  } else {
    const ull2 x = reinterpret_cast<const ull2*>(in)[i];
    if constexpr (KIND == 1) {
      ext_gp_leaf(f, lf.alpha, lf.beta, x.x, p[0]);
      ext_gp_leaf(f, lf.alpha, lf.beta, x.y, p[1]);
    } else if constexpr (KIND == 2) {
      p[0][0] = x.x;
      p[0][1] = 0;
      p[1][0] = x.y;
      p[1][1] = 0;
    } else {
      const ull2 y = reinterpret_cast<const ull2*>(in + stride)[i];
      p[0][0] = x.x;
      p[0][1] = y.x;
      p[1][0] = x.y;
      p[1][1] = y.y;
    }
  }
}

template <class F, bool FOLD, bool LEAF_IN, bool ONES>
__global__ void __launch_bounds__(kBlock) ext_fr_pass_kernel(F f, ExtFrTables tb, ExtGpLeaf lf, ExtFrLambda lam, u64 r0, u64 r1, size_t n_units, PassOut out) {
  __shared__ u64 lds[(kBlock / kWave) * 6];
  __shared__ u64 cells[12];
  __shared__ int lds_flag;
  const u64 r[2] = {r0, r1};
  u64 ra[2] = {0, 0};
  if constexpr (FOLD && LEAF_IN) ext_mul(f, lf.w, r, lf.alpha, ra);
  typename F::Acc acc[2][6];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int s = 0; s < 6; ++s) f.acc_zero(acc[h][s]);
  }
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 p[5][2][2];   // [table][entry][component]
    // the P pair first: folded and stored before the Q pair is loaded
    if constexpr (!ONES) {
#pragma unroll
      for (int q = kFrPL; q <= kFrPR; ++q) ext_fr_load<F, FOLD, LEAF_IN ? 2 : 0>(f, lf, r, ra, tb.in[q], tb.stride[q], tb.out[q], n_units, i, p[q]);
    }
#pragma unroll
    for (int q = kFrQL; q <= kFrQR; ++q) ext_fr_load<F, FOLD, LEAF_IN ? 1 : 0>(f, lf, r, ra, tb.in[q], tb.stride[q], tb.out[q], n_units, i, p[q]);
    ext_fr_load<F, FOLD, 0>(f, lf, r, ra, tb.in[kFrE], tb.stride[kFrE], tb.out[kFrE], n_units, i, p[kFrE]);
    if constexpr (ONES) ext_fr_accumulate_ones(f, lf.w, acc, lam.v, p[kFrE], p[kFrQL], p[kFrQR]);
    else ext_fr_accumulate(f, lf.w, acc, lam.v, p[kFrE], p[kFrPL], p[kFrPR], p[kFrQL], p[kFrQR]);
  }
  const u64 lo6 = reduce_cells<F, 6>(f, acc[0], lds);
  __syncthreads();   // the scratch of the first six sums has been read
  const u64 hi6 = reduce_cells<F, 6>(f, acc[1], lds);
  if (threadIdx.x < 6) {
    cells[threadIdx.x] = lo6;
    cells[6 + threadIdx.x] = hi6;
  }
  __syncthreads();
  const u64 word = threadIdx.x < 8 ? ext_gp_cells_to_word(f, lf.w, cells, (int)threadIdx.x) : 0;
  finish_pass<F, 8>(f, out, word, &lds_flag);
}

#endif   // __HIPCC__

}  // namespace sc
