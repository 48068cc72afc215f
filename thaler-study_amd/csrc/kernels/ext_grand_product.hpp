// Part of kernels.hpp (included there, in order, after ext_sumprod.hpp): the grand product argument of grand_product.hpp with
// every element in the quadratic extension K = F_p[X] / (X^2 - w) of ext_sumprod.hpp - the product tree over K, the three-table
// cubic sumcheck pass of one tree layer over extension tables, the eq table of a point of K^k, and the host code that finishes
// the small layers and the tails of the large ones.  The work per element is in SC_HD and plain inline functions, which compile
// without hipcc: tests/cpp/ext_gp_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract: that of grand_product.hpp word for word, every element in K)
//
//   An element of K is two Montgomery words (c0, c1), meaning c0 + c1 X; it crosses the ABI as two consecutive words.
//
//   Leaves.  The input is a base-field table t of 2^n entries, 1 <= n <= 28, and alpha, beta in K, alpha != 0:
//   V_n[i] = beta + alpha t[i], componentwise c0 = beta0 + alpha0 t[i], c1 = beta1 + alpha1 t[i] (ext_gp_leaf: two base
//   multiplications).  The leaves are NEVER STORED: they are formed in registers wherever layer n is read.
//
//   Tree.  For k = n-1 .. 0, V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k], x < 2^k, a product in K (ext_mul).  P = V_0[0] in K.
//   L_k = V_(k+1)[0 .. 2^k) and R_k = V_(k+1)[2^k .. 2^(k+1)).
//
//   Layer k = 0 .. n-1 turns the claim V_k~(z_k) = c_k, z_k in K^k, into a claim about V_(k+1); z_0 = (), c_0 = P.
//    - Rounds.  A sumcheck of k rounds over sum_{x in {0,1}^k} eq(z_k, x) L_k(x) R_k(x) = c_k, variable 0 first.  Before round j
//      the tables E, L, R have 2^(k-j) entries of K; with u_i(t) = u[2i] + t (u[2i+1] - u[2i]) the message is
//      H_j(t) = sum_i e_i(t) l_i(t) r_i(t) in K at t = 0, 1, 2, 3: eight words H(0).c0, H(0).c1, .., H(3).c0, H(3).c1.  V checks
//      H_j(0) + H_j(1) against the running claim and draws r_j in K (two words); the new claim is the cubic through the four values
//      at r_j; all three tables fold by r_j.  Layer 0 has no rounds.
//    - Finals.  P sends l = L~(r) and r' = R~(r) in K, four words.  V checks eq(z_k, r) l r' against the running claim.
//    - Combining challenge.  V draws rho_k in K; c_(k+1) = l + rho_k (r' - l) and z_(k+1) = (r, rho_k).
//   After layer n-1 the claim is V_n~(z_n) = c_n, that is t~(z_n) = (c_n - beta) alpha^-1 at z_n in K^n: the caller checks it with
//   sc_table_evaluate_ext or with an opening of a commitment to t at the extension point.
//
//   Fields with p <= 3 are refused, w must be a quadratic non-residue (the engine checks both on the host).  Nothing beyond the
//   book's statement is claimed: no zero knowledge, no Fiat-Shamir.
//
// THE LAYOUT  An extension table of 2^m entries is two planes of 2^m words, all c0 words then all c1 words, as in ext_sumprod.hpp.
// THE TREE is one pool block of two heaps of 2^n words each: layer k of plane c occupies words c 2^n + [2^k, 2^(k+1)), k < n.
// Every load and store keeps the shape of gp_tree_kernel and gp_pass_kernel: a lane reads and writes 16 contiguous bytes, a wave
// 1 KiB.
//   ext_gp_tree_kernel<F, LV, LEAF_IN>, LV = 1, 2, 3: the schedule and access pattern of gp_tree_kernel, per plane.  With LEAF_IN
//   (the first launch) it reads the base words of t and forms the leaves; otherwise it reads both planes of layer m.  It stores
//   both planes of the layers m-1 .. m-LV.
//   ext_gp_tree_tail_kernel<F, LEAF_IN>: one block takes a layer of at most 2^kExtGpTailLog entries down to V_0 through LDS
//   (two planes: 32 KiB), one barrier per level, and stores every layer.  LEAF_IN where n <= kExtGpTailLog.
//   Schedule: from layer n, LV = min(gp_tree_lv, layers left above kExtGpTailLog), then the tail kernel.
//
// THE CUBIC PASS  ext_gp_pass_kernel<F, FOLD, LEAF_IN>: one launch per round over E, L, R.  E is always two planes; L and R are two
// planes read straight from the tree - or, in layer n-1 only (LEAF_IN), the two halves of t as base words with the leaf map
// applied in registers: in round 0 (no fold, nothing stored) and in round 1 (FOLD).  The LEAF_IN fold uses that the map is affine:
// V(u0) + r (V(u1) - V(u0)) = beta + alpha u0 + (r alpha)(u1 - u0), four base multiplications per folded entry with r alpha formed
// once per thread (ext_gp_fold_leaf); the field identities are exact and a reduced word is unique, so the transcript is the same
// as with the leaves folded by ext_fold.  With FOLD a thread reads four consecutive entries of each table, folds them by the
// previous challenge and stores the two folded entries of both planes.
//
// ACCUMULATION (ext_gp_accumulate)  Per t = 0 .. 3: m = l(t) r(t) by ext_mul, reduced; then the three Karatsuba partial products
// of e(t) m go into lazy accumulators: e0 m0, e1 m1, (e0 + e1)(m0 + m1) - twelve per thread, kept as two groups of six
// (t = 0, 1 and t = 2, 3).  The map from the twelve sums to the eight words H(t) = (S00 + w S11, Sm - S00 - S11) is linear, so it
// commutes with the sum over blocks: every block applies it to ITS twelve block sums (ext_gp_cells_to_word, which is
// ext_cells_to_word over four triples) and the launch leaves through finish_pass<F, 8>.  The block sums are formed by two calls
// of reduce_cells<F, 6>: reduce_cells takes fewer than nine cells or a multiple of nine.  A thread adds at most
// 2^(kGpMaxLog - 2) / kBlock products to an accumulator (one block, layer 27, round 0), far below kAccMaxTerms.
//
// THE EQ TABLE  ext_eq_table_kernel<F>: eq(z, .) for z in K^k, k >= 1, into two planes: the per-entry product of eq_table_kernel in
// K; a thread forms the entries 2i and 2i + 1, which share the factors of the coordinates 1 .. k-1 (k + 1 products in K per pair).
//
// THE HOST FINISH  ext_gp_host_rounds: the rounds of a layer over host planes of E, L, R with the same fold, accumulate and map;
// ext_gp_host_eq: the eq table by doubling.  The engine runs the layers of at most 2^gp_host_log entries there entirely, and the
// tail of every larger layer from what its last launch wrote; where layer n itself falls into the host part the leaves are formed
// with ext_gp_leaf.  The transcript is the same wherever the hand-over falls.
//
// BYTE MODEL of the launch records (include/sumcheck_hip.h, kinds 39 .. 41)
//   SC_KIND_EXT_PRODUCT_TREE, from layer m = log_in: kf = LV (0: the tail kernel), ks = 1 with LEAF_IN, else 2.  Reads 8 * 2^m
//   (ks = 1) or 16 * 2^m (ks = 2); writes 16 * (2^m - 2^(m-LV)), the tail 16 * (2^m - 1).
//   SC_KIND_EXT_PRODUCT_PASS, log_in = m for 2^m entries per input table: kf = 1 if it folded, ks = 1 with LEAF_IN, else 2.  Reads
//   16 * 2^m for E plus 2 * 8 * 2^m (ks = 1) or 2 * 16 * 2^m (ks = 2) for L and R; writes 48 * 2^(m-1) with kf = 1, else 0.
//   SC_KIND_EXT_EQ_TABLE, log_in = k: reads the 2 k words of the point, writes 16 * 2^k.
#pragma once
#include <stddef.h>

#include <vector>

#include "../field.hpp"
#include "ext_sumprod.hpp"     // ext_mul, ext_fold, ext_fold_base, ext_host_fold, ext_cells_to_word
#include "grand_product.hpp"   // kGpMaxLog, kGpTailLog

namespace sc {

constexpr int kExtGpTailLog = kGpTailLog - 1;   // the tail kernel takes a layer of at most 2^this entries of K (two planes: 32 KiB of LDS)

// alpha, beta and w as a kernel argument
struct ExtGpLeaf {
  u64 w;
  u64 alpha[2], beta[2];
};

// ---- the work per element ------------------------------------------------------------------------------------------------

// a leaf: beta + alpha t, t a base word
template <class F>
SC_HD void ext_gp_leaf(const F& f, const u64 (&alpha)[2], const u64 (&beta)[2], u64 t, u64 (&o)[2]) {
  o[0] = f.add(beta[0], f.mul(alpha[0], t));
  o[1] = f.add(beta[1], f.mul(alpha[1], t));
}

// the leaves of two base words folded by r, with ra = r alpha: beta + alpha u0 + ra (u1 - u0)
template <class F>
SC_HD void ext_gp_fold_leaf(const F& f, const u64 (&alpha)[2], const u64 (&beta)[2], const u64 (&ra)[2], u64 u0, u64 u1, u64 (&o)[2]) {
  const u64 d = f.sub(u1, u0);
  u64 v[2];
  ext_gp_leaf(f, alpha, beta, u0, v);
  o[0] = f.add(v[0], f.mul(ra[0], d));
  o[1] = f.add(v[1], f.mul(ra[1], d));
}

// One index x of layer m - LV: in[j] = V_m[x + j 2^(m-LV)], j < 2^LV ([entry][component]).  out is the little heap above x:
// out[h + j], j < h, is V_(m-d)[x + j 2^(m-LV)] for h = 2^(LV-d), d = 1 .. LV (out[0] is not written); out[1] is V_(m-LV)[x].
template <class F, int LV>
SC_HD void ext_gp_tree_item(const F& f, u64 w, const u64 (&in)[1 << LV][2], u64 (&out)[1 << LV][2]) {
  constexpr int H = 1 << (LV - 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < H; ++j) ext_mul(f, w, in[j], in[j + H], out[H + j]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int h = H / 2; h >= 1; h /= 2) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < h; ++j) ext_mul(f, w, out[2 * h + j], out[3 * h + j], out[h + j]);
  }
}

// e(t) m into the accumulators of t: acc[t / 2][3 (t % 2)] += e0 m0, [.. + 1] += e1 m1, [.. + 2] += (e0 + e1)(m0 + m1)
template <class F>
SC_HD void ext_gp_mac_cells(const F& f, typename F::Acc (&acc)[2][6], int t, const u64 (&et)[2], const u64 (&m)[2]) {
  f.acc_mac(acc[t >> 1][3 * (t & 1)], et[0], m[0]);
  f.acc_mac(acc[t >> 1][3 * (t & 1) + 1], et[1], m[1]);
  f.acc_mac(acc[t >> 1][3 * (t & 1) + 2], f.add(et[0], et[1]), f.add(m[0], m[1]));
}

// One item of the cubic pass: the pairs (e, l, r)[0..1] of one index i ([entry][component]) -> the partial products of
// e_i(t) (l_i(t) r_i(t)), t = 0 .. 3: with m = l(t) r(t), acc[t / 2][3 (t % 2)] += e0 m0, [.. + 1] += e1 m1,
// [.. + 2] += (e0 + e1)(m0 + m1)
template <class F>
SC_HD void ext_gp_accumulate(const F& f, u64 w, typename F::Acc (&acc)[2][6], const u64 (&e)[2][2], const u64 (&l)[2][2], const u64 (&r)[2][2]) {
  u64 de[2], dl[2], dr[2], et[2], lt[2], rt[2];
  for (int c = 0; c < 2; ++c) {
    de[c] = f.sub(e[1][c], e[0][c]);
    dl[c] = f.sub(l[1][c], l[0][c]);
    dr[c] = f.sub(r[1][c], r[0][c]);
    et[c] = e[0][c];
    lt[c] = l[0][c];
    rt[c] = r[0][c];
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      for (int c = 0; c < 2; ++c) {
        et[c] = e[1][c];
        lt[c] = l[1][c];
        rt[c] = r[1][c];
      }
    } else if (t > 1) {
      for (int c = 0; c < 2; ++c) {
        et[c] = f.add(et[c], de[c]);
        lt[c] = f.add(lt[c], dl[c]);
        rt[c] = f.add(rt[c], dr[c]);
      }
    }
    u64 m[2];
    ext_mul(f, w, lt, rt, m);
    ext_gp_mac_cells(f, acc, t, et, m);
  }
}

// word k < 8 of the message from the twelve sums (S00, S11, Sm per t): H(t).c0 = S00 + w S11 (k = 2 t), H(t).c1 = Sm - S00 - S11
template <class F>
SC_HD u64 ext_gp_cells_to_word(const F& f, u64 w, const u64* cells, int k) {
  return ext_cells_to_word(f, w, cells, k);
}

// ---- the host finish ---------------------------------------------------------------------------------------------------

// A host table is two planes: pl[2 q] the c0 words, pl[2 q + 1] the c1 words of table q = 0, 1, 2 (E, L, R).

// the eight words of a round over host tables of 2 n_units entries
template <class F>
inline void ext_gp_host_sums(const F& f, u64 w, u64* const* pl, size_t n_units, u64 (&out)[8]) {
  typename F::Acc acc[2][6];
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < 6; ++s) f.acc_zero(acc[h][s]);
  for (size_t i = 0; i < n_units; ++i) {
    u64 p[3][2][2];
    for (int q = 0; q < 3; ++q)
      for (int h = 0; h < 2; ++h)
        for (int c = 0; c < 2; ++c) p[q][h][c] = pl[2 * q + c][2 * i + h];
    ext_gp_accumulate(f, w, acc, p[0], p[1], p[2]);
  }
  u64 cells[12];
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < 6; ++s) cells[6 * h + s] = f.acc_get(acc[h][s]);
  for (int k = 0; k < 8; ++k) out[k] = ext_gp_cells_to_word(f, w, cells, k);
}

// eq(z, .) over k variables, z in K^k (2 k words), as host planes of 2^k words: out[i] = prod_j (bit_j(i) ? z[j] : 1 - z[j])
template <class F>
inline void ext_gp_host_eq(const F& f, u64 w, const u64* z, int k, u64* out0, u64* out1) {
  out0[0] = f.one();
  out1[0] = 0;
  for (int j = 0; j < k; ++j) {
    const size_t half = (size_t)1 << j;
    const u64 zj[2] = {z[2 * j], z[2 * j + 1]};
    for (size_t c = half; c-- > 0;) {
      const u64 base[2] = {out0[c], out1[c]};
      u64 hi[2];
      ext_mul(f, w, base, zj, hi);
      out0[c + half] = hi[0];
      out1[c + half] = hi[1];
      out0[c] = f.sub(base[0], hi[0]);
      out1[c] = f.sub(base[1], hi[1]);
    }
  }
}

// The rounds first .. first + log_len - 1 of a layer over the host planes pl[0 .. 6) of E, L, R, 2^log_len entries each (folded in
// place; on return pl[2][0], pl[3][0] are l and pl[4][0], pl[5][0] are r').  `given`: the eight words of round `first`, when the
// device has already formed them, else null.  next(round, msg, c) receives a round's eight words and returns false to end the
// call - or sets the challenge c[0..1].  challenges[2 (first ..)] receive what next() drew.  Returns false when next() did.
template <class F, class Next>
inline bool ext_gp_host_rounds(const F& f, u64 w, u64* const* pl, int log_len, size_t first, const u64* given, u64* challenges, Next&& next) {
  for (int j = 0; j < log_len; ++j) {
    const size_t n_units = (size_t)1 << (log_len - j - 1);
    u64 msg[8];
    if (j == 0 && given) {
      for (int s = 0; s < 8; ++s) msg[s] = given[s];
    } else {
      ext_gp_host_sums(f, w, pl, n_units, msg);
    }
    u64 c[2] = {0, 0};
    if (!next(first + (size_t)j, msg, c)) return false;
    challenges[2 * (first + (size_t)j)] = c[0];
    challenges[2 * (first + (size_t)j) + 1] = c[1];
    for (int q = n_units > 1 ? 0 : 1; q < 3; ++q) ext_host_fold(f, w, c, pl[2 * q], pl[2 * q + 1], n_units, false);   // (nobody reads the last E)
  }
  return true;
}

#if defined(__HIPCC__)

static_assert((((u64)1 << (kGpMaxLog - 2)) / kBlock) <= GoldilocksMont::kAccMaxTerms && (((u64)1 << (kGpMaxLog - 2)) / kBlock) <= MontGeneric::kAccMaxTerms,
              "the products one thread of ext_gp_pass_kernel adds to a lazy accumulator (one block, layer 27, round 0)");
static_assert(2 * sizeof(u64) << kExtGpTailLog <= 32 * 1024, "the tail kernel's two planes in LDS");

// Layers m-1 .. m-LV from layer m.  LEAF_IN: src = t, 2^m base words, the leaves formed here; else the planes of layer m at src and
// src + src_stride.  tree: the two heaps (plane c at tree + c heap; layer k at word 2^k of its heap).  n_units = 2^(m-LV-1)
// threads' worth of work: unit i owns the indices 2i, 2i+1 of layer m - LV.  log_low = m - LV >= 1.
template <class F, int LV, bool LEAF_IN>
__global__ void __launch_bounds__(kBlock) ext_gp_tree_kernel(F f, ExtGpLeaf lf, const u64* __restrict__ src, size_t src_stride, u64* __restrict__ tree,
                                                             size_t heap, int log_low, size_t n_units) {
  constexpr int W = 1 << LV;
  const size_t dist = (size_t)1 << log_low;   // words between a unit's loads
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 a[W][2], b[W][2], oa[W][2], ob[W][2];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const ull2 x = *reinterpret_cast<const ull2*>(src + (size_t)j * dist + 2 * i);
      if constexpr (LEAF_IN) {
        ext_gp_leaf(f, lf.alpha, lf.beta, x.x, a[j]);
        ext_gp_leaf(f, lf.alpha, lf.beta, x.y, b[j]);
      } else {
        const ull2 y = *reinterpret_cast<const ull2*>(src + src_stride + (size_t)j * dist + 2 * i);
        a[j][0] = x.x;
        a[j][1] = y.x;
        b[j][0] = x.y;
        b[j][1] = y.y;
      }
    }
    ext_gp_tree_item<F, LV>(f, lf.w, a, oa);
    ext_gp_tree_item<F, LV>(f, lf.w, b, ob);
#pragma unroll
    for (int h = W / 2; h >= 1; h /= 2) {
      // layer log_low + log2 h: 2^log_low h entries at word 2^log_low h of each heap
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u64* layer = tree + (size_t)c * heap + (size_t)h * dist;
#pragma unroll
        for (int j = 0; j < h; ++j) *reinterpret_cast<ull2*>(layer + (size_t)j * dist + 2 * i) = ull2{oa[h + j][c], ob[h + j][c]};
      }
    }
  }
}

// Layers m-1 .. 0 from layer m (1 <= m <= kExtGpTailLog; src as in ext_gp_tree_kernel): one block
template <class F, bool LEAF_IN>
__global__ void __launch_bounds__(kBlock) ext_gp_tree_tail_kernel(F f, ExtGpLeaf lf, const u64* __restrict__ src, size_t src_stride,
                                                                  u64* __restrict__ tree, size_t heap, int m) {
  __shared__ u64 v[2][1 << kExtGpTailLog];
  const int n = 1 << m;
  for (int x = threadIdx.x; x < n; x += kBlock) {
    if constexpr (LEAF_IN) {
      u64 o[2];
      ext_gp_leaf(f, lf.alpha, lf.beta, src[x], o);
      v[0][x] = o[0];
      v[1][x] = o[1];
    } else {
      v[0][x] = src[x];
      v[1][x] = src[src_stride + x];
    }
  }
  __syncthreads();
  for (int k = m - 1; k >= 0; --k) {
    const int half = 1 << k;
    // thread x reads entries x and x + half and writes entry x: nobody else touches either this level
    for (int x = threadIdx.x; x < half; x += kBlock) {
      const u64 lo[2] = {v[0][x], v[1][x]}, hi[2] = {v[0][x + half], v[1][x + half]};
      u64 y[2];
      ext_mul(f, lf.w, lo, hi, y);
      v[0][x] = y[0];
      v[1][x] = y[1];
      tree[half + x] = y[0];
      tree[heap + half + x] = y[1];
    }
    __syncthreads();
  }
}

// eq(z, .) for z in K^k, k >= 1 (rv.v[2 j], rv.v[2 j + 1] = z_j), into the planes at out and out + 2^k; n_pairs = 2^(k-1): unit i
// forms the entries 2i, 2i+1
template <class F>
__global__ void __launch_bounds__(kBlock) ext_eq_table_kernel(F f, RVec rv, u64 w, int k, size_t n_pairs, u64* __restrict__ out) {
  const u64 z0[2] = {rv.v[0], rv.v[1]};
  const u64 nz0[2] = {f.sub(f.one(), z0[0]), f.sub(0, z0[1])};
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_pairs; i += (size_t)gridDim.x * kBlock) {
    u64 acc[2] = {f.one(), 0};
    for (int j = 1; j < k; ++j) {
      const bool set = (i >> (j - 1)) & 1;
      const u64 zj[2] = {rv.v[2 * j], rv.v[2 * j + 1]};
      const u64 fj[2] = {set ? zj[0] : f.sub(f.one(), zj[0]), set ? zj[1] : f.sub(0, zj[1])};
      u64 nx[2];
      ext_mul(f, w, acc, fj, nx);
      acc[0] = nx[0];
      acc[1] = nx[1];
    }
    u64 lo[2], hi[2];
    ext_mul(f, w, acc, nz0, lo);
    ext_mul(f, w, acc, z0, hi);
    reinterpret_cast<ull2*>(out)[i] = ull2{lo[0], hi[0]};
    reinterpret_cast<ull2*>(out + 2 * n_pairs)[i] = ull2{lo[1], hi[1]};
  }
}

// One round of the cubic sumcheck over tables T[0..2] = E, L, R of K: table q is the planes at in[q] and in[q] + stride[q] - but
// with LEAF_IN in[1], in[2] are base words (the halves of t) and the leaf map is applied here.  FOLD: the tables have 4 n_units
// entries; unit i folds entries 4i .. 4i+3 of each by r = (r0, r1) into entries 2i, 2i+1 of the planes at out[.] and
// out[.] + 2 n_units, and adds them to the twelve sums.  Otherwise: 2 n_units entries, nothing stored.  Eight words leave.
struct ExtGpTables {
  const u64* in[3];
  size_t stride[3];
  u64* out[3];
};
template <class F, bool FOLD, bool LEAF_IN>
__global__ void __launch_bounds__(kBlock) ext_gp_pass_kernel(F f, ExtGpTables tb, ExtGpLeaf lf, u64 r0, u64 r1, size_t n_units, PassOut out) {
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
    u64 p[3][2][2];   // [table][entry][component]
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const bool leaf = LEAF_IN && q > 0;
      if constexpr (FOLD) {
        const ull2* src = reinterpret_cast<const ull2*>(tb.in[q]) + 2 * i;
        const ull2 lo = src[0], hi = src[1];
        if (leaf) {
          ext_gp_fold_leaf(f, lf.alpha, lf.beta, ra, lo.x, lo.y, p[q][0]);
          ext_gp_fold_leaf(f, lf.alpha, lf.beta, ra, hi.x, hi.y, p[q][1]);
        } else {
          const ull2* src1 = reinterpret_cast<const ull2*>(tb.in[q] + tb.stride[q]) + 2 * i;
          const ull2 lo1 = src1[0], hi1 = src1[1];
          const u64 u[4][2] = {{lo.x, lo1.x}, {lo.y, lo1.y}, {hi.x, hi1.x}, {hi.y, hi1.y}};
          ext_fold(f, lf.w, r, u[0], u[1], p[q][0]);
          ext_fold(f, lf.w, r, u[2], u[3], p[q][1]);
        }
        reinterpret_cast<ull2*>(tb.out[q])[i] = ull2{p[q][0][0], p[q][1][0]};
        reinterpret_cast<ull2*>(tb.out[q] + 2 * n_units)[i] = ull2{p[q][0][1], p[q][1][1]};
      } else {
        const ull2 x = reinterpret_cast<const ull2*>(tb.in[q])[i];
        if (leaf) {
          ext_gp_leaf(f, lf.alpha, lf.beta, x.x, p[q][0]);
          ext_gp_leaf(f, lf.alpha, lf.beta, x.y, p[q][1]);
        } else {
          const ull2 y = reinterpret_cast<const ull2*>(tb.in[q] + tb.stride[q])[i];
          p[q][0][0] = x.x;
          p[q][0][1] = y.x;
          p[q][1][0] = x.y;
          p[q][1][1] = y.y;
        }
      }
    }
    ext_gp_accumulate(f, lf.w, acc, p[0], p[1], p[2]);
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
