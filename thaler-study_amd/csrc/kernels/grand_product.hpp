// Part of kernels.hpp (included there, in order): the grand product argument - the product tree of a table, the three-table
// cubic sumcheck pass of one tree layer, an affine map of a table, and the host code that finishes the small layers and the
// tails of the large ones.  The host parts (SC_HD and plain inline functions) compile without hipcc:
// tests/cpp/gp_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract; Thaler, "Proofs, Arguments, and Zero-Knowledge", section 4.6: the GKR protocol specialised to a
// binary tree of multiplication gates; Setty, "Spartan", section 7: product circuits)
//
//   All tables are LE tables of Montgomery words, variable 0 first, as everywhere in the ABI.
//
//   Tree.  The input is V_n = t, 2^n entries, 1 <= n <= 28.  For k = n-1 .. 0, V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k], x < 2^k:
//   the tree splits by halves, the new variable of V_(k+1) is its highest.  The claimed product is P = V_0[0].
//   L_k = V_(k+1)[0 .. 2^k) and R_k = V_(k+1)[2^k .. 2^(k+1)): two contiguous tables of k variables inside one buffer.
//
//   Layer k = 0 .. n-1 turns the claim V_k~(z_k) = c_k, z_k in F^k, into a claim about V_(k+1); z_0 = (), c_0 = P.
//    - Rounds.  A sumcheck of k rounds over sum_{x in {0,1}^k} eq(z_k, x) L_k(x) R_k(x) = c_k, variable 0 first.  Before round j
//      the tables E, L, R have 2^(k-j) entries; with u_i(t) = u[2i] + t (u[2i+1] - u[2i]) the message is
//      H_j(t) = sum_i e_i(t) l_i(t) r_i(t) at t = 0, 1, 2, 3.  V checks H_j(0) + H_j(1) against the running claim and draws r_j;
//      the new claim is the cubic through the four values at r_j; all three tables fold by r_j.  Layer 0 has no rounds.
//    - Finals.  P sends l = L~(r) and r' = R~(r).  V checks eq(z_k, r) l r' against the running claim (at k = 0: l r' = P).
//    - Combining challenge.  V draws rho_k; c_(k+1) = l + rho_k (r' - l) and z_(k+1) = (r, rho_k).
//   After layer n-1 the claim is t~(z_n) = c_n: the caller checks it with sc_table_evaluate or with an opening of a commitment
//   to t.
//
//   Fields with p <= 3 are refused (interpolation on {0, 1, 2, 3} needs 2 and 3 invertible).  Nothing beyond the book's
//   statement is claimed: no security level, no zero knowledge, no Fiat-Shamir.
//
// THE TREE is one pool block in heap layout: layer k occupies words [2^k, 2^(k+1)), k = 0 .. n-1 (word 0 is unused); V_n is the
// caller's table, borrowed and never written.
//   gp_tree_kernel<F, LV>, LV = 1, 2, 3: one launch reads layer m once and writes layers m-1 .. m-LV.  A thread owns two adjacent
//   indices x, x+1 of layer m-LV: 2^LV 16-byte loads at a distance of 2^(m-LV) words, each lane-contiguous across the wave, the
//   2^LV - 1 products per index (gp_tree_item), and every intermediate layer stored with 16-byte lane-contiguous stores.  No LDS,
//   no atomics.  m - LV >= 1.
//   gp_tree_tail_kernel<F>: one block takes a layer of at most 2^kGpTailLog words down to V_0 through LDS, one barrier per level,
//   and stores every layer.
//   Schedule: from layer n, LV = min(kGpTreeLv, layers left above kGpTailLog), then the tail kernel.
//
// THE CUBIC PASS  gp_pass_kernel<F, FOLD>: one launch per round over E, L, R.  With FOLD a thread reads four consecutive entries
// of each table (two 16-byte loads), folds them by the previous challenge (zc_fold4 of kernels/r1cs.hpp), stores the two folded
// entries and adds e(t) l(t) r(t), t = 0 .. 3, into four lazy accumulators (gp_accumulate); round 0 reads pairs and stores
// nothing.  The sums leave through reduce_cells<F, 4> / finish_pass<F, 4>.  Inputs are never written: the first launch of a
// layer reads L and R straight from the tree.
//
// THE HOST FINISH  gp_host_rounds: the rounds of a layer over host copies of E, L, R with the same fold and accumulate; the
// engine runs the layers of at most 2^gp_host_log entries there entirely, and the tail of every larger layer from the tables
// its last launch wrote.
#pragma once
#include <vector>

#include "../field.hpp"
#include "r1cs.hpp"   // zc_fold4

namespace sc {

constexpr int kGpMaxLog = 28;     // n at most
constexpr int kGpTailLog = 12;    // the tail kernel takes a layer of at most 2^this words (32 KiB of LDS)
constexpr int kGpTreeLv = 3;      // layers per launch above the tail (measured: DESIGN.md section 9 item 16)
constexpr int kGpHostLogMax = 12; // option "gp_host_log" at most

// One index x of layer m - LV: in[j] = V_m[x + j 2^(m-LV)], j < 2^LV.  out is the little heap above x: out[h + j], j < h, is
// V_(m-d)[x + j 2^(m-LV)] for h = 2^(LV-d), d = 1 .. LV (out[0] is not written); out[1] is V_(m-LV)[x].
template <class F, int LV>
SC_HD void gp_tree_item(const F& f, const u64 (&in)[1 << LV], u64 (&out)[1 << LV]) {
  constexpr int H = 1 << (LV - 1);
#pragma unroll
  for (int j = 0; j < H; ++j) out[H + j] = f.mul(in[j], in[j + H]);
#pragma unroll
  for (int h = H / 2; h >= 1; h /= 2) {
#pragma unroll
    for (int j = 0; j < h; ++j) out[h + j] = f.mul(out[2 * h + j], out[3 * h + j]);
  }
}

// One item of the cubic pass: the pairs (e, l, r)[0..1] of one index i -> H(0..3) += e_i(t) l_i(t) r_i(t).
template <class F>
SC_HD void gp_accumulate(const F& f, typename F::Acc (&acc)[4], const u64 (&e)[2], const u64 (&l)[2], const u64 (&r)[2]) {
  const u64 de = f.sub(e[1], e[0]), dl = f.sub(l[1], l[0]), dr = f.sub(r[1], r[0]);
  u64 et = e[0], lt = l[0], rt = r[0];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      et = e[1]; lt = l[1]; rt = r[1];
    } else if (t > 1) {
      et = f.add(et, de); lt = f.add(lt, dl); rt = f.add(rt, dr);
    }
    f.acc_mac(acc[t], et, f.mul(lt, rt));
  }
}

// ---- the host finish ---------------------------------------------------------------------------------------------------

// H(0..3) of a round over host tables of 2 n_units entries
template <class F>
inline void gp_host_sums(const F& f, const u64* e, const u64* l, const u64* r, size_t n_units, u64 (&out)[4]) {
  typename F::Acc acc[4];
  for (int t = 0; t < 4; ++t) f.acc_zero(acc[t]);
  for (size_t i = 0; i < n_units; ++i) {
    const u64 ei[2] = {e[2 * i], e[2 * i + 1]}, li[2] = {l[2 * i], l[2 * i + 1]}, ri[2] = {r[2 * i], r[2 * i + 1]};
    gp_accumulate(f, acc, ei, li, ri);
  }
  for (int t = 0; t < 4; ++t) out[t] = f.acc_get(acc[t]);
}

// u (2 n_out entries) folded by c in place to n_out entries; n_out odd only when it is 1
template <class F>
inline void gp_host_fold(const F& f, u64 c, u64* u, size_t n_out) {
  if (n_out == 1) {
    u[0] = f.add(u[0], f.mul(c, f.sub(u[1], u[0])));
    return;
  }
  for (size_t i = 0; i < n_out / 2; ++i) {
    const u64 q[4] = {u[4 * i], u[4 * i + 1], u[4 * i + 2], u[4 * i + 3]};
    u64 o[2];
    zc_fold4(f, c, q, o);
    u[2 * i] = o[0];
    u[2 * i + 1] = o[1];
  }
}

// eq(z, .) over k variables as a host table: out[i] = prod_j (bit_j(i) ? z[j] : 1 - z[j]); out has 2^k entries
template <class F>
inline void gp_host_eq(const F& f, const u64* z, int k, u64* out) {
  out[0] = f.one();
  for (int j = 0; j < k; ++j) {
    const size_t half = (size_t)1 << j;
    for (size_t c = half; c-- > 0;) {
      const u64 base = out[c];
      out[c + half] = f.mul(base, z[j]);
      out[c] = f.sub(base, out[c + half]);
    }
  }
}

// The rounds first .. first + log_len - 1 of a layer over host tables e, l, r of 2^log_len entries each (folded in place; on
// return l[0] and r[0] are the finals).  `given`: H(0..3) of round `first`, when the device has already formed it, else null.
// next(round, msg, &c) receives a round's four values and returns false to end the call - or sets the challenge c.
// challenges[first ..] receive what next() drew.  Returns false when next() did.
template <class F, class Next>
inline bool gp_host_rounds(const F& f, u64* e, u64* l, u64* r, int log_len, size_t first, const u64* given, u64* challenges, Next&& next) {
  for (int j = 0; j < log_len; ++j) {
    const size_t n_units = (size_t)1 << (log_len - j - 1);
    u64 msg[4];
    if (j == 0 && given) {
      for (int t = 0; t < 4; ++t) msg[t] = given[t];
    } else {
      gp_host_sums(f, e, l, r, n_units, msg);
    }
    u64 c = 0;
    if (!next(first + (size_t)j, msg, &c)) return false;
    challenges[first + (size_t)j] = c;
    gp_host_fold(f, c, l, n_units);
    gp_host_fold(f, c, r, n_units);
    if (n_units > 1) gp_host_fold(f, c, e, n_units);   // (nobody reads the last E)
  }
  return true;
}

#if defined(__HIPCC__)

// Layers m-1 .. m-LV from layer m = src (2^m words); tree: the heap (layer k at word 2^k).  n_units = 2^(m-LV-1) threads' worth
// of work: unit i owns the indices 2i, 2i+1 of layer m - LV.  log_low = m - LV >= 1.
template <class F, int LV>
__global__ void __launch_bounds__(kBlock) gp_tree_kernel(F f, const u64* __restrict__ src, u64* __restrict__ tree, int log_low, size_t n_units) {
  constexpr int W = 1 << LV;
  const size_t dist = (size_t)1 << log_low;   // words between a unit's loads
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 a[W], b[W], oa[W], ob[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const ull2 x = *reinterpret_cast<const ull2*>(src + (size_t)j * dist + 2 * i);
      a[j] = x.x;
      b[j] = x.y;
    }
    gp_tree_item<F, LV>(f, a, oa);
    gp_tree_item<F, LV>(f, b, ob);
#pragma unroll
    for (int h = W / 2; h >= 1; h /= 2) {
      // layer log_low + log2 h: 2^log_low h words at tree + 2^log_low h
      u64* layer = tree + (size_t)h * dist;
#pragma unroll
      for (int j = 0; j < h; ++j) *reinterpret_cast<ull2*>(layer + (size_t)j * dist + 2 * i) = ull2{oa[h + j], ob[h + j]};
    }
  }
}

// Layers m-1 .. 0 from layer m = src (2^m words, 1 <= m <= kGpTailLog): one block
template <class F>
__global__ void __launch_bounds__(kBlock) gp_tree_tail_kernel(F f, const u64* __restrict__ src, u64* __restrict__ tree, int m) {
  __shared__ u64 v[1 << kGpTailLog];
  const int n = 1 << m;
  for (int x = threadIdx.x; x < n; x += kBlock) v[x] = src[x];
  __syncthreads();
  for (int k = m - 1; k >= 0; --k) {
    const int half = 1 << k;
    // thread x reads v[x] and v[x + half] and writes v[x]: nobody else touches either this level
    for (int x = threadIdx.x; x < half; x += kBlock) {
      const u64 y = f.mul(v[x], v[x + half]);
      v[x] = y;
      tree[half + x] = y;
    }
    __syncthreads();
  }
}

// One round of the cubic sumcheck over tables T[0..2] = E, L, R.  FOLD: the tables have 4 n_units entries; unit i folds entries
// 4i .. 4i+3 of each by r into entries 2i, 2i+1 of out[.] and adds them to H(0..3).  Otherwise: 2 n_units entries, nothing stored.
struct GpTables {
  const u64* in[3];
  u64* out[3];
};
template <class F, bool FOLD>
__global__ void __launch_bounds__(kBlock) gp_pass_kernel(F f, GpTables tb, u64 r, size_t n_units, PassOut out) {
  __shared__ u64 lds[(kBlock / kWave) * 4];
  __shared__ int lds_flag;
  typename F::Acc acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) f.acc_zero(acc[s]);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 p[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
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
    gp_accumulate(f, acc, p[0], p[1], p[2]);
  }
  const u64 mine = reduce_cells<F, 4>(f, acc, lds);
  finish_pass<F, 4>(f, out, mine, &lds_flag);
}

// out[i] = alpha t[i] + beta over n_pairs pairs of words
template <class F>
__global__ void __launch_bounds__(kBlock) table_affine_kernel(F f, const u64* __restrict__ t, u64 alpha, u64 beta, size_t n_pairs, u64* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_pairs; i += (size_t)gridDim.x * kBlock) {
    const ull2 x = reinterpret_cast<const ull2*>(t)[i];
    reinterpret_cast<ull2*>(out)[i] = ull2{f.add(f.mul(alpha, x.x), beta), f.add(f.mul(alpha, x.y), beta)};
  }
}

#endif   // __HIPCC__

}  // namespace sc
