// Folded openings of the Ligero-style commitment (ligero.hpp's contract): instead of sending
// the two combined rows of an opening (2^c words each), the prover proves what the verifier needs of them by the interleaved
// sumcheck and codeword folding of Basefold, over the Reed-Solomon code and the column tree the commitment already has, folding
// up to three variables between two committed layers.  A schedule of ones (a_s = 1 everywhere) is the binary opening:
// sc_ligero_fold_begin's, one committed layer per variable.
//
// Shape      The commitment is an sc_ligero with SC_CODE_RS: R = 2^r rows, C = 2^c columns, n = r + c, 1 <= c, L = 2^l0,
//            l0 = c + rho, E[i][j] as in ligero.hpp.  w_l is the contract's root of order 2^l: w_l = w_max^(2^(s-l)).
// Schedule   a_0 .. a_(S-1), 1 <= a_s <= 3, sum a_s = c.  Stage s starts at round i_s = a_0 + .. + a_(s-1) and owns the layer
//            U_(i_s) of M_s = 2^(l0 - i_s) words; the layers between two stage starts exist nowhere.
// Opening    at z, z_lo = z[:c], z_hi = z[c:]; every word a Montgomery word.
//            1. the root.                           2. V sends gamma in F^R.
//            3. P sends v = u_z(z_lo) and v_gamma = u_gamma(z_lo) (u_z = sum_i eq(z_hi, i) row_i, u_gamma = sum_i gamma_i row_i,
//               the multilinear extension LE).      4. V sends beta.
//            5. w_i = eq(z_hi, i) + beta gamma_i; m = sum_i w_i row_i = u_z + beta u_gamma; U_0 = Enc(m) = sum_i w_i E[i][.], L
//               words, never committed: V recomputes its entries from opened columns.  Claim s = v + beta v_gamma =
//               sum_b m[b] eq(z_lo, b).
// Fold       of U_i (M = 2^(l0-i) words) with alpha_i into U_(i+1) (M / 2 words): for j < M / 2, x = w_(l0-i)^j,
//                 even = (U_i[j] + U_i[j + M/2]) / 2,  odd = (U_i[j] - U_i[j + M/2]) / (2 x),
//                 U_(i+1)[j] = even + alpha_i (odd - even)
//            which is the codeword of fix_variables(m_i, [alpha_i]) at half the length, in natural order again.
// Rounds     i = 0 .. c-1: P sends (H(0), H(1), H(2)) of the product sumcheck over (m, eq(z_lo)) - sc_prover_round's - and, exactly
//            when i = i_s, s >= 1, root_s of the tree over U_(i_s); V checks H(0) + H(1) against the running claim and sends
//            alpha_i.  After alpha_(i_s + a_s - 1) P folds U_(i_s) by the a_s challenges of the stage: a_s successive folds, bit
//            for bit.  Word j of the result depends on the 2^(a_s) words of leaf j alone: level l of the stage folds the words t
//            and t + 2^(a_s-1-l) of the leaf, t < 2^(a_s-1-l), at x = (w_(l0-i_s)^(j + t M_s/2^a_s))^(2^l).
// Final      P sends the final value: U_c is 2^rho equal words.  V checks H_(c-1)(alpha_(c-1)) = final eq(z_lo, alpha).
// Tree       of stage s >= 1: M_s / 2^(a_s) leaves, leaf j = SHA-256(le64(canon U[j]) || le64(canon U[j + M_s/2^a_s]) || .. ||
//            le64(canon U[j + (2^a_s - 1) M_s/2^a_s])) - the column leaf of U read as a 2^(a_s) x M_s/2^(a_s) row-major matrix;
//            nodes and paths as sc_merkle_*'s.
// Queries    V draws `queries` indices q in [0, L / 2^(a_0)), with replacement; per query P opens the 2^(a_0) columns
//            q + t L/2^(a_0) (sc_ligero_open_columns, unchanged) and, for every stage s >= 1, leaf j_s = q mod (M_s / 2^(a_s)):
//            2^(a_s) words and a path of l0 - i_s - a_s digests.  V checks the column paths; U_0[q'] = sum_i w_i col_q'[i] at
//            the opened columns; that folding stage s's words gives word number floor(j_s / (M_(s+1) / 2^(a_(s+1)))) of stage
//            s+1's leaf; that the last stage gives the final value; every path.  V returns v.
// All ones   every layer U_1 .. U_(c-1) is committed, a leaf is the pair (U_i[j], U_i[j + M/2]), a query opens the columns q
//            and q + L / 2 and per layer two words and l0 - i - 1 digests, and the fold of layer i's pair is the low word of
//            layer i+1's pair if j_i < 2^(l0-i-2), else the high one.
// Limits     those of the commitment; the expander code does not fold.  No security level is claimed, nothing is
//            claimed about soundness, and the number of queries an arity needs is not analysed.
//
// rs_fold_kernel<F, A, AN> folds A variables and, for AN >= 1, hashes the leaves of the next stage's tree (arity AN) in the same
// launch, straight into the bottom stored level of a MerkleLevels block: the folded codeword is not read again for its tree.
// The thread of leaf j' < M' / 2^AN (M' = M / 2^A) produces that leaf's 2^AN words one after the other, each from 2^A loads at
// stride M', stores it and puts it into the SHA-256 block - never more than 2^A words and one block are live; AN = 3 is one
// full block and the padding block.  AN = 0: no tree, and the thread produces two words as for AN = 1, without the hash (one
// word per thread was 4 - 9 % slower at M = 2^24); so M' >= 2, which every caller has.  Every access is one word per lane at
// consecutive addresses.  With h = 1/2 one fold of a pair is
//   U'[j] = (a + b) h (1 - alpha) + (a - b) h alpha / x
// three products, h (1 - alpha) and h alpha from the host.  1 / x = w_(l0-i)^(-j) = w_l0^(L - j 2^i): one table set of the
// layer-0 length serves every layer - the twist tables of ligero_long.hpp (lo[e mod 2^12] hi[e >> 12], two loads and a
// product) from l0 = 12 on, below it the context's table of w_l0^e, e < L / 2, through w^(L - e) = -w^(L/2 - e) (one load).
// That is 1 / x of the leaf's word 0 (rs_fold_xinv); word t' has it times eta[t'] = w_M^(-t' M'/2^AN), and within a word the
// sub-position t of level l times zeta^(t 2^l), zeta = w_M^(-M'): rs_fold_constants folds these into the level's constant
// (c1z).  The per-item code and rs_fold_constants compile for the host, where tests/cpp/rs_fold_host_harness.cpp replays them.
#pragma once
#include "ligero_long.hpp"
#include "sha256.hpp"

namespace sc {

constexpr int kRsFoldTwistMinLog = kRsTwistLoLog;   // layer-0 lengths from 2^this on read the twist tables

struct RsFoldArgs {
  const u64* lo;   // l0 >= kRsFoldTwistMinLog: the twist tables of length 2^l0; below: lo[e] = w_l0^e, e < L / 2, and hi is null
  const u64* hi;
  int log_len0;    // l0
  int shift;       // the layer: M = 2^(l0 - shift), w_M = w_l0^(2^shift)
  u64 c0[3];       // level l: (1 - alpha_l) / 2
  u64 c1z[7];      // level l, sub-position t < 2^(A-1-l), at [2^A - 2^(A-l) + t]: alpha_l / 2 * zeta^(t 2^l), zeta = w_M^(-M/2^A)
  u64 eta[8];      // eta[t'] = w_M^(-t' M / 2^(A+W)): 1 / x of word t' of an item over that of its word 0
};

// W: an item - a thread's work - is 2^W output words: the leaf of 2^AN words, and two words where there is no tree
constexpr int rs_fold_item_log(int an) { return an ? an : 1; }

// c0, c1z and eta of a launch that folds with alphas[0 .. a) in items of 2^w words.  f: mul, sub and one on Montgomery words
// (host only); half = 1 / 2, zeta = w_M^(-M/2^a) and eta = w_M^(-M/2^(a+w)): roots of order 2^a and 2^(a+w), whatever M
template <class F>
void rs_fold_constants(const F& f, u64 half, u64 zeta, u64 eta, const u64* alphas, int a, int w, RsFoldArgs* k) {
  for (int l = 0; l < a; ++l, zeta = f.mul(zeta, zeta)) {
    const u64 c1 = f.mul(half, alphas[l]);
    k->c0[l] = f.sub(half, c1);
    u64 z = f.one();
    for (int t = 0; t < 1 << (a - 1 - l); ++t, z = f.mul(z, zeta)) k->c1z[(1 << a) - (1 << (a - l)) + t] = f.mul(c1, z);
  }
  k->eta[0] = f.one();
  for (int t = 1; t < 1 << w; ++t) k->eta[t] = f.mul(k->eta[t - 1], eta);
}

// e with 1 / x = w_l0^e for x = w_M^j, j < M / 2
SC_HD u32 rs_fold_exp(int log_len0, int shift, u32 j) { return ((1u << log_len0) - (j << shift)) & ((1u << log_len0) - 1); }

template <class F>
SC_HD u64 rs_fold_xinv(const F& f, const RsFoldArgs& a, u32 j) {
  const u32 e = rs_fold_exp(a.log_len0, a.shift, j);
  if (a.hi) return f.mul(a.lo[e & ((1u << kRsTwistLoLog) - 1)], a.hi[e >> kRsTwistLoLog]);
  // e = 0 or L / 2 < e < L: w^e = -w^(e - L/2)
  return e ? f.sub(0, a.lo[e - (1u << (a.log_len0 - 1))]) : f.one();
}

// A successive folds of the 2^A words u[t] = U[j + t M/2^A] in place; xinv = 1 / x of j at the first level.  Returns the word
template <int A, class F>
SC_HD u64 rs_fold_word(const F& f, const RsFoldArgs& k, u64 xinv, u64 (&u)[1 << A]) {
#pragma unroll
  for (int l = 0; l < A; ++l) {
    const int half = 1 << (A - 1 - l), at = (1 << A) - (1 << (A - l));
#pragma unroll
    for (int t = 0; t < half; ++t)
      u[t] = f.add(f.mul(f.add(u[t], u[t + half]), k.c0[l]), f.mul(f.sub(u[t], u[t + half]), f.mul(k.c1z[at + t], xinv)));
    if (l + 1 < A) xinv = f.mul(xinv, xinv);
  }
  return u[0];
}

// the item j < items = M' / 2^W, M' = M / 2^A, W = rs_fold_item_log(AN): out[j + t' items], t' < 2^W, each from
// U[j + t' items + t M'], t < 2^A; for AN >= 1 the item is output leaf j and d = SHA-256 over the 8 * 2^AN bytes
// le64(canon out[j]) || le64(canon out[j + items]) || ..
template <int A, int AN, class F>
SC_HD void rs_fold_item(const F& f, const RsFoldArgs& k, u32 j, u32 items, const u64* __restrict__ U, u64* __restrict__ out, u32 (&d)[8]) {
  constexpr int W = rs_fold_item_log(AN);
  const u64 xinv = rs_fold_xinv(f, k, j);
  const u64 stride = (u64)items << W;
  u32 blk[16];
#pragma unroll
  for (int w = 0; w < (1 << W); ++w) {
    const u64 jo = j + (u64)w * items;
    u64 u[1 << A];
#pragma unroll
    for (int t = 0; t < (1 << A); ++t) u[t] = U[jo + t * stride];
    const u64 o = rs_fold_word<A>(f, k, w ? f.mul(xinv, k.eta[w]) : xinv, u);
    out[jo] = o;
    if constexpr (AN > 0) {
      const u64 v = f.from_mont(o);
      blk[2 * w] = __builtin_bswap32((u32)v);
      blk[2 * w + 1] = __builtin_bswap32((u32)(v >> 32));
    }
  }
  if constexpr (AN > 0) {
    sha256_init(d);
    if constexpr (AN == 3) {
      sha256_compress(d, blk);
      sha256_compress_pad64(d);
    } else {
#pragma unroll
      for (int i = (2 << AN); i < 16; ++i) blk[i] = 0;
      blk[2 << AN] = 0x80000000u;
      blk[15] = 64u << AN;
      sha256_compress(d, blk);
    }
  }
}

}  // namespace sc

#if defined(__HIPCC__)
namespace sc {

// out = U (2^(A+W) `items` words, W = rs_fold_item_log(AN)) folded A times; AN >= 1: digests[j] = the digest of leaf j of out, j < items
template <class F, int A, int AN>
__global__ __launch_bounds__(kBlock) void rs_fold_kernel(F f, const u64* __restrict__ U, u64* __restrict__ out, RsFoldArgs a, u32 items,
                                                         u32* __restrict__ digests) {
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < items; j += gridDim.x * blockDim.x) {
    u32 d[8];
    rs_fold_item<A, AN>(f, a, j, items, U, out, d);
    if constexpr (AN > 0) st_digest(digests + 8 * (u64)j, d);
  }
}

// m = a + beta b, the row the folded opening proves about
template <class F>
__global__ __launch_bounds__(kBlock) void rs_fold_mix_kernel(F f, const u64* __restrict__ a, const u64* __restrict__ b, u64 beta, u32 len,
                                                             u64* __restrict__ m) {
  for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < len; k += gridDim.x * blockDim.x) m[k] = f.add(a[k], f.mul(beta, b[k]));
}

}  // namespace sc
#endif
