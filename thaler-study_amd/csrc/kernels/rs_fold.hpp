// Folded openings of the Ligero-style commitment (ligero.hpp's contract): instead of sending the two
// combined rows of an opening (2^c words each), the prover proves what the verifier needs of them by the interleaved sumcheck
// and codeword folding of Basefold, over the Reed-Solomon code and the column tree the commitment already has.
//
// Shape      The commitment is an sc_ligero with SC_CODE_RS: R = 2^r rows, C = 2^c columns, n = r + c, 1 <= c, L = 2^l0,
//            l0 = c + rho, E[i][j] as in ligero.hpp.  w_l is the contract's root of order 2^l: w_l = w_max^(2^(s-l)).
// Opening    at z, z_lo = z[:c], z_hi = z[c:]; every word a Montgomery word.
//            1. the root.                           2. V sends gamma in F^R.
//            3. P sends v = u_z(z_lo) and v_gamma = u_gamma(z_lo) (u_z = sum_i eq(z_hi, i) row_i, u_gamma = sum_i gamma_i row_i,
//               the multilinear extension LE).      4. V sends beta.
//            5. w_i = eq(z_hi, i) + beta gamma_i; m = sum_i w_i row_i = u_z + beta u_gamma; U_0 = Enc(m) = sum_i w_i E[i][.], L
//               words, never committed: V recomputes its entries from opened columns.  Claim s = v + beta v_gamma =
//               sum_b m[b] eq(z_lo, b).
//            6. round i = 0 .. c-1: P sends (H(0), H(1), H(2)) of the product sumcheck over (m, eq(z_lo)) - sc_prover_round's -
//               and, for i >= 1, root_i of the tree over U_i; V checks H(0) + H(1) against the running claim and sends alpha_i;
//               P folds U_i (M = 2^(l0-i) words) into U_(i+1) (M / 2 words): for j < M / 2, x = w_(l0-i)^j,
//                 even = (U_i[j] + U_i[j + M/2]) / 2,  odd = (U_i[j] - U_i[j + M/2]) / (2 x),
//                 U_(i+1)[j] = even + alpha_i (odd - even)
//               which is the codeword of fix_variables(m_i, [alpha_i]) at half the length, in natural order again.
//            7. P sends the final value: U_c is 2^rho equal words.  V checks H_(c-1)(alpha_(c-1)) = final eq(z_lo, alpha).
//            8. V draws `queries` indices q in [0, L / 2), with replacement.
//            9. per query P opens the columns q and q + L / 2 (sc_ligero_open_columns, unchanged) and, for every layer
//               i = 1 .. c-1, leaf j_i = q mod 2^(l0-i-1) of its tree: two words and a path of l0 - i - 1 digests.
//            10. per query V checks both column paths; U_0[q] = sum_i w_i col_q[i] and the same at q + L / 2; that folding
//               layer i's pair with alpha_i at x = w_(l0-i)^(j_i) gives the word of layer i+1's pair at position j_i (the low
//               word if j_i < 2^(l0-i-2), else the high one); every layer path; that the last fold is the final value.  V
//               returns v.
// Tree       of layer i (1 <= i <= c-1): M / 2 leaves, leaf j = SHA-256(le64(canon U_i[j]) || le64(canon U_i[j + M/2])) - the
//            column leaf of U_i read as a 2 x M/2 row-major matrix; nodes and paths as sc_merkle_*'s.
// Limits     those of the commitment; the expander code does not fold.  No security level is claimed.
//
// rs_fold_kernel does one fold and, where the next layer gets a tree, its leaves, in one launch: the thread of j < M / 4 loads
// U[j], U[j + M/4], U[j + M/2], U[j + 3M/4] - the pairs of j and of j + M/4 - writes U'[j] and U'[j + M/4] and hashes them, which
// is leaf j of U', straight into the bottom stored level of a MerkleLevels block: the folded codeword is not read again for its
// tree.  Every access is one word per lane at consecutive addresses.  With h = 1/2 the fold is
//   U'[j] = (a + b) h (1 - alpha) + (a - b) h alpha / x
// three products per word, h (1 - alpha) and h alpha from the host.  1 / x = w_(l0-i)^(-j) = w_l0^(L - j 2^i): one table set of
// the layer-0 length serves every layer - the twist tables of ligero_long.hpp (lo[e mod 2^12] hi[e >> 12], two loads and a
// product) from l0 = 12 on, below it the context's table of w_l0^e, e < L / 2, through w^(L - e) = -w^(L/2 - e) (one load).
// The second pair's 1 / x is the first's times w_M^(-M/4), the inverse fourth root, a kernel argument.
// The per-item arithmetic compiles for the host, where tests/cpp/rs_fold_host_harness.cpp replays it.
//
// Staged openings: up to three variables folded between two committed layers.
// Schedule   a_0 .. a_(S-1), 1 <= a_s <= 3, sum a_s = c.  Stage s starts at round i_s = a_0 + .. + a_(s-1) and owns the layer
//            U_(i_s) of M_s = 2^(l0 - i_s) words; the layers between two stage starts exist nowhere.  All ones: the opening above.
// Tree       of stage s >= 1: M_s / 2^(a_s) leaves, leaf j = SHA-256(le64(canon U[j]) || le64(canon U[j + M_s/2^a_s]) || .. ||
//            le64(canon U[j + (2^a_s - 1) M_s/2^a_s])) - the column leaf of U read as a 2^(a_s) x M_s/2^(a_s) row-major matrix.
// Rounds     the c sumcheck rounds as above; round i's message carries root_s exactly when i = i_s, s >= 1.  After
//            alpha_(i_s + a_s - 1) P folds U_(i_s) by the a_s challenges of the stage: a_s successive folds of step 6, bit for
//            bit.  Word j of the result depends on the 2^(a_s) words of leaf j alone: level l of the stage folds the words
//            t and t + 2^(a_s-1-l) of the leaf, t < 2^(a_s-1-l), at x = (w_(l0-i_s)^(j + t M_s/2^a_s))^(2^l).
// Final      U_c is 2^rho equal words; the last-round check is step 7's.
// Queries    V draws q in [0, L / 2^(a_0)); P opens the 2^(a_0) columns q + t L/2^(a_0) and, for every stage s >= 1, leaf
//            j_s = q mod (M_s / 2^(a_s)): 2^(a_s) words and a path of l0 - i_s - a_s digests.  V checks the column paths; U_0 at
//            the opened columns; that folding stage s's words gives word number floor(j_s / (M_(s+1) / 2^(a_(s+1)))) of stage
//            s+1's leaf; that the last stage gives the final value; every path.
// Nothing is claimed about soundness, and the number of queries an arity needs is not analysed.
//
// rs_fold_many_kernel<F, A, AN> folds A variables and, for AN >= 1, hashes the leaves of the next stage's tree (arity AN) in the
// same launch: the thread of leaf j' < M' / 2^AN (M' = M / 2^A) produces that leaf's 2^AN words one after the other, each from 2^A
// loads at stride M', stores it and puts it into the SHA-256 block - never more than 2^A words and one block are live; AN = 3
// is one full block and the padding block.  AN = 0: no tree, one word per thread.  1 / x of the leaf's word 0 comes from the
// same layer-0 tables (rs_fold_xinv); word t' has it times eta[t'] = w_M^(-t' M'/2^AN), and within a word the sub-position t of
// level l times zeta^(t 2^l), zeta = w_M^(-M'): the host folds these into the level's constant (c1z), so a pair costs three
// products as above.  tests/cpp/rs_fold_many_host_harness.cpp replays the item on the host.
#pragma once
#include "ligero_long.hpp"
#include "sha256.hpp"

namespace sc {

constexpr int kRsFoldTwistMinLog = kRsTwistLoLog;   // layer-0 lengths from 2^this on read the twist tables

struct RsFoldTables {
  const u64* lo;   // l0 >= kRsFoldTwistMinLog: the twist tables of length 2^l0; below: lo[e] = w_l0^e, e < L / 2, and hi is null
  const u64* hi;
  int log_len0;    // l0
  int shift;       // the layer: M = 2^(l0 - shift), w_M = w_l0^(2^shift)
};

struct RsFoldArgs : RsFoldTables {
  u64 c0, c1;      // (1 - alpha) / 2, alpha / 2
  u64 inv_w4;      // w_M^(-M/4): the inverse of the fourth root of unity
};

struct RsFoldManyArgs : RsFoldTables {
  u64 c0[3];       // level l: (1 - alpha_l) / 2
  u64 c1z[7];      // level l, sub-position t < 2^(A-1-l), at [2^A - 2^(A-l) + t]: alpha_l / 2 * zeta^(t 2^l), zeta = w_M^(-M/2^A)
  u64 eta[8];      // eta[t'] = w_M^(-t' M / 2^(A+AN)): 1 / x of word t' of an output leaf over that of its word 0
};

// e with 1 / x = w_l0^e for x = w_M^j, j < M / 2
SC_HD u32 rs_fold_exp(int log_len0, int shift, u32 j) { return ((1u << log_len0) - (j << shift)) & ((1u << log_len0) - 1); }

template <class F>
SC_HD u64 rs_fold_xinv(const F& f, const RsFoldTables& a, u32 j) {
  const u32 e = rs_fold_exp(a.log_len0, a.shift, j);
  if (a.hi) return f.mul(a.lo[e & ((1u << kRsTwistLoLog) - 1)], a.hi[e >> kRsTwistLoLog]);
  // e = 0 or L / 2 < e < L: w^e = -w^(e - L/2)
  return e ? f.sub(0, a.lo[e - (1u << (a.log_len0 - 1))]) : f.one();
}

// one fold of the pair (a, b) = (U[j], U[j + M/2]); xinv = 1 / x
template <class F>
SC_HD u64 rs_fold_pair(const F& f, const RsFoldArgs& k, u64 xinv, u64 a, u64 b) {
  return f.add(f.mul(f.add(a, b), k.c0), f.mul(f.sub(a, b), f.mul(k.c1, xinv)));
}

// the item of j < M / 4: u = U[j], U[j + M/4], U[j + M/2], U[j + 3M/4]; o = U'[j], U'[j + M/4]
template <class F>
SC_HD void rs_fold_item(const F& f, const RsFoldArgs& k, u32 j, const u64 (&u)[4], u64 (&o)[2]) {
  const u64 xinv = rs_fold_xinv(f, k, j);
  o[0] = rs_fold_pair(f, k, xinv, u[0], u[2]);
  o[1] = rs_fold_pair(f, k, f.mul(xinv, k.inv_w4), u[1], u[3]);
}

// leaf j of U': SHA-256 over the 16 bytes le64(canon o[0]) || le64(canon o[1]), one block with its padding
template <class F>
SC_HD void rs_fold_leaf(const F& f, const u64 (&o)[2], u32 (&d)[8]) {
  const u64 lo = f.from_mont(o[0]), hi = f.from_mont(o[1]);
  const u32 blk[16] = {__builtin_bswap32((u32)lo), __builtin_bswap32((u32)(lo >> 32)), __builtin_bswap32((u32)hi),
                       __builtin_bswap32((u32)(hi >> 32)), 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 128u};
  sha256_init(d);
  sha256_compress(d, blk);
}

// A successive folds of the 2^A words u[t] = U[j + t M/2^A] in place; xinv = 1 / x of j at the first level.  Returns the word
template <int A, class F>
SC_HD u64 rs_fold_many_word(const F& f, const RsFoldManyArgs& k, u64 xinv, u64 (&u)[1 << A]) {
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

// the item of output leaf j < leaves = M' / 2^AN, M' = M / 2^A: out[j + t' leaves], t' < 2^AN, each from U[j + t' leaves + t M'],
// t < 2^A; for AN >= 1, d = SHA-256 over the 8 * 2^AN bytes le64(canon out[j]) || le64(canon out[j + leaves]) || ..
template <int A, int AN, class F>
SC_HD void rs_fold_many_item(const F& f, const RsFoldManyArgs& k, u32 j, u32 leaves, const u64* __restrict__ U, u64* __restrict__ out,
                             u32 (&d)[8]) {
  const u64 xinv = rs_fold_xinv(f, k, j);
  const u64 stride = (u64)leaves << AN;
  u32 blk[16];
#pragma unroll
  for (int w = 0; w < (1 << AN); ++w) {
    const u64 jo = j + (u64)w * leaves;
    u64 u[1 << A];
#pragma unroll
    for (int t = 0; t < (1 << A); ++t) u[t] = U[jo + t * stride];
    const u64 o = rs_fold_many_word<A>(f, k, w ? f.mul(xinv, k.eta[w]) : xinv, u);
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

// out = the fold of U (4 `quarter` words); kHash: leaves[j] = the digest of leaf j of out, j < quarter
template <class F, bool kHash>
__global__ __launch_bounds__(kBlock) void rs_fold_kernel(F f, const u64* __restrict__ U, u64* __restrict__ out, RsFoldArgs a, u32 quarter,
                                                         u32* __restrict__ leaves) {
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < quarter; j += gridDim.x * blockDim.x) {
    const u64 u[4] = {U[j], U[j + quarter], U[j + 2 * (u64)quarter], U[j + 3 * (u64)quarter]};
    u64 o[2];
    rs_fold_item(f, a, j, u, o);
    out[j] = o[0];
    out[j + quarter] = o[1];
    if constexpr (kHash) {
      u32 d[8];
      rs_fold_leaf(f, o, d);
      st_digest(leaves + 8 * (u64)j, d);
    }
  }
}

// out = U (2^(A+AN) `leaves` words) folded A times; AN >= 1: digests[j] = the digest of leaf j of out, j < leaves
template <class F, int A, int AN>
__global__ __launch_bounds__(kBlock) void rs_fold_many_kernel(F f, const u64* __restrict__ U, u64* __restrict__ out, RsFoldManyArgs a,
                                                              u32 leaves, u32* __restrict__ digests) {
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < leaves; j += gridDim.x * blockDim.x) {
    u32 d[8];
    rs_fold_many_item<A, AN>(f, a, j, leaves, U, out, d);
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
