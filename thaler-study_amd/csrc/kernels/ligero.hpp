// Ligero-style polynomial commitment (Thaler, "Proofs, Arguments, and Zero-Knowledge", section 10.5; the reference has no such
// crate): the table as a matrix, its rows Reed-Solomon encoded, the columns of the codeword matrix Merkle-hashed.
//
// Shape      A table w of 2^n entries, LE (index bit j = variable j), is R = 2^r rows by C = 2^c columns, n = r + c: row i is
//            w[i C .. (i+1) C); variables 0..c-1 select the column, c..n-1 the row.
// Encoding   log_blowup rho in {1, 2}, codeword length L = 2^(c+rho).  Row i is the coefficient vector of a polynomial of
//            degree < C, evaluated at the powers of w_L in natural order: E[i][j] = sum_{k<C} w[i C + k] w_L^(j k), j < L.
//            E is row-major (E[i][j] at i L + j), an ordinary table of 2^(n+rho) Montgomery words.
// Root       s = the 2-adicity of p - 1; g = the smallest integer >= 2 with g^((p-1)/2) = -1; w_max = g^((p-1)/2^s);
//            w_L = w_max^(2^(s-c-rho)).  Derived on the host from the context's modulus, never passed in.
//            (Goldilocks: s = 32, g = 7, w_max = 1753635133440165772; 2013265921: 27, 11, 1227303670; 65537: 16, 3, 3; 257: 8, 3, 3.)
// Limits     c + rho <= 14 (one codeword row, 128 KiB, in the LDS of a CU) for sc_rs_encode_rows / sc_ligero_commit, c + rho <= 24 for
//            their _long forms, which run this file's kernel up to 14 and the two launches of ligero_long.hpp above (at 2^24 the
//            stored tree is 1 GiB); n + rho <= 29; c + rho <= s; one device, one rank.
// Digest     Leaf j = SHA-256 of the R 8 bytes le64(canon E[0][j]) || .. || le64(canon E[R-1][j]), standard padding (R = 1:
//            sha256_leaf); nodes are sha256_node; L leaves, every level kept (64 L bytes: 1 MiB at L = 2^14); paths bottom up, bytes as
//            sc_merkle_open's.
//
// rs_encode_rows_kernel is a decimation-in-TIME transform: the bit reversal happens on the way IN.  Coefficient k of a row goes
// to LDS position bitrev_c(k) 2^rho, which is bitrev_(c+rho)(k) (the high coefficients are zero); the butterfly levels then run
// with half-sizes 1, 2, .., L/2 and leave the L evaluations in natural order, so the stores are one coalesced run.  The first
// rho levels only meet the zero fill - a butterfly (a, 0) gives (a, a) whatever its twiddle - so instead of zero-filling and
// running them, the load writes every coefficient to the 2^rho consecutive positions those levels would copy it to and the
// levels start at half-size 2^rho: c levels over L words instead of c + rho.  The c levels are done four at a time in
// registers (radix 16: sixteen words at stride h, 32 butterflies, one LDS read and one write per word), a last pass taking
// the 1..3 levels left over.  Twiddles: level s of a pass needs w_L^((j + low h) L / (2 h 2^s)) = base_s * W16^(low 2^(3-s)),
// base_s = w_L^(j L / (2 h 2^s)) from the context's table of w_L powers (one load per level) and the eight powers of
// W16 = w_L^(L/16) from the kernel arguments (eleven products per sixteen words).
//
// LDS image: word i lives at i + 2 (i >> 5) (two words of padding per 32).  In the first pass (h = 2^rho) a wave's lanes are
// (group, j) with the groups 16 h words apart: padded, 32 lanes of a half fall on 2^rho g + j mod 32, all different; in every
// later pass h >= 32 and the lanes read consecutive words.  The padding is even, so the final 16-byte reads stay aligned.
#pragma once
#include "merkle.hpp"
#include "row_code.hpp"

namespace sc {

constexpr int kRsMaxLog = 14;        // c + rho at most: L = 2^14 words in LDS
constexpr int kRsMaxThreads = 1024;     // Goldilocks: four waves per SIMD hide the LDS round trips
constexpr int kRsMaxThreadsGeneric = 512;   // the generic field's products need more than the 128 registers of that shape
constexpr int kLigeroMaxCombine = 4;

struct RsRoots {
  u64 w16[8];   // W16^k, Montgomery (entries whose order the field lacks are never read)
};

SC_HD size_t rs_lds_words(int tile_log) { return ((size_t)1 << tile_log) + ((size_t)2 << tile_log >> 5) + 2; }
template <class F>
constexpr int rs_max_threads() {
  return std::is_same<F, GoldilocksMont>::value ? kRsMaxThreads : kRsMaxThreadsGeneric;
}
inline int rs_threads(int tile_log, int max_threads) {
  const int t = 1 << (tile_log > 4 ? tile_log - 4 : 0);
  return t < kWave ? kWave : (t > max_threads ? max_threads : t);
}

}  // namespace sc

#if defined(__HIPCC__)
namespace sc {

__device__ __forceinline__ u32 rs_slot(u32 i) { return i + ((i >> 5) << 1); }

// Q levels (half-sizes h .. h 2^(Q-1), h = 2^hlog) over the block's tile of 2^tile_log words, in place: every butterfly set of
// 2^Q words at stride h belongs to one thread, so passes need a barrier between them and nothing inside.
template <class F, int Q>
__device__ __forceinline__ void rs_radix_pass(const F& f, u64* __restrict__ lds, const u64* __restrict__ tw, const RsRoots& roots,
                                              int hlog, int log_len, int tile_log) {
  constexpr int N = 1 << Q;
  const u32 sets = 1u << (tile_log - Q), hmask = (1u << hlog) - 1;
  for (u32 b = threadIdx.x; b < sets; b += blockDim.x) {
    const u32 j = b & hmask, base = ((b >> hlog) << (hlog + Q)) + j;
    u64 v[N];
#pragma unroll
    for (int t = 0; t < N; ++t) v[t] = lds[rs_slot(base + ((u32)t << hlog))];
#pragma unroll
    for (int s = 0; s < Q; ++s) {
      const u64 base_tw = tw[(size_t)j << (log_len - 1 - hlog - s)];
#pragma unroll
      for (int low = 0; low < (1 << s); ++low) {
        const u64 w = low == 0 ? base_tw : f.mul(base_tw, roots.w16[(low << (3 - s)) & 7]);
#pragma unroll
        for (int m = 0; m < (N >> (s + 1)); ++m) {
          const int t = low + (m << (s + 1));
          const u64 a = v[t], x = f.mul(v[t + (1 << s)], w);
          v[t] = f.add(a, x);
          v[t + (1 << s)] = f.sub(a, x);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < N; ++t) lds[rs_slot(base + ((u32)t << hlog))] = v[t];
  }
}

// One block encodes 2^(tile_log - c - rho) consecutive rows: their coefficients are one contiguous run of w, their codewords
// one contiguous run of E.  vec: both runs are 16-byte aligned and at least two words long.
template <class F>
__global__ __launch_bounds__(rs_max_threads<F>()) void rs_encode_rows_kernel(F f, const u64* __restrict__ w, u64* __restrict__ E,
                                                                       const u64* __restrict__ tw, RsRoots roots, int c, int rho,
                                                                       int tile_log, int vec) {
  extern __shared__ __attribute__((aligned(16))) u64 rs_lds[];
  u64* lds = rs_lds;
  const int log_len = c + rho;
  const u32 in_words = 1u << (tile_log - rho), cmask = (1u << c) - 1;
  const u64* src = w + (u64)blockIdx.x * in_words;
  u64* dst = E + ((u64)blockIdx.x << tile_log);
  // in: coefficient k of local row q -> positions q L + bitrev_c(k) 2^rho + (0 .. 2^rho - 1)
  auto place = [&](u32 e, u64 x) {
    const u32 k = e & cmask;
    const u32 pos = ((e >> c) << log_len) + ((c ? (__brev(k) >> (32 - c)) : 0u) << rho);
    for (int t = 0; t < (1 << rho); ++t) lds[rs_slot(pos + t)] = x;
  };
  if (vec) {
    for (u32 q = threadIdx.x; q < in_words / 2; q += blockDim.x) {
      const ull2 x = *reinterpret_cast<const ull2*>(src + 2 * q);
      place(2 * q, x.x);
      place(2 * q + 1, x.y);
    }
  } else {
    for (u32 e = threadIdx.x; e < in_words; e += blockDim.x) place(e, src[e]);
  }
  __syncthreads();
  int hlog = rho, left = c;
  for (; left >= 4; left -= 4, hlog += 4) {
    rs_radix_pass<F, 4>(f, lds, tw, roots, hlog, log_len, tile_log);
    __syncthreads();
  }
  if (left == 3) rs_radix_pass<F, 3>(f, lds, tw, roots, hlog, log_len, tile_log);
  else if (left == 2) rs_radix_pass<F, 2>(f, lds, tw, roots, hlog, log_len, tile_log);
  else if (left == 1) rs_radix_pass<F, 1>(f, lds, tw, roots, hlog, log_len, tile_log);
  if (left) __syncthreads();
  // out: natural order, two words per lane (slots of an even word and its successor are adjacent and 16-byte aligned)
  const u32 out_words = 1u << tile_log;
  if (vec) {
    for (u32 q = threadIdx.x; q < out_words / 2; q += blockDim.x)
      *reinterpret_cast<ull2*>(dst + 2 * q) = *reinterpret_cast<const ull2*>(lds + rs_slot(2 * q));
  } else {
    for (u32 e = threadIdx.x; e < out_words; e += blockDim.x) dst[e] = lds[rs_slot(e)];
  }
}

// Leaf j of the commitment: SHA-256 over column j of E (canonical values, 8 little-endian bytes each), one lane per column.  For
// a fixed row the lanes of a wave read 64 consecutive words.  Eight rows fill one 64-byte block, with compile-time indices;
// R < 8 rows (8, 16, 32 bytes) share their block with the padding, R >= 8 is R / 8 data blocks and a padding block.
template <class F>
__global__ __launch_bounds__(kBlock) void column_leaf_kernel(F f, const u64* __restrict__ E, u32 rows, u32 len, u32* __restrict__ out) {
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < len; j += gridDim.x * blockDim.x) {
    u32 st[8], blk[16];
    sha256_init(st);
    if (rows < 8) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u64 v = 0;
        if ((u32)i < rows) v = f.from_mont(E[(u64)i * len + j]);
        blk[2 * i] = (u32)i < rows ? __builtin_bswap32((u32)v) : ((u32)i == rows ? 0x80000000u : 0u);
        blk[2 * i + 1] = (u32)i < rows ? __builtin_bswap32((u32)(v >> 32)) : 0u;
      }
      blk[15] = 64 * rows;
      sha256_compress(st, blk);
    } else {
#pragma unroll 1
      for (u32 i0 = 0; i0 < rows; i0 += 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const u64 v = f.from_mont(E[(u64)(i0 + i) * len + j]);
          blk[2 * i] = __builtin_bswap32((u32)v);
          blk[2 * i + 1] = __builtin_bswap32((u32)(v >> 32));
        }
        sha256_compress(st, blk);
      }
      const u64 bits = (u64)rows * 64;
#pragma unroll
      for (int i = 0; i < 16; ++i) blk[i] = 0;
      blk[0] = 0x80000000u;
      blk[14] = (u32)(bits >> 32);
      blk[15] = (u32)bits;
      sha256_compress(st, blk);
    }
    st_digest(out + 8 * (u64)j, st);
  }
}

// out[m][k] = sum_i W[m][i] w[i C + k] for M weight vectors in one read of the table.  blockIdx.x takes V 256 columns, blockIdx.y
// the rows [y rows_per, (y+1) rows_per); a thread owns V adjacent columns (V = 2: one 16-byte load per row).  The products are
// accumulated unreduced and reduced every kAccMaxTerms rows.  part[y][m][k]: summed by row_combine_sum_kernel, or the result
// itself when gridDim.y = 1.
template <class F, int M, int V>
__global__ __launch_bounds__(kBlock) void row_combine_kernel(F f, const u64* __restrict__ w, const u64* __restrict__ W, u64 rows,
                                                             u64 rows_per, u32 cols, u64* __restrict__ part) {
  const u32 k = (blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (k >= cols) return;
  const u64 i0 = blockIdx.y * rows_per, i1 = i0 + rows_per < rows ? i0 + rows_per : rows;
  u64 res[M][V];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int v = 0; v < V; ++v) res[m][v] = 0;
  for (u64 a = i0; a < i1; a += F::kAccMaxTerms) {
    const u64 b = a + F::kAccMaxTerms < i1 ? a + F::kAccMaxTerms : i1;
    typename F::Acc acc[M][V];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int v = 0; v < V; ++v) f.acc_zero(acc[m][v]);
    for (u64 i = a; i < b; ++i) {
      u64 x[V];
      if constexpr (V == 2) {
        const ull2 t = *reinterpret_cast<const ull2*>(w + i * cols + k);
        x[0] = t.x;
        x[1] = t.y;
      } else {
        x[0] = w[i * cols + k];
      }
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const u64 wt = W[(u64)m * rows + i];
#pragma unroll
        for (int v = 0; v < V; ++v) f.acc_mac(acc[m][v], x[v], wt);
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int v = 0; v < V; ++v) res[m][v] = f.add(res[m][v], f.acc_get(acc[m][v]));
  }
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int v = 0; v < V; ++v) part[((u64)blockIdx.y * M + m) * cols + k + v] = res[m][v];
}

// out[e] = sum_y part[y][e], e < words = M C
template <class F>
__global__ __launch_bounds__(kBlock) void row_combine_sum_kernel(F f, const u64* __restrict__ part, u32 splits, u32 words, u64* __restrict__ out) {
  for (u32 e = blockIdx.x * blockDim.x + threadIdx.x; e < words; e += gridDim.x * blockDim.x) {
    u64 s = part[e];
    for (u32 y = 1; y < splits; ++y) s = f.add(s, part[(u64)y * words + e]);
    out[e] = s;
  }
}

// Opening q (one block each, grid-strided): the R Montgomery words of column index[q] of E (stride L) to vals[q][R], and the
// c + rho sibling digests of leaf index[q] to sib[q][depth][8].  levels: the whole tree bottom up (merkle.hpp).
__global__ __launch_bounds__(kBlock) void column_open_kernel(const u64* __restrict__ E, const u32* __restrict__ levels,
                                                             const u64* __restrict__ index, u32 count, u64 rows, u32 len, int depth,
                                                             u64* __restrict__ vals, u32* __restrict__ sib) {
  for (u32 q = blockIdx.x; q < count; q += gridDim.x) {
    const u32 j = (u32)index[q];
    for (u64 i = threadIdx.x; i < rows; i += blockDim.x) vals[(u64)q * rows + i] = E[i * len + j];
    for (u32 e = threadIdx.x; e < (u32)depth * 8; e += blockDim.x) {
      const u32 l = e >> 3;
      const u32 off = merkle_level_offset(len, (int)l);
      sib[((u64)q * depth + l) * 8 + (e & 7)] = levels[(u64)(off + ((j >> l) ^ 1)) * 8 + (e & 7)];
    }
  }
}

}  // namespace sc
#endif
