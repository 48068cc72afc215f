// Part of kernels.hpp (included there, in order): C = A * B of two 2^k x 2^k field matrices (sc_matmul) - the product that
// Thaler's MatMult protocol proves (matrix-multiplication/src/lib.rs, its tests `randomized_test` / `matrix_test_from_book`).
#pragma once

namespace sc {

// ------------------------------------------------------------------------------------
// Layout: row-major, column index in the low k bits (the convention of sc_matmul_g_new).  All words are Montgomery
// residues, so C[i][j] = sum_y A[i][y] (*) B[y][j] = (sum_y a b) R^-1 mod p.
//
// Hot path: the int8 matrix cores on the words' BYTES.  With a = sum_i 2^(8i) a_i, b = sum_j 2^(8j) b_j,
//     sum_y a b = sum_d 2^(8d) T_d,    T_d = sum_{i + j = d} sum_y a_i[y] b_j[y]      (d = 0..14: 15 diagonals)
// and every T_d is an exact integer.  1. matmul_bytes_a_kernel / matmul_bytes_b_kernel repack A into eight byte planes
// A8[i][row][y] and B into eight TRANSPOSED planes B8t[j][col][y] (both MFMA operands are then 16 contiguous bytes per
// lane, as in matsq_bytes_kernel), padding y up to KP = max(2^k, 64) with the byte 0x80, and take the plane sums
// SA[i][row] = sum_y a_i, SB[j][col] = sum_y b_j.  2. matmul_mfma_kernel: one wave per 16 x 16 tile of C,
// v_mfma_i32_16x16x64_i8 over y in steps of 64, byte pair (i, j) into the accumulator of its diagonal i + j.
//
// Signed bytes: the instruction multiplies SIGNED bytes; s = u ^ 0x80 = u - 128 (the padding byte is s = 0), and
//     sum_y u u' = sum_y s s' + 128 (SA_i + SB_j) - 16384 K                  (K = 2^k, the real contraction length)
//
// ACCUMULATOR BOUND.  |s s'| <= 128 * 128 = 2^14 (reached only by s = s' = -128, i.e. byte 0 against byte 0; the most
// negative product is -128 * 127).  A diagonal takes at most 8 byte pairs, so one y adds at most 8 * 2^14 = 2^17 to an
// int32 accumulator: a run of R contraction steps is exact while 2^17 R <= 2^31 - 1, i.e. R <= 16383.  Runs are whole
// MFMA steps of 64: kMatmulRunSteps = 255 steps = 16320 y (2^17 * 16320 = 2139095040 < 2^31).  At k = 14 (K = 16384 =
// 256 steps) the contraction therefore takes two runs; 256 steps in one run would reach exactly 2^31 on all-zero
// words and wrap.  Behind each run the wave adds its 15 accumulators, signed and shifted by 8d, into a 192-bit sum per
// output entry (three words; the true value sum_y a b < 2^142) and clears them.
//
// Epilogue: the 192-bit sum plus the offset terms, then ONE reduction: wide_get(w0, w1, w2) = w * 2^-64 mod p, which
// also supplies the R^-1 of the Montgomery products.  The loop never sees p: the same code serves every modulus.
//
// Traffic model (what tools/matmul_timing.py reports): the repack reads 16 K^2 bytes (A and B) and writes 16 K KP bytes
// of planes; the product reads each plane byte once per tile row / column it meets - 16 K KP (K / 16) bytes from the
// caches - and writes 8 K^2 bytes of C.
//
// Comparison path (option matmul_path = 2) and small matrices: matmul_tiled_kernel (the field's lazy multiply-add on the
// VALU: matsq_tiled_kernel's 64 x 64 tiles with two inputs) and, below 64 x 64, matmul_kernel (one thread per entry).
constexpr int kMatmulStepK = 64;          // y per v_mfma_i32_16x16x64_i8
constexpr int kMatmulRunSteps = 255;      // MFMA steps one int32 accumulator run takes (bound above)
constexpr int kMatmulMaxRunK = kMatmulRunSteps * kMatmulStepK;
static_assert((long long)8 * 128 * 128 * kMatmulMaxRunK <= 2147483647ll, "a run must fit int32 on the worst byte pattern");
constexpr int kMatmulBRun = 256;          // y per thread of matmul_bytes_b_kernel

typedef int mm_v4i __attribute__((ext_vector_type(4)));

// A -> A8[i][row][y] (i = byte), SA[i][row] += sum_y byte.  Thread = (row, 16 consecutive y): coalesced 128-byte reads,
// 16-byte writes per plane; the row sums are reduced over the lanes of one row before the atomics.  KP / 16 >= 4 chunks
// per row, a power of two: a wave holds whole rows, or a run of chunks of one row.
template <class F>
__global__ void __launch_bounds__(kBlock)
matmul_bytes_a_kernel(F f, const u64* __restrict__ A, int k, size_t KP, unsigned char* __restrict__ A8, unsigned* __restrict__ SA) {
  const size_t n = (size_t)1 << k, cpr = KP / 16, total = n * cpr, plane = n * KP;
  const int seg = (int)(cpr < (size_t)kWave ? cpr : (size_t)kWave), lane = threadIdx.x & (kWave - 1);
  for (size_t base = (size_t)blockIdx.x * kBlock; base < total; base += (size_t)gridDim.x * kBlock) {
    const size_t t = base + threadIdx.x;   // (total is a multiple of kBlock or below it: whole waves stay in step)
    const bool live = t < total;
    const size_t row = live ? t / cpr : 0, y0 = live ? (t % cpr) * 16 : 0;
    unsigned w[8][4], s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s[i] = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) w[i][q] = 0x80808080u;
    }
    if (live && y0 < n) {
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const ull2 v = *reinterpret_cast<const ull2*>(A + row * n + y0 + e);
        const u64 vv[2] = {v.x, v.y};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const unsigned b = (unsigned)(vv[h] >> (8 * i)) & 0xFF;
            const int ee = e + h;
            w[i][ee >> 2] = (w[i][ee >> 2] & ~(0xFFu << (8 * (ee & 3)))) | (b << (8 * (ee & 3)));
            s[i] += b;
          }
      }
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint4*>(A8 + i * plane + row * KP + y0) = uint4{w[i][0], w[i][1], w[i][2], w[i][3]};
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      for (int off = 1; off < seg; off <<= 1) s[i] += (unsigned)__shfl_xor((int)s[i], off, kWave);
    if (live && (lane & (seg - 1)) == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) atomicAdd(SA + i * n + row, s[i]);
    }
  }
}

// B -> B8t[j][col][y] = byte j of B[y][col], SB[j][col] += sum_y byte.  Thread = (col, run of kMatmulBRun y): lanes own
// consecutive columns, so every read instruction is 512 contiguous bytes; a thread writes its run as 16-byte pieces.
template <class F>
__global__ void __launch_bounds__(kBlock)
matmul_bytes_b_kernel(F f, const u64* __restrict__ B, int k, size_t KP, unsigned char* __restrict__ B8t, unsigned* __restrict__ SB) {
  const size_t n = (size_t)1 << k, run = KP < (size_t)kMatmulBRun ? KP : (size_t)kMatmulBRun, total = n * (KP / run), plane = n * KP;
  for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (size_t)gridDim.x * kBlock) {
    const size_t col = t % n, y_begin = (t / n) * run;
    unsigned s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t y0 = y_begin; y0 < y_begin + run; y0 += 16) {
      unsigned w[8][4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[i][q] = 0x80808080u;
      if (y0 < n) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const u64 v = B[(y0 + e) * n + col];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const unsigned b = (unsigned)(v >> (8 * i)) & 0xFF;
            w[i][e >> 2] = (w[i][e >> 2] & ~(0xFFu << (8 * (e & 3)))) | (b << (8 * (e & 3)));
            s[i] += b;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint4*>(B8t + i * plane + col * KP + y0) = uint4{w[i][0], w[i][1], w[i][2], w[i][3]};
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) atomicAdd(SB + i * n + col, s[i]);
  }
}

// w += x * 2^sh (x signed, 0 <= sh < 128; w a 192-bit two's-complement sum)
__device__ __forceinline__ void mm_wide_add(u64 (&w)[3], long long x, int sh) {
  const u64 ext = x < 0 ? ~0ull : 0ull;
  u64 l0, l1, l2;
  if (sh == 0) { l0 = (u64)x; l1 = ext; l2 = ext; }
  else if (sh < 64) { l0 = (u64)x << sh; l1 = (u64)(x >> (64 - sh)); l2 = ext; }
  else if (sh == 64) { l0 = 0; l1 = (u64)x; l2 = ext; }
  else { l0 = 0; l1 = (u64)x << (sh - 64); l2 = (u64)(x >> (128 - sh)); }
  u64 t;
  const bool c0 = __builtin_add_overflow(w[0], l0, &t);
  w[0] = t;
  const bool c1 = __builtin_add_overflow(w[1], l1, &t);
  const bool c2 = __builtin_add_overflow(t, (u64)(c0 ? 1 : 0), &t);
  w[1] = t;
  w[2] += l2 + (c1 ? 1 : 0) + (c2 ? 1 : 0);
}

// One wave per 16 x 16 tile of C.  Fragments (16x16x64 i8): lane (r = lane & 15, g = lane >> 4) supplies row r of the
// A tile and column r of the B tile, y = y0 + 16 g + (0..15) for both - whatever y order the instruction uses inside a
// step, the pairs it forms have the same y.  C/D layout: col = lane & 15, row = 4 (lane >> 4) + reg.
template <class F>
__global__ void __launch_bounds__(kBlock)
matmul_mfma_kernel(F f, const unsigned char* __restrict__ A8, const unsigned char* __restrict__ B8t, const unsigned* __restrict__ SA,
                   const unsigned* __restrict__ SB, int k, size_t KP, u64* __restrict__ C) {
  const size_t n = (size_t)1 << k, plane = n * KP, tiles_x = n / 16, n_tiles = tiles_x * tiles_x, steps = KP / kMatmulStepK;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, r = lane & 15, g = lane >> 4;
  for (size_t tid = (size_t)blockIdx.x * (kBlock / kWave) + wave; tid < n_tiles; tid += (size_t)gridDim.x * (kBlock / kWave)) {
    const size_t r0 = (tid / tiles_x) * 16, c0 = (tid % tiles_x) * 16;
    const unsigned char* ap = A8 + (r0 + r) * KP + 16 * g;
    const unsigned char* bp = B8t + (c0 + r) * KP + 16 * g;
    u64 w[4][3];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e][0] = w[e][1] = w[e][2] = 0;
    for (size_t s0 = 0; s0 < steps; s0 += kMatmulRunSteps) {
      const size_t s1 = s0 + kMatmulRunSteps < steps ? s0 + kMatmulRunSteps : steps;
      mm_v4i acc[15];
#pragma unroll
      for (int d = 0; d < 15; ++d) acc[d] = mm_v4i{0, 0, 0, 0};
      for (size_t s = s0; s < s1; ++s) {
        mm_v4i a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          a[i] = *reinterpret_cast<const mm_v4i*>(ap + i * plane + s * kMatmulStepK);
          b[i] = *reinterpret_cast<const mm_v4i*>(bp + i * plane + s * kMatmulStepK);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          a[i] ^= 0x80808080;
          b[i] ^= 0x80808080;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i + j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i + j], 0, 0, 0);
      }
#pragma unroll
      for (int d = 0; d < 15; ++d)
#pragma unroll
        for (int e = 0; e < 4; ++e) mm_wide_add(w[e], (long long)acc[d][e], 8 * d);
    }
    const size_t col = c0 + r;
    unsigned sb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sb[j] = SB[j * n + col];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t row = r0 + 4 * g + e;
      unsigned sa[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) sa[i] = SA[i * n + row];
#pragma unroll
      for (int d = 0; d < 15; ++d) {
        long long c = 0;
        int pairs = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (d - i >= 0 && d - i < 8) {
            c += (long long)sa[i] + (long long)sb[d - i];
            ++pairs;
          }
        mm_wide_add(w[e], 128 * c - 16384ll * (long long)n * pairs, 8 * d);
      }
      C[row * n + col] = f.wide_get(w[e][0], w[e][1], (u32)w[e][2]);   // (w2 < 2^14)
    }
  }
}

// C[(z << k) | x] = sum_y A[(z << k) | y] B[(y << k) | x], one thread per entry (any k)
template <class F>
__global__ void __launch_bounds__(kBlock)
matmul_kernel(F f, const u64* __restrict__ A, const u64* __restrict__ B, int k, u64* __restrict__ C) {
  const size_t n = (size_t)1 << k, total = n * n;
  for (size_t o = (size_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += (size_t)gridDim.x * kBlock) {
    const size_t z = o >> k, x = o & (n - 1);
    typename F::Acc acc;
    f.acc_zero(acc);
    for (size_t y = 0; y < n; ++y) f.acc_mac(acc, A[(z << k) | y], B[(y << k) | x]);
    C[o] = f.acc_get(acc);
  }
}

// matsq_tiled_kernel with two inputs (k >= 6): a block owns a 64 x 64 tile of C and walks y in steps of 32, staging
// B[y][x0..x0+64) and, transposed, At[y][z0..z0+64) = A[(z << k) | y] in LDS; every thread accumulates a 4 x 4 patch.
template <class F>
__global__ void __launch_bounds__(kBlock)
matmul_tiled_kernel(F f, const u64* __restrict__ A, const u64* __restrict__ B, int k, u64* __restrict__ C) {
  constexpr int TS = 64, KT = 32;
  __shared__ ull2 lds_b[KT * TS / 2];   // B[yy][xx], 16 KiB
  __shared__ u64 lds_a[KT * TS];        // At[yy][zz], 16 KiB
  const size_t n = (size_t)1 << k;
  const int tiles = (int)(n / TS);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int tile = blockIdx.x; tile < tiles * tiles; tile += gridDim.x) {
    const size_t x0 = (size_t)(tile % tiles) * TS, z0 = (size_t)(tile / tiles) * TS;
    typename F::Acc acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) f.acc_zero(acc[j][i]);
    for (size_t y0 = 0; y0 < n; y0 += KT) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (threadIdx.x >> 5) + 8 * i, pc = threadIdx.x & 31;
        lds_b[row * (TS / 2) + pc] = reinterpret_cast<const ull2*>(B + ((y0 + row) << k) + x0)[pc];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int zz = (threadIdx.x >> 4) + 16 * i, pc = threadIdx.x & 15;
        const ull2 v = reinterpret_cast<const ull2*>(A + ((z0 + zz) << k) + y0)[pc];
        lds_a[(2 * pc) * TS + zz] = v.x;
        lds_a[(2 * pc + 1) * TS + zz] = v.y;
      }
      __syncthreads();
      for (int yy = 0; yy < KT; ++yy) {
        const ull2 b01 = lds_b[yy * (TS / 2) + 2 * tx], b23 = lds_b[yy * (TS / 2) + 2 * tx + 1];
        const ull2 a01 = reinterpret_cast<const ull2*>(lds_a + yy * TS)[2 * ty],
                   a23 = reinterpret_cast<const ull2*>(lds_a + yy * TS)[2 * ty + 1];
        const u64 b[4] = {b01.x, b01.y, b23.x, b23.y}, a[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) f.acc_mac(acc[j][i], a[j], b[i]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ull2 o0 = {f.acc_get(acc[j][0]), f.acc_get(acc[j][1])}, o1 = {f.acc_get(acc[j][2]), f.acc_get(acc[j][3])};
      ull2* dst = reinterpret_cast<ull2*>(C + ((z0 + 4 * ty + j) << k) + x0 + 4 * tx);
      dst[0] = o0;
      dst[1] = o1;
    }
  }
}

}  // namespace sc
