// Part of kernels.hpp (included there, in order): the two kernels behind an argument for rank-1 constraint satisfiability with a
// committed witness - a sparse matrix-vector product over the field and a cubic sumcheck pass with an eq factor.  The host parts
// (SC_HD) compile without hipcc: tests/cpp/r1cs_host_harness.cpp replays them.
//
// THE PROTOCOL (the contract; Thaler, "Proofs, Arguments, and Zero-Knowledge", section 8.4: Spartan's two sumchecks, the witness
// half of z committed by Ligero, thaler-study_amd/ligero_pcs.py)
//
//   Instance.  A, B, C in F^(2^s x 2^m), each a list of (row, col, val) triples; val is a Montgomery word < p, like every table
//   word of the ABI; triples with the same (row, col) add.  z in F^(2^m) is one LE table: z[0 .. 2^(m-1)) is the public half
//   x = (1, io_1, .., io_k, 0, ..), z[2^(m-1) .. 2^m) the witness w, so z~(y) = (1 - y[m-1]) x~(y[:m-1]) + y[m-1] w~(y[:m-1]).
//   The statement is (A z) o (B z) = C z.  Both sumchecks bind variable 0 first, the order of sc_prove.
//
//    1. P commits w (m - 1 variables) with ligero_pcs.Prover.commit / commit_long and sends the root.
//    2. V draws tau in F^s.
//    3. Sumcheck 1, cubic, over sum_x eq(tau, x) (Az(x) Bz(x) - Cz(x)), claimed to be 0.  Before round j = 0 .. s-1 the four
//       tables E_j (E_0 = eq(tau, .)), A_j, B_j, C_j have 2^(s-j) entries; with u_i(t) = u[2i] + t (u[2i+1] - u[2i]) the round
//       message is H_j(t) = sum_{i < 2^(s-j-1)} e_i(t) (a_i(t) b_i(t) - c_i(t)) at t = 0, 1, 2, 3.  V checks H_j(0) + H_j(1)
//       against the running claim (0 at j = 0), draws r_j, and the new claim is the cubic through the four values at r_j.  All four
//       tables fold by r_j.  After s rounds P sends v_A, v_B, v_C = A_s[0], B_s[0], C_s[0] and V checks
//       eq(tau, r_x) (v_A v_B - v_C) against the claim.  Fields with p <= 3 are refused: interpolation on {0, 1, 2, 3} needs 2 and
//       3 invertible.
//    4. V draws rho_A, rho_B, rho_C.
//    5. P builds T[y] = sum_k rho_k sum_i eq(r_x, i) M_k[i][y]: the three transposed products with the one vector eq(r_x, .).
//    6. Sumcheck 2 is the existing product prover sc_prove(T, z), claim rho_A v_A + rho_B v_B + rho_C v_C, m rounds, ending at r_y.
//    7. V computes T~(r_y) = sum_k rho_k sum_{(i,j,v) in M_k} eq(r_x, i) v eq(r_y, j) from the instance on the host:
//       O(nnz + 2^s + 2^m).  This verifier reads the instance; kernels/spark.hpp states the exchange that hands T~(r_y) to one that holds its roots.
//    8. V computes x~(r_y[:m-1]) from the public inputs.
//    9. V obtains w~(r_y[:m-1]) from one opening of the commitment (the plain Verifier, or a folded opening through open_folded).
//   10. V checks T~(r_y) z~(r_y) against the last claim of sumcheck 2.
//
//   Soundness.  Nothing beyond the book's statement of each part is claimed: no security level, no zero knowledge.
//
// THE SPARSE PRODUCT  y = M v over a row-sorted image of M: three parallel streams row[], col[] (u32) and val[] (u64), nnz entries,
// rows non-decreasing.  The same kernel serves M^T v over the row-sorted image of M^T.  Row lengths are heavily skewed in the
// transposed direction (the constant column of an R1CS holds an entry per constraint), so the work is split by NONZEROS: block b
// owns the entries [b N_b, (b+1) N_b), N_b = kSpmvBlockEntries, thread t of it the kSpmvRun consecutive entries from
// b N_b + t kSpmvRun.  A thread forms val v[col] in a lazy accumulator per row segment (spmv_item): the rows that begin and end
// inside its run are finished and stored, its first and last segment are handed to the block, which adds them by row with a
// segmented scan in LDS (seg_block_reduce).  Of the block's rows those strictly between its first and its last entry's row are
// finished and stored; the first and the last stay open and leave as two carries (row, value) per block - (row, 0) for the second
// when the block holds one row.  A second, one-block launch (spmv_carry_kernel) walks the 2 x blocks carries, which are sorted by
// row, with the same code and STORES every row's sum: a row is either finished by exactly one block or made of carries alone.  y
// is zeroed on the stream before the product (the empty rows).  No atomics on field words, no cross-block hand-off: two launches
// on the stream.  The val, col and row streams are read as consecutive words per lane; the gather of v is the only irregular
// access.
//
// THE CUBIC PASS  zc_pass_kernel<F, FOLD>: one launch per round.  With FOLD a thread reads four consecutive entries of each of
// the four tables, folds them by the previous challenge to two entries, stores those and accumulates H(0..3) from the folded
// pair (zc_fold4, zc_accumulate); round 0 reads two entries per table, folds nothing and stores nothing.  The sums leave through finish_pass<F, 4>.
// No scratch, no LDS beyond the reduction.
#pragma once
#include <vector>

#include "../field.hpp"

namespace sc {

constexpr int kSpmvRun = 8;                            // consecutive entries of one thread
constexpr int kSpmvThreads = 256;
constexpr int kSpmvBlockEntries = kSpmvThreads * kSpmvRun;   // N_b = 2048: the run of entries one block owns
constexpr u32 kSpmvNoRow = 0xFFFFFFFFu;                // a thread past the end of the entries

struct SegPart {
  u32 row;
  u64 val;
};

// One thread's run: n <= K entries (row[k], val[k]) against vec[k] = v[col[k]], rows non-decreasing.  Rows strictly inside the run
// are stored to y; head = the first segment, tail = the last one - (the same row, 0) when the run is one segment, so that the
// block's list of parts stays sorted by row; an empty run gives (kSpmvNoRow, 0) twice.
template <class F, int K>
SC_HD void spmv_item(const F& f, const u32 (&row)[K], const u64 (&val)[K], const u64 (&vec)[K], int n, u64* __restrict__ y, SegPart& head,
                     SegPart& tail) {
  head.row = tail.row = kSpmvNoRow;
  head.val = tail.val = 0;
  if (n <= 0) return;
  typename F::Acc acc;
  f.acc_zero(acc);
  u32 cur = row[0];
  bool first = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (k < n) {
      if (row[k] != cur) {
        const u64 v = f.acc_get(acc);
        if (first) {
          head.row = cur;
          head.val = v;
          first = false;
        } else {
          y[cur] = v;
        }
        f.acc_zero(acc);
        cur = row[k];
      }
      f.acc_mac(acc, val[k], vec[k]);
    }
  }
  const u64 v = f.acc_get(acc);
  if (first) {
    head.row = cur;
    head.val = v;
    tail.row = cur;
    tail.val = 0;
  } else {
    tail.row = cur;
    tail.val = v;
  }
}

// What a block does with the total of one row of its list of parts: the rows of its first and of its last entry stay open
// (open[0], open[1]; a block of one row leaves (that row, 0) as the second), every other row is finished.
SC_HD void seg_place(u32 row, u64 total, u32 first_row, u32 last_row, u64* __restrict__ y, SegPart* open) {
  if (row == first_row) open[0].val = total;
  else if (row == last_row) open[1].val = total;
  else y[row] = total;
}

// One item of the cubic pass: the pairs (e, a, b, c)[0..1] of one index i -> H(0..3) += e_i(t) (a_i(t) b_i(t) - c_i(t)).
template <class F>
SC_HD void zc_accumulate(const F& f, typename F::Acc (&acc)[4], const u64 (&e)[2], const u64 (&a)[2], const u64 (&b)[2], const u64 (&c)[2]) {
  const u64 de = f.sub(e[1], e[0]), da = f.sub(a[1], a[0]), db = f.sub(b[1], b[0]), dc = f.sub(c[1], c[0]);
  u64 et = e[0], at = a[0], bt = b[0], ct = c[0];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t == 1) {
      et = e[1]; at = a[1]; bt = b[1]; ct = c[1];
    } else if (t > 1) {
      et = f.add(et, de); at = f.add(at, da); bt = f.add(bt, db); ct = f.add(ct, dc);
    }
    f.acc_mac(acc[t], et, f.sub(f.mul(at, bt), ct));
  }
}
// u[0..3] -> the two entries folded by r: u[2i] + r (u[2i+1] - u[2i])
template <class F>
SC_HD void zc_fold4(const F& f, u64 r, const u64 (&u)[4], u64 (&o)[2]) {
  o[0] = f.add(u[0], f.mul(r, f.sub(u[1], u[0])));
  o[1] = f.add(u[2], f.mul(r, f.sub(u[3], u[2])));
}

// The row-sorted image of nnz entries (key[e], other[e], val[e]), key < n_keys: a stable counting sort on the host - the entries
// of a row keep the order they were given in.  The outputs have nnz entries each.
inline void image_sort(const u32* key, const u32* other, const u64* val, size_t nnz, size_t n_keys, u32* srow, u32* scol, u64* sval) {
  std::vector<size_t> start(n_keys + 1, 0);
  for (size_t e = 0; e < nnz; ++e) start[(size_t)key[e] + 1] += 1;
  for (size_t k = 0; k < n_keys; ++k) start[k + 1] += start[k];
  for (size_t e = 0; e < nnz; ++e) {
    const size_t at = start[key[e]]++;
    srow[at] = key[e];
    scol[at] = other[e];
    sval[at] = val[e];
  }
}

#if defined(__HIPCC__)

// The block's 2 x BS parts (thread t: head at slot 2t, tail at 2t + 1; sorted by row, kSpmvNoRow last) summed by row with a
// segmented inclusive scan in LDS; the row totals go where seg_place says.  open[0..1] (LDS) are valid after the call.
// first_row / last_row: the rows of the block's first and last entry.
template <class F, int BS>
__device__ __forceinline__ void seg_block_reduce(const F& f, const SegPart& head, const SegPart& tail, u32 first_row, u32 last_row,
                                                 u64* __restrict__ y, u32* srow, u64* sval, SegPart* open) {
  constexpr int N = 2 * BS;
  const int t = threadIdx.x;
  srow[2 * t] = head.row;
  sval[2 * t] = head.val;
  srow[2 * t + 1] = tail.row;
  sval[2 * t + 1] = tail.val;
  if (t == 0) {
    open[0].row = first_row;
    open[0].val = 0;
    open[1].row = last_row;
    open[1].val = 0;
  }
  __syncthreads();
  // slots t and t + BS
  const u32 r0 = srow[t], r1 = srow[t + BS];
  for (int d = 1; d < N; d <<= 1) {
    const int q0 = t, q1 = t + BS;
    const bool h0 = q0 >= d && srow[q0 - d] == r0, h1 = q1 >= d && srow[q1 - d] == r1;
    const u64 x0 = h0 ? sval[q0 - d] : 0, x1 = h1 ? sval[q1 - d] : 0;
    __syncthreads();
    if (h0) sval[q0] = f.add(sval[q0], x0);
    if (h1) sval[q1] = f.add(sval[q1], x1);
    __syncthreads();
  }
  // the last slot of every row holds its total
  if (r0 != kSpmvNoRow && srow[t + 1] != r0) seg_place(r0, sval[t], first_row, last_row, y, open);
  if (r1 != kSpmvNoRow && (t + BS == N - 1 || srow[t + BS + 1] != r1)) seg_place(r1, sval[t + BS], first_row, last_row, y, open);
  __syncthreads();
}

// y = M v, the block's share.  nnz > 0; grid = ceil(nnz / kSpmvBlockEntries); y zeroed before.  carry_row / carry_val: 2 per block.
template <class F>
__global__ void __launch_bounds__(kSpmvThreads)
spmv_kernel(F f, const u32* __restrict__ row, const u32* __restrict__ col, const u64* __restrict__ val, size_t nnz, const u64* __restrict__ v,
            u64* __restrict__ y, u32* __restrict__ carry_row, u64* __restrict__ carry_val) {
  constexpr int K = kSpmvRun;
  __shared__ u32 srow[2 * kSpmvThreads + 1];
  __shared__ u64 sval[2 * kSpmvThreads];
  __shared__ SegPart open[2];
  const size_t base = (size_t)blockIdx.x * kSpmvBlockEntries;
  const size_t lo = base + (size_t)threadIdx.x * K;
  const size_t end = (base + kSpmvBlockEntries < nnz) ? base + kSpmvBlockEntries : nnz;
  u32 r[K], c[K];
  u64 x[K], g[K];
  int n = 0;
  if (lo + K <= nnz) {
    // whole run: eight consecutive words of every stream per lane (the streams are 32-byte aligned at every multiple of K)
    const uint4* rp = reinterpret_cast<const uint4*>(row + lo);
    const uint4* cp = reinterpret_cast<const uint4*>(col + lo);
    const ulonglong2* xp = reinterpret_cast<const ulonglong2*>(val + lo);
#pragma unroll
    for (int h = 0; h < K / 4; ++h) {
      const uint4 rr = rp[h], cc = cp[h];
      r[4 * h] = rr.x; r[4 * h + 1] = rr.y; r[4 * h + 2] = rr.z; r[4 * h + 3] = rr.w;
      c[4 * h] = cc.x; c[4 * h + 1] = cc.y; c[4 * h + 2] = cc.z; c[4 * h + 3] = cc.w;
    }
#pragma unroll
    for (int h = 0; h < K / 2; ++h) {
      const ulonglong2 xx = xp[h];
      x[2 * h] = xx.x;
      x[2 * h + 1] = xx.y;
    }
    n = K;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool in = lo + k < nnz;
      r[k] = in ? row[lo + k] : kSpmvNoRow;
      c[k] = in ? col[lo + k] : 0;
      x[k] = in ? val[lo + k] : 0;
      n += in ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) g[k] = (k < n) ? v[c[k]] : 0;
  SegPart head, tail;
  spmv_item<F, K>(f, r, x, g, n, y, head, tail);
  const u32 first_row = row[base], last_row = row[end - 1];
  seg_block_reduce<F, kSpmvThreads>(f, head, tail, first_row, last_row, y, srow, sval, open);
  if (threadIdx.x < 2) {
    carry_row[2 * (size_t)blockIdx.x + threadIdx.x] = open[threadIdx.x].row;
    carry_val[2 * (size_t)blockIdx.x + threadIdx.x] = open[threadIdx.x].val;
  }
}

// The second launch, one block: y[row] = the sum of the carries of that row, for every row among the n carries (sorted by row).
// The carries are walked kSpmvBlockEntries at a time with the code of the product (val * 1); a chunk's open first and last rows
// are joined to the running row by thread 0.
template <class F>
__global__ void __launch_bounds__(kSpmvThreads)
spmv_carry_kernel(F f, const u32* __restrict__ carry_row, const u64* __restrict__ carry_val, size_t n, u64* __restrict__ y) {
  constexpr int K = kSpmvRun;
  __shared__ u32 srow[2 * kSpmvThreads + 1];
  __shared__ u64 sval[2 * kSpmvThreads];
  __shared__ SegPart open[2];
  __shared__ SegPart run;
  if (threadIdx.x == 0) {
    run.row = kSpmvNoRow;
    run.val = 0;
  }
  const u64 one = f.one();
  for (size_t base = 0; base < n; base += kSpmvBlockEntries) {
    const size_t lo = base + (size_t)threadIdx.x * K;
    const size_t end = (base + kSpmvBlockEntries < n) ? base + kSpmvBlockEntries : n;
    u32 r[K];
    u64 x[K], g[K];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool in = lo + k < n;
      r[k] = in ? carry_row[lo + k] : kSpmvNoRow;
      x[k] = in ? carry_val[lo + k] : 0;
      g[k] = one;
      cnt += in ? 1 : 0;
    }
    SegPart head, tail;
    spmv_item<F, K>(f, r, x, g, cnt, y, head, tail);
    seg_block_reduce<F, kSpmvThreads>(f, head, tail, carry_row[base], carry_row[end - 1], y, srow, sval, open);
    if (threadIdx.x == 0) {
      SegPart first = open[0];
      if (run.row == first.row) first.val = f.add(first.val, run.val);
      else if (run.row != kSpmvNoRow) y[run.row] = run.val;
      if (open[1].row == first.row) {
        run = first;
      } else {
        y[first.row] = first.val;
        run = open[1];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && run.row != kSpmvNoRow) y[run.row] = run.val;
}

// v[k n + i] = rho[k] eq[i], k < 3: the one vector of sc_r1cs_bind_rows' product over the three transposed images side by side
struct Rho3 {
  u64 w[3];
};
template <class F>
__global__ void __launch_bounds__(kBlock) scale3_kernel(F f, const u64* __restrict__ eq, Rho3 rho, size_t n, u64* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const u64 e = eq[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)k * n + i] = f.mul(rho.w[k], e);
  }
}

// One round of the cubic sumcheck over tables T[0..3] = E, A, B, C.  FOLD: the tables have 4 n_units entries; unit i folds entries
// 4i .. 4i+3 of each by r into entries 2i, 2i+1 of O[.] and adds them to H(0..3).  Otherwise: 2 n_units entries, nothing stored.
struct ZcTables {
  const u64* in[4];
  u64* out[4];
};
template <class F, bool FOLD>
__global__ void __launch_bounds__(kBlock) zc_pass_kernel(F f, ZcTables tb, u64 r, size_t n_units, PassOut out) {
  __shared__ u64 lds[(kBlock / kWave) * 4];
  __shared__ int lds_flag;
  typename F::Acc acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) f.acc_zero(acc[s]);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_units; i += (size_t)gridDim.x * kBlock) {
    u64 p[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
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
    zc_accumulate(f, acc, p[0], p[1], p[2], p[3]);
  }
  const u64 mine = reduce_cells<F, 4>(f, acc, lds);
  finish_pass<F, 4>(f, out, mine, &lds_flag);
}

#endif   // __HIPCC__

}  // namespace sc
