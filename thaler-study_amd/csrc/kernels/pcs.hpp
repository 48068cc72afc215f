// Relaxed PCS (relaxed-pcs/src/lib.rs of the reference): the prover's grid evaluation and its SHA-256 Merkle commitment.
//
// Grid order (IF::all_multidimentional_values, :46-63): the p^m points (v_0, .., v_{m-1}) of F^m sorted lexicographically by
// canonical value, v_0 the most significant digit: the leaf index of a point is o = sum_j v_j p^(m-1-j).  Its value is
// poly.evaluate(point) (:166-170), the dense MLE in LE order: point[0] binds index bit 0 of the table.  So variable 0 has input
// stride 1 but output stride p^(m-1).  The values are padded with zeros to N = 2^ceil(log2 p^m) (:172-177).
//
// The tree over the values is merkle.hpp's, its digests sha256.hpp's; this header adds the leaves: N of them, leaf digest
// sha256_leaf of the canonical value, the root of a one-leaf tree that leaf's digest.
#pragma once
#include "merkle.hpp"

namespace sc {

// Device footprint: the levels below kMerkleBase are not kept (at N = 2^28 the whole tree would be 16 GiB; from level 4 up it is
// N * 4 bytes); an opening recomputes its 2^kMerkleBase-leaf bottom subtree from the values, on the host.
constexpr int kMerkleBase = 4;
// sc_table_extend_grid: outputs of one axis chain per thread (one multiplication starts the chain, the rest are additions)
constexpr int kGridRun = 8;

}  // namespace sc

#if defined(__HIPCC__)
namespace sc {

// One axis of sc_table_extend_grid.  The table is viewed as (E, 2, B) - E = p^s extended digits in front, the binary axis being
// extended, B = 2^log_b binary entries behind it - and becomes (p, E, B): out[v E B + g] = in0 + v (in1 - in0), g = (e, b).  Taking
// the input's binary axes from the slowest (variable m - 1) down and putting each new axis in front leaves v_0 the slowest digit
// and v_{m-1} the fastest: the reference's leaf order.  Every thread extends one (e, b) over kGridRun consecutive v; lanes run
// along g, so every store of a wave is one contiguous run.  eb * ceil(p / kGridRun) < 2^30 (p^m <= 2^28).
__global__ __launch_bounds__(kBlock) void grid_extend_kernel(MontGeneric f, const u64* __restrict__ in, u64* __restrict__ out, u32 eb,
                                                             int log_b, u32 runs) {
  const u32 work = eb * runs, p = (u32)f.p;
  const u32 bmask = (1u << log_b) - 1;
  for (u32 wi = blockIdx.x * blockDim.x + threadIdx.x; wi < work; wi += gridDim.x * blockDim.x) {
    const u32 r = wi / eb, g = wi - r * eb;
    const u64 i0 = ((u64)(g >> log_b) << (log_b + 1)) | (g & bmask);
    const u64 x0 = in[i0], x1 = in[i0 + bmask + 1];
    const u64 d = f.sub(x1, x0);
    const u32 v0 = r * kGridRun, v1 = min(p, v0 + kGridRun);
    u64 acc = f.add(x0, f.mul(f.to_mont(v0), d));
    for (u32 v = v0; v < v1; ++v) {
      out[(u64)v * eb + g] = acc;
      acc = f.add(acc, d);
    }
  }
}

// Leaves up to level lb (<= kMerkleBase): every lane hashes the 2^lb consecutive leaves of one subtree and folds them to its root,
// which it writes (level lb, 8 words per node).  The pending left digests of the levels below live in four named register sets
// (s0..s3), picked by selects on the wave-uniform level: nothing is indexed at run time.  One leaf compression and one node
// (two compressions) are inlined; the loops stay loops.
template <class F>
__global__ __launch_bounds__(kBlock) void merkle_leaf_kernel(F f, const u64* __restrict__ values, int lb, u64 subtrees,
                                                             u32* __restrict__ out) {
  const u32 per = 1u << lb;
  for (u64 s = blockIdx.x * (u64)blockDim.x + threadIdx.x; s < subtrees; s += (u64)gridDim.x * blockDim.x) {
    const u64* v = values + (s << lb);
    u32 s0[8] = {}, s1[8] = {}, s2[8] = {}, s3[8] = {};
#pragma unroll 1
    for (u32 i = 0; i < per; ++i) {
      u32 d[8];
      sha256_leaf(f.from_mont(v[i]), d);
      int lvl = 0;
#pragma unroll 1
      for (; lvl < lb && ((i >> lvl) & 1); ++lvl) {
        u32 l[8], t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          l[k] = lvl == 0 ? s0[k] : lvl == 1 ? s1[k] : lvl == 2 ? s2[k] : s3[k];
          t[k] = d[k];
        }
        sha256_node(l, t, d);
      }
      if (lvl == lb) {
        st_digest(out + 8 * s, d);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          s0[k] = lvl == 0 ? d[k] : s0[k];
          s1[k] = lvl == 1 ? d[k] : s1[k];
          s2[k] = lvl == 2 ? d[k] : s2[k];
          s3[k] = lvl == 3 ? d[k] : s3[k];
        }
      }
    }
  }
}

// What sc_merkle_open needs from the device, one opening per thread: the 2^lb canonical values of the leaf's bottom subtree
// (vals[q][2^lb]) and its siblings at the stored levels lb .. n-1 (sib[q][n - lb][8]).  Indices are < 2^n (checked by the host).
template <class F>
__global__ __launch_bounds__(kBlock) void merkle_open_kernel(F f, const u64* __restrict__ values, const u32* __restrict__ levels,
                                                             const u64* __restrict__ index, u32 count, int n, int lb,
                                                             u64* __restrict__ vals, u32* __restrict__ sib) {
  for (u32 q = blockIdx.x * blockDim.x + threadIdx.x; q < count; q += gridDim.x * blockDim.x) {
    const u64 i = index[q];
    const u64 base = (i >> lb) << lb;
    for (u32 j = 0; j < (1u << lb); ++j) vals[((u64)q << lb) + j] = f.from_mont(values[base + j]);
    for (int l = lb; l < n; ++l) {
      const u64 s = (i >> l) ^ 1, off = merkle_level_offset((u64)1 << (n - lb), l - lb);
      u32* dst = sib + ((u64)q * (u64)(n - lb) + (u64)(l - lb)) * 8;
      for (int k = 0; k < 8; ++k) dst[k] = levels[(off + s) * 8 + k];
    }
  }
}

}  // namespace sc
#endif
