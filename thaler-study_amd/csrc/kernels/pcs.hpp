// Relaxed PCS (relaxed-pcs/src/lib.rs of the reference): the prover's grid evaluation and its SHA-256 Merkle commitment.
//
// Grid order (IF::all_multidimentional_values, :46-63): the p^m points (v_0, .., v_{m-1}) of F^m sorted lexicographically by
// canonical value, v_0 the most significant digit: the leaf index of a point is o = sum_j v_j p^(m-1-j).  Its value is
// poly.evaluate(point) (:166-170), the dense MLE in LE order: point[0] binds index bit 0 of the table.  So variable 0 has input
// stride 1 but output stride p^(m-1).  The values are padded with zeros to N = 2^ceil(log2 p^m) (:172-177).
//
// Merkle tree (this project's configuration; the reference's test hashes with Pedersen over JubJub):
//   leaf digest  SHA-256(le64(canonical value))   - 8 bytes, what to_uncompressed_bytes gives for an Fp64; never the Montgomery word
//   node digest  SHA-256(left digest || right digest), 64 bytes, at every level (the one above the leaves included)
//   N leaves; the root of a one-leaf tree is that leaf's digest.
// In word form SHA-256 reads its message big-endian: a leaf block is W0 = bswap32(lo32), W1 = bswap32(hi32), W2 = 0x80000000,
// W15 = 64, every other word 0; a node's first block is the left digest's 8 words then the right's, no swaps, and its second
// block is the constant padding block (W0 = 0x80000000, W15 = 512), whose schedule the compiler folds into constants.  Digests stay
// 8 u32 words end to end; bytes appear only at the ABI (each word big-endian).  Meant to equal arkworks' MerkleTree with Sha256 as
// both hashes and IdentityDigestConverter - as intent only: byte identity with it is not pinned here.
//
// The SHA-256 part of this header is plain host + device code (tests/cpp/pcs_host_harness.cpp compiles it with g++, the
// engine's openings run it on the host); the kernels below need hipcc.
#pragma once
#include "../field.hpp"

namespace sc {

SC_HD u32 sha_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }   // constant n: v_alignbit_b32

SC_HD void sha256_init(u32 (&st)[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// One SHA-256 compression of the 16-word block into the chaining value st.  The message schedule is a rolling window of 16
// words and the 64 rounds are unrolled, so every index is a compile-time constant: nothing is indexed at run time (a run-time
// indexed W[64] would live in scratch).
SC_HD void sha256_compress(u32 (&st)[8], const u32 (&blk)[16]) {
  const u32 K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  u32 w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = blk[i];
  u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) {   // w[t] = s1(w[t-2]) + w[t-7] + s0(w[t-15]) + w[t-16], in place of w[t-16]
      const u32 x = w[(t + 1) & 15], y = w[(t + 14) & 15];
      w[t & 15] += (sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3)) + w[(t + 9) & 15] + (sha_rotr(y, 17) ^ sha_rotr(y, 19) ^ (y >> 10));
    }
    const u32 t1 = h + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + (g ^ (e & (f ^ g))) + K[t] + w[t & 15];
    const u32 t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) | (c & (a | b)));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// the padding block of a 64-byte message: a constant, so its schedule and K[t] + W[t] fold into literals
SC_HD void sha256_compress_pad64(u32 (&st)[8]) {
  const u32 pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512u};
  sha256_compress(st, pad);
}

// leaf digest: SHA-256 of the 8 little-endian bytes of the CANONICAL value
SC_HD void sha256_leaf(u64 canonical, u32 (&out)[8]) {
  const u32 blk[16] = {__builtin_bswap32((u32)canonical), __builtin_bswap32((u32)(canonical >> 32)), 0x80000000u, 0, 0, 0, 0, 0,
                       0, 0, 0, 0, 0, 0, 0, 64u};
  sha256_init(out);
  sha256_compress(out, blk);
}

// node digest: SHA-256(left || right), two compressions; out may not alias l or r
SC_HD void sha256_node(const u32 (&l)[8], const u32 (&r)[8], u32 (&out)[8]) {
  u32 blk[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    blk[i] = l[i];
    blk[8 + i] = r[i];
  }
  sha256_init(out);
  sha256_compress(out, blk);
  sha256_compress_pad64(out);
}

// Device footprint: the levels below kMerkleBase are not kept (at N = 2^28 the whole tree would be 16 GiB; from level 4 up it is
// N * 4 bytes); an opening recomputes its 2^kMerkleBase-leaf bottom subtree from the values, on the host.
constexpr int kMerkleBase = 4;
// levels with at most this many nodes are finished by one block (merkle_top_kernel), not by a launch each
constexpr int kMerkleTopNodes = 256;
// sc_table_extend_grid: outputs of one axis chain per thread (one multiplication starts the chain, the rest are additions)
constexpr int kGridRun = 8;

}  // namespace sc

#if defined(__HIPCC__)
namespace sc {

__device__ __forceinline__ void ld_digest(const u32* __restrict__ p, u32 (&d)[8]) {
  const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 4);
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}
__device__ __forceinline__ void st_digest(u32* __restrict__ p, const u32 (&d)[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]);
  *reinterpret_cast<uint4*>(p + 4) = make_uint4(d[4], d[5], d[6], d[7]);
}

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

// one level of the tree: node k = H(in[2k] || in[2k+1]), one node per lane
__global__ __launch_bounds__(kBlock) void merkle_level_kernel(const u32* __restrict__ in, u64 nodes, u32* __restrict__ out) {
  for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < nodes; k += (u64)gridDim.x * blockDim.x) {
    u32 l[8], r[8], d[8];
    ld_digest(in + 16 * k, l);
    ld_digest(in + 16 * k + 8, r);
    sha256_node(l, r, d);
    st_digest(out + 8 * k, d);
  }
}

// The top of the tree in ONE block: `in` holds in_nodes <= 2 kMerkleTopNodes digests, every level above it follows it in memory
// (levels are stored contiguously, bottom up) up to the root.  A barrier between levels makes a level's stores visible to the
// block's reads of the next.
__global__ __launch_bounds__(kBlock) void merkle_top_kernel(u32* in, u32 in_nodes) {
  while (in_nodes > 1) {
    const u32 nodes = in_nodes >> 1;
    u32* out = in + 8 * (u64)in_nodes;
    for (u32 k = threadIdx.x; k < nodes; k += blockDim.x) {
      u32 l[8], r[8], d[8];
      ld_digest(in + 16 * k, l);
      ld_digest(in + 16 * k + 8, r);
      sha256_node(l, r, d);
      st_digest(out + 8 * k, d);
    }
    __syncthreads();
    in = out;
    in_nodes = nodes;
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
    u64 off = 0;   // first node of level l among the stored ones
    for (int l = lb; l < n; ++l) {
      const u64 s = (i >> l) ^ 1;
      u32* dst = sib + ((u64)q * (u64)(n - lb) + (u64)(l - lb)) * 8;
      for (int k = 0; k < 8; ++k) dst[k] = levels[(off + s) * 8 + k];
      off += (u64)1 << (n - l);
    }
  }
}

}  // namespace sc
#endif
