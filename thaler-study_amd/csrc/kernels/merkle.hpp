// A binary tree of SHA-256 digests, whatever its leaves are (the Relaxed PCS, pcs.hpp, and the Ligero-style commitments, ligero.hpp,
// hash their own): the layout of the stored levels - bottom up in one run of 8-word nodes, B nodes, then B / 2, .., then the root -
// the kernels that finish a tree whose bottom level has been written, and the host half of an opening.
#pragma once
#include <vector>

#include "sha256.hpp"

namespace sc {

// levels with at most this many nodes are finished by one block (merkle_top_kernel), not by a launch each
constexpr int kMerkleTopNodes = 256;

// Node offset of level l (0 = the bottom stored level, B nodes) among the stored levels: B + B/2 + .. + B >> (l-1).  The root of
// a tree of B = 2^k bottom nodes is node 2B - 2.
template <class T>
SC_HD T merkle_level_offset(T bottom_nodes, int l) {
  return 2 * bottom_nodes - ((2 * bottom_nodes) >> l);
}

// ---- the host half of an opening ----

inline void put_digest(uint8_t* out, const u32* w) {   // the ABI's bytes: each word big-endian
  for (int k = 0; k < 8; ++k) {
    out[4 * k] = (uint8_t)(w[k] >> 24);
    out[4 * k + 1] = (uint8_t)(w[k] >> 16);
    out[4 * k + 2] = (uint8_t)(w[k] >> 8);
    out[4 * k + 3] = (uint8_t)w[k];
  }
}

// Path bytes from the sibling words a device gathered: sib[q][levels][8] become the digests first .. first + levels - 1 of
// the `count` paths of `depth` digests each.
inline void put_paths(uint8_t* paths, int depth, int first, const u32* sib, size_t count, int levels) {
  for (size_t q = 0; q < count; ++q)
    for (int l = 0; l < levels; ++l) put_digest(paths + (q * depth + first + l) * 32, sib + (q * levels + l) * 8);
}

// The levels below lb of one opening, where a tree stores none: the bottom subtree of leaf i is rebuilt from its 2^lb canonical
// values `vals` (the shared compression function).  *leaf = the value of leaf i, path[0 .. 32 lb) = its lb lowest siblings.
inline void merkle_path_host(int lb, u64 i, const u64* vals, u64* leaf, uint8_t* path) {
  const u32 per = 1u << lb, li = (u32)(i & (per - 1));
  std::vector<u32> cur(8 * per), next(4 * per);
  for (u32 j = 0; j < per; ++j) sha256_leaf(vals[j], *reinterpret_cast<u32(*)[8]>(&cur[8 * j]));
  *leaf = vals[li];
  for (int l = 0; l < lb; ++l) {
    put_digest(path + 32 * l, &cur[8 * ((li >> l) ^ 1)]);
    for (u32 k = 0; k < (per >> (l + 1)); ++k)
      sha256_node(*reinterpret_cast<const u32(*)[8]>(&cur[16 * k]), *reinterpret_cast<const u32(*)[8]>(&cur[16 * k + 8]),
                  *reinterpret_cast<u32(*)[8]>(&next[8 * k]));
    std::swap(cur, next);
  }
}

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

}  // namespace sc
#endif
