// Host build of the SHA-256 compression in thaler-study_amd/csrc/kernels/sha256.hpp (the function the Merkle kernels and the
// engine's openings share) so that its digests are checked against hashlib on CPU, and timed there as a one-core baseline; and
// of the host half of an opening and the layout of the stored levels (kernels/merkle.hpp).
#include <chrono>

#include "../../thaler-study_amd/csrc/kernels/merkle.hpp"
using namespace sc;
extern "C" {
// out[8 i ..] = words of the leaf digest of canonical[i]
void ph_leaf(const u64* canonical, u32* out, size_t n) {
  for (size_t i = 0; i < n; ++i) sha256_leaf(canonical[i], *reinterpret_cast<u32(*)[8]>(out + 8 * i));
}
// out[8] = node digest of (l, r)
void ph_node(const u32* l, const u32* r, u32* out) {
  sha256_node(*reinterpret_cast<const u32(*)[8]>(l), *reinterpret_cast<const u32(*)[8]>(r), *reinterpret_cast<u32(*)[8]>(out));
}
// root words of the tree over 2^n canonical leaves, bottom up level by level (the host reference the GPU tree is timed against);
// *seconds = the wall time of the hashing
void ph_root(const u64* canonical, int n, u32* root, double* seconds) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t N = (size_t)1 << n;
  u32* lev = new u32[8 * N];
  for (size_t i = 0; i < N; ++i) sha256_leaf(canonical[i], *reinterpret_cast<u32(*)[8]>(lev + 8 * i));
  for (size_t m = N / 2; m >= 1; m /= 2) {
    for (size_t k = 0; k < m; ++k) {
      u32 d[8];
      sha256_node(*reinterpret_cast<const u32(*)[8]>(lev + 16 * k), *reinterpret_cast<const u32(*)[8]>(lev + 16 * k + 8), d);
      for (int w = 0; w < 8; ++w) lev[8 * k + w] = d[w];
    }
  }
  for (int w = 0; w < 8; ++w) root[w] = lev[w];
  delete[] lev;
  *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
// node offset of level l among the stored levels above `bottom_nodes` nodes
u64 ph_level_offset(u64 bottom_nodes, int l) { return merkle_level_offset(bottom_nodes, l); }
// one opening as sc_merkle_open finishes it on the host: vals = the 2^lb canonical values of leaf i's bottom subtree, sib[n - lb][8]
// = its siblings at the stored levels; *leaf and path[32 n]
void ph_path(int n, int lb, u64 i, const u64* vals, const u32* sib, u64* leaf, uint8_t* path) {
  merkle_path_host(lb, i, vals, leaf, path);
  put_paths(path, n, lb, sib, 1, n - lb);
}
}
