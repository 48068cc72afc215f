// SHA-256 as the commitments hash with it (this project's configuration; the reference's test hashes with Pedersen over JubJub,
// DESIGN.md section 9), shared by the Merkle kernels (merkle.hpp), the leaf kernels of pcs.hpp and ligero.hpp, and the host.
//
//   leaf digest  SHA-256(le64(canonical value))   - 8 bytes, what to_uncompressed_bytes gives for an Fp64; never the Montgomery word
//   node digest  SHA-256(left digest || right digest), 64 bytes, at every level (the one above the leaves included)
// In word form SHA-256 reads its message big-endian: a leaf block is W0 = bswap32(lo32), W1 = bswap32(hi32), W2 = 0x80000000,
// W15 = 64, every other word 0; a node's first block is the left digest's 8 words then the right's, no swaps, and its second
// block is the constant padding block (W0 = 0x80000000, W15 = 512), whose schedule the compiler folds into constants.  Digests stay
// 8 u32 words end to end; bytes appear only at the ABI (each word big-endian).  Meant to equal arkworks' MerkleTree with Sha256 as
// both hashes and IdentityDigestConverter - as intent only: byte identity with it is not pinned here.
//
// Plain host + device code: tests/cpp/pcs_host_harness.cpp compiles it with g++, the engine's openings run it on the host.
// field.hpp is here for the integer typedefs and SC_HD alone.
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

}  // namespace sc
