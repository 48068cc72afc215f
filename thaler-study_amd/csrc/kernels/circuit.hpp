// Part of kernels.hpp (included there, in order): gkr_protocol::circuit::Circuit::evaluate.
#pragma once

namespace sc {

// ------------------------------------------------------------------------------------
// One layer of Circuit::evaluate (gkr-protocol/src/circuit.rs:99-124):
//   out[a] = in[in0[a]] + in[in1[a]]   (type 0, add)    or    in[in0[a]] * in[in1[a]]   (type 1, mul)
// The layer's gate list is ONE block of 32-bit words [type | in0 | in1], each array `stride` words
// long (a multiple of four: every array starts on a 16-byte boundary) - the layout the sparse W
// sumcheck (gkr_sparse_phase1/2_kernel) reads, so a device-resident circuit serves both.
// Per gate: 12 B of gate words streamed once (one 16-byte piece of each array per lane = four
// gates), two gathered 8-B words of the layer below (a table the previous launch just wrote, far
// smaller than the gate stream: mostly cache-served), one 8-B store left cacheable (the next launch
// gathers from it).  Inputs were checked on upload (sc_circuit_create): every index is < the
// length of `in`.  Layers of fewer than four gates go through the scalar tail.
template <class F, bool NT>
__global__ void __launch_bounds__(kBlock)
circuit_layer_kernel(F f, const unsigned* __restrict__ words, size_t n, size_t stride, const u64* __restrict__ in,
                     u64* __restrict__ out) {
  const ull2* type4 = reinterpret_cast<const ull2*>(words);
  const ull2* in04 = reinterpret_cast<const ull2*>(words + stride);
  const ull2* in14 = reinterpret_cast<const ull2*>(words + 2 * stride);
  const size_t groups = n >> 2;
  for (size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (size_t)gridDim.x * kBlock) {
    const ull2 t = ld16<NT>(type4 + g), a = ld16<NT>(in04 + g), b = ld16<NT>(in14 + g);
    const unsigned tt[4] = {(unsigned)t.x, (unsigned)(t.x >> 32), (unsigned)t.y, (unsigned)(t.y >> 32)};
    const unsigned ia[4] = {(unsigned)a.x, (unsigned)(a.x >> 32), (unsigned)a.y, (unsigned)(a.y >> 32)};
    const unsigned ib[4] = {(unsigned)b.x, (unsigned)(b.x >> 32), (unsigned)b.y, (unsigned)(b.y >> 32)};
    u64 x[4], y[4], o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // all eight gathers in flight before the first is used
      x[j] = in[ia[j]];
      y[j] = in[ib[j]];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = tt[j] ? f.mul(x[j], y[j]) : f.add(x[j], y[j]);
    ull2* o4 = reinterpret_cast<ull2*>(out) + 2 * g;
    st16<false>(o4, ull2{o[0], o[1]});
    st16<false>(o4 + 1, ull2{o[2], o[3]});
  }
  if (n < 4 && blockIdx.x == 0 && threadIdx.x < n) {
    const size_t a = threadIdx.x;
    const u64 x = in[words[stride + a]], y = in[words[2 * stride + a]];
    out[a] = words[a] ? f.mul(x, y) : f.add(x, y);
  }
}

}  // namespace sc
