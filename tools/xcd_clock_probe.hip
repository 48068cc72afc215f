// Do the wall clocks (wall_clock64, 100 MHz) that different XCDs read agree?  Stand-alone, not part of the product; the
// precondition of clock-aligned write slots in wfold_pass_kernel.
//
// No block waits for another.  Lane 0 of every block draws kDraws tickets from ONE agent-scope counter and stamps the wall clock
// before the add is issued and after its value has returned.  The adds are executed one after the other at the counter's home, so
// the tickets are a chip-wide order of events: for tickets i < j, drawn on XCDs a and b, add i happened before add j, i.e.
//     clock_a - clock_b  >  before_i - after_j
// Over all such pairs this bounds the offset of every pair of XCDs from both sides; the width of the interval is about the round
// trip of an add (1-2 us), which is what "agree" can mean here.  The host prints, per pair of XCDs, the interval in ticks, and
// the widest bound over all pairs.
//   xcd_clock_probe [blocks]      default: one block per CU
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

constexpr int kDraws = 32;
struct Rec {
  unsigned long long before, after;
  unsigned ticket, xcc;
};

__global__ void __launch_bounds__(64) probe(unsigned* counter, Rec* out, unsigned cap) {
  if (threadIdx.x != 0) return;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 7u;
  for (int d = 0; d < kDraws; ++d) {
    unsigned long long t0 = wall_clock64();
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t0) : : "memory");   // the clock read is asynchronous: it has returned before the add is issued
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t1 = wall_clock64();
    if (t < cap) out[t] = Rec{t0, t1, t, xcc};
  }
}

int main(int argc, char** argv) {
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const int blocks = argc > 1 ? std::max(8, std::min(atoi(argv[1]), 1024)) : cus;
  const unsigned cap = (unsigned)blocks * kDraws;
  unsigned* counter;
  Rec* out;
  CK(hipMalloc(&counter, 64));
  CK(hipMalloc(&out, cap * sizeof(Rec)));
  std::vector<Rec> h(cap);
  long long worst_lo = 0, worst_hi = 0;   // over the launches: the widest bounds seen
  for (int rep = 0; rep < 4; ++rep) {     // (the first launch loads the code object: its stamps are as good as any)
    CK(hipMemset(counter, 0, 64));
    CK(hipMemset(out, 0xFF, cap * sizeof(Rec)));
    hipLaunchKernelGGL(probe, dim3(blocks), dim3(64), 0, 0, counter, out, cap);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), out, cap * sizeof(Rec), hipMemcpyDeviceToHost));
    // lo[a][b] = max over tickets i < j, i drawn on a, j on b, of before_i - after_j: clock_a - clock_b > lo[a][b]
    const long long none = -(1ll << 62);
    long long lo[8][8];
    unsigned long long max_before[8];
    bool seen[8] = {};
    int per_xcc[8] = {};
    for (auto& row : lo) for (long long& v : row) v = none;
    unsigned long long rt_sum = 0, rt_max = 0;
    for (unsigned t = 0; t < cap; ++t) {
      const Rec& r = h[t];
      if (r.ticket != t || r.xcc > 7) { printf("record %u missing\n", t); return 1; }
      for (int a = 0; a < 8; ++a)
        if (seen[a]) lo[a][r.xcc] = std::max(lo[a][r.xcc], (long long)(max_before[a] - r.after));
      max_before[r.xcc] = seen[r.xcc] ? std::max(max_before[r.xcc], r.before) : r.before;
      seen[r.xcc] = true;
      per_xcc[r.xcc] += 1;
      rt_sum += r.after - r.before;
      rt_max = std::max(rt_max, r.after - r.before);
    }
    printf("launch %d: %d blocks x %d draws; draws per XCD:", rep, blocks, kDraws);
    for (int a = 0; a < 8; ++a) printf(" %d", per_xcc[a]);
    printf("; round trip of an add: mean %.0f ticks, max %llu (10 ns each)\n", (double)rt_sum / cap, rt_max);
    long long lo_all = 0, hi_all = 0;
    for (int a = 0; a < 8; ++a) {
      if (!seen[a]) continue;
      printf("  clock[%d] - clock[b] in ticks:", a);
      for (int b = 0; b < 8; ++b) {
        if (b == a || !seen[b] || lo[a][b] == none || lo[b][a] == none) { printf("        .      "); continue; }
        printf(" (%5lld,%5lld)", lo[a][b], -lo[b][a]);
        lo_all = std::min(lo_all, lo[a][b]);
        hi_all = std::max(hi_all, -lo[b][a]);
      }
      printf("\n");
    }
    printf("  every pair's offset lies inside (%lld, %lld) ticks\n", lo_all, hi_all);
    // a pair whose interval excludes zero has clocks that provably differ
    for (int a = 0; a < 8; ++a)
      for (int b = 0; b < 8; ++b)
        if (a != b && seen[a] && seen[b] && lo[a][b] > 0) printf("  clock[%d] is AHEAD of clock[%d] by more than %lld ticks\n", a, b, lo[a][b]);
    worst_lo = std::min(worst_lo, lo_all);
    worst_hi = std::max(worst_hi, hi_all);
  }
  printf("xcd_clock_probe: over 4 launches every pair of XCD wall clocks agrees to within (%lld, %lld) ticks = (%.2f, %.2f) us\n", worst_lo,
         worst_hi, worst_lo / 100.0, worst_hi / 100.0);
  return 0;
}
