// Stand-alone timing of wfold_pass_kernel<GoldilocksMont, 4, 5> (the fold behind the matrix-core first pass) and of
// wgrid_pass_kernel<., 5> - not part of the product.  Built against ANY copy of the kernel headers (-DKERNELS_HPP='"path"'), so
// two source states run side by side on one box and one set of tables: tools/run_wfbench.sh builds `base` from a saved copy
// and `new` from the tree, the GPU box alternates them.  Every run prints a checksum of the 243 cells and of the folded tables:
// a variant that is faster and wrong shows at once.
//   wfbench <tag> [log ...]      e.g. wfbench new 21 23 25 28
// The clock-aligned write slots of wfold_pass_kernel (kernels/grid_pass.hpp, WfSlots) are settings of one build: WF_SLOTS lists them,
// e.g. WF_SLOTS=0:0:0,800:0:0,800:0:1,800:600:0,800:600:1 WF_ALT=3 wfbench new 28 - every setting on the same tables, in turn.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifndef KERNELS_HPP
#define KERNELS_HPP "../thaler-study_amd/csrc/kernels.hpp"
#endif
#include KERNELS_HPP
using namespace sc;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

__global__ void xor_fold(const u64* t, size_t n, u64* out) {
  u64 acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc ^= t[i] * (2 * i + 1);
  atomicXor((unsigned long long*)out, (unsigned long long)acc);
}

int main(int argc, char** argv) {
  const char* tag = argc > 1 ? argv[1] : "new";
  std::vector<int> logs;
  for (int i = 2; i < argc; ++i) logs.push_back(atoi(argv[i]));
  if (logs.empty()) logs = {25, 28};
  const int max_log = *std::max_element(logs.begin(), logs.end());
  const size_t N = (size_t)1 << max_log;
  u64 *A, *B, *A2, *B2, *P, *GR, *mb, *chk;
  unsigned* T;
  CK(hipMalloc(&A, N * 8)); CK(hipMalloc(&B, N * 8)); CK(hipMalloc(&A2, N / 2)); CK(hipMalloc(&B2, N / 2));
  CK(hipMalloc(&P, (size_t)1024 * kGridChunk * 8)); CK(hipMalloc(&GR, (size_t)32 * kGridChunk * 8));
  CK(hipMalloc(&T, 64 * sizeof(unsigned))); CK(hipMemset(T, 0, 64 * sizeof(unsigned)));
  CK(hipHostMalloc(&mb, kMailboxWords * 8 + 64, hipHostMallocMapped)); memset(mb, 0, kMailboxWords * 8 + 64);
  CK(hipMalloc(&chk, 16));
  GoldilocksMont f;
  hipLaunchKernelGGL((generate_kernel<GoldilocksMont>), dim3(2048), dim3(kBlock), 0, 0, f, (u64)0xA5A5000000000001ull, (u64)0, N, A);
  hipLaunchKernelGGL((generate_kernel<GoldilocksMont>), dim3(2048), dim3(kBlock), 0, 0, f, (u64)0xB6B6000000000002ull, (u64)0, N, B);
  CK(hipDeviceSynchronize());
  int per_cu = 0, cus = 0;
  CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&wfold_pass_kernel<GoldilocksMont, 4, 5, true>), kWfThreads, 0));
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  FoldW fw;
  for (int c = 0; c < 16; ++c) fw.w[c] = 0x9E3779B97F4A7C15ull * (c + 3) % 0xFFFFFFFF00000001ull;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  u64 seq = 0;
  const int reps = getenv("WF_REPS") ? atoi(getenv("WF_REPS")) : 30;
  // slot settings "period:width:stagger" (ticks of 10 ns), comma-separated in WF_SLOTS; "0:0:0" is the kernel without slots.  Headers
  // from before the slots know only that one.  WF_ALT: how often the whole list is gone through (alternations); WF_SHAPE=53:
  // the (5,3) form instead of (4,5)
  struct Setting { unsigned period, width, stagger; };
  std::vector<Setting> settings;
  if (const char* e = getenv("WF_SLOTS")) {
    for (const char* q = e; *q;) {
      Setting st{0, 0, 0};
      if (sscanf(q, "%u:%u:%u", &st.period, &st.width, &st.stagger) != 3) { printf("WF_SLOTS: bad entry at '%s'\n", q); return 1; }
      settings.push_back(st);
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
  }
  if (settings.empty()) settings.push_back(Setting{0, 0, 0});
  const int alt = getenv("WF_ALT") ? atoi(getenv("WF_ALT")) : 1;
  const bool shape53 = getenv("WF_SHAPE") && atoi(getenv("WF_SHAPE")) == 53;
  const int kf = shape53 ? 5 : 4, ks = shape53 ? 3 : 5, n_cells = shape53 ? 27 : 243;
  const u64 r_top = shape53 ? 0x9E3779B97F4A7C15ull * 21 % 0xFFFFFFFF00000001ull : 0;
  for (int lg : logs) {
    const size_t n_tiles = (size_t)1 << (lg - 12);
    const int grid = (int)std::min<size_t>(n_tiles, (size_t)per_cu * cus);
    for (int round = 0; round < alt; ++round) {
      for (const Setting& st : settings) {
#ifndef SC_WFOLD_SLOTS
        if (st.period) continue;
#endif
        std::vector<float> ts;
        for (int r = 0; r < reps + 3; ++r) {
          WgOut wo;
          wo.partials = P; wo.group_rows = GR; wo.tickets = T; wo.mailbox = mb; wo.seq = ++seq; wo.limbs_dev = nullptr;
          CK(hipEventRecord(e0));
#ifdef SC_WFOLD_SLOTS
          WfSlots sl;
          sl.period = st.period; sl.width = st.width; sl.stagger = st.stagger;
          if (shape53) {
            if (st.period) hipLaunchKernelGGL((wfold_pass_kernel<GoldilocksMont, 5, 3, true, true>), dim3(grid), dim3(kWfThreads), 0, 0, f, A, B, A2, B2, fw, r_top, n_tiles, wo, sl);
            else hipLaunchKernelGGL((wfold_pass_kernel<GoldilocksMont, 5, 3, true, false>), dim3(grid), dim3(kWfThreads), 0, 0, f, A, B, A2, B2, fw, r_top, n_tiles, wo, sl);
          } else {
            if (st.period) hipLaunchKernelGGL((wfold_pass_kernel<GoldilocksMont, 4, 5, true, true>), dim3(grid), dim3(kWfThreads), 0, 0, f, A, B, A2, B2, fw, r_top, n_tiles, wo, sl);
            else hipLaunchKernelGGL((wfold_pass_kernel<GoldilocksMont, 4, 5, true, false>), dim3(grid), dim3(kWfThreads), 0, 0, f, A, B, A2, B2, fw, r_top, n_tiles, wo, sl);
          }
#else
          if (shape53) hipLaunchKernelGGL((wfold_pass_kernel<GoldilocksMont, 5, 3, true>), dim3(grid), dim3(kWfThreads), 0, 0, f, A, B, A2, B2, fw, r_top, n_tiles, wo);
          else hipLaunchKernelGGL((wfold_pass_kernel<GoldilocksMont, 4, 5, true>), dim3(grid), dim3(kWfThreads), 0, 0, f, A, B, A2, B2, fw, r_top, n_tiles, wo);
#endif
          CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
          float ms; CK(hipEventElapsedTime(&ms, e0, e1));
          if (r >= 3) ts.push_back(ms);
        }
        std::sort(ts.begin(), ts.end());
        u64 cells = 0;
        for (int c = 0; c < n_cells; ++c) cells ^= mb[kMailboxWide + c] * (2 * c + 1);
        CK(hipMemset(chk, 0, 16));
        hipLaunchKernelGGL(xor_fold, dim3(1024), dim3(256), 0, 0, A2, (size_t)1 << (lg - kf), chk);
        hipLaunchKernelGGL(xor_fold, dim3(1024), dim3(256), 0, 0, B2, (size_t)1 << (lg - kf), chk + 1);
        u64 h[2]; CK(hipMemcpy(h, chk, 16, hipMemcpyDeviceToHost));
        CK(hipMemset(A2, 0, (size_t)8 << (lg - kf))); CK(hipMemset(B2, 0, (size_t)8 << (lg - kf)));   // (the next setting must write every entry itself)
        const double bytes = 16.0 * (double)((size_t)1 << lg) + 16.0 * (double)((size_t)1 << (lg - kf));
        printf("%-6s wfold(%d,%d)@%d grid=%d slots %u:%u:%u : median %.1f us  min %.1f  p90 %.1f -> %.2f TB/s | cells %016llx tables %016llx %016llx seq %s\n", tag, kf, ks,
               lg, grid, st.period, st.width, st.stagger, ts[ts.size() / 2] * 1e3, ts[0] * 1e3, ts[ts.size() * 9 / 10] * 1e3, bytes / (ts[ts.size() / 2] * 1e3) / 1e6,
               (unsigned long long)cells, (unsigned long long)h[0], (unsigned long long)h[1], mb[kMailboxSeq] == seq ? "ok" : "BAD");
        fflush(stdout);
      }
    }
  }
  if (getenv("WF_SLOTS")) return 0;   // (a slots run: the fold pass alone)
  // the five-round pass on cache-resident tables (wgrid_pass_kernel<., 5, false>, kf = 5): the launch behind it in a proof
  for (int lg : {21, 16}) {
    int pc = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, reinterpret_cast<const void*>(&wgrid_pass_kernel<GoldilocksMont, 5, false>), kBlock, 0));
    GridW gw;
    for (int c = 0; c < 32; ++c) gw.w[c] = 0x9E3779B97F4A7C15ull * (c + 5) % 0xFFFFFFFF00000001ull;
    const size_t n_out = (size_t)1 << (lg - 5);
    const size_t n_iter = (n_out + kWgEntries - 1) / kWgEntries;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((n_iter + 3) / 4, std::min(pc * cus, 1024)));
    std::vector<float> ts;
    for (int r = 0; r < reps + 3; ++r) {
      WgOut wo;
      wo.partials = P; wo.group_rows = GR; wo.tickets = T; wo.mailbox = mb; wo.seq = ++seq; wo.limbs_dev = nullptr;
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL((wgrid_pass_kernel<GoldilocksMont, 5, false>), dim3(grid), dim3(kBlock), 0, 0, f, A, B, A2, B2, gw, 5, n_out, wo);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 3) ts.push_back(ms);
    }
    std::sort(ts.begin(), ts.end());
    u64 cells = 0;
    for (int c = 0; c < 243; ++c) cells ^= mb[kMailboxWide + c] * (2 * c + 1);
    printf("%-6s wgrid(5,5)@%d grid=%d: median %.1f us  min %.1f | cells %016llx\n", tag, lg, grid, ts[ts.size() / 2] * 1e3, ts[0] * 1e3, (unsigned long long)cells);
  }
  return 0;
}
