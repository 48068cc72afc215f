// Part of kernels.hpp (included there, in order): batch_pass_kernel - one grid pass over every instance of a batch of
// independent product sumchecks (sc_prove_batch).
#pragma once

namespace sc {

// ------------------------------------------------------------------------------------
// A batch of B proofs of the same size is B times a small proof: below ~2^21 entries a pass is launch latency and dependent
// memory trips, not bytes (wgrid_pass_kernel above).  One launch here does the pass of EVERY instance: blockIdx.y is the
// instance, blockIdx.x a block of that instance's rows.  Inside an instance the work is exactly wgrid_body's (fold kf <= 5
// pending challenges, the 3^KS cells of the next KS rounds; its row striding reads blockIdx.x / gridDim.x, i.e. the instance's
// own blocks), so every instance's cells are those of its own grid pass.  Per instance the launch reads a BatchDesc from a small
// device array the host copies in before the launch: the tables in and out and the fold weights of that instance's challenges.
//
// Finish: one ticket per instance.  Every block leaves its row of cells in partials[instance][block] (agent-scope, write-through),
// drains its stores - the folded tables' included - and draws the instance's ticket; the instance's last block adds the rows and
// stores the instance's cells to the pinned output (system scope), drains, and draws the batch ticket.  The block that draws
// the batch's last ticket resets it and publishes the sequence word: the host reads every instance's cells after ONE wait.
// Each last block resets its instance's ticket: all counters are zero between launches.
constexpr int kBatchMaxBlocks = 128;   // blocks per instance at most (the instance's last block adds that many rows)
struct BatchDesc {
  const u64* a;   // the instance's tables of 2^log_in entries (the caller's - only read - or the folded ones of the pass before)
  const u64* b;
  u64* a2;        // its folded tables of 2^(log_in - kf) entries (kf > 0)
  u64* b2;
  GridW gw;       // the fold weights of its kf pending challenges
};
struct BatchOut {
  u64* partials;      // [instances][gridDim.x][kGridChunk]
  unsigned* tickets;  // [0]: instances done; [1 + i]: blocks of instance i done; all zero between launches
  u64* cells;         // pinned host memory: [instances][kGridMaxCells]
  u64* mailbox;
  u64 seq;
  int host_out;       // the folded tables are pinned host memory (the host finishes from them): system-scope stores
};

template <class F, int KS>
__device__ __forceinline__ void batch_finish(const F& f, u64 total, const BatchOut& out, int inst) {
  constexpr int kPow3[6] = {1, 3, 9, 27, 81, 243};
  constexpr int cells = kPow3[KS], kLoads = 16;
  __shared__ int lds_flag;
  const int tid = threadIdx.x, n_blocks = gridDim.x;
  const u64* rows = out.partials + (size_t)inst * n_blocks * kGridChunk;
  if (tid < cells)
    __hip_atomic_store(out.partials + ((size_t)inst * n_blocks + blockIdx.x) * kGridChunk + tid, total, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its row and its folded entries have left
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(out.tickets + 1 + inst, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (t == (unsigned)n_blocks - 1) ? 1 : 0;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds_flag = last;
  }
  __syncthreads();
  if (!lds_flag) return;
  if (tid < cells) {   // the instance's rows, kLoads loads in flight at a time
    u64 s = 0;
    for (int q0 = 0; q0 < n_blocks; q0 += kLoads) {
      u64 x[kLoads];
#pragma unroll
      for (int q = 0; q < kLoads; ++q)
        x[q] = (q0 + q < n_blocks) ? __hip_atomic_load(rows + (size_t)(q0 + q) * kGridChunk + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#pragma unroll
      for (int q = 0; q < kLoads; ++q) s = f.add(s, x[q]);
    }
    __hip_atomic_store(out.cells + (size_t)inst * kGridMaxCells + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (tid == 0) __hip_atomic_store(out.tickets + 1 + inst, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the instance's cells have left before its batch ticket is drawn
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(out.tickets, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == gridDim.y - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(out.tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(out.mailbox + kMailboxSeq, out.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <class F, int KS, bool PF>
__global__ void __launch_bounds__(kBlock)
batch_pass_kernel(F f, const BatchDesc* __restrict__ desc, int kf, size_t n_out, BatchOut out) {
  const int inst = blockIdx.y;
  const BatchDesc& d = desc[inst];
  const GridW gw = d.gw;
  const u64 total = wgrid_body<F, KS, PF>(f, d.a, d.b, d.a2, d.b2, gw, kf, n_out, out.host_out != 0);
  batch_finish<F, KS>(f, total, out, inst);
}

}  // namespace sc
