// Part of sumcheck_hip.hip (included there, in order): what the three commitments (engine/abi_pcs.inc, abi_ligero.inc,
// abi_expander.inc; the entry points of the last two: abi_row_code.inc) share on the host: their guards, the one way they launch
// a kernel, and the tree of digests above whatever leaves each of them hashes (kernels/merkle.hpp).

using sc::u32;

namespace {

int one_device_only(sc_ctx* ctx, const char* what) {
  if (is_multi(ctx) || ctx->world > 1)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: runs on a context of one device and one rank (this one is %s)", what,
                is_multi(ctx) ? "a multi-device handle" : "sharded");
  return SC_OK;
}

// blocks of a grid-strided kernel with one item per thread: every wave slot at most (eight blocks per CU)
unsigned strided_grid(const sc_ctx* ctx, u64 threads) {
  return (unsigned)std::max<u64>(1, std::min<u64>((threads + sc::kBlock - 1) / sc::kBlock, (u64)8 * ctx->num_cus));
}

// Record (option "time_kernels": the fields of `r` but ms), launch, check, end: `launch()` performs the launch of `kernel`, a field
// dispatch included
template <class Launch>
int launch_recorded(sc_ctx* ctx, const sc_launch_record& r, const char* kernel, Launch&& launch) {
  SC_TRY(timer_begin(ctx, r.kind, r.kf, r.ks, r.log_in, r.bytes_read, r.bytes_written));
  launch();
  if (hipGetLastError() != hipSuccess) {
    poison(ctx);
    return fail(ctx, SC_ERR_HIP, "%s launch failed", kernel);
  }
  return timer_end(ctx);
}

// More dynamic LDS than a launch gets by default (64 KiB), for the row encoders: asked for once per kernel and context, as the
// most the kernel ever takes (`max_bytes`)
hipError_t allow_dynamic_lds(sc_ctx* ctx, const void* kernel, size_t max_bytes) {
  if (ctx->lds_allowed.count(kernel)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes);
  if (e == hipSuccess) ctx->lds_allowed.insert(kernel);
  return e;
}

// A table of this context that the host builds at first use (workspace like d_points: not a pool block): if *slot is empty,
// `fill(h)` writes its `words` host words and *slot becomes their device copy
template <class Fill>
int upload_once(sc_ctx* ctx, u64** slot, size_t words, const char* what, Fill&& fill) {
  if (*slot) return SC_OK;
  std::vector<u64> h(words);
  fill(h.data());
  u64* d = nullptr;
  SC_HIP(ctx, hipMalloc(&d, words * sizeof(u64)));
  if (hipMemcpy(d, h.data(), words * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    poison(ctx);
    return fail(ctx, SC_ERR_HIP, "%s upload failed", what);
  }
  *slot = d;
  return SC_OK;
}

// The stored levels of a tree, 2^log_bottom nodes at the bottom one, in one pool block: 8 words per node, level l at node
// sc::merkle_level_offset(2^log_bottom, l); and the root, which merkle_finish reads back.
struct MerkleLevels {
  PoolBuf d;
  int log_bottom = 0;
  uint32_t root[8] = {};

  int alloc(sc_ctx* ctx, int log_b) {
    log_bottom = log_b;
    return d.alloc(ctx, 4 * (((size_t)2 << log_b) - 1));
  }
  u32* words() const { return reinterpret_cast<u32*>(d.get()); }
};

// Finish a tree whose bottom stored level has been written: one merkle_level_kernel launch per level while a level has more than
// 2 kMerkleTopNodes nodes, then the rest in one block; the root comes back to the host.  `level` numbers the bottom stored level
// in the launch records, `log_in` is theirs.
int merkle_finish(sc_ctx* ctx, MerkleLevels* t, int level, int log_in) {
  u32* in = t->words();
  u64 in_nodes = (u64)1 << t->log_bottom;
  for (; in_nodes > 2 * (u64)sc::kMerkleTopNodes; in_nodes /= 2, ++level) {
    const u64 nodes = in_nodes / 2;
    u32* out = in + 8 * in_nodes;
    SC_TRY(launch_recorded(ctx, {SC_KIND_MERKLE, 1, level + 1, log_in, 32 * in_nodes, 32 * nodes}, "merkle_level_kernel", [&] {
      hipLaunchKernelGGL(sc::merkle_level_kernel, dim3(strided_grid(ctx, nodes)), dim3(sc::kBlock), 0, ctx->stream, (const u32*)in, nodes, out);
    }));
    in = out;
  }
  if (in_nodes > 1)
    SC_TRY(launch_recorded(ctx, {SC_KIND_MERKLE, 2, level + 1, log_in, 32 * (2 * in_nodes - 2), 32 * (in_nodes - 1)}, "merkle_top_kernel", [&] {
      hipLaunchKernelGGL(sc::merkle_top_kernel, dim3(1), dim3(sc::kBlock), 0, ctx->stream, in, (u32)in_nodes);
    }));
  const u64 root_node = sc::merkle_level_offset((u64)1 << t->log_bottom, t->log_bottom);
  SC_HIP(ctx, hipMemcpyAsync(t->root, t->words() + 8 * root_node, 32, hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

}  // namespace
