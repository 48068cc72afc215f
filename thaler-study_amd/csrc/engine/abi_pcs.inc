// Part of sumcheck_hip.hip (included there, in order): C ABI: the relaxed PCS - the prover's grid evaluation (kernels/pcs.hpp, which
// states the leaf order) and the SHA-256 Merkle commitment of any table: its leaves here, the tree above them engine/merkle.inc's.

// A commitment: the stored levels lb .. n of the tree over the 2^n entries of a borrowed table.  The levels below lb are recomputed
// from the table by every opening.
struct sc_merkle_tree {
  const sc_ctx* ctx = nullptr;
  const sc_table* t = nullptr;   // borrowed: must outlive the tree
  int n = 0, lb = 0;
  MerkleLevels levels;   // 2^(n - lb) nodes at the bottom
};

namespace {

constexpr size_t kGridMaxPoints = (size_t)1 << 28;   // p^m <= 2^28: N <= 2^28 values (2 GiB)
constexpr size_t kOpenChunk = 4096;                  // openings per launch of merkle_open_kernel

// One grid_extend_kernel launch per variable, m - 1 first (kernels/pcs.hpp): stage s reads p^s 2^(m-s) words and writes
// p^(s+1) 2^(m-s-1).  The stages alternate between `out` and `scratch` so that the last one writes `out`.
int grid_extend_impl(sc_ctx* ctx, const u64* in, size_t m, u64* out, u64* scratch) {
  const sc::MontGeneric f(ctx->fp);
  const u64 p = ctx->fp.p;
  const u32 runs = (u32)((p + sc::kGridRun - 1) / sc::kGridRun);
  const u64* src = in;
  u64 E = 1;
  for (size_t s = 0; s < m; ++s) {
    const int j = (int)(m - 1 - s);
    const u64 eb = E << j;
    u64* dst = (j % 2 == 0) ? out : scratch;
    SC_TRY(launch_recorded(ctx, {SC_KIND_GRID_EXTEND, j, (int)m, (int)m, 16 * eb, 8 * eb * p}, "grid_extend_kernel", [&] {
      hipLaunchKernelGGL(sc::grid_extend_kernel, dim3(strided_grid(ctx, eb * runs)), dim3(sc::kBlock), 0, ctx->stream, f, src, dst, (u32)eb, j, runs);
    }));
    src = dst;
    E *= p;
  }
  return SC_OK;
}

// The leaf kernel up to level lb, then the tree above it
int merkle_build(sc_ctx* ctx, sc_merkle_tree* tr) {
  const int n = tr->n, lb = tr->lb;
  const u64 subtrees = (u64)1 << (n - lb);
  SC_TRY(launch_recorded(ctx, {SC_KIND_MERKLE, 0, lb, n, (u64)8 << n, 32 * subtrees}, "merkle_leaf_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::merkle_leaf_kernel<F>), dim3(strided_grid(ctx, subtrees)), dim3(sc::kBlock), 0, ctx->stream, f,
                                         (const u64*)tr->t->d, lb, subtrees, tr->levels.words()));
  }));
  return merkle_finish(ctx, &tr->levels, lb, n);
}

}  // namespace

// relaxed-pcs/src/lib.rs:166-181 (Prover::new up to the tree): W~ at every point of F^m in the reference's leaf order.
extern "C" int sc_table_extend_grid(sc_ctx* ctx, const sc_table* t, size_t m, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  SC_TRY(one_device_only(ctx, "sc_table_extend_grid"));
  SC_TRY(check_table(ctx, t, "sc_table_extend_grid"));
  if (m >= 63 || t->len != ((size_t)1 << m))
    return fail(ctx, SC_ERR_ARG, "sc_table_extend_grid: the table has %zu entries, not 2^m = 2^%zu", t->len, m);
  const u64 p = ctx->fp.p;
  size_t pm = 1;
  for (size_t s = 0; s < m; ++s) {
    if (p > kGridMaxPoints / pm)
      return fail(ctx, SC_ERR_UNSUPPORTED, "sc_table_extend_grid: p^m = %llu^%zu points exceed 2^28", (unsigned long long)p, m);
    pm *= p;
  }
  size_t N = 1;
  while (N < pm) N <<= 1;
  SC_TRY(set_device(ctx));
  TableBuf o;
  SC_TRY(o.alloc(ctx, N));
  if (m == 0) {
    if (hipMemcpyAsync(o->d, t->d, sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
      poison(ctx);
      return fail(ctx, SC_ERR_HIP, "sc_table_extend_grid: copy failed");
    }
  } else {
    // the stages that do not write `out` write scratch: the largest of them, p^(s+1) 2^(m-s-1) for m-1-s odd
    size_t scratch_words = 0, E = 1;
    for (size_t s = 0; s < m; ++s) {
      if ((m - 1 - s) % 2 == 1) scratch_words = std::max(scratch_words, (E * p) << (m - 1 - s));
      E *= p;
    }
    PoolBuf scratch;   // (given back at the end of this block: stream-ordered reuse)
    if (scratch_words) SC_TRY(scratch.alloc(ctx, scratch_words));
    SC_TRY(grid_extend_impl(ctx, t->d, m, o->d, scratch));
  }
  if (N > pm && hipMemsetAsync(o->d + pm, 0, (N - pm) * sizeof(u64), ctx->stream) != hipSuccess) {
    poison(ctx);
    return fail(ctx, SC_ERR_HIP, "sc_table_extend_grid: memset failed");
  }
  *out = o.release();
  return SC_OK;
}

// MerkleTree::new over the values (relaxed-pcs/src/lib.rs:185-186), with this project's SHA-256 configuration
extern "C" int sc_merkle_commit(sc_ctx* ctx, const sc_table* t, sc_merkle_tree** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  SC_TRY(one_device_only(ctx, "sc_merkle_commit"));
  SC_TRY(check_table(ctx, t, "sc_merkle_commit"));
  const int n = log2_of(t->len);
  if (n > 28) return fail(ctx, SC_ERR_ARG, "sc_merkle_commit: 2^%d leaves (at most 2^28)", n);
  SC_TRY(set_device(ctx));
  sc_merkle_tree* tr = new (std::nothrow) sc_merkle_tree;
  if (!tr) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  tr->ctx = ctx;
  tr->t = t;
  tr->n = n;
  tr->lb = std::min(n, sc::kMerkleBase);
  int rc = tr->levels.alloc(ctx, n - tr->lb);
  if (rc == SC_OK) rc = merkle_build(ctx, tr);
  if (rc != SC_OK) {
    delete tr;
    return rc;
  }
  *out = tr;
  return SC_OK;
}

// MerkleTree::root (lib.rs:197-199): 32 bytes
extern "C" int sc_merkle_root(const sc_merkle_tree* tr, uint8_t root[32]) {
  if (!tr || !root) return SC_ERR_ARG;
  sc::put_digest(root, tr->levels.root);
  return SC_OK;
}

extern "C" int sc_merkle_depth(const sc_merkle_tree* tr, size_t* depth) {
  if (!tr || !depth) return SC_ERR_ARG;
  *depth = (size_t)tr->n;
  return SC_OK;
}

// MerkleTree::generate_proof for `count` leaves (lib.rs:207-213)
extern "C" int sc_merkle_open(sc_ctx* ctx, const sc_merkle_tree* tr, const uint64_t* index, size_t count, uint64_t* leaves,
                              uint8_t* paths) {
  if (!ctx || !tr) return SC_ERR_ARG;
  if (tr->ctx != ctx) return fail(ctx, SC_ERR_ARG, "sc_merkle_open: the tree belongs to another context");
  if (count == 0) return SC_OK;
  if (!index || !leaves || (!paths && tr->n > 0)) return fail(ctx, SC_ERR_ARG, "sc_merkle_open: null array");
  const int n = tr->n, lb = tr->lb, ns = n - lb;
  const u64 N = (u64)1 << n, per = (u64)1 << lb;
  for (size_t q = 0; q < count; ++q)
    if (index[q] >= N)
      return fail(ctx, SC_ERR_ARG, "sc_merkle_open: index %llu of opening %zu is not below N = 2^%d", (unsigned long long)index[q], q, n);
  SC_TRY(set_device(ctx));
  const size_t chunk = std::min(count, kOpenChunk);
  PoolBuf buf;
  SC_TRY(buf.alloc(ctx, chunk * (1 + per + 4 * (size_t)ns)));
  u64* d_idx = buf;
  u64* d_vals = d_idx + chunk;
  u32* d_sib = reinterpret_cast<u32*>(d_vals + chunk * per);
  std::vector<u64> hv(chunk * per);
  std::vector<u32> hs(std::max<size_t>(1, chunk * ns * 8));
  for (size_t q0 = 0; q0 < count; q0 += chunk) {
    const size_t c = std::min(chunk, count - q0);
    const u64 moved = (u64)c * (8 * per + 32 * ns);
    SC_HIP(ctx, hipMemcpyAsync(d_idx, index + q0, c * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    SC_TRY(launch_recorded(ctx, {SC_KIND_MERKLE, 3, lb, n, moved, moved}, "merkle_open_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f,
                        hipLaunchKernelGGL((sc::merkle_open_kernel<F>), dim3(strided_grid(ctx, c)), dim3(sc::kBlock), 0, ctx->stream, f,
                                           (const u64*)tr->t->d, (const u32*)tr->levels.words(), (const u64*)d_idx, (u32)c, n, lb, d_vals, d_sib));
    }));
    SC_HIP(ctx, hipMemcpyAsync(hv.data(), d_vals, c * per * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    if (ns > 0) SC_HIP(ctx, hipMemcpyAsync(hs.data(), d_sib, c * ns * 32, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the levels below lb from the values, on the host; the stored ones are the gathered siblings
    for (size_t q = 0; q < c; ++q) sc::merkle_path_host(lb, index[q0 + q], &hv[q * per], &leaves[q0 + q], paths + (q0 + q) * 32 * n);
    sc::put_paths(paths + q0 * 32 * n, n, lb, hs.data(), c, ns);
  }
  return SC_OK;
}

extern "C" int sc_merkle_tree_destroy(sc_ctx* ctx, sc_merkle_tree* tr) {
  if (!tr) return SC_OK;
  if (!ctx || tr->ctx != ctx) return SC_ERR_ARG;
  delete tr;
  return SC_OK;
}
