// Part of sumcheck_hip.hip (included there, in order): C ABI: the relaxed PCS - the prover's grid evaluation and the SHA-256
// Merkle commitment of any table (kernels/pcs.hpp, which states the leaf order and the hashing contract).

using sc::u32;

// A commitment: the stored levels lb .. n of the tree over the 2^n entries of a borrowed table, bottom up, 8 words per node, in
// one pool block.  The levels below lb are recomputed from the table by every opening.
struct sc_merkle_tree {
  const sc_ctx* ctx = nullptr;
  const sc_table* t = nullptr;   // borrowed: must outlive the tree
  int n = 0, lb = 0;
  PoolBuf d_levels;
  uint32_t root[8] = {};
};

namespace {

constexpr size_t kGridMaxPoints = (size_t)1 << 28;   // p^m <= 2^28: N <= 2^28 values (2 GiB)
constexpr size_t kOpenChunk = 4096;                  // openings per launch of merkle_open_kernel

int pcs_one_device(sc_ctx* ctx, const char* what) {
  if (is_multi(ctx) || ctx->world > 1)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: runs on a context of one device and one rank (this one is %s)", what,
                is_multi(ctx) ? "a multi-device handle" : "sharded");
  return SC_OK;
}

int pcs_launched(sc_ctx* ctx, const char* kernel) {
  if (hipGetLastError() != hipSuccess) {
    poison(ctx);
    return fail(ctx, SC_ERR_HIP, "%s launch failed", kernel);
  }
  return SC_OK;
}

unsigned pcs_grid(const sc_ctx* ctx, u64 threads) {
  return (unsigned)std::max<u64>(1, std::min<u64>((threads + sc::kBlock - 1) / sc::kBlock, (u64)8 * ctx->num_cus));
}

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
    SC_TRY(timer_begin(ctx, SC_KIND_GRID_EXTEND, j, (int)m, (int)m, 16 * eb, 8 * eb * p));
    hipLaunchKernelGGL(sc::grid_extend_kernel, dim3(pcs_grid(ctx, eb * runs)), dim3(sc::kBlock), 0, ctx->stream, f, src, dst, (u32)eb, j,
                       runs);
    SC_TRY(pcs_launched(ctx, "grid_extend_kernel"));
    SC_TRY(timer_end(ctx));
    src = dst;
    E *= p;
  }
  return SC_OK;
}

// The leaf kernel up to level lb, one launch per level while a level has more than kMerkleTopNodes nodes, then the rest of the
// tree in one block; the root comes back to the host.
int merkle_build(sc_ctx* ctx, sc_merkle_tree* tr) {
  const int n = tr->n, lb = tr->lb;
  u32* in = reinterpret_cast<u32*>(tr->d_levels.get());
  u64 in_nodes = (u64)1 << (n - lb);
  SC_TRY(timer_begin(ctx, SC_KIND_MERKLE, 0, lb, n, (u64)8 << n, 32 * in_nodes));
  SC_DISPATCH_FIELD(ctx, F, f,
                    hipLaunchKernelGGL((sc::merkle_leaf_kernel<F>), dim3(pcs_grid(ctx, in_nodes)), dim3(sc::kBlock), 0, ctx->stream, f,
                                       (const u64*)tr->t->d, lb, in_nodes, in));
  SC_TRY(pcs_launched(ctx, "merkle_leaf_kernel"));
  SC_TRY(timer_end(ctx));
  int level = lb;
  while (in_nodes > 2 * (u64)sc::kMerkleTopNodes) {
    const u64 nodes = in_nodes / 2;
    u32* out = in + 8 * in_nodes;
    SC_TRY(timer_begin(ctx, SC_KIND_MERKLE, 1, level + 1, n, 32 * in_nodes, 32 * nodes));
    hipLaunchKernelGGL(sc::merkle_level_kernel, dim3(pcs_grid(ctx, nodes)), dim3(sc::kBlock), 0, ctx->stream, (const u32*)in, nodes, out);
    SC_TRY(pcs_launched(ctx, "merkle_level_kernel"));
    SC_TRY(timer_end(ctx));
    in = out;
    in_nodes = nodes;
    ++level;
  }
  if (in_nodes > 1) {
    SC_TRY(timer_begin(ctx, SC_KIND_MERKLE, 2, level + 1, n, 32 * (2 * in_nodes - 2), 32 * (in_nodes - 1)));
    hipLaunchKernelGGL(sc::merkle_top_kernel, dim3(1), dim3(sc::kBlock), 0, ctx->stream, in, (u32)in_nodes);
    SC_TRY(pcs_launched(ctx, "merkle_top_kernel"));
    SC_TRY(timer_end(ctx));
  }
  const u64 total = ((u64)2 << (n - lb)) - 1;
  SC_HIP(ctx, hipMemcpyAsync(tr->root, reinterpret_cast<const u32*>(tr->d_levels.get()) + 8 * (total - 1), 32, hipMemcpyDeviceToHost,
                             ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

void put_digest(uint8_t* out, const u32* w) {   // the ABI's bytes: each word big-endian
  for (int k = 0; k < 8; ++k) {
    out[4 * k] = (uint8_t)(w[k] >> 24);
    out[4 * k + 1] = (uint8_t)(w[k] >> 16);
    out[4 * k + 2] = (uint8_t)(w[k] >> 8);
    out[4 * k + 3] = (uint8_t)w[k];
  }
}

// One opening on the host: the bottom subtree from its 2^lb canonical values (the shared compression function), then the
// stored siblings the device gathered.
void merkle_path_host(int n, int lb, u64 i, const u64* vals, const u32* sib, u64* leaf, uint8_t* path) {
  const u32 per = 1u << lb, li = (u32)(i & (per - 1));
  std::vector<u32> cur(8 * per), next(4 * per);
  for (u32 j = 0; j < per; ++j) sc::sha256_leaf(vals[j], *reinterpret_cast<u32(*)[8]>(&cur[8 * j]));
  *leaf = vals[li];
  for (int l = 0; l < lb; ++l) {
    put_digest(path + 32 * l, &cur[8 * ((li >> l) ^ 1)]);
    for (u32 k = 0; k < (per >> (l + 1)); ++k)
      sc::sha256_node(*reinterpret_cast<const u32(*)[8]>(&cur[16 * k]), *reinterpret_cast<const u32(*)[8]>(&cur[16 * k + 8]),
                      *reinterpret_cast<u32(*)[8]>(&next[8 * k]));
    std::swap(cur, next);
  }
  for (int l = lb; l < n; ++l) put_digest(path + 32 * l, sib + 8 * (l - lb));
}

}  // namespace

// relaxed-pcs/src/lib.rs:166-181 (Prover::new up to the tree): W~ at every point of F^m in the reference's leaf order.
extern "C" int sc_table_extend_grid(sc_ctx* ctx, const sc_table* t, size_t m, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  SC_TRY(pcs_one_device(ctx, "sc_table_extend_grid"));
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
  SC_TRY(pcs_one_device(ctx, "sc_merkle_commit"));
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
  int rc = tr->d_levels.alloc(ctx, 4 * (((size_t)2 << (n - tr->lb)) - 1));
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
  put_digest(root, tr->root);
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
  int rc = SC_OK;
  for (size_t q0 = 0; q0 < count && rc == SC_OK; q0 += chunk) {
    const size_t c = std::min(chunk, count - q0);
    const u64 moved = (u64)c * (8 * per + 32 * ns);
    if (hipMemcpyAsync(d_idx, index + q0, c * sizeof(u64), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
      poison(ctx);
      rc = fail(ctx, SC_ERR_HIP, "sc_merkle_open: copy failed");
      break;
    }
    rc = timer_begin(ctx, SC_KIND_MERKLE, 3, lb, n, moved, moved);
    if (rc != SC_OK) break;
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::merkle_open_kernel<F>), dim3(pcs_grid(ctx, c)), dim3(sc::kBlock), 0, ctx->stream, f,
                                         (const u64*)tr->t->d, reinterpret_cast<const u32*>(tr->d_levels.get()), (const u64*)d_idx, (u32)c, n,
                                         lb, d_vals, d_sib));
    rc = pcs_launched(ctx, "merkle_open_kernel");
    if (rc == SC_OK) rc = timer_end(ctx);
    if (rc != SC_OK) break;
    if (hipMemcpyAsync(hv.data(), d_vals, c * per * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        (ns > 0 && hipMemcpyAsync(hs.data(), d_sib, c * ns * 32, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
      poison(ctx);
      rc = fail(ctx, SC_ERR_HIP, "sc_merkle_open: read-back failed");
      break;
    }
    for (size_t q = 0; q < c; ++q)
      merkle_path_host(n, lb, index[q0 + q], &hv[q * per], &hs[q * ns * 8], &leaves[q0 + q], paths ? paths + (q0 + q) * 32 * n : nullptr);
  }
  return rc;
}

extern "C" int sc_merkle_tree_destroy(sc_ctx* ctx, sc_merkle_tree* tr) {
  if (!tr) return SC_OK;
  if (!ctx || tr->ctx != ctx) return SC_ERR_ARG;
  delete tr;
  return SC_OK;
}
