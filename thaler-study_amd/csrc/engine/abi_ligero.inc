// Part of sumcheck_hip.hip (included there, in order): the Ligero-style commitment - the commitment itself (sc_ligero), the
// Reed-Solomon row code (its shape check, its workspace - the field's two-adic root, the twiddle and twist tables - and its encoder,
// which serves rows longer than the LDS of a CU through kernels/ligero_long.hpp), the SHA-256 Merkle tree over the columns of the
// codeword matrix, and the C ABI of what an opening needs: linear combinations of the rows and opened columns (kernels/ligero.hpp
// states the contract).  The tree above the column leaves is engine/merkle.inc's; the entry points that encode and commit, over
// this code or the one of engine/abi_expander.inc, are engine/abi_row_code.inc's.

// A commitment: the codeword matrix E (owned) and every level of the tree over its L columns.
struct sc_ligero {
  const sc_ctx* ctx = nullptr;
  const sc_table* t = nullptr;   // borrowed: must outlive the commitment
  int r = 0, c = 0, rho = 0;
  int code = SC_CODE_RS;         // the row code of E: Reed-Solomon, or the expander code of engine/abi_expander.inc
  TableBuf E;
  MerkleLevels levels;   // L nodes at the bottom
};

namespace {

constexpr size_t kLigeroOpenWords = (size_t)1 << 22;   // column words gathered per launch of column_open_kernel

// s, the 2-adicity of p - 1, and w_max = g^((p-1)/2^s) (Montgomery) for the smallest g >= 2 with g^((p-1)/2) = -1: found at the
// first call on this context and kept on it.  Everything that needs either number asks here
struct TwoAdicRoot { int s; u64 w_max; };
TwoAdicRoot two_adic_root(sc_ctx* ctx) {
  if (!ctx->rs_root_known) {
    const HostField hf(ctx->fp);
    const u64 p = hf.f.p;
    int s = 0;
    while ((((p - 1) >> s) & 1) == 0) ++s;
    const u64 minus_one = hf.neg(hf.one());
    u64 g = hf.add(hf.one(), hf.one());
    while (hf.pow(g, (p - 1) / 2) != minus_one) g = hf.add(g, hf.one());
    ctx->rs_two_adicity = s;
    ctx->rs_w_max = hf.pow(g, (p - 1) >> s);
    ctx->rs_root_known = true;
  }
  return {ctx->rs_two_adicity, ctx->rs_w_max};
}

// RowCode::shape of Reed-Solomon (engine/abi_row_code.inc): what a table and a shape must satisfy, in the order a caller is told;
// *n = log2 of the table.  Short rows: a codeword in the LDS of a CU; long_rows: the two launches of kernels/ligero_long.hpp
int rs_shape(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, bool long_rows, const char* what, int* n) {
  SC_TRY(one_device_only(ctx, what));
  SC_TRY(check_table(ctx, t, what));
  *n = log2_of(t->len);
  if (log_blowup < 1 || log_blowup > 2) return fail(ctx, SC_ERR_ARG, "%s: log_blowup is %zu, not 1 or 2", what, log_blowup);
  if (log_cols > (size_t)*n) return fail(ctx, SC_ERR_ARG, "%s: log_cols = %zu exceeds the table's %d variables", what, log_cols, *n);
  if (!long_rows && log_cols + log_blowup > (size_t)sc::kRsMaxLog)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+%zu) words does not fit the LDS of a CU (at most 2^%d)", what, log_cols,
                log_blowup, sc::kRsMaxLog);
  if (log_cols + log_blowup > (size_t)sc::kRsLongMaxLog)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+%zu) words is longer than 2^%d (there the stored tree is 1 GiB and a tile's strided segments 32 bytes)",
                what, log_cols, log_blowup, sc::kRsLongMaxLog);
  if (*n + log_blowup > 29) return fail(ctx, SC_ERR_UNSUPPORTED, "%s: 2^(%d+%zu) codeword words (at most 2^29)", what, *n, log_blowup);
  const int s = two_adic_root(ctx).s;
  if (log_cols + log_blowup > (size_t)s)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: p = %llu has 2-adicity %d: no root of unity of order 2^(%zu+%zu)", what,
                (unsigned long long)ctx->fp.p, s, log_cols, log_blowup);
  return SC_OK;
}

// the powers w_L^i, i < L/2 (at least one word), of this context, built on the host at first use; and the powers of W16
int rs_twiddles(sc_ctx* ctx, int log_len, const u64** tw, sc::RsRoots* roots) {
  const HostField hf(ctx->fp);
  const TwoAdicRoot root = two_adic_root(ctx);
  const int s = root.s;
  for (int k = 0; k < 8; ++k) {
    // W16^k = w_max^(k 2^s / 16) where the field has that root
    const int tz = k ? __builtin_ctz(k) : 4;
    roots->w16[k] = s + tz >= 4 ? hf.pow(root.w_max, s >= 4 ? (u64)k << (s - 4) : (u64)k >> (4 - s)) : 0;
  }
  SC_TRY(upload_once(ctx, &ctx->d_rs_twiddles[log_len], std::max<size_t>(1, ((size_t)1 << log_len) / 2), "twiddle", [&](u64* h) {
    u64 w = root.w_max;
    for (int k = s; k > log_len; --k) w = hf.mul(w, w);
    h[0] = hf.one();
    for (size_t i = 1; i < ((size_t)1 << log_len) / 2; ++i) h[i] = hf.mul(h[i - 1], w);
  }));
  *tw = ctx->d_rs_twiddles[log_len];
  return SC_OK;
}

// E = the encoding of the 2^(n-c) rows of `in`: one launch, every word of `in` read once and every word of E written once
int rs_encode_impl(sc_ctx* ctx, const u64* in, int n, int c, int rho, u64* E) {
  const int log_len = c + rho, tile_log = sc::row_tile_log(log_len, n + rho);
  const u64* tw = nullptr;
  sc::RsRoots roots;
  SC_TRY(rs_twiddles(ctx, log_len, &tw, &roots));
  const size_t lds = sc::rs_lds_words(tile_log) * sizeof(u64);
  const unsigned blocks = 1u << (n + rho - tile_log);
  const int vec = (tile_log - rho >= 1) && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(E)) & 15) == 0;
  if (lds > 65536)
    SC_DISPATCH_FIELD(ctx, F, f, (void)f; SC_HIP(ctx, allow_dynamic_lds(ctx, kernel_ptr(&sc::rs_encode_rows_kernel<F>),
                                                                         sc::rs_lds_words(sc::kRsMaxLog) * sizeof(u64))));
  return launch_recorded(ctx, {SC_KIND_RS_ENCODE, c, rho, n, (u64)8 << n, (u64)8 << (n + rho)}, "rs_encode_rows_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::rs_encode_rows_kernel<F>), dim3(blocks), dim3(sc::rs_threads(tile_log, sc::rs_max_threads<F>())), lds,
                                         ctx->stream, f, in, E, tw, roots, c, rho, tile_log, vec));
  });
}

// lo[i] = w_L^i, i < 2^12, then hi[i] = w_L^(2^12 i), i < 2^(log_len - 12): the twist tables of this context for L = 2^log_len,
// log_len >= 12, 2^12 + 2^(log_len - 12) host products at first use
int rs_twist_tables(sc_ctx* ctx, int log_len, const u64** lo, const u64** hi) {
  const HostField hf(ctx->fp);
  const size_t n_lo = (size_t)1 << sc::kRsTwistLoLog, n_hi = (size_t)1 << (log_len - sc::kRsTwistLoLog);
  const TwoAdicRoot root = two_adic_root(ctx);
  SC_TRY(upload_once(ctx, &ctx->d_rs_twist[log_len], n_lo + n_hi, "twist table", [&](u64* h) {
    u64 w = root.w_max;
    for (int k = root.s; k > log_len; --k) w = hf.mul(w, w);
    h[0] = hf.one();
    for (size_t i = 1; i < n_lo; ++i) h[i] = hf.mul(h[i - 1], w);
    const u64 step = hf.mul(h[n_lo - 1], w);
    h[n_lo] = hf.one();
    for (size_t i = 1; i < n_hi; ++i) h[n_lo + i] = hf.mul(h[n_lo + i - 1], step);
  }));
  *lo = ctx->d_rs_twist[log_len];
  *hi = *lo + n_lo;
  return SC_OK;
}

// RowCode::encode: E = the encoding of the rows of `in` at any c + rho <= kRsLongMaxLog: up to kRsMaxLog rs_encode_impl itself,
// above it the two launches of kernels/ligero_long.hpp - the column step writes E, the row step transforms it in place
int rs_encode_long_impl(sc_ctx* ctx, const u64* in, int n, int c, int rho, u64* E) {
  const int log_len = c + rho;
  if (log_len <= sc::kRsMaxLog) return rs_encode_impl(ctx, in, n, c, rho, E);
  const sc::RsLongSplit sp = sc::rs_long_split(log_len);
  const u64 *tw_a = nullptr, *tw_b = nullptr, *lo = nullptr, *hi = nullptr;
  sc::RsRoots roots;
  SC_TRY(rs_twiddles(ctx, sp.a, &tw_a, &roots));
  SC_TRY(rs_twiddles(ctx, sp.b, &tw_b, &roots));
  SC_TRY(rs_twist_tables(ctx, log_len, &lo, &hi));
  const size_t lds = sc::rs_lds_words(sp.tile_log) * sizeof(u64);
  const unsigned blocks = (unsigned)sc::rs_long_blocks(sp, n + rho);
  const int vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(E)) & 15) == 0;
  SC_DISPATCH_FIELD(ctx, F, f, (void)f; SC_HIP(ctx, allow_dynamic_lds(ctx, kernel_ptr(&sc::rs_long_column_kernel<F>), lds));
                    SC_HIP(ctx, allow_dynamic_lds(ctx, kernel_ptr(&sc::rs_long_row_kernel<F>), lds)));
  const u64 e_bytes = (u64)8 << (n + rho);
  SC_TRY(launch_recorded(ctx, {SC_KIND_RS_LONG, 0, sp.a, n, (u64)8 << n, e_bytes}, "rs_long_column_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::rs_long_column_kernel<F>), dim3(blocks), dim3(sc::rs_threads(sp.tile_log, sc::rs_max_threads<F>())),
                                         lds, ctx->stream, f, in, E, tw_a, roots, lo, hi, c, rho, vec));
  }));
  return launch_recorded(ctx, {SC_KIND_RS_LONG, 1, sp.b, n, e_bytes, e_bytes}, "rs_long_row_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::rs_long_row_kernel<F>), dim3(blocks), dim3(sc::rs_threads(sp.tile_log, sc::rs_max_threads<F>())), lds,
                                         ctx->stream, f, E, tw_b, roots, log_len, vec));
  });
}

// column_leaf_kernel over E, then the tree above the leaves
int ligero_tree_build(sc_ctx* ctx, sc_ligero* lg) {
  const int depth = lg->c + lg->rho, n = lg->r + lg->c;
  const u64 L = (u64)1 << depth, R = (u64)1 << lg->r;
  SC_TRY(launch_recorded(ctx, {SC_KIND_LIGERO, 0, lg->r, n, 8 * R * L, 32 * L}, "column_leaf_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::column_leaf_kernel<F>), dim3(strided_grid(ctx, L)), dim3(sc::kBlock), 0, ctx->stream, f,
                                         (const u64*)lg->E->d, (u32)R, (u32)L, lg->levels.words()));
  }));
  return merkle_finish(ctx, &lg->levels, 0, depth);
}

int ligero_check(sc_ctx* ctx, const sc_ligero* lg, const char* what) {
  if (lg->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: the commitment belongs to another context", what);
  return SC_OK;
}

}  // namespace

extern "C" int sc_ligero_root(const sc_ligero* lg, uint8_t root[32]) {
  if (!lg || !root) return SC_ERR_ARG;
  sc::put_digest(root, lg->levels.root);
  return SC_OK;
}

extern "C" int sc_ligero_shape(const sc_ligero* lg, size_t* log_rows, size_t* log_cols, size_t* log_blowup) {
  if (!lg || !log_rows || !log_cols || !log_blowup) return SC_ERR_ARG;
  *log_rows = (size_t)lg->r;
  *log_cols = (size_t)lg->c;
  *log_blowup = (size_t)lg->rho;
  return SC_OK;
}

namespace {

// d_out[m][k] = sum_i weights[m][i] w[i C + k], 1 <= count <= kLigeroMaxCombine, left on the device: the weights go to a pool
// buffer, one launch reads the table once (row ranges per block), a second adds the ranges' partial sums.  Queued on the
// context's stream: the caller drains it before `weights` (host memory) goes away
int ligero_combine_device(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* weights, size_t count, PoolBuf* out) {
  const u64 R = (u64)1 << lg->r, C = (u64)1 << lg->c;
  const int V = (lg->c >= 1 && (reinterpret_cast<uintptr_t>(lg->t->d) & 15) == 0) ? 2 : 1;
  const unsigned bx = (unsigned)((C / V + sc::kBlock - 1) / sc::kBlock);
  // row ranges: enough blocks for four per CU, none shorter than 256 rows
  u64 splits = 1;
  while (splits * 2 * bx <= (u64)4 * ctx->num_cus && splits * 2 * 256 <= R && splits < 32768) splits *= 2;
  const u64 rows_per = R / splits, words = count * C;
  PoolBuf d_w, d_part, d_out;
  SC_TRY(d_w.alloc(ctx, count * R));
  SC_TRY(d_out.alloc(ctx, words));
  if (splits > 1) SC_TRY(d_part.alloc(ctx, splits * words));
  SC_HIP(ctx, hipMemcpyAsync(d_w, weights, count * R * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
  u64* part = splits > 1 ? d_part.get() : d_out.get();
  SC_TRY(launch_recorded(ctx, {SC_KIND_LIGERO, 1, (int)count, lg->r + lg->c, 8 * (R * C + count * R), 8 * splits * words}, "row_combine_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3, 4>((int)count, [&](auto M) {
                        with_const<1, 2>(V, [&](auto VV) {
                          hipLaunchKernelGGL((sc::row_combine_kernel<F, M, VV>), dim3(bx, (unsigned)splits), dim3(sc::kBlock), 0, ctx->stream, f,
                                             (const u64*)lg->t->d, (const u64*)d_w.get(), R, rows_per, (sc::u32)C, part);
                        });
                      }));
  }));
  if (splits > 1)
    SC_TRY(launch_recorded(ctx, {SC_KIND_LIGERO, 1, 0, lg->r + lg->c, 8 * splits * words, 8 * words}, "row_combine_sum_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f,
                        hipLaunchKernelGGL((sc::row_combine_sum_kernel<F>), dim3(strided_grid(ctx, words)), dim3(sc::kBlock), 0, ctx->stream, f,
                                           (const u64*)d_part.get(), (sc::u32)splits, (sc::u32)words, d_out.get()));
    }));
  *out = std::move(d_out);
  return SC_OK;
}

}  // namespace

// out[m][k] = sum_i weights[m][i] w[i C + k]: ligero_combine_device, then the rows to the host
extern "C" int sc_ligero_combine_rows(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* weights, size_t count, uint64_t* out) {
  if (!ctx || !lg) return SC_ERR_ARG;
  SC_TRY(ligero_check(ctx, lg, "sc_ligero_combine_rows"));
  if (count > (size_t)sc::kLigeroMaxCombine)
    return fail(ctx, SC_ERR_ARG, "sc_ligero_combine_rows: %zu weight vectors (at most %d per call)", count, sc::kLigeroMaxCombine);
  if (count == 0) return SC_OK;
  if (!weights || !out) return fail(ctx, SC_ERR_ARG, "sc_ligero_combine_rows: null array");
  SC_TRY(set_device(ctx));
  PoolBuf d_out;
  SC_TRY(ligero_combine_device(ctx, lg, weights, count, &d_out));
  const size_t words = count << lg->c;
  SC_HIP(ctx, hipMemcpyAsync(out, d_out, words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SC_OK;
}

// values[q][R] (Montgomery) and paths[q][c+rho][32] of the columns cols[q]
extern "C" int sc_ligero_open_columns(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* cols, size_t count, uint64_t* values,
                                      uint8_t* paths) {
  if (!ctx || !lg) return SC_ERR_ARG;
  SC_TRY(ligero_check(ctx, lg, "sc_ligero_open_columns"));
  if (count == 0) return SC_OK;
  if (!cols || !values || !paths) return fail(ctx, SC_ERR_ARG, "sc_ligero_open_columns: null array");
  const int depth = lg->c + lg->rho;
  const u64 L = (u64)1 << depth, R = (u64)1 << lg->r;
  for (size_t q = 0; q < count; ++q)
    if (cols[q] >= L)
      return fail(ctx, SC_ERR_ARG, "sc_ligero_open_columns: column %llu of opening %zu is not below L = 2^%d", (unsigned long long)cols[q], q,
                  depth);
  SC_TRY(set_device(ctx));
  const size_t chunk = std::min<size_t>(count, std::max<size_t>(1, kLigeroOpenWords / R));
  PoolBuf buf;
  SC_TRY(buf.alloc(ctx, chunk * (1 + R + 4 * (size_t)depth)));
  u64* d_idx = buf;
  u64* d_vals = d_idx + chunk;
  u32* d_sib = reinterpret_cast<u32*>(d_vals + chunk * R);
  std::vector<u32> hs(chunk * depth * 8);
  for (size_t q0 = 0; q0 < count; q0 += chunk) {
    const size_t k = std::min(chunk, count - q0);
    const u64 moved = (u64)k * (8 * R + 32 * depth);
    SC_HIP(ctx, hipMemcpyAsync(d_idx, cols + q0, k * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    SC_TRY(launch_recorded(ctx, {SC_KIND_LIGERO, 2, (int)std::min<size_t>(k, 1u << 30), lg->r + lg->c, moved, moved}, "column_open_kernel", [&] {
      hipLaunchKernelGGL(sc::column_open_kernel, dim3((unsigned)std::min<size_t>(k, (size_t)8 * ctx->num_cus)), dim3(sc::kBlock), 0, ctx->stream,
                         (const u64*)lg->E->d, (const u32*)lg->levels.words(), (const u64*)d_idx, (u32)k, R, (u32)L, depth, d_vals, d_sib);
    }));
    SC_HIP(ctx, hipMemcpyAsync(values + q0 * R, d_vals, k * R * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(hs.data(), d_sib, k * depth * 32, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sc::put_paths(paths + q0 * depth * 32, depth, 0, hs.data(), k, depth);
  }
  return SC_OK;
}

extern "C" int sc_ligero_destroy(sc_ctx* ctx, sc_ligero* lg) {
  if (!lg) return SC_OK;
  if (!ctx || lg->ctx != ctx) return SC_ERR_ARG;
  delete lg;
  return SC_OK;
}
