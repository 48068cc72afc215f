// Part of sumcheck_hip.hip (included there, in order): C ABI: the Ligero-style commitment over the linear-time expander code of
// kernels/expander.hpp, for fields without two-adicity.  Only the encoder differs from engine/abi_ligero.inc: the commitment
// is an ordinary sc_ligero: the combinations and the openings are that file's, the tree engine/merkle.inc's.  The _long entry points
// serve rows longer than the LDS of a CU through the launches of kernels/expander_long.hpp.

namespace {

// the checks sc_xc_encode_rows and sc_ligero_commit_code(SC_CODE_EXPANDER) share with their _long forms; *n = log2 of the table.
// max_log: kXcMaxLogCols (a codeword in the LDS of a CU) or kXcLongMaxLogCols (the launches of kernels/expander_long.hpp)
int xc_shape(sc_ctx* ctx, const sc_table* t, size_t log_cols, const char* what, int* n, int max_log = sc::kXcMaxLogCols) {
  SC_TRY(one_device_only(ctx, what));
  SC_TRY(check_table(ctx, t, what));
  *n = log2_of(t->len);
  if (log_cols > (size_t)*n) return fail(ctx, SC_ERR_ARG, "%s: log_cols = %zu exceeds the table's %d variables", what, log_cols, *n);
  if (log_cols > (size_t)max_log)
    return max_log == sc::kXcMaxLogCols
               ? fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+1) words does not fit the LDS of a CU (at most 2^%d)", what, log_cols,
                      sc::kXcMaxLogCols + 1)
               : fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+1) words is longer than 2^%d (there the stored tree is 1 GiB)", what,
                      log_cols, max_log + 1);
  if (*n + 1 > 29) return fail(ctx, SC_ERR_UNSUPPORTED, "%s: 2^(%d+1) codeword words (at most 2^29)", what, *n);
  if (ctx->fp.p <= 63)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: p = %llu: the base code inverts 1 .. 63 and needs p > 63", what, (unsigned long long)ctx->fp.p);
  return SC_OK;
}

// the inverses 1/1 .. 1/63 of this context's field (the base matrices K[j][k] = 1/(j + k + 1) of every m <= 32), built on the
// host at first use
int xc_inverses(sc_ctx* ctx, const u64** inv) {
  SC_TRY(upload_once(ctx, &ctx->d_xc_inv, sc::kXcInvWords, "base matrix", [&](u64* h) {
    const HostField hf(ctx->fp);
    u64 s = hf.one();
    for (int i = 1; i < sc::kXcInvWords; ++i, s = hf.add(s, hf.one())) h[i] = hf.inv(s);
  }));
  *inv = ctx->d_xc_inv;
  return SC_OK;
}

// E = the encoding of the 2^(n-c) rows of `in`: one launch, every word of `in` read once and every word of E written once
int xc_encode_impl(sc_ctx* ctx, const u64* in, int n, int c, u64* E) {
  const int tile_log = sc::row_tile_log(c + 1, n + 1);
  const u64* inv = nullptr;
  SC_TRY(xc_inverses(ctx, &inv));
  const size_t lds = sc::xc_lds_words(tile_log) * sizeof(u64);
  const unsigned blocks = 1u << (n + 1 - tile_log);
  const int vec = c >= 1 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(E)) & 15) == 0;
  if (lds > 65536)
    SC_DISPATCH_FIELD(ctx, F, f, (void)f; SC_HIP(ctx, allow_dynamic_lds(ctx, kernel_ptr(&sc::xc_encode_rows_kernel<F>),
                                                                         sc::xc_lds_words(sc::kXcMaxLogCols + 1) * sizeof(u64))));
  return launch_recorded(ctx, {SC_KIND_XC_ENCODE, c, sc::xc_levels(c), n, (u64)8 << n, (u64)8 << (n + 1)}, "xc_encode_rows_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::xc_encode_rows_kernel<F>), dim3(blocks), dim3(sc::xc_threads(tile_log)), lds, ctx->stream, f, in, E, inv,
                                         c, tile_log, vec));
  });
}

// E = the encoding of the rows of `in` at any c <= kXcLongMaxLogCols: up to kXcMaxLogCols xc_encode_impl itself, above it the
// launches of kernels/expander_long.hpp on E - the systematic copy, the global levels down, the inner code, the global levels up
int xc_encode_long_impl(sc_ctx* ctx, const u64* in, int n, int c, u64* E) {
  if (c <= sc::kXcMaxLogCols) return xc_encode_impl(ctx, in, n, c, E);
  const sc::XcLongPlan pl = sc::xc_long_plan(c);
  const u64* inv = nullptr;
  SC_TRY(xc_inverses(ctx, &inv));
  const int log_len = c + 1, tile_log = pl.lm_i + 1;
  const u64 R = (u64)1 << (n - c);
  const size_t lds = sc::xc_lds_words(tile_log) * sizeof(u64);
  SC_DISPATCH_FIELD(ctx, F, f, (void)f;
                    SC_HIP(ctx, allow_dynamic_lds(ctx, kernel_ptr(&sc::xc_long_inner_kernel<F>), sc::xc_lds_words(sc::kXcMaxLogCols + 1) * sizeof(u64))));
  const u64 pairs = (u64)1 << (n - 1);
  SC_TRY(launch_recorded(ctx, {SC_KIND_XC_LONG, 0, c, n, (u64)8 << n, (u64)8 << n}, "xc_long_copy_kernel", [&] {
    hipLaunchKernelGGL(sc::xc_long_copy_kernel, dim3((unsigned)(pairs / sc::kBlock)), dim3(sc::kBlock), 0, ctx->stream, in, E, c, pairs);
  }));
  for (int k = 0; k < pl.levels; ++k) {
    const int lm = pl.lm[k];
    SC_TRY(launch_recorded(ctx, {SC_KIND_XC_LONG, 1, lm, n, (8 * R) << lm, (8 * R) << (lm - 2)}, "xc_long_down_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f,
                        hipLaunchKernelGGL((sc::xc_long_down_kernel<F>), dim3((unsigned)((R << (lm - 2)) / sc::kBlock)), dim3(sc::kBlock), 0,
                                           ctx->stream, f, E, log_len, pl.off[k], lm));
    }));
  }
  SC_TRY(launch_recorded(ctx, {SC_KIND_XC_LONG, 2, pl.lm_i, n, (8 * R) << pl.lm_i, (8 * R) << pl.lm_i}, "xc_long_inner_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::xc_long_inner_kernel<F>), dim3((unsigned)R), dim3(sc::xc_threads(tile_log)), lds, ctx->stream, f, E, inv,
                                         log_len, pl.off_i, pl.lm_i));
  }));
  for (int k = pl.levels - 1; k >= 0; --k) {
    const int lm = pl.lm[k];
    SC_TRY(launch_recorded(ctx, {SC_KIND_XC_LONG, 3, lm, n, (8 * R) << (lm - 1), (8 * R) << (lm - 1)}, "xc_long_up_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f,
                        hipLaunchKernelGGL((sc::xc_long_up_kernel<F>), dim3((unsigned)((R << (lm - 1)) / sc::kBlock)), dim3(sc::kBlock), 0,
                                           ctx->stream, f, E, log_len, pl.off[k], lm));
    }));
  }
  return SC_OK;
}

}  // namespace

extern "C" int sc_xc_encode_rows(sc_ctx* ctx, const sc_table* t, size_t log_cols, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  int n = 0;
  SC_TRY(xc_shape(ctx, t, log_cols, "sc_xc_encode_rows", &n));
  SC_TRY(set_device(ctx));
  TableBuf E;
  SC_TRY(E.alloc(ctx, (size_t)2 << n));
  SC_TRY(xc_encode_impl(ctx, t->d, n, (int)log_cols, E->d));
  *out = E.release();
  return SC_OK;
}

extern "C" int sc_ligero_commit_code(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, sc_ligero** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  if (code == SC_CODE_RS) return sc_ligero_commit(ctx, t, log_cols, log_blowup, out);
  if (code != SC_CODE_EXPANDER) return fail(ctx, SC_ERR_ARG, "sc_ligero_commit_code: code %d is neither SC_CODE_RS nor SC_CODE_EXPANDER", code);
  int n = 0;
  SC_TRY(xc_shape(ctx, t, log_cols, "sc_ligero_commit_code", &n));
  if (log_blowup != 1) return fail(ctx, SC_ERR_ARG, "sc_ligero_commit_code: the expander code has rate 1/2: log_blowup is %zu, not 1", log_blowup);
  return ligero_commit_with(ctx, t, n, (int)log_cols, 1, SC_CODE_EXPANDER, [&](u64* E) { return xc_encode_impl(ctx, t->d, n, (int)log_cols, E); }, out);
}

extern "C" int sc_xc_encode_rows_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  int n = 0;
  SC_TRY(xc_shape(ctx, t, log_cols, "sc_xc_encode_rows_long", &n, sc::kXcLongMaxLogCols));
  SC_TRY(set_device(ctx));
  TableBuf E;
  SC_TRY(E.alloc(ctx, (size_t)2 << n));
  SC_TRY(xc_encode_long_impl(ctx, t->d, n, (int)log_cols, E->d));
  *out = E.release();
  return SC_OK;
}

extern "C" int sc_ligero_commit_code_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, sc_ligero** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  if (code == SC_CODE_RS) return sc_ligero_commit_long(ctx, t, log_cols, log_blowup, out);
  if (code != SC_CODE_EXPANDER)
    return fail(ctx, SC_ERR_ARG, "sc_ligero_commit_code_long: code %d is neither SC_CODE_RS nor SC_CODE_EXPANDER", code);
  int n = 0;
  SC_TRY(xc_shape(ctx, t, log_cols, "sc_ligero_commit_code_long", &n, sc::kXcLongMaxLogCols));
  if (log_blowup != 1)
    return fail(ctx, SC_ERR_ARG, "sc_ligero_commit_code_long: the expander code has rate 1/2: log_blowup is %zu, not 1", log_blowup);
  return ligero_commit_with(ctx, t, n, (int)log_cols, 1, SC_CODE_EXPANDER, [&](u64* E) { return xc_encode_long_impl(ctx, t->d, n, (int)log_cols, E); }, out);
}

extern "C" int sc_ligero_code(const sc_ligero* lg, int* code) {
  if (!lg || !code) return SC_ERR_ARG;
  *code = lg->code;
  return SC_OK;
}
