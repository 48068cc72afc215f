// Part of sumcheck_hip.hip (included there, in order): the row code for fields without two-adicity - the linear-time expander
// code of kernels/expander.hpp: its shape check, its workspace (the table of inverses) and its encoder, which serves rows longer
// than the LDS of a CU through the launches of kernels/expander_long.hpp.  Only the encoder differs from engine/abi_ligero.inc:
// engine/abi_row_code.inc puts both behind the same entry points, and a commitment over this code is an ordinary sc_ligero.

namespace {

// RowCode::shape of the expander code (engine/abi_row_code.inc): what a table and a shape must satisfy, in the order a caller is
// told; *n = log2 of the table.  Short rows: a codeword in the LDS of a CU; long_rows: the launches of kernels/expander_long.hpp.
// The rate is 1/2: an encode entry point has no log_blowup and passes 1
int xc_shape(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, bool long_rows, const char* what, int* n) {
  SC_TRY(one_device_only(ctx, what));
  SC_TRY(check_table(ctx, t, what));
  *n = log2_of(t->len);
  if (log_cols > (size_t)*n) return fail(ctx, SC_ERR_ARG, "%s: log_cols = %zu exceeds the table's %d variables", what, log_cols, *n);
  if (!long_rows && log_cols > (size_t)sc::kXcMaxLogCols)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+1) words does not fit the LDS of a CU (at most 2^%d)", what, log_cols,
                sc::kXcMaxLogCols + 1);
  if (log_cols > (size_t)sc::kXcLongMaxLogCols)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+1) words is longer than 2^%d (there the stored tree is 1 GiB)", what,
                log_cols, sc::kXcLongMaxLogCols + 1);
  if (*n + 1 > 29) return fail(ctx, SC_ERR_UNSUPPORTED, "%s: 2^(%d+1) codeword words (at most 2^29)", what, *n);
  if (ctx->fp.p <= 63)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: p = %llu: the base code inverts 1 .. 63 and needs p > 63", what, (unsigned long long)ctx->fp.p);
  if (log_blowup != 1) return fail(ctx, SC_ERR_ARG, "%s: the expander code has rate 1/2: log_blowup is %zu, not 1", what, log_blowup);
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

// RowCode::encode: E = the encoding of the rows of `in` at any c <= kXcLongMaxLogCols (rho is 1): up to kXcMaxLogCols xc_encode_impl
// itself, above it the launches of kernels/expander_long.hpp on E - the systematic copy, the global levels down, the inner code,
// the global levels up
int xc_encode_long_impl(sc_ctx* ctx, const u64* in, int n, int c, int /*rho*/, u64* E) {
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
