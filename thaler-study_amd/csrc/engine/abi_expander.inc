// Part of sumcheck_hip.hip (included there, in order): C ABI: the Ligero-style commitment over the linear-time expander code of
// kernels/expander.hpp, for fields without two-adicity.  Only the encoder differs from engine/abi_ligero.inc: the commitment
// is an ordinary sc_ligero: the combinations and the openings are that file's, the tree engine/merkle.inc's.

namespace {

// the checks sc_xc_encode_rows and sc_ligero_commit_code(SC_CODE_EXPANDER) share; *n = log2 of the table
int xc_shape(sc_ctx* ctx, const sc_table* t, size_t log_cols, const char* what, int* n) {
  SC_TRY(one_device_only(ctx, what));
  SC_TRY(check_table(ctx, t, what));
  *n = log2_of(t->len);
  if (log_cols > (size_t)*n) return fail(ctx, SC_ERR_ARG, "%s: log_cols = %zu exceeds the table's %d variables", what, log_cols, *n);
  if (log_cols > (size_t)sc::kXcMaxLogCols)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^(%zu+1) words does not fit the LDS of a CU (at most 2^%d)", what, log_cols,
                sc::kXcMaxLogCols + 1);
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

extern "C" int sc_ligero_code(const sc_ligero* lg, int* code) {
  if (!lg || !code) return SC_ERR_ARG;
  *code = lg->code;
  return SC_OK;
}
