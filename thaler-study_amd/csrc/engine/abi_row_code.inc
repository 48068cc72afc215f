// Part of sumcheck_hip.hip (included there, in order, after both encoders): C ABI: the entry points that encode the rows of a table
// and commit to the columns of the codeword matrix.  A row code is a line of kRowCodes - the Reed-Solomon code of
// engine/abi_ligero.inc, the expander code of engine/abi_expander.inc - and a reach (rows in the LDS of a CU, or longer ones
// through HBM) an argument of its shape check: a further code or reach is added there, not as a further pair of entry points.

namespace {

struct RowCode {
  int id;   // SC_CODE_RS, SC_CODE_EXPANDER
  // every check of a table and a shape, in the order a caller is told; long_rows: the limit of the _long entry points
  int (*shape)(sc_ctx*, const sc_table*, size_t log_cols, size_t log_blowup, bool long_rows, const char* what, int* n);
  // E = the encoding of the rows of `in`, at any length a shape check lets through
  int (*encode)(sc_ctx*, const u64* in, int n, int c, int rho, u64* E);
};

constexpr RowCode kRowCodes[] = {{SC_CODE_RS, rs_shape, rs_encode_long_impl}, {SC_CODE_EXPANDER, xc_shape, xc_encode_long_impl}};

int row_code_of(sc_ctx* ctx, int code, const char* what, const RowCode** rc) {
  for (const RowCode& k : kRowCodes)
    if (k.id == code) {
      *rc = &k;
      return SC_OK;
    }
  return fail(ctx, SC_ERR_ARG, "%s: code %d is neither SC_CODE_RS nor SC_CODE_EXPANDER", what, code);
}

// the codeword matrix of a table, a table of 2^(n + log_blowup) words
int rows_encode(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, bool long_rows, const char* what,
                sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  const RowCode* rc = nullptr;
  int n = 0;
  SC_TRY(row_code_of(ctx, code, what, &rc));
  SC_TRY(rc->shape(ctx, t, log_cols, log_blowup, long_rows, what, &n));
  SC_TRY(set_device(ctx));
  TableBuf E;
  SC_TRY(E.alloc(ctx, (size_t)1 << (n + log_blowup)));
  SC_TRY(rc->encode(ctx, t->d, n, (int)log_cols, (int)log_blowup, E->d));
  *out = E.release();
  return SC_OK;
}

// the commitment to a table: the codeword matrix, then the tree over its columns
int rows_commit(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, bool long_rows, const char* what,
                sc_ligero** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  const RowCode* rc = nullptr;
  int n = 0;
  SC_TRY(row_code_of(ctx, code, what, &rc));
  SC_TRY(rc->shape(ctx, t, log_cols, log_blowup, long_rows, what, &n));
  SC_TRY(set_device(ctx));
  sc_ligero* lg = new (std::nothrow) sc_ligero;
  if (!lg) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  lg->ctx = ctx;
  lg->t = t;
  lg->c = (int)log_cols;
  lg->r = n - lg->c;
  lg->rho = (int)log_blowup;
  lg->code = code;
  int ok = lg->E.alloc(ctx, (size_t)1 << (n + lg->rho));
  if (ok == SC_OK) ok = lg->levels.alloc(ctx, lg->c + lg->rho);
  if (ok == SC_OK) ok = rc->encode(ctx, t->d, n, lg->c, lg->rho, lg->E->d);
  if (ok == SC_OK) ok = ligero_tree_build(ctx, lg);
  if (ok != SC_OK) {
    delete lg;
    return ok;
  }
  *out = lg;
  return SC_OK;
}

}  // namespace

extern "C" int sc_rs_encode_rows(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_table** out) {
  return rows_encode(ctx, t, log_cols, log_blowup, SC_CODE_RS, false, "sc_rs_encode_rows", out);
}

extern "C" int sc_rs_encode_rows_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_table** out) {
  return rows_encode(ctx, t, log_cols, log_blowup, SC_CODE_RS, true, "sc_rs_encode_rows_long", out);
}

extern "C" int sc_xc_encode_rows(sc_ctx* ctx, const sc_table* t, size_t log_cols, sc_table** out) {
  return rows_encode(ctx, t, log_cols, 1, SC_CODE_EXPANDER, false, "sc_xc_encode_rows", out);
}

extern "C" int sc_xc_encode_rows_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, sc_table** out) {
  return rows_encode(ctx, t, log_cols, 1, SC_CODE_EXPANDER, true, "sc_xc_encode_rows_long", out);
}

extern "C" int sc_ligero_commit(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_ligero** out) {
  return rows_commit(ctx, t, log_cols, log_blowup, SC_CODE_RS, false, "sc_ligero_commit", out);
}

extern "C" int sc_ligero_commit_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_ligero** out) {
  return rows_commit(ctx, t, log_cols, log_blowup, SC_CODE_RS, true, "sc_ligero_commit_long", out);
}

// (Reed-Solomon through these two is the plain commit, and reports under its name)
extern "C" int sc_ligero_commit_code(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, sc_ligero** out) {
  return code == SC_CODE_RS ? sc_ligero_commit(ctx, t, log_cols, log_blowup, out)
                            : rows_commit(ctx, t, log_cols, log_blowup, code, false, "sc_ligero_commit_code", out);
}

extern "C" int sc_ligero_commit_code_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, sc_ligero** out) {
  return code == SC_CODE_RS ? sc_ligero_commit_long(ctx, t, log_cols, log_blowup, out)
                            : rows_commit(ctx, t, log_cols, log_blowup, code, true, "sc_ligero_commit_code_long", out);
}

extern "C" int sc_ligero_code(const sc_ligero* lg, int* code) {
  if (!lg || !code) return SC_ERR_ARG;
  *code = lg->code;
  return SC_OK;
}
