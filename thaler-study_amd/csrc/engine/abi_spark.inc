// Part of sumcheck_hip.hip (included there, in order): SPARK over LogUp (kernels/spark.hpp states the protocol): the sparse matrix on
// the device with its index tables and counts, the gather, the tuples of the two indexed lookups, the cubic sumcheck over three
// arbitrary tables, and two tables the R1CS consumer needs (eq as a table, the row weights of the combined matrix).

struct sc_spark {
  sc_ctx* ctx = nullptr;
  int a = 0, b = 0, l = 0;       // 2^a x 2^b, N = 2^l entries with the padding
  size_t nnz = 0;
  PoolBuf row32, col32;          // the u32 index streams (N entries each, in blocks of u64 words)
  PoolBuf tab[5];                // row, col, val (N words), cr (2^a), cc (2^b): SC_SPARK_ROW .. SC_SPARK_CC
};

namespace {

int check_spark(sc_ctx* ctx, const sc_spark* sp, const char* what) {
  if (!sp || sp->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: not a sparse matrix of this context", what);
  return SC_OK;
}

size_t spark_table_len(const sc_spark* sp, int which) {
  return (size_t)1 << (which == SC_SPARK_CR ? sp->a : which == SC_SPARK_CC ? sp->b : sp->l);
}

// four entries per thread (two: the tail of a table of two)
unsigned spark_grid(const sc_ctx* ctx, size_t n) { return strided_grid(ctx, std::max<size_t>(1, n / 4)); }

// one dimension of the preprocessing: the field-word table of idx and its counts as field words
int spark_index(sc_ctx* ctx, const u32* idx, int l, int log_m, u64* words, u64* counts_out) {
  const size_t n = (size_t)1 << l, m_len = (size_t)1 << log_m;
  PoolBuf work;   // the u32 counters
  SC_TRY(work.alloc(ctx, std::max<size_t>(1, m_len / 2)));
  u32* const counts = reinterpret_cast<u32*>(work.get());
  SC_HIP(ctx, hipMemsetAsync(counts, 0, m_len * sizeof(u32), ctx->stream));
  const bool lds = log_m <= sc::kLookupLdsLog;
  // LDS histograms: a block's flush costs up to 2^m global adds, so few blocks with long runs (two per CU at most)
  const size_t n_units = std::max<size_t>(1, n / 4);
  const unsigned grid = lds ? (unsigned)std::max<u64>(1, std::min<u64>((n_units + 8 * sc::kBlock - 1) / (8 * sc::kBlock), (u64)2 * ctx->num_cus))
                            : strided_grid(ctx, n_units);
  SC_TRY(launch_recorded(ctx, {SC_KIND_SPARK_INDEX, 0, lds ? 1 : 0, l, (u64)4 << l, ((u64)8 << l) + ((u64)4 << log_m)}, "spark_index_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, with_bool(lds, [&](auto LDS) {
      hipLaunchKernelGGL((sc::spark_index_kernel<F, LDS>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, idx, n, log_m, words, counts);
    }));
  }));
  return launch_recorded(ctx, {SC_KIND_SPARK_INDEX, 1, 0, log_m, (u64)4 << log_m, (u64)8 << log_m}, "lookup_mont_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::lookup_mont_kernel<F>), dim3(strided_grid(ctx, m_len)), dim3(sc::kBlock), 0, ctx->stream, f,
                                                    (const u32*)counts, m_len, counts_out));
  });
}

// out = alpha - key - beta v over n entries; key == nullptr: the index itself
int spark_tuples(sc_ctx* ctx, const u32* key, const u64* v, u64 alpha, u64 beta, size_t n, u64* out) {
  const int log_n = log2_of(n);
  return launch_recorded(ctx, {SC_KIND_SPARK_TUPLE, key ? 0 : 1, 0, log_n, (u64)(key ? 12 : 8) << log_n, (u64)8 << log_n}, "spark_tuple_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, with_bool(!key, [&](auto IOTA) {
      hipLaunchKernelGGL((sc::spark_tuple_kernel<F, IOTA>), dim3(spark_grid(ctx, n)), dim3(sc::kBlock), 0, ctx->stream, f, key, v, alpha, beta, n, out);
    }));
  });
}

}  // namespace

extern "C" int sc_spark_create(sc_ctx* ctx, size_t log_rows, size_t log_cols, const uint32_t* row, const uint32_t* col, const uint64_t* val, size_t nnz,
                               sc_spark** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_spark_create"));
  if (!row || !col || !val || !out) return fail(ctx, SC_ERR_ARG, "sc_spark_create: a NULL argument");
  const size_t cap = (size_t)sc::kSparkMaxLog;
  if (log_rows < 1 || log_rows > cap || log_cols < 1 || log_cols > cap)
    return fail(ctx, SC_ERR_ARG, "sc_spark_create: log_rows = %zu and log_cols = %zu must be in 1..%d", log_rows, log_cols, sc::kSparkMaxLog);
  if (nnz < 1 || nnz > ((size_t)1 << sc::kSparkMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_spark_create: %zu entries (at least one, at most 2^%d)", nnz, sc::kSparkMaxLog);
  const int a = (int)log_rows, b = (int)log_cols, l = sc::spark_log_len(nnz), top = std::max(l, std::max(a, b));
  // (not require_cubic_field: one refusal, with one text, for both bounds on p)
  if (ctx->fp.p <= 3 || ctx->fp.p <= ((u64)1 << top))
    return fail(ctx, SC_ERR_UNSUPPORTED, "sc_spark_create: p = %llu: indices and counts of up to 2^%d must be field words, and a cubic through 0, 1, 2, 3 "
                "needs 2 and 3 invertible", (unsigned long long)ctx->fp.p, top);
  const size_t bad = sc::spark_first_bad(row, col, val, nnz, a, b, ctx->fp.p);
  if (bad < nnz)
    return fail(ctx, SC_ERR_ARG, "sc_spark_create: entry %zu is (%u, %u, %llu): outside 2^%d x 2^%d, or not a word below p", bad, row[bad], col[bad],
                (unsigned long long)val[bad], a, b);
  SC_TRY(set_device(ctx));
  std::unique_ptr<sc_spark> sp(new (std::nothrow) sc_spark);
  if (!sp) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  sp->ctx = ctx;
  sp->a = a;
  sp->b = b;
  sp->l = l;
  sp->nnz = nnz;
  const size_t n = (size_t)1 << l;
  std::vector<u32> prow(n), pcol(n);
  std::vector<u64> pval(n);
  sc::spark_pad(row, col, val, nnz, n, prow.data(), pcol.data(), pval.data());
  SC_TRY(sp->row32.alloc(ctx, n / 2));
  SC_TRY(sp->col32.alloc(ctx, n / 2));
  for (int w = 0; w < 5; ++w) SC_TRY(sp->tab[w].alloc(ctx, spark_table_len(sp.get(), w)));
  SC_HIP(ctx, hipMemcpyAsync(sp->row32.get(), prow.data(), n * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(sp->col32.get(), pcol.data(), n * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(sp->tab[SC_SPARK_VAL].get(), pval.data(), n * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
  SC_TRY(spark_index(ctx, reinterpret_cast<const u32*>(sp->row32.get()), l, a, sp->tab[SC_SPARK_ROW].get(), sp->tab[SC_SPARK_CR].get()));
  SC_TRY(spark_index(ctx, reinterpret_cast<const u32*>(sp->col32.get()), l, b, sp->tab[SC_SPARK_COL].get(), sp->tab[SC_SPARK_CC].get()));
  SC_HIP(ctx, sync_stream(ctx));   // (the host vectors go away)
  *out = sp.release();
  return SC_OK;
}

extern "C" int sc_spark_destroy(sc_ctx* ctx, sc_spark* sp) {
  if (!sp) return SC_OK;
  if (!ctx || sp->ctx != ctx) return SC_ERR_ARG;
  delete sp;   // (its blocks go back to the pool)
  return SC_OK;
}

extern "C" int sc_spark_table(sc_ctx* ctx, const sc_spark* sp, int which, sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_spark_table"));
  if (!out) return fail(ctx, SC_ERR_ARG, "sc_spark_table: a NULL argument");
  SC_TRY(check_spark(ctx, sp, "sc_spark_table"));
  if (which < SC_SPARK_ROW || which > SC_SPARK_CC) return fail(ctx, SC_ERR_ARG, "sc_spark_table: which = %d (0: row, 1: col, 2: val, 3: cr, 4: cc)", which);
  SC_TRY(set_device(ctx));
  const size_t len = spark_table_len(sp, which);
  TableBuf t;
  SC_TRY(t.alloc(ctx, len));
  const hipError_t e = hipMemcpyAsync(t->d, sp->tab[which].get(), len * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream);
  return table_done(ctx, t, e, "sc_spark_table", out);
}

extern "C" int sc_spark_gather(sc_ctx* ctx, const sc_spark* sp, const sc_table* u, const sc_table* w, sc_table** er, sc_table** ec) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_spark_gather"));
  if (!u || !w || !er || !ec) return fail(ctx, SC_ERR_ARG, "sc_spark_gather: a NULL argument");
  SC_TRY(check_spark(ctx, sp, "sc_spark_gather"));
  SC_TRY(check_table(ctx, u, "sc_spark_gather"));
  SC_TRY(check_table(ctx, w, "sc_spark_gather"));
  if (u->len != (size_t)1 << sp->a || w->len != (size_t)1 << sp->b)
    return fail(ctx, SC_ERR_ARG, "sc_spark_gather: tables of %zu and %zu entries, the matrix is 2^%d x 2^%d", u->len, w->len, sp->a, sp->b);
  SC_TRY(set_device(ctx));
  const size_t n = (size_t)1 << sp->l;
  TableBuf o[2];
  SC_TRY(o[0].alloc(ctx, n));
  SC_TRY(o[1].alloc(ctx, n));
  SC_TRY(launch_recorded(ctx, {SC_KIND_SPARK_GATHER, 0, 0, sp->l, (u64)24 << sp->l, (u64)16 << sp->l}, "spark_gather_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, {
      (void)f;
      hipLaunchKernelGGL((sc::spark_gather_kernel<F>), dim3(spark_grid(ctx, n)), dim3(sc::kBlock), 0, ctx->stream,
                         reinterpret_cast<const u32*>(sp->row32.get()), reinterpret_cast<const u32*>(sp->col32.get()), (const u64*)u->d, (const u64*)w->d,
                         n, o[0]->d, o[1]->d);
    });
  }));
  SC_HIP(ctx, sync_stream(ctx));
  *er = o[0].release();
  *ec = o[1].release();
  return SC_OK;
}

extern "C" int sc_spark_denominators(sc_ctx* ctx, const sc_spark* sp, int dim, const sc_table* t, const sc_table* e, uint64_t alpha, uint64_t beta,
                                     sc_table** den_w, sc_table** den_t) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_spark_denominators"));
  if (!t || !e || !den_w || !den_t) return fail(ctx, SC_ERR_ARG, "sc_spark_denominators: a NULL argument");
  SC_TRY(check_spark(ctx, sp, "sc_spark_denominators"));
  if (dim != 0 && dim != 1) return fail(ctx, SC_ERR_ARG, "sc_spark_denominators: dim = %d (0: row, 1: col)", dim);
  SC_TRY(check_table(ctx, t, "sc_spark_denominators"));
  SC_TRY(check_table(ctx, e, "sc_spark_denominators"));
  const int log_m = dim ? sp->b : sp->a;
  if (t->len != (size_t)1 << log_m || e->len != (size_t)1 << sp->l)
    return fail(ctx, SC_ERR_ARG, "sc_spark_denominators: tables of %zu and %zu entries, this dimension has 2^%d indices and the list 2^%d entries", t->len,
                e->len, log_m, sp->l);
  if (alpha >= ctx->fp.p || beta >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_spark_denominators: alpha or beta is not a word below p");
  SC_TRY(set_device(ctx));
  TableBuf o[2];
  SC_TRY(o[0].alloc(ctx, e->len));
  SC_TRY(o[1].alloc(ctx, t->len));
  const u32* idx = reinterpret_cast<const u32*>((dim ? sp->col32 : sp->row32).get());
  SC_TRY(spark_tuples(ctx, idx, e->d, alpha, beta, e->len, o[0]->d));
  SC_TRY(spark_tuples(ctx, nullptr, t->d, alpha, beta, t->len, o[1]->d));
  SC_HIP(ctx, sync_stream(ctx));
  *den_w = o[0].release();
  *den_t = o[1].release();
  return SC_OK;
}

extern "C" int sc_product3_prove(sc_ctx* ctx, const sc_table* a, const sc_table* b, const sc_table* c, sc_draw4_fn draw, void* user, uint64_t seed_r,
                                 uint64_t* c1, uint64_t* evals, uint64_t* challenges, uint64_t finals[3]) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_product3_prove"));
  SC_TRY(require_cubic_field(ctx, "sc_product3_prove"));
  if (!c1 || !finals) return fail(ctx, SC_ERR_ARG, "sc_product3_prove: a NULL argument");
  SC_TRY(check_table(ctx, a, "sc_product3_prove"));
  SC_TRY(check_table(ctx, b, "sc_product3_prove"));
  SC_TRY(check_table(ctx, c, "sc_product3_prove"));
  if (a->len != b->len || a->len != c->len || a->len < 2 || a->len > ((size_t)1 << sc::kGpMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_product3_prove: tables of %zu, %zu and %zu entries (equal, at least two, at most 2^%d)", a->len, b->len, c->len,
                sc::kGpMaxLog);
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  const sc::MontGeneric& hfield = hf.f;
  const int n = log2_of(a->len), T = ctx->gp_host_log;

  int rc = SC_OK;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    if (round == 0) *c1 = hf.add(msg[0], msg[1]);
    if (evals) memcpy(evals + 4 * round, msg, 4 * sizeof(u64));
    const u64 r = draw ? draw(user, round, msg) : seeded_challenge(ctx, hf, seed_r, round);
    if (r >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_product3_prove: draw() returned an unreduced challenge");
      return false;
    }
    *out = r;
    return true;
  };

  // the rounds the host runs: all of them over tables of at most 2^T entries, else the tail from what the last launch wrote
  const int te = n <= T ? n : std::max(T, 1);
  const size_t left = (size_t)1 << te;
  std::vector<u64> rs((size_t)n), host[3];
  for (int q = 0; q < 3; ++q) host[q].resize(left);
  PoolBuf cur[3];
  const u64* in[3] = {a->d, b->d, c->d};
  u64 e[4];
  if (n > te) SC_TRY(gp_device_rounds(ctx, n, te, gp_pass_resident(ctx), in, cur, rs.data(), e, &rc, next));
  for (int q = 0; q < 3; ++q) SC_HIP(ctx, hipMemcpyAsync(host[q].data(), in[q], left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  if (!sc::gp_host_rounds(hfield, host[0].data(), host[1].data(), host[2].data(), te, (size_t)(n - te), n > te ? e : nullptr, rs.data(), next)) return rc;
  // (gp_host_rounds leaves the two entries of its first table unfolded in the last round: nobody reads a layer's last E.  Here it
  // is a table like the others)
  finals[0] = hf.add(host[0][0], hf.mul(rs[(size_t)n - 1], hf.sub(host[0][1], host[0][0])));
  finals[1] = host[1][0];
  finals[2] = host[2][0];
  if (challenges) memcpy(challenges, rs.data(), (size_t)n * sizeof(u64));
  return SC_OK;
}

extern "C" int sc_table_eq(sc_ctx* ctx, const uint64_t* r, size_t n, sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_table_eq"));
  if (!r || !out) return fail(ctx, SC_ERR_ARG, "sc_table_eq: a NULL argument");
  if (n < 1 || n > (size_t)sc::kSparkMaxLog) return fail(ctx, SC_ERR_ARG, "sc_table_eq: n = %zu must be in 1..%d", n, sc::kSparkMaxLog);
  for (size_t i = 0; i < n; ++i)
    if (r[i] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_table_eq: r[%zu] is not a word below p", i);
  SC_TRY(set_device(ctx));
  PoolBuf eq;
  SC_TRY(build_eq_table(ctx, r, (int)n, &eq));
  TableBuf t;
  SC_TRY(t.wrap(ctx, std::move(eq), (size_t)1 << n));
  return table_done(ctx, t, hipSuccess, "sc_table_eq", out);
}

extern "C" int sc_r1cs_row_weights(sc_ctx* ctx, const sc_r1cs* r, const uint64_t* rx, const uint64_t rho[3], sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_r1cs_row_weights"));
  if (!rx || !rho || !out) return fail(ctx, SC_ERR_ARG, "sc_r1cs_row_weights: a NULL argument");
  SC_TRY(check_r1cs(ctx, r, "sc_r1cs_row_weights"));
  for (int i = 0; i < r->s; ++i)
    if (rx[i] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_r1cs_row_weights: rx[%d] is not a word below p", i);
  sc::Rho3 w;
  for (int k = 0; k < 3; ++k) {
    if (rho[k] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_r1cs_row_weights: rho[%d] is not a word below p", k);
    w.w[k] = rho[k];
  }
  SC_TRY(set_device(ctx));
  const size_t n = (size_t)1 << r->s;
  PoolBuf eq;
  SC_TRY(build_eq_table(ctx, rx, r->s, &eq));
  TableBuf t;
  SC_TRY(t.alloc(ctx, 4 * n));
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::scale3_kernel<F>), dim3(strided_grid(ctx, n)), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  (const u64*)eq.get(), w, n, t->d));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemsetAsync(t->d + 3 * n, 0, n * sizeof(u64), ctx->stream);
  return table_done(ctx, t, e, "sc_r1cs_row_weights", out);
}
