// Part of sumcheck_hip.hip (included there, in order): rank-1 constraint systems (kernels/r1cs.hpp states the protocol): the
// row-sorted images of A, B, C and of [A^T | B^T | C^T], the two sparse products over them, and the cubic sumcheck prover.

namespace {

// A row-sorted sparse matrix on the device: three parallel streams of nnz entries (kernels/r1cs.hpp)
struct SpmvImage {
  PoolBuf row, col, val;   // u32, u32, u64 (the u32 streams live in blocks of u64 words)
  size_t nnz = 0;
  int log_out = 0;         // log2 of the number of rows = of the product's length
};

constexpr int kR1csMaxLog = 26;

}  // namespace

struct sc_r1cs {
  sc_ctx* ctx = nullptr;
  int s = 0, m = 0;
  SpmvImage img[3];   // A, B, C
  SpmvImage imgT;     // [A^T | B^T | C^T]: 2^m rows, column k 2^s + i for entry (i, j) of matrix k
};

namespace {

// the entries (key[e], other[e], val[e]) in stable order of key < n_keys, uploaded as an image of n_keys rows
int upload_image(sc_ctx* ctx, const std::vector<u32>& key, const std::vector<u32>& other, const std::vector<u64>& val, int log_keys, SpmvImage* out) {
  const size_t nnz = key.size(), n_keys = (size_t)1 << log_keys;
  out->nnz = nnz;
  out->log_out = log_keys;
  if (nnz == 0) return SC_OK;
  std::vector<u32> srow(nnz), scol(nnz);
  std::vector<u64> sval(nnz);
  sc::image_sort(key.data(), other.data(), val.data(), nnz, n_keys, srow.data(), scol.data(), sval.data());
  SC_TRY(out->row.alloc(ctx, (nnz + 1) / 2));
  SC_TRY(out->col.alloc(ctx, (nnz + 1) / 2));
  SC_TRY(out->val.alloc(ctx, nnz));
  SC_HIP(ctx, hipMemcpyAsync(out->row.get(), srow.data(), nnz * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(out->col.get(), scol.data(), nnz * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(out->val.get(), sval.data(), nnz * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));   // (the host vectors go away)
  return SC_OK;
}

// y = M v on the stream: y zeroed, the product, the carries (SC_KIND_SPMV records, kf = 0 and 1).  y has 2^log_out words.
int launch_spmv(sc_ctx* ctx, const SpmvImage& M, const u64* v, u64* y, bool transposed) {
  const size_t n_out = (size_t)1 << M.log_out;
  const size_t n_blocks = (M.nnz + sc::kSpmvBlockEntries - 1) / sc::kSpmvBlockEntries;
  PoolBuf carry_row, carry_val;
  if (n_blocks) {
    SC_TRY(carry_row.alloc(ctx, n_blocks));   // 2 n_blocks u32
    SC_TRY(carry_val.alloc(ctx, 2 * n_blocks));
  }
  sc_launch_record rec = {SC_KIND_SPMV, 0, transposed ? 1 : 0, M.log_out, (u64)24 * M.nnz, (u64)8 * n_out + (u64)24 * n_blocks, 0.0};
  hipError_t e = hipSuccess;
  SC_TRY(launch_recorded(ctx, rec, "spmv_kernel", [&] {
    e = hipMemsetAsync(y, 0, n_out * sizeof(u64), ctx->stream);
    if (e != hipSuccess || !n_blocks) return;
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::spmv_kernel<F>), dim3((unsigned)n_blocks), dim3(sc::kSpmvThreads), 0, ctx->stream, f,
                                                    reinterpret_cast<const u32*>(M.row.get()), reinterpret_cast<const u32*>(M.col.get()),
                                                    (const u64*)M.val.get(), M.nnz, v, y, reinterpret_cast<u32*>(carry_row.get()), carry_val.get()));
  }));
  SC_HIP(ctx, e);
  if (!n_blocks) return SC_OK;
  rec.kf = 1;
  rec.bytes_read = (u64)24 * n_blocks;
  rec.bytes_written = (u64)8 * std::min<size_t>(2 * n_blocks, n_out);
  return launch_recorded(ctx, rec, "spmv_carry_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::spmv_carry_kernel<F>), dim3(1), dim3(sc::kSpmvThreads), 0, ctx->stream, f,
                                                    reinterpret_cast<const u32*>(carry_row.get()), (const u64*)carry_val.get(), 2 * n_blocks, y));
  });
}

int check_r1cs(sc_ctx* ctx, const sc_r1cs* r, const char* what) {
  if (!r || r->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: not a constraint system of this context", what);
  return SC_OK;
}

}  // namespace

extern "C" int sc_r1cs_create(sc_ctx* ctx, size_t log_rows, size_t log_cols, const uint32_t* const row[3], const uint32_t* const col[3],
                              const uint64_t* const val[3], const size_t nnz[3], sc_r1cs** out) {
  if (!ctx) return SC_ERR_ARG;
  if (!row || !col || !val || !nnz || !out) return fail(ctx, SC_ERR_ARG, "sc_r1cs_create: a NULL argument");
  SC_TRY(one_device_only(ctx, "sc_r1cs_create"));
  if (log_rows < 1 || log_rows > (size_t)kR1csMaxLog || log_cols < 2 || log_cols > (size_t)kR1csMaxLog)
    return fail(ctx, SC_ERR_ARG, "sc_r1cs_create: log_rows = %zu must be in 1..%d and log_cols = %zu in 2..%d", log_rows, kR1csMaxLog, log_cols,
                kR1csMaxLog);
  const size_t n_rows = (size_t)1 << log_rows, n_cols = (size_t)1 << log_cols;
  for (int k = 0; k < 3; ++k) {
    if (nnz[k] >= ((size_t)1 << 31)) return fail(ctx, SC_ERR_ARG, "sc_r1cs_create: matrix %d has %zu entries, at most 2^31 - 1 are served", k, nnz[k]);
    if (nnz[k] && (!row[k] || !col[k] || !val[k])) return fail(ctx, SC_ERR_ARG, "sc_r1cs_create: matrix %d has entries and a NULL array", k);
    for (size_t e = 0; e < nnz[k]; ++e)
      if (row[k][e] >= n_rows || col[k][e] >= n_cols || val[k][e] >= ctx->fp.p)
        return fail(ctx, SC_ERR_ARG, "sc_r1cs_create: entry %zu of matrix %d is (%u, %u, %llu): outside 2^%zu x 2^%zu, or not a word below p", e, k,
                    row[k][e], col[k][e], (unsigned long long)val[k][e], log_rows, log_cols);
  }
  SC_TRY(set_device(ctx));
  std::unique_ptr<sc_r1cs> r(new (std::nothrow) sc_r1cs);
  if (!r) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  r->ctx = ctx;
  r->s = (int)log_rows;
  r->m = (int)log_cols;
  std::vector<u32> tk, to;
  std::vector<u64> tv;
  for (int k = 0; k < 3; ++k) {
    const std::vector<u32> rk(row[k], row[k] + nnz[k]), ck(col[k], col[k] + nnz[k]);
    const std::vector<u64> vk(val[k], val[k] + nnz[k]);
    SC_TRY(upload_image(ctx, rk, ck, vk, r->s, &r->img[k]));
    tk.insert(tk.end(), ck.begin(), ck.end());
    for (size_t e = 0; e < nnz[k]; ++e) to.push_back((u32)((size_t)k * n_rows + rk[e]));
    tv.insert(tv.end(), vk.begin(), vk.end());
  }
  SC_TRY(upload_image(ctx, tk, to, tv, r->m, &r->imgT));
  *out = r.release();
  return SC_OK;
}

extern "C" int sc_r1cs_destroy(sc_ctx* ctx, sc_r1cs* r) {
  if (!r) return SC_OK;
  if (!ctx || r->ctx != ctx) return SC_ERR_ARG;
  delete r;   // (its blocks go back to the pool)
  return SC_OK;
}

extern "C" int sc_r1cs_mul(sc_ctx* ctx, const sc_r1cs* r, const sc_table* z, sc_table** az, sc_table** bz, sc_table** cz) {
  if (!ctx) return SC_ERR_ARG;
  if (!az || !bz || !cz) return fail(ctx, SC_ERR_ARG, "sc_r1cs_mul: a NULL argument");
  SC_TRY(one_device_only(ctx, "sc_r1cs_mul"));
  SC_TRY(check_r1cs(ctx, r, "sc_r1cs_mul"));
  SC_TRY(check_table(ctx, z, "sc_r1cs_mul"));
  if (z->len != (size_t)1 << r->m) return fail(ctx, SC_ERR_ARG, "sc_r1cs_mul: z has %zu entries, the matrices 2^%d columns", z->len, r->m);
  SC_TRY(set_device(ctx));
  TableBuf t[3];
  for (int k = 0; k < 3; ++k) {
    SC_TRY(t[k].alloc(ctx, (size_t)1 << r->s));
    SC_TRY(launch_spmv(ctx, r->img[k], z->d, t[k]->d, false));
  }
  *az = t[0].release();
  *bz = t[1].release();
  *cz = t[2].release();
  return SC_OK;
}

extern "C" int sc_r1cs_bind_rows(sc_ctx* ctx, const sc_r1cs* r, const uint64_t* rx, const uint64_t rho[3], sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  if (!rx || !rho || !out) return fail(ctx, SC_ERR_ARG, "sc_r1cs_bind_rows: a NULL argument");
  SC_TRY(one_device_only(ctx, "sc_r1cs_bind_rows"));
  SC_TRY(check_r1cs(ctx, r, "sc_r1cs_bind_rows"));
  for (int i = 0; i < r->s; ++i)
    if (rx[i] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_r1cs_bind_rows: rx[%d] is not a word below p", i);
  sc::Rho3 w;
  for (int k = 0; k < 3; ++k) {
    if (rho[k] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_r1cs_bind_rows: rho[%d] is not a word below p", k);
    w.w[k] = rho[k];
  }
  SC_TRY(set_device(ctx));
  const size_t n = (size_t)1 << r->s;
  PoolBuf eq, v;
  SC_TRY(build_eq_table(ctx, rx, r->s, &eq));
  SC_TRY(v.alloc(ctx, 3 * n));
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::scale3_kernel<F>), dim3(strided_grid(ctx, n)), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  (const u64*)eq.get(), w, n, v.get()));
  SC_HIP(ctx, hipGetLastError());
  TableBuf t;
  SC_TRY(t.alloc(ctx, (size_t)1 << r->m));
  SC_TRY(launch_spmv(ctx, r->imgT, v, t->d, true));
  *out = t.release();
  return SC_OK;
}

extern "C" int sc_zerocheck_prove(sc_ctx* ctx, const sc_table* a, const sc_table* b, const sc_table* c, const uint64_t* tau, sc_draw4_fn draw,
                                  void* user, uint64_t seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges, uint64_t finals[3]) {
  if (!ctx) return SC_ERR_ARG;
  if (!tau || !c1 || !finals) return fail(ctx, SC_ERR_ARG, "sc_zerocheck_prove: a NULL argument");
  SC_TRY(one_device_only(ctx, "sc_zerocheck_prove"));
  SC_TRY(require_cubic_field(ctx, "sc_zerocheck_prove"));
  SC_TRY(check_table(ctx, a, "sc_zerocheck_prove"));
  SC_TRY(check_table(ctx, b, "sc_zerocheck_prove"));
  SC_TRY(check_table(ctx, c, "sc_zerocheck_prove"));
  if (a->len != b->len || a->len != c->len || a->len < 2)
    return fail(ctx, SC_ERR_ARG, "sc_zerocheck_prove: tables of %zu, %zu and %zu entries (equal, and at least two)", a->len, b->len, c->len);
  const int s = log2_of(a->len);
  for (int i = 0; i < s; ++i)
    if (tau[i] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_zerocheck_prove: tau[%d] is not a word below p", i);
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  int rc = SC_OK;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    if (round == 0) *c1 = hf.add(msg[0], msg[1]);
    if (evals) memcpy(evals + 4 * round, msg, 4 * sizeof(u64));
    const u64 r = draw ? draw(user, round, msg) : seeded_challenge(ctx, hf, seed_r, round);
    if (r >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_zerocheck_prove: draw() returned an unreduced challenge");
      return false;
    }
    *out = r;
    return true;
  };
  PoolBuf cur[4];
  SC_TRY(build_eq_table(ctx, tau, s, &cur[0]));
  const u64* in[4] = {cur[0].get(), a->d, b->d, c->d};
  const int resident = resident_blocks(ctx, &sc::zc_pass_kernel<sc::GoldilocksMont, true>, &sc::zc_pass_kernel<sc::MontGeneric, true>);
  // every round on the device: the launch of round s - 1 leaves its message and tables of two entries
  u64 own[64];   // (s < 64: a table has 2^s words)
  u64* const rs = challenges ? challenges : own;
  u64 e[4];
  SC_TRY((device_rounds<4, 1, 2>(ctx, 4, s, 1, in, cur, rs, e, &rc, [&](const DeviceRound& d, Launched* l) {
    const bool fold = d.round > 0;
    sc::ZcTables tb;
    for (int k = 0; k < 4; ++k) {
      tb.in[k] = d.in[k];
      tb.out[k] = d.out[k];
    }
    *l = {d.grid(resident), 4};
    SC_TRY(timer_begin(ctx, SC_KIND_ZEROCHECK, fold ? 1 : 0, 1, d.log_in, (u64)32 << d.log_in, fold ? (u64)32 << (d.log_in - 1) : 0));
    SC_DISPATCH_FIELD(ctx, F, f, with_bool(fold, [&](auto FOLD) {
      hipLaunchKernelGGL((sc::zc_pass_kernel<F, FOLD>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, d.r_prev[0], d.n_units, d.po);
    }));
    return SC_OK;
  }, next)));
  u64 r_last = 0;
  if (!next((size_t)s - 1, e, &r_last)) return rc;
  rs[(size_t)s - 1] = r_last;
  // the two entries left of A, B, C, folded by the last challenge on the host
  u64 last[3][2];
  for (int k = 0; k < 3; ++k) SC_HIP(ctx, hipMemcpyAsync(last[k], in[k + 1], 2 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  for (int k = 0; k < 3; ++k) finals[k] = hf.add(last[k][0], hf.mul(r_last, hf.sub(last[k][1], last[k][0])));
  return SC_OK;
}
