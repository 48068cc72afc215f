// Part of sumcheck_hip.hip (included there, in order): C ABI: tables and the product of two tables.

// =====================================================================================
// C ABI: tables
// =====================================================================================

extern "C" int sc_table_upload(sc_ctx* ctx, const uint64_t* host, size_t len, sc_table** out) {
  if (!ctx || !host || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_upload(ctx, host, len, out);
  if (!is_pow2(len)) return fail(ctx, SC_ERR_ARG, "sc_table_upload: len %zu is not a power of two", len);
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, len));
  return table_done(ctx, t, hipMemcpyAsync(t->d, host, len * sizeof(u64), hipMemcpyHostToDevice, ctx->stream), "upload", out);
}

// A table over device memory the CALLER owns (built by its own kernels, another library, a virtual-memory mapping it
// arranged itself): borrowed - never written, never freed here (sc_table_free only drops the handle; the pool ignores
// pointers it did not hand out) - and it must stay valid while any table or prover made from it lives.
extern "C" int sc_table_from_device(sc_ctx* ctx, const uint64_t* device_ptr, size_t len, sc_table** out) {
  if (!ctx || !device_ptr || !out) return SC_ERR_ARG;
  SC_NO_MULTI(ctx, "sc_table_from_device");
  if (!is_pow2(len)) return fail(ctx, SC_ERR_ARG, "sc_table_from_device: len %zu is not a power of two", len);
  if (((uintptr_t)device_ptr & 15) != 0 && len > 1) return fail(ctx, SC_ERR_ARG, "sc_table_from_device: the kernels read 16-byte pieces; align the table to 16 bytes");
  SC_TRY(set_device(ctx));
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, device_ptr) != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
    (void)hipGetLastError();
    return fail(ctx, SC_ERR_ARG, "sc_table_from_device: not a device pointer");
  }
  sc_table* t = new (std::nothrow) sc_table;
  if (!t) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  t->d = const_cast<u64*>(device_ptr);
  t->len = len;
  *out = t;
  return SC_OK;
}

extern "C" int sc_table_generate(sc_ctx* ctx, uint64_t seed, uint64_t start, size_t len, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_generate(ctx, seed, start, len, out);
  if (!is_pow2(len)) return fail(ctx, SC_ERR_ARG, "sc_table_generate: len %zu is not a power of two", len);
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, len));
  int grid = grid_for_wide(ctx, len);
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::generate_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream,
                                                  f, (u64)seed, (u64)start, len, t->d));
  return table_done(ctx, t, hipGetLastError(), "generate", out);
}

extern "C" int sc_table_clone(sc_ctx* ctx, const sc_table* t, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_clone(ctx, t, out);
  SC_TRY(check_table(ctx, t, "sc_table_clone"));
  SC_TRY(set_device(ctx));
  TableBuf c;
  SC_TRY(c.alloc(ctx, t->len));
  return table_done(ctx, c, hipMemcpyAsync(c->d, t->d, t->len * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream), "clone", out);
}

extern "C" int sc_table_download(sc_ctx* ctx, const sc_table* t, uint64_t* host, size_t len) {
  if (!ctx || !host) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_download(ctx, t, host, len);
  SC_TRY(check_table(ctx, t, "sc_table_download"));
  if (len != t->len) return fail(ctx, SC_ERR_ARG, "sc_table_download: len %zu != table len %zu", len, t->len);
  SC_TRY(set_device(ctx));
  SC_HIP(ctx, hipMemcpyAsync(host, t->d, len * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  return SC_OK;
}

extern "C" size_t sc_table_len(const sc_table* t) { return t ? t->len : 0; }
extern "C" const uint64_t* sc_table_device_ptr(const sc_table* t) { return t ? t->d : nullptr; }

extern "C" int sc_table_free(sc_ctx* ctx, sc_table* t) {
  if (!t) return SC_OK;
  if (!ctx) return SC_ERR_ARG;
  if (is_multi(ctx) || !t->parts.empty()) return multi_table_free(ctx, t);
  PoolBuf(ctx, t->d).reset();   // the block goes back through its owner, like every other (a borrowed one, sc_table_from_device: ignored)
  delete t;
  return SC_OK;
}

extern "C" int sc_table_fix_variables(sc_ctx* ctx, const sc_table* in, const uint64_t* r, size_t k, int order,
                                      sc_table** out) {
  if (!ctx || !out || (k && !r)) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_fix_variables(ctx, in, r, k, order, out);
  SC_TRY(check_table(ctx, in, "sc_table_fix_variables"));
  if (order != SC_ORDER_LE && order != SC_ORDER_BE) return fail(ctx, SC_ERR_ARG, "bad order %d", order);
  int nv = log2_of(in->len);
  if (k > (size_t)nv) {
    if (ctx->world > 1)
      return fail(ctx, SC_ERR_UNSUPPORTED, "fix_variables of %zu variables crosses shards (local has %d)", k, nv);
    return fail(ctx, SC_ERR_ARG, "fix_variables: k=%zu > num_vars=%d", k, nv);
  }
  if (ctx->world > 1 && order == SC_ORDER_BE && k > 0)
    return fail(ctx, SC_ERR_UNSUPPORTED, "BE fix_variables pairs entries of different shards");
  SC_TRY(set_device(ctx));
  PoolBuf folded;
  size_t folded_len = 0;
  SC_TRY(fold_chain(ctx, in->d, in->len, r, k, order, &folded, &folded_len));
  TableBuf t;
  SC_TRY(t.wrap(ctx, std::move(folded), folded_len));
  // no synchronisation: every consumer of the new table (and every release of the old one) is work on the
  // context's stream, behind these launches; a fault of theirs surfaces at the next call that waits
  *out = t.release();
  return SC_OK;
}

// Local evaluate of a device table at a full LE point, times `w_extra`; leaves the split limbs
// of the result in the mailbox (*from_mailbox) or in ctx->d_sums.
static int evaluate_local(sc_ctx* ctx, const u64* d, size_t len, const u64* pt_le, u64 w_extra, bool across,
                          bool* from_mailbox) {
  const int nv = log2_of(len);
  *from_mailbox = false;
  if (nv < 8) {
    // tiny table: fold chain, then scale into d_sums
    PoolBuf v1;
    size_t out_len = 0;
    SC_TRY(fold_chain(ctx, d, len, pt_le, (size_t)nv, SC_ORDER_LE, &v1, &out_len));
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::scale_split_kernel<F>), dim3(1), dim3(64), 0, ctx->stream, f,
                                                    (const u64*)v1, w_extra, ctx->d_sums));
    v1.reset();
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
  }
  const int ta = std::min(nv - 7, 10);
  // a wave streams 2^chunk_log consecutive 1 KiB tiles: long contiguous runs per wave read faster
  // (n = 28: 409 us with 16 tiles, 382 with 128), as long as there are chunks for every wave.  (Round 3 swept the grid
  // and the chunk size at 2^24 entries - 256 to 1024 blocks, 8 to 128 tiles per chunk: 36.4-38.8 us whatever the shape,
  // profiles/r03_mle24_sweep.txt; at that size the launch is its ~8 us floor plus 22 us of stream.)
  int chunk_log = std::min({ta, 7, std::max(3, nv - 17)});
  sc::RVec rv = make_rvec(pt_le, (size_t)nv);
  int grid = (int)std::min<size_t>(((((size_t)1 << (nv - 7)) >> chunk_log) + 3) / 4, (size_t)std::min(ctx->max_blocks, 1024));
  if (grid < 1) grid = 1;
  // more chunks than one per wave of a four-wave block per CU: one block per CU with all the waves it holds, which draw
  // chunks of 32 tiles from a counter in LDS (kernels.hpp; n = 28: 351 -> 333 us on one box, chunks of 128 tiles 340)
  int threads = sc::kBlock;
  if ((((size_t)1 << (nv - 7)) >> chunk_log) > (size_t)4 * std::min(ctx->num_cus, ctx->max_blocks)) {
    threads = ctx->gold ? sc::stream_block<sc::GoldilocksMont>::evaluate : sc::stream_block<sc::MontGeneric>::evaluate;
    grid = std::min(ctx->num_cus, ctx->max_blocks);
    chunk_log = std::min(chunk_log, 5);
  }
  const sc::PassOut out = next_pass_out(ctx, across, challenge_digest(pt_le, std::min(nv, 3), 0, nv), from_mailbox);
  const int nt = nv >= ctx->nt_load_log ? 1 : 0;
  SC_TRY(timer_begin(ctx, SC_KIND_EVALUATE, nv, 0, nv, (u64)8 << nv, 0));
  SC_DISPATCH_FIELD(ctx, F, f, with_bool(nt, [&](auto NT) {
    hipLaunchKernelGGL((sc::evaluate_kernel<F, NT>), dim3(grid), dim3(threads), 0, ctx->stream, f, d, nv, rv, ta, chunk_log, w_extra, out);
  }));
  SC_TRY(commit_pass_out(ctx, out, grid));
  SC_TRY(timer_end(ctx));
  return SC_OK;
}

// The launch half of sc_table_evaluate on ONE context: this rank's part of the evaluation (its shard at the local
// variables, times the weight of its rank bits) as split limbs, in the mailbox (*mb) or in ctx->d_sums.
static int table_evaluate_launch(sc_ctx* ctx, const u64* d, size_t len, const uint64_t* r, size_t n, int order, bool* mb) {
  if (order != SC_ORDER_LE && order != SC_ORDER_BE) return fail(ctx, SC_ERR_ARG, "bad order %d", order);
  int nl = log2_of(len);
  if (n != (size_t)(nl + ctx->log_world))
    return fail(ctx, SC_ERR_ARG, "evaluate: point has %zu entries, table has %d variables", n, nl + ctx->log_world);
  SC_TRY(set_device(ctx));
  const int g = ctx->log_world;
  // local part: LE -> the low nl variables are r[0..nl); BE -> the shard index is the leading
  // variables r[0..g), the local ones are r[g..n).  A BE evaluate is the LE evaluate at the
  // reversed point (same multilinear polynomial, index bits named in the opposite order).
  std::vector<u64> pt;
  if (order == SC_ORDER_LE) pt.assign(r, r + nl);
  else {
    pt.assign(r + g, r + n);
    std::reverse(pt.begin(), pt.end());
  }
  HostField hf(ctx->fp);
  u64 w = hf.one();
  for (int i = 0; i < g; ++i) {
    // rank bit i (LE) is variable nl+i; in BE order rank bit (g-1-i) is variable i
    u64 ri = (order == SC_ORDER_LE) ? r[nl + i] : r[g - 1 - i];
    bool bit = (ctx->rank >> i) & 1;
    w = hf.mul(w, bit ? ri : hf.sub(hf.one(), ri));
  }
  return evaluate_local(ctx, d, len, pt.data(), w, is_sharded(ctx), mb);
}

extern "C" int sc_table_evaluate(sc_ctx* ctx, const sc_table* t, const uint64_t* r, size_t n, int order,
                                 uint64_t* out) {
  if (!ctx || !out || (n && !r)) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_evaluate(ctx, t, r, n, order, out);
  SC_TRY(check_table(ctx, t, "sc_table_evaluate"));
  bool mb = false;
  SC_TRY(table_evaluate_launch(ctx, t->d, t->len, r, n, order, &mb));
  u64 res = 0;
  SC_TRY(collect_sums(ctx, 1, is_sharded(ctx), mb, &res));
  *out = res;
  return SC_OK;
}

// The launch half of sc_table_evaluate_many on ONE context for a batch of mb <= 16 points: this rank's parts of the mb
// evaluations as 2 M split limbs (M = 4, 8 or 16 >= mb; the padding points carry weight 0), in the mailbox or ctx->d_sums.
static int evaluate_many_launch(sc_ctx* ctx, const u64* d, size_t len, const uint64_t* points, size_t mb, size_t n, int order, int* M_out,
                                bool* from_mailbox) {
  const int nl = log2_of(len), g = ctx->log_world;
  if (n != (size_t)(nl + g)) return fail(ctx, SC_ERR_ARG, "evaluate_many: points have %zu entries, table has %d variables", n, nl + g);
  if (n > 64) return fail(ctx, SC_ERR_ARG, "evaluate_many: more than 64 variables");
  SC_TRY(set_device(ctx));
  if (!ctx->d_points) {
    // (each allocation guarded on its own: a retry after a failed hipMalloc must not allocate - and leak - the staging again)
    if (!ctx->h_points) SC_HIP(ctx, hipHostMalloc(&ctx->h_points, 16 * 64 * sizeof(u64), hipHostMallocDefault));
    SC_HIP(ctx, hipMalloc(&ctx->d_points, 16 * 64 * sizeof(u64)));
  }
  const int M = mb <= 4 ? 4 : mb <= 8 ? 8 : 16;   // (16 only on the Goldilocks kernels: the caller batches by eval_many_batch)
  HostField hf(ctx->fp);
  sc::EvalManyW wx;
  memset(ctx->h_points, 0, (size_t)M * 64 * sizeof(u64));
  for (int j = 0; j < 16; ++j) wx.w[j] = 0;
  for (size_t j = 0; j < mb; ++j) {
    const uint64_t* r = points + j * n;
    u64* pt = ctx->h_points + 64 * j;
    // local part and rank weight exactly as table_evaluate_launch
    if (order == SC_ORDER_LE) for (int i = 0; i < nl; ++i) pt[i] = r[i];
    else for (int i = 0; i < nl; ++i) pt[i] = r[n - 1 - i];
    u64 w = hf.one();
    for (int i = 0; i < g; ++i) {
      const u64 ri = (order == SC_ORDER_LE) ? r[nl + i] : r[g - 1 - i];
      w = hf.mul(w, ((ctx->rank >> i) & 1) ? ri : hf.sub(hf.one(), ri));
    }
    wx.w[j] = w;
  }
  SC_HIP(ctx, hipMemcpyAsync(ctx->d_points, ctx->h_points, (size_t)M * 64 * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
  const sc::PassOut out = next_pass_out(ctx, is_sharded(ctx), challenge_digest(points, (int)std::min<size_t>(n, 3), (int)mb, nl), from_mailbox);
  int grid = 1;
  SC_TRY(timer_begin(ctx, SC_KIND_EVALUATE, nl, (int)mb, nl, (u64)8 << nl, 0));
  if (nl < 8) {
#define SC_EMS(MM) SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::evaluate_many_small_kernel<F, MM>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, \
                                                                     f, d, nl, (const u64*)ctx->d_points, wx, out))
    if (M == 4) SC_EMS(4);
    else if (M == 8) SC_EMS(8);
    else SC_EMS(16);
#undef SC_EMS
  } else {
    const int ta = std::min(nl - 7, sc::kEvalManyTa);
    // at least ~4 chunks per wave of the launch (a wave draws them from the block's counter), at most one segment
    const int chunk_log = std::max(0, std::min(ta, nl - 7 - 14));
    const size_t n_chunks = ((size_t)1 << (nl - 7)) >> chunk_log;
    grid = (int)std::max<size_t>(1, std::min<size_t>((n_chunks + 3) / 4, (size_t)(M == 16 ? 2 : 3) * ctx->num_cus));
    grid = std::min(grid, ctx->max_blocks);
    const bool nt = nl >= ctx->nt_load_log;
#define SC_EM(MM)                                                                                                                  \
  do {                                                                                                                             \
    if (nt) SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::evaluate_many_kernel<F, MM, true>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, \
                                                            f, d, nl, (const u64*)ctx->d_points, ta, chunk_log, wx, out));        \
    else SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::evaluate_many_kernel<F, MM, false>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, \
                                                         f, d, nl, (const u64*)ctx->d_points, ta, chunk_log, wx, out));           \
  } while (0)
    if (M == 4) SC_EM(4);
    else if (M == 8) SC_EM(8);
    else if (!ctx->gold) return fail(ctx, SC_ERR_STATE, "evaluate_many: sixteen points per launch are a Goldilocks instantiation");
    else {   // sixteen nine-register accumulators + the generic field's constants do not fit a wave without spills: Goldilocks only
      typedef sc::GoldilocksMont F;
      F f(ctx->fp);
      if (nt) hipLaunchKernelGGL((sc::evaluate_many_kernel<F, 16, true>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, d, nl,
                                 (const u64*)ctx->d_points, ta, chunk_log, wx, out);
      else hipLaunchKernelGGL((sc::evaluate_many_kernel<F, 16, false>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, d, nl,
                              (const u64*)ctx->d_points, ta, chunk_log, wx, out);
    }
#undef SC_EM
  }
  SC_TRY(commit_pass_out(ctx, out, grid));
  SC_TRY(timer_end(ctx));
  *M_out = M;
  return SC_OK;
}

extern "C" int sc_table_evaluate_many(sc_ctx* ctx, const sc_table* t, const uint64_t* points, size_t m, size_t n, int order,
                                      uint64_t* out) {
  if (!ctx || (m && (!out || (n && !points)))) return SC_ERR_ARG;
  SC_TRY(check_table(ctx, t, "sc_table_evaluate_many"));
  if (order != SC_ORDER_LE && order != SC_ORDER_BE) return fail(ctx, SC_ERR_ARG, "bad order %d", order);
  const size_t eval_many_batch = ctx->gold ? 16 : 8;   // points per launch
  for (size_t done = 0; done < m;) {
    const size_t mb = std::min<size_t>(eval_many_batch, m - done);
    if (mb == 1) {   // a single point: the single-point kernel (two lazy sums per lane instead of one per point)
      SC_TRY(sc_table_evaluate(ctx, t, points + done * n, n, order, out + done));
      done += 1;
      continue;
    }
    u64 res[16];
    if (is_multi(ctx) && t->parts.size() == 1 && ctx->subs.size() > 1) {   // a table that lives on the first device
      const int rc1 = sc_table_evaluate_many(ctx->subs[0], t->parts[0], points + done * n, mb, n, order, res);
      if (rc1 != SC_OK) return fail(ctx, rc1, "%s", ctx->subs[0]->err.c_str());
    } else if (is_multi(ctx)) {
      SC_TRY(multi_enter(ctx));
      // every shard launches with the same M; multi_sums adds the shards' limbs (its ns must be known up front)
      const int M = mb <= 4 ? 4 : mb <= 8 ? 8 : 16;
      SC_TRY(multi_sums(ctx, M, [&](int d, sc_ctx* sub, bool* mbx) {
        int m_d = 0;
        return evaluate_many_launch(sub, t->parts[d]->d, t->parts[d]->len, points + done * n, mb, n, order, &m_d, mbx);
      }, res));
    } else {
      int M = 0;
      bool mbx = false;
      SC_TRY(evaluate_many_launch(ctx, t->d, t->len, points + done * n, mb, n, order, &M, &mbx));
      SC_TRY(collect_sums(ctx, M, is_sharded(ctx), mbx, res));
    }
    memcpy(out + done, res, mb * sizeof(u64));
    done += mb;
  }
  return SC_OK;
}

extern "C" int sc_table_relabel(sc_ctx* ctx, const sc_table* in, size_t a, size_t b, size_t k, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_table_relabel(ctx, in, a, b, k, out);
  SC_TRY(check_table(ctx, in, "sc_table_relabel"));
  if (ctx->world > 1) return fail(ctx, SC_ERR_UNSUPPORTED, "relabel on a sharded table");
  int nv = log2_of(in->len);
  if (a > b) std::swap(a, b);
  if (a + k > b || b + k > (size_t)nv) return fail(ctx, SC_ERR_ARG, "relabel(%zu,%zu,%zu) on %d variables", a, b, k, nv);
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, in->len));
  int grid = grid_for_wide(ctx, in->len);
  hipLaunchKernelGGL(sc::relabel_kernel, dim3(grid), dim3(sc::kBlock), 0, ctx->stream, (const u64*)in->d, t->d, in->len,
                     (unsigned)a, (unsigned)b, (unsigned)k);
  return table_done(ctx, t, hipGetLastError(), "relabel", out);
}

// =====================================================================================
// C ABI: product of two tables
// =====================================================================================

static int check_pair(const sc_ctx* ctx, const sc_table* a, const sc_table* b, const char* what) {
  SC_TRY(check_table(ctx, a, what));
  SC_TRY(check_table(ctx, b, what));
  if (a->len != b->len) return fail(ctx, SC_ERR_ARG, "%s: table lengths differ (%zu vs %zu)", what, a->len, b->len);
  return SC_OK;
}

extern "C" int sc_matmul_g_new(sc_ctx* ctx, const sc_table* A, const sc_table* B, size_t n, const uint64_t* point,
                               sc_table** a_out, sc_table** b_out) {
  if (!ctx || !point || !a_out || !b_out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_matmul_g_new(ctx, A, B, n, point, a_out, b_out);
  SC_TRY(check_pair(ctx, A, B, "sc_matmul_g_new"));
  if (is_sharded(ctx)) {
    // Row-block shards (top log2(world) bits of the row index = rank).  f_b = B~(z, r2) has
    // z = row, so the local rows ARE this rank's shard of f_b: no exchange.  f_a = A~(r1, z)
    // has z = column and sums over rows: every rank holds a partial vector over all columns;
    // they are summed as 32-bit limbs (one all-reduce of 2*2^n words) and each rank keeps
    // its own column range.  (SURVEY.md section 8e, "G::new".)
    SC_TRY(set_device(ctx));
    const int g = ctx->log_world;
    if (n < (size_t)g) return fail(ctx, SC_ERR_ARG, "sc_matmul_g_new: 2^%zu rows cannot be split over %d ranks", n, ctx->world);
    const size_t side = (size_t)1 << n, rows_local = side >> g;
    if (A->len != rows_local * side) return fail(ctx, SC_ERR_ARG, "sc_matmul_g_new: shard must hold 2^(2n)/world entries");
    if (side < 2) return fail(ctx, SC_ERR_UNSUPPORTED, "sc_matmul_g_new: sharded 1x1 matrices");
    TableBuf tb, ta;               // (given back in the order of the declarations read upwards: eq, partial, limbs, then the tables)
    PoolBuf fb, limbs, partial, eq;
    size_t fb_len = 0;
    SC_TRY(build_eq_table(ctx, point, (int)n, &eq));
    SC_TRY(partial.alloc(ctx, side));
    SC_TRY(limbs.alloc(ctx, 2 * side));
    SC_TRY(coldot(ctx, A->d, eq + (size_t)ctx->rank * rows_local, rows_local, side, partial));
    hipLaunchKernelGGL(sc::split_limbs_kernel, dim3(grid_for(ctx, side)), dim3(sc::kBlock), 0, ctx->stream,
                       (const u64*)partial, side, limbs.get());
    SC_TRY(allreduce_device(ctx, limbs, 2 * side));
    SC_TRY(ta.alloc(ctx, rows_local));
    const u64* mine = limbs + 2 * (size_t)ctx->rank * rows_local;
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::recombine_limbs_kernel<F>), dim3(grid_for(ctx, rows_local)),
                                                    dim3(sc::kBlock), 0, ctx->stream, f, mine, rows_local, ta->d));
    if (hipGetLastError() != hipSuccess) return fail(ctx, SC_ERR_HIP, "recombine_limbs_kernel launch failed");
    SC_TRY(fold_chain(ctx, B->d, B->len, point + n, n, SC_ORDER_LE, &fb, &fb_len));
    SC_TRY(tb.wrap(ctx, std::move(fb), fb_len));
    if (sync_stream(ctx) != hipSuccess) return fail(ctx, SC_ERR_HIP, "g_new: sync failed");
    *a_out = ta.release();
    *b_out = tb.release();
    return SC_OK;
  }
  if (A->len != ((size_t)1 << (2 * n))) return fail(ctx, SC_ERR_ARG, "sc_matmul_g_new: tables must have 2^(2n) entries");
  // matrix-multiplication/src/lib.rs:81-86.  relabel(0,n,n) + fix_variables(point[..n]) folds
  // the ROW index of A with LE weights: f_a[col] = sum_row eq(point[..n])[row] * A[row][col]
  // - one "column dot" pass over A, no transposed copy.  f_b folds the column index of B.
  SC_TRY(set_device(ctx));
  const size_t side = (size_t)1 << n;
  if (n == 0) {
    sc_table* ca = nullptr;
    SC_TRY(sc_table_clone(ctx, A, &ca));
    TableBuf ta(ctx, ca);
    SC_TRY(sc_table_clone(ctx, B, b_out));
    *a_out = ta.release();
    return SC_OK;
  }
  TableBuf ta;
  if (side >= 2) {
    PoolBuf eq;
    SC_TRY(build_eq_table(ctx, point, (int)n, &eq));
    SC_TRY(ta.alloc(ctx, side));
    SC_TRY(coldot(ctx, A->d, eq, side, side, ta->d));
  }
  SC_TRY(sc_table_fix_variables(ctx, B, point + n, n, SC_ORDER_LE, b_out));
  SC_HIP(ctx, sync_stream(ctx));
  *a_out = ta.release();
  return SC_OK;
}

extern "C" int sc_prod2_to_evaluations(sc_ctx* ctx, const sc_table* a, const sc_table* b, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_prod2_to_evaluations(ctx, a, b, out);
  SC_TRY(check_pair(ctx, a, b, "sc_prod2_to_evaluations"));
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, a->len));
  int grid = grid_for(ctx, a->len);
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::mul_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  (const u64*)a->d, (const u64*)b->d, t->d, a->len));
  return table_done(ctx, t, hipGetLastError(), "to_evaluations", out);
}

// Round sums of (a, b) as they are (no fold); handles the degenerate 1-entry tables.
static int round_sums_now(sc_ctx* ctx, const u64* a, const u64* b, int log_len, bool across, u64 e[3]) {
  if (log_len < 1) return fail(ctx, SC_ERR_ARG, "round sums need at least one variable");
  bool mb = false;
  SC_TRY(launch_pass(ctx, 0, 1, a, b, nullptr, nullptr, nullptr, log_len, across, &mb));
  SC_TRY(collect_sums(ctx, 3, across, mb, e));
  HostField hf(ctx->fp);
  e[2] = eval2_from_inf(hf, e[0], e[1], e[2]);  // the kernel sums H(0), H(1), H(inf)
  return SC_OK;
}

extern "C" int sc_prod2_round_sums(sc_ctx* ctx, const sc_table* a, const sc_table* b, uint64_t out_e[3]) {
  if (!ctx || !out_e) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_prod2_round_sums(ctx, a, b, out_e);
  SC_TRY(check_pair(ctx, a, b, "sc_prod2_round_sums"));
  SC_TRY(set_device(ctx));
  if (a->len < 2) return fail(ctx, SC_ERR_ARG, "sc_prod2_round_sums: tables have no variable left");
  return round_sums_now(ctx, a->d, b->d, log2_of(a->len), is_sharded(ctx), out_e);
}

extern "C" int sc_prod2_sum(sc_ctx* ctx, const sc_table* a, const sc_table* b, uint64_t* out_c1) {
  if (!ctx || !out_c1) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_prod2_sum(ctx, a, b, out_c1);
  SC_TRY(check_pair(ctx, a, b, "sc_prod2_sum"));
  SC_TRY(set_device(ctx));
  HostField hf(ctx->fp);
  if (a->len == 1) {
    // zero variables on this rank: the (partial) sum is the single product
    PoolBuf prod;
    SC_TRY(prod.alloc(ctx, 1));
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::mul_kernel<F>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, f,
                                                    (const u64*)a->d, (const u64*)b->d, prod.get(), (size_t)1));
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::scale_split_kernel<F>), dim3(1), dim3(64), 0, ctx->stream, f,
                                                    (const u64*)prod, hf.one(), ctx->d_sums));
    prod.reset();
    SC_HIP(ctx, hipGetLastError());
    return collect_sums(ctx, 1, is_sharded(ctx), false, out_c1);
  }
  u64 e[3];
  SC_TRY(round_sums_now(ctx, a->d, b->d, log2_of(a->len), is_sharded(ctx), e));
  *out_c1 = hf.add(e[0], e[1]);  // c_1 = H(0) + H(1)
  return SC_OK;
}

extern "C" int sc_prod2_fold_and_sums(sc_ctx* ctx, const sc_table* a, const sc_table* b, const uint64_t r[1],
                                      sc_table** a_out, sc_table** b_out, uint64_t out_e[3]) {
  if (!ctx || !r || !a_out || !b_out || !out_e) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_prod2_fold_and_sums(ctx, a, b, r, a_out, b_out, out_e);
  SC_TRY(check_pair(ctx, a, b, "sc_prod2_fold_and_sums"));
  SC_TRY(set_device(ctx));
  int nv = log2_of(a->len);
  if (nv < 2) return fail(ctx, SC_ERR_ARG, "sc_prod2_fold_and_sums: need >= 2 variables (fold one, sum over one)");
  TableBuf tb, ta;
  SC_TRY(ta.alloc(ctx, a->len / 2));
  SC_TRY(tb.alloc(ctx, a->len / 2));
  bool mb = false;
  SC_TRY(launch_pass(ctx, 1, 1, a->d, b->d, ta->d, tb->d, r, nv, is_sharded(ctx), &mb));
  SC_TRY(collect_sums(ctx, 3, is_sharded(ctx), mb, out_e));
  HostField hf(ctx->fp);
  out_e[2] = eval2_from_inf(hf, out_e[0], out_e[1], out_e[2]);
  *a_out = ta.release();
  *b_out = tb.release();
  return SC_OK;
}

extern "C" int sc_prod2_evaluate(sc_ctx* ctx, const sc_table* a, const sc_table* b, const uint64_t* point, size_t n,
                                 uint64_t* out) {
  if (!ctx || !out) return SC_ERR_ARG;
  SC_TRY(check_pair(ctx, a, b, "sc_prod2_evaluate"));
  u64 va = 0, vb = 0;
  SC_TRY(sc_table_evaluate(ctx, a, point, n, SC_ORDER_LE, &va));
  SC_TRY(sc_table_evaluate(ctx, b, point, n, SC_ORDER_LE, &vb));
  HostField hf(ctx->fp);
  *out = hf.mul(va, vb);
  return SC_OK;
}
