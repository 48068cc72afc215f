// Part of sumcheck_hip.hip (included there, in order): shared helpers of the table API: pool, fold chains, column dots, evaluate.

namespace {

// =====================================================================================
// shared helpers for the table API
// =====================================================================================

// The end of a call that launched a kernel (or queued a copy: e) into the fresh table t: the stream drained, t handed out - or
// freed and `what` reported
int table_done(sc_ctx* ctx, TableBuf& t, hipError_t e, const char* what, sc_table** out) {
  if (e == hipSuccess) e = sync_stream(ctx);
  if (e != hipSuccess) {
    t.reset();
    return fail(ctx, SC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  *out = t.release();
  return SC_OK;
}

sc::RVec make_rvec(const u64* r, size_t n) {
  sc::RVec rv;
  memset(&rv, 0, sizeof(rv));
  for (size_t i = 0; i < n && i < 64; ++i) rv.v[i] = r[i];
  return rv;
}

// eq table over `nbits` index bits: out[i] = prod_j (bit_j(i) ? r[j] : 1 - r[j]).
int build_eq_table(sc_ctx* ctx, const u64* r, int nbits, PoolBuf* out) {
  if (nbits > 40) return fail(ctx, SC_ERR_ARG, "eq table of 2^%d entries", nbits);
  PoolBuf t;
  SC_TRY(t.alloc(ctx, (size_t)1 << nbits));
  sc::RVec rv = make_rvec(r, (size_t)nbits);
  int grid = grid_for_wide(ctx, (size_t)1 << nbits);
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::eq_table_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  rv, 0, nbits, t.get()));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "eq_table_kernel: %s", hipGetErrorString(e));
  *out = std::move(t);
  return SC_OK;
}

// Launch shape of a row-walking kernel (kernels.hpp, coldot_kernel / gkr_phase1_kernel) over rows x M words: how many
// contiguous KiB a wave reads per row (PW: 4 where the row is long enough, measured +10-16 % over 1), how many blocks
// across the columns (gx) and how many chunks of rows (blockIdx.y) - ONE wave per SIMD in total (four waves per SIMD
// read 10-20 % slower with this access pattern, tools/rowwalk.hip), at least 16 rows per chunk so that the partial
// rows stay a small fraction of the table.
struct RowWalk {
  int pw;
  size_t gx, chunks, rows_per_chunk;
};
RowWalk row_walk_shape(const sc_ctx* ctx, size_t rows, size_t M) {
  const size_t mp = M / 2;
  RowWalk s;
  s.pw = (mp % 256 == 0 && mp >= 1024) ? 4 : (mp % 128 == 0 && mp >= 256) ? 2 : 1;
  const size_t n_spans = (mp + 64 * (size_t)s.pw - 1) / (64 * (size_t)s.pw);
  s.gx = std::min<size_t>((n_spans + 3) / 4, 1024);
  const size_t waves = 4 * (size_t)ctx->num_cus;   // one per SIMD
  size_t chunks = std::min<size_t>((waves + n_spans - 1) / n_spans, std::max<size_t>(rows / 16, 1));
  chunks = std::max<size_t>(1, std::min<size_t>(chunks, 1024));
  s.rows_per_chunk = (rows + chunks - 1) / chunks;
  s.rows_per_chunk = (s.rows_per_chunk + 3) / 4 * 4;   // whole batches of rows in flight
  s.chunks = (rows + s.rows_per_chunk - 1) / s.rows_per_chunk;
  return s;
}

// out[c] = sum_i w[i] * in[i*M + c], i < rows: one streaming pass (plus a small reduce when
// the rows are split over blockIdx.y for parallelism).  M must be even.
int coldot(sc_ctx* ctx, const u64* in, const u64* w, size_t rows, size_t M, u64* out) {
  const RowWalk rw = row_walk_shape(ctx, rows, M);
  const size_t gx = rw.gx, chunks = rw.chunks, rows_per_chunk = rw.rows_per_chunk;
  if (rows_per_chunk > sc::GoldilocksMont::kAccMaxTerms)   // one lazy accumulator sums rows_per_chunk products
    return fail(ctx, SC_ERR_UNSUPPORTED, "coldot: %zu rows per chunk exceed the lazy accumulator's capacity", rows_per_chunk);
  PoolBuf rows_buf;   // the chunks' partial rows
  if (chunks > 1) SC_TRY(rows_buf.alloc(ctx, chunks * M));
  u64* const partial = chunks > 1 ? rows_buf.get() : out;
  const int nt = (rows * M) >= ((size_t)1 << ctx->nt_load_log) ? 1 : 0;
  SC_TRY(timer_begin(ctx, SC_KIND_COLDOT, log2_of(rows), 0, log2_of(rows * M), (u64)8 * rows * M + 8 * rows, (u64)8 * M));
#define SC_COLDOT(NT, PW)                                                                                                  \
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::coldot_kernel<F, NT, PW>), dim3((unsigned)gx, (unsigned)chunks),    \
                                                  dim3(sc::kBlock), 0, ctx->stream, f, in, w, rows, rows_per_chunk, M, partial))
  if (nt) {
    if (rw.pw == 4) SC_COLDOT(true, 4);
    else if (rw.pw == 2) SC_COLDOT(true, 2);
    else SC_COLDOT(true, 1);
  } else {
    if (rw.pw == 4) SC_COLDOT(false, 4);
    else if (rw.pw == 2) SC_COLDOT(false, 2);
    else SC_COLDOT(false, 1);
  }
#undef SC_COLDOT
  if (chunks > 1) {
    int grid = grid_for_wide(ctx, M);
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::sum_rows_kernel<F>), dim3(grid, 1), dim3(sc::kBlock), 0, ctx->stream, f,
                                                    (const u64*)partial, (const u64*)partial, chunks, M, out, out));
    rows_buf.reset();
  }
  SC_HIP(ctx, hipGetLastError());
  SC_TRY(timer_end(ctx));
  return SC_OK;
}

// Fold k variables of a device table (LE or BE), producing a pool buffer.  `in` is never
// written.  LE: eight or more variables in one streaming segment-dot pass, fewer at up to three
// per pass (read N, write N/8).  BE: one "column dot" pass against the eq table of the k
// leading variables.
int fold_chain(sc_ctx* ctx, const u64* in, size_t len, const u64* r, size_t k, int order, PoolBuf* out,
               size_t* out_len) {
  if (k == 0) {
    PoolBuf cp;
    SC_TRY(cp.alloc(ctx, len));
    SC_HIP(ctx, hipMemcpyAsync(cp, in, len * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    *out = std::move(cp);
    *out_len = len;
    return SC_OK;
  }
  if (order == SC_ORDER_BE && k >= 2 && (len >> k) >= 2) {
    // eq index i has variable 0 (r[0]) as its MSB: reverse r for the LE-bit table builder
    std::vector<u64> rr(r, r + k);
    std::reverse(rr.begin(), rr.end());
    PoolBuf res, eq;   // (eq is given back first)
    SC_TRY(build_eq_table(ctx, rr.data(), (int)k, &eq));
    SC_TRY(res.alloc(ctx, len >> k));
    SC_TRY(coldot(ctx, in, eq, (size_t)1 << k, len >> k, res));
    *out = std::move(res);   // (eq goes back behind it: the launches that read it are queued)
    *out_len = len >> k;
    return SC_OK;
  }
  const u64* cur = in;
  PoolBuf owned;  // intermediate we own (never `in`)
  size_t cur_len = len;
  size_t done = 0;
  while (done < k) {
    int step;
    PoolBuf nxt_buf;
    u64* nxt = nullptr;   // = nxt_buf, once allocated (what the launches below capture)
    if (order == SC_ORDER_LE && k - done >= 8) {
      // many variables left: one streaming pass over contiguous segments (kernels.hpp, fix_low_kernel)
      step = (int)std::min<size_t>(17, k - done);
      const size_t nlen = cur_len >> step;
      SC_TRY(nxt_buf.alloc(ctx, nlen));
      nxt = nxt_buf;
      const sc::RVec rv = make_rvec(r + done, (size_t)step);
      // one segment per wave: four-wave blocks while there is at most one segment per wave of one block per CU, beyond that
      // one block per CU with all sixteen waves, which draw their segments from a counter in LDS (kernels.hpp, evaluate_kernel)
      int grid = (int)std::min<size_t>((nlen + 3) / 4, (size_t)std::min(ctx->max_blocks, 1024)), threads = sc::kBlock;
      if (nlen > (size_t)4 * std::min(ctx->num_cus, ctx->max_blocks)) {
        threads = ctx->gold ? sc::stream_block<sc::GoldilocksMont>::fix_low : sc::stream_block<sc::MontGeneric>::fix_low;
        grid = std::min(ctx->num_cus, ctx->max_blocks);
      }
      const int nt = cur_len >= ((size_t)1 << ctx->nt_load_log) ? 1 : 0;
      SC_TRY(timer_begin(ctx, SC_KIND_FIX_LOW, step, 0, log2_of(cur_len), (u64)8 * cur_len, (u64)8 * nlen));
      SC_DISPATCH_FIELD(ctx, F, f, with_bool(nt, [&](auto NT) {
        hipLaunchKernelGGL((sc::fix_low_kernel<F, NT>), dim3(grid), dim3(threads), 0, ctx->stream, f, cur, nxt, step, rv, nlen);
      }));
      SC_TRY(timer_end(ctx));
      cur_len = nlen;
    } else if (order == SC_ORDER_LE && k - done >= 4 && cur_len <= ((size_t)1 << 20) && (cur_len >> std::min<size_t>(5, k - done)) >= 1) {
      // a small table: four or five variables in one launch (kernels.hpp, fold_wide_kernel)
      step = (int)std::min<size_t>(5, k - done);
      const size_t nlen = cur_len >> step;
      SC_TRY(nxt_buf.alloc(ctx, nlen));
      nxt = nxt_buf;
      const sc::GridW gw = make_weights<sc::GridW>(ctx, r + done, step);
      SC_TRY(timer_begin(ctx, SC_KIND_FOLD, step, 0, log2_of(cur_len), (u64)8 * cur_len, (u64)8 * nlen));
      const int grid = grid_for(ctx, nlen);
      SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::fold_wide_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, cur, nxt,
                                                      gw, step, nlen));
      SC_TRY(timer_end(ctx));
      cur_len = nlen;
    } else if (order == SC_ORDER_LE) {
      step = (int)std::min<size_t>(3, k - done);
      while (step > 1 && (cur_len >> step) < 2) --step;
      size_t nlen = cur_len >> step;
      SC_TRY(nxt_buf.alloc(ctx, nlen));
      nxt = nxt_buf;
      const sc::FoldW fw = make_weights<sc::FoldW>(ctx, r + done, step);
      SC_TRY(timer_begin(ctx, SC_KIND_FOLD, step, 0, log2_of(cur_len), (u64)8 * cur_len, (u64)8 * nlen));
      if (nlen >= 2) {
        size_t n_units = nlen / 2;
        int grid = grid_for(ctx, n_units), threads = sc::kBlock, grab = ctx->dbg_fold_grab > 0 ? ctx->dbg_fold_grab : 1;   // four-wave blocks: one tile per draw
        if (n_units > (size_t)ctx->max_blocks * sc::kBlock * sc::kFoldGrab) {   // several runs per wave: one block per CU with all sixteen waves (kernels.hpp)
          threads = sc::kFoldBlock;
          grid = std::min(ctx->num_cus, ctx->max_blocks);
          grab = sc::kFoldGrab;
        }
        const int nt = cur_len >= ((size_t)1 << ctx->nt_load_log) ? 1 : 0;
        hipError_t ea = hipSuccess;
        SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3>(step, [&](auto KF) {
          with_bool(nt, [&](auto NT) {
            // more dynamic LDS than a launch gets by default: asked for once per kernel
            if (sc::fold_kernel_lds_bytes(KF, threads) > 65536 && !ctx->fold_lds_allowed[KF][NT]) {
              ea = hipFuncSetAttribute(kernel_ptr(&sc::fold_kernel<F, KF, NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)sc::fold_kernel_lds_bytes(KF, sc::kFoldBlock));
              if (ea != hipSuccess) return;
              ctx->fold_lds_allowed[KF][NT] = true;
            }
            hipLaunchKernelGGL((sc::fold_kernel<F, KF, NT>), dim3(grid), dim3(threads), sc::fold_kernel_lds_bytes(KF, threads), ctx->stream, f,
                               cur, nxt, fw, n_units, grab);
          });
        }));
        if (ea != hipSuccess) SC_TRY(fail(ctx, SC_ERR_HIP, "fold_kernel: %s", hipGetErrorString(ea)));
      } else {
        SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::fold_le_small_kernel<F>), dim3(1), dim3(64), 0,
                                                        ctx->stream, f, cur, nxt, r[done], nlen));
      }
      SC_TRY(timer_end(ctx));
      cur_len = nlen;
    } else {
      step = 1;
      size_t half = cur_len / 2;
      SC_TRY(nxt_buf.alloc(ctx, half));
      nxt = nxt_buf;
      int grid = grid_for(ctx, (half + 1) / 2);
      SC_TRY(timer_begin(ctx, SC_KIND_FOLD_BE, 1, 0, log2_of(cur_len), (u64)8 * cur_len, (u64)8 * half));
      SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::fold_be_kernel<F>), dim3(grid), dim3(sc::kBlock), 0,
                                                      ctx->stream, f, cur, nxt, r[done], half));
      SC_TRY(timer_end(ctx));
      cur_len = half;
    }
    {
      hipError_t le = hipGetLastError();
      if (le != hipSuccess) {
        poison(ctx);
        return fail(ctx, SC_ERR_HIP, "fold launch: %s", hipGetErrorString(le));
      }
    }
    owned = std::move(nxt_buf);  // the previous intermediate goes back here (stream-ordered reuse: single stream per context)
    cur = nxt;
    done += step;
  }
  *out = std::move(owned);
  *out_len = cur_len;
  return SC_OK;
}

int check_table(const sc_ctx* ctx, const sc_table* t, const char* what) {
  if (ctx && is_multi(ctx)) {
    // N parts - or ONE part on the first device for a table with fewer entries than the handle has devices (is_single)
    const bool split = t && t->parts.size() == ctx->subs.size(), single = t && t->parts.size() == 1 && t->len < ctx->subs.size();
    if (!t || t->d || !(split || single) || !is_pow2(t->len))
      return fail(ctx, SC_ERR_ARG, "%s: not a table of this multi-device handle", what);
    return SC_OK;
  }
  if (!t || !t->d || !is_pow2(t->len)) return fail(ctx, SC_ERR_ARG, "%s: table is null or not 2^k long", what);
  return SC_OK;
}

}  // namespace
