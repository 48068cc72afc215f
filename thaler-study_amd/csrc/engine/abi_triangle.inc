// Part of sumcheck_hip.hip (included there, in order): C ABI: triangle_counting::G.

// =====================================================================================
// C ABI: triangle_counting::G
// =====================================================================================

namespace {

struct TriView {
  const u64 *f1, *f2, *f3;
  int n1, n2, n3, xv, yv, zv;
};

int check_tri(const sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len, TriView* v) {
  SC_TRY(check_table(ctx, f1, "triangle G"));
  SC_TRY(check_table(ctx, f2, "triangle G"));
  SC_TRY(check_table(ctx, f3, "triangle G"));
  if (is_sharded(ctx) && !is_multi(ctx)) return fail(ctx, SC_ERR_UNSUPPORTED, "triangle G on a sharded context");   // (a multi-device handle's tables are whole tables)
  const int k = (int)var_len;
  v->f1 = f1->d; v->f2 = f2->d; v->f3 = f3->d;
  v->n1 = log2_of(f1->len); v->n2 = log2_of(f2->len); v->n3 = log2_of(f3->len);
  v->xv = v->n1 > k ? v->n1 - k : 0;          // triangle-counting/src/lib.rs:53-55
  v->yv = v->n2 > k ? v->n2 - k : 0;          // :57-59
  v->zv = v->n3 < k ? v->n3 : k;              // :61-67
  // the three copies must describe one consistent state (x fixed before y before z)
  const bool ok = (v->xv > 0) ? (v->n1 == v->xv + k && v->n2 == 2 * k && v->n3 == v->xv + k)
                : (v->yv > 0) ? (v->n1 == v->yv && v->n2 == v->yv + k && v->n3 == k)
                              : (v->n1 == 0 && v->n2 == v->zv && v->n3 == v->zv);
  if (!ok) return fail(ctx, SC_ERR_ARG, "triangle G: inconsistent table sizes (%d,%d,%d) for var_len %d", v->n1, v->n2, v->n3, k);
  return SC_OK;
}


}  // namespace

extern "C" int sc_tri_to_evaluations(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3,
                                     size_t var_len, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_tri_to_evaluations(ctx, f1, f2, f3, var_len, out);
  TriView v;
  SC_TRY(check_tri(ctx, f1, f2, f3, var_len, &v));
  SC_TRY(set_device(ctx));
  if (v.xv + v.yv + v.zv > 34) return fail(ctx, SC_ERR_ARG, "triangle to_evaluations: 2^%d entries", v.xv + v.yv + v.zv);
  const size_t total = (size_t)1 << (v.xv + v.yv + v.zv);
  TableBuf t;
  SC_TRY(t.alloc(ctx, total));
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::tri_to_evaluations_kernel<F>), dim3(grid_for_wide(ctx, total)),
                                                  dim3(sc::kBlock), 0, ctx->stream, f, v.f1, v.f2, v.f3, v.xv, v.yv, v.zv, t->d));
  return table_done(ctx, t, hipGetLastError(), "triangle to_evaluations", out);
}

extern "C" int sc_tri_round_sums(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len,
                                 uint64_t out_e[3]) {
  if (!ctx || !out_e) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_tri_round_sums(ctx, f1, f2, f3, var_len, out_e);
  TriView v;
  SC_TRY(check_tri(ctx, f1, f2, f3, var_len, &v));
  SC_TRY(set_device(ctx));
  if (v.xv + v.yv + v.zv < 1) return fail(ctx, SC_ERR_ARG, "triangle G: no variable left");
  const size_t total = (size_t)1 << (v.xv + v.yv + v.zv - 1);
  const int grid = grid_for_wide(ctx, total);
  sc::PassOut out = next_pass_out(ctx);
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::tri_sums_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  v.f1, v.f2, v.f3, v.xv, v.yv, v.zv, out));
  SC_TRY(commit_pass_out(ctx, out, grid));
  SC_TRY(collect_sums(ctx, 3, false, ctx->use_mailbox != 0, out_e));
  HostField hf(ctx->fp);
  out_e[2] = eval2_from_inf(hf, out_e[0], out_e[1], out_e[2]);
  return SC_OK;
}

extern "C" int sc_tri_fix_variables(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3,
                                    size_t var_len, const uint64_t* r, size_t k, sc_table** f1_out, sc_table** f2_out,
                                    sc_table** f3_out) {
  // (a multi-device handle: the three sc_table_fix_variables below are the handle's)
  if (!ctx || (k && !r) || !f1_out || !f2_out || !f3_out) return SC_ERR_ARG;
  TriView v;
  SC_TRY(check_tri(ctx, f1, f2, f3, var_len, &v));
  const size_t xv = v.xv, yv = v.yv;
  if (k > (size_t)(v.xv + v.yv + v.zv)) return fail(ctx, SC_ERR_ARG, "triangle fix_variables: k=%zu > num_vars", k);
  // triangle-counting/src/lib.rs:90-105
  const size_t n_xy = std::min(xv + yv, k);
  const size_t n_yz = k > xv ? k - xv : 0;
  std::vector<u64> xz(r, r + std::min(xv, k));
  if (k > xv + yv) xz.insert(xz.end(), r + xv + yv, r + k);
  TableBuf o3, o2, o1;
  SC_TRY(sc_table_fix_variables(ctx, f1, r, n_xy, SC_ORDER_LE, o1.out(ctx)));
  SC_TRY(sc_table_fix_variables(ctx, f2, r + std::min(xv, k), n_yz, SC_ORDER_LE, o2.out(ctx)));
  SC_TRY(sc_table_fix_variables(ctx, f3, xz.data(), xz.size(), SC_ORDER_LE, o3.out(ctx)));
  *f1_out = o1.release();
  *f2_out = o2.release();
  *f3_out = o3.release();
  return SC_OK;
}

extern "C" int sc_tri_evaluate(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len,
                               const uint64_t* point, size_t n, uint64_t* out) {
  if (!ctx || !out || (n && !point)) return SC_ERR_ARG;
  TriView v;
  SC_TRY(check_tri(ctx, f1, f2, f3, var_len, &v));
  if (n != (size_t)(v.xv + v.yv + v.zv)) return fail(ctx, SC_ERR_ARG, "triangle evaluate: point has %zu entries, G has %d variables", n, v.xv + v.yv + v.zv);
  // :72-84
  std::vector<u64> xz(point, point + v.xv);
  xz.insert(xz.end(), point + v.xv + v.yv, point + n);
  u64 e1 = 0, e2 = 0, e3 = 0;
  SC_TRY(sc_table_evaluate(ctx, f1, point, (size_t)(v.xv + v.yv), SC_ORDER_LE, &e1));
  SC_TRY(sc_table_evaluate(ctx, f2, point + v.xv, (size_t)(v.yv + v.zv), SC_ORDER_LE, &e2));
  SC_TRY(sc_table_evaluate(ctx, f3, xz.data(), xz.size(), SC_ORDER_LE, &e3));
  HostField hf(ctx->fp);
  *out = hf.mul(hf.mul(e1, e3), e2);   // :86
  return SC_OK;
}

// Three product-of-two-tables sumchecks in a row (see include/sumcheck_hip.h).
struct sc_tri_prover {
  sc_ctx* ctx = nullptr;     // (a prover of a multi-device handle: its first device - everything after the square runs there)
  sc_ctx* handle = nullptr;
  const u64* adj = nullptr;  // borrowed 2^(2k) table
  int k = 0;
  size_t next_round = 0;
  std::vector<u64> r;        // every challenge received
  sc_prover* sub = nullptr;  // current phase's engine
  sc_table ta, tb;           // views handed to sc_prover_create
  PoolBuf P, f3r, f1y, Q, f2r;
  PoolBuf adj_full;          // sharded contexts: the gathered adjacency table
  u64 scale = 0;             // f1(r_x, r_y) in the z phase
  u64 c1 = 0;
};

namespace {

// Fold the challenges the sub-prover has not applied yet plus `r_last`; hand back the table(s) asked for (a null
// a_out / b_out: that table is not needed, its folds are not launched).
int prover_finish(sc_prover* pr, u64 r_last, PoolBuf* a_out, PoolBuf* b_out, size_t* len_out) {
  sc_ctx* ctx = pr->ctx;
  std::vector<u64> rs(pr->pending);   // the sub-prover's own state is left untouched
  rs.push_back(r_last);
  PoolBuf na, nb;
  size_t la = 0, lb = 0;
  if (pr->host_mode) {
    // the host has taken the sub-prover's tables over (engine/abi_prover.inc: host_tail; only option mixes with one-round passes
    // get here before a phase ends): fold copies of them on the host and hand device copies back
    HostField hf(ctx->fp);
    for (int t = 0; t < 2; ++t) {
      if (!(t ? b_out : a_out)) continue;
      std::vector<u64> v(t ? pr->hb : pr->ha);
      for (const u64 r : rs) {
        const size_t half = v.size() / 2;
        if (half == 0) return fail(ctx, SC_ERR_STATE, "prover_finish: more challenges than variables");
        for (size_t i = 0; i < half; ++i) v[i] = hf.add(v[2 * i], hf.mul(r, hf.sub(v[2 * i + 1], v[2 * i])));
        v.resize(half);
      }
      PoolBuf d;
      SC_TRY(d.alloc(ctx, v.size()));
      if (hipMemcpyAsync(d, v.data(), v.size() * sizeof(u64), hipMemcpyHostToDevice, ctx->stream) != hipSuccess || sync_stream(ctx) != hipSuccess)
        return fail(ctx, SC_ERR_HIP, "prover_finish: upload failed");
      (t ? nb : na) = std::move(d);
      (t ? lb : la) = v.size();
    }
  } else {
    const size_t len = (size_t)1 << pr->cur_log;
    if (a_out) SC_TRY(fold_chain(ctx, pr->sh[0].cur_a, len, rs.data(), rs.size(), SC_ORDER_LE, &na, &la));
    if (b_out) SC_TRY(fold_chain(ctx, pr->sh[0].cur_b, len, rs.data(), rs.size(), SC_ORDER_LE, &nb, &lb));
  }
  if (a_out) *a_out = std::move(na);
  if (b_out) *b_out = std::move(nb);
  *len_out = a_out ? la : lb;
  return SC_OK;
}

// one word of device memory to the host: through the pinned mailbox (a one-wave kernel + a spin on its sequence word,
// ~5 us) rather than hipMemcpyAsync + hipStreamSynchronize (~40 us of host time around an 8-byte copy)
int fetch_word(sc_ctx* ctx, const u64* d, u64* out) {
  if (ctx->use_mailbox) {
    const u64 seq = ctx->mailbox_seq + 1;
    hipLaunchKernelGGL(sc::mailbox_copy_kernel, dim3(1), dim3(sc::kWave), 0, ctx->stream, d, 1, ctx->d_mailbox, seq);
    SC_HIP(ctx, hipGetLastError());
    ctx->mailbox_seq = seq;
    SC_TRY(wait_mailbox(ctx, seq));
    *out = ctx->h_mailbox[0];
    return SC_OK;
  }
  SC_HIP(ctx, hipMemcpyAsync(out, d, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  return SC_OK;
}

int tri_start_phase(sc_tri_prover* tp, const u64* a, const u64* b, size_t len) {
  tp->ta.d = const_cast<u64*>(a);
  tp->ta.len = len;
  tp->tb.d = const_cast<u64*>(b);
  tp->tb.len = len;
  if (tp->sub) sc_prover_destroy(tp->sub);
  tp->sub = nullptr;
  return prover_create_impl(tp->ctx, &tp->ta, &tp->tb, /*replicated=*/true, &tp->sub);   // whole tables on every rank
}

// Rows [z_begin, z_begin + z_rows) of P = the square of the adjacency matrix (index (z << k) | x), from the WHOLE adjacency
// table on this device: the n^3 work of the proof, the part that splits over ranks / devices.
int tri_square_rows(sc_ctx* ctx, const u64* adj, int k, u64* P, size_t z_begin, size_t z_rows) {
  const size_t n = (size_t)1 << k, full_len = n * n;
  SC_TRY(timer_begin(ctx, SC_KIND_MATSQ, k, 0, 2 * k, (u64)8 * full_len, (u64)8 * z_rows * n));
  if (k >= 6 && z_rows >= 64) {
    // adjacency tables are 0/1 (G::new_adj_matrix): their square is a count, computed exactly by the int8 matrix
    // cores.  Bytes + flag, the MFMA kernel, and behind it the generic kernel, which runs only if the flag says
    // the table held something else - no host round trip decides.
    PoolBuf bytes;   // T8 | T8t | flag
    SC_TRY(bytes.alloc(ctx, 2 * (full_len / 8) + 8));
    unsigned char* t8 = reinterpret_cast<unsigned char*>(bytes.get());
    unsigned char* t8t = t8 + full_len;
    unsigned* flag = reinterpret_cast<unsigned*>(bytes.get() + 2 * (full_len / 8));
    const size_t tiles = (z_rows / 64) * (n / 64);   // 64 x 64 output tiles of this rank's rows
    const int grid = (int)std::min<size_t>(tiles, (size_t)4 * ctx->num_cus);
    const size_t tiles32 = (z_rows / 32) * (n / 32);
    if (hipMemsetAsync(flag, 0, sizeof(unsigned), ctx->stream) != hipSuccess) return fail(ctx, SC_ERR_HIP, "matsq: memset failed");
    SC_DISPATCH_FIELD(ctx, F, f, {
      hipLaunchKernelGGL((sc::matsq_bytes_kernel<F>), dim3((unsigned)std::min<size_t>((n / 64) * (n / 64), (size_t)8 * ctx->num_cus)),
                         dim3(sc::kBlock), 0, ctx->stream, f, adj, k, t8, t8t, flag);
      hipLaunchKernelGGL((sc::matsq_mfma_kernel<F>), dim3((unsigned)std::min<size_t>((tiles32 + 3) / 4, (size_t)8 * ctx->num_cus)),
                         dim3(sc::kBlock), 0, ctx->stream, f, (const unsigned char*)t8, (const unsigned char*)t8t, k, P, z_begin,
                         z_rows, (const unsigned*)flag);
      hipLaunchKernelGGL((sc::matsq_tiled_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, adj, k, P, z_begin,
                         z_rows, (const unsigned*)flag);
    });
    bytes.reset();   // stream-ordered reuse
  } else {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::matsq_kernel<F>), dim3(grid_for_wide(ctx, z_rows * n)), dim3(sc::kBlock),
                                                    0, ctx->stream, f, adj, k, P, z_begin, z_rows));
  }
  if (hipGetLastError() != hipSuccess) return fail(ctx, SC_ERR_HIP, "matsq kernel launch failed");
  return timer_end(ctx);
}

}  // namespace

// On a sharded context `adj` is this rank's rows of the adjacency table (top log2(world) bits of the row index
// = rank).  The n^3 work - the matrix square - is split by rows of P across the ranks; the adjacency table and
// P are gathered (n^2 words each) and the three product sumchecks on 2^(2k)- and 2^k-entry tables run
// replicated on every rank with no further exchange.
static int multi_tri_prover_create(sc_ctx* m, const sc_table* adj, size_t var_len, sc_tri_prover** out);
extern "C" int sc_tri_prover_create(sc_ctx* ctx, const sc_table* adj, size_t var_len, sc_tri_prover** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_tri_prover_create(ctx, adj, var_len, out);
  SC_TRY(check_table(ctx, adj, "sc_tri_prover_create"));
  const bool sharded = is_sharded(ctx) && ctx->world > 1;
  const size_t full_len = (size_t)1 << (2 * var_len);
  if (var_len < 1 || var_len > 15 || adj->len * (size_t)(sharded ? ctx->world : 1) != full_len)
    return fail(ctx, SC_ERR_ARG, "sc_tri_prover_create: adjacency table must have 2^(2*var_len) entries (over all ranks)");
  if (sharded && var_len < (size_t)ctx->log_world)
    return fail(ctx, SC_ERR_ARG, "sc_tri_prover_create: fewer rows than ranks");
  SC_TRY(set_device(ctx));
  sc_tri_prover* tp = new (std::nothrow) sc_tri_prover;
  if (!tp) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  tp->ctx = ctx;
  tp->adj = adj->d;
  tp->k = (int)var_len;
  int rc = SC_OK;
  if (sharded) {
    rc = gather_table(ctx, adj->d, adj->len, &tp->adj_full);
    tp->adj = tp->adj_full;
  }
  const size_t n = (size_t)1 << var_len;
  const size_t z_rows = sharded ? n / ctx->world : n, z_begin = sharded ? (size_t)ctx->rank * z_rows : 0;
  if (rc == SC_OK) rc = tp->P.alloc(ctx, full_len);
  if (rc == SC_OK) rc = tri_square_rows(ctx, tp->adj, tp->k, tp->P, z_begin, z_rows);
  if (rc == SC_OK && sharded) {
    // every rank computed its rows of P: gather the whole square
    PoolBuf full;
    rc = gather_table(ctx, tp->P + z_begin * n, z_rows * n, &full);
    if (rc == SC_OK) tp->P = std::move(full);   // (the rows go back)
  }
  // x phase: sum_{x,z} P(x,z) f3(x,z), both indexed (z << k) | x
  if (rc == SC_OK) rc = tri_start_phase(tp, tp->P, tp->adj, full_len);
  if (rc != SC_OK) {
    sc_tri_prover_destroy(tp);
    return rc;
  }
  tp->c1 = tp->sub->c1;
  *out = tp;
  return SC_OK;
}

extern "C" int sc_tri_prover_c1(const sc_tri_prover* pr, uint64_t* out) {
  if (!pr || !out) return SC_ERR_ARG;
  *out = pr->c1;
  return SC_OK;
}

static int tri_prover_round_impl(sc_tri_prover* tp, uint64_t r_prev, size_t j, uint64_t out_e[3]);
extern "C" int sc_tri_prover_round(sc_tri_prover* tp, uint64_t r_prev, size_t j, uint64_t out_e[3]) {
  if (!tp || !out_e) return SC_ERR_ARG;
  const int rc = tri_prover_round_impl(tp, r_prev, j, out_e);
  if (rc != SC_OK && tp->handle) (void)fail(tp->handle, rc, "%s", tp->ctx->err.c_str());   // the caller reads errors from the handle
  return rc;
}
static int tri_prover_round_impl(sc_tri_prover* tp, uint64_t r_prev, size_t j, uint64_t out_e[3]) {
  sc_ctx* ctx = tp->ctx;
  const size_t k = (size_t)tp->k;
  if (j != tp->next_round) return fail(ctx, SC_ERR_STATE, "sc_tri_prover_round: expected round %zu, got %zu", tp->next_round, j);
  if (j >= 3 * k) return fail(ctx, SC_ERR_STATE, "sc_tri_prover_round: all %zu rounds done", 3 * k);
  if (j != 0 && r_prev >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_tri_prover_round: challenge is not reduced");
  SC_TRY(set_device(ctx));
  if (j != 0) tp->r.push_back(r_prev);
  // a failed round leaves the challenge list as it was, so the round can be retried
#define SC_TRY_POP(expr)                        \
  do {                                          \
    int rc_ = (expr);                           \
    if (rc_ != SC_OK) {                         \
      if (j != 0) tp->r.pop_back();             \
      return rc_;                               \
    }                                           \
  } while (0)
  HostField hf(ctx->fp);
  const size_t n = (size_t)1 << k;
  if (j == k) {
    // x fully fixed at r_x = r[0..k): P(r_x, .) is not needed any more, f3(r_x, .) is
    PoolBuf pb;
    size_t len = 0;
    SC_TRY_POP(prover_finish(tp->sub, r_prev, nullptr, &pb, &len));   // P(r_x, .) is not needed
    tp->f3r = std::move(pb);  // f3(r_x, z), 2^k entries (an earlier one goes back)
    size_t l1 = 0;
    tp->f1y.reset();
    SC_TRY_POP(fold_chain(ctx, tp->adj, n * n, tp->r.data(), k, SC_ORDER_LE, &tp->f1y, &l1));  // f1(r_x, y)
    if (!tp->Q) SC_TRY_POP(tp->Q.alloc(ctx, n));
    SC_TRY_POP(coldot(ctx, tp->adj, tp->f3r, n, n, tp->Q));  // Q[y] = sum_z f2[(z<<k)|y] f3r[z]
    SC_TRY_POP(tri_start_phase(tp, tp->f1y, tp->Q, n));
  } else if (j == 2 * k) {
    PoolBuf pa;
    size_t len = 0;
    SC_TRY_POP(prover_finish(tp->sub, r_prev, &pa, nullptr, &len));   // Q(r_y) is not needed
    const int fr = fetch_word(ctx, pa, &tp->scale);                    // f1(r_x, r_y)
    pa.reset();
    SC_TRY_POP(fr);
    size_t l2 = 0;
    tp->f2r.reset();
    SC_TRY_POP(fold_chain(ctx, tp->adj, n * n, tp->r.data() + k, k, SC_ORDER_LE, &tp->f2r, &l2));  // f2(r_y, z)
    SC_TRY_POP(tri_start_phase(tp, tp->f2r, tp->f3r, n));
  }
  const size_t local_j = j % k;
  const bool phase_start = (local_j == 0);
  u64 e[3];
  SC_TRY_POP(sc_prover_round(tp->sub, phase_start ? hf.one() : r_prev, local_j, e));
#undef SC_TRY_POP
  if (j >= 2 * k) {
    for (int i = 0; i < 3; ++i) e[i] = hf.mul(e[i], tp->scale);
  }
  memcpy(out_e, e, sizeof(e));
  tp->next_round = j + 1;
  return SC_OK;
}

extern "C" int sc_tri_prove(sc_ctx* ctx, const sc_table* adj, size_t var_len, sc_draw_fn draw, void* user, uint64_t seed_r,
                            uint64_t* c1, uint64_t* evals, uint64_t* challenges) {
  if (!ctx) return SC_ERR_ARG;
  sc_tri_prover* tp = nullptr;
  SC_TRY(sc_tri_prover_create(ctx, adj, var_len, &tp));
  if (c1) *c1 = tp->c1;
  const int rc = run_rounds(ctx, tp, 3 * (size_t)tp->k, sc_tri_prover_round, draw, user, seed_r, evals, challenges);
  sc_tri_prover_destroy(tp);
  return rc;
}

extern "C" int sc_tri_prover_destroy(sc_tri_prover* tp) {
  if (!tp) return SC_OK;
  if (tp->sub) sc_prover_destroy(tp->sub);
  delete tp;
  return SC_OK;
}

// Prover<F, G> for G::new_adj_matrix on a multi-device handle: the adjacency table (a table of the handle, split by rows)
// is gathered whole onto every device, every device squares its rows of P on its own matrix cores, the rows go to the
// first device (hipMemcpyPeerAsync) and the three product sumchecks on 2^(2k)- and 2^k-entry tables run there.
static int multi_tri_prover_create(sc_ctx* m, const sc_table* adj, size_t var_len, sc_tri_prover** out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, adj, "sc_tri_prover_create"));
  const size_t N = m->subs.size(), full_len = (size_t)1 << (2 * var_len), n = (size_t)1 << var_len;
  if (var_len < 1 || var_len > 15 || adj->len != full_len)
    return fail(m, SC_ERR_ARG, "sc_tri_prover_create: adjacency table must have 2^(2*var_len) entries");
  if (n < N) return fail(m, SC_ERR_ARG, "sc_tri_prover_create: fewer rows than devices");
  sc_ctx* first = m->subs[0];
  sc_tri_prover* tp = new (std::nothrow) sc_tri_prover;
  if (!tp) return fail(m, SC_ERR_OOM, "host allocation failed");
  tp->ctx = first;
  tp->handle = m;
  tp->k = (int)var_len;
  const size_t z_rows = n / N;
  PoolBuf whole[kMaxSubs];   // the adjacency table, whole on every device
  int rc = set_device(first);
  if (rc == SC_OK) rc = tp->P.alloc(first, full_len);
  // (every device's stream writes its rows into P: the first device's stream must be done with the recycled block - ADVICE r04)
  if (rc == SC_OK && hipStreamSynchronize(first->stream) != hipSuccess) rc = fail(first, SC_ERR_HIP, "triangle: draining the first device's stream failed");
  if (rc == SC_OK)
    rc = multi_run(m, [&](int d, sc_ctx* sub) -> int {
      SC_TRY(multi_gather_to(m, adj, sub, &whole[d]));
      PoolBuf rows;   // this device's rows of P, addressed like the whole matrix (given back on return: the copy is drained)
      SC_TRY(rows.alloc(sub, z_rows * n));
      SC_TRY(tri_square_rows(sub, whole[d], tp->k, rows - (size_t)d * z_rows * n, (size_t)d * z_rows, z_rows));
      hipError_t e = hipMemcpyPeerAsync(tp->P + (size_t)d * z_rows * n, first->device, rows, sub->device, z_rows * n * sizeof(u64), sub->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(sub->stream);
      if (e != hipSuccess) return fail(sub, SC_ERR_HIP, "triangle: sending a device's rows of the square to the first device: %s", hipGetErrorString(e));
      return SC_OK;
    });
  for (size_t d = 1; d < N; ++d) whole[d].reset();
  if (rc == SC_OK) {
    tp->adj_full = std::move(whole[0]);   // (released with the prover)
    tp->adj = tp->adj_full;
    rc = set_device(first);
    if (rc == SC_OK) rc = tri_start_phase(tp, tp->P, tp->adj, full_len);   // x phase: sum_{x,z} P(x,z) f3(x,z)
    if (rc != SC_OK) (void)fail(m, rc, "%s", first->err.c_str());
  } else {
    whole[0].reset();
  }
  if (rc != SC_OK) {
    sc_tri_prover_destroy(tp);
    return rc;
  }
  tp->c1 = tp->sub->c1;
  *out = tp;
  return SC_OK;
}
