// Part of sumcheck_hip.hip (included there, in order): C ABI: gkr_protocol::round_polynomial::W.

// =====================================================================================
// C ABI: gkr_protocol::round_polynomial::W
// =====================================================================================

namespace {

struct WView {
  const u64 *add, *mul, *w_b, *w_c;
  int kb, kc;       // variables of b and c (global)
  size_t rows = 0;  // values of c this rank holds (2^kc unsharded)
};

int check_w(const sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
            WView* v) {
  SC_TRY(check_table(ctx, add, "gkr W"));
  SC_TRY(check_table(ctx, mul, "gkr W"));
  SC_TRY(check_table(ctx, w_b, "gkr W"));
  SC_TRY(check_table(ctx, w_c, "gkr W"));
  // sharded contexts: add and mul are this rank's rows of c (top log2(world) bits of the index = rank), w_b and w_c are
  // whole on every rank - the layout of sc_gkr_prover_create
  v->kb = log2_of(w_b->len);
  v->kc = log2_of(w_c->len);
  if (is_multi(ctx)) {   // whole tables behind a handle (no device pointers here: the callers go part by part or through the first device)
    if (add->len != mul->len || add->len != ((size_t)1 << (v->kb + v->kc)))
      return fail(ctx, SC_ERR_ARG, "gkr W: add/mul must have num_vars(w_b) + num_vars(w_c) variables");
    v->rows = (size_t)1 << v->kc;
    v->add = v->mul = v->w_b = v->w_c = nullptr;
    return SC_OK;
  }
  if (add->len != mul->len || add->len * (size_t)ctx->world != ((size_t)1 << (v->kb + v->kc)))
    return fail(ctx, SC_ERR_ARG, "gkr W: add/mul must have num_vars(w_b) + num_vars(w_c) variables (over all ranks)");
  if (ctx->world > 1 && v->kc < ctx->log_world)
    return fail(ctx, SC_ERR_UNSUPPORTED, "sharded gkr W: fewer rows of c than ranks");
  v->rows = add->len >> v->kb;
  v->add = add->d;
  v->mul = mul->d;
  v->w_b = w_b->d;
  v->w_c = w_c->d;
  return SC_OK;
}

// (H(0), H(1), H(2)) of the current round; the summed variable is w_b's while it has any.  Sharded: every rank sums
// over its own rows of c (the pairs of the summed variable are shard-local: index bit 0), the limbs are added across
// the ranks like a pass's.
int w_round_sums(sc_ctx* ctx, const WView& w, u64 e[3]) {
  if (w.kb + w.kc < 1) return fail(ctx, SC_ERR_ARG, "gkr W: no variable left");
  const bool across = is_sharded(ctx);
  const size_t c0 = across ? (size_t)ctx->rank * w.rows : 0;   // first value of c on this rank
  const u64 *V, *Fx;
  int logV;
  if (w.kb >= 1) {
    V = w.w_b;
    logV = w.kb;
    Fx = w.w_c + c0;
  } else {
    if (w.rows < 2) return fail(ctx, SC_ERR_UNSUPPORTED, "sharded gkr W: the summed variable crosses shards");
    V = w.w_c + c0;
    logV = log2_of(w.rows);
    Fx = w.w_b;
  }
  const size_t n_pieces = (w.rows << w.kb) / 2;
  int grid = grid_for(ctx, n_pieces);
  bool mb = false;
  const u64 dg[1] = {(u64)w.kb << 32 | (u64)w.kc};
  sc::PassOut out = next_pass_out(ctx, across, challenge_digest(dg, 1, 0, 77), &mb);
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_sums_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  w.add, w.mul, V, logV, Fx, n_pieces, out));
  SC_TRY(commit_pass_out(ctx, out, grid));
  SC_TRY(collect_sums(ctx, 3, across, mb, e));
  HostField hf(ctx->fp);
  e[2] = eval2_from_inf(hf, e[0], e[1], e[2]);
  return SC_OK;
}

int evaluate_replicated(sc_ctx* ctx, const u64* d, size_t len, const u64* pt, u64* out);
int fetch_word(sc_ctx* ctx, const u64* d, u64* out);

}  // namespace

// the same entry points on a multi-device handle (bottom of this file)
static int multi_gkr_wiring(sc_ctx* m, const int32_t* gate_type, const uint32_t* in0, const uint32_t* in1, size_t k_i, size_t k_next,
                            const uint64_t* r_i, sc_table** add_out, sc_table** mul_out);
static int multi_gkr_w_evaluate(sc_ctx* m, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
                                const uint64_t* point, size_t n, uint64_t* out);
static int multi_gkr_prover_create(sc_ctx* m, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
                                   sc_gkr_prover** out);
static int multi_gather_to(sc_ctx* m, const sc_table* t, sc_ctx* dst, PoolBuf* out);

extern "C" int sc_gkr_wiring(sc_ctx* ctx, const int32_t* gate_type, const uint32_t* in0, const uint32_t* in1, size_t k_i,
                             size_t k_next, const uint64_t* r_i, sc_table** add_out, sc_table** mul_out) {
  if (!ctx || !gate_type || !in0 || !in1 || (k_i && !r_i) || !add_out || !mul_out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_gkr_wiring(ctx, gate_type, in0, in1, k_i, k_next, r_i, add_out, mul_out);
  if (k_i > 30 || k_next > 15) return fail(ctx, SC_ERR_ARG, "sc_gkr_wiring: layer too large");
  if (ctx->world > 1 && k_next < (size_t)ctx->log_world) return fail(ctx, SC_ERR_UNSUPPORTED, "sc_gkr_wiring: fewer rows of c than ranks");
  SC_TRY(set_device(ctx));
  // sharded: every rank gets the whole gate list and keeps the gates whose c (= in1) falls into its rows - the shard
  // (top log2(world) index bits = rank) of the tables, with no exchange
  const size_t n_gates = (size_t)1 << k_i, n_next = (size_t)1 << k_next, rows = n_next / (size_t)ctx->world, len = rows * n_next;
  const unsigned row_lo = (unsigned)((size_t)ctx->rank * rows);
  for (size_t a = 0; a < n_gates; ++a) {
    if ((gate_type[a] != 0 && gate_type[a] != 1) || in0[a] >= n_next || in1[a] >= n_next)
      return fail(ctx, SC_ERR_ARG, "sc_gkr_wiring: gate %zu is malformed", a);
  }
  TableBuf tm, ta;
  PoolBuf gates, eq;  // gates: [type | in0 | in1] as 32-bit words
  SC_TRY(build_eq_table(ctx, r_i, (int)k_i, &eq));
  SC_TRY(gates.alloc(ctx, (3 * n_gates * 4 + 7) / 8 + 1));
  SC_TRY(ta.alloc(ctx, len));
  SC_TRY(tm.alloc(ctx, len));
  int* d_type = (int*)gates.get();
  unsigned* d_in0 = (unsigned*)gates.get() + n_gates;
  unsigned* d_in1 = (unsigned*)gates.get() + 2 * n_gates;
  hipError_t e = hipMemcpyAsync(d_type, gate_type, n_gates * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in0, in0, n_gates * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in1, in1, n_gates * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(ta->d, 0, len * sizeof(u64), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(tm->d, 0, len * sizeof(u64), ctx->stream);
  if (e == hipSuccess) {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_wiring_scatter_kernel<F>), dim3(grid_for_wide(ctx, n_gates)),
                                                    dim3(sc::kBlock), 0, ctx->stream, f, (const u64*)eq, (const int*)d_type,
                                                    (const unsigned*)d_in0, (const unsigned*)d_in1, n_gates, (int)k_next,
                                                    row_lo, (unsigned)rows, ta->d, tm->d));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = sync_stream(ctx);
  if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "sc_gkr_wiring: %s", hipGetErrorString(e));
  *add_out = ta.release();
  *mul_out = tm.release();
  return SC_OK;
}

extern "C" int sc_gkr_w_to_evaluations(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                                       const sc_table* w_c, sc_table** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_gkr_w_to_evaluations(ctx, add, mul, w_b, w_c, out);
  WView w;
  SC_TRY(check_w(ctx, add, mul, w_b, w_c, &w));
  SC_TRY(set_device(ctx));
  // The reference's output order is b-major while a sharded context holds rows of c: the result, like every table there,
  // is this rank's contiguous shard of the OUTPUT (top index bits = rank, i.e. a range of b), which needs every rank's
  // rows of add and mul - they are gathered whole for the duration of the call (round 4; SC_ERR_UNSUPPORTED before).
  const bool sharded = is_sharded(ctx) && ctx->world > 1;
  PoolBuf add_full, mul_full;
  if (sharded) {
    if (w.kb < ctx->log_world) return fail(ctx, SC_ERR_UNSUPPORTED, "gkr W to_evaluations: fewer values of b than ranks");
    SC_TRY(gather_pair(ctx, w.add, w.mul, add->len, &add_full, &mul_full));
  }
  const size_t total = (size_t)1 << (w.kb + w.kc), count = sharded ? total / (size_t)ctx->world : total;
  const size_t begin = sharded ? (size_t)ctx->rank * count : 0;
  TableBuf t;
  SC_TRY(t.alloc(ctx, count));
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_to_evaluations_kernel<F>), dim3(grid_for_wide(ctx, count)),
                                                  dim3(sc::kBlock), 0, ctx->stream, f, sharded ? add_full.get() : w.add,
                                                  sharded ? mul_full.get() : w.mul, w.w_b, w.kb, w.w_c, w.kc, begin, count, t->d));
  add_full.reset();   // stream-ordered
  mul_full.reset();
  return table_done(ctx, t, hipGetLastError(), "gkr to_evaluations", out);
}

extern "C" int sc_gkr_w_round_sums(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                                   const sc_table* w_c, uint64_t out_e[3]) {
  if (!ctx || !out_e) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_gkr_w_round_sums(ctx, add, mul, w_b, w_c, out_e);
  WView w;
  SC_TRY(check_w(ctx, add, mul, w_b, w_c, &w));
  SC_TRY(set_device(ctx));
  return w_round_sums(ctx, w, out_e);
}

extern "C" int sc_gkr_w_fix_variables(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                                      const sc_table* w_c, const uint64_t* r, size_t k, sc_table** add_out,
                                      sc_table** mul_out, sc_table** w_b_out, sc_table** w_c_out) {
  if (!ctx || (k && !r) || !add_out || !mul_out || !w_b_out || !w_c_out) return SC_ERR_ARG;
  WView w;   // (a multi-device handle: the four sc_table_fix_variables below are the handle's - shard by shard while the variables
  SC_TRY(check_w(ctx, add, mul, w_b, w_c, &w));   // stay inside the shards, through the first device across the device bits)
  if (k > (size_t)(w.kb + w.kc)) return fail(ctx, SC_ERR_ARG, "gkr fix_variables: k=%zu > num_vars=%d", k, w.kb + w.kc);
  const size_t k_b = std::min<size_t>(k, (size_t)w.kb), k_c = k - k_b;   // round_polynomial.rs:60-63
  TableBuf oc, ob, om, oa;
  SC_TRY(sc_table_fix_variables(ctx, add, r, k, SC_ORDER_LE, oa.out(ctx)));
  SC_TRY(sc_table_fix_variables(ctx, mul, r, k, SC_ORDER_LE, om.out(ctx)));
  SC_TRY(sc_table_fix_variables(ctx, w_b, r, k_b, SC_ORDER_LE, ob.out(ctx)));
  SC_TRY(sc_table_fix_variables(ctx, w_c, r + k_b, k_c, SC_ORDER_LE, oc.out(ctx)));
  *add_out = oa.release();
  *mul_out = om.release();
  *w_b_out = ob.release();
  *w_c_out = oc.release();
  return SC_OK;
}

extern "C" int sc_gkr_w_evaluate(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                                 const sc_table* w_c, const uint64_t* point, size_t n, uint64_t* out) {
  if (ctx && is_multi(ctx)) return multi_gkr_w_evaluate(ctx, add, mul, w_b, w_c, point, n, out);
  if (!ctx || !out || (n && !point)) return SC_ERR_ARG;
  WView w;
  SC_TRY(check_w(ctx, add, mul, w_b, w_c, &w));
  if (n != (size_t)(w.kb + w.kc)) return fail(ctx, SC_ERR_ARG, "gkr evaluate: point has %zu entries, W has %d variables", n, w.kb + w.kc);
  u64 ae = 0, me = 0, wb = 0, wc = 0;
  SC_TRY(sc_table_evaluate(ctx, add, point, n, SC_ORDER_LE, &ae));
  SC_TRY(sc_table_evaluate(ctx, mul, point, n, SC_ORDER_LE, &me));
  SC_TRY(evaluate_replicated(ctx, w_b->d, w_b->len, point, &wb));          // whole on every rank
  SC_TRY(evaluate_replicated(ctx, w_c->d, w_c->len, point + w.kb, &wc));
  HostField hf(ctx->fp);
  *out = hf.add(hf.mul(ae, hf.add(wb, wc)), hf.mul(me, hf.mul(wb, wc)));   // round_polynomial.rs:56
  return SC_OK;
}

// The W prover in its two-phase form (kernels.hpp, "Two-phase form of the W sumcheck"): the rounds over
// the b variables are ONE product-of-two-tables proof on [P | L] x [W_b | 1], the rounds over the c
// variables one on [Q | w* add_r] x [W_c | 1]; both run on the pass engine of sc_prover.  add and mul are
// streamed twice per layer (dense form) or the gate list is scattered twice (sparse form).
struct sc_gkr_prover {
  sc_ctx* ctx = nullptr;
  // dense form: borrowed tables, index (c << kb) | b (this rank's rows of c on a sharded context)
  const u64 *add = nullptr, *mul = nullptr;
  size_t add_len = 0;
  // both forms: W_b and W_c, whole on every rank
  const u64 *w_b = nullptr, *w_c = nullptr;
  int kb = 0, kc = 0;   // variables of b / c when the prover was created
  // sparse form: the gate list on the device and eq(r_i, a)
  bool sparse = false;
  size_t n_gates = 0;
  int* sp_type = nullptr;
  unsigned *sp_in0 = nullptr, *sp_in1 = nullptr;
  PoolBuf sp_val;
  PoolBuf sp_words;   // pool block backing sp_type / sp_in0 / sp_in1 (empty: the words are a circuit's)
  size_t num_vars = 0, next_round = 0;
  u64 c1 = 0;
  std::vector<u64> r;        // challenges received
  // current phase
  sc_prover* sub = nullptr;
  sc_table ta, tb;
  PoolBuf TA, TB;
  // multi-device handle (round 4): `ctx` above is the handle's FIRST device - the 2^(k+1)-entry product proofs of both
  // phases run there, on whole tables - and every device streams its own rows of c of add / mul: dev[d] is a view of this
  // prover on device d (its parts of add and mul, its own whole copy of W_c).  W_b and W_c whole on the first device.
  sc_ctx* handle = nullptr;
  std::vector<sc_gkr_prover> dev;
  std::vector<PoolBuf> owned;  // [device] the whole copy of W_c (pool memory of that device); [n + 0] W_b whole on the first device
                               // (a dev[] view owns nothing: its pointers are borrowed from the prover it belongs to)
};

namespace {

// value of a whole (unsharded) device table at an LE point, on this rank alone
int evaluate_replicated(sc_ctx* ctx, const u64* d, size_t len, const u64* pt, u64* out) {
  if (len == 1) return fetch_word(ctx, d, out);
  HostField hf(ctx->fp);
  bool mb = false;
  SC_TRY(evaluate_local(ctx, d, len, pt, hf.one(), false, &mb));
  return collect_sums(ctx, 1, false, mb, out);
}

// P and L of the b phase (dense form): one streaming pass over add and mul
int gkr_dense_phase1(sc_gkr_prover* pr, u64* P, u64* L) {
  sc_ctx* ctx = pr->ctx;
  const size_t M = (size_t)1 << pr->kb;
  const size_t rows = pr->add_len / M;   // this rank's values of c
  const u64* w = pr->w_c + (is_sharded(ctx) ? (size_t)ctx->rank * rows : 0);
  const RowWalk rw = row_walk_shape(ctx, rows, M);
  const size_t gx = rw.gx, chunks = rw.chunks, rows_per_chunk = rw.rows_per_chunk;
  if (rows_per_chunk > sc::GoldilocksMont::kAccMaxTerms)
    return fail(ctx, SC_ERR_UNSUPPORTED, "gkr: %zu rows per chunk exceed the lazy accumulator's capacity", rows_per_chunk);
  PoolBuf rows_L, rows_P;   // the chunks' partial rows (given back on return, P's first)
  if (chunks > 1) {
    SC_TRY(rows_P.alloc(ctx, chunks * M));
    SC_TRY(rows_L.alloc(ctx, chunks * M));
  }
  u64 *const pP = chunks > 1 ? rows_P.get() : P, *const pL = chunks > 1 ? rows_L.get() : L;
  const int nt = pr->add_len >= ((size_t)1 << ctx->nt_load_log) ? 1 : 0;
  SC_TRY(timer_begin(ctx, SC_KIND_GKR, pr->kc, 0, log2_of(pr->add_len), (u64)16 * pr->add_len + 8 * rows, (u64)16 * M));
  {
#define SC_PHASE1(NT, PW)                                                                                                   \
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_phase1_kernel<F, NT, PW>), dim3((unsigned)gx, (unsigned)chunks),  \
                                                  dim3(sc::kBlock), 0, ctx->stream, f, pr->add, pr->mul, w, rows, rows_per_chunk, M, pP, pL))
    if (nt) {
      if (rw.pw == 4) SC_PHASE1(true, 4);
      else if (rw.pw == 2) SC_PHASE1(true, 2);
      else SC_PHASE1(true, 1);
    } else {
      if (rw.pw == 4) SC_PHASE1(false, 4);
      else if (rw.pw == 2) SC_PHASE1(false, 2);
      else SC_PHASE1(false, 1);
    }
#undef SC_PHASE1
    if (chunks > 1) {
      const int grid = grid_for_wide(ctx, M);
      SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::sum_rows_kernel<F>), dim3(grid, 2), dim3(sc::kBlock), 0, ctx->stream, f,
                                                      (const u64*)pP, (const u64*)pL, chunks, M, P, L));
    }
    if (hipGetLastError() != hipSuccess) {
      poison(ctx);
      return fail(ctx, SC_ERR_HIP, "gkr phase-1 launch failed");
    }
  }
  return timer_end(ctx);
}

// sum a vector of residues over the ranks of a sharded context (split limbs, exact), in place
int allreduce_residues(sc_ctx* ctx, u64* v, size_t n) {
  if (!is_sharded(ctx) || ctx->world == 1) return SC_OK;
  PoolBuf limbs;
  SC_TRY(limbs.alloc(ctx, 2 * n));
  hipLaunchKernelGGL(sc::split_limbs_kernel, dim3(grid_for(ctx, n)), dim3(sc::kBlock), 0, ctx->stream, (const u64*)v, n, limbs.get());
  SC_TRY(allreduce_device(ctx, limbs, 2 * n));
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::recombine_limbs_kernel<F>), dim3(grid_for(ctx, n)), dim3(sc::kBlock), 0,
                                                  ctx->stream, f, (const u64*)limbs, n, v));
  if (hipGetLastError() != hipSuccess) return fail(ctx, SC_ERR_HIP, "recombine_limbs_kernel launch failed");
  return SC_OK;
}

// Build the phase's tables and start its product prover.  which = 0: b variables; 1: c variables (b fixed at
// pr->r[0 .. kb)).
int gkr_start_phase(sc_gkr_prover* pr, int which) {
  sc_ctx* ctx = pr->ctx;
  HostField hf(ctx->fp);
  if (pr->sub) sc_prover_destroy(pr->sub);
  pr->sub = nullptr;
  pr->TA.reset();   // (before the new pair is built: its blocks are what the phase's tables are made in)
  pr->TB.reset();
  const int kv = which == 0 ? pr->kb : pr->kc;   // variables of this phase
  const size_t n = (size_t)1 << kv;
  PoolBuf X, Y;   // P, L  or  add_r, mul_r
  u64 wstar = 0;
  const bool sharded_dense = !pr->sparse && !pr->handle && is_sharded(ctx) && ctx->world > 1;
  if (pr->handle && !pr->sparse && pr->handle->subs.size() > 1) {
    // every device streams its rows of c; the first device adds / concatenates what the others send (hipMemcpyPeerAsync: xGMI)
    sc_ctx* m = pr->handle;
    const size_t N = m->subs.size();
    PoolBuf stage_buf;   // which == 0: [P rows | L rows], N rows of n words each; which == 1: [add_r | mul_r], n words each
    SC_TRY(stage_buf.alloc(ctx, 2 * N * n));
    u64* const stage = stage_buf;
    // (the other devices' streams write into it: nothing of this context's stream may still be using the recycled block)
    if (sync_stream(ctx) != hipSuccess) return fail(ctx, SC_ERR_HIP, "gkr: draining the first device's stream failed");
    if (which == 1) SC_TRY(evaluate_replicated(ctx, pr->w_b, (size_t)1 << pr->kb, pr->r.data(), &wstar));
    SC_TRY(multi_run(m, [&](int d, sc_ctx* sub) -> int {
      sc_gkr_prover& v = pr->dev[d];
      SC_TRY(set_device(sub));
      PoolBuf y, x;   // (given back on return, x first: the copies are drained)
      size_t lx = n, ly = n;
      if (which == 0) {
        SC_TRY(x.alloc(sub, n));
        SC_TRY(y.alloc(sub, n));
        SC_TRY(gkr_dense_phase1(&v, x, y));
      } else {
        SC_TRY(fold_chain(sub, v.add, v.add_len, pr->r.data(), (size_t)pr->kb, SC_ORDER_LE, &x, &lx));
        SC_TRY(fold_chain(sub, v.mul, v.add_len, pr->r.data(), (size_t)pr->kb, SC_ORDER_LE, &y, &ly));
      }
      // which == 0: row d of the P block and of the L block; which == 1: slice d of add_r and of mul_r
      u64* dx = which == 0 ? stage + (size_t)d * n : stage + (size_t)d * lx;
      u64* dy = which == 0 ? stage + N * n + (size_t)d * n : stage + n + (size_t)d * ly;
      hipError_t e = hipMemcpyPeerAsync(dx, ctx->device, x, sub->device, lx * sizeof(u64), sub->stream);
      if (e == hipSuccess) e = hipMemcpyPeerAsync(dy, ctx->device, y, sub->device, ly * sizeof(u64), sub->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(sub->stream);
      if (e != hipSuccess) return fail(sub, SC_ERR_HIP, "gkr: sending a device's part to the first device: %s", hipGetErrorString(e));
      return SC_OK;
    }));
    SC_TRY(set_device(ctx));
    SC_TRY(X.alloc(ctx, n));
    SC_TRY(Y.alloc(ctx, n));
    if (which == 0) {
      SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::sum_rows_kernel<F>), dim3(grid_for_wide(ctx, n), 2), dim3(sc::kBlock), 0, ctx->stream,
                                                      f, (const u64*)stage, (const u64*)(stage + N * n), N, n, X.get(), Y.get()));
      if (hipGetLastError() != hipSuccess) return fail(ctx, SC_ERR_HIP, "gkr: sum of the devices' P and L failed to launch");
    } else {
      hipError_t e = hipMemcpyAsync(X, stage, n * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(Y, stage + n, n * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream);
      if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "gkr: %s", hipGetErrorString(e));
    }
    // (the stage goes back here, stream-ordered)
  } else if (which == 0) {
    SC_TRY(X.alloc(ctx, n));
    SC_TRY(Y.alloc(ctx, n));
    if (pr->sparse) {
      hipError_t e = hipMemsetAsync(X, 0, n * sizeof(u64), ctx->stream);
      if (e == hipSuccess) e = hipMemsetAsync(Y, 0, n * sizeof(u64), ctx->stream);
      if (e == hipSuccess) {
        SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_sparse_phase1_kernel<F>), dim3(grid_for_wide(ctx, pr->n_gates)),
                                                        dim3(sc::kBlock), 0, ctx->stream, f, (const u64*)pr->sp_val,
                                                        (const int*)pr->sp_type, (const unsigned*)pr->sp_in0,
                                                        (const unsigned*)pr->sp_in1, pr->n_gates, pr->w_c, X.get(), Y.get()));
        e = hipGetLastError();
      }
      if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "gkr sparse phase 1: %s", hipGetErrorString(e));
    } else {
      SC_TRY(gkr_dense_phase1(pr, X, Y));
      // sharded: every rank summed its own rows of c; P and L are the sums over the ranks
      if (sharded_dense) SC_TRY(allreduce_residues(ctx, X, n));
      if (sharded_dense) SC_TRY(allreduce_residues(ctx, Y, n));
    }
  } else {
    // w* = W_b(r_b)
    SC_TRY(evaluate_replicated(ctx, pr->w_b, (size_t)1 << pr->kb, pr->r.data(), &wstar));
    if (pr->sparse) {
      PoolBuf eqb;   // (given back at the end of this block)
      SC_TRY(build_eq_table(ctx, pr->r.data(), pr->kb, &eqb));
      SC_TRY(X.alloc(ctx, n));
      SC_TRY(Y.alloc(ctx, n));
      hipError_t e = hipMemsetAsync(X, 0, n * sizeof(u64), ctx->stream);
      if (e == hipSuccess) e = hipMemsetAsync(Y, 0, n * sizeof(u64), ctx->stream);
      if (e == hipSuccess) {
        SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_sparse_phase2_kernel<F>), dim3(grid_for_wide(ctx, pr->n_gates)),
                                                        dim3(sc::kBlock), 0, ctx->stream, f, (const u64*)pr->sp_val,
                                                        (const int*)pr->sp_type, (const unsigned*)pr->sp_in0,
                                                        (const unsigned*)pr->sp_in1, pr->n_gates, (const u64*)eqb, X.get(), Y.get()));
        e = hipGetLastError();
      }
      if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "gkr sparse phase 2: %s", hipGetErrorString(e));
    } else {
      // add(r_b, .) and mul(r_b, .): fix the kb low variables of both tables (one streaming pass each)
      size_t la = 0, lm = 0;
      SC_TRY(fold_chain(ctx, pr->add, pr->add_len, pr->r.data(), (size_t)pr->kb, SC_ORDER_LE, &X, &la));
      SC_TRY(fold_chain(ctx, pr->mul, pr->add_len, pr->r.data(), (size_t)pr->kb, SC_ORDER_LE, &Y, &lm));
      if (sharded_dense) {
        // every rank holds its rows of c: gather the whole 2^kc-entry tables (the rows go back as the gathered tables move in)
        PoolBuf gx, gy;
        SC_TRY(gather_pair(ctx, X, Y, la, &gx, &gy));
        X = std::move(gx);
        Y = std::move(gy);
      }
    }
  }
  SC_TRY(pr->TA.alloc(ctx, 2 * n));
  SC_TRY(pr->TB.alloc(ctx, 2 * n));
  {
    const u64 sY = which == 0 ? 0 : wstar, sZ = which == 0 ? hf.one() : wstar;
    const u64* Z = which == 0 ? Y : X;
    const u64* V = which == 0 ? pr->w_b : pr->w_c;
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gkr_combine_kernel<F>), dim3(grid_for_wide(ctx, n)), dim3(sc::kBlock), 0,
                                                    ctx->stream, f, (const u64*)X, (const u64*)(which == 0 ? X : Y), sY, Z, sZ, V, n,
                                                    pr->TA.get(), pr->TB.get()));
    if (hipGetLastError() != hipSuccess) return fail(ctx, SC_ERR_HIP, "gkr_combine_kernel launch failed");
  }
  X.reset();   // stream-ordered: the combine kernel is ahead of any reuse
  Y.reset();
  pr->ta.d = pr->TA;
  pr->ta.len = 2 * n;
  pr->tb.d = pr->TB;
  pr->tb.len = 2 * n;
  return prover_create_impl(ctx, &pr->ta, &pr->tb, true, &pr->sub);
}

int gkr_prover_begin(sc_gkr_prover* pr) {
  pr->num_vars = (size_t)(pr->kb + pr->kc);
  SC_TRY(gkr_start_phase(pr, pr->kb >= 1 ? 0 : 1));
  pr->c1 = pr->sub->c1;   // sum of [X | lin] . [V | 1] = sum_b W(b) P(b) + L(b) = sum of f
  return SC_OK;
}

}  // namespace

extern "C" int sc_gkr_prover_create_sparse(sc_ctx* ctx, const int32_t* gate_type, const uint32_t* in0, const uint32_t* in1,
                                           size_t k_i, size_t k_next, const uint64_t* r_i, const sc_table* w_next,
                                           sc_gkr_prover** out) {
  if (!ctx || !gate_type || !in0 || !in1 || (k_i && !r_i) || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) {
    // O(gates) work and 2^k-entry tables: nothing to split.  The prover runs on the handle's first device, over a whole copy
    // of W_{i+1} gathered from the handle's table (owned by the prover through a one-device table).
    SC_TRY(multi_enter(ctx));
    SC_TRY(check_table(ctx, w_next, "sc_gkr_prover_create_sparse"));
    sc_ctx* first = ctx->subs[0];
    PoolBuf whole;
    int rc = multi_gather_to(ctx, w_next, first, &whole);
    sc_table view;
    view.d = whole;
    view.len = w_next->len;
    sc_gkr_prover* pr = nullptr;
    if (rc == SC_OK) rc = sc_gkr_prover_create_sparse(first, gate_type, in0, in1, k_i, k_next, r_i, &view, &pr);
    if (rc != SC_OK) return fail(ctx, rc, "%s", first->err.c_str());
    pr->handle = ctx;
    pr->owned.resize(ctx->subs.size() + 1);
    pr->owned[ctx->subs.size()] = std::move(whole);   // released with the prover (on its context: the first device)
    *out = pr;
    return SC_OK;
  }
  SC_TRY(check_table(ctx, w_next, "sc_gkr_prover_create_sparse"));
  if (k_i > 30 || k_next < 1 || k_next > 26 || w_next->len != ((size_t)1 << k_next))
    return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create_sparse: bad layer sizes");
  SC_TRY(set_device(ctx));
  const size_t n_gates = (size_t)1 << k_i, n_next = (size_t)1 << k_next;
  for (size_t a = 0; a < n_gates; ++a)
    if ((gate_type[a] != 0 && gate_type[a] != 1) || in0[a] >= n_next || in1[a] >= n_next)
      return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create_sparse: gate %zu is malformed", a);
  sc_gkr_prover* pr = new (std::nothrow) sc_gkr_prover;
  if (!pr) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  pr->ctx = ctx;
  pr->sparse = true;
  pr->n_gates = n_gates;
  pr->w_b = pr->w_c = w_next->d;   // on a sharded context: the whole table, on every rank
  pr->kb = pr->kc = (int)k_next;
  int rc = pr->sp_words.alloc(ctx, (3 * n_gates * 4 + 7) / 8 + 1);   // type | in0 | in1 as 32-bit words
  if (rc == SC_OK) rc = build_eq_table(ctx, r_i, (int)k_i, &pr->sp_val);  // eq(r_i, a): the gate's weight
  if (rc == SC_OK) {
    pr->sp_type = (int*)pr->sp_words.get();
    pr->sp_in0 = (unsigned*)pr->sp_words.get() + n_gates;
    pr->sp_in1 = (unsigned*)pr->sp_words.get() + 2 * n_gates;
    hipError_t e = hipMemcpyAsync(pr->sp_type, gate_type, n_gates * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pr->sp_in0, in0, n_gates * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pr->sp_in1, in1, n_gates * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = sync_stream(ctx);   // host arrays may go away after return
    if (e != hipSuccess) rc = fail(ctx, SC_ERR_HIP, "sc_gkr_prover_create_sparse: %s", hipGetErrorString(e));
  }
  if (rc == SC_OK) rc = gkr_prover_begin(pr);
  if (rc != SC_OK) {
    sc_gkr_prover_destroy(pr);
    return rc;
  }
  *out = pr;
  return SC_OK;
}

extern "C" int sc_gkr_prover_create(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                                    const sc_table* w_c, sc_gkr_prover** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_gkr_prover_create(ctx, add, mul, w_b, w_c, out);
  SC_TRY(check_table(ctx, add, "gkr W"));
  SC_TRY(check_table(ctx, mul, "gkr W"));
  SC_TRY(check_table(ctx, w_b, "gkr W"));
  SC_TRY(check_table(ctx, w_c, "gkr W"));
  SC_TRY(set_device(ctx));
  const int kb = log2_of(w_b->len), kc = log2_of(w_c->len);
  // sharded: add and mul are this rank's rows of c (top log2(world) bits of the index = rank); W_b and W_c whole
  if (add->len != mul->len || add->len * (size_t)ctx->world != ((size_t)1 << (kb + kc)))
    return fail(ctx, SC_ERR_ARG, "gkr W: add/mul must have num_vars(w_b) + num_vars(w_c) variables");
  if (kb + kc < 1) return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create: W has no variables");
  if (ctx->world > 1 && (kc < ctx->log_world || kb < 1))
    return fail(ctx, SC_ERR_UNSUPPORTED, "sharded gkr W needs at least log2(world) variables of c and one of b");
  sc_gkr_prover* pr = new (std::nothrow) sc_gkr_prover;
  if (!pr) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  pr->ctx = ctx;
  pr->add = add->d;
  pr->mul = mul->d;
  pr->add_len = add->len;
  pr->w_b = w_b->d;
  pr->w_c = w_c->d;
  pr->kb = kb;
  pr->kc = kc;
  int rc = gkr_prover_begin(pr);
  if (rc != SC_OK) {
    sc_gkr_prover_destroy(pr);
    return rc;
  }
  *out = pr;
  return SC_OK;
}

extern "C" int sc_gkr_prover_c1(const sc_gkr_prover* pr, uint64_t* out) {
  if (!pr || !out) return SC_ERR_ARG;
  *out = pr->c1;
  return SC_OK;
}

static int gkr_prover_round_impl(sc_gkr_prover* pr, uint64_t r_prev, size_t j, uint64_t out_e[3]);
extern "C" int sc_gkr_prover_round(sc_gkr_prover* pr, uint64_t r_prev, size_t j, uint64_t out_e[3]) {
  if (!pr || !out_e) return SC_ERR_ARG;
  const int rc = gkr_prover_round_impl(pr, r_prev, j, out_e);
  // a prover of a multi-device handle works on the handle's first device: the caller reads errors from the handle
  if (rc != SC_OK && pr->handle && pr->handle->err != pr->ctx->err) (void)fail(pr->handle, rc, "%s", pr->ctx->err.c_str());
  return rc;
}
static int gkr_prover_round_impl(sc_gkr_prover* pr, uint64_t r_prev, size_t j, uint64_t out_e[3]) {
  sc_ctx* ctx = pr->ctx;
  if (j != pr->next_round) return fail(ctx, SC_ERR_STATE, "sc_gkr_prover_round: expected round %zu, got %zu", pr->next_round, j);
  if (j >= pr->num_vars) return fail(ctx, SC_ERR_STATE, "sc_gkr_prover_round: all %zu rounds done", pr->num_vars);
  if (j != 0 && r_prev >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_round: challenge is not reduced");
  SC_TRY(set_device(ctx));
  HostField hf(ctx->fp);
  if (j != 0) pr->r.push_back(r_prev);
  size_t local_j = j;
  bool phase_start = (j == 0);
  if (pr->kb >= 1 && j >= (size_t)pr->kb) {
    local_j = j - (size_t)pr->kb;
    if (local_j == 0) {
      // b is fixed at r[0 .. kb): build the c phase
      const int rc = gkr_start_phase(pr, 1);
      if (rc != SC_OK) {
        pr->r.pop_back();
        return rc;
      }
      phase_start = true;
    }
  }
  const int rc = sc_prover_round(pr->sub, phase_start ? hf.one() : r_prev, local_j, out_e);
  if (rc != SC_OK) {
    if (j != 0) pr->r.pop_back();
    return rc;
  }
  pr->next_round = j + 1;
  return SC_OK;
}

// Whole W sumcheck in one call (sc_prove's contract): create, 2k rounds, the challenge of each round drawn on the host
// after that round's sums have been read back.
template <class P, class RoundFn>
static int run_rounds(sc_ctx* ctx, P* pr, size_t num_vars, RoundFn round, sc_draw_fn draw, void* user, uint64_t seed_r,
                      uint64_t* evals, uint64_t* challenges) {
  HostField hf(ctx->fp);
  u64 r_j = hf.one();   // callers pass F::one() for round 0
  for (size_t j = 0; j < num_vars; ++j) {
    u64 e[3];
    SC_TRY(round(pr, r_j, j, e));
    if (evals) memcpy(evals + 3 * j, e, sizeof(e));
    r_j = draw ? draw(user, j, e) : seeded_challenge(ctx, hf, seed_r, j);
    if (r_j >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "draw() returned an unreduced challenge");
    if (challenges) challenges[j] = r_j;
  }
  return SC_OK;
}

extern "C" int sc_gkr_prove(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
                            sc_draw_fn draw, void* user, uint64_t seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges) {
  if (!ctx) return SC_ERR_ARG;
  sc_gkr_prover* pr = nullptr;
  SC_TRY(sc_gkr_prover_create(ctx, add, mul, w_b, w_c, &pr));
  if (c1) *c1 = pr->c1;
  const int rc = run_rounds(ctx, pr, pr->num_vars, sc_gkr_prover_round, draw, user, seed_r, evals, challenges);
  sc_gkr_prover_destroy(pr);
  return rc;
}

extern "C" int sc_gkr_prover_destroy(sc_gkr_prover* pr) {
  if (!pr) return SC_OK;
  if (pr->sub) sc_prover_destroy(pr->sub);
  delete pr;   // (every buffer it owns goes back to the pool of the context it came from)
  return SC_OK;
}

// =====================================================================================
// gkr_protocol::round_polynomial::W on a multi-device handle (round 4)
// =====================================================================================
//
// add_i(r_i,.,.) and mul_i(r_i,.,.) - the 4^k-entry tables, the only large objects of a GKR layer - are tables of the
// handle: device d holds its rows of c.  W_b / W_c are 2^k-entry tables of the handle too (split like every table); the
// prover gathers them whole (64 KiB at k = 13).  Per layer every device streams its part of add and mul twice (P and L;
// then add(r_b,.) and mul(r_b,.)), sends 2 x 2^k words (phase 1) or its 2 x 2^k / N-word slices (phase 2) to the first
// device, and the two 2^(k+1)-entry product proofs run there, on ordinary single-device passes.

static int multi_gkr_wiring(sc_ctx* m, const int32_t* gate_type, const uint32_t* in0, const uint32_t* in1, size_t k_i, size_t k_next,
                            const uint64_t* r_i, sc_table** add_out, sc_table** mul_out) {
  SC_TRY(multi_enter(m));
  const size_t N = m->subs.size();
  if (k_next > 15 || ((size_t)1 << k_next) < N) return fail(m, SC_ERR_ARG, "sc_gkr_wiring: 2^%zu rows of c over %zu devices", k_next, N);
  const size_t len = (size_t)1 << (2 * k_next);
  TableBuf tm(m, new_multi_table(N, len), /*multi=*/true), ta(m, new_multi_table(N, len), /*multi=*/true);
  if (!ta.get() || !tm.get()) return fail(m, SC_ERR_OOM, "host allocation failed");
  SC_TRY(multi_run(m, [&](int d, sc_ctx* sub) { return sc_gkr_wiring(sub, gate_type, in0, in1, k_i, k_next, r_i, &ta->parts[d], &tm->parts[d]); },
                   /*recoverable=*/true));
  *add_out = ta.release();
  *mul_out = tm.release();
  return SC_OK;
}

static int multi_gkr_w_evaluate(sc_ctx* m, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
                                const uint64_t* point, size_t n, uint64_t* out) {
  if (!out || (n && !point)) return SC_ERR_ARG;
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, add, "gkr W"));
  SC_TRY(check_table(m, mul, "gkr W"));
  SC_TRY(check_table(m, w_b, "gkr W"));
  SC_TRY(check_table(m, w_c, "gkr W"));
  const size_t kb = (size_t)log2_of(w_b->len), kc = (size_t)log2_of(w_c->len);
  if (add->len != mul->len || add->len != ((size_t)1 << (kb + kc)) || n != kb + kc)
    return fail(m, SC_ERR_ARG, "gkr evaluate: the point / add / mul must have num_vars(w_b) + num_vars(w_c) variables");
  u64 ae = 0, me = 0, wb = 0, wc = 0;
  SC_TRY(sc_table_evaluate(m, add, point, n, SC_ORDER_LE, &ae));
  SC_TRY(sc_table_evaluate(m, mul, point, n, SC_ORDER_LE, &me));
  SC_TRY(sc_table_evaluate(m, w_b, point, kb, SC_ORDER_LE, &wb));
  SC_TRY(sc_table_evaluate(m, w_c, point + kb, kc, SC_ORDER_LE, &wc));
  HostField hf(m->fp);
  *out = hf.add(hf.mul(ae, hf.add(wb, wc)), hf.mul(me, hf.mul(wb, wc)));   // round_polynomial.rs:56
  return SC_OK;
}

// a whole copy of a handle's table on one of its devices (pool memory of `dst`)
static int multi_gather_to(sc_ctx* m, const sc_table* t, sc_ctx* dst, PoolBuf* out) {
  const size_t N = t->parts.size(), part = t->len / N;   // (N = 1: a table that lives whole on the first device)
  SC_TRY(set_device(dst));
  PoolBuf whole;
  SC_TRY(whole.alloc(dst, t->len));
  // the parts are read on dst's stream: whatever their own devices' streams are still writing into them (a table call of the
  // handle returns unsynchronised by design, e.g. sc_table_fix_variables) must have landed first - ADVICE r04
  for (size_t q = 0; q < N; ++q)
    if (m->subs[q] != dst && hipStreamSynchronize(m->subs[q]->stream) != hipSuccess)
      return fail(dst, SC_ERR_HIP, "gathering a table of the handle: draining device %zu's stream failed", q);
  for (size_t q = 0; q < N; ++q) {
    const hipError_t e = hipMemcpyPeerAsync(whole + q * part, dst->device, t->parts[q]->d, m->subs[q]->device, part * sizeof(u64), dst->stream);
    if (e != hipSuccess) return fail(dst, SC_ERR_HIP, "gathering a table of the handle: %s", hipGetErrorString(e));
  }
  if (hipStreamSynchronize(dst->stream) != hipSuccess) return fail(dst, SC_ERR_HIP, "gathering a table of the handle: synchronize failed");
  *out = std::move(whole);
  return SC_OK;
}

static int multi_gkr_prover_create(sc_ctx* m, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
                                   sc_gkr_prover** out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, add, "gkr W"));
  SC_TRY(check_table(m, mul, "gkr W"));
  SC_TRY(check_table(m, w_b, "gkr W"));
  SC_TRY(check_table(m, w_c, "gkr W"));
  const size_t N = m->subs.size();
  const int kb = log2_of(w_b->len), kc = log2_of(w_c->len), g = m->log_world;
  if (add->len != mul->len || add->len != ((size_t)1 << (kb + kc)))
    return fail(m, SC_ERR_ARG, "gkr W: add/mul must have num_vars(w_b) + num_vars(w_c) variables");
  if (kb + kc < 1) return fail(m, SC_ERR_ARG, "sc_gkr_prover_create: W has no variables");
  if (N > 1 && (kc < g || kb < 1)) return fail(m, SC_ERR_UNSUPPORTED, "gkr W on %zu devices needs at least log2(devices) variables of c and one of b", N);
  sc_gkr_prover* pr = new (std::nothrow) sc_gkr_prover;
  if (!pr) return fail(m, SC_ERR_OOM, "host allocation failed");
  sc_ctx* first = m->subs[0];
  pr->ctx = first;
  pr->handle = m;
  pr->kb = kb;
  pr->kc = kc;
  pr->add_len = add->parts[0]->len;
  pr->add = add->parts[0]->d;
  pr->mul = mul->parts[0]->d;
  pr->owned.resize(N + 1);
  // W_c whole on every device (phase 1 reads the rows a device owns), W_b whole on the first one
  int rc = multi_run(m, [&](int d, sc_ctx* sub) { return multi_gather_to(m, w_c, sub, &pr->owned[d]); });
  if (rc == SC_OK) {
    rc = multi_gather_to(m, w_b, first, &pr->owned[N]);
    if (rc != SC_OK) rc = fail(m, rc, "%s", first->err.c_str());
  }
  if (rc == SC_OK) {
    pr->w_c = pr->owned[0];
    pr->w_b = pr->owned[N];
    pr->dev.resize(N);
    for (size_t d = 0; d < N; ++d) {
      sc_gkr_prover& v = pr->dev[d];
      v.ctx = m->subs[d];
      v.add = add->parts[d]->d;
      v.mul = mul->parts[d]->d;
      v.add_len = add->parts[d]->len;
      v.w_c = pr->owned[d];
      v.kb = kb;
      v.kc = kc;
    }
    rc = gkr_prover_begin(pr);
    if (rc != SC_OK && m->err.empty()) (void)fail(m, rc, "%s", first->err.c_str());
    else if (rc != SC_OK && first->err.size()) (void)fail(m, rc, "%s", first->err.c_str());
  }
  if (rc != SC_OK) {
    sc_gkr_prover_destroy(pr);
    return rc;
  }
  *out = pr;
  return SC_OK;
}
