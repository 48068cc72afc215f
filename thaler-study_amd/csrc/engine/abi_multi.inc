// Part of sumcheck_hip.hip (included there, last): C ABI of the multi-device handle - sc_ctx_create_multi and the table /
// product entry points on it (the prover's side is in abi_prover.inc; the runtime in multi.inc).

// =====================================================================================
// C ABI: one handle, N devices, one process (SURVEY.md section 8b / 8e)
// =====================================================================================

extern "C" int sc_ctx_create_multi(const sc_field* f, const int* devices, int n_devices, sc_ctx** out) {
  if (!f || !devices || !out) return fail(nullptr, SC_ERR_ARG, "sc_ctx_create_multi: null argument");
  if (n_devices < 1 || n_devices > kMaxSubs || !is_pow2((size_t)n_devices))
    return fail(nullptr, SC_ERR_ARG, "sc_ctx_create_multi: %d devices (a power of two up to %d: the hypercube is split by index bits)",
                n_devices, kMaxSubs);
  sc_ctx* m = new (std::nothrow) sc_ctx;
  if (!m) return fail(nullptr, SC_ERR_OOM, "host allocation failed");
  m->transport = Transport::kLocal;
  m->world = n_devices;
  m->log_world = log2_of((size_t)n_devices);
  m->partial_rows = 4096;   // (only so that the handle's copy of "max_blocks" validates like a shard's)
  for (int d = 0; d < n_devices; ++d) {
    sc_ctx* sub = nullptr;
    int rc = sc_ctx_create(f, devices[d], &sub);
    if (rc == SC_OK) {
      m->subs.push_back(sub);
      sub->parent = m;
      if (n_devices > 1) {
        sub->rank = d;
        sub->world = n_devices;
        sub->log_world = m->log_world;
        sub->transport = Transport::kLocal;
      }
    }
    if (rc != SC_OK) {
      for (sc_ctx* s : m->subs) sc_ctx_destroy(s);
      m->subs.clear();
      delete m;
      return rc;
    }
  }
  m->fp = m->subs[0]->fp;
  m->gold = m->subs[0]->gold;
  m->device = devices[0];
  m->num_cus = m->subs[0]->num_cus;
  m->max_blocks = m->subs[0]->max_blocks;
  m->mrt = new (std::nothrow) MultiRuntime;
  if (!m->mrt) {
    for (sc_ctx* s : m->subs) sc_ctx_destroy(s);
    m->subs.clear();
    delete m;
    return fail(nullptr, SC_ERR_OOM, "host allocation failed");
  }
  m->mrt->start(n_devices);
  // the tail slots of the shards' pinned buffers: the lower half for the handle's provers (the same index on every shard), the
  // upper half for provers created on a shard itself (the small product proofs of the GKR phases run on the first device)
  for (int i = kTailSlots / 2 - 1; i >= 0; --i) m->tail_free.push_back(i);
  for (sc_ctx* s : m->subs) {
    s->tail_free.clear();
    for (int i = kTailSlots - 1; i >= kTailSlots / 2; --i) s->tail_free.push_back(i);
  }
  *out = m;
  return SC_OK;
}

static int multi_destroy(sc_ctx* m) {
  if (m->mrt) {
    m->mrt->stop();
    delete m->mrt;
  }
  for (sc_ctx* s : m->subs) sc_ctx_destroy(s);
  m->subs.clear();   // (sc_ctx_destroy on it would dispatch here again)
  delete m;
  return SC_OK;
}

static int multi_set_option(sc_ctx* m, const char* key, int64_t value) {
  SC_TRY(multi_enter(m));
  const std::string k(key);
  if (k == "use_mailbox" && !value) return fail(m, SC_ERR_UNSUPPORTED, "a multi-device handle adds its shards' sums from their mailboxes");
  if (const OptionSpec* o = find_option(key); o && (o->flags & kOptPeer))
    return fail(m, SC_ERR_UNSUPPORTED, "'%s' belongs to the peer transport; a multi-device handle has no exchange between kernels", key);
  for (sc_ctx* s : m->subs) {
    const int rc = sc_ctx_set_option(s, key, value);
    if (rc != SC_OK) return fail(m, rc, "%s", s->err.c_str());
  }
  return SC_OK;
}

static int multi_synchronize(sc_ctx* m) {
  SC_TRY(multi_enter(m));
  return multi_run(m, [](int, sc_ctx* sub) { return sc_ctx_synchronize(sub); });
}

// ---- the first-device path (round 5) ---------------------------------------------------------------------------
//
// Everything a handle cannot do shard by shard - a table with fewer entries than devices, fix_variables across the device
// bits (LE: more variables than a shard has; BE: the first variable IS a device bit), relabel, and the callers' GENERIC trait
// methods (sc_gkr_w_round_sums / _to_evaluations, sc_tri_round_sums / _to_evaluations: the reference's fallback loop
// `fix_variables -> to_univariate`, gkr-protocol/src/round_polynomial.rs:59-90, triangle-counting/src/lib.rs:89-132, which
// walks every evaluation every round and is the slow path there too) - runs on the handle's FIRST device on whole tables:
// gather (hipMemcpyPeerAsync; xGMI between distinct devices), the ordinary entry point of that device's context, scatter of
// table results back into the handle's layout.  Functional, not fast: the native engines (sc_prover_*, sc_gkr_prover_*,
// sc_tri_prover_*) are the paths that use every device.  A table with fewer entries than the handle has devices lives
// whole on the first device ("single": one part).
namespace {

struct FirstView {
  sc_table view;        // an ordinary table of subs[0] holding the whole of a handle's table (borrowed or `owned`)
  PoolBuf owned;
};
int to_first(sc_ctx* m, const sc_table* t, FirstView* v) {
  sc_ctx* first = m->subs[0];
  v->owned.reset();
  v->view.len = t->len;
  if (t->parts.size() == 1) {   // single, or a handle over one device
    v->view.d = t->parts[0]->d;
    return SC_OK;
  }
  SC_TRY(multi_gather_to(m, t, first, &v->owned));
  v->view.d = v->owned;
  return SC_OK;
}
void drop_first(FirstView* v) { v->owned.reset(); }
// an ordinary table of subs[0] (consumed) -> a table of the handle
int from_first(sc_ctx* m, TableBuf&& w_in, sc_table** out) {
  sc_ctx* first = m->subs[0];
  const size_t N = m->subs.size();
  if (N == 1 || w_in->len < N) {
    TableBuf w(std::move(w_in));
    sc_table* t = new_multi_table(1, w->len);
    if (!t) return fail(m, SC_ERR_OOM, "host allocation failed");
    t->parts[0] = w.release();
    *out = t;
    return SC_OK;
  }
  const size_t part = w_in->len / N;
  TableBuf t(m, new_multi_table(N, w_in->len), /*multi=*/true);
  TableBuf w(std::move(w_in));   // (goes back first)
  if (!t.get()) return fail(m, SC_ERR_OOM, "host allocation failed");
  // every device allocates its part and drains its stream (the first device's stream writes into the recycled block)
  SC_TRY(multi_run(m, [&](int d, sc_ctx* sub) -> int {
    SC_TRY(set_device(sub));
    SC_TRY(new_table(sub, part, &t->parts[d]));
    SC_HIP(sub, hipStreamSynchronize(sub->stream));
    return SC_OK;
  }, /*recoverable=*/true));
  SC_TRY(set_device(first));
  for (size_t q = 0; q < N; ++q) {
    const hipError_t e = hipMemcpyPeerAsync(t->parts[q]->d, m->subs[q]->device, w->d + q * part, first->device, part * sizeof(u64), first->stream);
    if (e != hipSuccess) return fail(m, SC_ERR_HIP, "scattering a table over the handle's devices: %s", hipGetErrorString(e));
  }
  if (hipStreamSynchronize(first->stream) != hipSuccess) return fail(m, SC_ERR_HIP, "scattering a table over the handle's devices: synchronize failed");
  w.reset();
  *out = t.release();
  return SC_OK;
}
// the two results of one call on the first device -> two tables of the handle (or none)
int from_first_pair(sc_ctx* m, TableBuf&& wa, TableBuf&& wb, sc_table** a_out, sc_table** b_out) {
  TableBuf ta;   // (adopted as a table the handle hands out: should the second fail, it is freed the way a caller would, sc_table_free on the handle)
  SC_TRY(from_first(m, std::move(wa), ta.out(m)));
  SC_TRY(from_first(m, std::move(wb), b_out));
  *a_out = ta.release();
  return SC_OK;
}
// rc of a call made on the first device -> the handle's error
int first_rc(sc_ctx* m, int rc) { return rc == SC_OK ? SC_OK : fail(m, rc, "%s", m->subs[0]->err.c_str()); }
// The first device's context is shard 0 of world N (Transport::kLocal): for a call on WHOLE tables it is, for the duration of
// that call, an ordinary unsharded context.  (Objects created inside - a prover over tables that live on the first device -
// record "not sharded" at creation and stay that way.)
struct AsWhole {
  sc_ctx* c;
  Transport t;
  int rank, world, log_world;
  explicit AsWhole(sc_ctx* ctx) : c(ctx), t(ctx->transport), rank(ctx->rank), world(ctx->world), log_world(ctx->log_world) {
    c->transport = Transport::kNone;
    c->rank = 0;
    c->world = 1;
    c->log_world = 0;
  }
  ~AsWhole() {
    c->transport = t;
    c->rank = rank;
    c->world = world;
    c->log_world = log_world;
  }
};
template <class Fn>
int on_first(sc_ctx* m, Fn fn) {
  AsWhole whole(m->subs[0]);
  return first_rc(m, fn(m->subs[0]));
}

// op(first, views[0..n)) -> a table: gather the inputs, run, scatter the result
int via_first_table(sc_ctx* m, std::initializer_list<const sc_table*> ins, const std::function<int(sc_ctx*, FirstView*, sc_table**)>& op, sc_table** out) {
  FirstView v[4];
  int n = 0, rc = SC_OK;
  for (const sc_table* t : ins) {
    rc = to_first(m, t, &v[n]);
    if (rc != SC_OK) break;
    ++n;
  }
  TableBuf w;
  if (rc == SC_OK) rc = on_first(m, [&](sc_ctx* first) { return op(first, v, w.out(first)); });
  for (int i = 0; i < n; ++i) drop_first(&v[i]);
  if (rc != SC_OK) return rc;
  return from_first(m, std::move(w), out);
}
// op(first, views) -> words on the host
int via_first_value(sc_ctx* m, std::initializer_list<const sc_table*> ins, const std::function<int(sc_ctx*, FirstView*)>& op) {
  FirstView v[4];
  int n = 0, rc = SC_OK;
  for (const sc_table* t : ins) {
    rc = to_first(m, t, &v[n]);
    if (rc != SC_OK) break;
    ++n;
  }
  if (rc == SC_OK) rc = on_first(m, [&](sc_ctx* first) { return op(first, v); });
  for (int i = 0; i < n; ++i) drop_first(&v[i]);
  return rc;
}

}  // namespace

// ---- tables (new_multi_table / drop_multi_table / make_multi_table: multi.inc) ------------------------

static int multi_table_upload(sc_ctx* m, const uint64_t* host, size_t len, sc_table** out) {
  SC_TRY(multi_enter(m));
  if (is_pow2(len) && len < m->subs.size()) {   // fewer entries than devices: whole on the first device
    TableBuf w;
    SC_TRY(on_first(m, [&](sc_ctx* first) { return sc_table_upload(first, host, len, w.out(first)); }));
    return from_first(m, std::move(w), out);
  }
  SC_TRY(check_multi_len(m, len, "sc_table_upload"));
  const size_t part = len / m->subs.size();
  return make_multi_table(m, len, [&](int d, sc_ctx* sub, sc_table** p) { return sc_table_upload(sub, host + (size_t)d * part, part, p); }, out);
}

static int multi_table_generate(sc_ctx* m, uint64_t seed, uint64_t start, size_t len, sc_table** out) {
  SC_TRY(multi_enter(m));
  if (is_pow2(len) && len < m->subs.size()) {
    TableBuf w;
    SC_TRY(on_first(m, [&](sc_ctx* first) { return sc_table_generate(first, seed, start, len, w.out(first)); }));
    return from_first(m, std::move(w), out);
  }
  SC_TRY(check_multi_len(m, len, "sc_table_generate"));
  const size_t part = len / m->subs.size();
  return make_multi_table(m, len, [&](int d, sc_ctx* sub, sc_table** p) { return sc_table_generate(sub, seed, start + (u64)d * part, part, p); },
                          out);
}

static int multi_table_clone(sc_ctx* m, const sc_table* t, sc_table** out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, t, "sc_table_clone"));
  if (is_single(m, t)) {
    TableBuf w;
    SC_TRY(on_first(m, [&](sc_ctx* first) { return sc_table_clone(first, t->parts[0], w.out(first)); }));
    return from_first(m, std::move(w), out);
  }
  return make_multi_table(m, t->len, [&](int d, sc_ctx* sub, sc_table** p) { return sc_table_clone(sub, t->parts[d], p); }, out);
}

static int multi_table_download(sc_ctx* m, const sc_table* t, uint64_t* host, size_t len) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, t, "sc_table_download"));
  if (len != t->len) return fail(m, SC_ERR_ARG, "sc_table_download: len %zu != table len %zu", len, t->len);
  if (is_single(m, t)) return on_first(m, [&](sc_ctx* first) { return sc_table_download(first, t->parts[0], host, len); });
  const size_t part = len / m->subs.size();
  return multi_run(m, [&](int d, sc_ctx* sub) { return sc_table_download(sub, t->parts[d], host + (size_t)d * part, part); },
                   /*recoverable=*/true);
}

static int multi_table_free(sc_ctx* m, sc_table* t) {
  if (!is_multi(m) || (t->parts.size() != m->subs.size() && t->parts.size() != 1))
    return fail(m, SC_ERR_ARG, "sc_table_free: the table does not belong to this context");
  drop_multi_table(m, t);   // pool bookkeeping only: no launcher threads needed
  return SC_OK;
}

// fix_variables of the k LOW variables while they stay inside a shard (LE order; the sumcheck callers' order)
static int multi_table_fix_variables(sc_ctx* m, const sc_table* in, const uint64_t* r, size_t k, int order, sc_table** out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, in, "sc_table_fix_variables"));
  const int nl = log2_of(in->parts[0]->len);
  if (k > (size_t)log2_of(in->len)) return fail(m, SC_ERR_ARG, "fix_variables: k=%zu > num_vars=%d", k, log2_of(in->len));
  if (order != SC_ORDER_LE && order != SC_ORDER_BE) return fail(m, SC_ERR_ARG, "bad order %d", order);
  // across the device bits (LE: more variables than a shard has; BE: the first variable is the top index bit, a device bit), or
  // a table that lives on the first device anyway: the first-device path (round 5; SC_ERR_UNSUPPORTED before)
  if (m->subs.size() > 1 && k > 0 && (is_single(m, in) || k > (size_t)nl || order == SC_ORDER_BE))
    return via_first_table(m, {in}, [&](sc_ctx* first, FirstView* v, sc_table** w) { return sc_table_fix_variables(first, &v[0].view, r, k, order, w); }, out);
  if (is_single(m, in)) return multi_table_clone(m, in, out);   // (k = 0)
  return make_multi_table(m, in->len >> k, [&](int d, sc_ctx* sub, sc_table** p) { return sc_table_fix_variables(sub, in->parts[d], r, k, order, p); },
                          out);
}

static int multi_table_evaluate(sc_ctx* m, const sc_table* t, const uint64_t* r, size_t n, int order, uint64_t* out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, t, "sc_table_evaluate"));
  if (is_single(m, t)) return on_first(m, [&](sc_ctx* first) { return sc_table_evaluate(first, t->parts[0], r, n, order, out); });
  return multi_sums(m, 1, [&](int d, sc_ctx* sub, bool* mb) {
    return table_evaluate_launch(sub, t->parts[d]->d, t->parts[d]->len, r, n, order, mb);
  }, out);
}

// ---- product of two tables ----------------------------------------------------------------------

static int multi_prod2_to_evaluations(sc_ctx* m, const sc_table* a, const sc_table* b, sc_table** out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_pair(m, a, b, "sc_prod2_to_evaluations"));
  if (is_single(m, a))
    return via_first_table(m, {a, b}, [&](sc_ctx* first, FirstView* v, sc_table** w) { return sc_prod2_to_evaluations(first, &v[0].view, &v[1].view, w); }, out);
  return make_multi_table(m, a->len, [&](int d, sc_ctx* sub, sc_table** p) { return sc_prod2_to_evaluations(sub, a->parts[d], b->parts[d], p); }, out);
}

static int multi_prod2_round_sums(sc_ctx* m, const sc_table* a, const sc_table* b, uint64_t out_e[3]) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_pair(m, a, b, "sc_prod2_round_sums"));
  const size_t part = a->parts[0]->len;
  if (a->len < 2) return fail(m, SC_ERR_ARG, "sc_prod2_round_sums: no variable left");
  if (is_single(m, a) || part < 2)   // the pairs of the round's variable are not inside a shard: the first-device path
    return via_first_value(m, {a, b}, [&](sc_ctx* first, FirstView* v) { return sc_prod2_round_sums(first, &v[0].view, &v[1].view, out_e); });
  const bool across = m->subs.size() > 1;
  SC_TRY(multi_sums(m, 3, [&](int d, sc_ctx* sub, bool* mb) {
    SC_TRY(set_device(sub));
    return launch_pass(sub, 0, 1, a->parts[d]->d, b->parts[d]->d, nullptr, nullptr, nullptr, log2_of(part), across, mb);
  }, out_e));
  HostField hf(m->fp);
  out_e[2] = eval2_from_inf(hf, out_e[0], out_e[1], out_e[2]);   // the kernel sums H(0), H(1), H(inf)
  return SC_OK;
}

static int multi_prod2_sum(sc_ctx* m, const sc_table* a, const sc_table* b, uint64_t* out_c1) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_pair(m, a, b, "sc_prod2_sum"));
  HostField hf(m->fp);
  if (is_single(m, a)) return via_first_value(m, {a, b}, [&](sc_ctx* first, FirstView* v) { return sc_prod2_sum(first, &v[0].view, &v[1].view, out_c1); });
  if (a->parts[0]->len == 1) {
    // one entry per shard: the partial sum is the single product
    return multi_sums(m, 1, [&](int d, sc_ctx* sub, bool* mb) -> int {
      SC_TRY(set_device(sub));
      PoolBuf prod;
      SC_TRY(prod.alloc(sub, 1));
      SC_DISPATCH_FIELD(sub, F, f, hipLaunchKernelGGL((sc::mul_kernel<F>), dim3(1), dim3(sc::kBlock), 0, sub->stream, f,
                                                      (const u64*)a->parts[d]->d, (const u64*)b->parts[d]->d, prod.get(), (size_t)1));
      SC_DISPATCH_FIELD(sub, F, f, hipLaunchKernelGGL((sc::scale_split_kernel<F>), dim3(1), dim3(64), 0, sub->stream, f,
                                                      (const u64*)prod, hf.one(), sub->d_sums));
      prod.reset();
      SC_HIP(sub, hipGetLastError());
      *mb = false;
      return SC_OK;
    }, out_c1);
  }
  u64 e[3];
  SC_TRY(multi_prod2_round_sums(m, a, b, e));
  *out_c1 = hf.add(e[0], e[1]);   // c_1 = H(0) + H(1)
  return SC_OK;
}

static int multi_prod2_fold_and_sums(sc_ctx* m, const sc_table* a, const sc_table* b, const uint64_t r[1], sc_table** a_out,
                                     sc_table** b_out, uint64_t out_e[3]) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_pair(m, a, b, "sc_prod2_fold_and_sums"));
  const size_t part = a->parts[0]->len;
  const int nv = log2_of(part);
  if (log2_of(a->len) < 2) return fail(m, SC_ERR_ARG, "sc_prod2_fold_and_sums: needs >= 2 variables (fold one, sum over one)");
  if (is_single(m, a) || nv < 2) {
    // the fold or the next round's pairs cross the shards: both on the first device, the folded tables scattered back
    FirstView va, vb;
    SC_TRY(to_first(m, a, &va));
    int rc = to_first(m, b, &vb);
    TableBuf wb, wa;
    if (rc == SC_OK) rc = on_first(m, [&](sc_ctx* first) { return sc_prod2_fold_and_sums(first, &va.view, &vb.view, r, wa.out(first), wb.out(first), out_e); });
    drop_first(&va);
    drop_first(&vb);
    if (rc != SC_OK) return rc;
    return from_first_pair(m, std::move(wa), std::move(wb), a_out, b_out);
  }
  TableBuf tb(m, new_multi_table(m->subs.size(), a->len / 2), /*multi=*/true), ta(m, new_multi_table(m->subs.size(), a->len / 2), /*multi=*/true);
  if (!ta.get() || !tb.get()) return fail(m, SC_ERR_OOM, "host allocation failed");
  const bool across = m->subs.size() > 1;
  SC_TRY(multi_sums(m, 3, [&](int d, sc_ctx* sub, bool* mb) -> int {
    SC_TRY(set_device(sub));
    SC_TRY(new_table(sub, part / 2, &ta->parts[d]));
    SC_TRY(new_table(sub, part / 2, &tb->parts[d]));
    return launch_pass(sub, 1, 1, a->parts[d]->d, b->parts[d]->d, ta->parts[d]->d, tb->parts[d]->d, r, nv, across, mb);
  }, out_e));
  HostField hf(m->fp);
  out_e[2] = eval2_from_inf(hf, out_e[0], out_e[1], out_e[2]);
  *a_out = ta.release();
  *b_out = tb.release();
  return SC_OK;
}

// G::new on a multi-device handle (matrix-multiplication/src/lib.rs:77-92; BASELINE config 5's shape): A and B are split
// by ROW blocks over the devices (they are the handle's tables of 2^(2n) entries: top index bits = row).  f_b = B~(z, r2)
// has z = row, so each device folds its own rows: no exchange.  f_a = A~(r1, z) has z = column and sums over rows: every
// device computes a partial vector over all columns from its rows (coldot), sends column block q to device q
// (hipMemcpyPeerAsync: xGMI between distinct devices, 2^n * 8 / N bytes each) and device q adds the N partial blocks mod p.
static int multi_matmul_g_new(sc_ctx* m, const sc_table* A, const sc_table* B, size_t n, const uint64_t* point, sc_table** a_out,
                              sc_table** b_out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_pair(m, A, B, "sc_matmul_g_new"));
  const size_t N = m->subs.size();
  const int g = m->log_world;
  if (A->len != ((size_t)1 << (2 * n))) return fail(m, SC_ERR_ARG, "sc_matmul_g_new: tables must have 2^(2n) entries");
  if (N > 1 && n >= 1 && (n < (size_t)g || (((size_t)1 << n) >> g) < 2)) {
    // matrices with fewer than two columns per device: G::new on the first device, f_a and f_b handed back in the handle's layout
    FirstView va, vb;
    SC_TRY(to_first(m, A, &va));
    int rc = to_first(m, B, &vb);
    TableBuf wb, wa;
    if (rc == SC_OK) rc = on_first(m, [&](sc_ctx* first) { return sc_matmul_g_new(first, &va.view, &vb.view, n, point, wa.out(first), wb.out(first)); });
    drop_first(&va);
    drop_first(&vb);
    if (rc != SC_OK) return rc;
    return from_first_pair(m, std::move(wa), std::move(wb), a_out, b_out);
  }
  if (n < (size_t)g || n == 0) return fail(m, n == 0 && N == 1 ? SC_ERR_UNSUPPORTED : SC_ERR_ARG, "sc_matmul_g_new: 2^%zu rows cannot be split over %zu devices", n, N);
  const size_t side = (size_t)1 << n, rows_local = side >> g, cols_local = side >> g;
  if (N == 1) {
    TableBuf tb(m, new_multi_table(1, side), /*multi=*/true), ta(m, new_multi_table(1, side), /*multi=*/true);
    if (!ta.get() || !tb.get()) return fail(m, SC_ERR_OOM, "host allocation failed");
    const int rc = sc_matmul_g_new(m->subs[0], A->parts[0], B->parts[0], n, point, &ta->parts[0], &tb->parts[0]);
    if (rc != SC_OK) return fail(m, rc, "%s", m->subs[0]->err.c_str());
    *a_out = ta.release();
    *b_out = tb.release();
    return SC_OK;
  }
  if (cols_local < 2) return fail(m, SC_ERR_UNSUPPORTED, "sc_matmul_g_new: fewer than two columns per device");
  TableBuf tb(m, new_multi_table(N, side), /*multi=*/true), ta(m, new_multi_table(N, side), /*multi=*/true);
  if (!ta.get() || !tb.get()) return fail(m, SC_ERR_OOM, "host allocation failed");
  PoolBuf stage[kMaxSubs];   // stage[q]: N partial blocks of device q's columns, [source][cols_local]
  PoolBuf partial[kMaxSubs];
  // phase 1: partial vectors, scattered by column block
  // (stage[d] is written by the OTHER devices' streams: a pool block is stream-ordered on its own context's stream only, so its
  // owner drains that stream before anyone else may touch the block - ADVICE r04; multi_run returns when every device has)
  int rc = multi_run(m, [&](int d, sc_ctx* sub) -> int {
    SC_TRY(set_device(sub));
    SC_TRY(stage[d].alloc(sub, N * cols_local));
    SC_TRY(partial[d].alloc(sub, side));
    SC_HIP(sub, hipStreamSynchronize(sub->stream));
    return SC_OK;
  });
  if (rc == SC_OK)
    rc = multi_run(m, [&](int d, sc_ctx* sub) -> int {
      SC_TRY(set_device(sub));
      PoolBuf eq;
      SC_TRY(build_eq_table(sub, point, (int)n, &eq));
      const int r2 = coldot(sub, A->parts[d]->d, eq + (size_t)d * rows_local, rows_local, side, partial[d]);
      eq.reset();
      SC_TRY(r2);
      for (size_t q = 0; q < N; ++q)
        SC_HIP(sub, hipMemcpyPeerAsync(stage[q] + (size_t)d * cols_local, m->subs[q]->device, partial[d] + q * cols_local, sub->device,
                                       cols_local * sizeof(u64), sub->stream));
      SC_HIP(sub, hipStreamSynchronize(sub->stream));
      return SC_OK;
    });
  // phase 2: every device adds the blocks it received; f_b from its own rows
  if (rc == SC_OK)
    rc = multi_run(m, [&](int d, sc_ctx* sub) -> int {
      SC_TRY(set_device(sub));
      SC_TRY(new_table(sub, cols_local, &ta->parts[d]));
      SC_DISPATCH_FIELD(sub, F, f, hipLaunchKernelGGL((sc::sum_rows_kernel<F>), dim3(grid_for_wide(sub, cols_local), 1), dim3(sc::kBlock), 0,
                                                      sub->stream, f, (const u64*)stage[d], (const u64*)stage[d], N, cols_local,
                                                      ta->parts[d]->d, ta->parts[d]->d));
      SC_HIP(sub, hipGetLastError());
      PoolBuf folded;
      size_t folded_len = 0;
      SC_TRY(fold_chain(sub, B->parts[d]->d, B->parts[d]->len, point + n, n, SC_ORDER_LE, &folded, &folded_len));
      TableBuf fb;
      SC_TRY(fb.wrap(sub, std::move(folded), folded_len));
      tb->parts[d] = fb.release();
      SC_HIP(sub, hipStreamSynchronize(sub->stream));
      return SC_OK;
    });
  for (size_t d = 0; d < N; ++d) {
    stage[d].reset();
    partial[d].reset();
  }
  SC_TRY(rc);
  *a_out = ta.release();
  *b_out = tb.release();
  return SC_OK;
}

// ---- the generic trait path of the callers' own polynomial types, and relabel: first-device path (top of this file) ----------

static int multi_table_relabel(sc_ctx* m, const sc_table* in, size_t a, size_t b, size_t k, sc_table** out) {
  SC_TRY(multi_enter(m));
  SC_TRY(check_table(m, in, "sc_table_relabel"));
  return via_first_table(m, {in}, [&](sc_ctx* first, FirstView* v, sc_table** w) { return sc_table_relabel(first, &v[0].view, a, b, k, w); }, out);
}

// gkr_protocol::round_polynomial::W, generic methods (gkr-protocol/src/round_polynomial.rs:59-119).  On the first device the
// tables are ordinary whole tables: an unsharded W.
static int multi_gkr_w_to_evaluations(sc_ctx* m, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c, sc_table** out) {
  SC_TRY(multi_enter(m));
  WView w;
  SC_TRY(check_w(m, add, mul, w_b, w_c, &w));
  return via_first_table(m, {add, mul, w_b, w_c}, [&](sc_ctx* first, FirstView* v, sc_table** t) {
    return sc_gkr_w_to_evaluations(first, &v[0].view, &v[1].view, &v[2].view, &v[3].view, t);
  }, out);
}
static int multi_gkr_w_round_sums(sc_ctx* m, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c, uint64_t out_e[3]) {
  SC_TRY(multi_enter(m));
  WView w;
  SC_TRY(check_w(m, add, mul, w_b, w_c, &w));
  return via_first_value(m, {add, mul, w_b, w_c}, [&](sc_ctx* first, FirstView* v) {
    return sc_gkr_w_round_sums(first, &v[0].view, &v[1].view, &v[2].view, &v[3].view, out_e);
  });
}

// triangle_counting::G, generic methods (triangle-counting/src/lib.rs:89-166)
static int multi_tri_to_evaluations(sc_ctx* m, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len, sc_table** out) {
  SC_TRY(multi_enter(m));
  TriView tv;
  SC_TRY(check_tri(m, f1, f2, f3, var_len, &tv));
  return via_first_table(m, {f1, f2, f3}, [&](sc_ctx* first, FirstView* v, sc_table** t) {
    return sc_tri_to_evaluations(first, &v[0].view, &v[1].view, &v[2].view, var_len, t);
  }, out);
}
static int multi_tri_round_sums(sc_ctx* m, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len, uint64_t out_e[3]) {
  SC_TRY(multi_enter(m));
  TriView tv;
  SC_TRY(check_tri(m, f1, f2, f3, var_len, &tv));
  return via_first_value(m, {f1, f2, f3}, [&](sc_ctx* first, FirstView* v) {
    return sc_tri_round_sums(first, &v[0].view, &v[1].view, &v[2].view, var_len, out_e);
  });
}
