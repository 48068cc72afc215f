// Part of sumcheck_hip.hip (included there, in order): C ABI: field helpers, context, options.

// =====================================================================================
// C ABI: field helpers
// =====================================================================================

extern "C" int sc_field_from_modulus(uint64_t p, sc_field* out) {
  if (!out) return SC_ERR_ARG;
  sc::FieldParams fp;
  if (!sc::field_params_from_modulus(p, &fp)) return SC_ERR_ARG;
  out->p = fp.p;
  out->p_inv_neg = fp.p_inv_neg;
  out->r_mod_p = fp.r_mod_p;
  out->r2_mod_p = fp.r2_mod_p;
  return SC_OK;
}

static sc::FieldParams to_params(const sc_field* f) {
  sc::FieldParams fp;
  fp.p = f->p;
  fp.p_inv_neg = f->p_inv_neg;
  fp.r_mod_p = f->r_mod_p;
  fp.r2_mod_p = f->r2_mod_p;
  return fp;
}

extern "C" uint64_t sc_field_to_mont(const sc_field* f, uint64_t canonical) {
  HostField hf(to_params(f));
  return hf.mul(canonical % f->p, f->r2_mod_p);
}
extern "C" uint64_t sc_field_from_mont(const sc_field* f, uint64_t mont) {
  HostField hf(to_params(f));
  return hf.mul(mont, 1);
}

// matrix-multiplication/src/lib.rs:17-60 with x = 0, 1, 2: Lagrange basis polynomials
// scaled by y_i / denominator_i and summed coefficient-wise.
extern "C" int sc_interpolate_quadratic(const sc_field* f, const uint64_t e[3], uint64_t c[3]) {
  if (!f || !e || !c || f->p < 3) return SC_ERR_ARG;
  HostField hf(to_params(f));
  u64 x[3] = {0, hf.one(), hf.add(hf.one(), hf.one())};
  c[0] = c[1] = c[2] = 0;
  for (int i = 0; i < 3; ++i) {
    int j = (i + 1) % 3, k = (i + 2) % 3;
    u64 dinv = hf.inv(hf.mul(hf.sub(x[i], x[j]), hf.sub(x[i], x[k])));
    u64 w = hf.mul(e[i], dinv);
    c[0] = hf.add(c[0], hf.mul(hf.mul(x[j], x[k]), w));
    c[1] = hf.add(c[1], hf.mul(hf.sub(hf.neg(x[j]), x[k]), w));
    c[2] = hf.add(c[2], w);
  }
  return SC_OK;
}

// =====================================================================================
// C ABI: context
// =====================================================================================

extern "C" int sc_abi_version(void) { return SC_ABI_VERSION; }

extern "C" int sc_ctx_create(const sc_field* f, int device, sc_ctx** out) {
  if (!f || !out) return fail(nullptr, SC_ERR_ARG, "sc_ctx_create: null argument");
  sc_field chk;
  if (sc_field_from_modulus(f->p, &chk) != SC_OK || chk.p_inv_neg != f->p_inv_neg ||
      chk.r_mod_p != f->r_mod_p || chk.r2_mod_p != f->r2_mod_p)
    return fail(nullptr, SC_ERR_ARG, "sc_ctx_create: inconsistent field constants for p=%llu",
                (unsigned long long)f->p);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, SC_ERR_HIP, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(nullptr, SC_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
  sc_ctx* ctx = new (std::nothrow) sc_ctx;
  if (!ctx) return fail(nullptr, SC_ERR_OOM, "host allocation failed");
  ctx->fp = to_params(f);
  ctx->gold = (f->p == sc::GoldilocksMont::P);
  ctx->device = device;
#define SC_CREATE_HIP(call)                                                                \
  do {                                                                                     \
    hipError_t e2_ = (call);                                                               \
    if (e2_ != hipSuccess) {                                                               \
      int rc_ = fail(nullptr, SC_ERR_HIP, "%s: %s", #call, hipGetErrorString(e2_));        \
      sc_ctx_destroy(ctx);                                                                 \
      return rc_;                                                                          \
    }                                                                                      \
  } while (0)
  SC_CREATE_HIP(hipSetDevice(device));
  SC_CREATE_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->num_cus = cus;
    ctx->max_blocks = 3 * ctx->num_cus;
  }
  ctx->partial_rows = 4096;
  SC_CREATE_HIP(hipMalloc(&ctx->d_partials, ctx->partial_rows * 32 * sizeof(u64)));
  SC_CREATE_HIP(hipMalloc(&ctx->d_sums, 512 * sizeof(u64)));   // up to 2 x 243 split limbs of a five-round pass
  SC_CREATE_HIP(hipHostMalloc(&ctx->h_sums, 512 * sizeof(u64), hipHostMallocDefault));
  SC_CREATE_HIP(hipMalloc(&ctx->d_ticket, 64));
  SC_CREATE_HIP(hipMemset(ctx->d_ticket, 0, 64));
  SC_CREATE_HIP(hipHostMalloc(&ctx->h_mailbox, sc::kMailboxWords * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
  memset(ctx->h_mailbox, 0, sc::kMailboxWords * sizeof(u64));
  SC_CREATE_HIP(hipMalloc(&ctx->d_wg_partials, (size_t)kWgMaxBlocks * sc::kGridChunk * sizeof(u64)));
  SC_CREATE_HIP(hipMalloc(&ctx->d_wg_groups, (size_t)(kWgMaxBlocks / sc::kWgGroupBlocks) * sc::kGridChunk * sizeof(u64)));
  SC_CREATE_HIP(hipMalloc(&ctx->d_wg_tickets, 64 * sizeof(unsigned)));
  SC_CREATE_HIP(hipMemset(ctx->d_wg_tickets, 0, 64 * sizeof(unsigned)));
  SC_CREATE_HIP(hipHostGetDevicePointer((void**)&ctx->d_mailbox, ctx->h_mailbox, 0));
  SC_CREATE_HIP(hipHostMalloc(&ctx->h_tail, kTailSlots * kTailSlotWords * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
  memset(ctx->h_tail, 0, kTailSlots * kTailSlotWords * sizeof(u64));
  SC_CREATE_HIP(hipHostGetDevicePointer((void**)&ctx->d_tail, ctx->h_tail, 0));
  for (int i = kTailSlots - 1; i >= 0; --i) ctx->tail_free.push_back(i);
  SC_CREATE_HIP(hipDeviceSynchronize());
  for (int i = 0; i < sc_ctx::kTimerRing; ++i) {
    SC_CREATE_HIP(hipEventCreate(&ctx->kt_ev[i][0]));
    SC_CREATE_HIP(hipEventCreate(&ctx->kt_ev[i][1]));
  }
#undef SC_CREATE_HIP
  *out = ctx;
  return SC_OK;
}

extern "C" int sc_ctx_destroy(sc_ctx* ctx) {
  if (!ctx) return SC_OK;
  if (is_multi(ctx)) return multi_destroy(ctx);
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)sync_stream(ctx);
  if (ctx->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm);
  for (int q = 0; q < sc::kMaxPeers; ++q)
    if (ctx->peer_ipc_opened[q] && ctx->peer_base[q]) (void)hipIpcCloseMemHandle(ctx->peer_base[q]);
  if (ctx->peer_region) (void)hipFree(ctx->peer_region);
  for (auto& kv : ctx->pool_free) (void)hipFree(kv.second);
  for (auto& kv : ctx->pool_live) (void)hipFree(kv.first);
  if (ctx->d_partials) (void)hipFree(ctx->d_partials);
  if (ctx->d_wg_partials) (void)hipFree(ctx->d_wg_partials);
  if (ctx->d_wg_groups) (void)hipFree(ctx->d_wg_groups);
  if (ctx->d_wg_tickets) (void)hipFree(ctx->d_wg_tickets);
  if (ctx->d_gram_rows) (void)hipFree(ctx->d_gram_rows);
  if (ctx->d_sums) (void)hipFree(ctx->d_sums);
  if (ctx->h_sums) (void)hipHostFree(ctx->h_sums);
  if (ctx->h_mailbox) (void)hipHostFree(ctx->h_mailbox);
  if (ctx->h_tail) (void)hipHostFree(ctx->h_tail);
  if (ctx->h_points) (void)hipHostFree(ctx->h_points);
  if (ctx->d_points) (void)hipFree(ctx->d_points);
  for (u64* tw : ctx->d_rs_twiddles)
    if (tw) (void)hipFree(tw);
  for (u64* tw : ctx->d_rs_twist)
    if (tw) (void)hipFree(tw);
  if (ctx->d_xc_inv) (void)hipFree(ctx->d_xc_inv);
  if (ctx->h_batch_desc) (void)hipHostFree(ctx->h_batch_desc);
  if (ctx->h_batch) (void)hipHostFree(ctx->h_batch);
  if (ctx->d_ticket) (void)hipFree(ctx->d_ticket);
  for (int i = 0; i < sc_ctx::kTimerRing; ++i)
    for (int k = 0; k < 2; ++k)
      if (ctx->kt_ev[i][k]) (void)hipEventDestroy(ctx->kt_ev[i][k]);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return SC_OK;
}

extern "C" const char* sc_last_error(const sc_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

static int prewarm(sc_ctx* ctx, size_t num_vars);   // abi_prover.inc

// The options that are plain settings of the context: sc_ctx_set_option validates and stores them, sc_ctx_get_option reads
// them back.  A value is accepted in lo..hi, or as 0 too (kOptOff: 0 = never), or is any value stored as 0 / 1 (kOptBool).
// kOptPeer: the option belongs to the peer transport, and a multi-device handle (no exchange between kernels) refuses it.
enum : unsigned { kOptBool = 1, kOptOff = 2, kOptPeer = 4 };
struct OptionSpec {
  const char* name;
  int sc_ctx::*member;
  int64_t lo, hi;
  unsigned flags;
};
const OptionSpec kOptions[] = {
    {"vars_per_pass", &sc_ctx::vars_per_pass, 1, 2, 0},
    {"first_pass_vars", &sc_ctx::first_pass_vars, 0, 4, 0},   // 0 auto; 4: the matrix-core pass at any size
    {"grid_pass", &sc_ctx::grid_pass, 0, 1, kOptBool},
    {"grid_log", &sc_ctx::grid_log, 0, 26, 0},
    {"grid_max_vars", &sc_ctx::grid_max_vars, 1, sc::kGridMaxVars, 0},
    {"grid_sharded", &sc_ctx::grid_sharded, 0, 1, kOptBool},
    {"grid_blocks", &sc_ctx::grid_blocks, 0, kWgMaxBlocks, 0},
    {"fold_dma", &sc_ctx::fold_dma, 0, 1, kOptBool},
    {"pipe32", &sc_ctx::pipe32, 0, 1, kOptBool},
    {"pipe32_log", &sc_ctx::pipe32_log, 11, 40, 0},
    {"gram_log", &sc_ctx::gram_log, 14, 40, kOptOff},
    {"wfold_log", &sc_ctx::wfold_log, 12, 40, kOptOff},
    {"wfold_min_log", &sc_ctx::wfold_min_log, 12, 40, 0},
    {"wfold5_min_log", &sc_ctx::wfold5_min_log, 12, 40, 0},
    {"wfold_always", &sc_ctx::wfold_always, 0, 1, kOptBool},
    {"wfold_slot_period", &sc_ctx::wfold_slot_period, -1, 1 << 24, 0},   // ticks of 10 ns; 0: no slots; -1: by table size (launch_wfold_pass)
    {"wfold_slot_width", &sc_ctx::wfold_slot_width, 0, 1 << 24, 0},
    {"wfold_slot_stagger", &sc_ctx::wfold_slot_stagger, 0, 1, kOptBool},
    {"matmul_path", &sc_ctx::matmul_path, 0, 2, 0},   // 0 auto, 1 int8 matrix cores, 2 VALU
    {"host_tail_log", &sc_ctx::host_tail_log, 0, kTailLogMax, 0},
    {"gp_host_log", &sc_ctx::gp_host_log, 0, sc::kGpHostLogMax, 0},
    {"gp_tree_lv", &sc_ctx::gp_tree_lv, 1, 3, 0},
    {"fr_host_log", &sc_ctx::fr_host_log, 0, sc::kFrHostLogMax, 0},
    {"fr_tree_lv", &sc_ctx::fr_tree_lv, 1, sc::kFrTreeLvMax, 0},
    {"tail_log", &sc_ctx::tail_log, 0, 40, 0},
    {"max_blocks", &sc_ctx::max_blocks, 1, INT64_MAX, 0},   // (1..partial_rows: sc_ctx_set_option)
    {"time_kernels", &sc_ctx::time_kernels, 0, 1, kOptBool},   // recorded pairs stay in the ring until it fills or the totals are read
    {"use_mailbox", &sc_ctx::use_mailbox, 0, 1, kOptBool},
    {"nt_load_log", &sc_ctx::nt_load_log, INT64_MIN, INT64_MAX, 0},
    {"nt_store_log", &sc_ctx::nt_store_log, INT64_MIN, INT64_MAX, 0},
    {"pool_contiguous", &sc_ctx::pool_contiguous, 0, 1, kOptBool},
    {"dbg_fold_grab", &sc_ctx::dbg_fold_grab, 0, 16, 0},
    {"rccl_timeout_ms", &sc_ctx::rccl_timeout_ms, 1, 3600000, 0},
    {"arena_log", &sc_ctx::arena_log, 4, 26, kOptPeer},   // (only before sc_ctx_comm_peer_export: sc_ctx_set_option)
    {"peer_spin_ms", &sc_ctx::peer_spin_ms, 1, 600000, kOptPeer},
    {"peer_connect_ms", &sc_ctx::peer_connect_ms, 1, 3600000, kOptPeer},
    {"dbg_delay_ms", &sc_ctx::dbg_delay_ms, 0, 10000, kOptPeer},
    {"dbg_skip_tag", &sc_ctx::dbg_skip_tag, 0, 1, kOptBool | kOptPeer},
};
static const OptionSpec* find_option(const char* key) {
  for (const OptionSpec& o : kOptions)
    if (strcmp(o.name, key) == 0) return &o;
  return nullptr;
}

extern "C" int sc_ctx_set_option(sc_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return SC_ERR_ARG;
  const std::string k(key);
  if (k == "prewarm") return value < 0 ? fail(ctx, SC_ERR_ARG, "prewarm: num_vars must be >= 0") : prewarm(ctx, (size_t)value);   // an action, not a setting
  if (is_multi(ctx)) SC_TRY(multi_set_option(ctx, key, value));   // every shard first (they validate); then the handle's own copy
  if (k == "stat_reset") {
    ctx->stat_wait_ns = ctx->stat_launch_ns = 0;
    ctx->pool_peak_words = ctx->pool_live_words;
    return SC_OK;
  }
  const OptionSpec* o = find_option(key);
  if (!o) return fail(ctx, SC_ERR_ARG, "unknown option '%s'", key);
  if (o->member == &sc_ctx::max_blocks && (value < 1 || value > (int64_t)ctx->partial_rows))
    return fail(ctx, SC_ERR_ARG, "max_blocks must be 1..%zu", ctx->partial_rows);
  if (!(o->flags & kOptBool) && (value < o->lo || value > o->hi) && !((o->flags & kOptOff) && value == 0))
    return fail(ctx, SC_ERR_ARG, "%s must be %s%lld..%lld", key, (o->flags & kOptOff) ? "0 (never) or " : "", (long long)o->lo, (long long)o->hi);
  if (o->member == &sc_ctx::arena_log && ctx->peer_region) return fail(ctx, SC_ERR_STATE, "arena_log must be set before sc_ctx_comm_peer_export");
  ctx->*o->member = (o->flags & kOptBool) ? (value ? 1 : 0) : (int)value;
  return SC_OK;
}

// a pool statistic of one context, or its sum over the shards of a multi-device handle
static int64_t pool_stat(const sc_ctx* ctx, size_t (*of)(const sc_ctx*)) {
  if (!is_multi(ctx)) return (int64_t)of(ctx);
  int64_t sum = 0;
  for (const sc_ctx* sub : ctx->subs) sum += (int64_t)of(sub);
  return sum;
}

extern "C" int sc_ctx_get_option(const sc_ctx* ctx, const char* key, int64_t* value) {
  if (!ctx || !key || !value) return SC_ERR_ARG;
  const std::string k(key);
  if (k == "stat_wait_ns") *value = (int64_t)(is_multi(ctx) ? ctx->subs[0]->stat_wait_ns : ctx->stat_wait_ns);
  else if (k == "stat_launch_ns") *value = (int64_t)(is_multi(ctx) ? ctx->subs[0]->stat_launch_ns : ctx->stat_launch_ns);
  else if (k == "stat_pool_live_blocks") *value = pool_stat(ctx, [](const sc_ctx* c) { return c->pool_live.size(); });
  else if (k == "stat_pool_live_words") *value = pool_stat(ctx, [](const sc_ctx* c) { return c->pool_live_words; });
  else if (k == "stat_pool_peak_words") *value = pool_stat(ctx, [](const sc_ctx* c) { return c->pool_peak_words; });
  else if (k == "transport") *value = (int64_t)ctx->transport;   // 0 none, 1 RCCL, 2 host callbacks, 3 peer, 4 local (a multi-device handle and its shards)
  else if (k == "n_devices") *value = is_multi(ctx) ? (int64_t)ctx->subs.size() : 1;
  else if (k == "comm_nranks") {
    // how many ranks the data plane really spans: RCCL's own count (ncclCommCount) when it is the transport
    int n = ctx->world;
    if (ctx->transport == Transport::kRccl) {
      n = 0;
      if (!g_rccl.CommCount || !ctx->comm || g_rccl.CommCount(ctx->comm, &n) != ncclSuccess)
        return fail(ctx, SC_ERR_RCCL, "ncclCommCount failed");
    }
    *value = n;
  } else if (const OptionSpec* o = find_option(key)) {
    *value = ctx->*o->member;
  } else {
    return fail(ctx, SC_ERR_ARG, "unknown option '%s'", key);
  }
  return SC_OK;
}

extern "C" int sc_ctx_synchronize(sc_ctx* ctx) {
  if (!ctx) return SC_ERR_ARG;
  if (is_multi(ctx)) return multi_synchronize(ctx);
  SC_TRY(set_device(ctx));
  SC_HIP(ctx, sync_stream(ctx));
  return SC_OK;
}

// (a multi-device handle: the stream of its first shard)
extern "C" void* sc_ctx_stream(const sc_ctx* ctx) { return !ctx ? nullptr : (void*)(is_multi(ctx) ? ctx->subs[0]->stream : ctx->stream); }

extern "C" int sc_ctx_kernel_time(sc_ctx* ctx, double out[2], int reset) {
  if (!ctx || !out) return SC_ERR_ARG;
  if (is_multi(ctx)) {   // a multi-device handle reports its first shard: one GPU's launches over its own shard
    for (size_t d = 1; d < ctx->subs.size(); ++d) {
      double drop[2];
      (void)sc_ctx_kernel_time(ctx->subs[d], drop, reset);
    }
    return sc_ctx_kernel_time(ctx->subs[0], out, reset);
  }
  SC_TRY(set_device(ctx));
  drain_kernel_timers(ctx);
  out[0] = (double)ctx->kt_n;
  out[1] = ctx->kt_ms;
  if (reset) {
    ctx->kt_n = 0;
    ctx->kt_ms = 0.0;
  }
  return SC_OK;
}

extern "C" int sc_ctx_launch_log(sc_ctx* ctx, sc_launch_record* out, size_t cap, size_t* n_out, int reset) {
  if (!ctx || !n_out || (cap && !out)) return SC_ERR_ARG;
  if (is_multi(ctx)) {
    for (size_t d = 1; d < ctx->subs.size(); ++d) {
      size_t drop = 0;
      (void)sc_ctx_launch_log(ctx->subs[d], nullptr, 0, &drop, reset);
    }
    return sc_ctx_launch_log(ctx->subs[0], out, cap, n_out, reset);
  }
  SC_TRY(set_device(ctx));
  drain_kernel_timers(ctx);
  const size_t n = std::min(cap, ctx->launch_log.size());
  for (size_t i = 0; i < n; ++i) out[i] = ctx->launch_log[i];
  *n_out = ctx->launch_log.size();
  if (reset) ctx->launch_log.clear();
  return SC_OK;
}
