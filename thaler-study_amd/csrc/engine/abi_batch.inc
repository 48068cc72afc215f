// Part of sumcheck_hip.hip (included there, in order): C ABI: sc_prove_batch - a batch of independent product sumchecks of the
// same size, one launch per pass for the whole batch (kernels/batch.hpp).

// =====================================================================================
// C ABI: sc_prove_batch
// =====================================================================================
//
// Every instance keeps the schedule, the host work and the transcript of its own sc_prove: the batch runs the planner of one
// proof at that size (plan_pass, as sc_plan_proof shows it) and replaces each of its launches by ONE batch_pass_kernel launch
// over all instances with the same (kf, ks).  Each instance is an sc_prover that never launches anything itself: the batched
// launch fills its cells (S), and from there the single-proof code answers its rounds (prover_answer), hands over to the host
// (host_fold) and finishes there (host_round).

namespace {

constexpr int kBatchMaxLog = 20;       // the batched kernel serves 1 <= n <= this: larger proofs go one after another
constexpr size_t kBatchMaxCount = 1024;   // instances of one call at most

// The schedule of one proof at n on this context, checked for what the batched kernel can do: passes of kf <= 5 / ks <= 5 on
// whole tables, at most one hand-over to the host.  *tail_log = log2 entries per table handed to the host (-1: none).
bool batch_plan_ok(const sc_ctx* ctx, int n, int* tail_log) {
  const PlanOpts o = plan_opts_of(ctx, true);
  int cur_log = n, kf = 0;
  bool on_host = false;
  *tail_log = -1;
  for (size_t j = 0; j < (size_t)n;) {
    const PassPlan p = plan_pass(o, (size_t)n, j, kf, cur_log, false, on_host);
    if (p.error || p.gather_first || p.kind == PassPlan::kRankPass) return false;
    if (p.kind == PassPlan::kHostTail) return true;
    if (kf > sc::kGridMaxVars || p.ks < 1 || p.ks > sc::kGridMaxVars || cur_log < kf + p.ks) return false;
    cur_log -= kf;
    if (p.to_host) *tail_log = cur_log;
    on_host = p.to_host;
    kf = p.ks;
    j += (size_t)p.ks;
  }
  return true;
}

// the context's pinned batch memory for `count` instances: descriptors, and cells + handed-over tables
int batch_reserve(sc_ctx* ctx, size_t count, int tail_log) {
  const size_t desc_bytes = count * sizeof(sc::BatchDesc);
  if (desc_bytes > ctx->batch_desc_bytes) {
    if (ctx->h_batch_desc) (void)hipHostFree(ctx->h_batch_desc);
    ctx->h_batch_desc = nullptr;
    ctx->batch_desc_bytes = 0;
    SC_HIP(ctx, hipHostMalloc(&ctx->h_batch_desc, desc_bytes, hipHostMallocDefault));
    ctx->batch_desc_bytes = desc_bytes;
  }
  const size_t words = count * ((size_t)sc::kGridMaxCells + (tail_log >= 0 ? (size_t)2 << tail_log : 0));
  if (words > ctx->batch_words) {
    if (ctx->h_batch) (void)hipHostFree(ctx->h_batch);
    ctx->h_batch = ctx->d_batch = nullptr;
    ctx->batch_words = 0;
    SC_HIP(ctx, hipHostMalloc(&ctx->h_batch, words * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
    SC_HIP(ctx, hipHostGetDevicePointer((void**)&ctx->d_batch, ctx->h_batch, 0));
    ctx->batch_words = words;
  }
  return SC_OK;
}

// blocks per instance: the resident grid shared among the instances, at least one, at most what the instance has rows for
int batch_blocks_per_instance(sc_ctx* ctx, size_t count, size_t n_out) {
  const int resident = resident_grid(ctx, ctx->gold ? kernel_ptr(&sc::batch_pass_kernel<sc::GoldilocksMont, 5, false>)
                                                    : kernel_ptr(&sc::batch_pass_kernel<sc::MontGeneric, 5, false>),
                                     sc::kBlock, 2 * ctx->num_cus);
  constexpr size_t kWaves = sc::kBlock / sc::kWave;
  const size_t n_iter = (n_out + sc::kWgEntries - 1) / sc::kWgEntries;
  const size_t share = ((size_t)resident + count - 1) / count;
  return (int)std::max<size_t>(1, std::min({share, (n_iter + kWaves - 1) / kWaves, (size_t)sc::kBatchMaxBlocks}));
}

// The device buffers of one call: descriptors, partial rows, tickets (zeroed once; every launch leaves them at zero).
// (Declared in the reverse of the order they go back in.)
struct BatchBufs {
  PoolBuf tickets, partials, desc;
  PoolBuf folded;   // the instances' current folded tables, [instance][table][2^cur_log] (null: the caller's tables)
};

// One pass over every instance: fold its kf pending challenges of tables of 2^log_in entries, the 3^ks cells of the next ks
// rounds into its S.  to_host: the folded tables go to the pinned batch memory (after the cells), the host finishes from them.
int batch_pass(sc_ctx* ctx, std::vector<sc_prover>& pr, BatchBufs& bb, int kf, int ks, int log_in, bool to_host, size_t j) {
  const size_t count = pr.size(), n_out = (size_t)1 << (log_in - kf);
  PoolBuf folded;
  u64* out_base = nullptr;
  if (kf > 0) {
    if (to_host) {
      out_base = ctx->d_batch + count * sc::kGridMaxCells;
    } else {
      SC_TRY(folded.alloc(ctx, count * 2 * n_out));
      out_base = folded;
    }
  }
  sc::BatchDesc* hd = static_cast<sc::BatchDesc*>(ctx->h_batch_desc);
  for (size_t i = 0; i < count; ++i) {
    sc::BatchDesc& d = hd[i];
    d.a = pr[i].sh[0].cur_a;
    d.b = pr[i].sh[0].cur_b;
    d.a2 = out_base ? out_base + i * 2 * n_out : nullptr;
    d.b2 = out_base ? d.a2 + n_out : nullptr;
    d.gw = make_weights<sc::GridW>(ctx, pr[i].pending.data(), kf);
  }
  const int bpi = batch_blocks_per_instance(ctx, count, n_out);
  constexpr size_t kWaves = sc::kBlock / sc::kWave;
  const size_t n_iter = (n_out + sc::kWgEntries - 1) / sc::kWgEntries;
  const bool pf = (kf == 0 || kf == 2) && n_iter > (size_t)bpi * kWaves;   // (launch_grid_pass's rule)
  sc::BatchOut bo;
  bo.partials = bb.partials;
  bo.tickets = reinterpret_cast<unsigned*>(bb.tickets.get());
  bo.cells = ctx->d_batch;
  bo.mailbox = ctx->d_mailbox;
  bo.seq = ctx->mailbox_seq + 1;
  bo.host_out = to_host ? 1 : 0;
  const sc::BatchDesc* dd = reinterpret_cast<const sc::BatchDesc*>(bb.desc.get());
  if (hipMemcpyAsync(bb.desc, hd, count * sizeof(sc::BatchDesc), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return fail(ctx, SC_ERR_HIP, "sc_prove_batch: descriptor copy failed");
  // the launch log: log_in and kf / ks as a grid pass's; the batch size is bytes_read / (16 * 2^log_in)
  SC_TRY(timer_begin(ctx, SC_KIND_BATCH_PASS, kf, ks, log_in, (u64)count * (16ull << log_in), kf > 0 ? (u64)count * (16ull << (log_in - kf)) : 0));
  {
    const dim3 grid((unsigned)bpi, (unsigned)count);
    SC_DISPATCH_FIELD(ctx, F, f, with_bool(pf, [&](auto PF) {
      with_const<1, 2, 3, 4, 5>(ks, [&](auto KS) {
        hipLaunchKernelGGL((sc::batch_pass_kernel<F, KS, PF>), grid, dim3(sc::kBlock), 0, ctx->stream, f, dd, kf, n_out, bo);
      });
    }));
    if (hipGetLastError() != hipSuccess) {
      poison(ctx);
      return fail(ctx, SC_ERR_HIP, "batch_pass_kernel launch failed");
    }
  }
  SC_TRY(timer_end(ctx));
  ctx->mailbox_seq += 1;
  SC_TRY(wait_mailbox(ctx, ctx->mailbox_seq));
  const int cells = pow3(ks);
  for (size_t i = 0; i < count; ++i) {
    sc_prover& p = pr[i];
    memcpy(p.S, ctx->h_batch + i * sc::kGridMaxCells, (size_t)cells * sizeof(u64));
    if (kf > 0) {
      p.sh[0].cur_a = out_base + i * 2 * n_out;
      p.sh[0].cur_b = p.sh[0].cur_a + n_out;
      p.cur_log = log_in - kf;
      p.pending.clear();
    }
    p.on_host = to_host;
    p.cache_ks = ks;
    p.cache_round = j;
    p.g_known = -1;
  }
  if (kf > 0) bb.folded = std::move(folded);   // the tables of the pass before are read: their block goes back (stream-ordered reuse)
  return SC_OK;
}

// every instance's rounds, on a context of one device and one rank, 1 <= n <= kBatchMaxLog
int prove_batch_impl(sc_ctx* ctx, size_t count, const sc_table* const* a, const sc_table* const* b, int n, int tail_log,
                     sc_draw_batch_fn draw, void* user, const uint64_t* seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges) {
  std::vector<sc_prover> pr;
  try {
    pr.resize(count);
    for (size_t i = 0; i < count; ++i) {
      sc_prover& p = pr[i];
      p.ctx = ctx;
      p.sh.resize(1);
      p.sh[0].ctx = ctx;
      p.sh[0].cur_a = a[i]->d;
      p.sh[0].cur_b = b[i]->d;
      p.cur_log = n;
      p.num_vars = (size_t)n;
      p.pending.reserve(sc::kGridMaxVars + 1);
      if (tail_log >= 0) {
        p.ha.reserve((size_t)1 << tail_log);
        p.hb.reserve((size_t)1 << tail_log);
      }
    }
  } catch (const std::bad_alloc&) {
    return fail(ctx, SC_ERR_OOM, "sc_prove_batch: no host memory for %zu instances", count);
  }
  SC_TRY(batch_reserve(ctx, count, tail_log));
  BatchBufs bb;
  const size_t rows = count * (size_t)batch_blocks_per_instance(ctx, count, (size_t)1 << n);   // (the most: the first pass's)
  int rc = bb.desc.alloc(ctx, (count * sizeof(sc::BatchDesc) + 7) / 8);
  if (rc == SC_OK) rc = bb.partials.alloc(ctx, rows * sc::kGridChunk);
  if (rc == SC_OK) rc = bb.tickets.alloc(ctx, (count + 1 + 1) / 2);
  if (rc == SC_OK && hipMemsetAsync(bb.tickets, 0, (count + 1) * sizeof(unsigned), ctx->stream) != hipSuccess)
    rc = fail(ctx, SC_ERR_HIP, "sc_prove_batch: memset failed");
  const PlanOpts o = plan_opts_of(ctx, true);
  HostField hf(ctx->fp);
  int kf = 0, cur_log = n;
  bool on_host = false, host_mode = false;
  size_t pass_end = 0;   // rounds below this are answered from the cells of the last pass
  for (size_t j = 0; j < (size_t)n && rc == SC_OK; ++j) {
    if (!host_mode && j == pass_end) {
      const PassPlan p = plan_pass(o, (size_t)n, j, kf, cur_log, false, on_host);
      if (p.kind == PassPlan::kHostTail) {   // the pass before wrote every instance's tables after the cells
        const u64* h = ctx->h_batch + count * sc::kGridMaxCells;
        const size_t in_len = (size_t)1 << cur_log, out_len = in_len >> kf;
        for (size_t i = 0; i < count; ++i) {
          sc_prover& q = pr[i];
          const sc::GridW gw = make_weights<sc::GridW>(ctx, q.pending.data(), kf);
          q.ha.resize(out_len);
          q.hb.resize(out_len);
          host_fold(hf.f, gw, kf, h + i * 2 * in_len, q.ha.data(), out_len);
          host_fold(hf.f, gw, kf, h + i * 2 * in_len + in_len, q.hb.data(), out_len);
          enter_host_mode(&q);
        }
        host_mode = true;
      } else {
        rc = batch_pass(ctx, pr, bb, kf, p.ks, cur_log, p.to_host, j);
        if (rc != SC_OK) break;
        cur_log -= kf;
        on_host = p.to_host;
        kf = p.ks;
        pass_end = j + (size_t)p.ks;
      }
    }
    for (size_t i = 0; i < count; ++i) {
      sc_prover& q = pr[i];
      u64 e[3];
      if (host_mode) host_round(&q, e);
      else prover_answer(&q, j, e);
      if (j == 0) c1[i] = hf.add(e[0], e[1]);
      if (evals) memcpy(evals + 3 * (i * (size_t)n + j), e, sizeof(e));
      const u64 r = draw ? draw(user, i, j, e) : seeded_challenge(ctx, hf, seed_r[i], j);
      if (r >= ctx->fp.p) {
        rc = fail(ctx, SC_ERR_ARG, "sc_prove_batch: draw() returned an unreduced challenge (instance %zu, round %zu)", i, j);
        break;
      }
      if (challenges) challenges[i * (size_t)n + j] = r;
      q.pending.push_back(r);
    }
  }
  return rc;
}

struct BatchDraw {   // one instance's draw behind sc_prove's callback (the proofs that go one after another)
  sc_draw_batch_fn draw;
  void* user;
  size_t instance;
};
uint64_t batch_draw_one(void* u, size_t round, const uint64_t evals[3]) {
  const BatchDraw* d = static_cast<const BatchDraw*>(u);
  return d->draw(d->user, d->instance, round, evals);
}

}  // namespace

extern "C" int sc_prove_batch(sc_ctx* ctx, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_batch_fn draw,
                              void* user, const uint64_t* seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges) {
  if (!ctx) return SC_ERR_ARG;
  if (count == 0 || !a || !b || !seed_r || !c1) return fail(ctx, SC_ERR_ARG, "sc_prove_batch: no instances, or a NULL array");
  if (is_multi(ctx) || is_sharded(ctx) || ctx->world > 1)
    return fail(ctx, SC_ERR_UNSUPPORTED, "sc_prove_batch: batches run on a context of one device and one rank (this one is %s)",
                is_multi(ctx) ? "a multi-device handle" : "sharded");
  if (count > kBatchMaxCount) return fail(ctx, SC_ERR_ARG, "sc_prove_batch: %zu instances (at most %zu per call)", count, kBatchMaxCount);
  for (size_t i = 0; i < count; ++i) {
    SC_TRY(check_pair(ctx, a[i], b[i], "sc_prove_batch"));
    if (a[i]->len != a[0]->len)
      return fail(ctx, SC_ERR_ARG, "sc_prove_batch: instance %zu has 2^%d entries, instance 0 2^%d", i, log2_of(a[i]->len), log2_of(a[0]->len));
  }
  SC_TRY(set_device(ctx));
  const int n = log2_of(a[0]->len);
  int tail_log = -1;
  if (n >= 1 && n <= kBatchMaxLog && ctx->use_mailbox && batch_plan_ok(ctx, n, &tail_log))
    return prove_batch_impl(ctx, count, a, b, n, tail_log, draw, user, seed_r, c1, evals, challenges);
  // n = 0, n > kBatchMaxLog, or options without a batched schedule: the instances one after another, each its own sc_prove
  for (size_t i = 0; i < count; ++i) {
    BatchDraw bd{draw, user, i};
    SC_TRY(sc_prove(ctx, a[i], b[i], draw ? batch_draw_one : nullptr, &bd, seed_r[i], c1 + i, evals ? evals + 3 * (size_t)n * i : nullptr,
                    challenges ? challenges + (size_t)n * i : nullptr));
  }
  return SC_OK;
}
