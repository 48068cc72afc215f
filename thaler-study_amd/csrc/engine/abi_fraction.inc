// Part of sumcheck_hip.hip (included there, in order): LogUp lookups (kernels/fraction.hpp states the protocol): the fraction-sum
// trees of two tables, the layered cubic sumcheck over them with a host finish, and the multiplicities of a lookup.

struct sc_frac {
  sc_ctx* ctx = nullptr;
  int n = 0;
  const sc_table* p = nullptr;   // layer n of the numerators, or null: all ones.  Borrowed until sc_frac_destroy, never written
  const sc_table* q = nullptr;   // layer n of the denominators: borrowed, never written
  PoolBuf tree[2];               // p's and q's heap: layer k at words [2^k, 2^(k+1)), k < n
  u64 root[2] = {0, 0};          // (P, Q)
};

namespace {

int check_frac(sc_ctx* ctx, const sc_frac* g, const char* what) {
  if (!g || g->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: not a fraction tree of this context", what);
  return SC_OK;
}

// layer k of p (which = 0) or q (1), 0 <= k <= n; null for layer n of an all-ones p
const u64* fr_layer_ptr(const sc_frac* g, int which, int k) {
  if (k < g->n) return g->tree[which].get() + ((size_t)1 << k);
  const sc_table* t = which ? g->q : g->p;
  return t ? t->d : nullptr;
}

// the launches of the trees (tree_schedule): fr_tree_kernel from layer m over lv layers, fr_tree_tail_kernel below layer kFrTailLog
int fr_build_trees(sc_ctx* ctx, sc_frac* g, int tree_lv) {
  u64* const pt = g->tree[0].get();
  u64* const qt = g->tree[1].get();
  return tree_schedule(g->n, sc::kFrTailLog, tree_lv, [&](int m, int lv) {
    const u64* ps = fr_layer_ptr(g, 0, m);
    const u64* qs = fr_layer_ptr(g, 1, m);
    const bool ones = !ps;
    const u64 read = (u64)(ones ? 8 : 16) << m;
    if (lv == 0)
      return launch_recorded(ctx, {SC_KIND_FRACTION_TREE, 0, ones ? 1 : 2, m, read, ((u64)16 << m) - 16}, "fr_tree_tail_kernel", [&] {
        SC_DISPATCH_FIELD(ctx, F, f, with_bool(ones, [&](auto ONES) {
          hipLaunchKernelGGL((sc::fr_tree_tail_kernel<F, ONES>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, f, ps, qs, pt, qt, m);
        }));
      });
    const int log_low = m - lv;
    const size_t n_units = (size_t)1 << (log_low - 1);
    const int grid = grid_for(ctx, n_units);
    return launch_recorded(ctx, {SC_KIND_FRACTION_TREE, lv, ones ? 1 : 2, m, read, ((u64)16 << m) - ((u64)16 << log_low)}, "fr_tree_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3>(lv, [&](auto LV) {
        with_bool(ones, [&](auto ONES) {
          hipLaunchKernelGGL((sc::fr_tree_kernel<F, LV, ONES>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, ps, qs, pt, qt, log_low, n_units);
        });
      }));
    });
  });
}

}  // namespace

extern "C" int sc_frac_create(sc_ctx* ctx, const sc_table* p, const sc_table* q, sc_frac** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_frac_create"));
  SC_TRY(require_cubic_field(ctx, "sc_frac_create"));
  if (!q || !out) return fail(ctx, SC_ERR_ARG, "sc_frac_create: a NULL argument");
  SC_TRY(check_table(ctx, q, "sc_frac_create"));
  if (p) SC_TRY(check_table(ctx, p, "sc_frac_create"));
  if (q->len < 2 || q->len > ((size_t)1 << sc::kFrMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_frac_create: tables of %zu entries (at least two, at most 2^%d)", q->len, sc::kFrMaxLog);
  if (p && p->len != q->len) return fail(ctx, SC_ERR_ARG, "sc_frac_create: p has %zu entries, q has %zu", p->len, q->len);
  SC_TRY(set_device(ctx));
  std::unique_ptr<sc_frac> g(new (std::nothrow) sc_frac);
  if (!g) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  g->ctx = ctx;
  g->n = log2_of(q->len);
  g->p = p;
  g->q = q;
  SC_TRY(g->tree[0].alloc(ctx, q->len));
  SC_TRY(g->tree[1].alloc(ctx, q->len));
  SC_TRY(fr_build_trees(ctx, g.get(), ctx->fr_tree_lv));
  SC_HIP(ctx, hipMemcpyAsync(&g->root[0], g->tree[0].get() + 1, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(&g->root[1], g->tree[1].get() + 1, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  *out = g.release();
  return SC_OK;
}

extern "C" int sc_frac_destroy(sc_ctx* ctx, sc_frac* g) {
  if (!g) return SC_OK;
  if (!ctx || g->ctx != ctx) return SC_ERR_ARG;
  delete g;   // (the trees go back to the pool)
  return SC_OK;
}

extern "C" int sc_frac_root(const sc_frac* g, uint64_t out[2]) {
  if (!g || !out) return SC_ERR_ARG;
  out[0] = g->root[0];
  out[1] = g->root[1];
  return SC_OK;
}

extern "C" int sc_frac_layer(sc_ctx* ctx, const sc_frac* g, size_t k, int which, sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_frac_layer"));
  if (!out) return fail(ctx, SC_ERR_ARG, "sc_frac_layer: a NULL argument");
  SC_TRY(check_frac(ctx, g, "sc_frac_layer"));
  if (k >= (size_t)g->n) return fail(ctx, SC_ERR_ARG, "sc_frac_layer: layer %zu of trees with layers 0 .. %d", k, g->n - 1);
  if (which != 0 && which != 1) return fail(ctx, SC_ERR_ARG, "sc_frac_layer: which = %d (0: p, 1: q)", which);
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, (size_t)1 << k));
  const hipError_t e = hipMemcpyAsync(t->d, fr_layer_ptr(g, which, (int)k), sizeof(u64) << k, hipMemcpyDeviceToDevice, ctx->stream);
  return table_done(ctx, t, e, "sc_frac_layer", out);
}

extern "C" int sc_frac_prove(sc_ctx* ctx, const sc_frac* g, sc_draw_frac_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                             uint64_t* challenges, uint64_t* point, uint64_t claims[2]) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_frac_prove"));
  SC_TRY(require_cubic_field(ctx, "sc_frac_prove"));
  if (!finals || !point || !claims) return fail(ctx, SC_ERR_ARG, "sc_frac_prove: a NULL argument");
  SC_TRY(check_frac(ctx, g, "sc_frac_prove"));
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  const sc::MontGeneric& hfield = hf.f;
  const int n = g->n, T = ctx->fr_host_log;
  const bool ones = !g->p;
  // the bottom of both trees on the host, once per proof: the layers 0 .. min(T + 1, n) in the heap layout (layer k <= T reads
  // layer k + 1; layer n is the caller's tables, or ones)
  const int top = std::min(T + 1, n);
  std::vector<u64> bottom[2];
  for (int w = 0; w < 2; ++w) {
    bottom[w].resize((size_t)2 << top);
    const size_t tree_words = std::min((size_t)2 << top, (size_t)1 << n);
    SC_HIP(ctx, hipMemcpyAsync(bottom[w].data(), g->tree[w].get(), tree_words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    if (top == n) {
      const u64* src = fr_layer_ptr(g, w, n);
      if (src) SC_HIP(ctx, hipMemcpyAsync(bottom[w].data() + tree_words, src, sizeof(u64) << n, hipMemcpyDeviceToHost, ctx->stream));
      else std::fill(bottom[w].begin() + (ptrdiff_t)tree_words, bottom[w].end(), hfield.one());
    }
  }
  SC_HIP(ctx, sync_stream(ctx));
  const int resident = resident_blocks(ctx, &sc::fr_pass_kernel<sc::GoldilocksMont, true, false>, &sc::fr_pass_kernel<sc::MontGeneric, true, false>);

  // the challenger, in protocol order: per layer its lambda (k >= 1), one draw per round, and rho
  u64 n_draws = 0;
  int rc = SC_OK;
  auto challenge = [&](size_t layer, size_t round, const u64* msg, u64* out) {
    const u64 c = draw ? draw(user, layer, round, msg) : seeded_challenge(ctx, hf, seed_r, n_draws);
    if (c >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_frac_prove: draw() returned an unreduced challenge");
      return false;
    }
    if (challenges) challenges[n_draws] = c;
    n_draws += 1;
    *out = c;
    return true;
  };

  std::vector<u64> z((size_t)n), rs((size_t)n + 1), host[5];
  u64 lambda = 0, a_k = g->root[0], b_k = g->root[1];
  for (int k = 0; k < n; ++k) {
    const size_t len = (size_t)1 << k;
    const int nt = ones && k == n - 1 ? 3 : 5;   // the tables of this layer: E, QL, QR (, PL, PR)
    u64* const ev = evals ? evals + 2 * (size_t)k * (size_t)(k > 0 ? k - 1 : 0) : nullptr;   // 4 k (k - 1) / 2 words before layer k
    auto next = [&](size_t round, const u64* msg, u64* out) {
      if (ev) memcpy(ev + 4 * round, msg, 4 * sizeof(u64));
      return challenge((size_t)k, round, msg, out);
    };
    u64* tb[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (k <= T) {
      // the whole layer on the host
      host[sc::kFrE].resize(len);
      sc::gp_host_eq(hfield, z.data(), k, host[sc::kFrE].data());
      const u64* pk = bottom[0].data() + 2 * len;
      const u64* qk = bottom[1].data() + 2 * len;
      host[sc::kFrQL].assign(qk, qk + len);
      host[sc::kFrQR].assign(qk + len, qk + 2 * len);
      if (nt == 5) {
        host[sc::kFrPL].assign(pk, pk + len);
        host[sc::kFrPR].assign(pk + len, pk + 2 * len);
      }
      for (int q = 0; q < nt; ++q) tb[q] = host[q].data();
      if (!sc::fr_host_rounds(hfield, tb, nt, lambda, k, 0, nullptr, rs.data(), next)) return rc;
    } else {
      // the device runs the rounds 0 .. k - te; the launch of round k - te leaves tables of 2^te entries, which the host takes
      const int te = std::max(T, 1);
      PoolBuf cur[5];
      SC_TRY(build_eq_table(ctx, z.data(), k, &cur[0]));
      const u64* pk = fr_layer_ptr(g, 0, k + 1);
      const u64* qk = fr_layer_ptr(g, 1, k + 1);
      const u64* in[5] = {cur[0].get(), qk, qk + len, nt == 5 ? pk : nullptr, nt == 5 ? pk + len : nullptr};
      u64 e[4];
      SC_TRY((device_rounds<5, 1, 2>(ctx, nt, k, te, in, cur, rs.data(), e, &rc, [&](const DeviceRound& d, Launched* l) {
        const bool fold = d.round > 0;
        sc::FrTables ft;
        for (int q = 0; q < 5; ++q) {
          ft.in[q] = q < nt ? d.in[q] : nullptr;
          ft.out[q] = d.out[q];
        }
        *l = {d.grid(resident), 4};
        SC_TRY(timer_begin(ctx, SC_KIND_FRACTION_PASS, fold ? 1 : 0, nt, d.log_in, (u64)(8 * nt) << d.log_in, fold ? (u64)(8 * nt) << (d.log_in - 1) : 0));
        SC_DISPATCH_FIELD(ctx, F, f, with_bool(fold, [&](auto FOLD) {
          with_bool(nt == 3, [&](auto ONES) {
            hipLaunchKernelGGL((sc::fr_pass_kernel<F, FOLD, ONES>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, ft, d.r_prev[0], lambda, d.n_units,
                               d.po);
          });
        }));
        return SC_OK;
      }, next)));
      const size_t left = (size_t)1 << te;
      for (int q = 0; q < nt; ++q) {
        host[q].resize(left);
        tb[q] = host[q].data();
        SC_HIP(ctx, hipMemcpyAsync(tb[q], in[q], left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      }
      SC_HIP(ctx, sync_stream(ctx));
      if (!sc::fr_host_rounds(hfield, tb, nt, lambda, te, (size_t)(k - te), e, rs.data(), next)) return rc;
    }
    const u64 one = hfield.one();
    const u64 fin[4] = {nt == 5 ? tb[sc::kFrPL][0] : one, nt == 5 ? tb[sc::kFrPR][0] : one, tb[sc::kFrQL][0], tb[sc::kFrQR][0]};   // pl, pr, ql, qr
    memcpy(finals + 4 * (size_t)k, fin, sizeof(fin));
    u64 rho = 0;
    if (!challenge((size_t)k, (size_t)k, fin, &rho)) return rc;
    rs[(size_t)k] = rho;
    a_k = hf.add(fin[0], hf.mul(rho, hf.sub(fin[1], fin[0])));
    b_k = hf.add(fin[2], hf.mul(rho, hf.sub(fin[3], fin[2])));
    std::copy(rs.begin(), rs.begin() + k + 1, z.begin());   // z_(k+1) = (r, rho_k)
    if (k + 1 < n && !challenge((size_t)k, (size_t)k + 1, nullptr, &lambda)) return rc;   // lambda of the next layer
  }
  memcpy(point, z.data(), (size_t)n * sizeof(u64));
  claims[0] = a_k;
  claims[1] = b_k;
  return SC_OK;
}

extern "C" int sc_lookup_count(sc_ctx* ctx, const sc_table* w, const sc_table* t, const uint32_t* idx_host, sc_table** mult, uint64_t* mismatches) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_lookup_count"));
  if (!w || !t || !idx_host || !mult || !mismatches) return fail(ctx, SC_ERR_ARG, "sc_lookup_count: a NULL argument");
  SC_TRY(check_table(ctx, w, "sc_lookup_count"));
  SC_TRY(check_table(ctx, t, "sc_lookup_count"));
  const size_t cap = (size_t)1 << sc::kFrMaxLog;
  if (w->len < 2 || w->len > cap || t->len < 2 || t->len > cap)
    return fail(ctx, SC_ERR_ARG, "sc_lookup_count: tables of %zu and %zu entries (at least two, at most 2^%d each)", w->len, t->len, sc::kFrMaxLog);
  const int n = log2_of(w->len), m = log2_of(t->len);
  if (ctx->fp.p <= ((u64)1 << std::max(n, m)))
    return fail(ctx, SC_ERR_UNSUPPORTED, "sc_lookup_count: p = %llu: a count of up to 2^%d must be a field word", (unsigned long long)ctx->fp.p, std::max(n, m));
  SC_TRY(set_device(ctx));
  // one block: the u32 counters, then the mismatch counter (its own word), then the indices
  const size_t count_words = std::max<size_t>(1, t->len / 2), idx_words = w->len / 2;
  PoolBuf work;
  SC_TRY(work.alloc(ctx, count_words + 1 + idx_words));
  u32* const counts = reinterpret_cast<u32*>(work.get());
  u32* const bad = reinterpret_cast<u32*>(work.get() + count_words);
  u32* const idx = reinterpret_cast<u32*>(work.get() + count_words + 1);
  SC_HIP(ctx, hipMemsetAsync(work.get(), 0, (count_words + 1) * sizeof(u64), ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(idx, idx_host, w->len * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
  TableBuf o;
  SC_TRY(o.alloc(ctx, t->len));
  const size_t n_pairs = w->len / 2;
  const bool lds = m <= sc::kLookupLdsLog;
  // LDS histograms: a block's flush costs up to 2^m global adds, so few blocks with long runs (two per CU at most)
  const unsigned grid = lds ? (unsigned)std::max<u64>(1, std::min<u64>((n_pairs + 8 * sc::kBlock - 1) / (8 * sc::kBlock), (u64)2 * ctx->num_cus))
                            : strided_grid(ctx, n_pairs);
  SC_TRY(launch_recorded(ctx, {SC_KIND_LOOKUP_COUNT, 0, lds ? 1 : 0, n, (u64)20 << n, (u64)4 << m}, "lookup_count_kernel", [&] {
    with_bool(lds, [&](auto LDS) {
      hipLaunchKernelGGL((sc::lookup_count_kernel<LDS>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, (const u64*)w->d, (const u64*)t->d, (const u32*)idx,
                         n_pairs, m, counts, bad);
    });
  }));
  SC_TRY(launch_recorded(ctx, {SC_KIND_LOOKUP_COUNT, 1, 0, m, (u64)4 << m, (u64)8 << m}, "lookup_mont_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::lookup_mont_kernel<F>), dim3(strided_grid(ctx, t->len)), dim3(sc::kBlock), 0, ctx->stream, f,
                                                    (const u32*)counts, t->len, o->d));
  }));
  u32 bad_host = 0;
  SC_HIP(ctx, hipMemcpyAsync(&bad_host, bad, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
  SC_TRY(table_done(ctx, o, hipGetLastError(), "sc_lookup_count", mult));
  *mismatches = bad_host;
  return SC_OK;
}
