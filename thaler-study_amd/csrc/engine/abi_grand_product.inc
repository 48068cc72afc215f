// Part of sumcheck_hip.hip (included there, in order): the grand product argument (kernels/grand_product.hpp states the
// protocol): the product tree of a table, the layered cubic sumcheck over it with a host finish, and the affine map of a table.

struct sc_gp {
  sc_ctx* ctx = nullptr;
  int n = 0;
  const sc_table* t = nullptr;   // V_n: borrowed until sc_gp_destroy, never written
  PoolBuf tree;                  // heap layout: layer k at words [2^k, 2^(k+1)), k < n
  u64 product = 0;               // V_0[0]
};

namespace {

int check_gp(sc_ctx* ctx, const sc_gp* g, const char* what) {
  if (!g || g->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: not a product tree of this context", what);
  return SC_OK;
}

// layer k of the tree, 0 <= k <= n
const u64* gp_layer_ptr(const sc_gp* g, int k) { return k == g->n ? g->t->d : g->tree.get() + ((size_t)1 << k); }

// the launches of the tree (tree_schedule): gp_tree_kernel from layer m over lv layers, gp_tree_tail_kernel below layer kGpTailLog
int gp_build_tree(sc_ctx* ctx, sc_gp* g, int tree_lv) {
  u64* const tree = g->tree.get();
  return tree_schedule(g->n, sc::kGpTailLog, tree_lv, [&](int m, int lv) {
    const u64* src = gp_layer_ptr(g, m);
    if (lv == 0)
      return launch_recorded(ctx, {SC_KIND_PRODUCT_TREE, 0, 0, m, (u64)8 << m, ((u64)8 << m) - 8}, "gp_tree_tail_kernel", [&] {
        SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::gp_tree_tail_kernel<F>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, f, src, tree, m));
      });
    const int log_low = m - lv;
    const size_t n_units = (size_t)1 << (log_low - 1);
    const int grid = grid_for(ctx, n_units);
    return launch_recorded(ctx, {SC_KIND_PRODUCT_TREE, lv, 0, m, (u64)8 << m, ((u64)8 << m) - ((u64)8 << log_low)}, "gp_tree_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3>(lv, [&](auto LV) {
        hipLaunchKernelGGL((sc::gp_tree_kernel<F, LV>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, src, tree, log_low, n_units);
      }));
    });
  });
}

// The device rounds of a cubic sumcheck over three tables of 2^k entries (device_rounds with gp_pass_kernel, SC_KIND_PRODUCT_PASS,
// four values per round); in, cur, rs, e, stopped and next as there
template <class Next>
int gp_device_rounds(sc_ctx* ctx, int k, int te, int resident, const u64* (&in)[3], PoolBuf (&cur)[3], u64* rs, u64 (&e)[4], const int* stopped,
                     Next&& next) {
  return device_rounds<3, 1, 2>(ctx, 3, k, te, in, cur, rs, e, stopped, [&](const DeviceRound& d, Launched* l) {
    const bool fold = d.round > 0;
    sc::GpTables tb;
    for (int q = 0; q < 3; ++q) {
      tb.in[q] = d.in[q];
      tb.out[q] = d.out[q];
    }
    *l = {d.grid(resident), 4};
    SC_TRY(timer_begin(ctx, SC_KIND_PRODUCT_PASS, fold ? 1 : 0, 1, d.log_in, (u64)24 << d.log_in, fold ? (u64)24 << (d.log_in - 1) : 0));
    SC_DISPATCH_FIELD(ctx, F, f, with_bool(fold, [&](auto FOLD) {
      hipLaunchKernelGGL((sc::gp_pass_kernel<F, FOLD>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, d.r_prev[0], d.n_units, d.po);
    }));
    return SC_OK;
  }, next);
}

// how many blocks of gp_pass_kernel the device holds at once
int gp_pass_resident(sc_ctx* ctx) {
  return resident_blocks(ctx, &sc::gp_pass_kernel<sc::GoldilocksMont, true>, &sc::gp_pass_kernel<sc::MontGeneric, true>);
}

}  // namespace

extern "C" int sc_gp_create(sc_ctx* ctx, const sc_table* t, sc_gp** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_gp_create"));
  SC_TRY(require_cubic_field(ctx, "sc_gp_create"));
  if (!t || !out) return fail(ctx, SC_ERR_ARG, "sc_gp_create: a NULL argument");
  SC_TRY(check_table(ctx, t, "sc_gp_create"));
  if (t->len < 2 || t->len > ((size_t)1 << sc::kGpMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_gp_create: a table of %zu entries (at least two, at most 2^%d)", t->len, sc::kGpMaxLog);
  SC_TRY(set_device(ctx));
  std::unique_ptr<sc_gp> g(new (std::nothrow) sc_gp);
  if (!g) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  g->ctx = ctx;
  g->n = log2_of(t->len);
  g->t = t;
  SC_TRY(g->tree.alloc(ctx, t->len));
  SC_TRY(gp_build_tree(ctx, g.get(), ctx->gp_tree_lv));
  SC_HIP(ctx, hipMemcpyAsync(&g->product, g->tree.get() + 1, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  *out = g.release();
  return SC_OK;
}

extern "C" int sc_gp_destroy(sc_ctx* ctx, sc_gp* g) {
  if (!g) return SC_OK;
  if (!ctx || g->ctx != ctx) return SC_ERR_ARG;
  delete g;   // (the tree goes back to the pool)
  return SC_OK;
}

extern "C" int sc_gp_product(const sc_gp* g, uint64_t* out) {
  if (!g || !out) return SC_ERR_ARG;
  *out = g->product;
  return SC_OK;
}

extern "C" int sc_gp_layer(sc_ctx* ctx, const sc_gp* g, size_t k, sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_gp_layer"));
  if (!out) return fail(ctx, SC_ERR_ARG, "sc_gp_layer: a NULL argument");
  SC_TRY(check_gp(ctx, g, "sc_gp_layer"));
  if (k >= (size_t)g->n) return fail(ctx, SC_ERR_ARG, "sc_gp_layer: layer %zu of a tree with layers 0 .. %d", k, g->n - 1);
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, (size_t)1 << k));
  const hipError_t e = hipMemcpyAsync(t->d, gp_layer_ptr(g, (int)k), sizeof(u64) << k, hipMemcpyDeviceToDevice, ctx->stream);
  return table_done(ctx, t, e, "sc_gp_layer", out);
}

extern "C" int sc_gp_prove(sc_ctx* ctx, const sc_gp* g, sc_draw_gp_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                           uint64_t* challenges, uint64_t* point, uint64_t* claim) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_gp_prove"));
  SC_TRY(require_cubic_field(ctx, "sc_gp_prove"));
  if (!finals || !point || !claim) return fail(ctx, SC_ERR_ARG, "sc_gp_prove: a NULL argument");
  SC_TRY(check_gp(ctx, g, "sc_gp_prove"));
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  const sc::MontGeneric& hfield = hf.f;
  const int n = g->n, T = ctx->gp_host_log;
  // the bottom of the tree on the host, once per proof: the layers 0 .. min(T + 1, n) in the heap layout (layer k <= T reads
  // V_(k+1); V_n is the caller's table)
  const int top = std::min(T + 1, n);
  std::vector<u64> bottom((size_t)2 << top);
  {
    const size_t tree_words = std::min((size_t)2 << top, (size_t)1 << n);
    SC_HIP(ctx, hipMemcpyAsync(bottom.data(), g->tree.get(), tree_words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    if (top == n) SC_HIP(ctx, hipMemcpyAsync(bottom.data() + tree_words, g->t->d, sizeof(u64) << n, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, sync_stream(ctx));
  }
  const int resident = gp_pass_resident(ctx);

  // the challenger, in protocol order: one draw per round and one per rho
  u64 n_draws = 0;
  int rc = SC_OK;
  auto challenge = [&](size_t layer, size_t round, const u64* msg, u64* out) {
    const u64 c = draw ? draw(user, layer, round, msg) : seeded_challenge(ctx, hf, seed_r, n_draws);
    n_draws += 1;
    if (c >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_gp_prove: draw() returned an unreduced challenge");
      return false;
    }
    *out = c;
    return true;
  };

  std::vector<u64> z((size_t)n), rs((size_t)n + 1), he, hl, hr;
  u64 c_k = g->product;
  for (int k = 0; k < n; ++k) {
    const size_t len = (size_t)1 << k;
    u64* const ev = evals ? evals + 2 * (size_t)k * (size_t)(k > 0 ? k - 1 : 0) : nullptr;   // 4 k (k - 1) / 2 words before layer k
    auto next = [&](size_t round, const u64* msg, u64* out) {
      if (ev) memcpy(ev + 4 * round, msg, 4 * sizeof(u64));
      return challenge((size_t)k, round, msg, out);
    };
    if (k <= T) {
      // the whole layer on the host
      he.resize(len);
      sc::gp_host_eq(hfield, z.data(), k, he.data());
      const u64* lk = bottom.data() + 2 * len;
      hl.assign(lk, lk + len);
      hr.assign(lk + len, lk + 2 * len);
      if (!sc::gp_host_rounds(hfield, he.data(), hl.data(), hr.data(), k, 0, nullptr, rs.data(), next)) return rc;
    } else {
      // the device runs the rounds 0 .. k - te; the launch of round k - te leaves tables of 2^te entries, which the host takes
      const int te = std::max(T, 1);
      PoolBuf cur[3];
      SC_TRY(build_eq_table(ctx, z.data(), k, &cur[0]));
      const u64* lk = gp_layer_ptr(g, k + 1);
      const u64* in[3] = {cur[0].get(), lk, lk + len};
      u64 e[4];
      SC_TRY(gp_device_rounds(ctx, k, te, resident, in, cur, rs.data(), e, &rc, next));
      const size_t left = (size_t)1 << te;
      he.resize(left);
      hl.resize(left);
      hr.resize(left);
      u64* const host[3] = {he.data(), hl.data(), hr.data()};
      for (int q = 0; q < 3; ++q) SC_HIP(ctx, hipMemcpyAsync(host[q], in[q], left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      SC_HIP(ctx, sync_stream(ctx));
      if (!sc::gp_host_rounds(hfield, he.data(), hl.data(), hr.data(), te, (size_t)(k - te), e, rs.data(), next)) return rc;
    }
    const u64 fin[2] = {hl[0], hr[0]};
    finals[2 * (size_t)k] = fin[0];
    finals[2 * (size_t)k + 1] = fin[1];
    u64 rho = 0;
    if (!challenge((size_t)k, (size_t)k, fin, &rho)) return rc;
    rs[(size_t)k] = rho;
    if (challenges) memcpy(challenges + (size_t)k * ((size_t)k + 1) / 2, rs.data(), ((size_t)k + 1) * sizeof(u64));
    c_k = hf.add(fin[0], hf.mul(rho, hf.sub(fin[1], fin[0])));
    std::copy(rs.begin(), rs.begin() + k + 1, z.begin());   // z_(k+1) = (r, rho_k)
  }
  memcpy(point, z.data(), (size_t)n * sizeof(u64));
  *claim = c_k;
  return SC_OK;
}

extern "C" int sc_table_affine(sc_ctx* ctx, const sc_table* t, uint64_t alpha, uint64_t beta, sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_table_affine"));
  if (!t || !out) return fail(ctx, SC_ERR_ARG, "sc_table_affine: a NULL argument");
  SC_TRY(check_table(ctx, t, "sc_table_affine"));
  if (t->len < 2) return fail(ctx, SC_ERR_ARG, "sc_table_affine: a table of %zu entries (at least two)", t->len);
  if (alpha >= ctx->fp.p || beta >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_table_affine: alpha or beta is not a word below p");
  SC_TRY(set_device(ctx));
  TableBuf o;
  SC_TRY(o.alloc(ctx, t->len));
  const size_t n_pairs = t->len / 2;
  SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::table_affine_kernel<F>), dim3(strided_grid(ctx, n_pairs)), dim3(sc::kBlock), 0, ctx->stream, f,
                                                  (const u64*)t->d, alpha, beta, n_pairs, o->d));
  return table_done(ctx, o, hipGetLastError(), "sc_table_affine", out);
}
