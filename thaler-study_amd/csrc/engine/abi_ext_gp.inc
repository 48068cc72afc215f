// Part of sumcheck_hip.hip (included there, in order, after abi_ext.inc): the grand product argument over the quadratic extension
// K = F_p[X] / (X^2 - w) (kernels/ext_grand_product.hpp states the protocol): the product tree of the leaves beta + alpha t over K,
// the layered cubic sumcheck over it with every challenge in K, and its host finish.

struct sc_gp_ext {
  sc_ctx* ctx = nullptr;
  int n = 0;
  const sc_table* t = nullptr;   // the base table under the leaves: borrowed until sc_gp_destroy_ext, never written
  sc::ExtGpLeaf lf;              // w, alpha, beta
  PoolBuf tree;                  // two heaps of 2^n words: layer k of plane c at words c 2^n + [2^k, 2^(k+1)), k < n
  u64 product[2] = {0, 0};       // V_0[0]
};

namespace {

int check_gp_ext(sc_ctx* ctx, const sc_gp_ext* g, const char* what) {
  if (!g || g->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: not an extension product tree of this context", what);
  return SC_OK;
}

// the launches of the tree (tree_schedule): ext_gp_tree_kernel from layer m over lv layers, ext_gp_tree_tail_kernel below layer
// kExtGpTailLog; the launch from layer n forms the leaves in registers
int ext_gp_build_tree(sc_ctx* ctx, sc_gp_ext* g, int tree_lv) {
  u64* const tree = g->tree.get();
  const size_t heap = (size_t)1 << g->n;
  const sc::ExtGpLeaf lf = g->lf;
  return tree_schedule(g->n, sc::kExtGpTailLog, tree_lv, [&](int m, int lv) {
    const bool leaf_in = m == g->n;
    const u64* src = leaf_in ? (const u64*)g->t->d : (const u64*)tree + ((size_t)1 << m);
    const u64 read = (u64)(leaf_in ? 8 : 16) << m;
    if (lv == 0)
      return launch_recorded(ctx, {SC_KIND_EXT_PRODUCT_TREE, 0, leaf_in ? 1 : 2, m, read, ((u64)16 << m) - 16}, "ext_gp_tree_tail_kernel", [&] {
        SC_DISPATCH_FIELD(ctx, F, f, with_bool(leaf_in, [&](auto LEAF_IN) {
          hipLaunchKernelGGL((sc::ext_gp_tree_tail_kernel<F, LEAF_IN>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, f, lf, src, heap, tree, heap, m);
        }));
      });
    const int log_low = m - lv;
    const size_t n_units = (size_t)1 << (log_low - 1);
    const int grid = grid_for(ctx, n_units);
    return launch_recorded(ctx, {SC_KIND_EXT_PRODUCT_TREE, lv, leaf_in ? 1 : 2, m, read, ((u64)16 << m) - ((u64)16 << log_low)}, "ext_gp_tree_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f, with_bool(leaf_in, [&](auto LEAF_IN) {
        with_const<1, 2, 3>(lv, [&](auto LV) {
          hipLaunchKernelGGL((sc::ext_gp_tree_kernel<F, LV, LEAF_IN>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, lf, src, heap, tree, heap, log_low,
                             n_units);
        });
      }));
    });
  });
}

// eq(z, .) for z in K^k, k >= 1, as two planes of 2^k words in one pool block
int build_ext_eq_table(sc_ctx* ctx, u64 w, const u64* z, int k, PoolBuf* out) {
  PoolBuf t;
  SC_TRY(t.alloc(ctx, (size_t)2 << k));
  const sc::RVec rv = make_rvec(z, (size_t)2 * k);
  const size_t n_pairs = (size_t)1 << (k - 1);
  const int grid = grid_for_wide(ctx, n_pairs);
  u64* const o = t.get();
  SC_TRY(launch_recorded(ctx, {SC_KIND_EXT_EQ_TABLE, 0, 0, k, (u64)16 * k, (u64)16 << k}, "ext_eq_table_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::ext_eq_table_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, rv, w, k, n_pairs, o));
  }));
  *out = std::move(t);
  return SC_OK;
}

}  // namespace

extern "C" int sc_gp_create_ext(sc_ctx* ctx, uint64_t w, const sc_table* t, const uint64_t alpha[2], const uint64_t beta[2], sc_gp_ext** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_gp_create_ext"));
  SC_TRY(require_cubic_field(ctx, "sc_gp_create_ext"));
  if (!t || !alpha || !beta || !out) return fail(ctx, SC_ERR_ARG, "sc_gp_create_ext: a NULL argument");
  SC_TRY(check_table(ctx, t, "sc_gp_create_ext"));
  if (t->len < 2 || t->len > ((size_t)1 << sc::kGpMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_gp_create_ext: a table of %zu entries (at least two, at most 2^%d)", t->len, sc::kGpMaxLog);
  const HostField hf(ctx->fp);
  SC_TRY(check_nonresidue(ctx, hf, w, "sc_gp_create_ext"));
  for (int c = 0; c < 2; ++c)
    if (alpha[c] >= ctx->fp.p || beta[c] >= ctx->fp.p)
      return fail(ctx, SC_ERR_ARG, "sc_gp_create_ext: component %d of alpha or beta is not a word below p", c);
  if (alpha[0] == 0 && alpha[1] == 0) return fail(ctx, SC_ERR_ARG, "sc_gp_create_ext: alpha is zero");
  SC_TRY(set_device(ctx));
  std::unique_ptr<sc_gp_ext> g(new (std::nothrow) sc_gp_ext);
  if (!g) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  g->ctx = ctx;
  g->n = log2_of(t->len);
  g->t = t;
  g->lf.w = w;
  for (int c = 0; c < 2; ++c) {
    g->lf.alpha[c] = alpha[c];
    g->lf.beta[c] = beta[c];
  }
  SC_TRY(g->tree.alloc(ctx, 2 * t->len));
  SC_TRY(ext_gp_build_tree(ctx, g.get(), ctx->gp_tree_lv));
  SC_HIP(ctx, hipMemcpyAsync(&g->product[0], g->tree.get() + 1, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, hipMemcpyAsync(&g->product[1], g->tree.get() + t->len + 1, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  *out = g.release();
  return SC_OK;
}

extern "C" int sc_gp_destroy_ext(sc_ctx* ctx, sc_gp_ext* g) {
  if (!g) return SC_OK;
  if (!ctx || g->ctx != ctx) return SC_ERR_ARG;
  delete g;   // (the tree goes back to the pool)
  return SC_OK;
}

extern "C" int sc_gp_product_ext(const sc_gp_ext* g, uint64_t out[2]) {
  if (!g || !out) return SC_ERR_ARG;
  out[0] = g->product[0];
  out[1] = g->product[1];
  return SC_OK;
}

extern "C" int sc_gp_layer_ext(sc_ctx* ctx, const sc_gp_ext* g, size_t k, sc_table** c0, sc_table** c1) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_gp_layer_ext"));
  if (!c0 || !c1) return fail(ctx, SC_ERR_ARG, "sc_gp_layer_ext: a NULL argument");
  SC_TRY(check_gp_ext(ctx, g, "sc_gp_layer_ext"));
  if (k >= (size_t)g->n) return fail(ctx, SC_ERR_ARG, "sc_gp_layer_ext: layer %zu of a tree with layers 0 .. %d", k, g->n - 1);
  SC_TRY(set_device(ctx));
  TableBuf a, b;
  SC_TRY(a.alloc(ctx, (size_t)1 << k));
  SC_TRY(b.alloc(ctx, (size_t)1 << k));
  const u64* src = g->tree.get() + ((size_t)1 << k);
  hipError_t e = hipMemcpyAsync(a->d, src, sizeof(u64) << k, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(b->d, src + ((size_t)1 << g->n), sizeof(u64) << k, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = sync_stream(ctx);
  if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "sc_gp_layer_ext: %s", hipGetErrorString(e));   // (both tables are freed)
  *c0 = a.release();
  *c1 = b.release();
  return SC_OK;
}

extern "C" int sc_gp_prove_ext(sc_ctx* ctx, const sc_gp_ext* g, sc_draw_gp_ext_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                               uint64_t* challenges, uint64_t* point, uint64_t* claim) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_gp_prove_ext"));
  SC_TRY(require_cubic_field(ctx, "sc_gp_prove_ext"));
  if (!finals || !point || !claim) return fail(ctx, SC_ERR_ARG, "sc_gp_prove_ext: a NULL argument");
  SC_TRY(check_gp_ext(ctx, g, "sc_gp_prove_ext"));
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  const sc::MontGeneric& hfield = hf.f;
  const sc::ExtGpLeaf& lf = g->lf;
  const u64 w = lf.w;
  const int n = g->n, T = ctx->gp_host_log;
  const size_t heap = (size_t)1 << n;
  // the bottom of the tree on the host, once per proof: the layers 0 .. min(T + 1, n) of both planes in the heap layout (layer
  // k <= T reads V_(k+1); V_n is formed here from the caller's table)
  const int top = std::min(T + 1, n);
  std::vector<u64> bottom[2], base_words;
  {
    const size_t tree_words = std::min((size_t)2 << top, heap);
    for (int c = 0; c < 2; ++c) {
      bottom[c].resize((size_t)2 << top);
      SC_HIP(ctx, hipMemcpyAsync(bottom[c].data(), g->tree.get() + (size_t)c * heap, tree_words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (top == n) {
      base_words.resize(heap);
      SC_HIP(ctx, hipMemcpyAsync(base_words.data(), g->t->d, heap * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    }
    SC_HIP(ctx, sync_stream(ctx));
    for (size_t i = 0; i < base_words.size(); ++i) {
      u64 o[2];
      sc::ext_gp_leaf(hfield, lf.alpha, lf.beta, base_words[i], o);
      bottom[0][heap + i] = o[0];
      bottom[1][heap + i] = o[1];
    }
  }
  // (the resident blocks of the planes-in fold: the most registers)
  const int resident = resident_blocks(ctx, &sc::ext_gp_pass_kernel<sc::GoldilocksMont, true, false>, &sc::ext_gp_pass_kernel<sc::MontGeneric, true, false>);

  // the challenger, in protocol order: one draw per round and one per rho, two words each
  u64 n_draws = 0;
  int rc = SC_OK;
  auto challenge = [&](size_t layer, size_t round, const u64* msg, u64* out) {
    u64 c[2];
    if (draw) {
      draw(user, layer, round, msg, c);
    } else {
      for (int s = 0; s < 2; ++s) c[s] = seeded_challenge(ctx, hf, seed_r, 2 * n_draws + (u64)s);
    }
    n_draws += 1;
    if (c[0] >= ctx->fp.p || c[1] >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_gp_prove_ext: draw() returned a challenge with an unreduced component");
      return false;
    }
    out[0] = c[0];
    out[1] = c[1];
    return true;
  };

  std::vector<u64> z((size_t)2 * n), rs((size_t)2 * (n + 1)), host, leaves;
  u64 c_k[2] = {g->product[0], g->product[1]};
  for (int k = 0; k < n; ++k) {
    const size_t len = (size_t)1 << k;
    u64* const ev = evals ? evals + 4 * (size_t)k * (size_t)(k > 0 ? k - 1 : 0) : nullptr;   // 8 k (k - 1) / 2 words before layer k
    auto next = [&](size_t round, const u64* msg, u64* out) {
      if (ev) memcpy(ev + 8 * round, msg, 8 * sizeof(u64));
      return challenge((size_t)k, round, msg, out);
    };
    u64* pl[6];
    if (k <= T) {
      // the whole layer on the host
      host.assign(6 * len, 0);
      for (int q = 0; q < 6; ++q) pl[q] = host.data() + (size_t)q * len;
      sc::ext_gp_host_eq(hfield, w, z.data(), k, pl[0], pl[1]);
      for (int c = 0; c < 2; ++c) {
        const u64* lk = bottom[c].data() + 2 * len;
        std::copy(lk, lk + len, pl[2 + c]);
        std::copy(lk + len, lk + 2 * len, pl[4 + c]);
      }
      if (!sc::ext_gp_host_rounds(hfield, w, pl, k, 0, nullptr, rs.data(), next)) return rc;
    } else {
      // the device runs the rounds 0 .. k - te; the launch of round k - te leaves tables of 2^te entries, which the host takes
      const int te = std::max(T, 1);
      PoolBuf cur[3];
      SC_TRY(build_ext_eq_table(ctx, w, z.data(), k, &cur[0]));
      // The layer's own tables: E in two planes of 2^k words, the halves of layer k + 1 as planes a heap apart - or, under the
      // leaves (k = n - 1), the halves of t as base words.  The launches of rounds 0 and 1 read them (round 1 is the first fold);
      // from round 2 on a launch reads folded tables, two adjacent planes of 2^log_in words.
      const bool leaf_layer = k == n - 1;
      const u64* lk = leaf_layer ? (const u64*)g->t->d : (const u64*)g->tree.get() + 2 * len;
      const u64* in[3] = {cur[0].get(), lk, lk + len};
      u64 e[8];
      SC_TRY((device_rounds<3, 2, 4>(ctx, 3, k, te, in, cur, rs.data(), e, &rc, [&](const DeviceRound& d, Launched* l) {
        const bool fold = d.round > 0, own = d.round <= 1, leaf = own && leaf_layer;
        sc::ExtGpTables tb;
        for (int q = 0; q < 3; ++q) {
          tb.in[q] = d.in[q];
          tb.stride[q] = own ? (q == 0 ? len : heap) : (size_t)1 << d.log_in;
          tb.out[q] = d.out[q];
        }
        *l = {d.grid(resident), 8};
        SC_TRY(timer_begin(ctx, SC_KIND_EXT_PRODUCT_PASS, fold ? 1 : 0, leaf ? 1 : 2, d.log_in, ((u64)16 << d.log_in) + ((u64)(leaf ? 16 : 32) << d.log_in),
                           fold ? (u64)48 << (d.log_in - 1) : 0));
        SC_DISPATCH_FIELD(ctx, F, f, with_bool(fold, [&](auto FOLD) {
          with_bool(leaf, [&](auto LEAF_IN) {
            hipLaunchKernelGGL((sc::ext_gp_pass_kernel<F, FOLD, LEAF_IN>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, lf, d.r_prev[0], d.r_prev[1],
                               d.n_units, d.po);
          });
        }));
        return SC_OK;
      }, next)));
      // what the host takes: folded tables (planes 2^te words apart) - or, where the one launch folded nothing (k = te), the
      // layer's own, whose leaves are formed below
      const size_t left = (size_t)1 << te;
      const bool folded = k > te, leaves_in = leaf_layer && !folded;
      host.assign(6 * left, 0);
      for (int q = 0; q < 6; ++q) pl[q] = host.data() + (size_t)q * left;
      if (leaves_in) leaves.resize(2 * left);
      for (int q = 0; q < 3; ++q) {
        if (leaves_in && q > 0) {
          SC_HIP(ctx, hipMemcpyAsync(leaves.data() + (size_t)(q - 1) * left, in[q], left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
          continue;
        }
        const size_t stride = folded ? left : q == 0 ? len : heap;
        for (int c = 0; c < 2; ++c) SC_HIP(ctx, hipMemcpyAsync(pl[2 * q + c], in[q] + (size_t)c * stride, left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      }
      SC_HIP(ctx, sync_stream(ctx));
      if (leaves_in)
        for (int q = 1; q < 3; ++q)
          for (size_t i = 0; i < left; ++i) {
            u64 o[2];
            sc::ext_gp_leaf(hfield, lf.alpha, lf.beta, leaves[(size_t)(q - 1) * left + i], o);
            pl[2 * q][i] = o[0];
            pl[2 * q + 1][i] = o[1];
          }
      if (!sc::ext_gp_host_rounds(hfield, w, pl, te, (size_t)(k - te), e, rs.data(), next)) return rc;
    }
    const u64 fin[4] = {pl[2][0], pl[3][0], pl[4][0], pl[5][0]};
    memcpy(finals + 4 * (size_t)k, fin, sizeof(fin));
    u64 rho[2] = {0, 0};
    if (!challenge((size_t)k, (size_t)k, fin, rho)) return rc;
    rs[2 * (size_t)k] = rho[0];
    rs[2 * (size_t)k + 1] = rho[1];
    if (challenges) memcpy(challenges + (size_t)k * ((size_t)k + 1), rs.data(), 2 * ((size_t)k + 1) * sizeof(u64));
    const u64 l[2] = {fin[0], fin[1]}, r2[2] = {fin[2], fin[3]};
    sc::ext_fold(hfield, w, rho, l, r2, c_k);
    std::copy(rs.begin(), rs.begin() + 2 * (k + 1), z.begin());   // z_(k+1) = (r, rho_k)
  }
  memcpy(point, z.data(), (size_t)2 * n * sizeof(u64));
  claim[0] = c_k[0];
  claim[1] = c_k[1];
  return SC_OK;
}
