// Part of sumcheck_hip.hip (included there, in order, after abi_ext_gp.inc): LogUp's fraction sums over the quadratic extension
// K = F_p[X] / (X^2 - w) (kernels/ext_fraction.hpp states the protocol): the fraction-sum trees of the leaves (p, beta + alpha t) over
// K, the layered cubic sumcheck over them with every challenge in K, and its host finish.

struct sc_frac_ext {
  sc_ctx* ctx = nullptr;
  int n = 0;
  const sc_table* p = nullptr;   // the base table under the numerators, or null: all ones.  Borrowed until sc_frac_destroy_ext, never written
  const sc_table* t = nullptr;   // the base table under the denominators: borrowed, never written
  sc::ExtGpLeaf lf;              // w, alpha, beta
  PoolBuf tree;                  // four heaps of 2^n words (p.c0, p.c1, q.c0, q.c1): layer k of heap h at words h 2^n + [2^k, 2^(k+1)), k < n
  u64 root[4] = {0, 0, 0, 0};    // (P, Q)
};

namespace {

int check_frac_ext(sc_ctx* ctx, const sc_frac_ext* g, const char* what) {
  if (!g || g->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: not an extension fraction tree of this context", what);
  return SC_OK;
}

// the launches of the tree (tree_schedule): ext_fr_tree_kernel from layer m over lv layers, ext_fr_tree_tail_kernel below layer
// kExtFrTailLog; the launch from layer n forms the leaves in registers
int ext_fr_build_tree(sc_ctx* ctx, sc_frac_ext* g, int tree_lv) {
  u64* const tree = g->tree.get();
  const size_t heap = (size_t)1 << g->n;
  const sc::ExtGpLeaf lf = g->lf;
  const bool ones_in = !g->p;
  return tree_schedule(g->n, sc::kExtFrTailLog, tree_lv, [&](int m, int lv) {
    const bool leaf_in = m == g->n, ones = leaf_in && ones_in;
    const u64* ps = leaf_in ? (g->p ? (const u64*)g->p->d : nullptr) : (const u64*)tree + ((size_t)1 << m);
    const u64* qs = leaf_in ? (const u64*)g->t->d : (const u64*)tree + 2 * heap + ((size_t)1 << m);
    const int ks = leaf_in ? (ones ? 1 : 2) : 4;
    const u64 read = (u64)(8 * ks) << m;
    if (lv == 0)
      return launch_recorded(ctx, {SC_KIND_EXT_FRACTION_TREE, 0, ks, m, read, ((u64)32 << m) - 32}, "ext_fr_tree_tail_kernel", [&] {
        SC_DISPATCH_FIELD(ctx, F, f, with_bool(leaf_in, [&](auto LEAF_IN) {
          with_bool(ones, [&](auto ONES) {
            hipLaunchKernelGGL((sc::ext_fr_tree_tail_kernel<F, LEAF_IN, ONES>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, f, lf, ps, qs, heap, tree, heap, m);
          });
        }));
      });
    const int log_low = m - lv;
    const size_t n_units = (size_t)1 << (log_low - 1);
    const int grid = grid_for(ctx, n_units);
    return launch_recorded(ctx, {SC_KIND_EXT_FRACTION_TREE, lv, ks, m, read, ((u64)32 << m) - ((u64)32 << log_low)}, "ext_fr_tree_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3>(lv, [&](auto LV) {
        // (ONES only with LEAF_IN: three forms)
        if (ones)
          hipLaunchKernelGGL((sc::ext_fr_tree_kernel<F, LV, true, true>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, lf, ps, qs, heap, tree, heap, log_low,
                             n_units);
        else
          with_bool(leaf_in, [&](auto LEAF_IN) {
            hipLaunchKernelGGL((sc::ext_fr_tree_kernel<F, LV, LEAF_IN, false>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, lf, ps, qs, heap, tree, heap,
                               log_low, n_units);
          });
      }));
    });
  });
}

}  // namespace

extern "C" int sc_frac_create_ext(sc_ctx* ctx, uint64_t w, const sc_table* p, const sc_table* t, const uint64_t alpha[2], const uint64_t beta[2],
                                  sc_frac_ext** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_frac_create_ext"));
  SC_TRY(require_cubic_field(ctx, "sc_frac_create_ext"));
  if (!t || !alpha || !beta || !out) return fail(ctx, SC_ERR_ARG, "sc_frac_create_ext: a NULL argument");
  SC_TRY(check_table(ctx, t, "sc_frac_create_ext"));
  if (p) SC_TRY(check_table(ctx, p, "sc_frac_create_ext"));
  if (t->len < 2 || t->len > ((size_t)1 << sc::kFrMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_frac_create_ext: a table of %zu entries (at least two, at most 2^%d)", t->len, sc::kFrMaxLog);
  if (p && p->len != t->len) return fail(ctx, SC_ERR_ARG, "sc_frac_create_ext: p has %zu entries, t has %zu", p->len, t->len);
  const HostField hf(ctx->fp);
  SC_TRY(check_nonresidue(ctx, hf, w, "sc_frac_create_ext"));
  for (int c = 0; c < 2; ++c)
    if (alpha[c] >= ctx->fp.p || beta[c] >= ctx->fp.p)
      return fail(ctx, SC_ERR_ARG, "sc_frac_create_ext: component %d of alpha or beta is not a word below p", c);
  if (alpha[0] == 0 && alpha[1] == 0) return fail(ctx, SC_ERR_ARG, "sc_frac_create_ext: alpha is zero");
  SC_TRY(set_device(ctx));
  std::unique_ptr<sc_frac_ext> g(new (std::nothrow) sc_frac_ext);
  if (!g) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  g->ctx = ctx;
  g->n = log2_of(t->len);
  g->p = p;
  g->t = t;
  g->lf.w = w;
  for (int c = 0; c < 2; ++c) {
    g->lf.alpha[c] = alpha[c];
    g->lf.beta[c] = beta[c];
  }
  SC_TRY(g->tree.alloc(ctx, 4 * t->len));
  SC_TRY(ext_fr_build_tree(ctx, g.get(), ctx->fr_tree_lv));
  for (int h = 0; h < 4; ++h)
    SC_HIP(ctx, hipMemcpyAsync(&g->root[h], g->tree.get() + (size_t)h * t->len + 1, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  *out = g.release();
  return SC_OK;
}

extern "C" int sc_frac_destroy_ext(sc_ctx* ctx, sc_frac_ext* g) {
  if (!g) return SC_OK;
  if (!ctx || g->ctx != ctx) return SC_ERR_ARG;
  delete g;   // (the tree goes back to the pool)
  return SC_OK;
}

extern "C" int sc_frac_root_ext(const sc_frac_ext* g, uint64_t out[4]) {
  if (!g || !out) return SC_ERR_ARG;
  for (int h = 0; h < 4; ++h) out[h] = g->root[h];
  return SC_OK;
}

extern "C" int sc_frac_layer_ext(sc_ctx* ctx, const sc_frac_ext* g, size_t k, int which, sc_table** c0, sc_table** c1) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_frac_layer_ext"));
  if (!c0 || !c1) return fail(ctx, SC_ERR_ARG, "sc_frac_layer_ext: a NULL argument");
  SC_TRY(check_frac_ext(ctx, g, "sc_frac_layer_ext"));
  if (k >= (size_t)g->n) return fail(ctx, SC_ERR_ARG, "sc_frac_layer_ext: layer %zu of trees with layers 0 .. %d", k, g->n - 1);
  if (which != 0 && which != 1) return fail(ctx, SC_ERR_ARG, "sc_frac_layer_ext: which = %d (0: p, 1: q)", which);
  SC_TRY(set_device(ctx));
  TableBuf a, b;
  SC_TRY(a.alloc(ctx, (size_t)1 << k));
  SC_TRY(b.alloc(ctx, (size_t)1 << k));
  const size_t heap = (size_t)1 << g->n;
  const u64* src = g->tree.get() + (size_t)(2 * which) * heap + ((size_t)1 << k);
  hipError_t e = hipMemcpyAsync(a->d, src, sizeof(u64) << k, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(b->d, src + heap, sizeof(u64) << k, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = sync_stream(ctx);
  if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "sc_frac_layer_ext: %s", hipGetErrorString(e));   // (both tables are freed)
  *c0 = a.release();
  *c1 = b.release();
  return SC_OK;
}

extern "C" int sc_frac_prove_ext(sc_ctx* ctx, const sc_frac_ext* g, sc_draw_frac_ext_fn draw, void* user, uint64_t seed_r, uint64_t* evals,
                                 uint64_t* finals, uint64_t* challenges, uint64_t* point, uint64_t claims[4]) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_frac_prove_ext"));
  SC_TRY(require_cubic_field(ctx, "sc_frac_prove_ext"));
  if (!finals || !point || !claims) return fail(ctx, SC_ERR_ARG, "sc_frac_prove_ext: a NULL argument");
  SC_TRY(check_frac_ext(ctx, g, "sc_frac_prove_ext"));
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  const sc::MontGeneric& hfield = hf.f;
  const sc::ExtGpLeaf& lf = g->lf;
  const u64 w = lf.w, one = hfield.one();
  const int n = g->n, T = ctx->fr_host_log;
  const size_t heap = (size_t)1 << n;
  const bool ones = !g->p;
  // the bottom of the four heaps on the host, once per proof: the layers 0 .. min(T + 1, n) in the heap layout (layer k <= T reads
  // layer k + 1; layer n is formed here from the caller's tables)
  const int top = std::min(T + 1, n);
  std::vector<u64> bottom[4], base_words[2];
  {
    const size_t tree_words = std::min((size_t)2 << top, heap);
    for (int h = 0; h < 4; ++h) {
      bottom[h].resize((size_t)2 << top);
      SC_HIP(ctx, hipMemcpyAsync(bottom[h].data(), g->tree.get() + (size_t)h * heap, tree_words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (top == n) {
      base_words[1].resize(heap);
      SC_HIP(ctx, hipMemcpyAsync(base_words[1].data(), g->t->d, heap * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      if (!ones) {
        base_words[0].resize(heap);
        SC_HIP(ctx, hipMemcpyAsync(base_words[0].data(), g->p->d, heap * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      }
    }
    SC_HIP(ctx, sync_stream(ctx));
    for (size_t i = 0; i < base_words[1].size(); ++i) {
      u64 o[2];
      sc::ext_gp_leaf(hfield, lf.alpha, lf.beta, base_words[1][i], o);
      bottom[0][heap + i] = ones ? one : base_words[0][i];
      bottom[1][heap + i] = 0;
      bottom[2][heap + i] = o[0];
      bottom[3][heap + i] = o[1];
    }
  }
  // (the resident blocks of the planes-in fold over five tables: the most registers)
  const int resident =
      resident_blocks(ctx, &sc::ext_fr_pass_kernel<sc::GoldilocksMont, true, false, false>, &sc::ext_fr_pass_kernel<sc::MontGeneric, true, false, false>);

  // the challenger, in protocol order: per layer its lambda (k >= 1), one draw per round, and rho - two words each
  u64 n_draws = 0;
  int rc = SC_OK;
  auto challenge = [&](size_t layer, size_t round, const u64* msg, u64* out) {
    u64 c[2];
    if (draw) {
      draw(user, layer, round, msg, c);
    } else {
      for (int s = 0; s < 2; ++s) c[s] = seeded_challenge(ctx, hf, seed_r, 2 * n_draws + (u64)s);
    }
    if (c[0] >= ctx->fp.p || c[1] >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_frac_prove_ext: draw() returned a challenge with an unreduced component");
      return false;
    }
    if (challenges) {
      challenges[2 * n_draws] = c[0];
      challenges[2 * n_draws + 1] = c[1];
    }
    n_draws += 1;
    out[0] = c[0];
    out[1] = c[1];
    return true;
  };

  std::vector<u64> z((size_t)2 * n), rs((size_t)2 * (n + 1)), host, leaves;
  u64 lambda[2] = {0, 0}, a_k[2] = {g->root[0], g->root[1]}, b_k[2] = {g->root[2], g->root[3]};
  for (int k = 0; k < n; ++k) {
    const size_t len = (size_t)1 << k;
    const bool leaf_layer = k == n - 1;
    const int nt = ones && leaf_layer ? 3 : 5;   // the tables of this layer: E, QL, QR (, PL, PR)
    u64* const ev = evals ? evals + 4 * (size_t)k * (size_t)(k > 0 ? k - 1 : 0) : nullptr;   // 8 k (k - 1) / 2 words before layer k
    auto next = [&](size_t round, const u64* msg, u64* out) {
      if (ev) memcpy(ev + 8 * round, msg, 8 * sizeof(u64));
      return challenge((size_t)k, round, msg, out);
    };
    const sc::ExtFrLambda lam = {{lambda[0], lambda[1]}};
    u64* pl[10] = {};
    // heap h of table q >= 1: QL, QR are the halves of q (heaps 2, 3), PL, PR those of p (heaps 0, 1)
    auto heap_of = [](int q, int c) { return (q == sc::kFrQL || q == sc::kFrQR ? 2 : 0) + c; };
    auto right = [](int q) { return q == sc::kFrQR || q == sc::kFrPR; };
    if (k <= T) {
      // the whole layer on the host
      host.assign((size_t)2 * nt * len, 0);
      for (int q = 0; q < 2 * nt; ++q) pl[q] = host.data() + (size_t)q * len;
      sc::ext_gp_host_eq(hfield, w, z.data(), k, pl[0], pl[1]);
      for (int q = 1; q < nt; ++q)
        for (int c = 0; c < 2; ++c) {
          const u64* lk = bottom[heap_of(q, c)].data() + 2 * len + (right(q) ? len : 0);
          std::copy(lk, lk + len, pl[2 * q + c]);
        }
      if (!sc::ext_fr_host_rounds(hfield, w, pl, nt, lam.v, k, 0, nullptr, rs.data(), next)) return rc;
    } else {
      // the device runs the rounds 0 .. k - te; the launch of round k - te leaves tables of 2^te entries, which the host takes
      const int te = std::max(T, 1);
      PoolBuf cur[5];
      SC_TRY(build_ext_eq_table(ctx, w, z.data(), k, &cur[0]));
      // The layer's own tables: E in two planes of 2^k words, the halves of layer k + 1 as planes a heap apart - or, under the
      // leaves (k = n - 1), the halves of t and p as base words.  The launches of rounds 0 and 1 read them (round 1 is the first
      // fold); from round 2 on a launch reads folded tables, two adjacent planes of 2^log_in words.
      const u64* in[5] = {cur[0].get(), nullptr, nullptr, nullptr, nullptr};
      for (int q = 1; q < nt; ++q) {
        const bool is_q = q == sc::kFrQL || q == sc::kFrQR;
        const u64* lk = leaf_layer ? (const u64*)(is_q ? g->t->d : g->p->d) : (const u64*)g->tree.get() + (size_t)heap_of(q, 0) * heap + 2 * len;
        in[q] = lk + (right(q) ? len : 0);
      }
      u64 e[8];
      SC_TRY((device_rounds<5, 2, 4>(ctx, nt, k, te, in, cur, rs.data(), e, &rc, [&](const DeviceRound& d, Launched* l) {
        const bool fold = d.round > 0, own = d.round <= 1, leaf = own && leaf_layer;
        sc::ExtFrTables tb;
        for (int q = 0; q < 5; ++q) {
          tb.in[q] = q < nt ? d.in[q] : nullptr;
          tb.stride[q] = own ? (q == 0 ? len : heap) : (size_t)1 << d.log_in;
          tb.out[q] = d.out[q];
        }
        *l = {d.grid(resident), 8};
        const int ks = (nt - 1) * (leaf ? 1 : 2);   // the words per entry of L and R it reads
        SC_TRY(timer_begin(ctx, SC_KIND_EXT_FRACTION_PASS, fold ? 1 : 0, ks, d.log_in, ((u64)16 << d.log_in) + ((u64)(8 * ks) << d.log_in),
                           fold ? (u64)(16 * nt) << (d.log_in - 1) : 0));
        SC_DISPATCH_FIELD(ctx, F, f, with_bool(fold, [&](auto FOLD) {
          with_bool(leaf, [&](auto LEAF_IN) {
            with_bool(nt == 3, [&](auto ONES) {
              hipLaunchKernelGGL((sc::ext_fr_pass_kernel<F, FOLD, LEAF_IN, ONES>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, lf, lam, d.r_prev[0],
                                 d.r_prev[1], d.n_units, d.po);
            });
          });
        }));
        return SC_OK;
      }, next)));
      // what the host takes: folded tables (planes 2^te words apart) - or, where the one launch folded nothing (k = te), the
      // layer's own, whose leaves are formed below
      const size_t left = (size_t)1 << te;
      const bool folded = k > te, leaves_in = leaf_layer && !folded;
      host.assign((size_t)2 * nt * left, 0);
      for (int q = 0; q < 2 * nt; ++q) pl[q] = host.data() + (size_t)q * left;
      if (leaves_in) leaves.resize((size_t)(nt - 1) * left);
      for (int q = 0; q < nt; ++q) {
        if (leaves_in && q > 0) {
          SC_HIP(ctx, hipMemcpyAsync(leaves.data() + (size_t)(q - 1) * left, in[q], left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
          continue;
        }
        const size_t stride = folded ? left : q == 0 ? len : heap;
        for (int c = 0; c < 2; ++c) SC_HIP(ctx, hipMemcpyAsync(pl[2 * q + c], in[q] + (size_t)c * stride, left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      }
      SC_HIP(ctx, sync_stream(ctx));
      if (leaves_in)
        for (int q = 1; q < nt; ++q)
          for (size_t i = 0; i < left; ++i) {
            const u64 x = leaves[(size_t)(q - 1) * left + i];
            u64 o[2] = {x, 0};   // a numerator: (p, 0)
            if (q == sc::kFrQL || q == sc::kFrQR) sc::ext_gp_leaf(hfield, lf.alpha, lf.beta, x, o);
            pl[2 * q][i] = o[0];
            pl[2 * q + 1][i] = o[1];
          }
      if (!sc::ext_fr_host_rounds(hfield, w, pl, nt, lam.v, te, (size_t)(k - te), e, rs.data(), next)) return rc;
    }
    // pl, pr, ql, qr
    u64 fin[8] = {one, 0, one, 0, pl[2 * sc::kFrQL][0], pl[2 * sc::kFrQL + 1][0], pl[2 * sc::kFrQR][0], pl[2 * sc::kFrQR + 1][0]};
    if (nt == 5) {
      fin[0] = pl[2 * sc::kFrPL][0];
      fin[1] = pl[2 * sc::kFrPL + 1][0];
      fin[2] = pl[2 * sc::kFrPR][0];
      fin[3] = pl[2 * sc::kFrPR + 1][0];
    }
    memcpy(finals + 8 * (size_t)k, fin, sizeof(fin));
    u64 rho[2] = {0, 0};
    if (!challenge((size_t)k, (size_t)k, fin, rho)) return rc;
    rs[2 * (size_t)k] = rho[0];
    rs[2 * (size_t)k + 1] = rho[1];
    const u64 fpl[2] = {fin[0], fin[1]}, fpr[2] = {fin[2], fin[3]}, fql[2] = {fin[4], fin[5]}, fqr[2] = {fin[6], fin[7]};
    sc::ext_fold(hfield, w, rho, fpl, fpr, a_k);
    sc::ext_fold(hfield, w, rho, fql, fqr, b_k);
    std::copy(rs.begin(), rs.begin() + 2 * (k + 1), z.begin());   // z_(k+1) = (r, rho_k)
    if (k + 1 < n && !challenge((size_t)k, (size_t)k + 1, nullptr, lambda)) return rc;   // lambda of the next layer
  }
  memcpy(point, z.data(), (size_t)2 * n * sizeof(u64));
  claims[0] = a_k[0];
  claims[1] = a_k[1];
  claims[2] = b_k[0];
  claims[3] = b_k[1];
  return SC_OK;
}
