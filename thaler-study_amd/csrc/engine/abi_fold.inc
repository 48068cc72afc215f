// Part of sumcheck_hip.hip (included there, in order, after abi_row_code.inc): C ABI: the folded opening of a Reed-Solomon
// sc_ligero (kernels/rs_fold.hpp states the contract) - one launch of folds of a codeword (sc_rs_fold, sc_rs_fold_many), and
// the prover of an opening: the two claims (begin), the sumcheck rounds with the folds and the layer trees between them
// (prove), and the opened layer leaves (query).  The rows are combined by engine/abi_ligero.inc, encoded by the row code's
// encoder, the rounds are sc_prover_round's and the trees engine/merkle.inc's; what is new is rs_fold_kernel.

// An opening in progress: the two combined rows until prove has run, then the layers of the stages 1 .. S-1 and their trees.
struct sc_ligero_fold {
  const sc_ctx* ctx = nullptr;
  const sc_ligero* lg = nullptr;   // borrowed: must outlive the opening
  bool proved = false;
  int kind = SC_KIND_RS_FOLD;      // of its fold records; begun with a schedule: SC_KIND_RS_FOLD_MANY
  std::vector<int> arities;        // a_0 .. a_(S-1); sc_ligero_fold_begin: c ones
  std::vector<u64> z_lo;
  PoolBuf rows;                    // u_z, then u_gamma: C words each
  std::vector<PoolBuf> layers;     // layers[k] = U_(i_(k+1)), the layer of stage k+1: 2^(l0 - i_(k+1)) words
  std::vector<MerkleLevels> trees; // trees[k]: over the 2^(l0 - i_(k+1) - a_(k+1)) leaves of that layer
};

namespace {

// out = the 2^log_m words of U folded `a` times with alphas[0 .. a), 2^(log_m - a) >= 2 words; an != 0: the digests of out's
// leaves of 2^an words go to `leaves`.  As layer l0 - log_m of an opening whose layer 0 has 2^log_len0 words.  One launch,
// recorded as `kind`: SC_KIND_RS_FOLD (a = 1, an <= 1; kf = 1 if hashed) or SC_KIND_RS_FOLD_MANY (kf = a)
int rs_fold_launch(sc_ctx* ctx, const u64* U, int log_m, int log_len0, const u64* alphas, int a, int an, int log_in, u64* out, u32* leaves,
                   int kind) {
  const HostField hf(ctx->fp);
  const TwoAdicRoot root = two_adic_root(ctx);
  sc::RsFoldArgs k = {};
  // zeta = w_M^(-M/2^a) and eta = w_M^(-M/2^(a+w)): the inverses of the contract's roots of those orders
  const int w = sc::rs_fold_item_log(an);
  sc::rs_fold_constants(hf, hf.inv(hf.add(hf.one(), hf.one())), hf.inv(hf.pow(root.w_max, (u64)1 << (root.s - a))),
                        hf.inv(hf.pow(root.w_max, (u64)1 << (root.s - a - w))), alphas, a, w, &k);
  k.log_len0 = log_len0;
  k.shift = log_len0 - log_m;
  if (log_len0 >= sc::kRsFoldTwistMinLog) {
    SC_TRY(rs_twist_tables(ctx, log_len0, &k.lo, &k.hi));
  } else {
    sc::RsRoots unused;
    SC_TRY(rs_twiddles(ctx, log_len0, &k.lo, &unused));
  }
  const u64 M = (u64)1 << log_m;
  const u32 items = (u32)(M >> (a + w));
  const int kf = kind == SC_KIND_RS_FOLD ? (an ? 1 : 0) : a;
  return launch_recorded(ctx, {kind, kf, log_m, log_in, 8 * M, (8 * M >> a) + (an ? 32 * (u64)items : 0)}, "rs_fold_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3>(a, [&](auto A) {
                        with_const<0, 1, 2, 3>(an, [&](auto AN) {
                          hipLaunchKernelGGL((sc::rs_fold_kernel<F, A, AN>), dim3(strided_grid(ctx, items)), dim3(sc::kBlock), 0, ctx->stream, f,
                                             U, out, k, items, leaves);
                        });
                      }));
  });
}

int fold_check(sc_ctx* ctx, const sc_ligero_fold* fd, const char* what) {
  if (fd->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: the opening belongs to another context", what);
  return SC_OK;
}

struct ProverGuard {
  sc_prover* p = nullptr;
  ~ProverGuard() { sc_prover_destroy(p); }
};
struct FoldGuard {
  sc_ligero_fold* p = nullptr;
  ~FoldGuard() { delete p; }
};

// sc_rs_fold (one == true: a single challenge, and the messages say so) and sc_rs_fold_many
int rs_fold_table(sc_ctx* ctx, const sc_table* u, const u64* alphas, size_t count, bool one, sc_table** out) {
  const char* what = one ? "sc_rs_fold" : "sc_rs_fold_many";
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  SC_TRY(one_device_only(ctx, what));
  SC_TRY(check_table(ctx, u, what));
  if (!one) {
    if (count < 1 || count > 3) return fail(ctx, SC_ERR_ARG, "sc_rs_fold_many: %zu challenges (1 .. 3 fold in one launch)", count);
    if (!alphas) return fail(ctx, SC_ERR_ARG, "sc_rs_fold_many: null pointer");
  }
  if (u->len < (size_t)2 << count) {
    if (one) return fail(ctx, SC_ERR_ARG, "sc_rs_fold: a codeword of %zu words (at least 4)", u->len);
    return fail(ctx, SC_ERR_ARG, "sc_rs_fold_many: a codeword of %zu words (at least %zu for %zu folds)", u->len, (size_t)2 << count, count);
  }
  const int log_m = log2_of(u->len), s = two_adic_root(ctx).s;
  if (log_m > sc::kRsLongMaxLog)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: a codeword of 2^%d words is longer than 2^%d", what, log_m, sc::kRsLongMaxLog);
  if (log_m > s)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: p = %llu has 2-adicity %d: no root of unity of order 2^%d", what, (unsigned long long)ctx->fp.p, s,
                log_m);
  for (size_t k = 0; k < count; ++k)
    if (alphas[k] >= ctx->fp.p)
      return one ? fail(ctx, SC_ERR_ARG, "sc_rs_fold: alpha is not reduced") : fail(ctx, SC_ERR_ARG, "sc_rs_fold_many: alpha %zu is not reduced", k);
  SC_TRY(set_device(ctx));
  TableBuf t;
  SC_TRY(t.alloc(ctx, u->len >> count));
  SC_TRY(rs_fold_launch(ctx, u->d, log_m, log_m, alphas, (int)count, 0, log_m, t->d, nullptr, one ? SC_KIND_RS_FOLD : SC_KIND_RS_FOLD_MANY));
  return table_done(ctx, t, hipSuccess, what, out);
}

}  // namespace

extern "C" int sc_rs_fold(sc_ctx* ctx, const sc_table* u, uint64_t alpha, sc_table** out) { return rs_fold_table(ctx, u, &alpha, 1, true, out); }

extern "C" int sc_rs_fold_many(sc_ctx* ctx, const sc_table* u, const uint64_t* alphas, size_t count, sc_table** out) {
  return rs_fold_table(ctx, u, alphas, count, false, out);
}

namespace {

// sc_ligero_fold_begin (arities == null: c ones, the binary opening) and sc_ligero_fold_begin_staged
int fold_begin(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* point, const uint64_t* gamma, const int32_t* arities, size_t stages,
               uint64_t claims[2], sc_ligero_fold** out, const char* what) {
  if (!lg || !point || !gamma || !claims) return fail(ctx, SC_ERR_ARG, "%s: null pointer", what);
  SC_TRY(one_device_only(ctx, what));
  SC_TRY(ligero_check(ctx, lg, what));
  if (lg->code != SC_CODE_RS)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: the expander code does not fold: a Reed-Solomon commitment is needed", what);
  if (lg->c == 0) return fail(ctx, SC_ERR_ARG, "%s: log_cols = 0 leaves nothing to fold: use the plain opening", what);
  if (arities) {
    size_t sum = 0;
    for (size_t k = 0; k < stages; ++k) {
      if (arities[k] < 1 || arities[k] > 3) return fail(ctx, SC_ERR_ARG, "%s: stage %zu folds %d variables (1 .. 3)", what, k, (int)arities[k]);
      sum += (size_t)arities[k];
    }
    if (sum != (size_t)lg->c) return fail(ctx, SC_ERR_ARG, "%s: the schedule folds %zu variables, log_cols is %d", what, sum, lg->c);
  }
  const size_t R = (size_t)1 << lg->r, C = (size_t)1 << lg->c;
  const u64 p = ctx->fp.p;
  for (int k = 0; k < lg->r + lg->c; ++k)
    if (point[k] >= p) return fail(ctx, SC_ERR_ARG, "%s: coordinate %d of the point is not reduced", what, k);
  for (size_t i = 0; i < R; ++i)
    if (gamma[i] >= p) return fail(ctx, SC_ERR_ARG, "%s: gamma[%zu] is not reduced", what, i);
  SC_TRY(set_device(ctx));
  FoldGuard guard{new (std::nothrow) sc_ligero_fold};
  sc_ligero_fold* fd = guard.p;
  if (!fd) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  fd->ctx = ctx;
  fd->lg = lg;
  fd->z_lo.assign(point, point + lg->c);
  if (arities) fd->kind = SC_KIND_RS_FOLD_MANY;
  if (arities) fd->arities.assign(arities, arities + stages);
  else fd->arities.assign((size_t)lg->c, 1);
  // the weights of u_z - eq(z_hi, i), LE - then gamma
  const HostField hf(ctx->fp);
  std::vector<u64> w(2 * R);
  w[0] = hf.one();
  for (int k = 0; k < lg->r; ++k) {
    const u64 r = point[lg->c + k];
    for (size_t i = 0; i < (size_t)1 << k; ++i) {
      const u64 hi = hf.mul(w[i], r);
      w[i + ((size_t)1 << k)] = hi;
      w[i] = hf.sub(w[i], hi);
    }
  }
  std::copy(gamma, gamma + R, w.begin() + R);
  SC_TRY(ligero_combine_device(ctx, lg, w.data(), 2, &fd->rows));
  for (int m = 0; m < 2; ++m) {
    sc_table row;   // (a view of the block: nothing to free)
    row.d = fd->rows.get() + m * C;
    row.len = C;
    SC_TRY(sc_table_evaluate(ctx, &row, fd->z_lo.data(), (size_t)lg->c, SC_ORDER_LE, &claims[m]));
  }
  guard.p = nullptr;
  *out = fd;
  return SC_OK;
}

}  // namespace

extern "C" int sc_ligero_fold_begin(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* point, const uint64_t* gamma, uint64_t claims[2],
                                    sc_ligero_fold** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  return fold_begin(ctx, lg, point, gamma, nullptr, 0, claims, out, "sc_ligero_fold_begin");
}

extern "C" int sc_ligero_fold_begin_staged(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* point, const uint64_t* gamma, const int32_t* arities,
                                           size_t stages, uint64_t claims[2], sc_ligero_fold** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  if (!arities || stages == 0) return fail(ctx, SC_ERR_ARG, "sc_ligero_fold_begin_staged: a null or empty schedule");
  return fold_begin(ctx, lg, point, gamma, arities, stages, claims, out, "sc_ligero_fold_begin_staged");
}

extern "C" int sc_ligero_fold_prove(sc_ctx* ctx, sc_ligero_fold* fd, uint64_t beta, sc_draw_fold_fn draw, void* user, uint64_t* evals,
                                    uint8_t* roots, uint64_t* challenges, uint64_t* final_value) {
  if (!ctx || !fd) return SC_ERR_ARG;
  SC_TRY(fold_check(ctx, fd, "sc_ligero_fold_prove"));
  const sc_ligero* lg = fd->lg;
  const int c = lg->c, rho = lg->rho, n = lg->r + lg->c, l0 = c + rho;
  const std::vector<int>& ar = fd->arities;
  const size_t S = ar.size();
  if (!draw || !evals || !final_value || (S > 1 && !roots)) return fail(ctx, SC_ERR_ARG, "sc_ligero_fold_prove: null pointer");
  if (fd->proved) return fail(ctx, SC_ERR_STATE, "sc_ligero_fold_prove: this opening has been proved already");
  if (beta >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_ligero_fold_prove: beta is not reduced");
  SC_TRY(set_device(ctx));
  const size_t C = (size_t)1 << c;
  // m = u_z + beta u_gamma and eq(z_lo): the two tables of the sumcheck
  TableBuf tm, teq;
  {
    PoolBuf m, eq;
    SC_TRY(m.alloc(ctx, C));
    const u64* rows = fd->rows.get();
    SC_DISPATCH_FIELD(ctx, F, f,
                      hipLaunchKernelGGL((sc::rs_fold_mix_kernel<F>), dim3(strided_grid(ctx, C)), dim3(sc::kBlock), 0, ctx->stream, f, rows,
                                         rows + C, beta, (u32)C, m.get()));
    if (hipGetLastError() != hipSuccess) {
      poison(ctx);
      return fail(ctx, SC_ERR_HIP, "rs_fold_mix_kernel launch failed");
    }
    SC_TRY(build_eq_table(ctx, fd->z_lo.data(), c, &eq));
    SC_TRY(tm.wrap(ctx, std::move(m), C));
    SC_TRY(teq.wrap(ctx, std::move(eq), C));
  }
  // U_0 = Enc(m): one row through the row code's encoder
  PoolBuf u0;
  SC_TRY(u0.alloc(ctx, (size_t)1 << l0));
  SC_TRY(rs_encode_long_impl(ctx, tm->d, c, c, rho, u0));
  const u64* cur = u0.get();
  ProverGuard pr;
  SC_TRY(sc_prover_create(ctx, tm.get(), teq.get(), &pr.p));
  std::vector<PoolBuf> layers;
  std::vector<MerkleLevels> trees;
  u64 alpha = 0;
  for (size_t st = 0, i0 = 0; st < S; i0 += (size_t)ar[st], ++st) {
    // the rounds of the stage; the first carries the root of the stage's layer
    u64 alphas[3];
    for (int k = 0; k < ar[st]; ++k) {
      const size_t i = i0 + (size_t)k;
      SC_TRY(sc_prover_round(pr.p, alpha, i, evals + 3 * i));
      uint8_t* root = st && k == 0 ? roots + 32 * (st - 1) : nullptr;
      if (root) sc::put_digest(root, trees.back().root);
      alpha = draw(user, i, evals + 3 * i, root);
      if (alpha >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_ligero_fold_prove: draw() returned an unreduced challenge");
      if (challenges) challenges[i] = alpha;
      alphas[k] = alpha;
    }
    // U_(i0) -> U_(i0 + a); every stage's layer but the last result gets its tree
    const int a = ar[st], log_m = l0 - (int)i0, an = st + 1 < S ? ar[st + 1] : 0;
    PoolBuf next;
    SC_TRY(next.alloc(ctx, (size_t)1 << (log_m - a)));
    MerkleLevels t;
    if (an) SC_TRY(t.alloc(ctx, log_m - a - an));
    u32* leaves = an ? t.words() : nullptr;
    SC_TRY(rs_fold_launch(ctx, cur, log_m, l0, alphas, a, an, n, next, leaves, fd->kind));
    if (an) {
      SC_TRY(merkle_finish(ctx, &t, 0, n));
      u0.reset();   // (U_0 goes back to the pool once it is folded; a layer stays with `layers`)
      cur = next.get();
      layers.push_back(std::move(next));
      trees.push_back(std::move(t));
    } else {
      SC_HIP(ctx, hipMemcpyAsync(final_value, next.get(), sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  fd->layers = std::move(layers);
  fd->trees = std::move(trees);
  fd->rows.reset();
  fd->proved = true;
  return SC_OK;
}

// pairs[q][W] (Montgomery), W = sum_{s>=1} 2^(a_s), and paths[q][P][32], P = sum_{s>=1} (l0 - i_s - a_s): the stages in order, each
// path bottom up
extern "C" int sc_ligero_fold_query(sc_ctx* ctx, const sc_ligero_fold* fd, const uint64_t* q, size_t count, uint64_t* pairs, uint8_t* paths) {
  if (!ctx || !fd) return SC_ERR_ARG;
  SC_TRY(fold_check(ctx, fd, "sc_ligero_fold_query"));
  if (!fd->proved) return fail(ctx, SC_ERR_STATE, "sc_ligero_fold_query: the opening has not been proved yet (sc_ligero_fold_prove)");
  if (count == 0) return SC_OK;
  const int c = fd->lg->c, l0 = c + fd->lg->rho, n = fd->lg->r + c;
  const std::vector<int>& ar = fd->arities;
  const size_t S = ar.size();
  if (!q || (S > 1 && (!pairs || !paths))) return fail(ctx, SC_ERR_ARG, "sc_ligero_fold_query: null array");
  for (size_t k = 0; k < count; ++k)
    if (q[k] >= (u64)1 << (l0 - ar[0]))
      return fail(ctx, SC_ERR_ARG, "sc_ligero_fold_query: index %llu of query %zu is not below L / %d = 2^%d", (unsigned long long)q[k], k,
                  1 << ar[0], l0 - ar[0]);
  if (S == 1) return SC_OK;
  SC_TRY(set_device(ctx));
  // stage s >= 1 as a 2^(a_s) x 2^depth[s] matrix, W words and P digests per query in all
  std::vector<int> depth(S, 0);
  size_t P = 0, W = 0;
  for (size_t s = 1, i = (size_t)ar[0]; s < S; i += (size_t)ar[s], ++s) {
    depth[s] = l0 - (int)i - ar[s];
    P += (size_t)depth[s];
    W += (size_t)1 << ar[s];
  }
  // every stage's launch is queued, then one wait: per chunk of queries and stage s, chunk indices, 2^(a_s) chunk words and
  // chunk depth[s] digests, the stages one behind the other
  const size_t chunk = std::min<size_t>(count, 1024), layers = S - 1;
  PoolBuf buf;
  SC_TRY(buf.alloc(ctx, chunk * (layers + W + 4 * P)));
  u64* d_idx = buf;
  u64* d_vals = d_idx + layers * chunk;
  u32* d_sib = reinterpret_cast<u32*>(d_vals + W * chunk);
  std::vector<u64> idx(layers * chunk), vals(W * chunk);
  std::vector<u32> hs(8 * P * chunk);
  for (size_t q0 = 0; q0 < count; q0 += chunk) {
    const size_t k = std::min(chunk, count - q0);
    for (size_t s = 1; s < S; ++s)
      for (size_t t = 0; t < k; ++t) idx[(s - 1) * chunk + t] = q[q0 + t] & (((u64)1 << depth[s]) - 1);
    SC_HIP(ctx, hipMemcpyAsync(d_idx, idx.data(), layers * chunk * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    size_t first = 0, word = 0;
    for (size_t s = 1; s < S; ++s) {
      // column j_s and its path, through the commitment's opening kernel
      const u64 rows = (u64)1 << ar[s], len = (u64)1 << depth[s], moved = (u64)k * (8 * rows + 32 * depth[s]);
      const size_t li = s - 1;
      SC_TRY(launch_recorded(ctx, {SC_KIND_LIGERO, 2, (int)k, n, moved, moved}, "column_open_kernel", [&] {
        hipLaunchKernelGGL(sc::column_open_kernel, dim3((unsigned)std::min<size_t>(k, (size_t)8 * ctx->num_cus)), dim3(sc::kBlock), 0, ctx->stream,
                           (const u64*)fd->layers[li].get(), (const u32*)fd->trees[li].words(), (const u64*)(d_idx + li * chunk), (u32)k, rows,
                           (u32)len, depth[s], d_vals + word * chunk, d_sib + 8 * first * chunk);
      }));
      first += (size_t)depth[s];
      word += (size_t)rows;
    }
    SC_HIP(ctx, hipMemcpyAsync(vals.data(), d_vals, W * chunk * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(hs.data(), d_sib, 32 * P * chunk, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    first = word = 0;
    for (size_t s = 1; s < S; ++s) {
      const size_t rows = (size_t)1 << ar[s];
      for (size_t t = 0; t < k; ++t) std::copy_n(&vals[word * chunk + rows * t], rows, pairs + (q0 + t) * W + word);
      sc::put_paths(paths + q0 * P * 32, (int)P, (int)first, hs.data() + 8 * first * chunk, k, depth[s]);
      first += (size_t)depth[s];
      word += rows;
    }
  }
  return SC_OK;
}

extern "C" int sc_ligero_fold_destroy(sc_ctx* ctx, sc_ligero_fold* fd) {
  if (!fd) return SC_OK;
  if (!ctx || fd->ctx != ctx) return SC_ERR_ARG;
  delete fd;
  return SC_OK;
}
