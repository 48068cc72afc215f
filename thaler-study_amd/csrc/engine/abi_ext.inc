// Part of sumcheck_hip.hip (included there, in order, after abi_multiopen.inc): the sum-of-products sumcheck with challenges from
// the quadratic extension K = F_p[X] / (X^2 - w), and the evaluation of a base table at a point of K^n (kernels/ext_sumprod.hpp
// states the conventions).  Round 0 is sumprod_pass_kernel, the base-field launch; every later device round is ext_sumprod_pass_kernel.

namespace {

// how many blocks of ext_sumprod_pass_kernel the device holds at once (the extension-in form of the widest T: the most registers)
int ext_sumprod_resident(sc_ctx* ctx) {
  return resident_blocks(ctx, &sc::ext_sumprod_pass_kernel<sc::GoldilocksMont, sc::kSumprodMaxPairs, false>,
                         &sc::ext_sumprod_pass_kernel<sc::MontGeneric, sc::kSumprodMaxPairs, false>);
}

// w must be a word below p and a quadratic non-residue: w^((p-1)/2) = -1
int check_nonresidue(sc_ctx* ctx, const HostField& hf, u64 w, const char* what) {
  if (w >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "%s: w is not a word below p", what);
  if (hf.pow(w, (ctx->fp.p - 1) / 2) != hf.neg(hf.one()))
    return fail(ctx, SC_ERR_ARG, "%s: w is not a quadratic non-residue of the field (w^((p-1)/2) is not p - 1)", what);
  return SC_OK;
}

}  // namespace

extern "C" int sc_sumprod_prove_ext(sc_ctx* ctx, uint64_t w, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_ext_fn draw,
                                    void* user, uint64_t seed_r, uint64_t c1[2], uint64_t* evals, uint64_t* challenges, uint64_t* finals_a,
                                    uint64_t* finals_b) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_sumprod_prove_ext"));
  if (!a || !b || !c1 || !finals_a || !finals_b) return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove_ext: a NULL argument");
  if (count < 1 || count > (size_t)sc::kSumprodMaxPairs)
    return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove_ext: count = %zu must be in 1..%d", count, sc::kSumprodMaxPairs);
  const int T = (int)count;
  for (int t = 0; t < T; ++t) {
    if (!a[t] || !b[t]) return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove_ext: pair %d has a NULL table", t);
    SC_TRY(check_table(ctx, a[t], "sc_sumprod_prove_ext"));
    SC_TRY(check_table(ctx, b[t], "sc_sumprod_prove_ext"));
  }
  const size_t len = a[0]->len;
  for (int t = 0; t < T; ++t)
    if (a[t]->len != len || b[t]->len != len)
      return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove_ext: pair %d has tables of %zu and %zu entries, pair 0 of %zu", t, a[t]->len, b[t]->len, len);
  if (len < 2 || !is_pow2(len) || len > ((size_t)1 << sc::kGpMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove_ext: tables of %zu entries (a power of two, at least two, at most 2^%d)", len, sc::kGpMaxLog);
  const HostField hf(ctx->fp);
  SC_TRY(check_nonresidue(ctx, hf, w, "sc_sumprod_prove_ext"));
  SC_TRY(set_device(ctx));
  const sc::MontGeneric& hfield = hf.f;
  const int n = log2_of(len), H = ctx->gp_host_log;

  int rc = SC_OK;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    if (round == 0) {
      c1[0] = hf.add(msg[0], msg[2]);
      c1[1] = hf.add(msg[1], msg[3]);
    }
    if (evals) memcpy(evals + 6 * round, msg, 6 * sizeof(u64));
    u64 r[2];
    if (draw) {
      draw(user, round, msg, r);
    } else {
      for (int k = 0; k < 2; ++k) r[k] = seeded_challenge(ctx, hf, seed_r, 2 * (u64)round + (u64)k);
    }
    if (r[0] >= ctx->fp.p || r[1] >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_sumprod_prove_ext: draw() returned a challenge with an unreduced component");
      return false;
    }
    out[0] = r[0];
    out[1] = r[1];
    return true;
  };

  // the rounds the host runs: all of them over tables of at most 2^H entries, else the tail from what the last launch wrote
  const int te = n <= H ? n : std::max(H, 1);
  const size_t left = (size_t)1 << te;
  std::vector<u64> rs((size_t)2 * n), host((size_t)4 * T * left, 0);   // per table: the c0 plane, then the c1 plane
  PoolBuf cur[2 * sc::kSumprodMaxPairs];
  const u64* in[2 * sc::kSumprodMaxPairs];
  u64* pl[4 * sc::kSumprodMaxPairs];
  for (int t = 0; t < T; ++t) {
    in[t] = a[t]->d;
    in[T + t] = b[t]->d;
  }
  for (int q = 0; q < 4 * T; ++q) pl[q] = host.data() + (size_t)q * left;
  u64 e[6];
  const bool on_device = n > te;
  if (on_device) {
    // Round 0 has nothing to fold and base tables: sumprod_pass_kernel, whose three sums are the c0 words of the round's message.
    // It is never the hand-over (n > te), so next() sees every message of that form and widens it first.  The launch of round 1
    // folds base tables into planes, every later one planes into planes; folded tables are two planes of 2 n_units words.
    const int resident0 = sumprod_pass_resident(ctx), resident = ext_sumprod_resident(ctx);
    auto widened = [&](size_t round, u64* msg, u64* out) {
      if (round == 0)
        for (int s = 2; s >= 0; --s) {
          msg[2 * s] = msg[s];
          msg[2 * s + 1] = 0;
        }
      return next(round, msg, out);
    };
    SC_TRY((device_rounds<2 * sc::kSumprodMaxPairs, 2, 4>(ctx, 2 * T, n, te, in, cur, rs.data(), e, &rc, [&](const DeviceRound& d, Launched* l) {
      const sc::SpTables tb = sumprod_tables(d, T);
      const u64 words = ((u64)2 * (u64)T) << d.log_in;   // entries of all input tables
      if (d.round == 0) {
        *l = {d.grid(resident0), 3};
        SC_TRY(timer_begin(ctx, SC_KIND_SUMPROD_PASS, 0, T, d.log_in, 8 * words, 0));
        SC_DISPATCH_FIELD(ctx, F, f, with_const<1, 2, 3, 4, 5, 6, 7, 8>(T, [&](auto TT) {
          hipLaunchKernelGGL((sc::sumprod_pass_kernel<F, TT, false>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, (u64)0, d.n_units, d.po);
        }));
        return SC_OK;
      }
      const bool base_in = d.round == 1;
      *l = {d.grid(resident), 6};
      SC_TRY(timer_begin(ctx, SC_KIND_SUMPROD_EXT_PASS, base_in ? 1 : 2, T, d.log_in, (base_in ? 8 : 16) * words, 8 * words));
      SC_DISPATCH_FIELD(ctx, F, f, with_bool(base_in, [&](auto BASE_IN) {
        with_const<1, 2, 3, 4, 5, 6, 7, 8>(T, [&](auto TT) {
          hipLaunchKernelGGL((sc::ext_sumprod_pass_kernel<F, TT, BASE_IN>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, w, d.r_prev[0],
                             d.r_prev[1], d.n_units, d.po);
        });
      }));
      return SC_OK;
    }, widened)));
  }
  // a folded table is its two planes, adjacent; a base table fills the c0 plane and leaves the zeros of the c1 plane
  for (int q = 0; q < 2 * T; ++q)
    SC_HIP(ctx, hipMemcpyAsync(pl[2 * q], in[q], (on_device ? 2 : 1) * left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  if (!sc::ext_host_rounds(hfield, w, (size_t)T, pl, te, (size_t)(n - te), !on_device, on_device ? e : nullptr, rs.data(), next)) return rc;
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < 2; ++k) {
      finals_a[2 * t + k] = pl[2 * t + k][0];
      finals_b[2 * t + k] = pl[2 * (T + t) + k][0];
    }
  if (challenges) memcpy(challenges, rs.data(), (size_t)2 * n * sizeof(u64));
  return SC_OK;
}

extern "C" int sc_table_evaluate_ext(sc_ctx* ctx, uint64_t w, const sc_table* t, const uint64_t* point, size_t n, uint64_t out[2]) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_table_evaluate_ext"));
  if (!t || !point || !out) return fail(ctx, SC_ERR_ARG, "sc_table_evaluate_ext: a NULL argument");
  SC_TRY(check_table(ctx, t, "sc_table_evaluate_ext"));
  if (n < 1 || n > (size_t)sc::kGpMaxLog || t->len != ((size_t)1 << n))
    return fail(ctx, SC_ERR_ARG, "sc_table_evaluate_ext: a table of %zu entries and a point of %zu coordinates (2^n entries, n in 1..%d)", t->len, n,
                sc::kGpMaxLog);
  for (size_t i = 0; i < 2 * n; ++i)
    if (point[i] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_table_evaluate_ext: component %zu of coordinate %zu is not a word below p", i % 2, i / 2);
  const HostField hf(ctx->fp);
  SC_TRY(check_nonresidue(ctx, hf, w, "sc_table_evaluate_ext"));
  SC_TRY(set_device(ctx));
  const int nv = (int)n, H = ctx->gp_host_log;
  const int te = nv <= H ? nv : std::max(H, 1);
  const size_t left = (size_t)1 << te;
  // the same folds as the prover's, one table, down to the hand-over: launch j folds coordinate j
  PoolBuf cur, nxt;
  const u64* in = t->d;
  for (int j = 0; j < nv - te; ++j) {
    const bool base_in = j == 0;
    const int log_in = nv - j;
    const size_t n_units = (size_t)1 << (log_in - 2);
    SC_TRY(nxt.alloc(ctx, (size_t)4 * n_units));
    u64* const o = nxt.get();
    const unsigned grid = strided_grid(ctx, n_units);
    const u64 words = (u64)1 << log_in;
    SC_TRY(launch_recorded(ctx, {SC_KIND_SUMPROD_EXT_PASS, base_in ? 1 : 2, 0, log_in, (base_in ? 8 : 16) * words, 8 * words}, "ext_fold_kernel", [&] {
      SC_DISPATCH_FIELD(ctx, F, f, with_bool(base_in, [&](auto BASE_IN) {
        hipLaunchKernelGGL((sc::ext_fold_kernel<F, BASE_IN>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, in, o, w, point[2 * j], point[2 * j + 1],
                           n_units);
      }));
    }));
    cur = std::move(nxt);
    in = cur.get();
  }
  const bool on_device = nv > te;
  std::vector<u64> host(2 * left, 0);
  SC_HIP(ctx, hipMemcpyAsync(host.data(), in, (on_device ? 2 : 1) * left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  sc::ext_host_evaluate(hf.f, w, host.data(), host.data() + left, te, point + 2 * (size_t)(nv - te), !on_device);
  out[0] = host[0];
  out[1] = host[left];
  return SC_OK;
}
