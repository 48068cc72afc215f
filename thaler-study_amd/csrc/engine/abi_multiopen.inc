// Part of sumcheck_hip.hip (included there, in order): batched openings (kernels/multiopen.hpp states the protocol): the weighted
// sum of eq tables and the sumcheck over a sum of products of table pairs with shared challenges and a host finish.

namespace {

// how many blocks of sumprod_pass_kernel the device holds at once (the occupancy does not depend on T: the loop over t is not unrolled)
int sumprod_pass_resident(sc_ctx* ctx) {
  return resident_blocks(ctx, &sc::sumprod_pass_kernel<sc::GoldilocksMont, sc::kSumprodMaxPairs, true>,
                         &sc::sumprod_pass_kernel<sc::MontGeneric, sc::kSumprodMaxPairs, true>);
}

// the 2T tables of a device round (a_0 .. a_(T-1), b_0 .. b_(T-1)) as the sum-of-products kernels take them
sc::SpTables sumprod_tables(const DeviceRound& d, int T) {
  sc::SpTables tb;
  memset(&tb, 0, sizeof(tb));
  for (int t = 0; t < T; ++t) {
    tb.a[t] = d.in[t];
    tb.ao[t] = d.out[t];
    tb.b[t] = d.in[T + t];
    tb.bo[t] = d.out[T + t];
  }
  return tb;
}

}  // namespace

extern "C" int sc_table_eq_sum(sc_ctx* ctx, const uint64_t* points, const uint64_t* coeffs, size_t count, size_t n, sc_table** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_table_eq_sum"));
  if (!points || !coeffs || !out) return fail(ctx, SC_ERR_ARG, "sc_table_eq_sum: a NULL argument");
  if (count < 1 || count > (size_t)sc::kEqSumMaxCount || n < 1 || n > (size_t)sc::kEqSumMaxLog)
    return fail(ctx, SC_ERR_ARG, "sc_table_eq_sum: count = %zu must be in 1..%d and n = %zu in 1..%d", count, sc::kEqSumMaxCount, n, sc::kEqSumMaxLog);
  for (size_t i = 0; i < count * n; ++i)
    if (points[i] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_table_eq_sum: coordinate %zu of point %zu is not a word below p", i % n, i / n);
  for (size_t k = 0; k < count; ++k)
    if (coeffs[k] >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "sc_table_eq_sum: coeffs[%zu] is not a word below p", k);
  SC_TRY(set_device(ctx));
  // the points and, behind them, the coefficients: one small block the kernel reads
  std::vector<u64> host(points, points + count * n);
  host.insert(host.end(), coeffs, coeffs + count);
  PoolBuf pc;
  SC_TRY(pc.alloc(ctx, host.size()));
  SC_HIP(ctx, hipMemcpyAsync(pc.get(), host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
  TableBuf t;
  SC_TRY(t.alloc(ctx, (size_t)1 << n));
  const size_t n_high = (size_t)1 << (n > (size_t)sc::kEqSumLoLog ? n - sc::kEqSumLoLog : 0);
  const unsigned grid = strided_grid(ctx, n_high);   // (one chunk of kBlock high indices per block and turn)
  SC_TRY(launch_recorded(ctx, {SC_KIND_EQ_SUM, 0, (int)count, (int)n, (u64)8 * host.size(), (u64)8 << n}, "eq_sum_kernel", [&] {
    SC_DISPATCH_FIELD(ctx, F, f, hipLaunchKernelGGL((sc::eq_sum_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, (const u64*)pc.get(),
                                                    (int)count, (int)n, t->d));
  }));
  return table_done(ctx, t, hipSuccess, "sc_table_eq_sum", out);   // (drains the stream: the host vector and the block go away)
}

extern "C" int sc_sumprod_prove(sc_ctx* ctx, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_fn draw, void* user,
                                uint64_t seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges, uint64_t* finals_a, uint64_t* finals_b) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(one_device_only(ctx, "sc_sumprod_prove"));
  if (!a || !b || !c1 || !finals_a || !finals_b) return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove: a NULL argument");
  if (count < 1 || count > (size_t)sc::kSumprodMaxPairs)
    return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove: count = %zu must be in 1..%d", count, sc::kSumprodMaxPairs);
  const int T = (int)count;
  for (int t = 0; t < T; ++t) {
    if (!a[t] || !b[t]) return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove: pair %d has a NULL table", t);
    SC_TRY(check_table(ctx, a[t], "sc_sumprod_prove"));
    SC_TRY(check_table(ctx, b[t], "sc_sumprod_prove"));
  }
  const size_t len = a[0]->len;
  for (int t = 0; t < T; ++t)
    if (a[t]->len != len || b[t]->len != len)
      return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove: pair %d has tables of %zu and %zu entries, pair 0 of %zu", t, a[t]->len, b[t]->len, len);
  if (len < 2 || !is_pow2(len) || len > ((size_t)1 << sc::kGpMaxLog))
    return fail(ctx, SC_ERR_ARG, "sc_sumprod_prove: tables of %zu entries (a power of two, at least two, at most 2^%d)", len, sc::kGpMaxLog);
  SC_TRY(set_device(ctx));
  const HostField hf(ctx->fp);
  const sc::MontGeneric& hfield = hf.f;
  const int n = log2_of(len), H = ctx->gp_host_log;

  int rc = SC_OK;
  auto next = [&](size_t round, const u64* msg, u64* out) {
    if (round == 0) *c1 = hf.add(msg[0], msg[1]);
    if (evals) memcpy(evals + 3 * round, msg, 3 * sizeof(u64));
    const u64 r = draw ? draw(user, round, msg) : seeded_challenge(ctx, hf, seed_r, round);
    if (r >= ctx->fp.p) {
      rc = fail(ctx, SC_ERR_ARG, "sc_sumprod_prove: draw() returned an unreduced challenge");
      return false;
    }
    *out = r;
    return true;
  };

  // the rounds the host runs: all of them over tables of at most 2^H entries, else the tail from what the last launch wrote
  const int te = n <= H ? n : std::max(H, 1);
  const size_t left = (size_t)1 << te;
  std::vector<u64> rs((size_t)n), host((size_t)2 * T * left);
  PoolBuf cur[2 * sc::kSumprodMaxPairs];
  const u64* in[2 * sc::kSumprodMaxPairs];
  u64* ha[sc::kSumprodMaxPairs];
  u64* hb[sc::kSumprodMaxPairs];
  for (int t = 0; t < T; ++t) {
    in[t] = a[t]->d;
    in[T + t] = b[t]->d;
    ha[t] = host.data() + (size_t)t * left;
    hb[t] = host.data() + (size_t)(T + t) * left;
  }
  u64 e[3];
  if (n > te) {
    // one launch of sumprod_pass_kernel per round (SC_KIND_SUMPROD_PASS), three values each
    const int resident = sumprod_pass_resident(ctx);
    SC_TRY((device_rounds<2 * sc::kSumprodMaxPairs, 1, 2>(ctx, 2 * T, n, te, in, cur, rs.data(), e, &rc, [&](const DeviceRound& d, Launched* l) {
      const bool fold = d.round > 0;
      const sc::SpTables tb = sumprod_tables(d, T);
      const u64 bytes = ((u64)16 * (u64)T) << d.log_in;
      *l = {d.grid(resident), 3};
      SC_TRY(timer_begin(ctx, SC_KIND_SUMPROD_PASS, fold ? 1 : 0, T, d.log_in, bytes, fold ? bytes / 2 : 0));
      SC_DISPATCH_FIELD(ctx, F, f, with_bool(fold, [&](auto FOLD) {
        with_const<1, 2, 3, 4, 5, 6, 7, 8>(T, [&](auto TT) {
          hipLaunchKernelGGL((sc::sumprod_pass_kernel<F, TT, FOLD>), dim3(l->grid), dim3(sc::kBlock), 0, ctx->stream, f, tb, d.r_prev[0], d.n_units, d.po);
        });
      }));
      return SC_OK;
    }, next)));
  }
  for (int q = 0; q < 2 * T; ++q)
    SC_HIP(ctx, hipMemcpyAsync(host.data() + (size_t)q * left, in[q], left * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  if (!sc::sp_host_rounds(hfield, (size_t)T, ha, hb, te, (size_t)(n - te), n > te ? e : nullptr, rs.data(), next)) return rc;
  for (int t = 0; t < T; ++t) {
    finals_a[t] = ha[t][0];
    finals_b[t] = hb[t][0];
  }
  if (challenges) memcpy(challenges, rs.data(), (size_t)n * sizeof(u64));
  return SC_OK;
}
