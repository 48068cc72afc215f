// Part of sumcheck_hip.hip (included there, in order): C ABI: gkr_protocol::circuit::Circuit on the device, and the GKR
// prover driven over it.

// =====================================================================================
// C ABI: Circuit (gkr-protocol/src/circuit.rs:72-124) and the whole GKR prover (lib.rs:324-474)
// =====================================================================================

// A circuit resident on one context: every layer's gate list in ONE pool block of 32-bit words, layer i at off[i] as
// [type | in0 | in1], each array stride[i] = max(2^k[i], 4) words (16-byte aligned: kernels/circuit.hpp).  Checked once,
// on upload.
struct sc_circuit {
  sc_ctx* ctx = nullptr;   // the context that made it (its pool owns `words`)
  size_t depth = 0;
  std::vector<size_t> k;        // depth + 1 entries; k[depth] = input variables
  std::vector<size_t> off, stride;
  PoolBuf words;
};

namespace {

size_t circuit_stride(size_t k) { return std::max<size_t>((size_t)1 << k, 4); }

// the checks every call on a circuit makes, in this order: the context's kind (before looking at the circuit), then the
// circuit's owner
int check_circuit_ctx(sc_ctx* ctx, const sc_circuit* c, const char* what) {
  if (is_multi(ctx) || ctx->world > 1)
    return fail(ctx, SC_ERR_UNSUPPORTED, "%s: circuits live on a context of one device and one rank (this one is %s)", what,
                is_multi(ctx) ? "a multi-device handle" : "sharded");
  if (!c) return fail(ctx, SC_ERR_ARG, "%s: circuit is null", what);
  if (c->ctx != ctx) return fail(ctx, SC_ERR_ARG, "%s: the circuit was made on another context", what);
  return SC_OK;
}

const unsigned* circuit_layer_words(const sc_circuit* c, size_t i) { return (const unsigned*)c->words.get() + c->off[i]; }

// values[i] of every layer, from the input up (one launch per layer on the context's stream, no host sync between them)
// (on failure none is left)
int circuit_evaluate_impl(sc_ctx* ctx, const sc_circuit* c, const sc_table* input, std::vector<TableBuf>* values) {
  std::vector<TableBuf> v(c->depth);
  for (size_t i = c->depth; i-- > 0;) {
    const size_t n = (size_t)1 << c->k[i];
    const u64* in = i + 1 == c->depth ? input->d : v[i + 1]->d;
    SC_TRY(v[i].alloc(ctx, n));
    u64* out = v[i]->d;
    // streamed: 12 B of gate words in, 8 B out per gate (the two gathers are served from the layer the previous launch wrote)
    SC_TRY(timer_begin(ctx, SC_KIND_CIRCUIT, (int)c->k[i + 1], 0, (int)c->k[i], (u64)12 * n, (u64)8 * n));
    const unsigned* w = circuit_layer_words(c, i);
    const int grid = grid_for_wide(ctx, std::max<size_t>(n >> 2, 1));
    const bool nt = c->k[i] >= (size_t)ctx->nt_load_log;
    SC_DISPATCH_FIELD(ctx, F, f, with_bool(nt, [&](auto NT) {
      hipLaunchKernelGGL((sc::circuit_layer_kernel<F, NT>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, w, n, c->stride[i], in, out);
    }));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      poison(ctx);
      return fail(ctx, SC_ERR_HIP, "circuit_layer_kernel (layer %zu) launch failed: %s", i, hipGetErrorString(e));
    }
    SC_TRY(timer_end(ctx));
  }
  *values = std::move(v);
  return SC_OK;
}

int check_circuit_input(sc_ctx* ctx, const sc_circuit* c, const sc_table* input, const char* what) {
  SC_TRY(check_table(ctx, input, what));
  if (input->len != ((size_t)1 << c->k[c->depth]))
    return fail(ctx, SC_ERR_ARG, "%s: the input (layer %zu) has %zu entries, the circuit reads 2^%zu", what, c->depth, input->len,
                c->k[c->depth]);
  return SC_OK;
}

// the prover of layer i over the circuit's own gate words: sc_gkr_prover_create_sparse without the host check, the copy and
// the sync (sp_words stays null: the circuit owns the gate words, the prover frees only what it made)
int gkr_prover_create_circuit_impl(sc_ctx* ctx, const sc_circuit* c, size_t i, const uint64_t* r_i, const sc_table* w_next,
                                   sc_gkr_prover** out) {
  const size_t k_i = c->k[i], k_next = c->k[i + 1];
  sc_gkr_prover* pr = new (std::nothrow) sc_gkr_prover;
  if (!pr) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  pr->ctx = ctx;
  pr->sparse = true;
  pr->n_gates = (size_t)1 << k_i;
  pr->w_b = pr->w_c = w_next->d;
  pr->kb = pr->kc = (int)k_next;
  const unsigned* w = circuit_layer_words(c, i);
  pr->sp_type = (int*)w;
  pr->sp_in0 = (unsigned*)w + c->stride[i];
  pr->sp_in1 = (unsigned*)w + 2 * c->stride[i];
  int rc = build_eq_table(ctx, r_i, (int)k_i, &pr->sp_val);   // eq(r_i, a): the gate's weight
  if (rc == SC_OK) rc = gkr_prover_begin(pr);
  if (rc != SC_OK) {
    sc_gkr_prover_destroy(pr);
    return rc;
  }
  *out = pr;
  return SC_OK;
}

}  // namespace

extern "C" int sc_circuit_create(sc_ctx* ctx, size_t depth, const size_t* k, const int32_t* const* gate_type,
                                 const uint32_t* const* in0, const uint32_t* const* in1, sc_circuit** out) {
  if (!ctx || !out) return SC_ERR_ARG;
  *out = nullptr;
  if (is_multi(ctx) || ctx->world > 1)
    return fail(ctx, SC_ERR_UNSUPPORTED, "sc_circuit_create: circuits live on a context of one device and one rank (this one is %s)",
                is_multi(ctx) ? "a multi-device handle" : "sharded");
  if (depth < 1 || !k || !gate_type || !in0 || !in1) return fail(ctx, SC_ERR_ARG, "sc_circuit_create: no layers, or a null array");
  for (size_t i = 0; i < depth; ++i) {
    if (k[i] > 30) return fail(ctx, SC_ERR_ARG, "sc_circuit_create: layer %zu has 2^%zu gates (at most 2^30)", i, k[i]);
    if (k[i + 1] < 1 || k[i + 1] > 26)
      return fail(ctx, SC_ERR_ARG, "sc_circuit_create: layer %zu reads 2^%zu values (1 <= k[%zu] <= 26)", i, k[i + 1], i + 1);
    if (!gate_type[i] || !in0[i] || !in1[i]) return fail(ctx, SC_ERR_ARG, "sc_circuit_create: layer %zu: null gate array", i);
  }
  // every gate, once: the kernels index without bounds checks
  for (size_t i = 0; i < depth; ++i) {
    const size_t n = (size_t)1 << k[i], n_next = (size_t)1 << k[i + 1];
    for (size_t a = 0; a < n; ++a) {
      if (gate_type[i][a] != 0 && gate_type[i][a] != 1)
        return fail(ctx, SC_ERR_ARG, "sc_circuit_create: layer %zu gate %zu has type %d (0 = add, 1 = mul)", i, a, (int)gate_type[i][a]);
      if (in0[i][a] >= n_next || in1[i][a] >= n_next)
        return fail(ctx, SC_ERR_ARG, "sc_circuit_create: layer %zu gate %zu reads (%u, %u) of a layer of %zu values", i, a,
                    (unsigned)in0[i][a], (unsigned)in1[i][a], n_next);
    }
  }
  SC_TRY(set_device(ctx));
  sc_circuit* c = new (std::nothrow) sc_circuit;
  if (!c) return fail(ctx, SC_ERR_OOM, "host allocation failed");
  c->ctx = ctx;
  c->depth = depth;
  c->k.assign(k, k + depth + 1);
  size_t total = 0;   // 32-bit words
  for (size_t i = 0; i < depth; ++i) {
    c->off.push_back(total);
    c->stride.push_back(circuit_stride(k[i]));
    total += 3 * c->stride[i];
  }
  int rc = c->words.alloc(ctx, (total + 1) / 2);
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < depth && rc == SC_OK && e == hipSuccess; ++i) {
    const size_t n = (size_t)1 << k[i];
    unsigned* w = (unsigned*)c->words.get() + c->off[i];
    e = hipMemcpyAsync(w, gate_type[i], n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w + c->stride[i], in0[i], n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w + 2 * c->stride[i], in1[i], n * 4, hipMemcpyHostToDevice, ctx->stream);
  }
  if (rc == SC_OK && e == hipSuccess) e = sync_stream(ctx);   // the host arrays may go away after return
  if (rc == SC_OK && e != hipSuccess) rc = fail(ctx, SC_ERR_HIP, "sc_circuit_create: %s", hipGetErrorString(e));
  if (rc != SC_OK) {
    delete c;
    return rc;
  }
  *out = c;
  return SC_OK;
}

extern "C" int sc_circuit_destroy(sc_ctx* ctx, sc_circuit* c) {
  if (!c) return SC_OK;
  if (!ctx) return SC_ERR_ARG;
  if (c->ctx != ctx) return fail(ctx, SC_ERR_ARG, "sc_circuit_destroy: the circuit was made on another context");
  delete c;   // (its words go back stream-ordered, like every pool block)
  return SC_OK;
}

extern "C" int sc_circuit_evaluate(sc_ctx* ctx, const sc_circuit* c, const sc_table* input, sc_table** values) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(check_circuit_ctx(ctx, c, "sc_circuit_evaluate"));
  if (!values) return fail(ctx, SC_ERR_ARG, "sc_circuit_evaluate: values is null");
  SC_TRY(check_circuit_input(ctx, c, input, "sc_circuit_evaluate"));
  SC_TRY(set_device(ctx));
  std::vector<TableBuf> v;
  SC_TRY(circuit_evaluate_impl(ctx, c, input, &v));
  for (size_t i = 0; i < c->depth; ++i) values[i] = v[i].release();
  return SC_OK;
}

extern "C" int sc_gkr_prover_create_circuit(sc_ctx* ctx, const sc_circuit* c, size_t i, const uint64_t* r_i,
                                            const sc_table* w_next, sc_gkr_prover** out) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(check_circuit_ctx(ctx, c, "sc_gkr_prover_create_circuit"));
  if (!out) return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create_circuit: out is null");
  if (i >= c->depth) return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create_circuit: layer %zu of a circuit of %zu layers", i, c->depth);
  if (c->k[i] && !r_i) return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create_circuit: layer %zu: r_i is null", i);
  SC_TRY(check_table(ctx, w_next, "sc_gkr_prover_create_circuit"));
  if (w_next->len != ((size_t)1 << c->k[i + 1]))
    return fail(ctx, SC_ERR_ARG, "sc_gkr_prover_create_circuit: layer %zu reads 2^%zu values, w_next has %zu", i, c->k[i + 1], w_next->len);
  SC_TRY(set_device(ctx));
  return gkr_prover_create_circuit_impl(ctx, c, i, r_i, w_next, out);
}

extern "C" int sc_gkr_prove_circuit(sc_ctx* ctx, const sc_circuit* c, const sc_table* input, sc_draw_fn draw, void* user,
                                    uint64_t seed_r, uint64_t* outputs, uint64_t* c1, uint64_t* evals, uint64_t* q,
                                    uint64_t* draws) {
  if (!ctx) return SC_ERR_ARG;
  SC_TRY(check_circuit_ctx(ctx, c, "sc_gkr_prove_circuit"));
  SC_TRY(check_circuit_input(ctx, c, input, "sc_gkr_prove_circuit"));
  SC_TRY(set_device(ctx));
  HostField hf(ctx->fp);
  std::vector<TableBuf> values;   // (freed on return)
  SC_TRY(circuit_evaluate_impl(ctx, c, input, &values));   // Prover::new (lib.rs:346)
  int rc = SC_OK;
  if (outputs) {   // Begin (:363-367)
    hipError_t e = hipMemcpyAsync(outputs, values[0]->d, ((size_t)1 << c->k[0]) * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = sync_stream(ctx);
    if (e != hipSuccess) rc = fail(ctx, SC_ERR_HIP, "sc_gkr_prove_circuit: reading the outputs back: %s", hipGetErrorString(e));
  }
  // the reference Verifier's draws, in its order; evals = the round's sums when the draw follows a round message
  size_t t = 0;
  auto next = [&](const u64* e, u64* r) -> int {
    const u64 v = draw ? draw(user, t, e) : seeded_challenge(ctx, hf, seed_r, t);
    if (v >= ctx->fp.p) return fail(ctx, SC_ERR_ARG, "draw() returned an unreduced challenge (draw %zu)", t);
    if (draws) draws[t] = v;
    ++t;
    *r = v;
    return SC_OK;
  };
  std::vector<u64> r(c->k[0]);
  for (size_t j = 0; j < c->k[0] && rc == SC_OK; ++j) rc = next(nullptr, &r[j]);   // r_0 (:193)
  size_t round_base = 0, q_base = 0;
  for (size_t i = 0; i < c->depth && rc == SC_OK; ++i) {
    const size_t kn = c->k[i + 1], n = 2 * kn;
    const sc_table* w_next = i + 1 == c->depth ? input : values[i + 1].get();
    sc_gkr_prover* pr = nullptr;
    rc = gkr_prover_create_circuit_impl(ctx, c, i, r.data(), w_next, &pr);   // start_round (:373-436)
    if (rc != SC_OK) break;
    if (c1) c1[i] = pr->c1;
    std::vector<u64> ch(n);
    u64 r_prev = hf.one();
    for (size_t j = 0; j < n && rc == SC_OK; ++j) {
      // the last round's message goes out with q, after the verifier's final_random_point (:110-121, :439-456)
      if (j == n - 1) rc = next(nullptr, &ch[n - 1]);
      u64 e[3];
      if (rc == SC_OK) rc = gkr_prover_round_impl(pr, r_prev, j, e);
      if (rc != SC_OK) break;
      if (evals) memcpy(evals + 3 * (round_base + j), e, sizeof(e));
      if (j + 1 < n) {
        rc = next(e, &ch[j]);
        r_prev = ch[j];
      }
    }
    sc_gkr_prover_destroy(pr);
    // q = W_{i+1} restricted to the line through b* and c* (:442-444), on the device table
    std::vector<u64> qv(kn + 1);
    if (rc == SC_OK) rc = sc_table_restrict_to_line(ctx, w_next, ch.data(), ch.data() + kn, kn, qv.data());
    if (rc == SC_OK && q) memcpy(q + q_base, qv.data(), (kn + 1) * sizeof(u64));
    u64 r_line = 0;
    if (rc == SC_OK) rc = next(nullptr, &r_line);   // :153
    if (rc == SC_OK) {   // r_{i+1} = l(r_line) = b* + r_line (c* - b*)  (`line`, :278-289)
      r.resize(kn);
      for (size_t j = 0; j < kn; ++j) r[j] = hf.add(ch[j], hf.mul(r_line, hf.sub(ch[kn + j], ch[j])));
    }
    round_base += n;
    q_base += kn + 1;
  }
  return rc;
}
