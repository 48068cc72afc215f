// Part of sumcheck_hip.hip (included there, in order): C ABI: transports (RCCL, host callbacks, peer).

// =====================================================================================
// C ABI: sharding
// =====================================================================================

extern "C" int sc_comm_unique_id(uint8_t id[128]) {
  std::string why;
  if (!id) return SC_ERR_ARG;
  if (!load_rccl(&why)) return fail(nullptr, SC_ERR_RCCL, "%s", why.c_str());
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId u;
  ncclResult_t r = g_rccl.GetUniqueId(&u);
  if (r != ncclSuccess) return fail(nullptr, SC_ERR_RCCL, "ncclGetUniqueId failed (%d)", (int)r);
  memcpy(id, &u, 128);
  return SC_OK;
}

static int set_world(sc_ctx* ctx, int rank, int world) {
  if (world < 1 || !is_pow2((size_t)world) || rank < 0 || rank >= world)
    return fail(ctx, SC_ERR_ARG, "rank %d / world %d: world must be a power of two", rank, world);
  if (ctx->transport != Transport::kNone) return fail(ctx, SC_ERR_STATE, "communicator already initialised");
  ctx->rank = rank;
  ctx->world = world;
  ctx->log_world = log2_of((size_t)world);
  return SC_OK;
}

extern "C" int sc_ctx_comm_init_rccl(sc_ctx* ctx, const uint8_t id[128], int rank, int world) {
  SC_NO_MULTI(ctx, "sc_ctx_comm_init_rccl");
  if (!ctx || !id) return SC_ERR_ARG;
  std::string why;
  if (!load_rccl(&why)) return fail(ctx, SC_ERR_RCCL, "%s", why.c_str());
  SC_TRY(set_device(ctx));
  SC_TRY(set_world(ctx, rank, world));
  ncclUniqueId u;
  memcpy(&u, id, 128);
  ncclResult_t r = g_rccl.CommInitRank(&ctx->comm, world, u, rank);
  if (r != ncclSuccess) {
    ctx->world = 1;
    ctx->rank = 0;
    ctx->log_world = 0;
    return fail(ctx, SC_ERR_RCCL, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  }
  ctx->transport = Transport::kRccl;
  return SC_OK;
}

extern "C" int sc_ctx_comm_init_host(sc_ctx* ctx, int rank, int world, sc_allreduce_fn allreduce,
                                     sc_allgather_fn allgather, void* user) {
  SC_NO_MULTI(ctx, "sc_ctx_comm_init_host");
  if (!ctx || !allreduce || !allgather) return SC_ERR_ARG;
  SC_TRY(set_world(ctx, rank, world));
  ctx->host_allreduce = allreduce;
  ctx->host_allgather = allgather;
  ctx->host_user = user;
  ctx->transport = Transport::kHost;
  return SC_OK;
}

extern "C" int sc_ctx_comm_peer_export(sc_ctx* ctx, int rank, int world, uint8_t handle[64]) {
  SC_NO_MULTI(ctx, "sc_ctx_comm_peer_export");
  if (!ctx || !handle) return SC_ERR_ARG;
  SC_TRY(set_device(ctx));
  if (world > sc::kMaxPeers) return fail(ctx, SC_ERR_ARG, "the peer transport serves up to %d ranks (one node)", sc::kMaxPeers);
  if (ctx->peer_region) return fail(ctx, SC_ERR_STATE, "sc_ctx_comm_peer_export: already exported");
  SC_TRY(set_world(ctx, rank, world));
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  // inbox + header + two arenas of two tables
  const size_t words = kInboxRegionWords + kPeerHeaderWords + 2 * 2 * ((size_t)world << ctx->arena_log);
  // fine-grained device memory: written by the peers over xGMI while kernels of this rank poll it
  // (no coarse-grained fallback: a peer's stores into ordinary device memory are not guaranteed to be seen by
  // this device's caches across launches; a caller without fine-grained memory uses another transport)
  hipError_t e = hipExtMallocWithFlags((void**)&ctx->peer_region, words * sizeof(u64), hipDeviceMallocFinegrained);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ctx->peer_region = nullptr;
    ctx->world = 1; ctx->rank = 0; ctx->log_world = 0;
    return fail(ctx, SC_ERR_OOM, "peer region of %zu bytes: %s", words * sizeof(u64), hipGetErrorString(e));
  }
  ctx->peer_region_words = words;
  e = hipMemset(ctx->peer_region, 0, (kInboxRegionWords + kPeerHeaderWords) * sizeof(u64));
  const u64 header[4] = {kPeerMagic, (u64)world, (u64)rank, (u64)ctx->arena_log};
  if (e == hipSuccess) e = hipMemcpy(ctx->peer_region + kInboxRegionWords, header, sizeof(header), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  hipIpcMemHandle_t h;
  if (e == hipSuccess) e = hipIpcGetMemHandle(&h, ctx->peer_region);
  if (e != hipSuccess) {
    (void)hipFree(ctx->peer_region);
    ctx->peer_region = nullptr;
    ctx->world = 1; ctx->rank = 0; ctx->log_world = 0;
    return fail(ctx, SC_ERR_HIP, "exporting the peer region: %s", hipGetErrorString(e));
  }
  memcpy(handle, &h, 64);
  ctx->peer_exported = true;
  return SC_OK;
}

// Every peer region is mapped.  Before the transport is declared usable:
//  1. each mapped region's header must name the same world and arena size and the rank it is mapped as (offsets into a
//     peer's region are computed locally);
//  2. hello: one granule into every peer's inbox; the HOST then polls its own inbox until every peer's hello is there
//     (up to peer_connect_ms).  A peer that said hello has mapped this region, loaded its code object and run a kernel,
//     so from here on the ranks are in step and the in-kernel waits can be short (peer_spin_ms);
//  3. a self-test through the real paths - an in-kernel exchange of known limbs and a gather of known words - so that a
//     node whose fine-grained memory does not behave as the kernels assume (peer stores visible to a polling kernel,
//     gathered data visible to the next launch) fails HERE, with SC_ERR_RCCL, and not inside a proof.
static int peer_finish_connect(sc_ctx* ctx) {
  for (int q = 0; q < ctx->world; ++q) {
    u64 header[4] = {0, 0, 0, 0};
    SC_HIP(ctx, hipMemcpyAsync(header, ctx->peer_base[q] + kInboxRegionWords, sizeof(header), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, sync_stream(ctx));
    if (header[0] != kPeerMagic || header[1] != (u64)ctx->world || header[2] != (u64)q || header[3] != (u64)ctx->arena_log)
      return fail(ctx, SC_ERR_ARG, "peer %d's region was exported as rank %llu of %llu with arena_log %llu (expected rank %d of %d, arena_log %d)",
                  q, (unsigned long long)header[2], (unsigned long long)header[1], (unsigned long long)header[3], q, ctx->world, ctx->arena_log);
  }
  ctx->transport = Transport::kPeer;
  // every failure from here on goes through unusable(): the context is back in the "exported, not connected" state - it
  // keeps its rank and world so that the connect can be retried, and until one succeeds every computing call on it fails
  // with SC_ERR_STATE (set_device) instead of treating its tables as shards without a data plane
  auto unusable = [ctx](int rc) {
    ctx->transport = Transport::kNone;
    return rc;
  };
  sc::PeerX px;
  for (int q = 0; q < ctx->world; ++q) px.inbox[q] = ctx->peer_base[q];
  px.world = ctx->world;
  px.rank = ctx->rank;
  hipLaunchKernelGGL(sc::peer_hello_kernel, dim3(1), dim3(sc::kWave), 0, ctx->stream, px);
  if (hipGetLastError() != hipSuccess || sync_stream(ctx) != hipSuccess)
    return unusable(fail(ctx, SC_ERR_HIP, "peer hello launch failed"));
  {
    std::vector<u64> inbox((size_t)sc::kMaxPeers * sc::kInboxWords);
    const auto t0 = std::chrono::steady_clock::now();
    while (true) {
      if (hipMemcpyAsync(inbox.data(), ctx->peer_region, (size_t)ctx->world * sc::kInboxWords * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          sync_stream(ctx) != hipSuccess)
        return unusable(fail(ctx, SC_ERR_HIP, "reading the inbox failed"));
      int missing = -1;
      for (int q = 0; q < ctx->world; ++q)
        if (inbox[(size_t)q * sc::kInboxWords + sc::kInboxHello] != (((u64)sc::kHelloTag << 32) | (u64)(q + 1))) missing = q;
      if (missing < 0) break;
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el * 1e3 > ctx->peer_connect_ms)
        return unusable(fail(ctx, SC_ERR_RCCL, "peer connect: rank %d did not say hello within %d ms", missing, ctx->peer_connect_ms));
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
  }
  // self-test 1: in-kernel exchange.  limbs (rank + 1, 7) -> totals (world (world + 1) / 2, 7 world)
  {
    const u64 mine[2] = {(u64)ctx->rank + 1, 7};
    if (hipMemcpyAsync(ctx->d_sums, mine, sizeof(mine), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      return unusable(fail(ctx, SC_ERR_HIP, "self-test upload failed"));
    u64 got = 0;
    const int keep_delay = ctx->dbg_delay_ms;
    ctx->dbg_delay_ms = 0;
    const int rc = collect_sums(ctx, 1, true, false, &got);
    ctx->dbg_delay_ms = keep_delay;
    if (rc != SC_OK) return unusable(rc == SC_ERR_STATE ? fail(ctx, SC_ERR_RCCL, "peer self-test: digest mismatch") : rc);
    HostField hf(ctx->fp);
    const u64 want = hf.recombine((u64)ctx->world * (ctx->world + 1) / 2, 7 * (u64)ctx->world);
    if (got != want) return unusable(fail(ctx, SC_ERR_RCCL, "peer self-test: the in-kernel exchange summed to the wrong value"));
  }
  // self-test 2: gather (two chunk-sized rounds, so both arenas are exercised)
  {
    const size_t len = 64;
    PoolBuf dst, src;
    int rc = src.alloc(ctx, len);
    if (rc == SC_OK) rc = dst.alloc(ctx, len * ctx->world);
    std::vector<u64> host(len * ctx->world);
    for (int round = 0; round < 2 && rc == SC_OK; ++round) {
      for (size_t i = 0; i < len; ++i) host[i] = ((u64)(ctx->rank + 1) << 32) | ((u64)round << 16) | i;
      if (hipMemcpyAsync(src, host.data(), len * sizeof(u64), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = fail(ctx, SC_ERR_HIP, "self-test upload failed");
      if (rc == SC_OK) rc = peer_gather(ctx, src, nullptr, len, dst, nullptr);
      if (rc == SC_OK && (hipMemcpyAsync(host.data(), dst, len * ctx->world * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                          sync_stream(ctx) != hipSuccess))
        rc = fail(ctx, SC_ERR_HIP, "self-test download failed");
      for (int q = 0; q < ctx->world && rc == SC_OK; ++q)
        for (size_t i = 0; i < len; ++i)
          if (host[(size_t)q * len + i] != (((u64)(q + 1) << 32) | ((u64)round << 16) | i)) {
            rc = fail(ctx, SC_ERR_RCCL, "peer self-test: gathered word %zu of rank %d is wrong", i, q);
            break;
          }
    }
    src.reset();
    dst.reset();
    if (rc != SC_OK) return unusable(rc);
  }
  return SC_OK;
}

extern "C" int sc_ctx_comm_peer_connect(sc_ctx* ctx, const uint8_t* handles) {
  SC_NO_MULTI(ctx, "sc_ctx_comm_peer_connect");
  if (!ctx || !handles) return SC_ERR_ARG;
  if (!ctx->peer_exported || ctx->transport != Transport::kNone)
    return fail(ctx, SC_ERR_STATE, "sc_ctx_comm_peer_connect: call sc_ctx_comm_peer_export first (once)");
  SC_TRY(set_device(ctx, true));
  for (int q = 0; q < ctx->world; ++q) {
    if (q == ctx->rank) {
      ctx->peer_base[q] = ctx->peer_region;
      continue;
    }
    if (ctx->peer_ipc_opened[q]) continue;   // a retried connect
    hipIpcMemHandle_t h;
    memcpy(&h, handles + 64 * (size_t)q, 64);
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(ctx, SC_ERR_HIP, "mapping rank %d's peer region: %s", q, hipGetErrorString(e));
    ctx->peer_base[q] = (u64*)p;
    ctx->peer_ipc_opened[q] = true;
  }
  return peer_finish_connect(ctx);
}

extern "C" int sc_ctx_comm_peer_connect_local(sc_ctx* ctx, sc_ctx* const* peers) {
  SC_NO_MULTI(ctx, "sc_ctx_comm_peer_connect_local");
  if (!ctx || !peers) return SC_ERR_ARG;
  if (!ctx->peer_exported || ctx->transport != Transport::kNone)
    return fail(ctx, SC_ERR_STATE, "sc_ctx_comm_peer_connect_local: call sc_ctx_comm_peer_export first (once)");
  SC_TRY(set_device(ctx, true));
  for (int q = 0; q < ctx->world; ++q) {
    const sc_ctx* pq = (q == ctx->rank) ? ctx : peers[q];
    if (!pq || !pq->peer_region || pq->world != ctx->world || pq->rank != q || pq->arena_log != ctx->arena_log)
      return fail(ctx, SC_ERR_ARG, "peer %d is not an exported context of the same world", q);
    if (pq->device != ctx->device) {
      // contexts of one process on different GPUs: this device must be allowed to reach the peer's memory
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, ctx->device, pq->device) != hipSuccess || !can)
        return fail(ctx, SC_ERR_UNSUPPORTED, "device %d cannot access device %d's memory", ctx->device, pq->device);
      const hipError_t e = hipDeviceEnablePeerAccess(pq->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
        return fail(ctx, SC_ERR_HIP, "hipDeviceEnablePeerAccess(%d): %s", pq->device, hipGetErrorString(e));
      (void)hipGetLastError();
    }
    ctx->peer_base[q] = pq->peer_region;
  }
  return peer_finish_connect(ctx);
}

extern "C" int sc_ctx_comm_rank(const sc_ctx* ctx, int* rank, int* world) {
  if (!ctx) return SC_ERR_ARG;
  if (is_multi(ctx)) {   // its tables are whole tables: one rank, however many devices stand behind it ("n_devices")
    if (rank) *rank = 0;
    if (world) *world = 1;
    return SC_OK;
  }
  if (rank) *rank = ctx->rank;
  if (world) *world = ctx->world;
  return SC_OK;
}
