// Part of sumcheck_hip.hip (included there, in order): the sums of a sharded pass across the ranks; peer gathers.

namespace {

// =====================================================================================
// 2. collectives
// =====================================================================================

// RCCL plane: the communicator is given up.  A collective whose peer is gone (a rank that died, a rank out of step) never
// completes on its own - its kernel spins on the device and everything queued behind it waits - so past "rccl_timeout_ms" the
// host aborts the communicator (which makes RCCL's kernels leave), poisons the context and reports SC_ERR_RCCL; so it does
// when RCCL itself reports an asynchronous error (a peer's socket closed, a link down).
int rccl_give_up(sc_ctx* ctx, const char* why) {
  ctx->comm_failed = true;
  poison(ctx);
  ncclComm_t comm = ctx->comm;
  ctx->comm = nullptr;
  if (comm && g_rccl.CommAbort) (void)g_rccl.CommAbort(comm);
  return fail(ctx, SC_ERR_RCCL, "RCCL plane: %s (rank %d of %d); the communicator was aborted and this context is unusable", why, ctx->rank,
              ctx->world);
}

// nullptr, or why the communicator must be given up now (called from the waits, every few thousand spins)
const char* rccl_trouble(sc_ctx* ctx, double elapsed_s) {
  if (ctx->transport != Transport::kRccl || !ctx->comm || ctx->world <= 1) return nullptr;
  if (g_rccl.CommGetAsyncError) {
    ncclResult_t st = ncclSuccess;
    if (g_rccl.CommGetAsyncError(ctx->comm, &st) == ncclSuccess && st != ncclSuccess && st != ncclInProgress)
      return g_rccl.GetErrorString ? g_rccl.GetErrorString(st) : "asynchronous error";
  }
  if (elapsed_s * 1e3 > (double)ctx->rccl_timeout_ms) return "a collective did not complete within rccl_timeout_ms (a rank is gone or out of step)";
  return nullptr;
}

// sync_stream(ctx), bounded on the RCCL plane (where a collective may be in the stream)
hipError_t sync_stream(sc_ctx* ctx) {
  if (ctx->transport != Transport::kRccl || !ctx->comm || ctx->world <= 1) return hipStreamSynchronize(ctx->stream);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  for (;;) {
    hipError_t q = hipStreamQuery(ctx->stream);
    if (q != hipErrorNotReady) return q;
    if ((++spins & 0x3F) == 0) {
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (const char* why = rccl_trouble(ctx, el)) {
        (void)rccl_give_up(ctx, why);
        (void)hipStreamSynchronize(ctx->stream);   // the aborted collective leaves the stream; what was behind it runs on garbage nobody reads
        return hipErrorLaunchFailure;
      }
      if (el > 1e-3) std::this_thread::yield();
    }
  }
}

// Spin on the mailbox sequence word the kernel writes last (system-scope release store).
int wait_mailbox(sc_ctx* ctx, u64 seq) {
  const u64* flag = ctx->h_mailbox + sc::kMailboxSeq;
  unsigned spins = 0;
  auto t0 = std::chrono::steady_clock::now();
  struct Stat {
    sc_ctx* c;
    std::chrono::steady_clock::time_point t;
    ~Stat() { c->stat_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t).count(); }
  } stat{ctx, t0};
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
    if ((++spins & 0x3FFF) == 0) {
      hipError_t q = hipStreamQuery(ctx->stream);
      if (q != hipSuccess && q != hipErrorNotReady) {
        poison(ctx);
        return fail(ctx, SC_ERR_HIP, "pass kernel failed: %s", hipGetErrorString(q));
      }
      double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (const char* why = rccl_trouble(ctx, el)) return rccl_give_up(ctx, why);
      if (q == hipSuccess && el > 2.0) {
        poison(ctx);
        return fail(ctx, SC_ERR_HIP, "pass kernel finished but its mailbox word never arrived");
      }
      // (a kernel may itself wait up to peer_spin_ms for its peers: the host must outlast it)
      if (el > 120.0 + 1e-3 * ctx->peer_spin_ms) {
        poison(ctx);
        return fail(ctx, SC_ERR_HIP, "timed out waiting for the pass kernel");
      }
    }
    __builtin_ia32_pause();
  }
  return SC_OK;
}

// First half of finishing a pass: bring its 2*ns split limbs to the host - the mailbox the kernel published to, or d_sums
// (after the all-reduce on RCCL, after a one-wave exchange kernel on the peer transport) - and point *src at them.  On
// RCCL and the peer transport they are the totals over the ranks already; on a host transport and on Transport::kLocal
// (a shard of a multi-device handle) they are THIS rank's limbs and the caller sums them.
int fetch_limbs(sc_ctx* ctx, int ns, bool across_ranks, bool from_mailbox, u64** src_out) {
  const size_t count = 2 * (size_t)ns;
  u64* src = nullptr;
  if (from_mailbox) {
    SC_TRY(wait_mailbox(ctx, ctx->mailbox_seq));
    src = ctx->h_mailbox;
    // the kernel exchanged the limbs with the peers itself; the mailbox holds the totals, or why not
    if (across_ranks && ctx->transport == Transport::kPeer) SC_TRY(check_exchange(ctx, "sums"));
  } else if (across_ranks && ctx->transport == Transport::kPeer) {
    // limbs left in d_sums by a small kernel: one wave exchanges them with the peers and publishes
    const sc::PassOut po = next_pass_out(ctx, true, 0x5c5c5c5cu + (unsigned)ns);
    const u64* limbs = ctx->d_sums;
    switch (ns) {
      case 1: hipLaunchKernelGGL((sc::peer_exchange_kernel<1>), dim3(1), dim3(sc::kWave), 0, ctx->stream, limbs, po); break;
      case 3: hipLaunchKernelGGL((sc::peer_exchange_kernel<3>), dim3(1), dim3(sc::kWave), 0, ctx->stream, limbs, po); break;
      case 9: hipLaunchKernelGGL((sc::peer_exchange_kernel<9>), dim3(1), dim3(sc::kWave), 0, ctx->stream, limbs, po); break;
      default: hipLaunchKernelGGL((sc::peer_exchange_kernel<27>), dim3(1), dim3(sc::kWave), 0, ctx->stream, limbs, po); break;
    }
    SC_HIP(ctx, hipGetLastError());
    commit_peer(ctx);
    ctx->mailbox_seq += 1;
    return fetch_limbs(ctx, ns, true, true, src_out);
  } else {
    if (across_ranks && ctx->transport == Transport::kRccl) {
      ncclResult_t r = g_rccl.AllReduce(ctx->d_sums, ctx->d_sums, count, ncclUint64, ncclSum, ctx->comm,
                                        ctx->stream);
      if (r != ncclSuccess)
        return fail(ctx, SC_ERR_RCCL, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    }
    if (ctx->use_mailbox && count <= (size_t)sc::kMailboxSeq) {
      // device -> pinned mailbox by a one-wave kernel; the host spins instead of a
      // memcpy + stream synchronise (about 8 us less per pass)
      const u64 seq = ctx->mailbox_seq + 1;
      hipLaunchKernelGGL(sc::mailbox_copy_kernel, dim3(1), dim3(sc::kWave), 0, ctx->stream, (const u64*)ctx->d_sums,
                         (int)count, ctx->d_mailbox, seq);
      SC_HIP(ctx, hipGetLastError());
      ctx->mailbox_seq = seq;
      SC_TRY(wait_mailbox(ctx, seq));
      src = ctx->h_mailbox;
    } else {
      SC_HIP(ctx, hipMemcpyAsync(ctx->h_sums, ctx->d_sums, count * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      SC_HIP(ctx, sync_stream(ctx));
      src = ctx->h_sums;
    }
  }
  *src_out = src;
  return SC_OK;
}

// Finish a pass: fetch_limbs, sum them across ranks if a host transport is installed, and recombine into ns residues.
// (Never called on a shard of a multi-device handle: its host thread sums the shards' limbs itself, engine/multi.inc.)
int collect_sums(sc_ctx* ctx, int ns, bool across_ranks, bool from_mailbox, u64* out) {
  const size_t count = 2 * (size_t)ns;
  u64* src = nullptr;
  SC_TRY(fetch_limbs(ctx, ns, across_ranks, from_mailbox, &src));
  if (across_ranks && ctx->transport == Transport::kLocal)
    return fail(ctx, SC_ERR_STATE, "a shard of a multi-device handle was asked to finish a sharded pass on its own");
  if (across_ranks && ctx->transport == Transport::kHost) {
    if (src != ctx->h_sums) {
      memcpy(ctx->h_sums, src, count * sizeof(u64));
      src = ctx->h_sums;
    }
    if (ctx->host_allreduce(ctx->host_user, src, count) != 0)
      return fail(ctx, SC_ERR_RCCL, "host all-reduce callback failed");
  }
  HostField hf(ctx->fp);
  for (int s = 0; s < ns; ++s) out[s] = hf.recombine(src[2 * s], src[2 * s + 1]);
  return SC_OK;
}

// Peer transport: all-gather `len` words per rank of two device buffers (b may be null) into dst_a / dst_b
// (world * len words each, rank order, ordinary device memory).  The peers write into this rank's arena - at most
// 2^arena_log words per rank and table at a time, longer tables go in chunks - and every chunk is copied out on the
// stream before the next gather can touch that arena: two arenas are used alternately by the parity of a dedicated
// gather counter, and a peer can only be writing gather g + 1 once this rank's kernel of gather g has flagged, which
// sits behind the copy-out of gather g - 1 (the previous user of g + 1's arena) on this stream.
int peer_gather(sc_ctx* ctx, const u64* a, const u64* b, size_t len, u64* dst_a, u64* dst_b) {
  const size_t chunk_cap = (size_t)1 << ctx->arena_log;         // words per rank, table and chunk
  const size_t cap = (size_t)ctx->world << ctx->arena_log;      // words per table of an arena
  for (size_t off = 0; off < len; off += chunk_cap) {
    const size_t n = std::min(chunk_cap, len - off);
    const sc::PassOut out = next_pass_out(ctx, true, 0);
    const size_t arena_off = kInboxRegionWords + kPeerHeaderWords + (size_t)(ctx->gather_count & 1u) * 2 * cap;
    sc::PeerG pg;
    for (int q = 0; q < ctx->world; ++q) pg.arena[q] = ctx->peer_base[q] + arena_off;
    pg.table_stride = cap;
    const int grid = (int)std::min<size_t>(std::max<size_t>((n / 2 + sc::kBlock - 1) / sc::kBlock, 1), 256);
    hipLaunchKernelGGL(sc::peer_gather_kernel, dim3(grid), dim3(sc::kBlock), 0, ctx->stream, a + off, (b ? b : a) + off, n, pg, out);
    SC_HIP(ctx, hipGetLastError());
    commit_peer(ctx);
    ctx->gather_count += 1;
    ctx->mailbox_seq += 1;
    if (grid > 1) ctx->ticket_base += (unsigned)grid;
    SC_TRY(wait_mailbox(ctx, ctx->mailbox_seq));
    if (__atomic_load_n(ctx->h_mailbox + sc::kMailboxErr, __ATOMIC_ACQUIRE) != 0) {
      poison(ctx);
      return fail(ctx, SC_ERR_RCCL, "peer gather: a rank's tables did not arrive within %d ms", ctx->peer_spin_ms);
    }
    // arena rows [rank][n] -> dst rows [rank][len] at column `off`
    const u64* src = ctx->peer_base[ctx->rank] + arena_off;
    SC_HIP(ctx, hipMemcpy2DAsync(dst_a + off, len * sizeof(u64), src, n * sizeof(u64), n * sizeof(u64), (size_t)ctx->world,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    if (b && dst_b)
      SC_HIP(ctx, hipMemcpy2DAsync(dst_b + off, len * sizeof(u64), src + cap, n * sizeof(u64), n * sizeof(u64), (size_t)ctx->world,
                                   hipMemcpyDeviceToDevice, ctx->stream));
  }
  return SC_OK;
}

// All-gather `len` words per rank of a device buffer into a new pool buffer of len*world.
int gather_table(sc_ctx* ctx, const u64* local, size_t len, PoolBuf* out_full) {
  PoolBuf full;
  SC_TRY(full.alloc(ctx, len * ctx->world));
  if (ctx->transport == Transport::kPeer) {
    SC_TRY(peer_gather(ctx, local, nullptr, len, full, nullptr));
  } else if (ctx->transport == Transport::kRccl) {
    ncclResult_t r = g_rccl.AllGather(local, full, len, ncclUint64, ctx->comm, ctx->stream);
    if (r != ncclSuccess) return fail(ctx, SC_ERR_RCCL, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  } else {
    if (!ctx->host_allgather) return fail(ctx, SC_ERR_STATE, "gather_table: no host collectives installed on this context");
    std::vector<u64> send(len), recv(len * ctx->world);
    SC_HIP(ctx, hipMemcpyAsync(send.data(), local, len * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, sync_stream(ctx));
    if (ctx->host_allgather(ctx->host_user, send.data(), recv.data(), len) != 0)
      return fail(ctx, SC_ERR_RCCL, "host all-gather callback failed");
    SC_HIP(ctx, hipMemcpyAsync(full, recv.data(), recv.size() * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, sync_stream(ctx));
  }
  *out_full = std::move(full);
  return SC_OK;
}

// Sum `count` u64 words of a device buffer across ranks, in place (values are 32-bit limbs).
int allreduce_device(sc_ctx* ctx, u64* buf, size_t count) {
  if (ctx->transport == Transport::kPeer) {
    // gather every rank's vector, then sum the rows locally (plain u64 adds of limbs)
    PoolBuf all;   // (given back on return: stream-ordered reuse)
    SC_TRY(all.alloc(ctx, count * ctx->world));
    SC_TRY(peer_gather(ctx, buf, nullptr, count, all, nullptr));
    hipLaunchKernelGGL(sc::sum_limb_rows_kernel, dim3(grid_for(ctx, count)), dim3(sc::kBlock), 0, ctx->stream, (const u64*)all, ctx->world,
                       count, buf);
    if (hipGetLastError() != hipSuccess) return fail(ctx, SC_ERR_HIP, "sum_limb_rows_kernel launch failed");
    return SC_OK;
  }
  if (ctx->transport == Transport::kRccl) {
    ncclResult_t r = g_rccl.AllReduce(buf, buf, count, ncclUint64, ncclSum, ctx->comm, ctx->stream);
    if (r != ncclSuccess)
      return fail(ctx, SC_ERR_RCCL, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    return SC_OK;
  }
  if (!ctx->host_allreduce) return fail(ctx, SC_ERR_STATE, "allreduce_device: no host collectives installed on this context");
  std::vector<u64> host(count);
  SC_HIP(ctx, hipMemcpyAsync(host.data(), buf, count * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  if (ctx->host_allreduce(ctx->host_user, host.data(), count) != 0)
    return fail(ctx, SC_ERR_RCCL, "host all-reduce callback failed");
  SC_HIP(ctx, hipMemcpyAsync(buf, host.data(), count * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
  SC_HIP(ctx, sync_stream(ctx));
  return SC_OK;
}

}  // namespace
