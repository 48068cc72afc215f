// Part of sumcheck_hip.hip (included there, in order): launch helpers: grids, pass / grid-pass / rank-pass launches, the hand-off to the host mailbox.

namespace {

// =====================================================================================
// 3. launch helpers
// =====================================================================================

#define SC_DISPATCH_FIELD(ctx, F, f, ...)      \
  do {                                         \
    if ((ctx)->gold) {                         \
      typedef sc::GoldilocksMont F;            \
      F f((ctx)->fp);                          \
      __VA_ARGS__;                             \
    } else {                                   \
      typedef sc::MontGeneric F;               \
      F f((ctx)->fp);                          \
      __VA_ARGS__;                             \
    }                                          \
  } while (0)

// The one way a run-time choice (a streaming flag, ks, a (kf, ks) shape) becomes a template argument of a kernel:
// fn(std::integral_constant<int, V>) for the V of Vs equal to v.  Only the listed values are instantiated; any other v calls
// nothing.
template <int V>
using IntC = std::integral_constant<int, V>;
template <int... Vs, class Fn>
void with_const(int v, Fn&& fn) {
  (void)((v == Vs && (fn(IntC<Vs>{}), true)) || ...);
}
template <class Fn>
void with_bool(bool b, Fn&& fn) {
  if (b) fn(std::true_type{});
  else fn(std::false_type{});
}
// fn(KF, KS) for the (kf, ks) shapes pass_kernel is instantiated for (launch_pass admits exactly these)
template <class Fn>
void with_pass_shape(int kf, int ks, Fn&& fn) {
  with_const<0 * 4 + 1, 0 * 4 + 2, 0 * 4 + 3, 1 * 4 + 1, 1 * 4 + 2, 2 * 4 + 1, 2 * 4 + 2, 3 * 4 + 1, 3 * 4 + 2, 4 * 4 + 2>(
      kf * 4 + ks, [&](auto c) { fn(IntC<c / 4>{}, IntC<c % 4>{}); });
}

// w[c] = prod_j (bit_j(c) ? r[j] : 1 - r[j]), c < 2^kf: the weights of a kf-challenge fold, as sc::FoldW (kernels.hpp, kf <= 4)
// or sc::GridW (kernels/grid_pass.hpp, kf <= 5)
template <class W>
W make_weights(const sc_ctx* ctx, const u64* r, int kf) {
  HostField hf(ctx->fp);
  W out;
  for (u64& w : out.w) w = 0;
  out.w[0] = hf.one();
  for (int j = 0; j < kf; ++j) {
    const int half = 1 << j;
    for (int c = half - 1; c >= 0; --c) {
      const u64 base = out.w[c];
      out.w[c + half] = hf.mul(base, r[j]);
      out.w[c] = hf.mul(base, hf.sub(hf.one(), r[j]));
    }
  }
  return out;
}

// 3^k: the cells of a pass that serves k rounds
inline int pow3(int k) {
  int c = 1;
  while (k-- > 0) c *= 3;
  return c;
}

// (H(0), H(1), H(inf)) -> H(2) = 2 H(1) - H(0) + 2 H(inf)   (H quadratic, inf = leading coefficient)
u64 eval2_from_inf(const HostField& hf, u64 e0, u64 e1, u64 einf) {
  u64 t = hf.add(e1, einf);
  return hf.sub(hf.add(t, t), e0);
}

// the synthetic challenger of a call with draw == NULL: word `index` of the sequence under seed_r, a Montgomery word (a challenge
// of two words takes the indices 2 i and 2 i + 1)
u64 seeded_challenge(const sc_ctx* ctx, const HostField& hf, u64 seed_r, u64 index) {
  return hf.mul(sc::splitmix64(seed_r + index + 1) % ctx->fp.p, ctx->fp.r2_mod_p);
}

// add the durations of the recorded launches to the totals (waits for the last of them)
void drain_kernel_timers(sc_ctx* ctx) {
  if (ctx->kt_used == 0) return;
  (void)hipEventSynchronize(ctx->kt_ev[ctx->kt_used - 1][1]);
  for (int i = 0; i < ctx->kt_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->kt_ev[i][0], ctx->kt_ev[i][1]) == hipSuccess) {
      ctx->kt_ms += ms;
      ctx->kt_n += 1;
      if (ctx->launch_log.size() < sc_ctx::kLaunchLogCap) {
        sc_launch_record r = ctx->kt_meta[i];
        r.ms = ms;
        ctx->launch_log.push_back(r);
      }
    }
  }
  ctx->kt_used = 0;
}

// Bracket the launch(es) that follow with an event pair on the context's stream (option
// "time_kernels"); bytes_read / bytes_written are what the launch has to move through HBM (every
// input once, every output once).  timer_end() after the launch.
int timer_begin(sc_ctx* ctx, int kind, int kf, int ks, int log_in, u64 bytes_read, u64 bytes_written) {
  if (!ctx->time_kernels) return SC_OK;
  if (ctx->kt_used == sc_ctx::kTimerRing) drain_kernel_timers(ctx);
  sc_launch_record& m = ctx->kt_meta[ctx->kt_used];
  m.kind = kind;
  m.kf = kf;
  m.ks = ks;
  m.log_in = log_in;
  m.bytes_read = bytes_read;
  m.bytes_written = bytes_written;
  m.ms = 0.0;
  SC_HIP(ctx, hipEventRecord(ctx->kt_ev[ctx->kt_used][0], ctx->stream));
  return SC_OK;
}
int timer_end(sc_ctx* ctx) {
  if (!ctx->time_kernels) return SC_OK;
  SC_HIP(ctx, hipEventRecord(ctx->kt_ev[ctx->kt_used][1], ctx->stream));
  ctx->kt_used += 1;
  return SC_OK;
}

// The resident grid of a kernel at a block size: blocks per CU x CUs, asked once per context (prewarm asks ahead of the first
// proof); `fallback` where the runtime cannot tell.  The callers cap it as their launches need.
int resident_grid(sc_ctx* ctx, const void* fn, int block, int fallback) {
  int& slot = ctx->resident_grid[fn];
  if (slot == 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, 0) != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      slot = fallback;
    } else {
      slot = per_cu * ctx->num_cus;
    }
  }
  return slot;
}
template <class K>
const void* kernel_ptr(K* k) {
  return reinterpret_cast<const void*>(k);
}

// A pass is launched with at most as many blocks as are resident at once (occupancy x CUs) and
// grid-strides over the rest: with 4x more blocks than fit (the old fixed cap of 2048) the chip
// drains and refills between block generations and the last block has 4x more partial sums to
// reduce - 7 % of an n = 28 proof (measured with the max_blocks option: 2048 -> 2.31 ms,
// 1024 -> 2.20, 512 -> 2.13, 256 -> 2.27).
int pass_resident_blocks(sc_ctx* ctx, int kf, int ks) {
  const void* fn = nullptr;
  SC_DISPATCH_FIELD(ctx, F, f, (void)f; with_pass_shape(kf, ks, [&](auto KF, auto KS) { fn = kernel_ptr(&sc::pass_kernel<F, KF, KS, 1>); }));
  return fn ? resident_grid(ctx, fn, sc::pass_block_threads(kf, ks), ctx->max_blocks) : ctx->max_blocks;
}

// the pipelined whole-tile form of the three-variable fold (pass_kernel<F, 3, 2, NT | 4>): its own block size and occupancy
int pipe32_resident_blocks(sc_ctx* ctx) {
  const void* fn = ctx->gold ? kernel_ptr(&sc::pass_kernel<sc::GoldilocksMont, 3, 2, 5>) : kernel_ptr(&sc::pass_kernel<sc::MontGeneric, 3, 2, 5>);
  return resident_grid(ctx, fn, sc::kPipe32Threads, ctx->num_cus);
}

template <class F>
void launch_pass_t(sc_ctx* ctx, const F& f, int kf, int ks, const u64* A, const u64* B, u64* A2,
                   u64* B2, const sc::FoldW& fw, size_t n_units, int grid, int log_in, const sc::PassOut& out, bool pipe32) {
  dim3 g(grid), b(sc::pass_block_threads(kf, ks, pipe32 ? 4 : 0));
  hipStream_t s = ctx->stream;
  // streaming hints are compile-time (kernels.hpp, ld16/st16): 0 = cached, 1 = stream the inputs,
  // 3 = stream inputs and outputs; FORM adds 4 (the pipelined form) or 8 (the LDS-DMA form)
  const int nt = (log_in >= ctx->nt_load_log ? 1 : 0) | ((kf > 0 && (log_in - kf) >= ctx->nt_store_log) ? 2 : 0);
  auto go = [&](auto KF, auto KS, auto FORM) {
    with_const<3, 1, 0>(nt == 3 ? 3 : nt & 1, [&](auto NT) {
      hipLaunchKernelGGL((sc::pass_kernel<F, KF, KS, FORM | NT>), g, b, 0, s, f, A, B, A2, B2, fw, n_units, out);
    });
  };
  if constexpr (std::is_same<F, sc::GoldilocksMont>::value) {
    // the LDS-DMA form of the four-variable fold (whole tiles: launch_pass checks).  Goldilocks only: with the generic field's
    // constants in registers the form does not fit 256 VGPRs (20 bytes of scratch), and that field keeps the register-staged one
    if (kf == 4 && ks == 2 && ctx->fold_dma) return go(IntC<4>{}, IntC<2>{}, IntC<8>{});
  }
  if (pipe32) return go(IntC<3>{}, IntC<2>{}, IntC<4>{});   // (kf, ks) = (3, 2), whole tiles
  with_pass_shape(kf, ks, [&](auto KF, auto KS) { go(KF, KS, IntC<0>{}); });
}

constexpr size_t kInboxRegionWords = 2 * (size_t)sc::kMaxPeers * sc::kInboxWords;   // two parities
// a rank's exported region: [inbox (two parities) | header | two gather arenas of two tables].  The header lets a peer
// check, when it maps the region, that both sides compute the same offsets: {magic, world, rank, arena_log}
constexpr size_t kPeerHeaderWords = 8;
constexpr u64 kPeerMagic = 0x7363706565723033ull;   // "scpeer03"

// 32-bit digest of what a sharded pass folds: identical on every rank unless the ranks were fed
// different challenges (FNV-1a over the words)
unsigned challenge_digest(const u64* r, int kf, int ks, int log_in) {
  u64 h = 0xcbf29ce484222325ull;
  auto mix = [&h](u64 v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (v >> (8 * i)) & 0xFF;
      h *= 0x100000001b3ull;
    }
  };
  mix((u64)kf | ((u64)ks << 8) | ((u64)log_in << 16));
  for (int i = 0; i < kf; ++i) mix(r[i]);
  return (unsigned)(h ^ (h >> 32));
}

// Exchange fields of a sharded launch on the peer transport.  The tag advances with every such launch, in the
// same order on every rank - but only once the launch is known to be in the stream (commit_peer): a launch that
// failed locally must not leave this rank one tag ahead of its peers.
void fill_peer(sc_ctx* ctx, sc::PeerX& px, unsigned digest) {
  for (int q = 0; q < ctx->world; ++q) px.inbox[q] = ctx->peer_base[q];
  px.world = ctx->world;
  px.rank = ctx->rank;
  unsigned tag = ctx->xchg_tag + 1;
  if (ctx->dbg_skip_tag) {   // fault injection: this rank falls out of step
    tag += 1;
    ctx->dbg_skip_tag = 0;
  }
  if (tag == 0) tag = 1;
  ctx->xchg_next = tag;
  px.tag = tag;
  px.digest = digest;
  px.spin_ticks = (u64)ctx->peer_spin_ms * 100000ull;   // wall_clock64 runs at 100 MHz
  if (ctx->dbg_delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(ctx->dbg_delay_ms));   // fault injection: a late rank
}
inline void commit_peer(sc_ctx* ctx) {
  if (ctx->xchg_next) ctx->xchg_tag = ctx->xchg_next;
  ctx->xchg_next = 0;
}

// PassOut of the next launch that ends in finish_pass.  across_ranks: its sums are summed over the ranks - inside the
// kernel on the peer transport (digest = what the ranks must agree on), by a collective on the stream for RCCL (the
// limbs stay in d_sums), by the host for a host transport.  *from_mailbox tells collect_sums where the limbs are.
// Nothing is committed here: call commit_pass_out() once the launch is known to be in the stream.
sc::PassOut next_pass_out(sc_ctx* ctx, bool across_ranks = false, unsigned digest = 0, bool* from_mailbox = nullptr) {
  const bool peer = across_ranks && ctx->transport == Transport::kPeer;
  const bool mailbox = (ctx->use_mailbox || peer) && !(across_ranks && ctx->transport == Transport::kRccl);
  sc::PassOut out;
  out.partials = ctx->d_partials;
  out.n_rows = (int)ctx->partial_rows;
  out.ticket = ctx->d_ticket;
  out.ticket_base = ctx->ticket_base;
  out.sums_dev = ctx->d_sums;
  out.mailbox = mailbox ? ctx->d_mailbox : nullptr;
  out.seq = mailbox ? ctx->mailbox_seq + 1 : 0;
  if (peer) fill_peer(ctx, out.px, digest);
  if (from_mailbox) *from_mailbox = mailbox;
  return out;
}
int commit_pass_out(sc_ctx* ctx, const sc::PassOut& out, int grid) {
  SC_HIP(ctx, hipGetLastError());
  if (out.px.world > 0) commit_peer(ctx);
  if (out.mailbox) ctx->mailbox_seq += 1;
  if (grid > 1) ctx->ticket_base += (unsigned)grid;
  return SC_OK;
}

// WgOut of the next launch that leaves its cells in the wide mailbox (collect_grid).  tables: the kernel hands its partial
// rows over through the grid-pass partials, group rows and tickets; host_out: its folded tables go to the pinned tail buffer.
// across_ranks: the peer transport exchanges the cells inside the kernel (digest: salted per kind of pass), RCCL sums their
// limbs behind it (commit_wide_out), a host transport gets this rank's residues and sums them itself.  Nothing is committed
// here: call commit_wide_out() right after the launch.
sc::WgOut next_wide_out(sc_ctx* ctx, bool across_ranks, unsigned digest, bool tables, bool host_out) {
  sc::WgOut wo;
  wo.partials = tables ? ctx->d_wg_partials : nullptr;
  wo.group_rows = tables ? ctx->d_wg_groups : nullptr;
  wo.tickets = tables ? ctx->d_wg_tickets : nullptr;
  wo.mailbox = ctx->d_mailbox;
  wo.seq = ctx->mailbox_seq + 1;
  wo.limbs_dev = across_ranks && ctx->transport == Transport::kRccl ? ctx->d_sums : nullptr;
  wo.host_out = host_out ? 1 : 0;
  if (across_ranks && ctx->transport == Transport::kPeer) fill_peer(ctx, wo.px, digest);
  return wo;
}
// the launch is in the stream: only now do the exchange tag and the mailbox sequence move.  On RCCL the cells' 2 x cells limbs
// are summed on the stream behind the kernel and a small kernel hands the totals to the mailbox under the launch's sequence word.
int commit_wide_out(sc_ctx* ctx, const sc::WgOut& wo, int cells) {
  SC_HIP(ctx, hipGetLastError());
  if (wo.px.world > 0) commit_peer(ctx);
  SC_TRY(timer_end(ctx));
  if (wo.limbs_dev) {
    ncclResult_t nr = g_rccl.AllReduce(ctx->d_sums, ctx->d_sums, 2 * (size_t)cells, ncclUint64, ncclSum, ctx->comm, ctx->stream);
    if (nr != ncclSuccess) return fail(ctx, SC_ERR_RCCL, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(nr) : "?");
    hipLaunchKernelGGL(sc::mailbox_copy_wide_kernel, dim3(1), dim3(sc::kBlock), 0, ctx->stream, (const u64*)ctx->d_sums, 2 * cells,
                       ctx->d_mailbox, wo.seq);
    SC_HIP(ctx, hipGetLastError());
  }
  ctx->mailbox_seq += 1;
  return SC_OK;
}

// the pinned tail buffer: a pass's outputs there are read by the host (option "host_tail_log")
bool in_tail(const sc_ctx* ctx, const u64* p) { return p && ctx->d_tail && p >= ctx->d_tail && p < ctx->d_tail + kTailSlots * kTailSlotWords; }

// Launch one pass over tables of 2^log_in entries.  The 2*NS split limbs end up in the
// host mailbox (*from_mailbox = true; wait with collect_sums) or in ctx->d_sums when they
// still have to be all-reduced on the device (RCCL transport).
int launch_pass(sc_ctx* ctx, int kf, int ks, const u64* A, const u64* B, u64* A2, u64* B2, const u64* r,
                int log_in, bool across_ranks, bool* from_mailbox) {
  if (kf < 0 || kf > 4 || ks < 1 || ks > 3 || (ks == 3 && kf != 0) || (kf == 4 && (ks != 2 || log_in < 12)) || log_in < kf + ks)
    return fail(ctx, SC_ERR_ARG, "launch_pass: kf=%d ks=%d log_in=%d", kf, ks, log_in);
  const sc::FoldW fw = make_weights<sc::FoldW>(ctx, r, kf);
  size_t n_units = (size_t)1 << (log_in - kf - ks);
  // the three-variable fold on whole tiles of a large table: the pipelined form (kernels/pass.hpp)
  const bool pipe32 = kf == 3 && ks == 2 && ctx->pipe32 && n_units % sc::kWave == 0 && log_in >= ctx->pipe32_log;
  const size_t bs = (size_t)sc::pass_block_threads(kf, ks, pipe32 ? 4 : 0);
  int grid = (int)std::min<size_t>(std::max<size_t>((n_units + bs - 1) / bs, 1), (size_t)ctx->max_blocks);
  grid = std::min(grid, pipe32 ? pipe32_resident_blocks(ctx) : pass_resident_blocks(ctx, kf, ks));
  // A pass_kernel launch stores its folded tables with plain stores.  The host may read them (tables in the pinned tail buffer,
  // option "host_tail_log") only where that is safe: one block, one wave's worth of outputs - finish_pass drains wave 0 before the
  // sequence word leaves, nobody else has stored.  The planner hands over from pass_kernel only at <= 2^kTailSmallLog entries;
  // this is where that invariant is checked instead of assumed (ADVICE r05): anything larger must go through wgrid_pass_kernel,
  // whose hand-over is write-through at system scope (WgOut::host_out)
  if (kf > 0 && in_tail(ctx, A2) && (grid != 1 || ((size_t)1 << (log_in - kf)) > (size_t)sc::kWave))
    return fail(ctx, SC_ERR_STATE, "launch_pass: a pass_kernel launch of %d blocks would hand 2^%d-entry tables to the host with plain stores", grid,
                log_in - kf);
  const sc::PassOut out = next_pass_out(ctx, across_ranks, challenge_digest(r, kf, ks, log_in), from_mailbox);
  SC_TRY(timer_begin(ctx, SC_KIND_PASS, kf, ks, log_in, (u64)16 << log_in, kf > 0 ? (u64)16 << (log_in - kf) : 0));
  SC_DISPATCH_FIELD(ctx, F, f, launch_pass_t<F>(ctx, f, kf, ks, A, B, A2, B2, fw, n_units, grid, log_in, out, pipe32));
  // the launch is in the stream: only now do the ticket base, the mailbox sequence and the exchange tag move (a
  // failed launch must leave them where the device-side counter and the peers still are)
  SC_TRY(commit_pass_out(ctx, out, grid));
  SC_TRY(timer_end(ctx));
  return SC_OK;
}

int wait_mailbox(sc_ctx* ctx, u64 seq);

// after the sequence word of a launch that exchanged with the peers: did the exchange succeed?
int check_exchange(sc_ctx* ctx, const char* what) {
  const u64 err = __atomic_load_n(ctx->h_mailbox + sc::kMailboxErr, __ATOMIC_ACQUIRE);
  if (err == 0) return SC_OK;
  if (err & (u64)sc::kXchgTimeout) {
    poison(ctx);
    return fail(ctx, SC_ERR_RCCL, "peer exchange: a rank's %s did not arrive within %d ms (rank %d waited for rank %d at tag %u; that rank's "
                "slot held tag ..%04x)", what, ctx->peer_spin_ms, ctx->rank, (int)((err >> 8) & 0xFF), ctx->xchg_tag, (unsigned)((err >> 16) & 0x3FFF));
  }
  return fail(ctx, SC_ERR_STATE, "the ranks of this sharded prover were given different challenges");
}

// One pass by wgrid_pass_kernel: folds kf <= 5 pending challenges of tables of 2^log_in entries and leaves the 3^ks
// cells of the next ks <= 5 rounds in the wide mailbox (collect_grid).  Its counters rest at zero.  Sharded passes hand
// their cells over as next_wide_out describes.
int launch_grid_pass(sc_ctx* ctx, int kf, int ks, const u64* A, const u64* B, u64* A2, u64* B2, const u64* r, int log_in, bool across_ranks) {
  if (kf < 0 || kf > sc::kGridMaxVars || ks < 1 || ks > sc::kGridMaxVars || log_in < kf + ks)
    return fail(ctx, SC_ERR_ARG, "launch_grid_pass: kf=%d ks=%d log_in=%d", kf, ks, log_in);
  if (!ctx->use_mailbox) return fail(ctx, SC_ERR_STATE, "launch_grid_pass needs the host mailbox");
  const sc::GridW gw = make_weights<sc::GridW>(ctx, r, kf);
  const size_t n_out = (size_t)1 << (log_in - kf);
  const int resident = std::min(resident_grid(ctx, ctx->gold ? kernel_ptr(&sc::wgrid_pass_kernel<sc::GoldilocksMont, 5, false>)
                                                             : kernel_ptr(&sc::wgrid_pass_kernel<sc::MontGeneric, 5, false>),
                                              sc::kBlock, 2 * ctx->num_cus),
                                kWgMaxBlocks);
  constexpr size_t kWaves = sc::kBlock / sc::kWave;
  const size_t n_iter = (n_out + sc::kWgEntries - 1) / sc::kWgEntries;   // one per wave
  const size_t cap = ctx->grid_blocks > 0 ? (size_t)std::min(ctx->grid_blocks, resident) : (size_t)resident;
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((n_iter + kWaves - 1) / kWaves, cap));
  // outputs in the pinned tail buffer (the host finishes from them): stored write-through at system scope (WgOut::host_out)
  const sc::WgOut wo = next_wide_out(ctx, across_ranks, challenge_digest(r, kf, ks, log_in), true, in_tail(ctx, A2));
  SC_TRY(timer_begin(ctx, SC_KIND_GRID_PASS, kf, ks, log_in, (u64)16 << log_in, kf > 0 ? (u64)16 << (log_in - kf) : 0));
  // the prefetching instantiation: fan-ins 0 and 2 on tables that give a wave more than one iteration (kernels.hpp)
  const bool pf = (kf == 0 || kf == 2) && n_iter > (size_t)grid * kWaves;
  SC_DISPATCH_FIELD(ctx, F, f, with_bool(pf, [&](auto PF) {
    with_const<1, 2, 3, 4, 5>(ks, [&](auto KS) {
      hipLaunchKernelGGL((sc::wgrid_pass_kernel<F, KS, PF>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f, A, B, A2, B2, gw, kf, n_out, wo);
    });
  }));
  return commit_wide_out(ctx, wo, pow3(ks));
}
// wfold_pass_kernel (kernels/grid_pass.hpp): folds kf = 4 or 5 pending challenges of LARGE tables of 2^log_in entries (whole
// tiles: log_in >= 12) into A2 / B2 and leaves the 3^ks cells of the next ks rounds exactly as launch_grid_pass does
// (collect_grid(ctx, ks, across_ranks, .)).  Instantiated for (4, 5) - the fold behind the matrix-core first pass - and
// (5, 3..5) - the pass behind that on the largest tables; wfold_has() tells the planner.
bool wfold_has(int kf, int ks) { return (kf == 4 && ks == 5) || (kf == 5 && ks >= 3 && ks <= 5); }
// its resident grid: one block per CU
int wfold_resident_blocks(sc_ctx* ctx) {
  const void* fn = ctx->gold ? kernel_ptr(&sc::wfold_pass_kernel<sc::GoldilocksMont, 4, 5, true>)
                             : kernel_ptr(&sc::wfold_pass_kernel<sc::MontGeneric, 4, 5, true>);
  return std::min(resident_grid(ctx, fn, sc::kWfThreads, ctx->num_cus), kWgMaxBlocks);
}
int launch_wfold_pass(sc_ctx* ctx, int kf, int ks, const u64* A, const u64* B, u64* A2, u64* B2, const u64* r, int log_in, bool across_ranks) {
  if (log_in < 12 || !A2 || !B2 || !wfold_has(kf, ks)) return fail(ctx, SC_ERR_ARG, "launch_wfold_pass: kf=%d ks=%d log_in=%d", kf, ks, log_in);
  if (!ctx->use_mailbox) return fail(ctx, SC_ERR_STATE, "launch_wfold_pass needs the host mailbox");
  const sc::FoldW fw = make_weights<sc::FoldW>(ctx, r, 4);   // (the fifth challenge rides alone: out = h0 + r_5 (h1 - h0))
  const u64 r_top = kf == 5 ? r[4] : 0;
  const size_t n_tiles = (size_t)1 << (log_in - 12);
  const int grid = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n_tiles, (size_t)wfold_resident_blocks(ctx)), (size_t)ctx->max_blocks));
  const sc::WgOut wo = next_wide_out(ctx, across_ranks, challenge_digest(r, kf, ks, log_in) ^ 0x77666f6cu, true, false);
  SC_TRY(timer_begin(ctx, SC_KIND_WFOLD_PASS, kf, ks, log_in, (u64)16 << log_in, (u64)16 << (log_in - kf)));
  // the clock-aligned write slots (options "wfold_slot_*"): period 0 launches the kernel without them.  By default (-1) where they
  // were measured to pay - the four-challenge fold of tables of >= 2^25 entries, a 6 us slot every 24 us (one tile per wave and
  // period): 779 -> 734 us at 2^28, 112 -> 109 at 2^25, the staggered twin 796 / 115 (profiles/wfold_slots_sweep.txt); the (5, 3)
  // form at 2^24, two tiles per wave, gains nothing (57.1 -> 56.9 us) and stays without
  sc::WfSlots sl;
  if (ctx->wfold_slot_period < 0) {
    sl.period = (kf == 4 && log_in >= 25) ? 2400u : 0u;
    sl.width = 600u;
  } else {
    sl.period = (unsigned)ctx->wfold_slot_period;
    sl.width = (unsigned)ctx->wfold_slot_width;
    sl.stagger = (unsigned)ctx->wfold_slot_stagger;
  }
  SC_DISPATCH_FIELD(ctx, F, f, with_bool(log_in >= ctx->nt_load_log, [&](auto NT) {
    with_bool(sl.period != 0, [&](auto SLOTS) {
      auto go = [&](auto KF, auto KS) {
        hipLaunchKernelGGL((sc::wfold_pass_kernel<F, KF, KS, NT, SLOTS>), dim3(grid), dim3(sc::kWfThreads), 0, ctx->stream, f, A, B, A2, B2, fw, r_top,
                           n_tiles, wo, sl);
      };
      if (kf == 4) go(IntC<4>{}, IntC<5>{});
      else with_const<3, 4, 5>(ks, [&](auto KS) { go(IntC<5>{}, KS); });
    });
  }));
  return commit_wide_out(ctx, wo, pow3(ks));
}

// The four-round first pass of a large proof (kernels/gram.hpp): gram_pass_kernel accumulates the exact limb products of the
// Gram matrix of the tables' sixteen slices on the int8 matrix cores, every block reduces what it holds to the 81 cells of
// rounds 1..4 mod p, and the block that finishes last adds the blocks' rows and leaves the cells in the wide mailbox exactly as a
// grid pass does (collect_grid(ctx, 4, false, .)).  ONE launch since round 5 (the int32 partials and gram_finish_kernel are gone).
constexpr int kGramK = 4;
constexpr int kGramMaxBlocks = 1024;
// first use on this context: the hand-off rows + the ticket (zero at rest), and the kernels' dynamic LDS.  Nothing is left
// half-initialised if a step fails (ADVICE r04): the pointer is published only when rows, ticket and attributes are in place.
int gram_workspace(sc_ctx* ctx) {
  if (ctx->d_gram_rows) return SC_OK;
  const size_t bytes = (size_t)kGramMaxBlocks * sc::kGramRowWords * sizeof(u64) + 64;
  u64* p = nullptr;
  SC_HIP(ctx, hipMalloc(&p, bytes));
  hipError_t e = hipMemsetAsync(p, 0, bytes, ctx->stream);
  const int lds = sc::kGramStages * sc::kGramStageBytes;
  const void* fns[4] = {reinterpret_cast<const void*>(&sc::gram_pass_kernel<sc::GoldilocksMont, kGramK, true>),
                        reinterpret_cast<const void*>(&sc::gram_pass_kernel<sc::GoldilocksMont, kGramK, false>),
                        reinterpret_cast<const void*>(&sc::gram_pass_kernel<sc::MontGeneric, kGramK, true>),
                        reinterpret_cast<const void*>(&sc::gram_pass_kernel<sc::MontGeneric, kGramK, false>)};
  for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) {
    (void)hipFree(p);
    SC_HIP(ctx, e);
  }
  ctx->d_gram_rows = p;
  return SC_OK;
}
int launch_gram_pass(sc_ctx* ctx, const u64* A, const u64* B, int log_in, bool across_ranks) {
  typedef sc::GramGeo<kGramK> G;
  if (!ctx->use_mailbox) return fail(ctx, SC_ERR_STATE, "launch_gram_pass needs the host mailbox");
  const size_t len = (size_t)1 << log_in;
  if (len < (size_t)G::kEntriesPerStep * sc::kGramStages) return fail(ctx, SC_ERR_ARG, "launch_gram_pass: 2^%d entries are too few", log_in);
  const size_t n_steps = len / G::kEntriesPerStep;
  // partials: a power of two - one per block while the tables are small, more once a block's share passes the 2^16 rows an
  // int32 accumulator takes; each is a multiple of kGramStages steps
  size_t blocks = 1;
  while (blocks * 2 <= (size_t)std::min(std::min(ctx->num_cus, ctx->max_blocks), kGramMaxBlocks)) blocks *= 2;
  size_t n_partials = std::min(blocks, n_steps / sc::kGramStages);
  while (n_steps / n_partials > (size_t)G::kMaxSteps) n_partials *= 2;
  const size_t spp = n_steps / n_partials;
  const int grid = (int)std::min(blocks, n_partials);
  SC_TRY(gram_workspace(ctx));
  // the cells leave as a grid pass's do (next_wide_out; a multi-device handle sums the shards' residues on the host)
  const sc::WgOut wo = next_wide_out(ctx, across_ranks, challenge_digest(nullptr, 0, kGramK, log_in) ^ 0x6772616du, false, false);
  unsigned* ticket = reinterpret_cast<unsigned*>(ctx->d_gram_rows + (size_t)kGramMaxBlocks * sc::kGramRowWords);
  SC_TRY(timer_begin(ctx, SC_KIND_GRAM_PASS, 0, kGramK, log_in, (u64)16 << log_in, (u64)grid * sc::kGramRowWords * sizeof(u64)));
  const unsigned char* a8 = reinterpret_cast<const unsigned char*>(A);
  const unsigned char* b8 = reinterpret_cast<const unsigned char*>(B);
  const int lds = sc::kGramStages * sc::kGramStageBytes;
  SC_DISPATCH_FIELD(ctx, F, f, with_bool(log_in >= ctx->nt_load_log, [&](auto NT) {   // streaming hint as in launch_pass_t
    hipLaunchKernelGGL((sc::gram_pass_kernel<F, kGramK, NT>), dim3(grid), dim3(sc::kGramThreads), lds, ctx->stream, f, a8, b8,
                       (unsigned)n_partials, (unsigned)spp, ctx->d_gram_rows, ticket, wo);
  }));
  return commit_wide_out(ctx, wo, pow3(kGramK));
}

// its cells: wait for the sequence word; the residues, or (sharded) the limb totals of all ranks recombined mod p
int collect_grid(sc_ctx* ctx, int ks, bool across_ranks, u64* out) {
  SC_TRY(wait_mailbox(ctx, ctx->mailbox_seq));
  const int cells = pow3(ks);
  const u64* wide = ctx->h_mailbox + sc::kMailboxWide;
  if (!across_ranks) {
    for (int c = 0; c < cells; ++c) out[c] = wide[c];
    return SC_OK;
  }
  HostField hf(ctx->fp);
  if (ctx->transport == Transport::kHost) {
    // this rank's residues: split, sum over the ranks on the host, recombine
    std::vector<u64> limbs(2 * (size_t)cells);
    for (int c = 0; c < cells; ++c) {
      limbs[2 * c] = wide[c] & 0xFFFFFFFFull;
      limbs[2 * c + 1] = wide[c] >> 32;
    }
    if (ctx->host_allreduce(ctx->host_user, limbs.data(), limbs.size()) != 0)
      return fail(ctx, SC_ERR_RCCL, "host all-reduce callback failed");
    for (int c = 0; c < cells; ++c) out[c] = hf.recombine(limbs[2 * c], limbs[2 * c + 1]);
    return SC_OK;
  }
  if (ctx->transport == Transport::kPeer) SC_TRY(check_exchange(ctx, "sums"));
  for (int c = 0; c < cells; ++c) out[c] = hf.recombine(wide[2 * c], wide[2 * c + 1]);
  return SC_OK;
}

// The last pass of a sharded prover on the peer transport (kernels.hpp, rank_pass_kernel): folds the shard's 2^kf
// pending entries, exchanges the one entry left per table with the peers and leaves the world-entry tables in A2 / B2
// and the 3^log2(world) cells of the rank-bit rounds in out[].
int rank_pass(sc_ctx* ctx, int kf, const u64* A, const u64* B, u64* A2, u64* B2, const u64* r, u64* out) {
  if (ctx->transport != Transport::kPeer || !ctx->use_mailbox || kf < 0 || kf > sc::kGridMaxVars || ctx->log_world < 1 || ctx->log_world > 3)
    return fail(ctx, SC_ERR_STATE, "rank_pass: needs the peer transport, the mailbox and 2..8 ranks");
  const sc::GridW gw = make_weights<sc::GridW>(ctx, r, kf);
  const sc::WgOut wo = next_wide_out(ctx, true, challenge_digest(r, kf, ctx->log_world, kf) ^ 0x72616e6bu, true, false);
  SC_TRY(timer_begin(ctx, SC_KIND_GRID_PASS, kf, ctx->log_world, kf, (u64)16 << kf, (u64)16 << ctx->log_world));
  SC_DISPATCH_FIELD(ctx, F, f,
                    hipLaunchKernelGGL((sc::rank_pass_kernel<F>), dim3(1), dim3(sc::kBlock), 0, ctx->stream, f, A, B, A2, B2, gw, kf, wo));
  SC_TRY(commit_wide_out(ctx, wo, 0));
  SC_TRY(wait_mailbox(ctx, ctx->mailbox_seq));
  SC_TRY(check_exchange(ctx, "entries"));
  for (int c = 0, cells = pow3(ctx->log_world); c < cells; ++c) out[c] = ctx->h_mailbox[sc::kMailboxWide + c];
  return SC_OK;
}

}  // namespace
