// Part of sumcheck_hip.hip (included there, in order, before its first user abi_r1cs.inc): what the round-per-launch sumchecks
// share - the cubic zerocheck, the grand product and its triple-product form, the fraction sums, the sum of products and the two
// protocols over the quadratic extension: the driver of their device rounds, the resident grid of a pass kernel, the refusal of
// fields without a cubic, and the launch schedule of a layer tree.

namespace {

// how many blocks of a pass kernel the device holds at once, capped by max_blocks; `gold` and `generic` are the Goldilocks and
// the generic-field instantiation of the form a family measured its occupancy on
template <class KG, class KM>
int resident_blocks(sc_ctx* ctx, KG* gold, KM* generic) {
  const void* fn = ctx->gold ? kernel_ptr(gold) : kernel_ptr(generic);
  return std::min(resident_grid(ctx, fn, sc::kBlock, ctx->max_blocks), ctx->max_blocks);
}

int require_cubic_field(sc_ctx* ctx, const char* what) {
  if (ctx->fp.p > 3) return SC_OK;
  return fail(ctx, SC_ERR_UNSUPPORTED, "%s: p = %llu: a cubic through 0, 1, 2, 3 needs 2 and 3 invertible", what, (unsigned long long)ctx->fp.p);
}

// The launches of a layer tree over 2^n leaves: from layer n, up to tree_lv layers per launch down to layer tail_log, then the
// tail kernel.  launch(m, lv) reads layer m and writes the lv layers below it; lv = 0: the tail, every layer below m.
template <class Launch>
int tree_schedule(int n, int tail_log, int tree_lv, Launch&& launch) {
  int m = n;
  while (m > tail_log) {
    const int lv = std::min(tree_lv, m - tail_log);
    SC_TRY(launch(m, lv));
    m -= lv;
  }
  return launch(m, 0);
}

// One device round as its launch sees it
struct DeviceRound {
  int round;              // j
  int log_in;             // the tables at in[.] have 2^log_in entries: those of round j - 1, which the launch folds, or (j = 0) the caller's
  size_t n_units;         // 2^(k - j - 1): the pairs of entries of round j's tables
  const u64* const* in;   // what the launch reads: the caller's tables in rounds 0 and 1, the folded tables of round j - 1 from round 2
  u64* const* out;        // the tables of round j, which the launch writes; null in round 0, which folds nothing
  const u64* r_prev;      // the challenge of round j - 1
  sc::PassOut po;
  // the blocks of the launch: one thread per unit, at most `resident` blocks
  int grid(int resident) const { return (int)std::max<size_t>(1, std::min<size_t>((n_units + sc::kBlock - 1) / sc::kBlock, (size_t)resident)); }
};
// what the launch tells the driver: its blocks and how many sums it leaves with the hand-off
struct Launched {
  int grid, sums;
};

// The device rounds 0 .. k - te of a sumcheck over `nt` <= MAXT tables of 2^k entries, k >= te >= 1, one launch per round: round
// j > 0 folds the tables of round j - 1 by that round's challenge (CW words) and sums over what it folded.  Rounds 0 .. k - te - 1
// are completed - next(round, e, c) draws, rs[CW round ..] receives c - and the launch of round k - te leaves its message in e
// and tables of 2^te entries at in[.], which the host takes (k = te: one launch, no fold, in[.] as it was).  A folded table is
// UW n_units words.  in[.]: the tables of round 0, never written; cur[.] owns every folded table (a block cur[q] holds on entry,
// such as the eq table of a layer, is given back as that one was).  next() returning false ends the call with *stopped, and every
// block goes back with nxt[.] and the caller's cur[.].
//
// launch(d, &l) opens the launch record (timer_begin), dispatches the kernel of round d.round on d.grid(its resident blocks) and
// reports both in l; a launch that reports no blocks or no sums is refused before anything is committed.  e is the driver's own
// buffer of the round's message: next() may rewrite it in place before it reads it (sc_sumprod_prove_ext widens round 0 there).
//
// The order of the steps carries three invariants:
// - next_pass_out commits nothing; the ticket base, the mailbox sequence and the exchange tag move in commit_pass_out, once the
//   launch is known to be in the stream: a failed launch must leave them where the device-side counter and the peers still are.
// - the tables of round j - 1 go back to the pool (cur = nxt) only once the launch that reads them is queued: reuse of a pool
//   block is ordered by the context's one stream, so whoever takes those blocks next runs behind that launch - and they go back
//   before collect_sums waits, so that the next round's allocation finds them.
// - every block has an owner at every return: nxt[.] holds the tables of a round whose launch failed, cur[.] those the last
//   launch wrote, so a next() that refuses (or any SC_TRY that fails) hands all of them back.
template <int MAXT, int CW, int UW, class Launch, class Next>
int device_rounds(sc_ctx* ctx, int nt, int k, int te, const u64** in, PoolBuf* cur, u64* rs, u64* e, const int* stopped, Launch&& launch,
                  Next&& next) {
  PoolBuf nxt[MAXT];
  u64 r_prev[CW] = {};
  for (int j = 0; j <= k - te; ++j) {
    const bool fold = j > 0;
    u64* out[MAXT] = {};
    DeviceRound d = {j, fold ? k - j + 1 : k, (size_t)1 << (k - j - 1), in, out, r_prev, {}};
    if (fold)
      for (int q = 0; q < nt; ++q) {
        SC_TRY(nxt[q].alloc(ctx, (size_t)UW * d.n_units));
        out[q] = nxt[q].get();
      }
    bool mb = false;
    d.po = next_pass_out(ctx, false, 0, &mb);
    Launched l = {0, 0};
    SC_TRY(launch(d, &l));
    if (l.grid < 1 || l.sums < 1) return fail(ctx, SC_ERR_STATE, "device_rounds: the launch of round %d reported %d blocks and %d sums", j, l.grid, l.sums);
    SC_TRY(commit_pass_out(ctx, d.po, l.grid));
    SC_TRY(timer_end(ctx));
    if (fold)
      for (int q = 0; q < nt; ++q) {
        cur[q] = std::move(nxt[q]);
        in[q] = cur[q].get();
      }
    SC_TRY(collect_sums(ctx, l.sums, false, mb, e));
    if (j == k - te) break;   // the host draws this round's challenge
    if (!next((size_t)j, e, r_prev)) return *stopped;
    for (int s = 0; s < CW; ++s) rs[(size_t)CW * (size_t)j + s] = r_prev[s];
  }
  return SC_OK;
}

}  // namespace
