// Part of sumcheck_hip.hip (included there, in order): the runtime of a multi-device handle (sc_ctx_create_multi): launcher
// threads, the shards' sums added on the host.

// =====================================================================================
// One handle, N devices, one process
// =====================================================================================
//
// The reference's caller is ONE process holding ONE Prover (sum-check-protocol/src/lib.rs:73-117, driven by
// matrix-multiplication/benches/mm_benchmark.rs:88-96).  A multi-device handle lets that unchanged caller use every GPU
// of the node (SURVEY.md section 8b: sc_ctx_create(field, devices[], n_devices); 8e: "one process drives all 8 devices,
// so the host-supplied r_j needs no broadcast"): the handle owns one ordinary context per entry of devices[] - shard d
// of every table, rank d of world N on Transport::kLocal - and presents the sc_table_* / sc_prod2_* / sc_prover_* /
// sc_prove surface over the whole table.
//
// In one process the exchange step of a sharded pass needs no collective at all: every shard's kernel leaves its own
// sums in its own pinned mailbox, and the host adds the N mailboxes (split limbs, or whole residues mod p) before it
// answers the round.  What costs time is launching on N devices: a hipLaunchKernelGGL is ~3-5 us of host time, so one
// thread launching on eight devices in turn would put ~30 us of skew into every pass - as much as the whole pass on a
// 2^20-entry shard.  So the handle keeps one launcher thread per further device (shard 0 runs on the calling thread):
// a job is handed over through one cache line per thread (generation counter, ~0.2 us each way), the thread launches
// on ITS device, spins on ITS mailbox and reports.  Threads spin while a proof is in flight (rounds are microseconds
// apart) and park on a condition variable after kParkAfterUs without work, so an idle handle costs no CPU.

struct MultiRuntime {
  static constexpr int kParkAfterUs = 300;
  struct alignas(128) Slot {
    std::atomic<uint64_t> go{0};      // generation of the job handed to this thread
    std::atomic<uint64_t> done{0};    // generation it has finished
    std::atomic<int> parked{0};
    std::mutex mu;
    std::condition_variable cv;
  };
  int n = 0;                           // shards (threads: n - 1)
  std::vector<std::thread> threads;
  Slot slots[kMaxSubs];
  const std::function<void(int)>* job = nullptr;
  uint64_t gen = 0;
  std::atomic<bool> quit{false};
  std::atomic<bool> in_run{false};     // run() is neither re-entrant nor thread-safe (one job pointer, one generation): guarded

  void worker(int d) {
    Slot& s = slots[d];
    uint64_t seen = 0;
    auto idle_since = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (true) {
      const uint64_t g = s.go.load(std::memory_order_acquire);
      if (g != seen) {
        if (quit.load(std::memory_order_acquire)) return;
        (*job)(d);
        seen = g;
        s.done.store(g, std::memory_order_release);
        idle_since = std::chrono::steady_clock::now();
        spins = 0;
        continue;
      }
      __builtin_ia32_pause();
      if ((++spins & 0x3FF) == 0 &&
          std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - idle_since).count() > kParkAfterUs) {
        // park.  Dekker with run(): parked = 1 (seq_cst) then re-read go; run() stores go (seq_cst) then reads parked
        std::unique_lock<std::mutex> lk(s.mu);
        s.parked.store(1, std::memory_order_seq_cst);
        s.cv.wait(lk, [&] { return s.go.load(std::memory_order_seq_cst) != seen; });
        s.parked.store(0, std::memory_order_seq_cst);
        spins = 0;
      }
    }
  }
  void start(int n_shards) {
    n = n_shards;
    for (int d = 1; d < n; ++d) threads.emplace_back([this, d] { worker(d); });
  }
  // fn(d) for every shard d, shard 0 on the calling thread; returns when all are done.  false: a run is already in flight
  // (a nested multi_run, or a second caller thread on one handle - a context is not thread-safe, include/sumcheck_hip.h)
  bool run(const std::function<void(int)>& fn) {
    if (in_run.exchange(true, std::memory_order_acquire)) return false;
    struct Leave {
      std::atomic<bool>& f;
      ~Leave() { f.store(false, std::memory_order_release); }
    } leave{in_run};
    if (n > 1) {
      job = &fn;
      ++gen;
      for (int d = 1; d < n; ++d) {
        Slot& s = slots[d];
        s.go.store(gen, std::memory_order_seq_cst);
        if (s.parked.load(std::memory_order_seq_cst)) {
          std::lock_guard<std::mutex> lk(s.mu);
          s.cv.notify_one();
        }
      }
    }
    fn(0);
    for (int d = 1; d < n; ++d) {
      Slot& s = slots[d];
      while (s.done.load(std::memory_order_acquire) != gen) __builtin_ia32_pause();
    }
    return true;
  }
  void stop() {
    quit.store(true, std::memory_order_release);
    ++gen;
    for (int d = 1; d < n; ++d) {
      Slot& s = slots[d];
      s.go.store(gen, std::memory_order_seq_cst);
      std::lock_guard<std::mutex> lk(s.mu);
      s.cv.notify_one();
    }
    for (auto& t : threads) t.join();
    threads.clear();
  }
};

namespace {

// a table of a handle with fewer entries than the handle has devices lives whole on the first device: one part (abi_multi.inc,
// "the first-device path")
inline bool is_single(const sc_ctx* m, const sc_table* t) { return t && !t->d && t->parts.size() == 1 && m->subs.size() > 1; }

// entry check of every call on a multi-device handle (the handle itself has no device to select)
int multi_enter(sc_ctx* m) {
  if (m->poisoned)
    return fail(m, SC_ERR_STATE, "multi-device handle is unusable after an earlier failure (%s); destroy it", m->err.c_str());
  return SC_OK;
}

// fn(d, sub) on every shard in parallel; the first failure (lowest shard) becomes the handle's error.  A failure on
// some shards and not on others leaves them out of step, so the handle is poisoned unless `recoverable`.
int multi_run(sc_ctx* m, const std::function<int(int, sc_ctx*)>& fn, bool recoverable = false) {
  const int n = (int)m->subs.size();
  int rc[kMaxSubs] = {};
  // (no exception may leave a launcher thread - std::terminate - or cross the C ABI: a failed host allocation inside a job is
  // that shard's SC_ERR_OOM)
  const std::function<void(int)> job = [&](int d) {
    try {
      rc[d] = fn(d, m->subs[d]);
    } catch (const std::bad_alloc&) {
      rc[d] = fail(m->subs[d], SC_ERR_OOM, "host allocation failed");
    } catch (...) {
      rc[d] = fail(m->subs[d], SC_ERR_STATE, "unexpected exception in a shard's job");
    }
  };
  if (!m->mrt->run(job))
    return fail(m, SC_ERR_STATE, "the multi-device handle is already inside a call (nested or concurrent use of one handle)");
  for (int d = 0; d < n; ++d)
    if (rc[d] != SC_OK) {
      if (!recoverable || m->subs[d]->poisoned) m->poisoned = true;
      return fail(m, rc[d], "device shard %d of %d: %s", d, n, m->subs[d]->err.c_str());
    }
  return SC_OK;
}

// A launch per shard that leaves 2*ns split limbs (launch(d, sub, &from_mailbox)), fetched on the launching thread;
// the calling thread adds the shards' limbs and recombines mod p: the whole exchange step of a sharded pass.
int multi_sums(sc_ctx* m, int ns, const std::function<int(int, sc_ctx*, bool*)>& launch, u64* out) {
  const int n = (int)m->subs.size();
  u64 limbs[kMaxSubs][2 * sc::kMaxSums];
  SC_TRY(multi_run(m, [&](int d, sc_ctx* sub) -> int {
    bool mb = false;
    SC_TRY(launch(d, sub, &mb));
    u64* src = nullptr;
    SC_TRY(fetch_limbs(sub, ns, n > 1, mb, &src));
    memcpy(limbs[d], src, 2 * (size_t)ns * sizeof(u64));
    return SC_OK;
  }));
  HostField hf(m->fp);
  for (int s = 0; s < ns; ++s) {
    u64 lo = 0, hi = 0;
    for (int d = 0; d < n; ++d) {
      lo += limbs[d][2 * s];
      hi += limbs[d][2 * s + 1];
    }
    out[s] = hf.recombine(lo, hi);
  }
  return SC_OK;
}

}  // namespace

// ---- tables of a handle: N parts ----------------------------------------------------------------------

namespace {

sc_table* new_multi_table(size_t n_parts, size_t len) {
  sc_table* t = new (std::nothrow) sc_table;
  if (t) {
    t->parts.assign(n_parts, nullptr);
    t->len = len;
  }
  return t;
}
void drop_multi_table(sc_ctx* m, sc_table* t) {
  if (!t) return;
  for (size_t d = 0; d < t->parts.size() && d < m->subs.size(); ++d) TableBuf(m->subs[d], t->parts[d]).reset();   // (each part is an ordinary table of its device: freed through its owner)
  delete t;
}
// build a table of the handle part by part: make(d, sub, &part) on every shard in parallel
int make_multi_table(sc_ctx* m, size_t len, const std::function<int(int, sc_ctx*, sc_table**)>& make, sc_table** out) {
  TableBuf t(m, new_multi_table(m->subs.size(), len), /*multi=*/true);
  if (!t.get()) return fail(m, SC_ERR_OOM, "host allocation failed");
  SC_TRY(multi_run(m, [&](int d, sc_ctx* sub) { return make(d, sub, &t->parts[d]); }, /*recoverable=*/true));
  *out = t.release();
  return SC_OK;
}
int check_multi_len(sc_ctx* m, size_t len, const char* what) {
  if (!is_pow2(len) || len < m->subs.size())
    return fail(m, SC_ERR_ARG, "%s: len %zu must be a power of two of at least one entry per device (%zu)", what, len, m->subs.size());
  return SC_OK;
}

}  // namespace
