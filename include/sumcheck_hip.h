/*
 * sumcheck_hip.h - C ABI of libsumcheck_hip.so, the MI355X (gfx950) sumcheck prover hot path.
 *
 * Drop-in boundary.  In the reference (montekki/thaler-study, Rust) this path sits behind
 * the generic trait `SumCheckPolynomial<F>` (sum-check-protocol/src/lib.rs:121-156) driven
 * by `Prover<F,P>` (:73-117) / `Verifier<F,P>` (:227-331); the table arithmetic itself is
 * ark_poly::DenseMultilinearExtension.  There is no FFI in the reference; these entry
 * points are what a thin `-sys` crate would bind (INTEGRATION.md shows the Rust side).
 * Each function cites the reference interface (file:line, relative to the reference
 * root) it replaces.
 *
 * Conventions
 *  - Every uint64_t field element is the Montgomery residue x*2^64 mod p in [0,p): exactly
 *    the memory word of ark-ff's `Fp64<MontBackend<_,1>>`, so `&[F]` crosses zero-copy.
 *  - Tables are multilinear-extension evaluation tables of length 2^k; variable 0 is index
 *    bit 0 (ark-poly order, "LE") unless an `order` argument says otherwise.
 *  - Every function returns an int status (SC_OK = 0).  Nothing throws or aborts across the
 *    ABI; sc_last_error() gives the message for the last non-zero status on that context.
 *    The reference's prover methods are infallible by signature, so the Rust shim panics
 *    on a non-zero status (SURVEY.md section 8b "Errors").
 *  - A context is NOT thread-safe (the reference's `round` takes `&mut self`); use one
 *    context per prover thread.  Different contexts may be used concurrently.
 *  - A context owns one HIP stream on one device.  Calls are synchronous from the caller's
 *    point of view unless stated otherwise.
 *  - There is no CPU fallback: every entry point that computes fails with SC_ERR_HIP when
 *    no gfx950 device is usable.
 */
#ifndef SUMCHECK_HIP_H
#define SUMCHECK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_OK 0
#define SC_ERR_ARG 1         /* bad argument (null, non power-of-two length, wrong round index ...) */
#define SC_ERR_HIP 2         /* HIP runtime / no device */
#define SC_ERR_RCCL 3        /* collective layer */
#define SC_ERR_OOM 4         /* device or host allocation failed */
#define SC_ERR_STATE 5       /* call sequence violates the protocol state machine */
#define SC_ERR_UNSUPPORTED 6

#define SC_ORDER_LE 0 /* variable 0 = index bit 0: ark_poly::DenseMultilinearExtension */
#define SC_ORDER_BE 1 /* variable 0 = index MSB: multilinear-extensions/src/lib.rs:6-60 */

/* Field description.  Mirrors `#[derive(MontConfig)] #[modulus = "..."]`
 * (sum-check-protocol/src/lib.rs:349-354) as runtime constants. */
typedef struct sc_field {
  uint64_t p;         /* odd prime modulus, 2 < p < 2^64 */
  uint64_t p_inv_neg; /* -p^-1 mod 2^64 */
  uint64_t r_mod_p;   /* 2^64 mod p  (Montgomery form of 1) */
  uint64_t r2_mod_p;  /* 2^128 mod p */
} sc_field;

typedef struct sc_ctx sc_ctx;
typedef struct sc_table sc_table;
typedef struct sc_prover sc_prover;

/* ---- field helpers (host, O(1)) ------------------------------------------------------- */

/* Fill an sc_field from a modulus.  p = 2^64-2^32+1 selects the Goldilocks kernels. */
int sc_field_from_modulus(uint64_t p, sc_field* out);
/* canonical integer <-> Montgomery word (F::from_bigint / into_bigint) */
uint64_t sc_field_to_mont(const sc_field* f, uint64_t canonical);
uint64_t sc_field_from_mont(const sc_field* f, uint64_t mont);
/* interpolate_quadratic_poly through (0,e0),(1,e1),(2,e2): matrix-multiplication/src/lib.rs:17-60,
 * :124-130.  c[d] = coefficient of X^d. */
int sc_interpolate_quadratic(const sc_field* f, const uint64_t e[3], uint64_t c[3]);

/* ---- context ------------------------------------------------------------------------- */

int sc_ctx_create(const sc_field* f, int device, sc_ctx** out);
/* ONE handle over n_devices GPUs of this process (sc_ctx_create(field, devices[], n_devices); 8e: "one
 * process drives all 8 devices, so the host-supplied r_j needs no broadcast").  The reference's caller is one process
 * holding one Prover (sum-check-protocol/src/lib.rs:73-117, mm_benchmark.rs:88-96); with this handle that unchanged caller
 * uses every GPU of the node - no launcher, no communicator, no replicated verifier randomness.  n_devices: a power of two,
 * 1..8; devices[] may repeat a device (tests on a one-GPU box).  Every table created on the handle (sc_table_upload /
 * _generate / _clone / _fix_variables, sc_matmul_g_new, sc_prod2_*) is ONE table whose d-th contiguous 1/n_devices (top
 * log2(n_devices) index bits = d) lives on devices[d]; sc_table_evaluate, sc_prod2_*, sc_prover_* and sc_prove work on the
 * whole table.  In one process the exchange step of a pass needs no collective: every device's kernel leaves its own sums
 * in its own pinned mailbox and the calling thread adds them (split limbs / residues mod p) before it answers the round;
 * launches go out from one thread per device.  When a pass leaves <= 2^host_tail_log entries per table and device it writes
 * them to pinned host memory and the host finishes the proof (option "host_tail_log"): every launcher thread folds its
 * device's pending challenges, the calling thread serves the remaining rounds.  Results are bit-identical to a one-device context.
 * Also served: sc_gkr_wiring, sc_gkr_prover_* / sc_gkr_prove (the dense W prover: every device streams its rows of c of add_i /
 * mul_i, the small product proofs run on the first device), sc_gkr_w_evaluate, and sc_tri_prover_* / sc_tri_prove /
 * sc_tri_evaluate (every device squares its rows of the adjacency matrix).
 * Through the handle's FIRST device (round 5: gather, the ordinary call on whole tables, scatter of table results - functional,
 * not fast; SC_ERR_UNSUPPORTED before): tables with fewer entries than devices (they live on the first device), sc_table_fix_variables
 * across the device bits (either order), sc_table_relabel, the product calls on one-entry shards, sc_matmul_g_new on matrices with
 * fewer than two columns per device, and the callers' generic trait calls sc_gkr_w_round_sums / _to_evaluations / _fix_variables
 * and sc_tri_round_sums / _to_evaluations / _fix_variables - the reference's fallback loop fix_variables(&[r]) -> to_univariate
 * (gkr-protocol/src/round_polynomial.rs:59-90, triangle-counting/src/lib.rs:89-132) runs on a handle down to the constant.
 * Not served (SC_ERR_UNSUPPORTED): sc_table_from_device, sc_gkr_prover_create / sc_tri_prover_create on tables with fewer rows than
 * devices (sc_gkr_prover_create_sparse runs on the handle's first device), and the sc_ctx_comm_* calls (the handle is its own
 * communicator; sc_ctx_comm_rank reports rank 0 of 1 - its tables are whole tables; option "n_devices" counts the devices).
 * sc_table_device_ptr returns NULL; sc_ctx_stream, sc_ctx_kernel_time and sc_ctx_launch_log report the first device (one GPU's
 * launches over its own shard).  A handle is validated on ONE physical device only (devices[] naming device 0 N times: this pool's
 * boxes have one GPU); its cross-device copies are hipMemcpyPeerAsync and its tail outputs system-scope write-through stores. */
int sc_ctx_create_multi(const sc_field* f, const int* devices, int n_devices, sc_ctx** out);
int sc_ctx_destroy(sc_ctx* ctx);
/* message of the last failing call on ctx (ctx == NULL: last failing sc_ctx_create) */
const char* sc_last_error(const sc_ctx* ctx);
/* Tunables (all have working defaults; they exist for measurements and tests):
 *   "vars_per_pass"    rounds served by one device pass: 1 | 2 (default 2)
 *   "first_pass_vars"  rounds served by the prover's first pass, which has nothing to fold:
 *                      1 | 2 | 3 | 4, default 0 = four for tables (shards) of >= 2^"gram_log" entries (below), else three
 *                      for tables of >= 2^18 entries, two below (never more than vars_per_pass allows).  4 = the
 *                      matrix-core pass at any size from 2^14 entries (where it does not apply - smaller tables,
 *                      "vars_per_pass" 1, sharded provers with "grid_sharded" 0 - the same as 0)
 *   "fold_dma"         (default 1) pass_kernel<4,2>, the fold behind the matrix-core first pass, brings its sub-steps in by LDS-DMA
 *                      (Goldilocks; 0 and every other modulus: through registers).  Same results; for A/B measurements
 *   "pipe32"           (default 1) pass_kernel<3,2> on whole tiles of tables of >= 2^"pipe32_log" (default 20) entries runs in its
 *                      pipelined form (sub-steps of 64 outputs, loads in flight while the wave multiplies, three waves per
 *                      SIMD); 0 = the staged form everywhere.  Same results; for A/B measurements
 *   "gram_log"         (default 21; 0 = never, else 14..40) a proof on tables (a sharded one: shards) of >= 2^gram_log entries opens
 *                      with gram_pass_kernel: rounds 1..4 from ONE read, as exact integer limb products of the tables'
 *                      bytes on the int8 matrix cores; every block reduces its accumulators to the 81 cells mod p and the
 *                      block that finishes last adds them (ONE launch since round 5); the pass behind it folds four
 *                      variables (wfold_pass_kernel<4,5>, or pass_kernel<4,2>: below).  DESIGN.md section 4
 *   "wfold_log"        (default 40; 0 = never, else 12..40) the pass behind the matrix-core pass - four pending challenges, round 4 -
 *                      on tables (shards) of 2^"wfold_min_log" (default 21) .. 2^wfold_log entries may be wfold_pass_kernel<4,5>:
 *                      it folds the four challenges AND serves FIVE rounds (pass_kernel<4,2>: two).  Taken where the proof then
 *                      needs fewer launches (the planner counts both ways: n = 25, 27, 28, 29 on one device) or where the
 *                      alternative is a grid pass streaming the whole table (n = 21..24); "wfold_always" = 1: wherever it can
 *                      run.  "wfold5_min_log" (default 24): a grid pass with FIVE challenges to fold over tables of >= 2^this
 *                      entries runs in the same kernel's (5, 3..5) form.  Same results; DESIGN.md sections 4, 5
 *   "wfold_slot_period" (default -1; 0 = off; 1..2^24 in ticks of the device's 100 MHz wall clock, i.e. 10 ns) wfold_pass_kernel's
 *                      writes of the folded tables aligned in time across the chip: every XCD reads the same clock, so slots
 *                      [k period, k period + width) open on all of them at once, without communication and without any wave
 *                      waiting.  "wfold_slot_width" = 0: only the bulk write-back requests move to the period's boundaries;
 *                      > 0: a wave holds a tile's outputs in registers and stores them at the first sub-step boundary inside a
 *                      slot, at the end of its next tile at the latest (>= period: always open).  "wfold_slot_stagger" = 1
 *                      shifts the slots of the eight XCDs against each other by period / 8: the control of the measurement.
 *                      -1: period 2400 and width 600 (a 6 us slot every 24 us) for the four-challenge fold of tables of
 *                      >= 2^25 entries, where that was measured to pay (n = 28: 779 -> 734 us), none elsewhere; width and
 *                      stagger apply to an explicit period only.  Same results bit for bit at every setting; DESIGN.md section 5
 *   "host_tail_log"    (default 12; 0..12) the host finishes the proof: a pass whose folded tables have <= 2^host_tail_log
 *                      entries (per device on a multi-device handle) writes them to pinned host memory instead of the
 *                      pool, and every later round is served by the host from them - fold the pending challenges
 *                      (<= 2^13 multiply-adds), then one sub-microsecond round at a time - with NO further launch: the
 *                      last launch (or two) of every proof and every shard, ~13 us each, disappears; the planner aims its
 *                      grid passes at this hand-over (fewest launches up to it, fewest rounds per pass among those) - at
 *                      2^11 entries where the larger hand-over saves no launch (the host's first read of what the device
 *                      wrote costs ~0.1 us per KiB).  Not a CPU path
 *                      for the hot loop: what the host touches is what is left when 2^-18 of the work remains.  Applies
 *                      to unsharded provers (incl. a sharded one after its gather) and to multi-device handles; five-round
 *                      passes (and any pass with <= 32 outputs) hand over, 0 = off (a multi-device handle then hands
 *                      over once a shard holds <= 32 entries, as in round 4)
 *   "gp_host_log"      (default 10; 0..12) sc_gp_prove: the layers of <= 2^gp_host_log entries are proven on the host from one copy
 *                      of the bottom of the tree, and in every larger layer the launch that writes tables of 2^gp_host_log
 *                      entries is the last one: the host takes them and finishes the layer.  0: every round on the device,
 *                      the host folds the last two entries.  Same transcript at every value.  "gp_tree_lv" (default 3;
 *                      1..3): tree layers per launch of sc_gp_create above its one-block tail.  DESIGN.md section 9 item 16
 *   "fr_host_log"      (default 9; 0..12)  sc_frac_prove: what "gp_host_log" is to sc_gp_prove, over the two fraction trees: the layers
 *                      of <= 2^fr_host_log entries are proven on the host from one copy of the bottom of both trees, and in every
 *                      larger layer the launch that writes tables of 2^fr_host_log entries is the last one.  Same transcript at
 *                      every value.  "fr_tree_lv" (default 3; 1..3): tree layers per launch of sc_frac_create above its one-block
 *                      tail.  DESIGN.md section 9 item 17.  sc_frac_prove_ext and sc_frac_create_ext (item 22) follow both options
 *                      over their four heaps; the one-block tail of their trees takes layers of <= 2^10 entries
 *   "grid_pass"        the passes whose FOLDED tables have <= 2^"grid_log" (default 20) entries serve up to
 *                      "grid_max_vars" (default 5) rounds each and fold up to five pending challenges at once
 *                      (wgrid_pass_kernel); "grid_blocks" caps the launch (0 = what fits on the chip at once).
 *                      1 (default) | 0 = two rounds per pass all the way down.  Not used with "vars_per_pass" 1
 *                      or, for the first pass, an explicit "first_pass_vars" - those name their own schedules.
 *                      "grid_sharded" (1): the shards of a sharded prover go on with these passes too (cells
 *                      exchanged inside the kernel on the peer transport, summed by one collective per pass on
 *                      the others) until they are down to their pending challenges; on the peer transport one
 *                      small launch then serves the rounds of the rank bits (no gather).  0: two-round sharded
 *                      passes, gather at "tail_log".
 *   "tail_log"         shard log-size at which a sharded prover gathers with "grid_sharded" 0 (default 16)
 *   "max_blocks"       grid cap of the streaming kernels (default 3 per CU = 768); a pass never
 *                      launches more blocks than fit on the chip at once
 *   "use_mailbox"      kernels publish sums to pinned host memory the host spins on (default 1)
 *   "arena_log"        peer transport: a gather arena holds world * 2^arena_log words per table (default 17;
 *                      set before sc_ctx_comm_peer_export; longer gathers go in chunks)
 *   "peer_spin_ms"     peer transport: bound of every in-kernel wait for a peer = the largest skew between the
 *                      ranks' launches of the same pass that is tolerated (default 2000); past it the pass fails
 *                      with SC_ERR_RCCL on every rank that waited.  "peer_connect_ms" (default 120000): how long
 *                      sc_ctx_comm_peer_connect waits for every peer's hello (absorbs the start-up lag of a job)
 *   "rccl_timeout_ms"  RCCL plane: how long the host waits for work queued behind a collective - a sharded pass's sums, a
 *                      gathered table - before it gives the communicator up (default 30000).  A collective whose peer is gone
 *                      (a rank that died or is out of step) never completes on its own; past the bound, or as soon as
 *                      ncclCommGetAsyncError reports an error, the library calls ncclCommAbort, poisons the context and
 *                      returns SC_ERR_RCCL from the call that waited and from every later one
 *   "dbg_delay_ms" / "dbg_skip_tag"   fault injection for tests: delay every sharded launch of this rank on the
 *                      host / make its next sharded launch skip an exchange tag (a rank out of step)
 *   "pool_contiguous"  experiments: 1 = pool blocks of >= 1 MiB are asked for as physically contiguous VRAM
 *                      (hipDeviceMallocContiguous; default 0; experiments/r04_vmm_placement.md, addendum 2)
 *   "dbg_fold_grab"    measurements: tiles per draw of fold_kernel's four-wave launches (0 = the default, 1; 4 = round 3's
 *                      behaviour, profiles/r04_fold_small_grab_ab.txt)
 *   "time_kernels"     HIP-event timing of pass kernels (see sc_ctx_kernel_time)
 *   "prewarm"          an ACTION, not a setting: value = num_vars of the proofs to come.  Pays now what the first proof of that size
 *                      would pay on this context - the library's code object on the device, the resident-grid queries of the plan's
 *                      kernels, the matrix-core pass's workspace, the pool blocks of every folded table - for callers that prove
 *                      once (mm_benchmark.rs:88-96 builds g and proves).  On a multi-device handle every device does its shard's
 *                      share of this (the handle must be healthy: a poisoned handle refuses with SC_ERR_STATE like any other call)
 *   "stat_reset"       (set) zeroes, and "stat_wait_ns" / "stat_launch_ns" (get) read, where a proof's wall time goes on the host:
 *                      ns spent waiting for pass kernels (their run time + launch latency) and ns inside the pass launches (buffers,
 *                      weights, hipLaunchKernelGGL); the rest is host arithmetic between them.  Always on (four clock reads per pass).
 *                      On a multi-device handle both read the FIRST device's context only (the devices run side by side: their
 *                      waits overlap, a sum would count the same wall time N times)
 *   "stat_pool_live_blocks" / "stat_pool_live_words" / "stat_pool_peak_words"  (get) the device-buffer pool's bookkeeping: blocks
 *                      handed out and not yet given back (tables, prover state, buffers of a call in flight), their total capacity
 *                      in 64-bit words, and the high-water mark of that total; "stat_reset" sets the mark to the current total.
 *                      Host-side counters only.  On a multi-device handle each is the SUM over its devices' contexts
 *   "nt_load_log" / "nt_store_log"  table log-size from which loads / stores are nontemporal
 * Environment: SC_RCCL_LIBRARY = the RCCL build sc_ctx_comm_init_rccl / sc_comm_unique_id dlopen (a path; default librccl.so.1).
 * That library or nothing: a path that cannot be loaded is an error, never a silent second choice. */
int sc_ctx_set_option(sc_ctx* ctx, const char* key, int64_t value);
/* reads any option back; also read-only: "n_devices" (1, or the devices behind a multi-device handle), "transport" (0 none,
 * 1 RCCL, 2 host callbacks, 3 peer, 4 local = a multi-device handle) and "comm_nranks"
 * = the number of ranks the data plane spans as the transport itself reports it (ncclCommCount for RCCL) */
int sc_ctx_get_option(const sc_ctx* ctx, const char* key, int64_t* value);
int sc_ctx_synchronize(sc_ctx* ctx);
/* the context's hipStream_t (for HIP-event timing by a benchmark harness) */
void* sc_ctx_stream(const sc_ctx* ctx);
/* device-time accounting of the pass kernels launched since the last reset:
 * out[0] = number of pass launches, out[1] = sum of their durations in ms (HIP events on
 * the context's stream; enabled by option "time_kernels" = 1). */
int sc_ctx_kernel_time(sc_ctx* ctx, double out[2], int reset);
/* Per-launch records of the same instrumentation (option "time_kernels" = 1): what each timed
 * launch was, the HBM bytes it has to move (every input once, every output once) and its HIP-event
 * duration.  A benchmark derives bytes actually moved and per-kernel GB/s from the launches that
 * really ran instead of from a model.  Copies min(cap, n) records, stores the number available in
 * *n_out, clears the log if reset.  The log keeps at most 65536 records. */
#define SC_KIND_PASS 0       /* pass_kernel<kf,ks>: fold kf variables of both tables + grid sums of ks rounds */
/* 1 was a three-round tail kernel that wgrid_pass_kernel replaced (round 3) */
#define SC_KIND_EVALUATE 2   /* evaluate_kernel: one table, kf = number of variables */
#define SC_KIND_FOLD 3       /* fold_kernel<kf>: LE fix of kf <= 3 variables of one table */
#define SC_KIND_FIX_LOW 4    /* fix_low_kernel: LE fix of 8..17 variables in one pass */
#define SC_KIND_FOLD_BE 5    /* fold_be_kernel: BE fix of one variable */
#define SC_KIND_COLDOT 6     /* coldot_kernel (+ sum_rows_kernel): BE multi-variable fix / f_A of G::new */
#define SC_KIND_GKR 7        /* GKR W pass: fold add/mul/w + round sums */
#define SC_KIND_MATSQ 8      /* triangle counting: square of the adjacency matrix */
/* 9 was the resident prover kernel (removed in round 3: measured equal to launches) */
#define SC_KIND_GRID_PASS 10 /* wgrid_pass_kernel: fold kf <= 5 variables of tables of <= 2^20 folded entries + the 3^ks cells of ks <= 5 rounds */
#define SC_KIND_GRAM_PASS 11   /* gram_pass_kernel: the four-round first pass of a large proof on the int8 matrix cores (ks = 4) */
#define SC_KIND_WFOLD_PASS 13  /* wfold_pass_kernel: a fold of kf = 4 / 5 variables of large tables that serves ks = 5 / 3..5 rounds (behind the matrix-core first pass; the pass behind that) */
/* 12 was gram_finish_kernel (rounds 4: a second launch behind the gram pass; folded into gram_pass_kernel in round 5) */
#define SC_KIND_CIRCUIT 14     /* circuit_layer_kernel: one layer of sc_circuit_evaluate; log_in = k[i] (gates), kf = k[i+1]; bytes = the streamed 20 B per gate */
#define SC_KIND_MATMUL 15      /* sc_matmul: kf = 0 the byte repack, 1 matmul_mfma_kernel (int8 matrix cores), 2 matmul_tiled_kernel, 3 matmul_kernel (VALU); ks = n, log_in = 2n */
#define SC_KIND_BATCH_PASS 16  /* batch_pass_kernel: one pass of every instance of sc_prove_batch; kf, ks and log_in (= n at the first pass) as for a grid
                                * pass; the batch size is bytes_read / (16 * 2^log_in) */
#define SC_KIND_GRID_EXTEND 17 /* grid_extend_kernel: one axis of sc_table_extend_grid; kf = the variable extended, ks = log_in = m.  One launch
                                * per variable (not fused): bytes = what that launch reads and writes, about p/(p-2) times the output in all */
#define SC_KIND_MERKLE 18      /* sc_merkle_*: kf = 0 merkle_leaf_kernel (leaves up to level ks = min(n, 4)), 1 merkle_level_kernel (level ks),
                                * 2 merkle_top_kernel (levels ks .. n in one block), 3 merkle_open_kernel (an opening's gather); log_in = n */
#define SC_KIND_RS_ENCODE 19   /* rs_encode_rows_kernel: the row transform of sc_rs_encode_rows / sc_ligero_commit, one launch; kf = log_cols, ks = log_blowup,
                                * log_in = n; it reads the table once (8 * 2^n bytes) and writes the codewords once (8 * 2^(n + log_blowup)) */
#define SC_KIND_LIGERO 20      /* sc_ligero_*: kf = 0 column_leaf_kernel (ks = log2 rows; reads E, writes L digests), 1 row_combine_kernel (ks = the
                                * number of weight vectors; ks = 0: the launch that adds the row ranges' partial sums), 2 column_open_kernel
                                * (ks = openings of the launch); log_in = n.  The tree levels above the leaves are SC_KIND_MERKLE records */
#define SC_KIND_XC_ENCODE 21   /* xc_encode_rows_kernel: the row encoder of sc_xc_encode_rows / sc_ligero_commit_code(SC_CODE_EXPANDER), one launch;
                                * kf = log_cols, ks = recursion levels, log_in = n; it reads the table once (8 * 2^n bytes) and writes the
                                * codewords once (8 * 2^(n + 1)) */
#define SC_KIND_RS_LONG 22     /* the two launches of a long row transform (sc_rs_encode_rows_long / sc_ligero_commit_long, codewords of 2^15 .. 2^24
                                * words): kf = 0 the column step, rs_long_column_kernel (ks = a; reads the table, 8 * 2^n bytes, writes the codewords,
                                * 8 * 2^(n + log_blowup)), kf = 1 the row step, rs_long_row_kernel (ks = b; reads and writes the codewords in place);
                                * a + b = log_cols + log_blowup, log_in = n */
#define SC_KIND_XC_LONG 23     /* the launches of a long expander-code row (sc_xc_encode_rows_long / sc_ligero_commit_code_long, log_cols 14 .. 23;
                                * kernels/expander_long.hpp): kf = 0 xc_long_copy_kernel, the systematic part (ks = log_cols; reads and writes
                                * 8 * 2^n bytes); kf = 1 xc_long_down_kernel, one per level kept in global memory, ks = lm = log2 of the level's
                                * message (reads 8 * R * 2^lm, writes 8 * R * 2^(lm-2), R = 2^(n - log_cols) rows); kf = 2 xc_long_inner_kernel, the
                                * code below them in LDS (ks = lm_i = 12 or 13; reads and writes 8 * R * 2^lm_i); kf = 3 xc_long_up_kernel, one per
                                * global level (reads and writes 8 * R * 2^(lm-1)); log_in = n */
#define SC_KIND_RS_FOLD 24     /* rs_fold_kernel<F, 1, kf>: one fold of a Reed-Solomon codeword of M = 2^ks words (sc_rs_fold, sc_ligero_fold_prove), one launch; kf = 1 if
                                * it also hashed the leaves of the folded codeword's tree, else 0; log_in = n (sc_rs_fold: ks); it reads 8 * M bytes
                                * and writes 4 * M, plus 8 * M of digests with kf = 1.  The tree levels above the leaves are SC_KIND_MERKLE records */
#define SC_KIND_RS_FOLD_MANY 25 /* rs_fold_kernel<F, A, AN>: A = kf successive folds of a Reed-Solomon codeword of M = 2^ks words in one launch (sc_rs_fold_many,
                                * sc_ligero_fold_prove on an opening begun with a schedule); log_in = n (sc_rs_fold_many: ks); it reads 8 * M bytes and
                                * writes 8 * M / 2^A, plus 32 bytes per leaf of the next stage's tree when it hashed them */
#define SC_KIND_SPMV 26        /* a sparse product of sc_r1cs_mul / sc_r1cs_bind_rows over nnz entries in B = ceil(nnz / 2048) blocks: kf = 0 spmv_kernel
                                * (with the zeroing of its output; reads 24 * nnz bytes - row, col, val and the gathered word - and writes 8 * 2^log_in
                                * + 24 * B), kf = 1 spmv_carry_kernel (reads 24 * B, writes 8 * min(2 B, 2^log_in)); ks = 1 if transposed (bind_rows);
                                * log_in = log2 of the output length */
#define SC_KIND_ZEROCHECK 27   /* zc_pass_kernel: one round of sc_zerocheck_prove; kf = 1 if it folded the previous challenge, ks = 1, log_in = log2 of
                                * the tables it read: 4 * 8 * 2^log_in bytes read, and 4 * 8 * 2^(log_in - 1) written with kf = 1 */
#define SC_KIND_PRODUCT_TREE 28 /* a launch of sc_gp_create from layer m = log_in of the product tree: kf = LV = 1..3, gp_tree_kernel<F, LV>, which reads
                                * 8 * 2^m bytes and writes the layers m-1 .. m-LV, 8 * (2^m - 2^(m-LV)); kf = 0, gp_tree_tail_kernel, one block from
                                * a layer of <= 2^12 words down to V_0: 8 * 2^m read, 8 * (2^m - 1) written; ks = 0 */
#define SC_KIND_PRODUCT_PASS 29 /* gp_pass_kernel: one round of a layer of sc_gp_prove; kf = 1 if it folded the previous challenge, ks = 1, log_in = log2
                                * of the tables it read: 3 * 8 * 2^log_in bytes read, and 3 * 8 * 2^(log_in - 1) written with kf = 1 */
#define SC_KIND_FRACTION_TREE 30 /* a launch of sc_frac_create from layer m = log_in of the two fraction trees: kf = LV = 1..3, fr_tree_kernel<F, LV, ONES>;
                                 * ks = the tables it read: 2, or 1 where the numerator is all ones (m = n); it reads ks * 8 * 2^m bytes and writes
                                 * the layers m-1 .. m-LV of both trees, 2 * 8 * (2^m - 2^(m-LV)); kf = 0, fr_tree_tail_kernel, one block from a layer
                                 * of <= 2^11 entries down to the root: 2 * 8 * (2^m - 1) written */
#define SC_KIND_FRACTION_PASS 31 /* fr_pass_kernel: one round of a layer of sc_frac_prove; kf = 1 if it folded the previous challenge, ks = the tables it
                                 * read: 5 (E, QL, QR, PL, PR), or 3 in the top layer of an all-ones numerator; log_in = log2 of the tables it read:
                                 * ks * 8 * 2^log_in bytes read, and ks * 8 * 2^(log_in - 1) written with kf = 1 */
#define SC_KIND_LOOKUP_COUNT 32  /* sc_lookup_count: kf = 0 lookup_count_kernel (ks = 1: a private histogram per block in LDS, m <= 13; 0: adds to
                                 * global memory; log_in = n; reads 12 * 2^n bytes of w and idx and gathers 8 * 2^n of t, writes 4 * 2^m of
                                 * counters), kf = 1 lookup_mont_kernel (log_in = m; reads 4 * 2^m, writes 8 * 2^m) */
#define SC_KIND_SPARK_INDEX 33   /* sc_spark_create, one dimension: kf = 0 spark_index_kernel (ks = 1: a private histogram per block in LDS, at most
                                 * 2^13 counters; 0: adds to global memory; log_in = l; reads 4 * 2^l bytes of indices, writes 8 * 2^l of field
                                 * words and 4 * 2^m of counters), kf = 1 lookup_mont_kernel (log_in = m; reads 4 * 2^m, writes 8 * 2^m) */
#define SC_KIND_SPARK_GATHER 34  /* spark_gather_kernel: both dimensions of sc_spark_gather in one launch; log_in = l; reads 8 * 2^l bytes of
                                 * indices and gathers 16 * 2^l, writes 16 * 2^l */
#define SC_KIND_SPARK_TUPLE 35   /* spark_tuple_kernel: one table of sc_spark_denominators; kf = 1 where the key is the index itself; log_in = n
                                 * for 2^n entries; reads 8 * 2^n bytes (12 * 2^n with a key stream), writes 8 * 2^n */
#define SC_KIND_EQ_SUM 36        /* eq_sum_kernel: the one launch of sc_table_eq_sum; ks = the number of points, log_in = n; reads the ks * (n + 1)
                                 * words of points and coefficients, writes 8 * 2^n */
#define SC_KIND_SUMPROD_PASS 37  /* sumprod_pass_kernel: one round of sc_sumprod_prove; kf = 1 if it folded the previous challenge, ks = T, the
                                 * pairs of tables; log_in = log2 of the tables it read: 2 T * 8 * 2^log_in bytes read, and
                                 * 2 T * 8 * 2^(log_in - 1) written with kf = 1 */
#define SC_KIND_SUMPROD_EXT_PASS 38 /* ext_sumprod_pass_kernel: one round j >= 1 of sc_sumprod_prove_ext (round 0 is a kind 37 record); kf = 1
                                 * for base tables in (round 1), kf = 2 for extension tables in; ks = T; log_in = log2 of the entries per
                                 * table it read: 2 T * 8 * 2^log_in bytes read with kf = 1, 2 T * 16 * 2^log_in with kf = 2, and
                                 * 2 T * 16 * 2^(log_in - 1) written.  ks = 0: ext_fold_kernel, one launch of sc_table_evaluate_ext - the
                                 * same fold of ONE table, nothing summed: the same bytes with 2 T replaced by 1 */
#define SC_KIND_EXT_PRODUCT_TREE 39 /* a launch of sc_gp_create_ext from layer m = log_in of the product tree over K: kf = LV = 1..3,
                                 * ext_gp_tree_kernel<F, LV, LEAF_IN>; ks = 1 where it read the base table and formed the leaves (m = n),
                                 * else 2 (both planes of layer m); it reads ks * 8 * 2^m bytes and writes both planes of the layers
                                 * m-1 .. m-LV, 16 * (2^m - 2^(m-LV)); kf = 0, ext_gp_tree_tail_kernel, one block from a layer of <= 2^11
                                 * entries down to V_0: 16 * (2^m - 1) written */
#define SC_KIND_EXT_PRODUCT_PASS 40 /* ext_gp_pass_kernel: one round of a layer of sc_gp_prove_ext; kf = 1 if it folded the previous challenge;
                                 * ks = 1 where L and R are the halves of the base table with the leaves formed in registers (layer
                                 * n - 1), else 2 (planes from the tree or folded tables); log_in = log2 of the entries per table it
                                 * read: 16 * 2^log_in bytes of E plus 2 * ks * 8 * 2^log_in of L and R read, and 48 * 2^(log_in - 1)
                                 * written with kf = 1 */
#define SC_KIND_EXT_EQ_TABLE 41  /* ext_eq_table_kernel: eq(z, .) of a layer of sc_gp_prove_ext, z in K^k; log_in = k; reads the 2 k words
                                 * of the point, writes both planes, 16 * 2^k */
#define SC_KIND_EXT_FRACTION_TREE 42 /* a launch of sc_frac_create_ext from layer m = log_in of the fraction trees over K: kf = LV = 1..3,
                                 * ext_fr_tree_kernel<F, LV, LEAF_IN, ONES>; ks = the planes or base tables it read: 1 (m = n, all-ones
                                 * numerator: t), 2 (m = n: t and p), else 4 (the four planes of layer m); it reads ks * 8 * 2^m bytes and
                                 * writes the four planes of the layers m-1 .. m-LV, 32 * (2^m - 2^(m-LV)); kf = 0,
                                 * ext_fr_tree_tail_kernel, one block from a layer of <= 2^10 entries down to the root: 32 * (2^m - 1)
                                 * written */
#define SC_KIND_EXT_FRACTION_PASS 43 /* ext_fr_pass_kernel: one round of a layer of sc_frac_prove_ext; kf = 1 if it folded the previous
                                 * challenge; ks = the words per entry of L and R it read: 2 (layer n - 1, all-ones numerator: the
                                 * halves of t as base words), 4 (layer n - 1: the halves of t and p; or QL, QR in planes under an
                                 * all-ones numerator), 8 (QL, QR, PL, PR in planes); log_in = log2 of the entries per table it read:
                                 * 16 * 2^log_in bytes of E plus ks * 8 * 2^log_in read, and with kf = 1 both planes of every folded
                                 * table written: 80 * 2^(log_in - 1) with five tables, 48 * 2^(log_in - 1) with three.  The eq table
                                 * of a layer is a SC_KIND_EXT_EQ_TABLE record */
typedef struct sc_launch_record {
  int32_t kind;           /* SC_KIND_* */
  int32_t kf, ks;         /* variables folded / rounds served (meaning per kind above) */
  int32_t log_in;         /* log2 entries per input table */
  uint64_t bytes_read;    /* HBM bytes the launch must read */
  uint64_t bytes_written; /* HBM bytes the launch must write */
  double ms;              /* duration (HIP events on the context's stream) */
} sc_launch_record;
int sc_ctx_launch_log(sc_ctx* ctx, sc_launch_record* out, size_t cap, size_t* n_out, int reset);

/* ---- sharding (one process per GPU) ------------------------------ */

/* 128-byte RCCL unique id, created on rank 0 and broadcast by the caller. */
int sc_comm_unique_id(uint8_t id[128]);
/* Join an RCCL communicator.  After this call every table of ctx is the rank-th contiguous
 * shard (top log2(world) index bits = rank) of a table world times as long. */
int sc_ctx_comm_init_rccl(sc_ctx* ctx, const uint8_t id[128], int rank, int world);
/* Same sharding semantics with caller-supplied host collectives (used by tests and by
 * transports other than RCCL).  allreduce sums count uint64 words elementwise in place
 * across ranks (plain wrapping u64 adds; the library only ever sends 32-bit limbs);
 * allgather concatenates count words of every rank in rank order into recv. */
typedef int (*sc_allreduce_fn)(void* user, uint64_t* buf, size_t count);
typedef int (*sc_allgather_fn)(void* user, const uint64_t* send, uint64_t* recv, size_t count);
int sc_ctx_comm_init_host(sc_ctx* ctx, int rank, int world, sc_allreduce_fn allreduce,
                          sc_allgather_fn allgather, void* user);
/* Peer transport: the data plane of a one-node run without any collective launch.  Every rank exports a
 * small region of its HBM (an inbox for the per-pass round sums + arenas for gathers), maps every
 * other rank's region (HIP IPC, written over xGMI), and from then on the last workgroup of each sharded
 * pass exchanges its sums with the peers itself and hands the totals to its host (kernels.hpp, PeerX).
 * Up to 8 ranks.  Usage: export on every rank -> all-gather the 64-byte handles by any means (they are
 * plain bytes) -> connect with the world x 64 bytes in rank order.  connect verifies each mapped region's header
 * (same world and arena size, the expected rank), says hello to every peer and waits (up to "peer_connect_ms") until
 * every peer has said hello - by then all ranks have mapped, loaded their code and run a kernel - and then runs a
 * self-test through the real paths (an in-kernel exchange and a gather of known words); a node whose fine-grained
 * peer memory does not behave as the kernels assume fails here with SC_ERR_RCCL and the caller picks another
 * transport.  Afterwards the ranks must call the library in lockstep: an in-kernel wait for a peer is bounded by
 * "peer_spin_ms" (default 2 s).  Sharding semantics are those of sc_ctx_comm_init_rccl.  The challenges every rank
 * feeds to sc_prover_round / returns from `draw` must be identical; the exchange carries a digest of them and a
 * mismatch fails the pass with SC_ERR_STATE. */
int sc_ctx_comm_peer_export(sc_ctx* ctx, int rank, int world, uint8_t handle[64]);
int sc_ctx_comm_peer_connect(sc_ctx* ctx, const uint8_t* handles);
/* the same for ranks that are contexts of ONE process (threads; tests): peers[q] = rank q's context */
int sc_ctx_comm_peer_connect_local(sc_ctx* ctx, sc_ctx* const* peers);
int sc_ctx_comm_rank(const sc_ctx* ctx, int* rank, int* world);

/* ---- tables: DenseMultilinearExtension<F> on the device ------------------------------- */

/* DenseMultilinearExtension::from_evaluations_vec (matrix-multiplication/src/lib.rs:81,85) */
int sc_table_upload(sc_ctx* ctx, const uint64_t* host, size_t len, sc_table** out);
/* The same over device memory the caller already owns (its own kernels' output, another library's buffer, a mapping it made
 * with the HIP virtual-memory API): zero-copy and BORROWED - never written, never freed by the library (sc_table_free drops
 * the handle only); it must stay valid, and unchanged, while any table or prover made from it lives.  16-byte aligned. */
int sc_table_from_device(sc_ctx* ctx, const uint64_t* device_ptr, size_t len, sc_table** out);
/* Synthetic fill on the device:
 * t[i] = to_mont(splitmix64(seed + start + i) mod p), i < len. */
int sc_table_generate(sc_ctx* ctx, uint64_t seed, uint64_t start, size_t len, sc_table** out);
/* `.clone()` (every caller: Prover::new(g.clone()), matrix-multiplication/src/lib.rs:337) */
int sc_table_clone(sc_ctx* ctx, const sc_table* t, sc_table** out);
/* DenseMultilinearExtension::to_evaluations (matrix-multiplication/src/lib.rs:138-139) */
int sc_table_download(sc_ctx* ctx, const sc_table* t, uint64_t* host, size_t len);
size_t sc_table_len(const sc_table* t);
const uint64_t* sc_table_device_ptr(const sc_table* t);
int sc_table_free(sc_ctx* ctx, sc_table* t);

/* DenseMultilinearExtension::fix_variables(&r[..k]) (matrix-multiplication/src/lib.rs:83,86,
 * 104-105): new[b] = t[2b] + r*(t[2b+1]-t[2b]) per variable for SC_ORDER_LE; stride-half
 * pairing for SC_ORDER_BE.  *out has len >> k entries.  Input is not modified.  Asynchronous: the new table is
 * ready in the order of the context's stream (every sc_* call on the context is), sc_ctx_synchronize waits. */
int sc_table_fix_variables(sc_ctx* ctx, const sc_table* in, const uint64_t* r, size_t k, int order,
                           sc_table** out);
/* Polynomial::evaluate (matrix-multiplication/src/lib.rs:97-98) for SC_ORDER_LE;
 * vsbw_/cti_multilinear_from_evaluations (multilinear-extensions/src/lib.rs:6-48) for
 * SC_ORDER_BE.  n must equal log2(len) (times world when sharded: r then holds all n). */
int sc_table_evaluate(sc_ctx* ctx, const sc_table* t, const uint64_t* r, size_t n, int order,
                      uint64_t* out);
/* The same at m points in ONE pass over the table: points = m rows of n words, out = m values.  Callers that evaluate one
 * table several times - restrict_poly's k + 1 points on a line (gkr-protocol/src/lib.rs:291-321), a verifier's oracle
 * queries - pay one read of the table, one launch and one hand-off instead of m (batches of 16 points per launch, 8 on a
 * generic modulus; up to 4
 * points the pass stays memory-bound, beyond it is bound by the 2 m multiply-accumulates per 16 bytes).  Works on sharded
 * contexts and multi-device handles like sc_table_evaluate. */
int sc_table_evaluate_many(sc_ctx* ctx, const sc_table* t, const uint64_t* points, size_t m, size_t n, int order, uint64_t* out);
/* DenseMultilinearExtension::relabel(a, b, k) (matrix-multiplication/src/lib.rs:82) */
int sc_table_relabel(sc_ctx* ctx, const sc_table* in, size_t a, size_t b, size_t k, sc_table** out);

/* ---- product of two tables: matrix_multiplication::G --------------------------------- */

/* G::new (matrix-multiplication/src/lib.rs:77-92): A, B are 2^n x 2^n row-major tables of
 * 2^(2n) entries; point has 2n entries; outputs have 2^n entries. */
int sc_matmul_g_new(sc_ctx* ctx, const sc_table* A, const sc_table* B, size_t n,
                    const uint64_t* point, sc_table** a_out, sc_table** b_out);
/* C = A * B over the context's field (the product the MatMult protocol proves): A, B, C are 2^n x 2^n row-major
 * tables of 2^(2n) Montgomery words, column index in the low n bits (as in sc_matmul_g_new), so
 * C[i][j] = sum_k A[i][k] * B[k][j].  0 <= n <= 14.  The product runs on the int8 matrix cores from n = 5 (option
 * "matmul_path": 0 auto, 1 matrix cores from n = 4, 2 VALU); C comes from the context's pool and the scratch goes back to
 * it before the call returns.  SC_ERR_ARG: a null pointer, n > 14 or tables of another length; SC_ERR_UNSUPPORTED:
 * a sharded context or a multi-device handle. */
int sc_matmul(sc_ctx* ctx, const sc_table* A, const sc_table* B, size_t n, sc_table** C);
/* G::to_evaluations (matrix-multiplication/src/lib.rs:137-146): out[i] = a[i]*b[i] */
int sc_prod2_to_evaluations(sc_ctx* ctx, const sc_table* a, const sc_table* b, sc_table** out);
/* Prover::new's claim: sum_i a[i]*b[i] (sum-check-protocol/src/lib.rs:89) - never
 * materialises the product vector. */
int sc_prod2_sum(sc_ctx* ctx, const sc_table* a, const sc_table* b, uint64_t* out_c1);
/* G::to_univariate's three sums H(0),H(1),H(2) (matrix-multiplication/src/lib.rs:110-122) */
int sc_prod2_round_sums(sc_ctx* ctx, const sc_table* a, const sc_table* b, uint64_t out_e[3]);
/* G::fix_variables(&[r]) followed by to_univariate on the result, fused: one read of the
 * inputs, one write of the folded tables (matrix-multiplication/src/lib.rs:103-131). */
int sc_prod2_fold_and_sums(sc_ctx* ctx, const sc_table* a, const sc_table* b, const uint64_t r[1],
                           sc_table** a_out, sc_table** b_out, uint64_t out_e[3]);
/* G::evaluate (matrix-multiplication/src/lib.rs:96-101) */
int sc_prod2_evaluate(sc_ctx* ctx, const sc_table* a, const sc_table* b, const uint64_t* point,
                      size_t n, uint64_t* out);

/* ---- Prover<F, G> (sum-check-protocol/src/lib.rs:73-117) ------------------------------ */

/* Prover::new(g) (:88-97).  Borrows a and b (they must outlive the prover and are never
 * written, so the verifier's oracle copy needs no clone).  Computes c_1. */
int sc_prover_create(sc_ctx* ctx, const sc_table* a, const sc_table* b, sc_prover** out);
/* Prover::c_1 (:100-102) */
int sc_prover_c1(const sc_prover* pr, uint64_t* out);
/* Prover::num_vars (:114-116) */
int sc_prover_num_vars(const sc_prover* pr, size_t* out);
/* The schedule of a proof WITHOUT a device: the launches sc_prove would issue for a proof of num_vars variables on a
 * communicator of `world` ranks over `transport` (0 none, 1 RCCL, 2 host callbacks, 3 peer, 4 local: the devices of a
 * multi-device handle), computed by the same
 * planner the engine runs at every pass (pure host logic: callable - and tested - on a machine without a GPU).
 * Steps come in launch order; `kf` challenges are folded and `ks` rounds served by each; `log_in` = log2 entries per
 * table on a rank; `sharded` = its sums are exchanged across the ranks.  SC_PLAN_GATHER is the all-gather of both
 * tables (no rounds).  Returns SC_ERR_STATE for option combinations the engine would refuse. */
#define SC_PLAN_PASS 0       /* pass_kernel<kf,ks> */
#define SC_PLAN_GRID_PASS 1  /* wgrid_pass_kernel: up to five rounds */
#define SC_PLAN_RANK_PASS 2  /* rank_pass_kernel (peer transport): the rounds of the rank bits */
#define SC_PLAN_GATHER 3     /* all-gather of the shards; the proof goes on replicated */
#define SC_PLAN_HOST_TAIL 4  /* the host finishes: it folds the kf pending challenges of the <= 2^host_tail_log-entry tables the pass before
                              * wrote to pinned host memory (log_in = log2 entries per table and device) and serves every remaining
                              * round (ks) itself; no launch.  Always the last step */
#define SC_PLAN_GRAM_PASS 5  /* gram_pass_kernel: rounds 1..4 of a proof on tables (shards) of >= 2^gram_log entries */
#define SC_PLAN_WFOLD_PASS 6 /* wfold_pass_kernel: folds kf = 4 challenges (behind the matrix-core pass) and serves five rounds, or kf = 5 and ks = 3..5
                              * on tables of >= 2^wfold5_min_log entries: the streaming fold with a grid pass's cells */
/* ABI version of this header: bumped whenever a struct below grows or an enum is extended.  sc_abi_version()
 * returns the library's; a caller built against another major version must not pass structs.  Version 5 = round 5; version 6 =
 * round 6: the option block is initialised by sc_plan_options_init (a NEW symbol: the one-argument sc_plan_options_default of
 * version 4 and the two-argument one of version 5 are gone, so a caller built against either fails at link / load time instead
 * of handing the library a struct of another size - ADVICE r05). */
#define SC_ABI_VERSION 6
int sc_abi_version(void);
typedef struct sc_plan_options {   /* the context options the schedule depends on (sc_ctx_set_option names) */
  uint32_t struct_size;            /* sizeof(sc_plan_options) as the CALLER compiled it: set by sc_plan_options_init from its argument;
                                    * the library reads and writes no field beyond it (fields a caller's struct lacks take their defaults) */
  int32_t vars_per_pass, first_pass_vars, grid_pass, grid_log, grid_max_vars, grid_sharded, tail_log, use_mailbox, gram_log;
  int32_t host_tail_log;           /* since version 5 */
  int32_t wfold_log;               /* since version 5 */
  int32_t wfold_min_log;           /* since version 5 */
  int32_t wfold_always;            /* since version 5 */
  int32_t wfold5_min_log;          /* since version 5 */
} sc_plan_options;
typedef struct sc_plan_step {
  int32_t action, kf, ks, log_in, sharded;
} sc_plan_step;
/* struct_size = sizeof(sc_plan_options) at the call site */
void sc_plan_options_init(sc_plan_options* o, size_t struct_size);
int sc_plan_proof(const sc_plan_options* opt, size_t num_vars, int world, int transport, sc_plan_step* out, size_t cap,
                  size_t* n_out);

/* Prover::round(r_prev, j) (:105-112).  Rounds must be called in order j = 0,1,...;
 * r_prev is ignored for j == 0 like in the reference.  out_e = (H(0),H(1),H(2)) of the
 * round polynomial; sc_interpolate_quadratic turns it into the coefficients that
 * `univariate::SparsePolynomial` holds. */
int sc_prover_round(sc_prover* pr, uint64_t r_prev, size_t j, uint64_t out_e[3]);
int sc_prover_destroy(sc_prover* pr);

/* Whole interactive run in one call, the loop of mm_benchmark.rs:88-96: Prover::new, then
 * n rounds; after each round the challenge is obtained from `draw` (called on the host
 * with the round's three sums already read back - the verifier's rng.draw() at
 * sum-check-protocol/src/lib.rs:283, or a Fiat-Shamir hash).  draw == NULL uses the
 * synthetic challenger r_j = to_mont(splitmix64(seed_r + j + 1) mod p).
 * evals (3*n words) and challenges (n words) may be NULL.
 * Sharded contexts: every rank runs this call; `draw` is invoked on every rank and MUST return the same
 * challenge everywhere (derive it from the transcript, or draw on one rank and broadcast inside `draw`).
 * The peer transport checks this (digest in the exchange); the other transports do not. */
typedef uint64_t (*sc_draw_fn)(void* user, size_t round, const uint64_t evals[3]);
int sc_prove(sc_ctx* ctx, const sc_table* a, const sc_table* b, sc_draw_fn draw, void* user,
             uint64_t seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges);

/* A batch of `count` independent proofs of the same size, proved together: instance i is G_i = a[i] * b[i] (all tables 2^n
 * entries, the same n) and gets exactly what sc_prove(ctx, a[i], b[i], ..., seed_r[i], ...) gives it alone - c1[i], its
 * round polynomials evals[3*(i*n + j) ..] and challenges[i*n + j] (evals and challenges may be NULL).  This is not a random
 * linear combination of the instances: every transcript is bit-identical to its own sc_prove.  draw == NULL uses the synthetic
 * challenger of sc_prove over seed_r[i].  For 1 <= n <= 20 one launch (SC_KIND_BATCH_PASS) serves every instance at each pass
 * of the single-proof schedule (sc_plan_proof), so a batch makes as many launches as one proof.  Order of the draw calls:
 * round by round, and within a round in instance order 0 .. count-1; draw(user, i, j, evals) is called once instance i's
 * round-j polynomial is on the host.  For n = 0 and n > 20 the instances are proved one after another through sc_prove (the
 * same results, nothing gained: the draw calls then come instance by instance).  The tables are only read; one table may
 * appear in several instances.  Refused before any launch: count == 0, count > 1024 or a NULL array (SC_ERR_ARG), tables
 * that are not 2^n long or differ in length (SC_ERR_ARG), sharded contexts and multi-device handles (SC_ERR_UNSUPPORTED).
 * A draw that returns an unreduced challenge ends the call with SC_ERR_ARG, as in sc_prove. */
typedef uint64_t (*sc_draw_batch_fn)(void* user, size_t instance, size_t round, const uint64_t evals[3]);
int sc_prove_batch(sc_ctx* ctx, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_batch_fn draw, void* user,
                   const uint64_t* seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges);

/* ---- gkr_protocol::round_polynomial::W -----------------------
 *   f(b,c) = add_i(r_i,b,c) (W(b) + W(c)) + mul_i(r_i,b,c) W(b) W(c)
 * (gkr-protocol/src/round_polynomial.rs:13-44).  add/mul: tables of kb+kc variables indexed
 * (c << kb) | b; w_b: kb variables, w_c: kc variables (kb = kc = k_{i+1} when the sumcheck
 * starts; b variables are fixed first).
 * Sharded contexts: add/mul are this rank's rows of c (top log2(world) index bits = rank), w_b and w_c whole on
 * every rank.  sc_gkr_wiring builds exactly those shards (every rank passes the whole gate list and keeps the gates
 * of its rows: no exchange), the prover (sc_gkr_prover_*) and sc_gkr_w_round_sums / _fix_variables / _evaluate work
 * on them (sums exchanged like a pass's; fix_variables while the variables fixed stay shard-local, i.e. all of b
 * and all but the top log2(world) of c).  sc_gkr_w_to_evaluations returns, like every table of a sharded context, this rank's
 * contiguous shard of the result - whose order is b-major (the reference's), so the shard is a range of b and needs every
 * rank's rows of c: add and mul are gathered for the duration of the call (Prover::new only sums the result:
 * sc_gkr_prover_c1 gives that without it). */

/* add_i(r_i,.,.) and mul_i(r_i,.,.) of Prover::start_round (gkr-protocol/src/lib.rs:388-416)
 * straight from the gate list of layer i (2^k_i gates: type 0 = add, 1 = mul; inputs index
 * layer i+1, which has 2^k_next values); r_i has k_i entries.  Equals the reference's dense
 * predicate tables after fix_variables(r_i), without building them. */
int sc_gkr_wiring(sc_ctx* ctx, const int32_t* gate_type, const uint32_t* in0, const uint32_t* in1, size_t k_i,
                  size_t k_next, const uint64_t* r_i, sc_table** add_out, sc_table** mul_out);
/* W::to_evaluations (round_polynomial.rs:96-118): out[b*2^kc + c] = f(b,c) (the reference's order) */
int sc_gkr_w_to_evaluations(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                            const sc_table* w_c, sc_table** out);
/* W::to_univariate (round_polynomial.rs:78-90) as (H(0), H(1), H(2)): the round polynomial has
 * degree <= 2, so sc_interpolate_quadratic gives the coefficient vector the reference obtains
 * from its 4-point roots-of-unity interpolation. */
int sc_gkr_w_round_sums(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                        const sc_table* w_c, uint64_t out_e[3]);
/* W::fix_variables (round_polynomial.rs:59-76): r goes to add/mul and to w_b's variables first,
 * the rest to w_c. */
int sc_gkr_w_fix_variables(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                           const sc_table* w_c, const uint64_t* r, size_t k, sc_table** add_out,
                           sc_table** mul_out, sc_table** w_b_out, sc_table** w_c_out);
/* W::evaluate (round_polynomial.rs:48-57) */
int sc_gkr_w_evaluate(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                      const sc_table* w_c, const uint64_t* point, size_t n, uint64_t* out);
/* SumCheckProver<F, W<F>> (gkr-protocol/src/lib.rs:418-456 drives it): same contract as
 * sc_prover_*: create computes c_1, rounds in order, r_prev ignored at j = 0.  Two-phase linear-time form:
 * add and mul are streamed twice per LAYER (once for P(b) = sum_c add + mul W(c) and L(b) = sum_c add W(c), once
 * to fix b), the 2k rounds themselves run on 2^(k+1)-entry tables; round polynomials identical to the
 * reference's per-round walk. */
typedef struct sc_gkr_prover sc_gkr_prover;
int sc_gkr_prover_create(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b,
                         const sc_table* w_c, sc_gkr_prover** out);
/* The same prover straight from the gate list of layer i (arguments as sc_gkr_wiring) and the
 * 2^k_next values W_{i+1} of the next layer: add_i / mul_i have one non-zero per gate and W is
 * linear in them, so every round visits the 2^k_i gates instead of the 4^k_next table entries,
 * and the dense tables are never built.  Round polynomials are identical to the dense prover's. */
int sc_gkr_prover_create_sparse(sc_ctx* ctx, const int32_t* gate_type, const uint32_t* in0, const uint32_t* in1,
                                size_t k_i, size_t k_next, const uint64_t* r_i, const sc_table* w_next,
                                sc_gkr_prover** out);
/* the whole 2k-round W sumcheck in one call, challenges as in sc_prove (draw == NULL: the synthetic challenger);
 * evals has 3 * (kb + kc) words, challenges kb + kc */
int sc_gkr_prove(sc_ctx* ctx, const sc_table* add, const sc_table* mul, const sc_table* w_b, const sc_table* w_c,
                 sc_draw_fn draw, void* user, uint64_t seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges);
int sc_gkr_prover_c1(const sc_gkr_prover* pr, uint64_t* out);
int sc_gkr_prover_round(sc_gkr_prover* pr, uint64_t r_prev, size_t j, uint64_t out_e[3]);
int sc_gkr_prover_destroy(sc_gkr_prover* pr);

/* restrict_poly (gkr-protocol/src/lib.rs:291-321): the univariate
 * q(t) = W~(l(t)) for the line l(0) = b, l(1) = c (`line`, :278-289), as dense coefficients
 * out_coeffs[0..k] (degree <= k = number of variables).  Computed as the evaluations at t = 0..k - ONE
 * pass over the table for all k + 1 points (sc_table_evaluate_many) - plus exact interpolation on the host, instead
 * of the reference's O(k 2^k) product of linear factors; needs p > k.  Sharded contexts and multi-device handles: t is
 * split by its top index bits like every table there.  The reference returns a SparsePolynomial: drop zero terms. */
int sc_table_restrict_to_line(sc_ctx* ctx, const sc_table* t, const uint64_t* b, const uint64_t* c, size_t k,
                              uint64_t* out_coeffs);

/* ---- relaxed_pcs: the prover's grid evaluation and a SHA-256 Merkle commitment (relaxed-pcs/src/lib.rs) -----------------
 * Leaf order: all_multidimentional_values(m) (:46-63) lists the p^m points (v_0, .., v_{m-1}) of F^m sorted by canonical value,
 * v_0 the most significant digit: the point's leaf index is o = sum_j v_j p^(m-1-j), and its value is the dense LE MLE at it
 * (point[0] binds index bit 0 of the table; so variable 0 has input stride 1 but output stride p^(m-1)).
 * Merkle tree over N = 2^n leaves (this project's configuration: the reference's test hashes with Pedersen over JubJub):
 * leaf digest SHA-256(le64(canonical value)), node digest SHA-256(left || right) at every level; the root of a one-leaf tree is
 * its leaf's digest.  Digests are 32 bytes (SHA-256's own byte order).  Meant to equal arkworks' MerkleTree with Sha256 as both
 * hashes and IdentityDigestConverter; that byte identity is not pinned.  Sharded contexts and multi-device handles:
 * SC_ERR_UNSUPPORTED from every call below, before any work. */

/* :166-181: W~ at every point of F^m in that leaf order, t holding 2^m entries; *out has 2^ceil(log2 p^m) entries, Montgomery
 * like every table, zero past p^m.  One launch per variable (SC_KIND_GRID_EXTEND).  SC_ERR_ARG: t is not 2^m long;
 * SC_ERR_UNSUPPORTED: p^m > 2^28 (the Relaxed PCS also needs p > m for restrict_poly, sc_table_restrict_to_line). */
int sc_table_extend_grid(sc_ctx* ctx, const sc_table* t, size_t m, sc_table** out);
/* MerkleTree::new over the 2^n entries of t, n <= 28 (:185-186).  t is borrowed: it must outlive the tree, unchanged.  The
 * device keeps the levels from min(n, 4) up (N * 4 bytes of digests); an opening recomputes its 16-leaf bottom subtree. */
typedef struct sc_merkle_tree sc_merkle_tree;
int sc_merkle_commit(sc_ctx* ctx, const sc_table* t, sc_merkle_tree** out);
int sc_merkle_root(const sc_merkle_tree* tr, uint8_t root[32]);
/* depth = n = log2 N: the number of sibling digests in a path */
int sc_merkle_depth(const sc_merkle_tree* tr, size_t* depth);
/* MerkleTree::generate_proof (:207-213) for `count` leaves in one call: leaves[q] = the canonical value of leaf index[q],
 * paths[q][depth][32] its sibling digests bottom up.  To verify: h = leaf digest; at level l, h = H(h || s_l) if bit l of the
 * index is 0, else H(s_l || h); then h must equal the root.  SC_ERR_ARG: an index >= N. */
int sc_merkle_open(sc_ctx* ctx, const sc_merkle_tree* tr, const uint64_t* index, size_t count, uint64_t* leaves, uint8_t* paths);
int sc_merkle_tree_destroy(sc_ctx* ctx, sc_merkle_tree* tr);

/* ---- Ligero-style polynomial commitment: row Reed-Solomon encoding, column Merkle tree ----------------------------------
 * (Thaler's book, section 10.5; kernels/ligero.hpp states the contract.)  A table of 2^n entries is 2^(n - log_cols) rows of
 * 2^log_cols columns (row i = entries i 2^log_cols ..); every row, as the coefficients of a polynomial, is evaluated at the
 * L = 2^(log_cols + log_blowup) powers of w_L in natural order; leaf j of the tree is SHA-256 over column j of that matrix
 * (canonical values, 8 little-endian bytes each), nodes as sc_merkle_*.  w_L = w_max^(2^(s - log_cols - log_blowup)) with s the
 * 2-adicity of p - 1, w_max = g^((p-1)/2^s), g the smallest integer >= 2 with g^((p-1)/2) = -1: derived by the library.
 * SC_ERR_ARG: a null pointer, a table that is not 2^n long, log_cols > n, log_blowup not 1 or 2, more than 4 weight vectors, a
 * column index >= L, a commitment of another context.  SC_ERR_UNSUPPORTED: log_cols + log_blowup > 14 (one codeword has to fit the
 * LDS of a CU), n + log_blowup > 29, log_cols + log_blowup > s (the message names p and s), a sharded context or a multi-device
 * handle. */

/* the codeword matrix alone: *out has 2^(n + log_blowup) entries, E[i][j] at i L + j, Montgomery like every table */
int sc_rs_encode_rows(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_table** out);
/* encode and hash.  t is borrowed: it must outlive the commitment, unchanged (sc_ligero_combine_rows reads it).  The commitment
 * owns the codeword matrix and every level of the tree (at most 1 MiB). */
typedef struct sc_ligero sc_ligero;
int sc_ligero_commit(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_ligero** out);
int sc_ligero_root(const sc_ligero* lg, uint8_t root[32]);
int sc_ligero_shape(const sc_ligero* lg, size_t* log_rows, size_t* log_cols, size_t* log_blowup);
/* out[m][k] = sum_i weights[m][i] * t[i 2^log_cols + k] for count <= 4 vectors of 2^log_rows Montgomery words, in one read of the
 * table; out is count x 2^log_cols words.  count = 0 does nothing. */
int sc_ligero_combine_rows(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* weights, size_t count, uint64_t* out);
/* values[q][2^log_rows] = column cols[q] of the codeword matrix (Montgomery words), paths[q][log_cols + log_blowup][32] = the
 * sibling digests of leaf cols[q] bottom up (verified as sc_merkle_open's, from the column's leaf digest).  Indices may repeat. */
int sc_ligero_open_columns(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* cols, size_t count, uint64_t* values, uint8_t* paths);
int sc_ligero_destroy(sc_ctx* ctx, sc_ligero* lg);

/* Rows longer than the LDS of a CU: the same encoding and the same commitment for log_cols + log_blowup up to 24, through a
 * four-step transform (kernels/ligero_long.hpp): two launches, SC_KIND_RS_LONG, the second in place on the codeword matrix -
 * 8 * 2^n * (1 + 3 * 2^log_blowup) bytes of traffic in all.  Up to log_cols + log_blowup = 14 they run the single launch of the calls
 * above (SC_KIND_RS_ENCODE).  Every other limit and every error is as above, with SC_ERR_UNSUPPORTED for log_cols + log_blowup > 24
 * (the message names 2^24: there the stored tree is 1 GiB).  The commitment is an ordinary sc_ligero with code SC_CODE_RS:
 * sc_ligero_root / shape / code / combine_rows / open_columns / destroy serve it unchanged; its tree is 64 bytes per column. */
int sc_rs_encode_rows_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_table** out);
int sc_ligero_commit_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, sc_ligero** out);

/* ---- the same commitment over a linear-time expander code, for fields without two-adicity ------------------------------
 * (Thaler's book, section 10.5: Ligero with a linear-time code, as in Brakedown; kernels/expander.hpp states the contract,
 * "expander code 1".)  The code is systematic at rate 1/2: a row of 2^log_cols words encodes to itself followed by as many
 * check words, L = 2^(log_cols + 1), log_blowup = 1.  It needs only additions and multiplications by constants, so any prime
 * p > 63 is served, 2^64 - 59 included.  Its relative distance is NOT proved: no security level is claimed.
 * SC_ERR_ARG: a null pointer, a table that is not 2^n long, log_cols > n, an unknown code, log_blowup != 1 with
 * SC_CODE_EXPANDER.  SC_ERR_UNSUPPORTED: log_cols > 13 (one codeword has to fit the LDS of a CU), n + 1 > 29, p <= 63 (the
 * message names p), a sharded context or a multi-device handle. */
#define SC_CODE_RS 0
#define SC_CODE_EXPANDER 1
/* the codeword matrix alone: *out has 2^(n + 1) entries, E[i][j] at i L + j, Montgomery like every table */
int sc_xc_encode_rows(sc_ctx* ctx, const sc_table* t, size_t log_cols, sc_table** out);
/* sc_ligero_commit with the row code chosen: SC_CODE_RS is sc_ligero_commit itself.  The commitment is an ordinary sc_ligero:
 * sc_ligero_root / shape / combine_rows / open_columns / destroy serve it unchanged. */
int sc_ligero_commit_code(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, sc_ligero** out);
int sc_ligero_code(const sc_ligero* lg, int* code);
/* Expander-code rows longer than the LDS of a CU: the same code and the same commitment for log_cols up to 23 (codewords of up
 * to 2^24 words).  Above 13 the largest levels of the recursion run as launches over the codeword matrix in global memory
 * (kernels/expander_long.hpp; SC_KIND_XC_LONG records: a copy, one launch per such level on the way down, the in-LDS code
 * below them, one launch per level on the way up); up to 13 both run the single launch of the calls above
 * (SC_KIND_XC_ENCODE).  Every other limit and every error is as above, with SC_ERR_UNSUPPORTED for log_cols > 23 (the message
 * names 2^24: there the stored tree is 1 GiB).  sc_ligero_commit_code_long(SC_CODE_RS) is sc_ligero_commit_long itself; with
 * SC_CODE_EXPANDER the commitment is an ordinary sc_ligero of that code: sc_ligero_root / shape / code / combine_rows /
 * open_columns / destroy serve it unchanged. */
int sc_xc_encode_rows_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, sc_table** out);
int sc_ligero_commit_code_long(sc_ctx* ctx, const sc_table* t, size_t log_cols, size_t log_blowup, int code, sc_ligero** out);

/* ---- folded openings of the Reed-Solomon commitment: prove the combined row instead of sending it ----------------------
 * (kernels/rs_fold.hpp states the contract)  An opening of an sc_ligero with code SC_CODE_RS and
 * log_cols = c >= 1 at a point z: the prover sends v = u_z(z[:c]) and v_gamma = u_gamma(z[:c]) instead of the two combined rows,
 * and proves them by c rounds of the product sumcheck over (m, eq(z[:c])), m = u_z + beta u_gamma, interleaved with c folds of the
 * codeword U_0 = Enc(m) (Basefold); the layers U_1 .. U_(c-1) are committed with the commitment's column leaf (two rows) and tree.
 * With l0 = log_cols + log_blowup, w_l the contract's root of order 2^l: U_(i+1)[j] = even + alpha_i (odd - even), even =
 * (U_i[j] + U_i[j + M/2]) / 2, odd = (U_i[j] - U_i[j + M/2]) / (2 w_(l0-i)^j), M = 2^(l0-i), j < M / 2.  No security level is claimed.
 * SC_ERR_ARG: a null pointer, log_cols = 0 (use the plain opening), a commitment or an opening of another context, an index
 * >= L / 2, an unreduced point, gamma, beta, alpha or challenge, sc_rs_fold on a table of fewer than 4 words.
 * SC_ERR_UNSUPPORTED: an expander-code commitment, sc_rs_fold on more than 2^24 or more than 2^s words, a sharded context or a
 * multi-device handle.  SC_ERR_STATE: sc_ligero_fold_prove called twice, sc_ligero_fold_query before it. */

/* one fold alone: u holds M = 2^l words, 2 <= l <= min(24, s), a codeword in the contract's order; *out = its fold with alpha
 * at x = w_l^j, a new table of M / 2 words.  One launch of rs_fold_kernel<F, 1, 0> (SC_KIND_RS_FOLD, kf = 0). */
int sc_rs_fold(sc_ctx* ctx, const sc_table* u, uint64_t alpha, sc_table** out);
typedef struct sc_ligero_fold sc_ligero_fold;
/* the verifier's alpha_i for round i, called with the round's three sums and, for round >= 1, root_i (32 bytes; NULL at round 0) */
typedef uint64_t (*sc_draw_fold_fn)(void* user, size_t round, const uint64_t evals[3], const uint8_t* root);
/* steps 2 - 3: point = the n words of z, gamma = 2^log_rows words; claims[0] = v, claims[1] = v_gamma.  The two combined rows stay
 * on the device.  lg is borrowed: it must outlive the opening. */
int sc_ligero_fold_begin(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* point, const uint64_t* gamma, uint64_t claims[2],
                         sc_ligero_fold** out);
/* steps 4 - 7, once per opening: evals = 3 c words (every round's H(0), H(1), H(2)), roots = 32 (c - 1) bytes (root_1 ..
 * root_(c-1); may be NULL for c = 1), challenges = c words or NULL, *final_value = the word of U_c; `draw` is required and is
 * called once per round, in order.  One rs_fold_kernel<F, 1, 0 / 1> launch per round (SC_KIND_RS_FOLD); U_0 is encoded by the row encoder and not kept. */
int sc_ligero_fold_prove(sc_ctx* ctx, sc_ligero_fold* fd, uint64_t beta, sc_draw_fold_fn draw, void* user, uint64_t* evals,
                         uint8_t* roots, uint64_t* challenges, uint64_t* final_value);
/* step 9's layer openings for `count` indices q < L / 2 (the columns q and q + L / 2 come from sc_ligero_open_columns):
 * pairs[q][c - 1][2] = (U_i[j_i], U_i[j_i + M_i / 2]), j_i = q mod 2^(l0-i-1), for i = 1 .. c - 1 (Montgomery words);
 * paths[q][P][32], P = sum_{i=1}^{c-1} (l0 - i - 1): the layers in order, each path bottom up.  c = 1: nothing is written. */
int sc_ligero_fold_query(sc_ctx* ctx, const sc_ligero_fold* fd, const uint64_t* q, size_t count, uint64_t* pairs, uint8_t* paths);
int sc_ligero_fold_destroy(sc_ctx* ctx, sc_ligero_fold* fd);

/* ---- staged folded openings: up to three variables folded per committed layer ---------------
 * A schedule a_0 .. a_(S-1), 1 <= a_s <= 3, sum a_s = c: stage s starts at round i_s = a_0 + .. + a_(s-1) and owns the layer
 * U_(i_s) of M_s = 2^(l0 - i_s) words; the tree of a stage s >= 1 has M_s / 2^(a_s) leaves, leaf j = the column leaf of the words
 * U[j + t M_s / 2^(a_s)], t < 2^(a_s); a stage's fold is a_s successive folds of the opening above, bit for bit, in one launch
 * (SC_KIND_RS_FOLD_MANY).  kernels/rs_fold.hpp states the contract.  No security level is claimed, and the number of queries an
 * arity needs is not analysed.  On a handle begun with a schedule:
 *   sc_ligero_fold_prove  `draw` gets a non-NULL root exactly at the rounds i_s, s >= 1; roots = 32 (S - 1) bytes; one fold launch
 *                         and one tree per stage.
 *   sc_ligero_fold_query  q < L / 2^(a_0); pairs[q][W], W = sum_{s>=1} 2^(a_s): the words of leaf j_s = q mod (M_s / 2^(a_s)) of every
 *                         stage s >= 1 in order; paths[q][P][32], P = sum_{s>=1} (l0 - i_s - a_s).  The 2^(a_0) columns
 *                         q + t L / 2^(a_0) come from sc_ligero_open_columns.
 * sc_ligero_fold_begin is the schedule of c ones.  SC_ERR_ARG besides the above: a null or empty schedule, an entry outside
 * 1 .. 3, a sum other than c; sc_rs_fold_many: count outside 1 .. 3, fewer than 2^(count + 1) words, an unreduced alpha. */

/* count = 1 .. 3 successive folds in one launch: u holds M = 2^l words, count + 1 <= l <= min(24, s); *out = a new table of
 * M / 2^count words, word for word what `count` calls of sc_rs_fold give. */
int sc_rs_fold_many(sc_ctx* ctx, const sc_table* u, const uint64_t* alphas, size_t count, sc_table** out);
/* sc_ligero_fold_begin with the schedule arities[0 .. stages) stored in the opening */
int sc_ligero_fold_begin_staged(sc_ctx* ctx, const sc_ligero* lg, const uint64_t* point, const uint64_t* gamma, const int32_t* arities,
                                size_t stages, uint64_t claims[2], sc_ligero_fold** out);

/* ---- rank-1 constraint systems: the sparse products and the cubic sumcheck behind an argument for (A z) o (B z) = C z with a
 * committed witness (kernels/r1cs.hpp states the protocol) --------------------------------------
 * A, B, C are 2^log_rows x 2^log_cols, each a list of nnz[k] triples (row[k][e], col[k][e], val[k][e]); val is a Montgomery word
 * below p; triples with the same (row, col) add.  Limits: 1 <= log_rows <= 26, 2 <= log_cols <= 26, every nnz[k] < 2^31; one
 * device and one rank (SC_ERR_UNSUPPORTED on a sharded context or a multi-device handle, before anything else is looked at).
 * SC_ERR_ARG: a NULL argument, a shape outside the limits, a triple outside the matrix or with val >= p, a table of another
 * length, a word of tau, rho or rx that is not below p.  No security level and no zero knowledge are claimed. */
typedef struct sc_r1cs sc_r1cs;
/* Checks every triple on the host, sorts the row-major images of A, B, C and the one of [A^T | B^T | C^T] there (stable: the
 * entries of a row keep their order) and copies them into pool blocks; the host arrays may be freed on return. */
int sc_r1cs_create(sc_ctx* ctx, size_t log_rows, size_t log_cols, const uint32_t* const row[3], const uint32_t* const col[3],
                   const uint64_t* const val[3], const size_t nnz[3], sc_r1cs** out);
int sc_r1cs_destroy(sc_ctx* ctx, sc_r1cs* r);
/* az, bz, cz = A z, B z, C z: new tables of 2^log_rows words; z has 2^log_cols.  Per matrix the output is zeroed and two launches
 * follow on the stream (SC_KIND_SPMV: the product, kf = 0, then its carries, kf = 1; none for an empty matrix). */
int sc_r1cs_mul(sc_ctx* ctx, const sc_r1cs* r, const sc_table* z, sc_table** az, sc_table** bz, sc_table** cz);
/* out[y] = sum_k rho[k] sum_i eq(rx, i) M_k[i][y]: a new table of 2^log_cols words; rx has log_rows words.  One product over the
 * three transposed images side by side against the vector (rho_A eq, rho_B eq, rho_C eq), and its carries (ks = 1). */
int sc_r1cs_bind_rows(sc_ctx* ctx, const sc_r1cs* r, const uint64_t* rx, const uint64_t rho[3], sc_table** out);
/* The cubic sumcheck over sum_x eq(tau, x) (a(x) b(x) - c(x)) for three tables of equal length 2^s >= 2, variable 0 first: one
 * launch per round (SC_KIND_ZEROCHECK).  *c1 = H_0(0) + H_0(1) - whatever it is: refusing c1 != 0 is the verifier's part.
 * evals (4 s words, may be NULL): every round's H(0), H(1), H(2), H(3); challenges (s words, may be NULL); finals = the three
 * tables folded by every challenge.  draw(user, round, evals) returns the round's challenge, a word below p; draw == NULL: the
 * synthetic challenger of sc_prove over seed_r.  The tables are not modified.  SC_ERR_UNSUPPORTED: p <= 3 (the cubic through
 * 0, 1, 2, 3 needs 2 and 3 invertible). */
typedef uint64_t (*sc_draw4_fn)(void* user, size_t round, const uint64_t evals[4]);
int sc_zerocheck_prove(sc_ctx* ctx, const sc_table* a, const sc_table* b, const sc_table* c, const uint64_t* tau, sc_draw4_fn draw,
                       void* user, uint64_t seed_r, uint64_t* c1, uint64_t* evals, uint64_t* challenges, uint64_t finals[3]);

/* ---- the grand product argument: the product of the 2^n entries of a table is P, reduced to one evaluation claim about the
 * table's multilinear extension (kernels/grand_product.hpp states the protocol) -----------------
 * Tree: V_n = t, V_k[x] = V_(k+1)[x] V_(k+1)[x + 2^k], x < 2^k; P = V_0[0].  Layer k = 0 .. n-1 of the proof is a cubic sumcheck
 * of k rounds over sum_x eq(z_k, x) L_k(x) R_k(x) = c_k with L_k, R_k the two halves of V_(k+1), variable 0 first, four values
 * H(0..3) per round; then the finals l = L~(r), r' = R~(r), the combining challenge rho_k, c_(k+1) = l + rho_k (r' - l) and
 * z_(k+1) = (r, rho_k).  After layer n-1 the claim is t~(z_n) = c_n: check it with sc_table_evaluate or an opening of a
 * commitment to t.  Limits: 1 <= n <= 28, one device and one rank (SC_ERR_UNSUPPORTED on a sharded context or a multi-device
 * handle, before anything else is looked at), p > 3 (SC_ERR_UNSUPPORTED: the cubic through 0, 1, 2, 3 needs 2 and 3
 * invertible).  SC_ERR_ARG: a NULL argument, a table of fewer than two or more than 2^28 entries, a layer k >= n, a word of a
 * challenge, alpha or beta that is not below p.  No security level, no zero knowledge and no Fiat-Shamir are claimed. */
typedef struct sc_gp sc_gp;
/* Builds the tree (SC_KIND_PRODUCT_TREE launches) into one pool block of 2^n words, layer k at words [2^k, 2^(k+1)); t is
 * borrowed until sc_gp_destroy and never written. */
int sc_gp_create(sc_ctx* ctx, const sc_table* t, sc_gp** out);
int sc_gp_destroy(sc_ctx* ctx, sc_gp* g);
/* *out = V_0[0] */
int sc_gp_product(const sc_gp* g, uint64_t* out);
/* a copy of V_k, 0 <= k < n: a new table of 2^k words */
int sc_gp_layer(sc_ctx* ctx, const sc_gp* g, size_t k, sc_table** out);
/* round < layer: msg = H(0..3) of that round, returns r_round; round == layer: msg = (l, r'), returns rho_layer.  A word below p. */
typedef uint64_t (*sc_draw_gp_fn)(void* user, size_t layer, size_t round, const uint64_t* msg);
/* The n layers.  evals (4 n (n-1) / 2 words, may be NULL): every round's four values, layer by layer; finals (2 n words):
 * (l, r') of every layer; challenges (n (n-1) / 2 + n words, may be NULL): in protocol order, the rounds' challenges of a layer
 * and then its rho; point (n words) = z_n; *claim = c_n.  draw == NULL: the synthetic challenger of sc_prove over seed_r, one
 * draw per round and one per rho in protocol order.  One launch per round of a layer (SC_KIND_PRODUCT_PASS) down to the
 * hand-over to the host (option "gp_host_log"). */
int sc_gp_prove(sc_ctx* ctx, const sc_gp* g, sc_draw_gp_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                uint64_t* challenges, uint64_t* point, uint64_t* claim);
/* out[i] = alpha t[i] + beta: a new table of the length of t (at least two entries) */
int sc_table_affine(sc_ctx* ctx, const sc_table* t, uint64_t alpha, uint64_t beta, sc_table** out);

/* ---- LogUp lookups: the sum of 2^n fractions p_i / q_i is P / Q, reduced to one evaluation claim about p and one about q
 * (kernels/fraction.hpp states the protocol) -----------------------------------------------------
 * Trees: layer n = (p, q); p_k[x] = p_(k+1)[x] q_(k+1)[x + 2^k] + p_(k+1)[x + 2^k] q_(k+1)[x], q_k[x] = q_(k+1)[x] q_(k+1)[x + 2^k],
 * x < 2^k; (P, Q) = (p_0[0], q_0[0]).  Layer k = 0 .. n-1 of the proof: V's lambda_k (k >= 1), a cubic sumcheck of k rounds over
 * sum_x eq(z_k, x) (PL QR + PR QL + lambda_k QL QR)(x) = a_k + lambda_k b_k with PL, PR, QL, QR the halves of layer k+1, variable 0
 * first, four values H(0..3) per round; then the finals pl, pr, ql, qr, the combining challenge rho_k, a_(k+1) = pl + rho_k (pr - pl),
 * b_(k+1) = ql + rho_k (qr - ql) and z_(k+1) = (r, rho_k).  After layer n-1 the claims are p~(z_n) = a_n and q~(z_n) = b_n.
 * p == NULL: the numerator is all ones (the top layer reads three tables, not five; its finals pl = pr = 1; a_n must be 1).
 * Limits: 1 <= n <= 28, one device and one rank (SC_ERR_UNSUPPORTED on a sharded context or a multi-device handle, before
 * anything else is looked at), p > 3 (SC_ERR_UNSUPPORTED).  SC_ERR_ARG: a NULL argument, tables of different lengths, of fewer
 * than two or more than 2^28 entries, a layer k >= n, a challenge that is not a word below p.  No security level, no zero
 * knowledge and no Fiat-Shamir are claimed. */
typedef struct sc_frac sc_frac;
/* Builds both trees (SC_KIND_FRACTION_TREE launches) into two pool blocks of 2^n words, layer k at words [2^k, 2^(k+1)); p (may be
 * NULL: all ones) and q are borrowed until sc_frac_destroy and never written. */
int sc_frac_create(sc_ctx* ctx, const sc_table* p, const sc_table* q, sc_frac** out);
int sc_frac_destroy(sc_ctx* ctx, sc_frac* g);
/* out = (P, Q) */
int sc_frac_root(const sc_frac* g, uint64_t out[2]);
/* a copy of layer k, 0 <= k < n, of p (which = 0) or q (which = 1): a new table of 2^k words */
int sc_frac_layer(sc_ctx* ctx, const sc_frac* g, size_t k, int which, sc_table** out);
/* round < layer: msg = H(0..3) of that round, returns r_round; round == layer: msg = (pl, pr, ql, qr), returns rho_layer;
 * round == layer + 1: msg = NULL, returns lambda of layer + 1 (not called after the last layer).  A word below p. */
typedef uint64_t (*sc_draw_frac_fn)(void* user, size_t layer, size_t round, const uint64_t* msg);
/* The n layers.  evals (4 n (n-1) / 2 words, may be NULL): every round's four values, layer by layer; finals (4 n words):
 * (pl, pr, ql, qr) of every layer; challenges (n (n-1) / 2 + 2 n - 1 words, may be NULL): as they were drawn - rho_0, then per
 * layer k >= 1 lambda_k, its rounds' challenges and rho_k; point (n words) = z_n; claims = (a_n, b_n).  draw == NULL: the
 * synthetic challenger of sc_prove over seed_r, one draw per lambda, per round and per rho in that order.  One launch per round of a
 * layer (SC_KIND_FRACTION_PASS) down to the hand-over to the host (option "fr_host_log"). */
int sc_frac_prove(sc_ctx* ctx, const sc_frac* g, sc_draw_frac_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                  uint64_t* challenges, uint64_t* point, uint64_t claims[2]);
/* The multiplicities of a lookup: w (2^n entries), t (2^m entries), idx_host (2^n host words of 32 bits).  Every i with
 * idx_host[i] < 2^m and w[i] == t[idx_host[i]] adds one to entry idx_host[i] of *mult, a new table of t's length (Montgomery words
 * of the counts); every other i adds one to *mismatches and is not counted (SC_KIND_LOOKUP_COUNT).  SC_ERR_UNSUPPORTED:
 * p <= 2^max(n, m) (a count must be a field word). */
int sc_lookup_count(sc_ctx* ctx, const sc_table* w, const sc_table* t, const uint32_t* idx_host, sc_table** mult, uint64_t* mismatches);

/* ---- SPARK over LogUp: a committed sparse matrix and the proof of v = sum_k val_k U[row_k] W[col_k] (DESIGN.md section 9 item 18;
 * kernels/spark.hpp states the protocol) ---------------------------------------------------------------------------------------
 * M in F^(2^a x 2^b) is a list of nnz >= 1 triples, padded with (0, 0, 0) to N = 2^l entries, l = max(1, ceil(log2 nnz)); equal
 * (row, col) pairs add.  The object holds five tables: row and col (the indices as field words) and val, of l variables, and the
 * counts cr[i] = #{k < N : row_k = i} (a variables) and cc[j] = #{k < N : col_k = j} (b variables); the padding counts in cr[0]
 * and cc[0].  Limits: 1 <= l, a, b <= 28; p > 3 and p > 2^max(l, a, b) (SC_ERR_UNSUPPORTED: indices and counts must be field words);
 * one device and one rank (SC_ERR_UNSUPPORTED on a sharded context or a multi-device handle, before anything else is looked at).
 * SC_ERR_ARG: a NULL argument, an empty list, a triple outside the matrix or with a value that is not a word below p, tables of
 * the wrong length, a challenge that is not a word below p.  No security level, no zero knowledge and no Fiat-Shamir are claimed. */
typedef struct sc_spark sc_spark;
#define SC_SPARK_ROW 0
#define SC_SPARK_COL 1
#define SC_SPARK_VAL 2
#define SC_SPARK_CR 3
#define SC_SPARK_CC 4
/* Validates every triple on the host, pads, uploads, and builds row, col, cr and cc on the device (SC_KIND_SPARK_INDEX launches);
 * the host arrays may be freed on return.  A failure gives every block back. */
int sc_spark_create(sc_ctx* ctx, size_t log_rows, size_t log_cols, const uint32_t* row, const uint32_t* col, const uint64_t* val, size_t nnz,
                    sc_spark** out);
int sc_spark_destroy(sc_ctx* ctx, sc_spark* sp);
/* a copy of row, col, val, cr or cc (which = SC_SPARK_*) as a new table */
int sc_spark_table(sc_ctx* ctx, const sc_spark* sp, int which, sc_table** out);
/* er[k] = u[row_k] and ec[k] = w[col_k], k < N: two new tables from one launch (SC_KIND_SPARK_GATHER); u has 2^a entries, w 2^b */
int sc_spark_gather(sc_ctx* ctx, const sc_spark* sp, const sc_table* u, const sc_table* w, sc_table** er, sc_table** ec);
/* The denominators of one indexed lookup, dim = 0 (row) or 1 (col): den_w[k] = alpha - idx_k - beta e[k], k < N, and
 * den_t[i] = alpha - i - beta t[i] over t's 2^a (2^b) entries: two new tables, one launch each (SC_KIND_SPARK_TUPLE) */
int sc_spark_denominators(sc_ctx* ctx, const sc_spark* sp, int dim, const sc_table* t, const sc_table* e, uint64_t alpha, uint64_t beta,
                          sc_table** den_w, sc_table** den_t);
/* The cubic sumcheck over sum_x a(x) b(x) c(x), three tables of 2^n entries, 1 <= n <= 28, which are never written: n rounds of four
 * values H(0..3), variable 0 first.  *c1 = H_0(0) + H_0(1); evals (4 n words, may be NULL); challenges (n words, may be NULL);
 * finals = the three tables' extensions at the challenges.  draw == NULL: the synthetic challenger of sc_prove over seed_r.  One
 * launch per round (gp_pass_kernel, SC_KIND_PRODUCT_PASS) down to the hand-over to the host (option "gp_host_log"); the transcript
 * is the same at every value of the option. */
int sc_product3_prove(sc_ctx* ctx, const sc_table* a, const sc_table* b, const sc_table* c, sc_draw4_fn draw, void* user, uint64_t seed_r,
                      uint64_t* c1, uint64_t* evals, uint64_t* challenges, uint64_t finals[3]);
/* eq(r, .) over n variables, 1 <= n <= 28, as a new table of 2^n words: out[i] = prod_j (bit_j(i) ? r[j] : 1 - r[j]) */
int sc_table_eq(sc_ctx* ctx, const uint64_t* r, size_t n, sc_table** out);
/* The row weights of the combined matrix of an R1CS instance (row k 2^s + i = row i of matrix k): a new table of 2^(s+2) words,
 * (rho_A eq(rx, .), rho_B eq(rx, .), rho_C eq(rx, .), 0) - the vector sc_r1cs_bind_rows multiplies by, with a zero last quarter */
int sc_r1cs_row_weights(sc_ctx* ctx, const sc_r1cs* r, const uint64_t* rx, const uint64_t rho[3], sc_table** out);

/* ---- batched openings: many evaluation claims about committed tables of one shape, one joint opening (DESIGN.md section 9 item 19;
 * kernels/multiopen.hpp states the protocol) ------------------------------------------------------------------------------------
 * One device and one rank (SC_ERR_UNSUPPORTED on a sharded context or a multi-device handle, before anything else is looked at).
 * SC_ERR_ARG, before any launch: a NULL argument, a count out of range, tables of different or non-power-of-two length, a point or
 * coefficient word that is not below p. */
/* out[x] = sum_{k < count} coeffs[k] eq(points[k], x) as a new table of 2^n words; points: `count` rows of n Montgomery words;
 * 1 <= count <= 16, 1 <= n <= 28.  One launch (eq_sum_kernel, SC_KIND_EQ_SUM): one multiply-add per entry and point. */
int sc_table_eq_sum(sc_ctx* ctx, const uint64_t* points, const uint64_t* coeffs, size_t count, size_t n, sc_table** out);
/* The sumcheck over sum_x sum_{t < count} a[t](x) b[t](x) with ONE sequence of challenges shared by all pairs, 1 <= count <= 8, all
 * tables 2^n entries, 1 <= n <= 28, never written (a table may appear in several pairs): n rounds of three values H(0..2), variable 0
 * first.  This is not sc_prove_batch, whose instances are independent proofs.  *c1 = H_0(0) + H_0(1); evals (3 n words, may be
 * NULL); challenges (n words, may be NULL); finals_a[t], finals_b[t] = the tables' extensions at the challenges (count words each).
 * draw == NULL: the synthetic challenger of sc_product3_prove over seed_r; a challenge that is not below p ends the call with
 * SC_ERR_ARG.  One launch per round (sumprod_pass_kernel, SC_KIND_SUMPROD_PASS) down to the hand-over to the host (option
 * "gp_host_log"); the transcript is the same at every value of the option. */
int sc_sumprod_prove(sc_ctx* ctx, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_fn draw, void* user, uint64_t seed_r,
                     uint64_t* c1, uint64_t* evals, uint64_t* challenges, uint64_t* finals_a, uint64_t* finals_b);

/* ---- challenges from a quadratic extension field (kernels/ext_sumprod.hpp states the conventions) ----
 * K = F_p[X] / (X^2 - w): w is a quadratic non-residue of F_p, a Montgomery word, checked on the host (w^((p-1)/2) = p - 1, else
 * SC_ERR_ARG before any launch).  An element of K is two consecutive Montgomery words (c0, c1), meaning c0 + c1 X.  The tables are
 * base-field tables; the challenges, the round values and the finals are elements of K.  One device and one rank (SC_ERR_UNSUPPORTED
 * on a sharded context or a multi-device handle, before anything else is looked at). */
/* a round's challenge: msg = H(0).c0, H(0).c1, H(1).c0, H(1).c1, H(2).c0, H(2).c1; out receives (c0, c1), both below p */
typedef void (*sc_draw_ext_fn)(void* user, size_t round, const uint64_t msg[6], uint64_t out[2]);
/* sc_sumprod_prove with challenges from K: the same arguments, limits and refusals (1 <= count <= 8, all tables 2^n entries,
 * 1 <= n <= 28, never written, a table may appear in several pairs), and SC_ERR_ARG for a bad w or a challenge component that is
 * not below p.  n rounds of six words, variable 0 first; c1 = (H_0(0) + H_0(1), 0); evals (6 n words, may be NULL); challenges
 * (2 n words, may be NULL); finals_a, finals_b = the tables' extensions at the challenges (2 count words each).  draw == NULL: the
 * synthetic challenger r_j = (to_mont(splitmix64(seed_r + 2 j + 1) mod p), to_mont(splitmix64(seed_r + 2 j + 2) mod p)).  Round 0
 * is the launch of sc_sumprod_prove (SC_KIND_SUMPROD_PASS, kf = 0), every later device round one ext_sumprod_pass_kernel launch
 * (SC_KIND_SUMPROD_EXT_PASS), down to the hand-over to the host (option "gp_host_log", as in sc_sumprod_prove); the transcript is
 * the same at every value of the option. */
int sc_sumprod_prove_ext(sc_ctx* ctx, uint64_t w, size_t count, const sc_table* const* a, const sc_table* const* b, sc_draw_ext_fn draw, void* user,
                         uint64_t seed_r, uint64_t c1[2], uint64_t* evals, uint64_t* challenges, uint64_t* finals_a, uint64_t* finals_b);
/* The multilinear extension of a base-field table of 2^n entries at a point of K^n (2 n words, coordinate 0 first = variable 0),
 * 1 <= n <= 28, by the prover's own folds (ext_fold_kernel, SC_KIND_SUMPROD_EXT_PASS records with ks = 0) down to the host
 * hand-over of option "gp_host_log"; no table of 2^n weights is built.  SC_ERR_ARG: a bad w, a component that is not below p, a
 * table that has not 2^n entries. */
int sc_table_evaluate_ext(sc_ctx* ctx, uint64_t w, const sc_table* t, const uint64_t* point, size_t n, uint64_t out[2]);

/* ---- the grand product argument over K (kernels/ext_grand_product.hpp states the protocol) ----
 * The protocol of sc_gp_* with every element in K = F_p[X] / (X^2 - w): the leaves are V_n[i] = beta + alpha t[i] for a base-field
 * table t of 2^n entries, 1 <= n <= 28, and alpha, beta in K, alpha != 0; they are never stored.  The tree, the round values, the
 * challenges, the finals, the point and the claim are elements of K, two consecutive Montgomery words each.  One device and one
 * rank (SC_ERR_UNSUPPORTED on a sharded context or a multi-device handle, before anything else is looked at); p <= 3 is
 * SC_ERR_UNSUPPORTED; SC_ERR_ARG: a NULL argument, a tree of another context, a table of fewer than 2 or more than 2^28 entries, a
 * bad w (as sc_sumprod_prove_ext), a component of alpha or beta that is not below p, alpha = (0, 0). */
typedef struct sc_gp_ext sc_gp_ext;
/* The product tree over K (SC_KIND_EXT_PRODUCT_TREE; options "gp_tree_lv" as in sc_gp_create): one pool block of 2 * 2^n words.
 * `t` is borrowed until sc_gp_destroy_ext and never written. */
int sc_gp_create_ext(sc_ctx* ctx, uint64_t w, const sc_table* t, const uint64_t alpha[2], const uint64_t beta[2], sc_gp_ext** out);
int sc_gp_destroy_ext(sc_ctx* ctx, sc_gp_ext* g);
/* P = V_0[0] in K */
int sc_gp_product_ext(const sc_gp_ext* g, uint64_t out[2]);
/* copies of the two planes of V_k, k < n, as base tables of 2^k words (the c0 words, the c1 words): new tables the caller frees */
int sc_gp_layer_ext(sc_ctx* ctx, const sc_gp_ext* g, size_t k, sc_table** c0, sc_table** c1);
/* round < layer: msg = the eight words H(0).c0, H(0).c1, .., H(3).c1 of that round, out receives its challenge; round == layer:
 * msg = the four words of (l, r'), out receives rho; both components below p */
typedef void (*sc_draw_gp_ext_fn)(void* user, size_t layer, size_t round, const uint64_t* msg, uint64_t out[2]);
/* The n layers.  evals (may be NULL): 8 words per round, 8 k (k - 1) / 2 words before layer k; finals: 4 per layer; challenges (may
 * be NULL): 2 k (k + 1) / 2 words before layer k, the layer's rounds, then rho; point: 2 n words, z_n; claim: 2 words, c_n, so that
 * t~(z_n) = (c_n - beta) / alpha.  draw == NULL: the synthetic challenger, draw number d = 0, 1, .. in protocol order being
 * (to_mont(splitmix64(seed_r + 2 d + 1) mod p), to_mont(splitmix64(seed_r + 2 d + 2) mod p)).  A challenge with a component that
 * is not below p ends the call with SC_ERR_ARG.  One eq table (SC_KIND_EXT_EQ_TABLE) and one launch per round
 * (SC_KIND_EXT_PRODUCT_PASS) for every layer above the hand-over to the host (option "gp_host_log", as in sc_gp_prove); the
 * transcript is the same at every value of the option. */
int sc_gp_prove_ext(sc_ctx* ctx, const sc_gp_ext* g, sc_draw_gp_ext_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                    uint64_t* challenges, uint64_t* point, uint64_t* claim);

/* ---- LogUp's fraction sums over K (kernels/ext_fraction.hpp states the protocol) ----
 * The protocol of sc_frac_* with every element in K = F_p[X] / (X^2 - w).  The leaves are never stored: the denominators are
 * q_i = beta + alpha t[i] for a base-field table t of 2^n entries, 1 <= n <= 28, and alpha, beta in K, alpha != 0; the numerators
 * are a base-field table p embedded as (p_i, 0), or all ones (p == NULL: the top layer reads three tables, not five; its finals
 * pl = pr = (1, 0); a_n must be (1, 0)).  The trees, the root, the round values, the challenges, the finals, the point and the
 * claims are elements of K, two consecutive Montgomery words each.  One device and one rank (SC_ERR_UNSUPPORTED on a sharded
 * context or a multi-device handle, before anything else is looked at); p <= 3 is SC_ERR_UNSUPPORTED; SC_ERR_ARG: a NULL argument,
 * a tree of another context, tables of different lengths, of fewer than 2 or more than 2^28 entries, a layer k >= n, a bad w (as
 * sc_sumprod_prove_ext), a component of alpha or beta that is not below p, alpha = (0, 0). */
typedef struct sc_frac_ext sc_frac_ext;
/* The trees over K (SC_KIND_EXT_FRACTION_TREE; option "fr_tree_lv" as in sc_frac_create): one pool block of 4 * 2^n words, the heaps
 * p.c0, p.c1, q.c0, q.c1.  `p` (may be NULL) and `t` are borrowed until sc_frac_destroy_ext and never written. */
int sc_frac_create_ext(sc_ctx* ctx, uint64_t w, const sc_table* p, const sc_table* t, const uint64_t alpha[2], const uint64_t beta[2],
                       sc_frac_ext** out);
int sc_frac_destroy_ext(sc_ctx* ctx, sc_frac_ext* g);
/* out = (P.c0, P.c1, Q.c0, Q.c1) */
int sc_frac_root_ext(const sc_frac_ext* g, uint64_t out[4]);
/* copies of the two planes of layer k, k < n, of p (which = 0) or q (which = 1) as base tables of 2^k words (the c0 words, the c1
 * words): new tables the caller frees */
int sc_frac_layer_ext(sc_ctx* ctx, const sc_frac_ext* g, size_t k, int which, sc_table** c0, sc_table** c1);
/* round < layer: msg = the eight words H(0).c0, H(0).c1, .., H(3).c1 of that round, out receives its challenge; round == layer:
 * msg = the eight words of (pl, pr, ql, qr), out receives rho_layer; round == layer + 1: msg = NULL, out receives lambda of
 * layer + 1 (not called after the last layer).  Both components below p. */
typedef void (*sc_draw_frac_ext_fn)(void* user, size_t layer, size_t round, const uint64_t* msg, uint64_t out[2]);
/* The n layers.  evals (may be NULL): 8 words per round, 8 k (k - 1) / 2 words before layer k; finals: 8 per layer, (pl, pr, ql, qr);
 * challenges (2 (n (n-1) / 2 + 2 n - 1) words, may be NULL): two words each as they were drawn, in sc_frac_prove's order - rho_0,
 * then per layer k >= 1 lambda_k, its rounds' challenges and rho_k; point: 2 n words, z_n; claims: four words, (a_n, b_n), so that
 * p~(z_n) = a_n and t~(z_n) = (b_n - beta) / alpha.  draw == NULL: the synthetic challenger, draw number d = 0, 1, .. in that order
 * being (to_mont(splitmix64(seed_r + 2 d + 1) mod p), to_mont(splitmix64(seed_r + 2 d + 2) mod p)).  A challenge with a component
 * that is not below p ends the call with SC_ERR_ARG.  One eq table (SC_KIND_EXT_EQ_TABLE) and one launch per round
 * (SC_KIND_EXT_FRACTION_PASS) for every layer above the hand-over to the host (option "fr_host_log", as in sc_frac_prove); the
 * transcript is the same at every value of "fr_host_log", "fr_tree_lv" and "max_blocks". */
int sc_frac_prove_ext(sc_ctx* ctx, const sc_frac_ext* g, sc_draw_frac_ext_fn draw, void* user, uint64_t seed_r, uint64_t* evals, uint64_t* finals,
                      uint64_t* challenges, uint64_t* point, uint64_t claims[4]);

/* ---- gkr_protocol::circuit::Circuit on the device, and the whole GKR prover over it ----------------------------------
 * A circuit lives on ONE context of one device and one rank: sharded contexts (world > 1) and multi-device handles get
 * SC_ERR_UNSUPPORTED from every call below, before the circuit is looked at.  Limits are the sparse prover's:
 * k[i] <= 30, 1 <= k[i+1] <= 26. */
typedef struct sc_circuit sc_circuit;
/* circuit.rs:72-124: `depth` layers, layers[0] = outputs.  Layer i has 2^k[i] gates reading layer i+1;
 * k[depth] = number of input variables.  Gate arrays as for sc_gkr_wiring (type 0 = add, 1 = mul).
 * Checked once here (SC_ERR_ARG naming the layer and the gate), then copied to the device; the host arrays may be freed
 * on return.  The circuit must outlive every prover made from it (sc_gkr_prover_create_circuit). */
int sc_circuit_create(sc_ctx* ctx, size_t depth, const size_t* k /* depth + 1 */, const int32_t* const* gate_type,
                      const uint32_t* const* in0, const uint32_t* const* in1, sc_circuit** out);
int sc_circuit_destroy(sc_ctx* ctx, sc_circuit* c);
/* Circuit::evaluate (circuit.rs:99-124): values[i] (i < depth) = layer i's 2^k[i] values, new tables the caller frees;
 * `input` has 2^k[depth] entries.  One circuit_layer_kernel launch per layer, from the input up, on the context's stream
 * (no host sync between them). */
int sc_circuit_evaluate(sc_ctx* ctx, const sc_circuit* c, const sc_table* input, sc_table** values);
/* sc_gkr_prover_create_sparse for layer i (lib.rs:373-436), from the device-resident gate list: no host check, no copy,
 * no sync.  w_next = layer i+1's values (2^k[i+1] entries), r_i has k[i] entries.  i >= depth: SC_ERR_ARG. */
int sc_gkr_prover_create_circuit(sc_ctx* ctx, const sc_circuit* c, size_t i, const uint64_t* r_i,
                                 const sc_table* w_next, sc_gkr_prover** out);
/* The prover's side of the whole protocol (lib.rs:324-474, as the reference's protocol tests at :550-702 drive it) in
 * one call: evaluate, read the outputs back, then per layer the circuit-backed sparse prover's 2k rounds, q =
 * restrict_poly on the device table W_{i+1}, and r_{i+1} = b* + r (c* - b*) (`line`, :278-289).  Every output may be NULL:
 *   outputs  2^k[0] words: the Begin message
 *   c1       depth words: each layer's StartSumCheck claim
 *   evals    3 * sum_i 2 k[i+1] words: every round's H(0), H(1), H(2), layer by layer
 *   q        sum_i (k[i+1] + 1) words: each layer's restrict_poly coefficients, dense, lowest degree first
 *   draws    k[0] + sum_i (2 k[i+1] + 1) words: every challenge, in the order drawn
 * Draw order (the reference Verifier's): k[0] draws for r_0; then per layer 2k - 1 sumcheck draws, final_random_point,
 * and the line draw.  draw(user, t, evals) gets the running draw index t; evals is the round's three sums for a draw that
 * follows a round message, NULL for r_0's draws, final_random_point and the line draw.  draw == NULL: the synthetic
 * challenger of sc_prove over t (to_mont(splitmix64(seed_r + t + 1) mod p)). */
int sc_gkr_prove_circuit(sc_ctx* ctx, const sc_circuit* c, const sc_table* input, sc_draw_fn draw, void* user,
                         uint64_t seed_r, uint64_t* outputs, uint64_t* c1, uint64_t* evals, uint64_t* q, uint64_t* draws);

/* ---- triangle_counting::G -------------------------------------
 *   g(X,Y,Z) = f(X,Y) f(Y,Z) f(X,Z)   (triangle-counting/src/lib.rs:10-27)
 * three copies f1, f2, f3 of the adjacency MLE (2*var_len variables each before any fixing,
 * idx(i,j,nv) = (i << nv) | j, :168-172).  Variable counts of a partially fixed G follow
 * :53-67.  Sharded contexts: the prover (sc_tri_prover_*) is available - adj is this rank's rows of the
 * adjacency table; the matrix square (the n^3 work) is split across the ranks, the sumchecks on the 2^(2k)- and
 * 2^k-entry tables run replicated on every rank.  The generic trait methods (sc_tri_*) are single-rank only:
 * they serve arbitrary partially fixed states by walking all 2^(3k) evaluations like the reference, and a caller on a
 * sharded node runs them on an unsharded context of any one rank (the replicated fallback; SC_ERR_UNSUPPORTED
 * otherwise, never a silent wrong answer). */

/* G::to_evaluations (:138-165), order x outer, z inner */
int sc_tri_to_evaluations(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len,
                          sc_table** out);
/* G::to_univariate (:120-132) as (H(0), H(1), H(2)) of the degree-2 round polynomial, for G in
 * any state, by walking all remaining evaluations like the reference */
int sc_tri_round_sums(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len,
                      uint64_t out_e[3]);
/* G::fix_variables (:89-118) */
int sc_tri_fix_variables(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len,
                         const uint64_t* r, size_t k, sc_table** f1_out, sc_table** f2_out, sc_table** f3_out);
/* G::evaluate (:71-87) */
int sc_tri_evaluate(sc_ctx* ctx, const sc_table* f1, const sc_table* f2, const sc_table* f3, size_t var_len,
                    const uint64_t* point, size_t n, uint64_t* out);
/* Prover<F, G> for G::new_adj_matrix(adj) (:32-51): all 3*var_len rounds.  One n^3 pass
 * (P = adj-matrix squared) turns the x rounds into a product-of-two-tables sumcheck on (P, f3);
 * the y rounds run on (f1(r_x,.), Q) with Q[y] = sum_z f2(y,z) f3(r_x,z); the z rounds on
 * (f2(r_y,.), f3(r_x,.)) scaled by f1(r_x,r_y).  Same contract as sc_prover_*. */
typedef struct sc_tri_prover sc_tri_prover;
int sc_tri_prover_create(sc_ctx* ctx, const sc_table* adj, size_t var_len, sc_tri_prover** out);
/* all 3 * var_len rounds in one call, challenges as in sc_prove */
int sc_tri_prove(sc_ctx* ctx, const sc_table* adj, size_t var_len, sc_draw_fn draw, void* user, uint64_t seed_r,
                 uint64_t* c1, uint64_t* evals, uint64_t* challenges);
int sc_tri_prover_c1(const sc_tri_prover* pr, uint64_t* out);
int sc_tri_prover_round(sc_tri_prover* pr, uint64_t r_prev, size_t j, uint64_t out_e[3]);
int sc_tri_prover_destroy(sc_tri_prover* pr);

#ifdef __cplusplus
}
#endif
#endif /* SUMCHECK_HIP_H */
