//! Raw declarations of `include/sumcheck_hip.h`.  One item per C entry point, same order.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_int, c_void};

pub const SC_OK: c_int = 0;
pub const SC_ERR_ARG: c_int = 1;
pub const SC_ERR_HIP: c_int = 2;
pub const SC_ERR_RCCL: c_int = 3;
pub const SC_ERR_OOM: c_int = 4;
pub const SC_ERR_STATE: c_int = 5;
pub const SC_ERR_UNSUPPORTED: c_int = 6;
pub const SC_ORDER_LE: c_int = 0;
pub const SC_ORDER_BE: c_int = 1;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct sc_field {
    pub p: u64,
    pub p_inv_neg: u64,
    pub r_mod_p: u64,
    pub r2_mod_p: u64,
}

/// One timed launch (`sc_ctx_launch_log`); `kind` is one of the `SC_KIND_*` values of the header.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sc_launch_record {
    pub kind: i32,
    pub kf: i32,
    pub ks: i32,
    pub log_in: i32,
    pub bytes_read: u64,
    pub bytes_written: u64,
    pub ms: f64,
}

#[repr(C)]
pub struct sc_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_table {
    _private: [u8; 0],
}
/// `SC_ABI_VERSION` of the header these declarations were written against; `sc_abi_version()` is the library's.
pub const SC_ABI_VERSION: c_int = 6;
/// The context options the schedule depends on (`sc_plan_proof`).  `struct_size` is set by
/// `sc_plan_options_init(&mut o, size_of::<sc_plan_options>())`; the library touches nothing beyond it.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sc_plan_options {
    pub struct_size: u32,
    pub vars_per_pass: i32,
    pub first_pass_vars: i32,
    pub grid_pass: i32,
    pub grid_log: i32,
    pub grid_max_vars: i32,
    pub grid_sharded: i32,
    pub tail_log: i32,
    pub use_mailbox: i32,
    pub gram_log: i32,
    pub host_tail_log: i32,
    pub wfold_log: i32,
    pub wfold_min_log: i32,
    pub wfold_always: i32,
    pub wfold5_min_log: i32,
}
/// One launch of a planned proof: `action` is one of the `SC_PLAN_*` values of the header.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct sc_plan_step {
    pub action: i32,
    pub kf: i32,
    pub ks: i32,
    pub log_in: i32,
    pub sharded: i32,
}
#[repr(C)]
pub struct sc_prover {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_gkr_prover {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_tri_prover {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_circuit {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_merkle_tree {
    _private: [u8; 0],
}
#[repr(C)]
pub struct sc_ligero {
    _private: [u8; 0],
}
/// a folded opening in progress (`sc_ligero_fold_begin`)
#[repr(C)]
pub struct sc_ligero_fold {
    _private: [u8; 0],
}

/// a rank-1 constraint system on the device (`sc_r1cs_create`)
#[repr(C)]
pub struct sc_r1cs {
    _private: [u8; 0],
}

/// a product tree on the device (`sc_gp_create`)
#[repr(C)]
pub struct sc_gp {
    _private: [u8; 0],
}

/// a product tree over the quadratic extension on the device (`sc_gp_create_ext`)
#[repr(C)]
pub struct sc_gp_ext {
    _private: [u8; 0],
}

/// the fraction-sum trees over the quadratic extension on the device (`sc_frac_create_ext`)
#[repr(C)]
pub struct sc_frac_ext {
    _private: [u8; 0],
}

/// a pair of fraction-sum trees on the device (`sc_frac_create`)
#[repr(C)]
pub struct sc_frac {
    _private: [u8; 0],
}

/// a sparse matrix with its index tables and counts on the device (`sc_spark_create`)
#[repr(C)]
pub struct sc_spark {
    _private: [u8; 0],
}

pub type sc_allreduce_fn = Option<unsafe extern "C" fn(user: *mut c_void, buf: *mut u64, count: usize) -> c_int>;
pub type sc_allgather_fn =
    Option<unsafe extern "C" fn(user: *mut c_void, send: *const u64, recv: *mut u64, count: usize) -> c_int>;
pub type sc_draw_fn = Option<unsafe extern "C" fn(user: *mut c_void, round: usize, evals: *const u64) -> u64>;
/// sc_sumprod_prove_ext: msg = H(0), H(1), H(2) as (c0, c1) pairs, out = the challenge (c0, c1)
pub type sc_draw_ext_fn = Option<unsafe extern "C" fn(user: *mut c_void, round: usize, msg: *const u64, out: *mut u64)>;
/// `sc_ligero_fold_prove`: the verifier's alpha of a round; `root` = the round's layer root (32 bytes), null at round 0.
pub type sc_draw_fold_fn = Option<unsafe extern "C" fn(user: *mut c_void, round: usize, evals: *const u64, root: *const u8) -> u64>;
/// `sc_zerocheck_prove`: the verifier's challenge of a round; `evals` = the round's H(0), H(1), H(2), H(3).
pub type sc_draw4_fn = Option<unsafe extern "C" fn(user: *mut c_void, round: usize, evals: *const u64) -> u64>;
/// `sc_gp_prove`: `round < layer`: `msg` = H(0..3) of that round, returns its challenge; `round == layer`: `msg` = (l, r'), returns rho
pub type sc_draw_gp_fn = Option<unsafe extern "C" fn(user: *mut c_void, layer: usize, round: usize, msg: *const u64) -> u64>;
/// `sc_gp_prove_ext`: `round < layer`: `msg` = the eight words H(0).c0 .. H(3).c1, `out` = the challenge (c0, c1); `round == layer`:
/// `msg` = (l, r'), four words, `out` = rho
pub type sc_draw_gp_ext_fn = Option<unsafe extern "C" fn(user: *mut c_void, layer: usize, round: usize, msg: *const u64, out: *mut u64)>;
/// `sc_frac_prove`: `round < layer`: `msg` = H(0..3), returns its challenge; `round == layer`: `msg` = (pl, pr, ql, qr), returns rho;
/// `round == layer + 1`: `msg` is null, returns lambda of the next layer
pub type sc_draw_frac_fn = Option<unsafe extern "C" fn(user: *mut c_void, layer: usize, round: usize, msg: *const u64) -> u64>;
/// `sc_frac_prove_ext`: `round < layer`: `msg` = the eight words H(0).c0 .. H(3).c1, `out` = the challenge (c0, c1); `round == layer`:
/// `msg` = (pl, pr, ql, qr), eight words, `out` = rho; `round == layer + 1`: `msg` is null, `out` = lambda of the next layer
pub type sc_draw_frac_ext_fn = Option<unsafe extern "C" fn(user: *mut c_void, layer: usize, round: usize, msg: *const u64, out: *mut u64)>;
/// `sc_prove_batch`: called round by round, within a round in instance order.
pub type sc_draw_batch_fn = Option<unsafe extern "C" fn(user: *mut c_void, instance: usize, round: usize, evals: *const u64) -> u64>;

extern "C" {
    pub fn sc_field_from_modulus(p: u64, out: *mut sc_field) -> c_int;
    pub fn sc_field_to_mont(f: *const sc_field, canonical: u64) -> u64;
    pub fn sc_field_from_mont(f: *const sc_field, mont: u64) -> u64;
    pub fn sc_interpolate_quadratic(f: *const sc_field, e: *const u64, c: *mut u64) -> c_int;

    pub fn sc_ctx_create(f: *const sc_field, device: c_int, out: *mut *mut sc_ctx) -> c_int;
    /// one handle over `n_devices` GPUs of this process (a power of two, up to 8); every table made on it is split over
    /// the devices by its top index bits and the prover / evaluate / fix_variables calls work on the whole table
    pub fn sc_ctx_create_multi(f: *const sc_field, devices: *const c_int, n_devices: c_int, out: *mut *mut sc_ctx) -> c_int;
    pub fn sc_ctx_destroy(ctx: *mut sc_ctx) -> c_int;
    pub fn sc_last_error(ctx: *const sc_ctx) -> *const c_char;
    pub fn sc_ctx_set_option(ctx: *mut sc_ctx, key: *const c_char, value: i64) -> c_int;
    pub fn sc_ctx_get_option(ctx: *const sc_ctx, key: *const c_char, value: *mut i64) -> c_int;
    pub fn sc_ctx_synchronize(ctx: *mut sc_ctx) -> c_int;
    pub fn sc_ctx_stream(ctx: *const sc_ctx) -> *mut c_void;
    pub fn sc_ctx_kernel_time(ctx: *mut sc_ctx, out: *mut f64, reset: c_int) -> c_int;
    pub fn sc_ctx_launch_log(
        ctx: *mut sc_ctx,
        out: *mut sc_launch_record,
        cap: usize,
        n_out: *mut usize,
        reset: c_int,
    ) -> c_int;

    pub fn sc_comm_unique_id(id: *mut u8) -> c_int;
    pub fn sc_ctx_comm_init_rccl(ctx: *mut sc_ctx, id: *const u8, rank: c_int, world: c_int) -> c_int;
    pub fn sc_ctx_comm_init_host(
        ctx: *mut sc_ctx,
        rank: c_int,
        world: c_int,
        allreduce: sc_allreduce_fn,
        allgather: sc_allgather_fn,
        user: *mut c_void,
    ) -> c_int;
    pub fn sc_ctx_comm_peer_export(ctx: *mut sc_ctx, rank: c_int, world: c_int, handle: *mut u8) -> c_int;
    pub fn sc_ctx_comm_peer_connect(ctx: *mut sc_ctx, handles: *const u8) -> c_int;
    pub fn sc_ctx_comm_peer_connect_local(ctx: *mut sc_ctx, peers: *const *mut sc_ctx) -> c_int;
    pub fn sc_ctx_comm_rank(ctx: *const sc_ctx, rank: *mut c_int, world: *mut c_int) -> c_int;

    pub fn sc_table_upload(ctx: *mut sc_ctx, host: *const u64, len: usize, out: *mut *mut sc_table) -> c_int;
    /// a table over device memory the caller owns (borrowed: never written, never freed by the library)
    pub fn sc_table_from_device(ctx: *mut sc_ctx, device_ptr: *const u64, len: usize, out: *mut *mut sc_table) -> c_int;
    pub fn sc_table_generate(ctx: *mut sc_ctx, seed: u64, start: u64, len: usize, out: *mut *mut sc_table) -> c_int;
    pub fn sc_table_clone(ctx: *mut sc_ctx, t: *const sc_table, out: *mut *mut sc_table) -> c_int;
    pub fn sc_table_download(ctx: *mut sc_ctx, t: *const sc_table, host: *mut u64, len: usize) -> c_int;
    pub fn sc_table_len(t: *const sc_table) -> usize;
    pub fn sc_table_device_ptr(t: *const sc_table) -> *const u64;
    pub fn sc_table_free(ctx: *mut sc_ctx, t: *mut sc_table) -> c_int;
    pub fn sc_table_fix_variables(
        ctx: *mut sc_ctx,
        input: *const sc_table,
        r: *const u64,
        k: usize,
        order: c_int,
        out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_table_evaluate(
        ctx: *mut sc_ctx,
        t: *const sc_table,
        r: *const u64,
        n: usize,
        order: c_int,
        out: *mut u64,
    ) -> c_int;
    /// `sc_table_evaluate` at `m` points (rows of `n` words) in one pass over the table
    pub fn sc_table_evaluate_many(ctx: *mut sc_ctx, t: *const sc_table, points: *const u64, m: usize, n: usize, order: c_int, out: *mut u64) -> c_int;
    pub fn sc_table_relabel(
        ctx: *mut sc_ctx,
        input: *const sc_table,
        a: usize,
        b: usize,
        k: usize,
        out: *mut *mut sc_table,
    ) -> c_int;

    pub fn sc_matmul_g_new(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        n: usize,
        point: *const u64,
        a_out: *mut *mut sc_table,
        b_out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_matmul(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        n: usize,
        c: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_prod2_to_evaluations(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_prod2_sum(ctx: *mut sc_ctx, a: *const sc_table, b: *const sc_table, out_c1: *mut u64) -> c_int;
    pub fn sc_prod2_round_sums(ctx: *mut sc_ctx, a: *const sc_table, b: *const sc_table, out_e: *mut u64) -> c_int;
    pub fn sc_prod2_fold_and_sums(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        r: *const u64,
        a_out: *mut *mut sc_table,
        b_out: *mut *mut sc_table,
        out_e: *mut u64,
    ) -> c_int;
    pub fn sc_prod2_evaluate(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        point: *const u64,
        n: usize,
        out: *mut u64,
    ) -> c_int;

    pub fn sc_abi_version() -> c_int;
    pub fn sc_plan_options_init(o: *mut sc_plan_options, struct_size: usize);
    pub fn sc_plan_proof(
        opt: *const sc_plan_options,
        num_vars: usize,
        world: c_int,
        transport: c_int,
        out: *mut sc_plan_step,
        cap: usize,
        n_out: *mut usize,
    ) -> c_int;
    pub fn sc_prover_create(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        out: *mut *mut sc_prover,
    ) -> c_int;
    pub fn sc_prover_c1(pr: *const sc_prover, out: *mut u64) -> c_int;
    pub fn sc_prover_num_vars(pr: *const sc_prover, out: *mut usize) -> c_int;
    pub fn sc_prover_round(pr: *mut sc_prover, r_prev: u64, j: usize, out_e: *mut u64) -> c_int;
    pub fn sc_prover_destroy(pr: *mut sc_prover) -> c_int;
    pub fn sc_prove(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        draw: sc_draw_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
    ) -> c_int;
    pub fn sc_prove_batch(
        ctx: *mut sc_ctx,
        count: usize,
        a: *const *const sc_table,
        b: *const *const sc_table,
        draw: sc_draw_batch_fn,
        user: *mut c_void,
        seed_r: *const u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
    ) -> c_int;

    // ---- gkr_protocol::round_polynomial::W ------------------------------------------------
    pub fn sc_gkr_wiring(
        ctx: *mut sc_ctx,
        gate_type: *const i32,
        in0: *const u32,
        in1: *const u32,
        k_i: usize,
        k_next: usize,
        r_i: *const u64,
        add_out: *mut *mut sc_table,
        mul_out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_gkr_w_to_evaluations(
        ctx: *mut sc_ctx,
        add: *const sc_table,
        mul: *const sc_table,
        w_b: *const sc_table,
        w_c: *const sc_table,
        out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_gkr_w_round_sums(
        ctx: *mut sc_ctx,
        add: *const sc_table,
        mul: *const sc_table,
        w_b: *const sc_table,
        w_c: *const sc_table,
        out_e: *mut u64,
    ) -> c_int;
    pub fn sc_gkr_w_fix_variables(
        ctx: *mut sc_ctx,
        add: *const sc_table,
        mul: *const sc_table,
        w_b: *const sc_table,
        w_c: *const sc_table,
        r: *const u64,
        k: usize,
        add_out: *mut *mut sc_table,
        mul_out: *mut *mut sc_table,
        w_b_out: *mut *mut sc_table,
        w_c_out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_gkr_w_evaluate(
        ctx: *mut sc_ctx,
        add: *const sc_table,
        mul: *const sc_table,
        w_b: *const sc_table,
        w_c: *const sc_table,
        point: *const u64,
        n: usize,
        out: *mut u64,
    ) -> c_int;
    pub fn sc_gkr_prover_create(
        ctx: *mut sc_ctx,
        add: *const sc_table,
        mul: *const sc_table,
        w_b: *const sc_table,
        w_c: *const sc_table,
        out: *mut *mut sc_gkr_prover,
    ) -> c_int;
    pub fn sc_gkr_prover_create_sparse(
        ctx: *mut sc_ctx,
        gate_type: *const i32,
        in0: *const u32,
        in1: *const u32,
        k_i: usize,
        k_next: usize,
        r_i: *const u64,
        w_next: *const sc_table,
        out: *mut *mut sc_gkr_prover,
    ) -> c_int;
    pub fn sc_gkr_prove(
        ctx: *mut sc_ctx,
        add: *const sc_table,
        mul: *const sc_table,
        w_b: *const sc_table,
        w_c: *const sc_table,
        draw: sc_draw_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
    ) -> c_int;
    pub fn sc_gkr_prover_c1(pr: *const sc_gkr_prover, out: *mut u64) -> c_int;
    pub fn sc_gkr_prover_round(pr: *mut sc_gkr_prover, r_prev: u64, j: usize, out_e: *mut u64) -> c_int;
    pub fn sc_gkr_prover_destroy(pr: *mut sc_gkr_prover) -> c_int;
    pub fn sc_table_restrict_to_line(
        ctx: *mut sc_ctx,
        t: *const sc_table,
        b: *const u64,
        c: *const u64,
        k: usize,
        out_coeffs: *mut u64,
    ) -> c_int;
    // ---- gkr_protocol::circuit::Circuit on the device, and the whole GKR prover over it -------------------
    pub fn sc_circuit_create(
        ctx: *mut sc_ctx,
        depth: usize,
        k: *const usize,
        gate_type: *const *const i32,
        in0: *const *const u32,
        in1: *const *const u32,
        out: *mut *mut sc_circuit,
    ) -> c_int;
    pub fn sc_circuit_destroy(ctx: *mut sc_ctx, c: *mut sc_circuit) -> c_int;
    pub fn sc_circuit_evaluate(ctx: *mut sc_ctx, c: *const sc_circuit, input: *const sc_table, values: *mut *mut sc_table) -> c_int;
    pub fn sc_gkr_prover_create_circuit(
        ctx: *mut sc_ctx,
        c: *const sc_circuit,
        i: usize,
        r_i: *const u64,
        w_next: *const sc_table,
        out: *mut *mut sc_gkr_prover,
    ) -> c_int;
    pub fn sc_gkr_prove_circuit(
        ctx: *mut sc_ctx,
        c: *const sc_circuit,
        input: *const sc_table,
        draw: sc_draw_fn,
        user: *mut c_void,
        seed_r: u64,
        outputs: *mut u64,
        c1: *mut u64,
        evals: *mut u64,
        q: *mut u64,
        draws: *mut u64,
    ) -> c_int;

    // ---- triangle_counting::G ----------------------------------------------------------------
    pub fn sc_tri_to_evaluations(
        ctx: *mut sc_ctx,
        f1: *const sc_table,
        f2: *const sc_table,
        f3: *const sc_table,
        var_len: usize,
        out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_tri_round_sums(
        ctx: *mut sc_ctx,
        f1: *const sc_table,
        f2: *const sc_table,
        f3: *const sc_table,
        var_len: usize,
        out_e: *mut u64,
    ) -> c_int;
    pub fn sc_tri_fix_variables(
        ctx: *mut sc_ctx,
        f1: *const sc_table,
        f2: *const sc_table,
        f3: *const sc_table,
        var_len: usize,
        r: *const u64,
        k: usize,
        f1_out: *mut *mut sc_table,
        f2_out: *mut *mut sc_table,
        f3_out: *mut *mut sc_table,
    ) -> c_int;
    pub fn sc_tri_evaluate(
        ctx: *mut sc_ctx,
        f1: *const sc_table,
        f2: *const sc_table,
        f3: *const sc_table,
        var_len: usize,
        point: *const u64,
        n: usize,
        out: *mut u64,
    ) -> c_int;
    pub fn sc_tri_prover_create(
        ctx: *mut sc_ctx,
        adj: *const sc_table,
        var_len: usize,
        out: *mut *mut sc_tri_prover,
    ) -> c_int;
    pub fn sc_tri_prove(
        ctx: *mut sc_ctx,
        adj: *const sc_table,
        var_len: usize,
        draw: sc_draw_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
    ) -> c_int;
    pub fn sc_tri_prover_c1(pr: *const sc_tri_prover, out: *mut u64) -> c_int;
    pub fn sc_tri_prover_round(pr: *mut sc_tri_prover, r_prev: u64, j: usize, out_e: *mut u64) -> c_int;
    pub fn sc_tri_prover_destroy(pr: *mut sc_tri_prover) -> c_int;

    /// relaxed-pcs: W~ at every point of F^m in the reference's leaf order (v_0 the most significant digit), zero-padded
    pub fn sc_table_extend_grid(ctx: *mut sc_ctx, t: *const sc_table, m: usize, out: *mut *mut sc_table) -> c_int;
    /// SHA-256 Merkle commitment of a table of 2^n entries (n <= 28); `t` is borrowed and must outlive the tree
    pub fn sc_merkle_commit(ctx: *mut sc_ctx, t: *const sc_table, out: *mut *mut sc_merkle_tree) -> c_int;
    pub fn sc_merkle_root(tr: *const sc_merkle_tree, root: *mut u8) -> c_int;
    pub fn sc_merkle_depth(tr: *const sc_merkle_tree, depth: *mut usize) -> c_int;
    /// `count` openings: leaves[count] canonical, paths[count][depth][32] bottom up
    pub fn sc_merkle_open(
        ctx: *mut sc_ctx,
        tr: *const sc_merkle_tree,
        index: *const u64,
        count: usize,
        leaves: *mut u64,
        paths: *mut u8,
    ) -> c_int;
    pub fn sc_merkle_tree_destroy(ctx: *mut sc_ctx, tr: *mut sc_merkle_tree) -> c_int;

    /// Ligero-style commitment: every row of `t` (2^log_cols coefficients) evaluated at the 2^(log_cols + log_blowup) powers of w_L
    pub fn sc_rs_encode_rows(ctx: *mut sc_ctx, t: *const sc_table, log_cols: usize, log_blowup: usize, out: *mut *mut sc_table) -> c_int;
    /// encode the rows and Merkle-hash the columns of the codeword matrix; `t` is borrowed and must outlive the commitment
    pub fn sc_ligero_commit(ctx: *mut sc_ctx, t: *const sc_table, log_cols: usize, log_blowup: usize, out: *mut *mut sc_ligero) -> c_int;
    pub fn sc_ligero_root(lg: *const sc_ligero, root: *mut u8) -> c_int;
    pub fn sc_ligero_shape(lg: *const sc_ligero, log_rows: *mut usize, log_cols: *mut usize, log_blowup: *mut usize) -> c_int;
    /// out[count][2^log_cols] = the combinations of the rows by `count` <= 4 weight vectors of 2^log_rows words
    pub fn sc_ligero_combine_rows(ctx: *mut sc_ctx, lg: *const sc_ligero, weights: *const u64, count: usize, out: *mut u64) -> c_int;
    /// values[count][2^log_rows] Montgomery, paths[count][log_cols + log_blowup][32] bottom up
    pub fn sc_ligero_open_columns(
        ctx: *mut sc_ctx,
        lg: *const sc_ligero,
        cols: *const u64,
        count: usize,
        values: *mut u64,
        paths: *mut u8,
    ) -> c_int;
    pub fn sc_ligero_destroy(ctx: *mut sc_ctx, lg: *mut sc_ligero) -> c_int;
    /// sc_rs_encode_rows for log_cols + log_blowup up to 24: above 14 a four-step transform in two launches (SC_KIND_RS_LONG)
    pub fn sc_rs_encode_rows_long(ctx: *mut sc_ctx, t: *const sc_table, log_cols: usize, log_blowup: usize, out: *mut *mut sc_table) -> c_int;
    /// sc_ligero_commit over sc_rs_encode_rows_long: an ordinary sc_ligero with code SC_CODE_RS
    pub fn sc_ligero_commit_long(ctx: *mut sc_ctx, t: *const sc_table, log_cols: usize, log_blowup: usize, out: *mut *mut sc_ligero) -> c_int;

    /// the rows of `t` (2^log_cols words each) under the linear-time expander code: every row followed by as many check words
    pub fn sc_xc_encode_rows(ctx: *mut sc_ctx, t: *const sc_table, log_cols: usize, out: *mut *mut sc_table) -> c_int;
    /// sc_ligero_commit with the row code chosen (SC_CODE_RS or SC_CODE_EXPANDER; the latter needs log_blowup = 1)
    pub fn sc_ligero_commit_code(
        ctx: *mut sc_ctx,
        t: *const sc_table,
        log_cols: usize,
        log_blowup: usize,
        code: c_int,
        out: *mut *mut sc_ligero,
    ) -> c_int;
    pub fn sc_ligero_code(lg: *const sc_ligero, code: *mut c_int) -> c_int;
    /// sc_xc_encode_rows for log_cols up to 23: above 13 the largest levels run as launches over global memory (SC_KIND_XC_LONG)
    pub fn sc_xc_encode_rows_long(ctx: *mut sc_ctx, t: *const sc_table, log_cols: usize, out: *mut *mut sc_table) -> c_int;
    /// sc_ligero_commit_code over the long row encoders: SC_CODE_RS is sc_ligero_commit_long, SC_CODE_EXPANDER needs log_blowup = 1
    pub fn sc_ligero_commit_code_long(
        ctx: *mut sc_ctx,
        t: *const sc_table,
        log_cols: usize,
        log_blowup: usize,
        code: c_int,
        out: *mut *mut sc_ligero,
    ) -> c_int;
    /// one fold of a Reed-Solomon codeword of 2^l words (2 <= l <= 24) with alpha: one launch of the fold kernel at arity one, recorded as SC_KIND_RS_FOLD (24)
    pub fn sc_rs_fold(ctx: *mut sc_ctx, u: *const sc_table, alpha: u64, out: *mut *mut sc_table) -> c_int;
    /// `count` = 1 .. 3 successive folds of a codeword of 2^l words (count + 1 <= l <= 24) in one launch of the same kernel, recorded as SC_KIND_RS_FOLD_MANY (25)
    pub fn sc_rs_fold_many(ctx: *mut sc_ctx, u: *const sc_table, alphas: *const u64, count: usize, out: *mut *mut sc_table) -> c_int;
    /// a folded opening of a Reed-Solomon commitment at `point`: claims = (v, v_gamma); the combined rows stay on the device
    pub fn sc_ligero_fold_begin(
        ctx: *mut sc_ctx,
        lg: *const sc_ligero,
        point: *const u64,
        gamma: *const u64,
        claims: *mut u64,
        out: *mut *mut sc_ligero_fold,
    ) -> c_int;
    /// `sc_ligero_fold_begin` with a schedule: `stages` arities in 1 ..= 3 that sum to log_cols; prove and query then work per stage
    pub fn sc_ligero_fold_begin_staged(
        ctx: *mut sc_ctx,
        lg: *const sc_ligero,
        point: *const u64,
        gamma: *const u64,
        arities: *const i32,
        stages: usize,
        claims: *mut u64,
        out: *mut *mut sc_ligero_fold,
    ) -> c_int;
    /// the c sumcheck rounds with a fold and a layer tree per stage: evals 3 c words, roots 32 (S - 1) bytes, challenges c words or null
    pub fn sc_ligero_fold_prove(
        ctx: *mut sc_ctx,
        fd: *mut sc_ligero_fold,
        beta: u64,
        draw: sc_draw_fold_fn,
        user: *mut c_void,
        evals: *mut u64,
        roots: *mut u8,
        challenges: *mut u64,
        final_value: *mut u64,
    ) -> c_int;
    /// the opened leaves of `count` indices below L / 2^a_0: pairs count x sum_(s>=1) 2^a_s words, paths count x P x 32 bytes
    pub fn sc_ligero_fold_query(
        ctx: *mut sc_ctx,
        fd: *const sc_ligero_fold,
        q: *const u64,
        count: usize,
        pairs: *mut u64,
        paths: *mut u8,
    ) -> c_int;
    pub fn sc_ligero_fold_destroy(ctx: *mut sc_ctx, fd: *mut sc_ligero_fold) -> c_int;
    /// A, B, C of 2^log_rows x 2^log_cols as three lists of (row, col, val) triples: checked and sorted on the host, copied to the device
    pub fn sc_r1cs_create(
        ctx: *mut sc_ctx,
        log_rows: usize,
        log_cols: usize,
        row: *const *const u32,
        col: *const *const u32,
        val: *const *const u64,
        nnz: *const usize,
        out: *mut *mut sc_r1cs,
    ) -> c_int;
    pub fn sc_r1cs_destroy(ctx: *mut sc_ctx, r: *mut sc_r1cs) -> c_int;
    /// A z, B z, C z as new tables: per matrix a product and a carry launch, SC_KIND_SPMV (26)
    pub fn sc_r1cs_mul(
        ctx: *mut sc_ctx,
        r: *const sc_r1cs,
        z: *const sc_table,
        az: *mut *mut sc_table,
        bz: *mut *mut sc_table,
        cz: *mut *mut sc_table,
    ) -> c_int;
    /// out[y] = sum_k rho[k] sum_i eq(rx, i) M_k[i][y]: one transposed product over the three matrices
    pub fn sc_r1cs_bind_rows(ctx: *mut sc_ctx, r: *const sc_r1cs, rx: *const u64, rho: *const u64, out: *mut *mut sc_table) -> c_int;
    /// the cubic sumcheck over eq(tau, x) (a(x) b(x) - c(x)): one launch per round, SC_KIND_ZEROCHECK (27); evals 4 s words or null
    pub fn sc_zerocheck_prove(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        c: *const sc_table,
        tau: *const u64,
        draw: sc_draw4_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
        finals: *mut u64,
    ) -> c_int;
    /// the product tree of a table of 2^n entries, 1 <= n <= 28 (SC_KIND_PRODUCT_TREE, 28); `t` is borrowed until `sc_gp_destroy`
    pub fn sc_gp_create(ctx: *mut sc_ctx, t: *const sc_table, out: *mut *mut sc_gp) -> c_int;
    pub fn sc_gp_destroy(ctx: *mut sc_ctx, g: *mut sc_gp) -> c_int;
    /// V_0[0], the product of the table's entries
    pub fn sc_gp_product(g: *const sc_gp, out: *mut u64) -> c_int;
    /// a copy of layer k < n of the tree: a new table of 2^k words
    pub fn sc_gp_layer(ctx: *mut sc_ctx, g: *const sc_gp, k: usize, out: *mut *mut sc_table) -> c_int;
    /// the n layers of the grand product argument: one launch per device round, SC_KIND_PRODUCT_PASS (29); evals 4 n (n-1) / 2 words or
    /// null, finals 2 n, challenges n (n-1) / 2 + n or null, point n, claim 1
    pub fn sc_gp_prove(
        ctx: *mut sc_ctx,
        g: *const sc_gp,
        draw: sc_draw_gp_fn,
        user: *mut c_void,
        seed_r: u64,
        evals: *mut u64,
        finals: *mut u64,
        challenges: *mut u64,
        point: *mut u64,
        claim: *mut u64,
    ) -> c_int;
    /// out[i] = alpha t[i] + beta: a new table
    pub fn sc_table_affine(ctx: *mut sc_ctx, t: *const sc_table, alpha: u64, beta: u64, out: *mut *mut sc_table) -> c_int;
    /// the fraction-sum trees of (p, q), 2^n entries each, 1 <= n <= 28 (SC_KIND_FRACTION_TREE, 30); `p` null: all ones; both are
    /// borrowed until `sc_frac_destroy`
    pub fn sc_frac_create(ctx: *mut sc_ctx, p: *const sc_table, q: *const sc_table, out: *mut *mut sc_frac) -> c_int;
    pub fn sc_frac_destroy(ctx: *mut sc_ctx, g: *mut sc_frac) -> c_int;
    /// out[0..2] = (P, Q), the root of the trees
    pub fn sc_frac_root(g: *const sc_frac, out: *mut u64) -> c_int;
    /// a copy of layer k < n of p (`which` = 0) or q (1): a new table of 2^k words
    pub fn sc_frac_layer(ctx: *mut sc_ctx, g: *const sc_frac, k: usize, which: c_int, out: *mut *mut sc_table) -> c_int;
    /// the n layers of the fractional sumcheck: one launch per device round, SC_KIND_FRACTION_PASS (31); evals 4 n (n-1) / 2 words or
    /// null, finals 4 n, challenges n (n-1) / 2 + 2 n - 1 or null, point n, claims 2
    pub fn sc_frac_prove(
        ctx: *mut sc_ctx,
        g: *const sc_frac,
        draw: sc_draw_frac_fn,
        user: *mut c_void,
        seed_r: u64,
        evals: *mut u64,
        finals: *mut u64,
        challenges: *mut u64,
        point: *mut u64,
        claims: *mut u64,
    ) -> c_int;
    /// the multiplicities of a lookup (SC_KIND_LOOKUP_COUNT, 32): `mult` a new table of t's length, `mismatches` the entries left out
    pub fn sc_lookup_count(
        ctx: *mut sc_ctx,
        w: *const sc_table,
        t: *const sc_table,
        idx_host: *const u32,
        mult: *mut *mut sc_table,
        mismatches: *mut u64,
    ) -> c_int;
    /// a sparse matrix of 2^log_rows x 2^log_cols from nnz >= 1 triples, padded to 2^l entries: its index tables and counts are
    /// built on the device (SC_KIND_SPARK_INDEX, 33); the host arrays may be freed on return
    pub fn sc_spark_create(
        ctx: *mut sc_ctx,
        log_rows: usize,
        log_cols: usize,
        row: *const u32,
        col: *const u32,
        val: *const u64,
        nnz: usize,
        out: *mut *mut sc_spark,
    ) -> c_int;
    pub fn sc_spark_destroy(ctx: *mut sc_ctx, sp: *mut sc_spark) -> c_int;
    /// a copy of row (`which` = 0), col (1), val (2), cr (3) or cc (4) as a new table
    pub fn sc_spark_table(ctx: *mut sc_ctx, sp: *const sc_spark, which: c_int, out: *mut *mut sc_table) -> c_int;
    /// er[k] = u[row_k], ec[k] = w[col_k]: two new tables from one launch (SC_KIND_SPARK_GATHER, 34)
    pub fn sc_spark_gather(
        ctx: *mut sc_ctx,
        sp: *const sc_spark,
        u: *const sc_table,
        w: *const sc_table,
        er: *mut *mut sc_table,
        ec: *mut *mut sc_table,
    ) -> c_int;
    /// den_w[k] = alpha - idx_k - beta e[k] and den_t[i] = alpha - i - beta t[i] of dimension `dim` (0: row, 1: col): two new
    /// tables, one launch each (SC_KIND_SPARK_TUPLE, 35)
    pub fn sc_spark_denominators(
        ctx: *mut sc_ctx,
        sp: *const sc_spark,
        dim: c_int,
        t: *const sc_table,
        e: *const sc_table,
        alpha: u64,
        beta: u64,
        den_w: *mut *mut sc_table,
        den_t: *mut *mut sc_table,
    ) -> c_int;
    /// the cubic sumcheck over a(x) b(x) c(x): one launch per device round, SC_KIND_PRODUCT_PASS (29); evals 4 n words or null,
    /// challenges n words or null, finals 3
    pub fn sc_product3_prove(
        ctx: *mut sc_ctx,
        a: *const sc_table,
        b: *const sc_table,
        c: *const sc_table,
        draw: sc_draw4_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
        finals: *mut u64,
    ) -> c_int;
    /// eq(r, .) over n variables as a new table of 2^n words
    pub fn sc_table_eq(ctx: *mut sc_ctx, r: *const u64, n: usize, out: *mut *mut sc_table) -> c_int;
    /// (rho_A eq(rx, .), rho_B eq(rx, .), rho_C eq(rx, .), 0): a new table of 2^(s+2) words
    pub fn sc_r1cs_row_weights(ctx: *mut sc_ctx, r: *const sc_r1cs, rx: *const u64, rho: *const u64, out: *mut *mut sc_table) -> c_int;
    /// out[x] = sum_k coeffs[k] eq(points[k], x) as a new table of 2^n words: `count` <= 16 rows of n words, one launch
    /// (SC_KIND_EQ_SUM, 36)
    pub fn sc_table_eq_sum(
        ctx: *mut sc_ctx,
        points: *const u64,
        coeffs: *const u64,
        count: usize,
        n: usize,
        out: *mut *mut sc_table,
    ) -> c_int;
    /// the sumcheck over sum_t a[t](x) b[t](x), `count` <= 8 pairs under shared challenges: one launch per device round,
    /// SC_KIND_SUMPROD_PASS (37); evals 3 n words or null, challenges n words or null, finals_a and finals_b `count` words each
    pub fn sc_sumprod_prove(
        ctx: *mut sc_ctx,
        count: usize,
        a: *const *const sc_table,
        b: *const *const sc_table,
        draw: sc_draw_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
        finals_a: *mut u64,
        finals_b: *mut u64,
    ) -> c_int;
    /// sc_sumprod_prove with challenges from K = F_p[X]/(X^2 - w), w a non-residue (Montgomery word): six words per round,
    /// SC_KIND_SUMPROD_EXT_PASS (38) from round 1 on; c1 two words, evals 6 n or null, challenges 2 n or null, finals 2 `count` each
    pub fn sc_sumprod_prove_ext(
        ctx: *mut sc_ctx,
        w: u64,
        count: usize,
        a: *const *const sc_table,
        b: *const *const sc_table,
        draw: sc_draw_ext_fn,
        user: *mut c_void,
        seed_r: u64,
        c1: *mut u64,
        evals: *mut u64,
        challenges: *mut u64,
        finals_a: *mut u64,
        finals_b: *mut u64,
    ) -> c_int;
    /// the multilinear extension of a base table of 2^n entries at a point of K^n (2 n words); out: two words
    pub fn sc_table_evaluate_ext(ctx: *mut sc_ctx, w: u64, t: *const sc_table, point: *const u64, n: usize, out: *mut u64) -> c_int;
    /// the product tree over K of the leaves beta + alpha t[i], t a base table of 2^n entries, 1 <= n <= 28
    /// (SC_KIND_EXT_PRODUCT_TREE, 39); alpha, beta: two words each, alpha != 0; `t` is borrowed until `sc_gp_destroy_ext`
    pub fn sc_gp_create_ext(ctx: *mut sc_ctx, w: u64, t: *const sc_table, alpha: *const u64, beta: *const u64, out: *mut *mut sc_gp_ext) -> c_int;
    pub fn sc_gp_destroy_ext(ctx: *mut sc_ctx, g: *mut sc_gp_ext) -> c_int;
    /// V_0[0], two words
    pub fn sc_gp_product_ext(g: *const sc_gp_ext, out: *mut u64) -> c_int;
    /// copies of the two planes of V_k, k < n, as base tables of 2^k words
    pub fn sc_gp_layer_ext(ctx: *mut sc_ctx, g: *const sc_gp_ext, k: usize, c0: *mut *mut sc_table, c1: *mut *mut sc_table) -> c_int;
    /// the n layers with every challenge in K (SC_KIND_EXT_EQ_TABLE, 41, and SC_KIND_EXT_PRODUCT_PASS, 40): evals 8 words per round
    /// or null, finals 4 n, challenges n (n + 1) words or null, point 2 n, claim 2
    pub fn sc_gp_prove_ext(
        ctx: *mut sc_ctx,
        g: *const sc_gp_ext,
        draw: sc_draw_gp_ext_fn,
        user: *mut c_void,
        seed_r: u64,
        evals: *mut u64,
        finals: *mut u64,
        challenges: *mut u64,
        point: *mut u64,
        claim: *mut u64,
    ) -> c_int;
    /// the fraction-sum trees over K of the leaves (p[i], beta + alpha t[i]), p and t base tables of 2^n entries, 1 <= n <= 28
    /// (SC_KIND_EXT_FRACTION_TREE, 42); `p` null: all ones; alpha, beta: two words each, alpha != 0; both tables are borrowed until
    /// `sc_frac_destroy_ext`
    pub fn sc_frac_create_ext(
        ctx: *mut sc_ctx,
        w: u64,
        p: *const sc_table,
        t: *const sc_table,
        alpha: *const u64,
        beta: *const u64,
        out: *mut *mut sc_frac_ext,
    ) -> c_int;
    pub fn sc_frac_destroy_ext(ctx: *mut sc_ctx, g: *mut sc_frac_ext) -> c_int;
    /// (P, Q), four words
    pub fn sc_frac_root_ext(g: *const sc_frac_ext, out: *mut u64) -> c_int;
    /// copies of the two planes of layer k, k < n, of p (`which` = 0) or q (1) as base tables of 2^k words
    pub fn sc_frac_layer_ext(ctx: *mut sc_ctx, g: *const sc_frac_ext, k: usize, which: c_int, c0: *mut *mut sc_table, c1: *mut *mut sc_table) -> c_int;
    /// the n layers with every challenge in K (SC_KIND_EXT_EQ_TABLE, 41, and SC_KIND_EXT_FRACTION_PASS, 43): evals 8 words per round
    /// or null, finals 8 n, challenges 2 (n (n - 1) / 2 + 2 n - 1) words or null, point 2 n, claims 4
    pub fn sc_frac_prove_ext(
        ctx: *mut sc_ctx,
        g: *const sc_frac_ext,
        draw: sc_draw_frac_ext_fn,
        user: *mut c_void,
        seed_r: u64,
        evals: *mut u64,
        finals: *mut u64,
        challenges: *mut u64,
        point: *mut u64,
        claims: *mut u64,
    ) -> c_int;
}
