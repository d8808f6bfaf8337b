//! Raw bindings of `include/hsw.h` (ABI version 1).  One item per C declaration;
//! struct layouts are `#[repr(C)]` mirrors.  Not compiled in the build image.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_uint, c_void};

#[repr(C)] pub struct hsw_engine { _private: [u8; 0] }
#[repr(C)] pub struct hsw_gadget { _private: [u8; 0] }

pub const HSW_OK: c_int = 0;
pub const HSW_ERR_INVALID_ARG: c_int = 1;
pub const HSW_ERR_SHAPE: c_int = 2;
pub const HSW_ERR_NO_DEVICE: c_int = 3;
pub const HSW_ERR_HIP: c_int = 4;
pub const HSW_ERR_UNSUPPORTED: c_int = 5;
pub const HSW_ERR_TOO_LARGE: c_int = 6;
pub const HSW_ERR_NOMEM: c_int = 7;

pub const HSW_REPR_CANONICAL: u32 = 0;
pub const HSW_REPR_MONTGOMERY: u32 = 1;
pub const HSW_SKIP_GATE: u32 = 2;
pub const HSW_SKIP_CHIP: u32 = 4;
pub const HSW_HOST_REGISTER: u32 = 8;
pub const HSW_REPR_COMPACT64: u32 = 16;
/// The blocks are ONE message; `d_pre_states` holds its initial state only (small-batch launches).
pub const HSW_CHAINED: u32 = 32;
pub const HSW_MODE_DEFAULT: u32 = 0;
pub const HSW_MODE_HALO2_INTERNALS: u32 = 1;
pub const HSW_MAX_BREAKS: usize = 16;
pub const HSW_CELL_BYTES: usize = 32;
pub const HSW_GADGET_WHOLE_DIGEST: u32 = 1;
pub const HSW_GADGET_INDEPENDENT: u32 = 2;
pub const HSW_GADGET_CONTEXT_IMAGES: u32 = 4;
pub const HSW_GADGET_SHARED_CONTEXT: u32 = 8;
pub const HSW_GADGET_MAX_COLUMNS: u32 = 1024;

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_shape {
    pub num_bits_lookup: u32,
    pub num_advice_columns: u32,
    pub limbs_per_spread: u32,
    pub cells_per_spread: u32,
    pub cells_per_state_spread: u32,
    pub cells_per_sigma: u32,
    pub cells_per_ch: u32,
    pub cells_per_maj: u32,
    pub cells_per_sched_step: u32,
    pub cells_per_round: u32,
    pub off_words: u32,
    pub off_msg_spread: u32,
    pub off_sched: u32,
    pub off_state_spread: u32,
    pub off_rounds: u32,
    pub off_feed: u32,
    pub gate_cells_per_block: u32,
    pub spread_calls_per_block: u32,
    pub limb_calls_per_block: u32,
    pub chip_cells_per_block: u32,
    pub algorithmic_bytes_per_block: u64,
    pub mode: u32,
    pub lookup_cells_per_block: u32,
    pub gate_calls_per_block: u32,
    pub reserved_: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_pack_plan {
    pub n_breaks: u32,
    pub columns_touched: u32,
    pub break_cell: [u64; HSW_MAX_BREAKS],
    pub break_gap: [u64; HSW_MAX_BREAKS],
    pub span_cells: u64,
    pub end_row: u64,
}

/// `hsw_last_launch`: the kernel instantiation and work split of the most recent expansion launch.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct hsw_launch_info {
    pub limbs: u32,
    pub tile_cells: u32,
    pub tile_rows: u32,
    pub repr: u32,
    pub internals: u32,
    pub parts: u32,
    pub split: u32,
    /// expansion launches of this engine so far (wraps)
    pub seq: u32,
    pub n_blocks: u64,
    pub grid: u64,
}

#[repr(C)]
pub struct hsw_witness_args {
    pub d_blocks: *const u8,
    pub d_pre_states: *const u32,
    pub n_blocks: usize,
    pub spread_cursor0: u64,
    pub d_gate: *mut c_void,
    pub d_chip_dense: *mut c_void,
    pub d_chip_spread: *mut c_void,
    pub chip_col_stride: usize,
    pub d_next_states: *mut u32,
    pub d_lookup: *mut c_void,
    pub flags: u32,
    pub pack: *const hsw_pack_plan,
    /// whole-digest streams: blocks per digest / cells and lookup cells skipped between digests (0 = off)
    pub frame_every: u64,
    pub frame_cells: u64,
    pub frame_lookups: u64,
}

/// Cell counts of the frame `digest` puts around its block loop (reference src/lib.rs:122-178, 294-341).
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_frame_shape {
    pub n_blocks: u64,
    pub prologue_cells: u64,
    pub epilogue_cells: u64,
    pub prologue_lookups: u64,
    pub epilogue_lookups: u64,
    pub prologue_calls: u64,
    pub epilogue_calls: u64,
    pub digest_cells: u64,
    pub digest_lookups: u64,
}

/// One `digest()` call for `hsw_witness_frames`.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_frame_desc {
    pub input_len: u64,
    pub first_block: u64,
    pub prologue_cell: u64,
    pub epilogue_cell: u64,
    pub prologue_lookup: u64,
    pub epilogue_lookup: u64,
    pub zero_cell: u64,
    pub n_blocks: u32,
    pub num_round: u32,
    pub precomputed_round: u32,
    pub is_input_range_check: u32,
}

/// `hsw_witness_digests`: block streams + frames of n equally sized digests in one call.
#[repr(C)]
pub struct hsw_digests_args {
    pub blocks: hsw_witness_args,
    pub descs: *const hsw_frame_desc,
    pub n_digests: usize,
    pub d_blocks0: *const u8,
    pub d_pre_states0: *const u32,
    pub d_next_states0: *const u32,
    pub d_gate0: *mut c_void,
    pub d_lookup0: *mut c_void,
    pub frame_pack: *const hsw_pack_plan,
    pub host_next_states: *mut u32,
}

pub const HSW_STREAM_GATE: u64 = 0;
pub const HSW_STREAM_LOOKUP: u64 = 1;
pub const HSW_STREAM_CHIP_DENSE: u64 = 2;
pub const HSW_STREAM_CHIP_SPREAD: u64 = 3;

/// One cell wider than 64 bits in the compact delivery of a region.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_wide_cell {
    pub stream: u64,
    pub index: u64,
    pub value: [u64; 4],
}

/// `hsw_gadget_result_cells`: where the cells of one digest's `AssignedHashResult` sit.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_result_cells {
    pub input_len_cell: u64,
    pub input_bytes_cell0: u64,
    pub n_input_bytes: u64,
    pub output_byte_cells: [u64; 32],
    pub input_len_pos: [u64; 2],
    pub input_bytes_pos0: [u64; 2],
    pub output_byte_pos: [[u64; 2]; 32],
}

#[repr(C)]
pub struct hsw_region_compact {
    pub gate: *mut u64,
    pub lookup: *mut u64,
    pub chip_dense: *mut u64,
    pub chip_spread: *mut u64,
    pub wide: *mut hsw_wide_cell,
    pub wide_cap: usize,
    pub n_wide: usize,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_digest_info {
    pub num_round: usize,
    pub precomputed_round: usize,
    pub target_round: usize,
    pub n_blocks: usize,
}

/// `AssignedHashResult` (reference src/lib.rs:31-36) on values.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_hash_result {
    pub input_len: u64,
    pub first_block: usize,
    pub n_blocks: usize,
    pub spread_cursor0: u64,
    pub num_round: usize,
    pub target_round: usize,
    pub output_bytes: [u8; 32],
    /// HSW_GADGET_WHOLE_DIGEST: section starts of this digest in the gate / lookup streams (cells)
    pub prologue_cell: u64,
    pub block_cell: u64,
    pub epilogue_cell: u64,
    pub end_cell: u64,
    pub prologue_lookup: u64,
    pub block_lookup: u64,
    pub epilogue_lookup: u64,
}

pub const HSW_CELL_INPUT_BYTE0: i64 = -1;
pub const HSW_CELL_PRE_STATE0: i64 = -100;
pub const HSW_CELL_ZERO: i64 = -1000;
pub const HSW_CELL_HIDDEN: i64 = -2000;
pub const HSW_KIND_WITNESS: u8 = 0;
pub const HSW_KIND_CONSTANT: u8 = 1;
pub const HSW_KIND_EXISTING: u8 = 2;

/// Result of `hsw_verify_blocks`.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_verify_report {
    pub violations: u64,
    pub checks: u64,
    pub first_block: u64,
    pub first_cell: i64,
    pub first_class: u32,
    pub kernel_ms: f32,
}

/// One digest-to-digest copy constraint of a pass (`hsw_gadget_ties`): input-byte cell `dst_byte` of digest
/// `dst_hash` equals output-byte cell `src_byte` of digest `src_hash`.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug, PartialEq, Eq)]
pub struct hsw_cell_tie {
    pub src_hash: u64,
    pub dst_hash: u64,
    pub src_byte: u32,
    pub dst_byte: u32,
    pub src_cell: u64,
    pub dst_cell: u64,
}

/// Result of `hsw_gadget_verify_ties` / `hsw_gadget_verify_equal`.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_tie_report {
    pub violations: u64,
    pub checks: u64,
    pub first: u64,
    pub kernel_ms: f32,
}

pub const HSW_LOOKUP_RANGE: u32 = 0;
pub const HSW_LOOKUP_SPREAD: u32 = 1;
/// `hsw_lookup_counts.flags`: add to what the tables hold instead of zeroing the proofs' tables first.
pub const HSW_LOOKUP_ACCUMULATE: u32 = 1;

/// `n` lookup entries of proof `context` as consecutive device cells (`hsw_gadget_lookup_runs`): entries of the
/// lookup-advice column (`HSW_LOOKUP_RANGE`, `d_spread` null) or rows of chip column `column` (`HSW_LOOKUP_SPREAD`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_lookup_run {
    pub context: u64,
    pub table: u32,
    pub column: u32,
    pub first: u64,
    pub n: u64,
    pub d_cells: *mut c_void,
    pub d_spread: *mut c_void,
}

/// The caller's per-proof multiplicity tables (`hsw_gadget_lookup_multiplicities`): `contexts x pitch` u32 counters
/// each, a null table is skipped, a pitch of 0 is the table size.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_lookup_counts {
    pub d_range: *mut u32,
    pub d_spread: *mut u32,
    pub range_pitch: u64,
    pub spread_pitch: u64,
    pub flags: u32,
    pub reserved_: u32,
}

/// Result of `hsw_gadget_lookup_multiplicities`.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_lookup_report {
    pub range_entries: u64,
    pub spread_entries: u64,
    pub not_in_table: u64,
    pub first_context: u64,
    pub first_entry: u64,
    pub first_table: u32,
    pub first_column: u32,
    pub kernel_ms: f32,
    pub reserved_: u32,
}

/// `hsw_lookup_permuted.flags`: `d_m` holds the caller's multiplicities instead of receiving the counted ones.
pub const HSW_PERMUTED_GIVEN_M: u32 = 1;
/// `hsw_lookup_permuted.flags`: the spread row is `t + spread(t) * theta` instead of `t * theta + spread(t)`.
pub const HSW_PERMUTED_THETA_ON_SPREAD: u32 = 2;

/// Arguments of `hsw_gadget_lookup_permuted`: one A' and one S' device column of `usable_rows` cells per argument
/// (RANGE: per proof; SPREAD: per proof and chip column), host arrays of device pointers; `thetas` is host memory,
/// `d_m` device memory.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_lookup_permuted {
    pub table: u32,
    pub flags: u32,
    pub usable_rows: u64,
    pub n_arguments: usize,
    pub d_input_columns: *const *mut c_void,
    pub d_table_columns: *const *mut c_void,
    pub thetas: *const c_void,
    pub d_m: *mut u32,
    pub m_pitch: u64,
}

/// Result of `hsw_gadget_lookup_permuted`; `written == 0` with `HSW_OK` means the device refused (see the header).
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_permuted_report {
    pub arguments: u64,
    pub entries: u64,
    pub written: u64,
    pub not_in_table: u64,
    pub first_context: u64,
    pub first_entry: u64,
    pub first_table: u32,
    pub first_column: u32,
    pub overflow_arguments: u64,
    pub kernel_ms: f32,
    pub prepare_ms: f32,
    pub write_ms: f32,
    pub reserved_: u32,
}

/// `hsw_gadget_lookup_product` status bit: `Z[u] != 1`; the argument is written all the same.
pub const HSW_PRODUCT_OPEN: u32 = 1;
/// Status bit: some `(A'[i] + beta)(S'[i] + gamma)` is zero; the argument is not written.
pub const HSW_PRODUCT_ZERO_DENOM: u32 = 2;
/// Status bit: a stored cell that was read is not an encoding below p; the argument is not written.
pub const HSW_PRODUCT_CELL_NOT_BELOW_P: u32 = 4;

/// Arguments of `hsw_gadget_lookup_product`: per argument (numbered as in `hsw_lookup_permuted`) the unpermuted input
/// column(s), the permuted pair and the Z column of `usable_rows + 1` cells, as host arrays of device pointers; the
/// challenges are host memory, one 32-byte element per proof as stored.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_lookup_product {
    pub table: u32,
    pub flags: u32,
    pub usable_rows: u64,
    pub n_arguments: usize,
    pub d_inputs: *const *const c_void,
    pub d_inputs_spread: *const *const c_void,
    pub input_rows: *const u64,
    pub d_permuted_inputs: *const *const c_void,
    pub d_permuted_tables: *const *const c_void,
    pub d_products: *const *mut c_void,
    pub thetas: *const c_void,
    pub betas: *const c_void,
    pub gammas: *const c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_lookup_product`; `first_open` / `first_refused` are `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_product_report {
    pub arguments: u64,
    pub written: u64,
    pub open_arguments: u64,
    pub first_open: u64,
    pub refused_arguments: u64,
    pub first_refused: u64,
    pub tile_rows: u32,
    pub reserved_: u32,
    pub kernel_ms: f32,
    pub tiles_ms: f32,
    pub scan_ms: f32,
    pub write_ms: f32,
}

/// Arguments of `hsw_gadget_permutation_product`: per proof `n_columns` value columns in the permutation's order (host
/// array of device pointers, `[c * m + j]`), the key's `n_columns` sigma columns shared by the proofs, and per proof
/// `S = ceil(n_columns / chunk_columns)` Z columns of `usable_rows + 1` cells; challenges, `omega` and `delta` are host
/// memory, 32 bytes per element as stored.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_permutation_product {
    pub flags: u32,
    pub chunk_columns: u32,
    pub usable_rows: u64,
    pub n_columns: usize,
    pub d_columns: *const *const c_void,
    pub column_rows: *const u64,
    pub d_sigmas: *const *const c_void,
    pub d_products: *const *mut c_void,
    pub betas: *const c_void,
    pub gammas: *const c_void,
    pub omega: *const c_void,
    pub delta: *const c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_permutation_product`; `first_open` / `first_refused` are `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_permutation_report {
    pub proofs: u64,
    pub products: u64,
    pub written: u64,
    pub open_proofs: u64,
    pub first_open: u64,
    pub refused_proofs: u64,
    pub first_refused: u64,
    pub tile_rows: u32,
    pub reserved_: u32,
    pub kernel_ms: f32,
    pub tiles_ms: f32,
    pub scan_ms: f32,
    pub write_ms: f32,
}

pub const HSW_NTT_SHIFT_AFTER: u32 = 1;
pub const HSW_NTT_CELL_NOT_BELOW_P: u32 = 4;

/// Arguments of `hsw_gadget_ntt`: `n_columns` columns of `2^log_n` cells (host arrays of device pointers; an output may
/// be its own input), `input_rows` per column (NULL: all), and `omega`, `shift`, `scale` in host memory, 32 bytes each
/// as stored (`shift`, `scale` may be NULL: 1).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_ntt {
    pub flags: u32,
    pub log_n: u32,
    pub pass_log: u32,
    pub reserved_: u32,
    pub n_columns: usize,
    pub d_inputs: *const *const c_void,
    pub input_rows: *const u64,
    pub d_outputs: *const *mut c_void,
    pub omega: *const c_void,
    pub shift: *const c_void,
    pub scale: *const c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_ntt`; `first_refused` is `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_ntt_report {
    pub columns: u64,
    pub written: u64,
    pub refused_columns: u64,
    pub first_refused: u64,
    pub twiddle_bytes: u64,
    pub scratch_bytes: u64,
    pub launches: u32,
    pub pass_log: u32,
    pub kernel_ms: f32,
    pub twiddle_ms: f32,
}

pub const HSW_MSM_CELL_NOT_BELOW_P: u32 = 4;
pub const HSW_MSM_BASE_NOT_BELOW_Q: u32 = 8;
pub const HSW_MSM_MAX_WINDOW_BITS: u32 = 8;

/// Arguments of `hsw_gadget_msm`: `n_columns` columns of 32-byte cells (a host array of device pointers), `input_rows`
/// per column (NULL: `n_bases`), against `n_bases` affine G1 points in device memory (64 bytes each, Montgomery form
/// mod q, `(0, 0)` the identity); `out_points` is host memory, 64 bytes per column.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_msm {
    pub flags: u32,
    pub window_bits: u32,
    pub slice_rows: u32,
    pub reserved_: u32,
    pub n_columns: usize,
    pub n_bases: u64,
    pub d_bases: *const c_void,
    pub d_scalars: *const *const c_void,
    pub input_rows: *const u64,
    pub out_points: *mut c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_msm`; `first_refused` and `first_bad_base` are `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_msm_report {
    pub columns: u64,
    pub refused_columns: u64,
    pub first_refused: u64,
    pub bad_bases: u64,
    pub first_bad_base: u64,
    pub scratch_bytes: u64,
    pub window_bits: u32,
    pub windows: u32,
    pub slice_rows: u32,
    pub slices: u32,
    pub launches: u32,
    pub reserved_: u32,
    pub kernel_ms: f32,
    pub finish_ms: f32,
}

pub const HSW_OPEN_CELL_NOT_BELOW_P: u32 = 4;
pub const HSW_OPEN_MIN_TILE_ROWS: u32 = 256;
pub const HSW_OPEN_THREAD_ROWS: u32 = 8;

/// Arguments of `hsw_gadget_evaluate`: `n_columns` columns of 32-byte cells (a host array of device pointers),
/// `input_rows` per column (NULL: `rows`), `n_points` points in host memory (32 bytes each as stored, below p) and
/// `n_queries` (column, point) index pairs; `out_evals` is host memory, 32 bytes per query.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_evaluate {
    pub flags: u32,
    pub tile_rows: u32,
    pub rows: u64,
    pub n_columns: usize,
    pub d_columns: *const *const c_void,
    pub input_rows: *const u64,
    pub n_points: usize,
    pub points: *const c_void,
    pub n_queries: usize,
    pub query_column: *const u32,
    pub query_point: *const u32,
    pub out_evals: *mut c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_evaluate`; `first_refused` (a column) is `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_evaluate_report {
    pub columns: u64,
    pub queries: u64,
    pub refused_columns: u64,
    pub refused_queries: u64,
    pub first_refused: u64,
    pub scratch_bytes: u64,
    pub tile_rows: u32,
    pub tiles: u32,
    pub thread_rows: u32,
    pub launches: u32,
    pub kernel_ms: f32,
    pub reserved_: u32,
}

/// Arguments of `hsw_gadget_open`: group `g` folds the columns `group_columns[group_first[g] .. group_first[g + 1])` with
/// `challenges[g]` (the first column the highest power) and divides by `(X - points[g])`; `d_quotients[g]` receives
/// `rows` cells, `out_evals` (may be NULL) the value of the folded column at the point.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_open {
    pub flags: u32,
    pub tile_rows: u32,
    pub rows: u64,
    pub n_columns: usize,
    pub d_columns: *const *const c_void,
    pub input_rows: *const u64,
    pub n_groups: usize,
    pub group_first: *const u64,
    pub group_columns: *const u32,
    pub points: *const c_void,
    pub challenges: *const c_void,
    pub d_quotients: *const *mut c_void,
    pub out_evals: *mut c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_open`; `first_refused` (a group) is `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_open_report {
    pub groups: u64,
    pub written: u64,
    pub refused_groups: u64,
    pub first_refused: u64,
    pub scratch_bytes: u64,
    pub tile_rows: u32,
    pub tiles: u32,
    pub thread_rows: u32,
    pub launches: u32,
    pub batches: u32,
    pub reserved_: u32,
    pub kernel_ms: f32,
    pub reserved2_: f32,
}

/// Status bit of `hsw_gadget_shplonk_quotient` / `_open`: a stored cell that was read is not an encoding below p.
pub const HSW_SHPLONK_CELL_NOT_BELOW_P: u32 = 4;
/// The most points of one rotation set.
pub const HSW_SHPLONK_MAX_SET_POINTS: u32 = 16;

/// Arguments of both calls of SHPLONK's multi-point opening: rotation set `i` lists the columns
/// `set_columns[set_first[i] .. set_first[i + 1])` (folded with `y`, the first gets `y^0`) and the points
/// `set_points[set_point_first[i] .. set_point_first[i + 1])` of `points`; the sets fold with `v` (the first gets `v^0`).
/// `u` and `d_h` are NULL for `hsw_gadget_shplonk_quotient` and required for `hsw_gadget_shplonk_open`; `d_out` receives
/// `rows` cells.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_shplonk {
    pub flags: u32,
    pub tile_rows: u32,
    pub rows: u64,
    pub n_columns: usize,
    pub d_columns: *const *const c_void,
    pub input_rows: *const u64,
    pub n_points: usize,
    pub points: *const c_void,
    pub n_sets: usize,
    pub set_first: *const u64,
    pub set_columns: *const u32,
    pub set_point_first: *const u64,
    pub set_points: *const u32,
    pub y: *const c_void,
    pub v: *const c_void,
    pub u: *const c_void,
    pub d_h: *const c_void,
    pub d_out: *mut c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_shplonk_quotient` / `_open`; `refused` is 1 when the status bit is set (then `written` is 0).
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_shplonk_report {
    pub sets: u64,
    pub items: u64,
    pub columns: u64,
    pub written: u64,
    pub refused: u64,
    pub scratch_bytes: u64,
    pub tile_rows: u32,
    pub tiles: u32,
    pub thread_rows: u32,
    pub launches: u32,
    pub kernel_ms: f32,
    pub reserved_: u32,
}

/// Status bit of `hsw_gadget_quotient`: a stored cell that the proof read is not an encoding below p.
pub const HSW_QUOTIENT_CELL_NOT_BELOW_P: u32 = 4;
/// The most factors of one monomial of a gate.
pub const HSW_QUOTIENT_MAX_FACTORS: u32 = 8;
/// The greatest extension `log_n - log_rows`.
pub const HSW_QUOTIENT_MAX_EXTENSION: u32 = 8;

/// The gates of `hsw_gadget_quotient` as sums of monomials: all host arrays, copied, not kept.  Gate `g` owns the terms
/// `gate_first_term[g] .. gate_first_term[g + 1]`, term `t` the factors `term_first_factor[t] .. term_first_factor[t + 1]`
/// (at most `HSW_QUOTIENT_MAX_FACTORS`); a factor is a column of the shared index space and a rotation in base rows.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_quotient_gates {
    pub n_gates: usize,
    pub n_terms: usize,
    pub n_factors: usize,
    pub gate_first_term: *const u32,
    pub term_coeffs: *const c_void,
    pub term_first_factor: *const u32,
    pub factor_column: *const u32,
    pub factor_rotation: *const i32,
}

/// The lookup arguments of `hsw_gadget_quotient`: per lookup its input and its table columns, folded with theta (the
/// first listed the highest power), and per (proof, lookup) the device columns A', S' and Z in extended form.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_quotient_lookups {
    pub n_lookups: usize,
    pub first_input: *const u32,
    pub inputs: *const u32,
    pub first_table: *const u32,
    pub tables: *const u32,
    pub d_permuted_inputs: *const *const c_void,
    pub d_permuted_tables: *const *const c_void,
    pub d_products: *const *const c_void,
    pub thetas: *const c_void,
}

/// Arguments of `hsw_gadget_quotient`: `n_proofs` independent proofs of one circuit, every column `2^log_n` cells in
/// extended form; `d_h[c]` receives h of proof `c` on the extended coset.  See include/hsw.h for the expressions and
/// their order.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct hsw_quotient {
    pub flags: u32,
    pub log_rows: u32,
    pub log_n: u32,
    pub chunk_columns: u32,
    pub usable_rows: u64,
    pub n_proofs: usize,
    pub n_columns: usize,
    pub n_fixed: usize,
    pub d_columns: *const *const c_void,
    pub d_fixed: *const *const c_void,
    pub d_l0: *const c_void,
    pub d_l_last: *const c_void,
    pub d_l_active: *const c_void,
    pub gates: hsw_quotient_gates,
    pub n_perm_columns: usize,
    pub perm_columns: *const u32,
    pub d_sigmas: *const *const c_void,
    pub d_perm_products: *const *const c_void,
    pub lookups: hsw_quotient_lookups,
    pub betas: *const c_void,
    pub gammas: *const c_void,
    pub ys: *const c_void,
    pub omega_ext: *const c_void,
    pub zeta: *const c_void,
    pub delta: *const c_void,
    pub d_h: *const *mut c_void,
    pub status: *mut u32,
}

/// Result of `hsw_gadget_quotient`; `first_refused` (a proof) is `u64::MAX` where there is none.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_quotient_report {
    pub proofs: u64,
    pub written: u64,
    pub refused_proofs: u64,
    pub first_refused: u64,
    pub expressions: u64,
    pub scratch_bytes: u64,
    pub launches: u32,
    pub rows_per_thread: u32,
    pub kernel_ms: f32,
    pub gates_ms: f32,
    pub permutation_ms: f32,
    pub lookups_ms: f32,
    pub finish_ms: f32,
}

pub const HSW_CELL_TARGET: i64 = -3000;
pub const HSW_CELL_STATE0: i64 = -4000;

/// Sizes of the arrays `hsw_frame_structure` fills.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_frame_structure_counts {
    pub cells: u64,
    pub gate_rows: u64,
    pub assert_eq: u64,
    pub assert_const: u64,
    pub ranges: u64,
    pub lookups: u64,
}

/// Sizes of the arrays `hsw_block_structure` fills.
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct hsw_structure_counts {
    pub gate_cells: u64,
    pub gate_rows: u64,
    pub assert_eq: u64,
    pub ranges: u64,
    pub lookups: u64,
    pub limb_calls: u64,
}

/// Host destinations of `hsw_gadget_download_region` (any may be null).
#[repr(C)]
pub struct hsw_region_host {
    pub gate: *mut c_void,
    pub lookup: *mut c_void,
    pub chip_dense: *mut c_void,
    pub chip_spread: *mut c_void,
}

pub const HSW_TAPE_CONST: u32 = 0x8000_0000;
#[repr(C)]
pub struct hsw_region_tape {
    pub n_distinct: u64,
    pub distinct_capacity: u64,
    pub gate_cells: u64,
    pub lookup_cells: u64,
    pub limb_calls: u64,
    pub gate_code: *const u32,
    pub lookup_code: *const u32,
    pub chip_dense_code: *const u32,
    pub chip_spread_code: *const u32,
    pub consts: *const c_void,
    pub n_consts: u64,
}

#[repr(C)]
pub struct hsw_gadget_view {
    pub d_gate: *mut c_void,
    pub d_chip_dense: *mut c_void,
    pub d_chip_spread: *mut c_void,
    pub d_next_states: *mut u32,
    pub chip_col_stride: usize,
    pub blocks_done: usize,
    pub capacity_blocks: usize,
    pub num_limb_sum: u64,
    pub cur_hash_idx: usize,
    pub gate_cells: u64,
    pub gate_capacity: u64,
    pub d_lookup: *mut c_void,
    pub lookup_cells: u64,
    pub lookup_capacity: u64,
    pub max_rows: u64,
    pub columns: u64,
    pub origin_column: u64,
    pub origin_row: u64,
    pub origin_lookups: u64,
    pub origin_zero_loaded: u32,
    pub reserved_: u32,
}

/// hsw_context_region: proof h of an HSW_GADGET_CONTEXT_IMAGES gadget on the device (include/hsw.h).
#[repr(C)]
pub struct hsw_context_region {
    pub d_image: *mut c_void,
    pub d_lookup: *mut c_void,
    pub d_chip_dense: *mut c_void,
    pub d_chip_spread: *mut c_void,
    pub columns: u64,
    pub max_rows: u64,
    pub last_column_rows: u64,
    pub stream_cells: u64,
    pub first_stream_cell: u64,
    pub lookup_cells: u64,
    pub chip_rows: u64,
    pub chip_col_stride: u64,
    pub origin_column: u64,
    pub origin_row: u64,
    pub origin_lookups: u64,
    pub assigned: u32,
    pub reserved_: u32,
}

/// hsw_region_binding: caller-owned device columns a gadget's region is bound to (include/hsw.h).
#[repr(C)]
pub struct hsw_region_binding {
    pub d_columns: *mut c_void,
    pub column_pitch: u64,
    pub columns_capacity: u64,
    pub context_pitch: u64,
    pub d_lookup: *mut c_void,
    pub lookup_capacity: u64,
    pub lookup_pitch: u64,
    pub d_chip_dense: *mut c_void,
    pub d_chip_spread: *mut c_void,
    pub chip_col_stride: u64,
    pub chip_rows_capacity: u64,
    pub chip_context_pitch: u64,
}

/// hsw_column_tables: host arrays of device pointers, one per column per proof (hsw_gadget_bind_column_tables).
#[repr(C)]
pub struct hsw_column_tables {
    pub d_column_ptrs: *const *mut c_void,
    pub n_column_ptrs: usize,
    pub d_lookup_ptrs: *const *mut c_void,
    pub n_lookup_ptrs: usize,
    pub d_chip_dense_ptrs: *const *mut c_void,
    pub d_chip_spread_ptrs: *const *mut c_void,
    pub n_chip_ptrs: usize,
}

extern "C" {
    pub fn hsw_abi_version() -> u32;
    pub fn hsw_strerror(status: c_int) -> *const c_char;
    pub fn hsw_last_error(e: *const hsw_engine) -> *const c_char;

    pub fn hsw_shape_query(num_bits_lookup: u32, num_advice_columns: u32, out: *mut hsw_shape) -> c_int;
    pub fn hsw_shape_query_ex(num_bits_lookup: u32, num_advice_columns: u32, mode: u32, out: *mut hsw_shape) -> c_int;
    pub fn hsw_spread_table(num_bits_lookup: u32, dense_out: *mut u64, spread_out: *mut u64) -> c_int;
    pub fn hsw_cell_bytes(flags: u32) -> u32;
    pub fn hsw_neg_cells(shape: *const hsw_shape, out: *mut u32, cap: usize, n: *mut usize) -> c_int;
    pub fn hsw_chip_rows(shape: *const hsw_shape, spread_cursor0: u64, n_blocks: u64) -> u64;

    pub fn hsw_engine_create(device: c_int, hip_stream: *mut c_void, num_bits_lookup: u32,
                             num_advice_columns: u32, out: *mut *mut hsw_engine) -> c_int;
    pub fn hsw_engine_create_ex(device: c_int, hip_stream: *mut c_void, num_bits_lookup: u32,
                                num_advice_columns: u32, mode: u32, out: *mut *mut hsw_engine) -> c_int;
    pub fn hsw_engine_destroy(e: *mut hsw_engine);
    pub fn hsw_engine_shape(e: *const hsw_engine, out: *mut hsw_shape) -> c_int;
    pub fn hsw_engine_synchronize(e: *mut hsw_engine) -> c_int;
    pub fn hsw_engine_stream(e: *const hsw_engine, hip_stream: *mut *mut c_void, device: *mut c_int) -> c_int;
    pub fn hsw_engine_set_option(e: *mut hsw_engine, name: *const c_char, value: i64) -> c_int;
    pub fn hsw_last_launch(e: *const hsw_engine, out: *mut hsw_launch_info) -> c_int;
    /// Block streams and frames of n equally sized digests in one call (one kernel launch up to 128 blocks, in digests of up to 32).
    pub fn hsw_witness_digests(e: *mut hsw_engine, args: *const hsw_digests_args) -> c_int;
    pub fn hsw_gadget_result_cells(g: *const hsw_gadget, hash_idx: usize, out: *mut hsw_result_cells) -> c_int;
    pub fn hsw_gadget_download_region_compact(g: *mut hsw_gadget, dst: *mut hsw_region_compact) -> c_int;
    pub fn hsw_region_widen(compact: *const u64, n_cells: usize, stream_id: u64, wide: *const hsw_wide_cell,
                            n_wide: usize, cells32: *mut c_void) -> c_int;

    /// Replaces the block loop of reference src/lib.rs:180-238 over src/compression.rs:19-25.
    pub fn hsw_witness_blocks(e: *mut hsw_engine, d_blocks: *const u8, d_pre_states: *const u32,
                              n_blocks: usize, spread_cursor0: u64, d_gate: *mut c_void,
                              d_chip_dense: *mut c_void, d_chip_spread: *mut c_void,
                              chip_col_stride: usize, d_next_states: *mut u32, flags: u32) -> c_int;
    pub fn hsw_witness_blocks_ex(e: *mut hsw_engine, args: *const hsw_witness_args) -> c_int;
    pub fn hsw_witness_blocks_host(e: *mut hsw_engine, blocks: *const u8, pre_states: *const u32,
                                   n_blocks: usize, spread_cursor0: u64, gate: *mut c_void,
                                   chip_dense: *mut c_void, chip_spread: *mut c_void,
                                   chip_col_stride: usize, next_states: *mut u32, flags: u32) -> c_int;
    pub fn hsw_sha256_chain(e: *mut hsw_engine, d_blocks: *const u8, n_messages: usize,
                            blocks_per_message: usize, d_init_states: *const u32,
                            d_pre_states: *mut u32) -> c_int;

    pub fn hsw_pack_plan_query(shape: *const hsw_shape, n_blocks: usize, start_row: u64, max_rows: u64,
                               out: *mut hsw_pack_plan) -> c_int;
    pub fn hsw_gate_tape(shape: *const hsw_shape, lens_out: *mut u8, cap: usize, n_calls: *mut usize) -> c_int;

    pub fn hsw_digest_prepare(input: *const u8, input_len: usize, precomputed_input_len: usize,
                              max_variable_byte_size: usize, blocks_out: *mut u8,
                              init_state_out: *mut u32, info: *mut hsw_digest_info) -> c_int;
    pub fn hsw_gadget_create(e: *mut hsw_engine, max_variable_byte_sizes: *const usize, n_hashes: usize,
                             is_input_range_check: c_int, out: *mut *mut hsw_gadget) -> c_int;
    /// K Contexts (proofs) of one circuit with M digests each (a Context group, include/hsw.h).
    pub fn hsw_gadget_create_contexts(e: *mut hsw_engine, max_variable_byte_sizes: *const usize, digests_per_context: usize,
                                      n_contexts: usize, is_input_range_check: c_int, flags: u32,
                                      out: *mut *mut hsw_gadget) -> c_int;
    pub fn hsw_gadget_create_ex(e: *mut hsw_engine, max_variable_byte_sizes: *const usize, n_hashes: usize,
                                is_input_range_check: c_int, flags: u32, out: *mut *mut hsw_gadget) -> c_int;
    pub fn hsw_gadget_destroy(g: *mut hsw_gadget);
    pub fn hsw_gadget_set_columns(g: *mut hsw_gadget, max_rows: u64, n_columns: *mut u64) -> c_int;
    /// Distinct-value delivery: the input-independent tape, the packed new witnesses, the host replay.
    pub fn hsw_gadget_region_tape(g: *mut hsw_gadget, out: *mut hsw_region_tape) -> c_int;
    pub fn hsw_gadget_download_region_distinct(g: *mut hsw_gadget, distinct: *mut c_void, cap_cells: usize,
                                               n_cells: *mut usize) -> c_int;
    pub fn hsw_gadget_replay_region(g: *mut hsw_gadget, distinct: *const c_void, dst: *const hsw_region_host,
                                    threads: u32) -> c_int;
    /// Where the caller's `Context` stands: `ctx.advice_alloc[0]`, `ctx.zero_cell.is_some()`, `ctx.cells_to_lookup.len()`.
    pub fn hsw_gadget_set_origin(g: *mut hsw_gadget, column: u64, row: u64, zero_cell_loaded: c_int,
                                 lookups_already_queued: u64) -> c_int;
    /// Shared context: where the `Context` stands just before digest `h` (`ctx.advice_alloc[0]`, `ctx.cells_to_lookup.len()`).
    pub fn hsw_gadget_set_digest_origin(g: *mut hsw_gadget, h: usize, column: u64, row: u64, lookups_queued: u64) -> c_int;
    pub fn hsw_gadget_reset(g: *mut hsw_gadget) -> c_int;
    pub fn hsw_gadget_seek(g: *mut hsw_gadget, hash_idx: usize) -> c_int;
    /// Buffer placement: try `candidates` allocations of the chip columns, keep the one the gadget's own batch runs fastest on.
    pub fn hsw_gadget_place(g: *mut hsw_gadget, candidates: c_uint, ms_each: *mut f32, kept: *mut c_uint) -> c_int;
    pub fn hsw_verify_frames(e: *mut hsw_engine, descs: *const hsw_frame_desc, n: usize, d_blocks: *const u8,
                             d_pre_states: *const u32, d_next_states: *const u32, d_gate: *const c_void,
                             d_lookup: *const c_void, pack: *const hsw_pack_plan, flags: u32,
                             report: *mut hsw_verify_report) -> c_int;
    pub fn hsw_gadget_verify(g: *mut hsw_gadget, report: *mut hsw_verify_report) -> c_int;
    pub fn hsw_verify_blocks(e: *mut hsw_engine, args: *const hsw_witness_args, report: *mut hsw_verify_report) -> c_int;
    pub fn hsw_frame_structure(shape: *const hsw_shape, max_variable_byte_size: usize, is_input_range_check: c_int,
                               section: c_int, counts: *mut hsw_frame_structure_counts, cell_kind: *mut u8,
                               cell_ref: *mut i64, gate_rows: *mut u32, assert_eq: *mut i64,
                               assert_const: *mut i64, range: *mut i64, lookup_src: *mut i64) -> c_int;
    pub fn hsw_block_structure(shape: *const hsw_shape, counts: *mut hsw_structure_counts, cell_kind: *mut u8,
                               cell_ref: *mut i64, gate_rows: *mut u32, assert_eq: *mut i64, range: *mut i64,
                               lookup_src: *mut i64, chip: *mut i64, next_state: *mut i64) -> c_int;
    pub fn hsw_gadget_download_region(g: *mut hsw_gadget, dst: *const hsw_region_host) -> c_int;
    pub fn hsw_gadget_cell_position(g: *const hsw_gadget, cell: u64, column: *mut u64, row: *mut u64) -> c_int;
    pub fn hsw_gadget_context_region(g: *const hsw_gadget, h: usize, out: *mut hsw_context_region) -> c_int;
    pub fn hsw_gadget_bind_region(g: *mut hsw_gadget, b: *const hsw_region_binding) -> c_int;
    pub fn hsw_gadget_region_binding(g: *const hsw_gadget, out: *mut hsw_region_binding) -> c_int;
    /// Like hsw_gadget_bind_region with one device pointer per image column per proof (include/hsw.h).
    pub fn hsw_gadget_bind_columns(
        g: *mut hsw_gadget,
        b: *const hsw_region_binding,
        d_column_ptrs: *const *mut c_void,
        n_ptrs: usize,
    ) -> c_int;
    /// The lookup-advice and chip columns by pointer table too: every advice column an allocation of its own.
    pub fn hsw_gadget_bind_column_tables(
        g: *mut hsw_gadget,
        b: *const hsw_region_binding,
        t: *const hsw_column_tables,
    ) -> c_int;
    pub fn hsw_frame_query(shape: *const hsw_shape, max_variable_byte_size: usize, is_input_range_check: c_int,
                           out: *mut hsw_frame_shape) -> c_int;
    pub fn hsw_frame_tape(shape: *const hsw_shape, max_variable_byte_size: usize, is_input_range_check: c_int,
                          section: c_int, lens_out: *mut u8, cap: usize, n_calls: *mut usize) -> c_int;
    pub fn hsw_witness_frames(e: *mut hsw_engine, descs: *const hsw_frame_desc, n: usize, d_blocks: *const u8,
                              d_pre_states: *const u32, d_next_states: *const u32, d_gate: *mut c_void,
                              d_lookup: *mut c_void, pack: *const hsw_pack_plan, flags: u32) -> c_int;
    pub fn hsw_gadget_digest(g: *mut hsw_gadget, input: *const u8, input_len: usize,
                             precomputed_input_len: usize, result: *mut hsw_hash_result) -> c_int;
    pub fn hsw_gadget_digest_batch(g: *mut hsw_gadget, n: usize, inputs: *const *const u8,
                                   input_lens: *const usize, precomputed_input_lens: *const usize,
                                   results: *mut hsw_hash_result) -> c_int;
    /// `hsw_gadget_digest_batch` with the message bytes in device memory: `d_inputs`, `input_lens` and
    /// `precomputed_input_lens` are host arrays, `d_inputs[i]` a device pointer of any alignment.
    pub fn hsw_gadget_digest_batch_device(g: *mut hsw_gadget, n: usize, d_inputs: *const *const c_void,
                                          input_lens: *const usize, precomputed_input_lens: *const usize,
                                          results: *mut hsw_hash_result) -> c_int;
    /// `hsw_gadget_digest_batch_device` over dependency levels: `levels` (may be null: all 0) orders the messages,
    /// `d_outputs` (may be null, entries may be null) names the 32 device bytes that receive each digest, and a
    /// message may read what a message of a strictly lower level of the same call writes.
    pub fn hsw_gadget_digest_levels_device(g: *mut hsw_gadget, n: usize, d_inputs: *const *const c_void,
                                           input_lens: *const usize, precomputed_input_lens: *const usize,
                                           levels: *const u32, d_outputs: *const *mut c_void,
                                           results: *mut hsw_hash_result) -> c_int;
    /// The digest-to-digest copy constraints the device-fed calls of this pass imply, in (dst_hash, dst_byte) order.
    pub fn hsw_gadget_ties(g: *const hsw_gadget, out: *mut hsw_cell_tie, cap: usize, n: *mut usize,
                           prefix_bytes_untied: *mut u64) -> c_int;
    /// Device address of a gate-stream cell in the layout and binding in force.
    pub fn hsw_gadget_cell_address(g: *const hsw_gadget, cell: u64, d_cell: *mut *mut c_void) -> c_int;
    pub fn hsw_gadget_verify_ties(g: *mut hsw_gadget, report: *mut hsw_tie_report) -> c_int;
    pub fn hsw_gadget_verify_equal(g: *mut hsw_gadget, cells_a: *const u64, cells_b: *const u64, n: usize,
                                   report: *mut hsw_tie_report) -> c_int;
    /// The lookup entries the digests of this pass have written, as runs of device cells in (context, table,
    /// column, first) order; host only.
    pub fn hsw_gadget_lookup_runs(g: *const hsw_gadget, out: *mut hsw_lookup_run, cap: usize, n: *mut usize) -> c_int;
    /// Counts the listed entries into the caller's per-proof multiplicity tables on the device; synchronous.
    pub fn hsw_gadget_lookup_multiplicities(g: *mut hsw_gadget, out: *const hsw_lookup_counts,
                                            report: *mut hsw_lookup_report) -> c_int;
    /// halo2's permuted lookup columns A' and S' of every argument of one table, written on the device.
    pub fn hsw_gadget_lookup_permuted(g: *mut hsw_gadget, args: *const hsw_lookup_permuted,
                                      report: *mut hsw_permuted_report) -> c_int;
    /// The grand-product column Z of every argument of one table, written on the device; synchronous.
    pub fn hsw_gadget_lookup_product(g: *mut hsw_gadget, args: *const hsw_lookup_product,
                                     report: *mut hsw_product_report) -> c_int;
    /// The permutation argument's grand products Z of every proof, written on the device; synchronous.  Status bits
    /// per proof: `HSW_PRODUCT_*`.
    pub fn hsw_gadget_permutation_product(g: *mut hsw_gadget, args: *const hsw_permutation_product,
                                          report: *mut hsw_permutation_report) -> c_int;
    /// The Fr NTT of device columns, natural order in and out; synchronous.  Status bit per column:
    /// `HSW_NTT_CELL_NOT_BELOW_P` (the column is not written).
    pub fn hsw_gadget_ntt(g: *mut hsw_gadget, args: *const hsw_ntt, report: *mut hsw_ntt_report) -> c_int;
    /// The commitments of device columns: `out_points[b] = sum_j a[j] * G[j]` in BN254 G1, one affine point per column in
    /// host memory.  Per column `status[b]` carries `HSW_MSM_CELL_NOT_BELOW_P` (that column is not written) or
    /// `HSW_MSM_BASE_NOT_BELOW_Q` (nothing is written).
    pub fn hsw_gadget_msm(g: *mut hsw_gadget, args: *const hsw_msm, report: *mut hsw_msm_report) -> c_int;
    /// Device columns evaluated at points: `out_evals[i] = sum_j a[j] * z^j` per (column, point) query, in host memory.
    /// Per column `status[b]` carries `HSW_OPEN_CELL_NOT_BELOW_P` (no query of that column is written).
    pub fn hsw_gadget_evaluate(g: *mut hsw_gadget, args: *const hsw_evaluate, report: *mut hsw_evaluate_report) -> c_int;
    /// The opening quotients of GWC, written on the device: per group the fold with v and the division by `(X - z)`.
    /// Per group `status[g]` carries `HSW_OPEN_CELL_NOT_BELOW_P` (that group is not written).
    pub fn hsw_gadget_open(g: *mut hsw_gadget, args: *const hsw_open, report: *mut hsw_open_report) -> c_int;
    /// The quotient h(X) of device columns on the extended coset; probe for the symbol (HSW_ABI_MINOR 1).
    pub fn hsw_gadget_quotient(g: *mut hsw_gadget, args: *const hsw_quotient, report: *mut hsw_quotient_report) -> c_int;
    /// SHPLONK's first polynomial `h = sum_i v^i floor(c_i / Z_i)` over rotation sets of device columns, written on the
    /// device; `*status` carries `HSW_SHPLONK_CELL_NOT_BELOW_P` (nothing is written).  Probe for the symbol (HSW_ABI_MINOR 1).
    pub fn hsw_gadget_shplonk_quotient(g: *mut hsw_gadget, args: *const hsw_shplonk, report: *mut hsw_shplonk_report) -> c_int;
    /// SHPLONK's second polynomial `w = (L(X) - L(u)) / ((X - u) zd_0)` from the same sets, `h` and `u`; likewise.
    pub fn hsw_gadget_shplonk_open(g: *mut hsw_gadget, args: *const hsw_shplonk, report: *mut hsw_shplonk_report) -> c_int;
    pub fn hsw_gadget_streams(g: *mut hsw_gadget, view: *mut hsw_gadget_view) -> c_int;
    pub fn hsw_gadget_input_bytes(g: *mut hsw_gadget, hash_idx: usize, out: *mut u8, cap: usize,
                                  len: *mut usize) -> c_int;
    pub fn hsw_gadget_set_repr(g: *mut hsw_gadget, repr: u32) -> c_int;

    pub fn hsw_download(e: *mut hsw_engine, host_dst: *mut c_void, d_src: *const c_void, bytes: usize) -> c_int;
    pub fn hsw_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn hsw_host_free(p: *mut c_void);
    /// Device memory for witness streams: one virtual range backed by physical allocations of up to `chunk_bytes` (0 = 4 GiB).
    pub fn hsw_device_alloc(device: c_int, bytes: usize, chunk_bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn hsw_device_free(ptr: *mut c_void) -> c_int;
    pub fn hsw_fill_calibrate(e: *mut hsw_engine, d_buf: *mut c_void, bytes: usize, ms: *mut f32) -> c_int;
    pub fn hsw_last_kernel_ms(e: *mut hsw_engine, ms: *mut f32) -> c_int;
    pub fn hsw_set_timing(e: *mut hsw_engine, enabled: c_int) -> c_int;
}
