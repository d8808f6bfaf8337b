/*
 * hsw.h -- C ABI of the MI355X SHA-256 witness engine ("halo2 sha witness").
 *
 * This is the drop-in boundary for the hot path of zhmolly/halo2-dynamic-sha256:
 * the reference has NO FFI of its own (it is plain Rust calling halo2-base), so
 * the boundary is new and sits exactly where `Sha256DynamicConfig::digest`
 * calls `sha256_compression` once per 64-byte block:
 *
 *     reference src/lib.rs:180-189          the block loop (caller)
 *     reference src/compression.rs:19-25    sha256_compression(ctx, range,
 *                                           spread_config, bytes[64], pre_state[8])
 *     reference src/spread.rs:196-233       spread_limb (chip column placement)
 *
 * A Rust shim keeps `Sha256DynamicConfig`'s surface, pads/chains on the host,
 * calls hsw_witness_blocks() once for all blocks of a digest (or a batch of
 * digests) and replays the returned streams into `Context`/`Region`
 * (INTEGRATION.md shows the `extern "C"` block).
 *
 * Streams (DESIGN.md "Streams"):
 *   gate cells   per block G cells (hsw_shape.gate_cells_per_block; 66,308 at
 *                the reference's configuration), in the order the reference
 *                issues halo2-base gate calls, 4 cells per add/neg/mul_add gate
 *                and 1 per load_witness.
 *   chip columns the SpreadConfig advice columns denses[c] / spreads[c]
 *                (spread.rs:20-21): limb call #n (counted from
 *                SpreadConfig.num_limb_sum) lands in column n % ncols at row
 *                n / ncols (spread.rs:202-231).
 *   next states  8 u32 words per block (compression.rs:197-212).
 * One cell = 32 bytes = one BN254 scalar-field element, 4 little-endian 64-bit
 * limbs, canonical (HSW_REPR_CANONICAL) or Montgomery (HSW_REPR_MONTGOMERY,
 * the in-memory form of halo2curves' Fr) form; both are built.
 * Beyond the block loop: in HSW_MODE_HALO2_INTERNALS the engine also emits the
 * cells halo2-base / digest() allocate around it ("placement adaptor", "digest
 * frame" below), up to the literal advice-column image of the whole region.
 *
 * All entry points return an int status (HSW_OK = 0); nothing unwinds across
 * the ABI.  Shape violations that the reference would `assert!`/`debug_assert!`
 * on (lib.rs:57-59,89-90; spread.rs:37; compression.rs:26-27) are hard errors.
 */
#ifndef HSW_H
#define HSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSW_ABI_VERSION 3   /* 3: hsw_gadget_view grew the origin fields; hsw_gadget_set_origin */
#define HSW_ABI_MINOR 1     /* additions that leave every existing entry point as it was: 1: hsw_gadget_bind_column_tables; hsw_gadget_digest_batch_device and hsw_gadget_digest_levels_device came later under the same minor (probe for the symbol) */

/* ---- status codes ---- */
#define HSW_OK                 0
#define HSW_ERR_INVALID_ARG    1   /* NULL / misaligned / inconsistent argument */
#define HSW_ERR_SHAPE          2   /* 16 % num_bits_lookup != 0, ncols == 0, max % 64 != 0 ... */
#define HSW_ERR_NO_DEVICE      3   /* no usable gfx950 device / HIP runtime */
#define HSW_ERR_HIP            4   /* a HIP call failed; see hsw_last_error() */
#define HSW_ERR_UNSUPPORTED    5   /* valid request this build does not implement */
#define HSW_ERR_TOO_LARGE      6   /* message does not fit max_variable_byte_size (lib.rs:90) */
#define HSW_ERR_NOMEM          7

/* ---- flags for hsw_witness_blocks ---- */
#define HSW_REPR_CANONICAL     0u  /* cells hold the canonical integer, LE limbs */
#define HSW_REPR_MONTGOMERY    1u  /* cells hold x*2^256 mod p (halo2curves Fr memory form) */
#define HSW_REPR_COMPACT64    16u  /* transport form: 8-byte cells holding the low 64 bits of the canonical
                                      value.  Every cell of the path fits 64 bits except the field negations
                                      of ch (compression.rs:320-335; 256 cells per block at fixed positions,
                                      hsw_neg_cells): those hold x where the cell's value is -x = p - x.
                                      4x fewer bytes for PCIe-bound consumers; buffers are sized with
                                      hsw_cell_bytes(flags) = 8 instead of 32 */
#define HSW_REPR_MASK          (1u | 16u)
#define HSW_SKIP_GATE          2u  /* do not write the gate stream (d_gate may be NULL) */
#define HSW_SKIP_CHIP          4u  /* do not write the chip columns (pointers may be NULL) */

#define HSW_HOST_REGISTER       8u  /* DEPRECATED (to be removed at the next ABI version).  hsw_witness_blocks_host only.
                                      Accepted and IGNORED since ABI 2: the library
                                      never pins memory it does not own (hipHostRegister on a caller's heap buffers
                                      ended in GPU memory faults twice: a user-pointer registration does not survive
                                      the allocator trimming and re-growing its heap).  Pageable buffers take the
                                      runtime's staged copies; for the PCIe rate allocate with hsw_host_alloc. */
#define HSW_CHAINED            32u  /* hsw_witness_blocks(_ex): the n_blocks blocks are ONE message (lib.rs:180-238) and
                                      d_pre_states holds its initial state only (8 words); every wave derives its
                                      block's pre-state itself, so no chain pre-pass (hsw_sha256_chain) and no second
                                      launch is needed.  Small-batch launches only (<= 32 blocks at the 8-bit table),
                                      HSW_ERR_UNSUPPORTED otherwise.  d_next_states receives every block's output. */

#define HSW_CELL_BYTES         32u

typedef struct hsw_engine hsw_engine;

/* Shape of the streams for SpreadConfig::configure(num_bits_lookup,
 * num_advice_columns) (spread.rs:32-74).  All counts are per 64-byte block. */
typedef struct hsw_shape {
    uint32_t num_bits_lookup;        /* 16 % it == 0 (spread.rs:37) */
    uint32_t num_advice_columns;     /* >= 1 */
    uint32_t limbs_per_spread;       /* 16 / num_bits_lookup (spread.rs:84) */
    uint32_t cells_per_spread;       /* gate cells of one SpreadConfig::spread call */
    uint32_t cells_per_state_spread; /* state_to_spread_u32 (compression.rs:215-246) */
    uint32_t cells_per_sigma;        /* sigma_generic (compression.rs:702-882) */
    uint32_t cells_per_ch;           /* compression.rs:297-405 */
    uint32_t cells_per_maj;          /* compression.rs:460-519 */
    uint32_t cells_per_sched_step;   /* one idx of compression.rs:57-96 */
    uint32_t cells_per_round;        /* one idx of compression.rs:125-196 */
    /* offsets (in cells) of the six regions of one block's gate stream */
    uint32_t off_words;              /* compression.rs:31-47   16 x 16 cells */
    uint32_t off_msg_spread;         /* compression.rs:53-56   16 state_to_spread_u32 */
    uint32_t off_sched;              /* compression.rs:57-96   48 steps */
    uint32_t off_state_spread;       /* compression.rs:109-115 6 state_to_spread_u32 */
    uint32_t off_rounds;             /* compression.rs:125-196 64 rounds */
    uint32_t off_feed;               /* compression.rs:197-212 8 x 10 cells */
    uint32_t gate_cells_per_block;   /* G */
    uint32_t spread_calls_per_block; /* 2,060 */
    uint32_t limb_calls_per_block;   /* spread_calls * limbs_per_spread (cursor advance) */
    uint32_t chip_cells_per_block;   /* 2 * limb_calls_per_block */
    uint64_t algorithmic_bytes_per_block; /* (G + chip cells) * 32 + 64 + 32 + 32 */
    uint32_t mode;                   /* HSW_MODE_* this shape was computed for */
    uint32_t lookup_cells_per_block; /* entries of the lookup-advice column per block (3,184) */
    uint32_t gate_calls_per_block;   /* halo2-base assign_region calls per block (the tape length) */
    uint32_t reserved_;
} hsw_shape;

/* ---- engine modes ---- */
#define HSW_MODE_DEFAULT          0u
/* Also emit the cells halo2-base itself allocates inside the path -- the 4-cell
 * inner product [limb0, limb1, 2^16, a] of every range_check(a, 32) (760 per
 * block => G = 69,348) -- and make the lookup-advice column stream available
 * (what RangeConfig::finalize copies, lib.rs:469: 3,184 cells per block).
 * These follow halo2-lib v0.2.x (DESIGN.md assumption A3); the fork the
 * reference pins is not in its tree, so A3 is unpinned.  Every table width; with the 2- and 1-bit
 * tables only 32-byte cells (canonical / Montgomery), not HSW_REPR_COMPACT64. */
#define HSW_MODE_HALO2_INTERNALS  1u

/* Fill *out for the given SpreadConfig parameters.  Pure host arithmetic. */
int hsw_shape_query(uint32_t num_bits_lookup, uint32_t num_advice_columns, hsw_shape *out);
int hsw_shape_query_ex(uint32_t num_bits_lookup, uint32_t num_advice_columns, uint32_t mode,
                       hsw_shape *out);

/* SpreadConfig::load (spread.rs:165-194): the 2^num_bits_lookup rows
 * (i, spread(i)) of the lookup table, as u64 values.  Either output may be NULL. */
int hsw_spread_table(uint32_t num_bits_lookup, uint64_t *dense_out, uint64_t *spread_out);

/* Bytes per cell for a flags word: 8 with HSW_REPR_COMPACT64, else 32. */
uint32_t hsw_cell_bytes(uint32_t flags);
/* Block-relative gate-stream indices of the cells that hold a field negation
 * (4 per round, compression.rs:320-335), ascending; needed to decode
 * HSW_REPR_COMPACT64.  out may be NULL to query the count (256). */
int hsw_neg_cells(const hsw_shape *shape, uint32_t *out, size_t cap, size_t *n);

/* Number of rows every chip column buffer must hold for n_blocks blocks whose
 * first limb call is #spread_cursor0: buffer row 0 is absolute chip row
 * spread_cursor0 / ncols.  Returns 0 on a bad shape. */
uint64_t hsw_chip_rows(const hsw_shape *shape, uint64_t spread_cursor0, uint64_t n_blocks);

/* Engine bound to one HIP device and stream (hip_stream: a hipStream_t, or
 * NULL for the device's default stream).  One engine per host thread/stream;
 * calls on one engine are issued asynchronously in order on that stream. */
int hsw_engine_create(int device, void *hip_stream, uint32_t num_bits_lookup,
                      uint32_t num_advice_columns, hsw_engine **out);
int hsw_engine_create_ex(int device, void *hip_stream, uint32_t num_bits_lookup,
                         uint32_t num_advice_columns, uint32_t mode, hsw_engine **out);
void hsw_engine_destroy(hsw_engine *e);
int hsw_engine_shape(const hsw_engine *e, hsw_shape *out);
int hsw_engine_synchronize(hsw_engine *e);

/* Replaces n calls of sha256_compression (compression.rs:19-213).
 *
 *   d_blocks      n*64 message bytes            (device memory)
 *   d_pre_states  n*8 u32 pre-state words       (device memory)
 *   spread_cursor0  SpreadConfig.num_limb_sum before the first block
 *                 (spread.rs:26,202); block j starts at cursor0 + j*limb_calls_per_block
 *   d_gate        n*G cells (device memory); must be 16-byte aligned and should be
 *                 32-byte (cell) aligned: at 16 mod 32 every canonical cell straddles
 *                 two sectors and the launch runs ~45 % slower.  Any cell-aligned
 *                 position is fine -- the kernel realigns its write-out to 128-byte
 *                 lines (a few % slower than a line-aligned stream)
 *   d_chip_dense / d_chip_spread
 *                 ncols columns each; column c starts at base + c*chip_col_stride
 *                 cells; hsw_chip_rows() rows are written per column (cells of
 *                 the first/last row that belong to neighbouring calls are left
 *                 untouched when the cursor is not a multiple of ncols)
 *   d_next_states n*8 u32                       (device memory, may be NULL)
 *   flags         HSW_REPR_* | HSW_SKIP_*
 *
 * Asynchronous on the engine's stream. */
int hsw_witness_blocks(hsw_engine *e, const uint8_t *d_blocks, const uint32_t *d_pre_states,
                       size_t n_blocks, uint64_t spread_cursor0, void *d_gate,
                       void *d_chip_dense, void *d_chip_spread, size_t chip_col_stride,
                       uint32_t *d_next_states, uint32_t flags);

/* ------------------------------------------------------------------------
 * Placement adaptor: from streams to FlexGate advice columns.
 * halo2-lib v0.2.x FlexGate (Vertical strategy) fills ONE advice column after
 * another: every assign_region call of `len` cells goes to the current column
 * at the current row, or -- if row + len >= max_rows -- to row 0 of the next
 * column (assumption A3).  So advice columns are the linear gate stream with a
 * gap of unused tail rows at every column break.  hsw_pack_plan_query computes
 * the breaks for n_blocks blocks whose first cell lands at `start_row` of some
 * column; hsw_witness_blocks_ex applies them while writing.
 * ------------------------------------------------------------------------ */
#define HSW_MAX_BREAKS 16
typedef struct hsw_pack_plan {
    uint32_t n_breaks;
    uint32_t columns_touched;            /* 1 + n_breaks */
    uint64_t break_cell[HSW_MAX_BREAKS]; /* linear stream index of the first cell after break k */
    uint64_t break_gap[HSW_MAX_BREAKS];  /* unused tail rows of the column that break k closes */
    uint64_t span_cells;                 /* cells from the first written one to one past the last, gaps included */
    uint64_t end_row;                    /* row after the last cell in the last column (advice_alloc.1) */
} hsw_pack_plan;
int hsw_pack_plan_query(const hsw_shape *shape, size_t n_blocks, uint64_t start_row, uint64_t max_rows,
                        hsw_pack_plan *out);
/* The assign_region call lengths of one block (1 or 4 each), in stream order:
 * the tape a shim walks to replay the stream into halo2-base.  lens_out may be
 * NULL to query the count. */
int hsw_gate_tape(const hsw_shape *shape, uint8_t *lens_out, size_t cap, size_t *n_calls);

/* The constraint STRUCTURE of one block's gate stream (input independent): for every cell which
 * QuantumCell the reference hands to halo2-base there, plus everything else a replayer needs to
 * rebuild the gadget's constraint system around the value streams (what halo2 key generation
 * records): gate rows, assert_equal pairs, range_check bounds, lookup sources, spread-chip ties.
 * Built on the host by walking the reference's call sequence on symbolic cells
 * (csrc/hsw_structure.hpp); follows the engine mode of `shape` (HSW_MODE_HALO2_INTERNALS adds the
 * range_check rows).  Cell ids: >= 0 = block-relative stream index; < 0 = outside the block:
 * HSW_CELL_INPUT_BYTE0 - k (input byte k), HSW_CELL_PRE_STATE0 - i (pre-state word i),
 * HSW_CELL_ZERO (the Context's zero cell), HSW_CELL_HIDDEN (a halo2-base witness not in the stream). */
#define HSW_CELL_INPUT_BYTE0 (-1)
#define HSW_CELL_PRE_STATE0  (-100)
#define HSW_CELL_ZERO        (-1000)
#define HSW_CELL_HIDDEN      (-2000)
#define HSW_KIND_WITNESS  0
#define HSW_KIND_CONSTANT 1   /* cell_ref = the constant */
#define HSW_KIND_EXISTING 2   /* cell_ref = the cell it is copy-constrained to */
typedef struct hsw_structure_counts {
    uint64_t gate_cells, gate_rows, assert_eq, ranges, lookups, limb_calls;
} hsw_structure_counts;
/* Any output pointer may be NULL.  Sizes: cell_kind / cell_ref gate_cells; gate_rows gate_rows (first
 * cell of each row x0 + x1*x2 = x3); assert_eq 2*assert_eq; range 2*ranges (cell, bits); lookup_src
 * lookups; chip 2*limb_calls (cell tied to the dense chip cell, cell tied to the spread chip cell);
 * next_state 8 (the cells holding the block's output words). */
int hsw_block_structure(const hsw_shape *shape, hsw_structure_counts *counts, uint8_t *cell_kind,
                        int64_t *cell_ref, uint32_t *gate_rows, int64_t *assert_eq, int64_t *range,
                        int64_t *lookup_src, int64_t *chip, int64_t *next_state);

/* On-device check of a block witness against the gadget's constraint system -- what MockProver::verify
 * checks for the path (lib.rs:525-526): every gate row, copy constraint (Existing cells, assert_equal),
 * fixed constant, range_check bound, spread-chip cell (tied to its gate cell; (dense, spread) a row of the
 * spread table), lookup-column copy and next-state word, with the block bytes and pre-states entering
 * only through the cells they are copy-constrained to.  No value is recomputed from the inputs, so a
 * stream that passes IS the witness of its inputs (every cell is forced by those constraints).  Takes
 * the buffers and layout of a hsw_witness_blocks(_ex) call (canonical or Montgomery cells -- the latter
 * are reduced on load; pack and frame_* as given
 * there; chip, lookup and next-state pointers may be NULL = not checked).  A Montgomery cell is an encoding
 * m < p: a gate, chip or lookup cell whose stored limbs are >= p is reported (HSW_VERIFY_RANGE, _CHIP, _LOOKUP)
 * although it reduces to a value that satisfies every constraint.  A gate row is evaluated mod p whatever
 * its cells hold, so a forged row that still holds is not what is reported.  Synchronous. */
#define HSW_VERIFY_CONSTANT   1u
#define HSW_VERIFY_COPY       2u
#define HSW_VERIFY_GATE_ROW   3u
#define HSW_VERIFY_ASSERT_EQ  4u
#define HSW_VERIFY_RANGE      5u
#define HSW_VERIFY_CHIP       6u
#define HSW_VERIFY_LOOKUP     7u
#define HSW_VERIFY_NEXT_STATE 8u
typedef struct hsw_verify_report {
    uint64_t violations;       /* 0 = the stream satisfies the constraint system */
    uint64_t checks;           /* individual constraints evaluated */
    uint64_t first_block;      /* earliest failure (valid if violations != 0) */
    int64_t first_cell;        /* block-relative gate cell (lookup entry for HSW_VERIFY_LOOKUP) */
    uint32_t first_class;      /* HSW_VERIFY_* */
    float kernel_ms;
} hsw_verify_report;
struct hsw_witness_args;
int hsw_verify_blocks(hsw_engine *e, const struct hsw_witness_args *args, hsw_verify_report *report);
struct hsw_frame_desc;
struct hsw_pack_plan;
/* The same for the digest frames hsw_witness_frames wrote (one call = equally shaped digests: same
 * n_blocks and range-check setting): prologue and epilogue cells against hsw_frame_structure -- full
 * field arithmetic for the rows with full-width cells -- plus the facts and links of each digest (input
 * length, precomputed rounds, initial state, input bytes, pre-state of block b = next state of block
 * b - 1, the epilogue's candidate states).  first_cell: section-relative, bit 30 set for the epilogue. */
int hsw_verify_frames(hsw_engine *e, const struct hsw_frame_desc *descs, size_t n, const uint8_t *d_blocks,
                      const uint32_t *d_pre_states, const uint32_t *d_next_states, const void *d_gate,
                      const void *d_lookup, const struct hsw_pack_plan *pack, uint32_t flags,
                      hsw_verify_report *report);

typedef struct hsw_witness_args {
    const uint8_t *d_blocks;       /* as hsw_witness_blocks */
    const uint32_t *d_pre_states;
    size_t n_blocks;
    uint64_t spread_cursor0;
    void *d_gate;                  /* where stream cell 0 lands: column base + start_row cells; columns are
                                      max_rows cells apart, so hsw_pack_plan.span_cells cells are addressed */
    void *d_chip_dense, *d_chip_spread;
    size_t chip_col_stride;
    uint32_t *d_next_states;
    void *d_lookup;                /* n_blocks * lookup_cells_per_block cells (HSW_MODE_HALO2_INTERNALS), or NULL */
    uint32_t flags;                /* HSW_REPR_* | HSW_SKIP_* */
    const hsw_pack_plan *pack;     /* NULL = plain linear stream */
    /* Whole-digest streams (HSW_MODE_HALO2_INTERNALS; see "digest frame" below): the blocks are
     * those of consecutive digests of frame_every blocks each, and between the block streams of two
     * digests the gate stream skips frame_cells cells and the lookup stream frame_lookups cells (one
     * digest's epilogue + the next one's prologue, written by hsw_witness_frames).  0 = off. */
    uint64_t frame_every, frame_cells, frame_lookups;
} hsw_witness_args;
int hsw_witness_blocks_ex(hsw_engine *e, const hsw_witness_args *args);

/* Plain SHA-256 chain pre-pass (what makes the blocks of one message
 * independent; lib.rs:188,236): message m has blocks_per_message consecutive
 * blocks in d_blocks; its first pre-state is d_init_states[m*8..] (NULL = the
 * FIPS IV, compression.rs:1003-1012).  Writes the pre-state of every block to
 * d_pre_states (n_messages*blocks_per_message*8 u32).  Asynchronous. */
int hsw_sha256_chain(hsw_engine *e, const uint8_t *d_blocks, size_t n_messages,
                     size_t blocks_per_message, const uint32_t *d_init_states,
                     uint32_t *d_pre_states);

/* Host delivery: inputs and outputs are HOST memory.  Stages the inputs H2D, then
 * expands chunks of 128 blocks on the engine's stream into two device staging
 * slots while the previous chunk drains D2H on a second stream (kernel || copy
 * overlap), and synchronizes.  Any output pointer may be NULL (stream skipped).
 * Fastest with pinned output buffers (hsw_host_alloc, or HSW_HOST_REGISTER);
 * PCIe-bound either way: 2.39 MB per block.  (If spread_cursor0 is not a
 * multiple of num_advice_columns the call falls back to one unpipelined pass.)
 * As on the device, chip cells of the first / last row that belong to the
 * neighbouring calls keep what the caller's buffers hold. */
int hsw_witness_blocks_host(hsw_engine *e, const uint8_t *blocks, const uint32_t *pre_states,
                            size_t n_blocks, uint64_t spread_cursor0, void *gate,
                            void *chip_dense, void *chip_spread, size_t chip_col_stride,
                            uint32_t *next_states, uint32_t flags);

/* Pinned (page-locked) host memory for the buffers of hsw_witness_blocks_host. */
int hsw_host_alloc(size_t bytes, void **out);
void hsw_host_free(void *p);

/* Device memory for witness streams: one contiguous virtual range of `bytes` bytes on `device`, backed by separate
 * physical allocations of up to chunk_bytes each (0 = 4 GiB) through HIP's virtual memory management.  On MI355X the
 * write rate of an HBM-bound launch depends on where its output buffers sit; a gate stream in such a
 * range ran 2-4 % faster than in one plain hipMalloc buffer in every process tried, and was much less sensitive to
 * where the chip columns are (tools/vmmprobe).  Any device pointer works with every entry point of this library;
 * this is an offer, not a requirement.  hsw_device_free waits for the device, unmaps and releases the range;
 * HSW_ERR_INVALID_ARG for a pointer that did not come from hsw_device_alloc.  CAUTION (ROCm 7.2): a probe that
 * unmapped and re-created ranges between launches ended in GPU memory faults after a handful of cycles
 * (tools/vmmprobe), allocating and using ranges never did -- allocate them once, free them at shutdown. */
int hsw_device_alloc(int device, size_t bytes, size_t chunk_bytes, void **out);
int hsw_device_free(void *ptr);

/* Duration in milliseconds of the most recent expansion kernel launched by
 * hsw_witness_blocks on this engine, measured with HIP events recorded on the
 * engine's stream around that launch.  Synchronizes on the stop event. */
int hsw_last_kernel_ms(hsw_engine *e, float *ms);
/* Enable/disable the per-launch event pair (off by default: no overhead). */
int hsw_set_timing(hsw_engine *e, int enabled);

/* The stream / device an engine was created on. */
int hsw_engine_stream(const hsw_engine *e, void **hip_stream, int *device);

/* What the most recent expansion launch of this engine was: the kernel instantiation
 * hsw_expand_kernel<limbs, tile_cells, tile_rows, repr, internals> and its work split.  Lets a
 * measurement name the kernel it timed instead of assuming one (bench.py roofline.kernel). */
typedef struct hsw_launch_info {
    uint32_t limbs;        /* 16 / num_bits_lookup */
    uint32_t tile_cells;   /* cells per tile row = contiguous run of one unit */
    uint32_t tile_rows;    /* units one wave expands per phase */
    uint32_t repr;         /* 0 canonical, 1 Montgomery, 2 compact (8-byte cells) */
    uint32_t internals;    /* engine mode HSW_MODE_HALO2_INTERNALS */
    uint32_t parts;        /* waves per block */
    uint32_t split;        /* 0: every wave takes a share of every phase; 1: one phase program per wave;
                              2: one sub-unit program per wave (tiny batches); + 4: the wide table-path
                              instantiation of a gadget bound by hsw_gadget_bind_columns */
    uint32_t seq;          /* expansion launches of this engine so far (wraps): the difference across a call is the
                              number of expansion launches that call made.  Counts every launch of the streaming and
                              of the small-batch kernel, in every mode -- a call of more than 2^20 blocks is one launch
                              per chunk; frame, chain and verify launches are not counted.  (Was reserved_, always 0.) */
    uint64_t n_blocks;     /* blocks of that launch */
    uint64_t grid;         /* workgroups (= waves) of that launch */
} hsw_launch_info;
int hsw_last_launch(const hsw_engine *e, hsw_launch_info *out);

/* ------------------------------------------------------------------------
 * Gadget front-end: the host side of Sha256DynamicConfig::digest
 * (reference src/lib.rs:71-349) -- SHA-256 padding, zero fill up to the
 * FIXED maximum size, prefix pre-hash, chaining, "select state #n" -- over
 * the engine.  csrc/hsw_gadget.hpp holds the C++ class of the same name
 * (csrc/hsw_gadget_sha.cpp, _context.cpp, _digest.cpp; these entry points:
 * csrc/hsw_gadget.cpp).
 * ------------------------------------------------------------------------ */

typedef struct hsw_digest_info {
    size_t num_round;          /* real rounds incl. the precomputed ones (lib.rs:80-84) */
    size_t precomputed_round;  /* lib.rs:93 */
    size_t target_round;       /* num_round - precomputed_round (lib.rs:147-151) */
    size_t n_blocks;           /* max_variable_byte_size / 64: compressions synthesised (lib.rs:87,180) */
} hsw_digest_info;

/* lib.rs:77-117,153-160 on the host, no GPU: pads `input`, returns the
 * max_variable_byte_size bytes fed to the circuit (blocks_out, may be NULL)
 * and the state after the precomputed prefix (init_state_out, may be NULL).
 * HSW_ERR_SHAPE: max or precomputed length not a multiple of 64 (lib.rs:57-59,89);
 * HSW_ERR_TOO_LARGE: padded message does not fit (lib.rs:90). */
int hsw_digest_prepare(const uint8_t *input, size_t input_len, size_t precomputed_input_len,
                       size_t max_variable_byte_size, uint8_t *blocks_out,
                       uint32_t init_state_out[8], hsw_digest_info *info);

/* ------------------------------------------------------------------------
 * Digest frame: the cells Sha256DynamicConfig::digest itself
 * allocates around its block loop -- the prologue (lib.rs:122-178: lengths,
 * is_less_than_safe, the initial state, the input bytes and their optional
 * 8-bit range checks) and the epilogue (lib.rs:294-341: is_equal/select of the
 * state after round #target, the 32 digest bytes with their range checks and
 * recomposition).  With them the gate stream of one digest() call is, in order,
 *     prologue | [the Context's zero cell, at its first use] | n_blocks x G | epilogue
 * and the lookup-advice stream  prologue_lookups | n_blocks x 3,184 | 64.
 * Cell layout of the halo2-base calls involved (mul, sub, is_zero, is_equal,
 * select, is_less_than, range_check(.,8), the first load_zero) follows
 * halo2-lib v0.2.x: ASSUMPTION A4 (csrc/hsw_frame.hpp), unpinned
 * like A1-A3.  Needs an engine in HSW_MODE_HALO2_INTERNALS; canonical or
 * Montgomery cells (a frame has full-width cells, so no COMPACT64).
 * ------------------------------------------------------------------------ */
typedef struct hsw_frame_shape {
    uint64_t n_blocks;            /* max_variable_byte_size / 64 */
    uint64_t prologue_cells;      /* 46 + max (+ 4*max with is_input_range_check) */
    uint64_t epilogue_cells;      /* 76*(n_blocks + 1) + 288 */
    uint64_t prologue_lookups;    /* 3 (+ 2*max) */
    uint64_t epilogue_lookups;    /* 64 */
    uint64_t prologue_calls;      /* assign_region calls (tape entries) */
    uint64_t epilogue_calls;
    uint64_t digest_cells;        /* prologue + n_blocks*G + epilogue; the zero cell is not counted */
    uint64_t digest_lookups;
} hsw_frame_shape;
/* HSW_ERR_SHAPE: max not a multiple of 64 (lib.rs:57-59); HSW_ERR_TOO_LARGE: max above 2^32 bytes
 * (a frame counts its blocks in 32 bits). */
int hsw_frame_query(const hsw_shape *shape, size_t max_variable_byte_size, int is_input_range_check,
                    hsw_frame_shape *out);
/* The assign_region call lengths of the prologue (section 0) or epilogue
 * (section 1), like hsw_gate_tape.  lens_out may be NULL to query the count. */
int hsw_frame_tape(const hsw_shape *shape, size_t max_variable_byte_size, int is_input_range_check,
                   int section, uint8_t *lens_out, size_t cap, size_t *n_calls);

/* Constraint structure of the prologue (section 0) / epilogue (section 1), like hsw_block_structure.
 * Cell ids are section-relative; negative ids name cells of other sections: HSW_CELL_ZERO,
 * HSW_CELL_TARGET (assigned_target_round: prologue cell 34), HSW_CELL_STATE0 - (8 n + i) (word i of
 * candidate state n: n = 0 the prologue's cells 38..45, n >= 1 the next_state cells of block n - 1).
 * assert_const: pairs (cell, k) from assert_is_const.  Constants: -k stands for p - k. */
#define HSW_CELL_TARGET (-3000)
#define HSW_CELL_STATE0 (-4000)
typedef struct hsw_frame_structure_counts {
    uint64_t cells, gate_rows, assert_eq, assert_const, ranges, lookups;
} hsw_frame_structure_counts;
int hsw_frame_structure(const hsw_shape *shape, size_t max_variable_byte_size, int is_input_range_check,
                        int section, hsw_frame_structure_counts *counts, uint8_t *cell_kind, int64_t *cell_ref,
                        uint32_t *gate_rows, int64_t *assert_eq, int64_t *assert_const, int64_t *range,
                        int64_t *lookup_src);

typedef struct hsw_frame_desc {   /* one digest() call */
    uint64_t input_len;           /* lib.rs:77 */
    uint64_t first_block;         /* this digest's first block in d_blocks / d_pre_states / d_next_states */
    uint64_t prologue_cell;       /* gate-stream cell index where its prologue starts */
    uint64_t epilogue_cell;
    uint64_t prologue_lookup;     /* lookup-stream cell indices */
    uint64_t epilogue_lookup;
    uint64_t zero_cell;           /* gate-stream index of the Context's zero cell if this digest is the
                                     first to call load_zero in its Context, else UINT64_MAX */
    uint32_t n_blocks;            /* >= 1 */
    uint32_t num_round;           /* ceil((input_len + 9) / 64), lib.rs:80-84 (checked) */
    uint32_t precomputed_round;   /* lib.rs:93; num_round - precomputed_round <= n_blocks (lib.rs:90) */
    uint32_t is_input_range_check;
} hsw_frame_desc;
/* Writes the frames of n digests.  d_pre_states / d_next_states are the ones the
 * block expansion read / wrote (the candidate states of lib.rs:296 are
 * pre_states[first_block] and next_states[first_block .. first_block+n_blocks-1]);
 * descs is HOST memory.  d_lookup may be NULL.  pack (may be NULL): FlexGate column
 * breaks in the same absolute gate-stream indices as prologue_cell / epilogue_cell;
 * a frame cell at stream index i is written at i + the gaps of all breaks <= i.
 * Asynchronous on the engine's stream, ordered after earlier hsw_witness_blocks calls. */
int hsw_witness_frames(hsw_engine *e, const hsw_frame_desc *descs, size_t n, const uint8_t *d_blocks,
                       const uint32_t *d_pre_states, const uint32_t *d_next_states, void *d_gate,
                       void *d_lookup, const hsw_pack_plan *pack, uint32_t flags);

/* Block streams AND frames of n equally sized digests in one call: what hsw_witness_blocks_ex (with
 * frame_every = the digests' block count) followed by hsw_witness_frames do.  For up to 128 blocks in digests of
 * up to 32 -- the reference's own bench circuit is one 16-block digest -- it is ONE kernel launch: the frame cells are
 * written by extra waves of the expansion's grid, which take the candidate states from the chain inputs
 * (pre-state of block b + 1 = next state of block b) and compute the last block's output themselves, so
 * nothing waits for the expansion.  Larger batches: the two launches above.
 *   blocks            the block streams, exactly as for hsw_witness_blocks_ex
 *   descs, n_digests  as for hsw_witness_frames; first_block / cell indices relative to the *0 bases
 *   frame_pack        column breaks in absolute cells of d_gate0 (blocks.pack: relative to blocks.d_gate)
 *   host_next_states  optional: pinned host memory (hsw_host_alloc), blocks.n_blocks * 8 words; receives a
 *                     copy of the next states without a separate copy launch.  Valid after the stream has
 *                     been synchronized. */
typedef struct hsw_digests_args {
    hsw_witness_args blocks;
    const hsw_frame_desc *descs;
    size_t n_digests;
    const uint8_t *d_blocks0;
    const uint32_t *d_pre_states0;
    const uint32_t *d_next_states0;
    void *d_gate0, *d_lookup0;
    const hsw_pack_plan *frame_pack;
    uint32_t *host_next_states;
} hsw_digests_args;
int hsw_witness_digests(hsw_engine *e, const hsw_digests_args *args);

typedef struct hsw_gadget hsw_gadget;   /* Sha256DynamicConfig + its Context */

typedef struct hsw_hash_result {        /* AssignedHashResult (lib.rs:31-36) on values */
    uint64_t input_len;                 /* lib.rs:124-125 */
    size_t first_block;                 /* this hash's first block in the gadget's streams */
    size_t n_blocks;
    uint64_t spread_cursor0;            /* SpreadConfig.num_limb_sum when this digest began */
    size_t num_round, target_round;
    uint8_t output_bytes[32];           /* lib.rs:311-341 */
    /* HSW_GADGET_WHOLE_DIGEST only (else 0): where this digest's sections start in the
     * gadget's gate / lookup streams, in cells */
    uint64_t prologue_cell, block_cell, epilogue_cell, end_cell;
    uint64_t prologue_lookup, block_lookup, epilogue_lookup;
} hsw_hash_result;

typedef struct hsw_gadget_view {
    void *d_gate;                       /* capacity_blocks * G cells (device) */
    void *d_chip_dense, *d_chip_spread; /* ncols columns, chip_col_stride cells apart, row 0 = chip row 0 */
    uint32_t *d_next_states;
    size_t chip_col_stride;
    size_t blocks_done, capacity_blocks;
    uint64_t num_limb_sum;              /* spread.rs:26 */
    size_t cur_hash_idx;                /* lib.rs:43 */
    /* HSW_GADGET_WHOLE_DIGEST: d_gate is ONE stream of gate_cells cells (of gate_capacity), the
     * digests back to back with their frames; d_lookup the lookup-advice stream.  Else 0 / NULL. */
    uint64_t gate_cells, gate_capacity;
    void *d_lookup;
    uint64_t lookup_cells, lookup_capacity;
    uint64_t max_rows, columns;         /* hsw_gadget_set_columns: d_gate is columns x max_rows cells; else 0 */
    /* hsw_gadget_set_origin (all 0 by default): image column k is FlexGate column origin_column + k, stream
     * cell 0 sits at row origin_row of image column 0, the gadget's lookup entries start at d_lookup cell
     * origin_lookups (lookup_cells / lookup_capacity count from cell 0 of the buffer) */
    uint64_t origin_column, origin_row, origin_lookups;
    uint32_t origin_zero_loaded, reserved_;
} hsw_gadget_view;

/* Sha256DynamicConfig::configure (lib.rs:49-69) + new_context (lib.rs:351-360):
 * allocates HBM for sum(max_variable_byte_sizes)/64 blocks of streams. */
int hsw_gadget_create(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t n_hashes,
                      int is_input_range_check, hsw_gadget **out);
/* flags: HSW_GADGET_WHOLE_DIGEST = also emit the digest frames (engine must be in
 * HSW_MODE_HALO2_INTERNALS): the gadget's gate stream is then every advice cell the
 * reference's digest() calls allocate, in allocation order. */
#define HSW_GADGET_WHOLE_DIGEST 1u
/* With HSW_GADGET_WHOLE_DIGEST: every digest of the gadget is a synthesis OF ITS OWN -- K proofs of one circuit in
 * flight (the reference's bench circuit is one digest per proof, benches/digest.rs:93-129): each digest gets a
 * fresh Context (its own [Constant(0)] cell, A4-iii; its lookup entries and chip rows start at 0 of its own
 * columns), and hsw_gadget_digest_batch still expands all of them in ONE launch.  The K regions lie back to back
 * in the gadget's streams: digest h's gate cells are [prologue_cell, end_cell) and its lookup entries
 * [prologue_lookup, epilogue_lookup + 64) of hsw_hash_result -- cell for cell what a single-digest gadget writes
 * from cell 0 -- and its chip rows are rows [first_block * limb_calls_per_block / ncols, ...) of the chip columns
 * (needs n_blocks * limb_calls_per_block to be a multiple of num_advice_columns: HSW_ERR_UNSUPPORTED otherwise).
 * Linear streams only unless HSW_GADGET_CONTEXT_IMAGES: without it hsw_gadget_set_columns / hsw_gadget_set_origin
 * return HSW_ERR_UNSUPPORTED. */
#define HSW_GADGET_INDEPENDENT  2u
/* With HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT (else HSW_ERR_INVALID_ARG), and every max_variable_byte_size
 * equal (K proofs of one circuit; else HSW_ERR_UNSUPPORTED): every Context is a column image of its own, all starting
 * at the same Context origin, still written by one launch.  hsw_gadget_set_columns / hsw_gadget_set_origin are
 * accepted and apply to every Context alike (a failing call leaves the previous layout and buffers as they were).
 * Layout of Context (proof) h, S = columns x max_rows, Lp = lookups_already_queued + the digest's own lookup entries:
 *   gate cells     cells [h*S, (h+1)*S) of d_gate; image column k = FlexGate column origin_column + k of proof h; rows
 *                  [0, origin_row) of its column 0 are the caller's: never written, never touched by a delivery
 *   lookup column  cells [h*Lp, (h+1)*Lp) of d_lookup; its first lookups_already_queued cells are the caller's
 *   chip rows      as without the flag: rows [first_block * limb_calls_per_block / ncols, ...) of the chip columns
 *   zero cell      zero_cell_loaded holds for every Context: each stream is then one cell shorter
 * hsw_hash_result gate cells stay gadget-stream indices (the K streams back to back, stream_cells of
 * hsw_context_region each); its lookup indices are d_lookup cells.  hsw_gadget_cell_position /
 * hsw_gadget_result_cells map a stream cell to (FlexGate column, row) inside the owning Context's image.
 * Without hsw_gadget_set_columns the gate cells stay the linear stream (lookups and origin as above).
 * Deliveries: hsw_gadget_download_region writes the K images back to back (host layout = device layout; used rows
 * only); the region tape, distinct delivery and hsw_gadget_replay_region keep their meaning; hsw_gadget_verify and
 * hsw_gadget_place work.  hsw_gadget_download_region_compact and hsw_gadget_seek return HSW_ERR_UNSUPPORTED. */
#define HSW_GADGET_CONTEXT_IMAGES 4u
/* With HSW_GADGET_WHOLE_DIGEST, not with HSW_GADGET_INDEPENDENT / HSW_GADGET_CONTEXT_IMAGES (HSW_ERR_INVALID_ARG);
 * engines with the 8-bit spread table only (HSW_ERR_UNSUPPORTED): every digest of the pass works on the SAME halo2-base
 * Context, and the circuit may assign cells of its own between two digests (the gate / range chips, lib.rs:71-76 takes
 * whatever Context it is handed) -- an interlude, declared with hsw_gadget_set_digest_origin.
 *   - hsw_gadget_set_columns / hsw_gadget_set_origin accept layouts of up to HSW_GADGET_MAX_COLUMNS columns (instead
 *     of HSW_MAX_BREAKS + 1) and clear every declaration; hsw_gadget_reset keeps them, as it keeps the origin.
 *   - hsw_hash_result gate cells stay gadget-stream indices (the interludes take none); hsw_gadget_cell_position /
 *     hsw_gadget_result_cells report the FlexGate (column, row) after the jumps; *_lookup indices are d_lookup cells,
 *     i.e. positions in the Context's whole lookup queue, the caller's entries included.
 *   - interlude cells and lookup entries are the caller's: never written on the device, never touched in the
 *     caller's host buffers by hsw_gadget_download_region / hsw_gadget_replay_region.
 *   - a declaration may grow the image (or the lookup column): the engine is drained, the buffers reallocated and
 *     copied, so device pointers from earlier hsw_gadget_streams calls are stale after it.
 *   - hsw_gadget_verify checks the interludes' layout (the caller's lookup entries are skipped).
 *   - hsw_gadget_seek, hsw_gadget_download_region_compact and hsw_gadget_place return HSW_ERR_UNSUPPORTED.
 * Without the flag every call behaves as before. */
#define HSW_GADGET_SHARED_CONTEXT 8u
/* Columns a HSW_GADGET_SHARED_CONTEXT layout may span (at k = 17 one 1024-byte digest fills 9) */
#define HSW_GADGET_MAX_COLUMNS 1024u
int hsw_gadget_create_ex(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t n_hashes,
                         int is_input_range_check, uint32_t flags, hsw_gadget **out);
/* A Context group: n_contexts Contexts (proofs) of ONE circuit that makes digests_per_context digests -- the
 * reference's Sha256DynamicConfig with max_variable_byte_sizes of that length (lib.rs:40-43,86,347), synthesized K
 * times.  max_variable_byte_sizes lists ONE Context's M = digests_per_context sizes.  Every Context is laid out
 * exactly like a HSW_GADGET_SHARED_CONTEXT gadget of those M sizes (one zero cell, one lookup queue, one run of chip
 * rows, interludes between its digests, up to HSW_GADGET_MAX_COLUMNS columns), and the K layouts repeat like
 * HSW_GADGET_CONTEXT_IMAGES: with S = columns x max_rows and Lp = one Context's whole lookup queue (the caller's
 * queued and interlude entries included), Context c's image is cells [c*S, (c+1)*S) of d_gate, its lookup column
 * cells [c*Lp, (c+1)*Lp) of d_lookup, and its chip rows follow Context c-1's.
 *   flags          must contain HSW_GADGET_WHOLE_DIGEST (HSW_GADGET_SHARED_CONTEXT may be named too); any other bit,
 *                  digests_per_context = 0, n_contexts = 0 or an engine not in HSW_MODE_HALO2_INTERNALS:
 *                  HSW_ERR_INVALID_ARG.  Engines with the 8-bit spread table only (HSW_ERR_UNSUPPORTED), and one
 *                  Context's blocks x limb_calls_per_block must be a multiple of num_advice_columns
 *                  (HSW_ERR_UNSUPPORTED, as for HSW_GADGET_INDEPENDENT).
 *   pass order     digest d = c*M + j of the pass is digest j of Context c.  hsw_gadget_digest /
 *                  hsw_gadget_digest_batch take any n -- a batch may start or end in the middle of a Context -- and
 *                  a pass issued digest by digest, as one batch or in any split writes the same bytes.  A batch
 *                  costs one expansion launch per digest index it holds (M, not K*M) and one frame launch.
 *                  hsw_gadget_set_columns must have been called (HSW_ERR_UNSUPPORTED from the digest calls before).
 *   layout calls   hsw_gadget_set_columns, hsw_gadget_set_origin and hsw_gadget_set_digest_origin(g, j, ...) with
 *                  1 <= j < M describe ONE Context and apply to every Context alike; a call that fails leaves layout
 *                  and buffers as they were.  A call that changes the layout replaces the K images and lookup
 *                  columns by zeroed ones (device pointers from earlier queries are stale; a bound region,
 *                  hsw_gadget_bind_region, is neither replaced nor zeroed); the same declaration
 *                  again, pass after pass, keeps layout, buffers, region tape and the device's jump table.
 *   queries        hsw_gadget_context_region(g, c, ...) describes Context c (assigned: all M digests are).
 *                  hsw_hash_result gate cells are gadget-stream indices, the K Context streams (stream_cells each)
 *                  back to back; its lookup indices are d_lookup cells.  hsw_gadget_cell_position /
 *                  hsw_gadget_result_cells map into the owning Context's image, after its jumps.
 *   deliveries     hsw_gadget_download_region (K images back to back, used cells only), hsw_gadget_region_tape,
 *                  hsw_gadget_download_region_distinct, hsw_gadget_replay_region and hsw_gadget_verify work.  Rows
 *                  above the origin, interlude cells and the caller's lookup entries of EVERY Context are the
 *                  caller's: never written on the device, never touched in host buffers.
 *   refusals       hsw_gadget_seek, hsw_gadget_download_region_compact and hsw_gadget_place: HSW_ERR_UNSUPPORTED. */
int hsw_gadget_create_contexts(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t digests_per_context,
                               size_t n_contexts, int is_input_range_check, uint32_t flags, hsw_gadget **out);
void hsw_gadget_destroy(hsw_gadget *g);
/* HSW_GADGET_WHOLE_DIGEST, before the first digest: lay the gate stream out as the
 * FlexGate (Vertical) advice columns themselves -- column c = cells [c*max_rows,
 * (c+1)*max_rows) of d_gate, every assign_region call placed by the v0.2.x rule
 * `row + len >= max_rows -> next column` (assumption A3-iii), unassigned tail rows 0 (a bound
 * region, hsw_gadget_bind_region: columns column_pitch cells apart, unassigned cells the caller's, never zeroed).
 * max_rows = the gate's usable rows (RangeConfig.gate.max_rows, lib.rs:355).  The
 * layout depends only on max_variable_byte_sizes, never on the messages.
 * HSW_ERR_TOO_LARGE: more than HSW_MAX_BREAKS + 1 columns (HSW_GADGET_MAX_COLUMNS with HSW_GADGET_SHARED_CONTEXT). */
int hsw_gadget_set_columns(hsw_gadget *g, uint64_t max_rows, uint64_t *n_columns);
/* HSW_GADGET_WHOLE_DIGEST, before the first digest of a synthesis pass (fresh, or after hsw_gadget_reset;
 * before or after hsw_gadget_set_columns): where the caller's halo2-base Context stands when it hands
 * the region to the gadget.  The reference's digest() works on whatever Context it is given
 * (lib.rs:71-76, 351-360) -- a circuit that has used the gate / range chips before its first digest is
 * the normal case outside the reference's two harnesses.
 *   column, row              ctx.advice_alloc[0]: the FlexGate column in use and its next free row.
 *                            Stream cell 0 lands there and the column breaks follow from it (A3-iii);
 *                            with a column image, image column k = FlexGate column `column + k`, rows
 *                            [0, row) of image column 0 belong to the caller: they are never written by
 *                            the gadget and never touched in the caller's host buffers by the downloads.
 *                            hsw_gadget_cell_position / hsw_gadget_result_cells report FlexGate columns.
 *   zero_cell_loaded         ctx.zero_cell.is_some(): the Context already caches its [Constant(0)] cell
 *                            (A4-iii), so no digest of this gadget assigns one -- the stream is one cell
 *                            shorter and hsw_frame_desc.zero_cell is never set.
 *   lookups_already_queued   ctx.cells_to_lookup.len(): RangeConfig::finalize (lib.rs:469) copies the queue
 *                            into the lookup-advice column in order, so the gadget's entries start at that
 *                            index: d_lookup is reallocated with that many leading cells (zero, the
 *                            caller's; a bound region is never reallocated or zeroed, hsw_gadget_bind_region),
 *                            every *_lookup index of hsw_hash_result counts from cell 0.
 * The origin survives hsw_gadget_reset (the next synthesis of the same circuit starts at the same place).
 * HSW_ERR_INVALID_ARG: not a whole-digest context, digests already assigned in this pass, or row >= max_rows;
 * HSW_ERR_TOO_LARGE: the layout from that row needs more than HSW_MAX_BREAKS + 1 columns (the previous
 * origin and layout are kept). */
int hsw_gadget_set_origin(hsw_gadget *g, uint64_t column, uint64_t row, int zero_cell_loaded,
                          uint64_t lookups_already_queued);
/* HSW_GADGET_SHARED_CONTEXT with a column image: where the Context stands just before digest h of the pass, after the
 * caller's own cells since digest h-1 -- column, row = ctx.advice_alloc[0], lookups_queued = ctx.cells_to_lookup.len().
 * Digest h's prologue lands at (column, row); its lookup entries start at d_lookup cell lookups_queued.  The layout
 * depends only on max_variable_byte_sizes and the declarations, never on the messages: a batch prover may declare
 * every origin first and run the pass as one hsw_gadget_digest_batch.  Declaring h drops the declarations of every
 * later digest -- unless it repeats h's current declaration, which changes nothing (a prover that declares the same
 * interludes pass after pass keeps its layout, its device table and its tape positions).  A declaration that changes
 * the layout zeroes the image cells past digest h-1's end again (what an earlier layout wrote there; not in a bound
 * region, hsw_gadget_bind_region: its cells are the caller's, and a layout past its capacities is HSW_ERR_TOO_LARGE).  HSW_ERR_INVALID_ARG, with the layout unchanged: not a shared context or no column image, h = 0 or
 * h >= n_hashes, digest h already assigned in this pass, row >= max_rows, (column, row) before the next free cell
 * after digest h-1's layout (in (column, row) order), or lookups_queued below the queue length after digest h-1.
 * HSW_ERR_TOO_LARGE: the layout would need more than HSW_GADGET_MAX_COLUMNS columns. */
int hsw_gadget_set_digest_origin(hsw_gadget *g, size_t h, uint64_t column, uint64_t row, uint64_t lookups_queued);
/* Bind the gadget's region to device memory the CALLER owns -- a prover that keeps every advice column as a polynomial
 * of n = 2^k cells in HBM gets the cells written straight into its own columns, no copy afterwards.  For
 * HSW_GADGET_WHOLE_DIGEST gadgets with a column image (hsw_gadget_set_columns first: HSW_ERR_UNSUPPORTED without it,
 * and for linear or block-stream gadgets): the plain single image, HSW_GADGET_SHARED_CONTEXT,
 * HSW_GADGET_CONTEXT_IMAGES and hsw_gadget_create_contexts; 32-byte cells, canonical or Montgomery.
 * Cells, not bytes, throughout; image column k is FlexGate column origin_column + k as before.
 *   d_columns, column_pitch      image column k of proof c starts at cell c * context_pitch + k * column_pitch;
 *                                max_rows <= column_pitch <= 2^24, odd values included.  Rows [max_rows,
 *                                column_pitch) of a column (a prover's blinding rows) are never written.
 *   columns_capacity             image columns reserved per proof: the layout's `columns` must fit
 *   context_pitch                K > 1 proofs: >= columns_capacity * column_pitch
 *   d_lookup, lookup_capacity    the lookup-advice column of proof c starts at cell c * lookup_pitch and holds
 *   lookup_pitch                 lookup_capacity cells (>= Lp, the cells the layout needs); lookup_pitch >= lookup_capacity
 *   d_chip_dense, d_chip_spread  chip column k of proof c starts at cell c * chip_context_pitch + k * chip_col_stride and
 *   chip_col_stride              holds chip_rows_capacity rows (>= one proof's chip rows; chip_col_stride >=
 *   chip_rows_capacity           chip_rows_capacity).  Library-owned, proof c's rows follow proof c-1's in the same
 *   chip_context_pitch           columns; bound, every proof has chip rows of its own
 * A single-proof gadget ignores context_pitch, lookup_pitch and chip_context_pitch.  b = NULL: back to library-owned,
 * zeroed buffers (nothing to do on an unbound gadget).
 * When: on a fresh or reset gadget only (HSW_ERR_INVALID_ARG after the first digest of a pass).  The binding survives
 * hsw_gadget_reset and every layout call whose result still fits the declared capacities (hsw_gadget_set_columns with
 * max_rows <= column_pitch, hsw_gadget_set_origin, hsw_gadget_set_digest_origin); one that does not fit returns
 * HSW_ERR_TOO_LARGE and leaves layout and binding as they were -- a bound shared context never grows its image.
 * Checks, each leaving the previous binding or the library's buffers in place: a null pointer or one that is not
 * 128-byte aligned (whole lines for the realigned write-out), or a pitch below its minimum: HSW_ERR_INVALID_ARG; a
 * capacity below what the layout needs (columns, Lp, one proof's chip rows): HSW_ERR_TOO_LARGE.  The four areas must
 * be disjoint and live on the engine's device: the library does NOT check that.
 * Ownership: binding drains the engine and frees the library's own image, lookup and chip buffers.  Caller memory is
 * never freed, grown, zeroed or filled: cells the layout does not assign keep whatever the caller put there (a prover
 * zeroes its polynomials once) -- on a bound gadget this replaces every "zeroed" / "zeroed again" clause of
 * hsw_gadget_set_columns, hsw_gadget_set_origin, hsw_gadget_set_digest_origin and hsw_gadget_create_contexts.
 * What follows the binding with unchanged meaning: hsw_gadget_streams and hsw_gadget_context_region report the bound
 * pointers (chip_col_stride the bound one); hsw_gadget_cell_position / hsw_gadget_result_cells return the same
 * (FlexGate column, row) as an unbound gadget -- binding changes addresses, never positions; hsw_gadget_verify;
 * hsw_gadget_download_region / hsw_gadget_replay_region with host buffers laid out like the device (pitches included,
 * used rows only); the distinct delivery, whose 32-bit image positions now bound context_pitch x K (columns x
 * column_pitch for one proof): HSW_ERR_TOO_LARGE at 2^32 cells.  hsw_gadget_place, hsw_gadget_download_region_compact
 * and hsw_gadget_seek return HSW_ERR_UNSUPPORTED on a bound gadget. */
typedef struct hsw_region_binding {
    void    *d_columns;          /* image column 0 of proof 0 */
    uint64_t column_pitch;       /* cells from image column k to k+1;          >= max_rows */
    uint64_t columns_capacity;   /* image columns the caller reserved per proof */
    uint64_t context_pitch;      /* cells from proof c to c+1 (K > 1);         >= columns_capacity * column_pitch */
    void    *d_lookup;           /* lookup-advice column of proof 0 */
    uint64_t lookup_capacity;    /* cells per proof */
    uint64_t lookup_pitch;       /* cells from proof c to c+1;                 >= lookup_capacity */
    void    *d_chip_dense, *d_chip_spread;   /* chip row 0 of chip column 0 of proof 0 */
    uint64_t chip_col_stride;    /* cells from chip column k to k+1 */
    uint64_t chip_rows_capacity; /* rows per chip column per proof */
    uint64_t chip_context_pitch; /* cells from proof c to c+1 */
} hsw_region_binding;
int hsw_gadget_bind_region(hsw_gadget *g, const hsw_region_binding *b);   /* b = NULL: back to library-owned, zeroed buffers */
/* The geometry in force, also when library-owned (then: d_gate / max_rows / columns x max_rows, Lp, consecutive chip rows).
 * Columns by pointer table (hsw_gadget_bind_columns): d_columns = image column 0 of proof 0 and context_pitch = 0 --
 * "columns by pointer table": the other columns are wherever the caller's table said, no pitch describes them. */
int hsw_gadget_region_binding(const hsw_gadget *g, hsw_region_binding *out);
/* Like hsw_gadget_bind_region, but the FlexGate image columns are given one pointer each -- a prover that holds its
 * advice as one allocation per column per proof (halo2_proofs' Vec<Polynomial<F>>), in no address order:
 *   d_column_ptrs[c * b->columns_capacity + k] = device address of row 0 of image column k of proof c
 * (host array of n_ptrs = K * columns_capacity pointers, copied by the call; K = 1 for single-proof gadgets).
 * b->d_columns and b->context_pitch are ignored; b->column_pitch = cells each column allocation holds
 * (max_rows <= column_pitch <= 2^24; rows [max_rows, column_pitch) are never written); the lookup and chip areas
 * exactly as in hsw_gadget_bind_region (they keep the pitch model).  Same gadget kinds, same "fresh or reset gadget
 * only", same ownership rules, 32-byte cells, canonical or Montgomery; hsw_gadget_bind_region(g, NULL) unbinds.
 * HSW_ERR_INVALID_ARG: a null pointer or one not 128-byte aligned (table entries included), n_ptrs != K *
 * columns_capacity, a pitch out of range; HSW_ERR_TOO_LARGE: columns_capacity below the layout's columns, or a lookup /
 * chip capacity below what the layout needs; HSW_ERR_UNSUPPORTED without a column image.  A failing call leaves the
 * previous binding or the library's buffers in place.  Disjointness and device residency are NOT checked.
 * The binding survives hsw_gadget_reset and every layout call whose result still fits; a layout that needs more
 * columns than columns_capacity returns HSW_ERR_TOO_LARGE and changes nothing.
 * Binding changes addresses, never positions: hsw_gadget_cell_position, hsw_gadget_result_cells and hsw_hash_result
 * are those of an unbound gadget.  hsw_gadget_streams reports proof 0's column-0 pointer as d_gate and
 * hsw_gadget_context_region(g, c) proof c's column-0 pointer as d_image -- the further columns are the caller's
 * table's, not d_gate + a pitch.  hsw_gadget_verify works.  hsw_gadget_download_region works: its `gate` host buffer
 * is laid out as an UNBOUND gadget's (K images of columns x max_rows cells back to back, used rows only -- a host
 * buffer cannot mirror scattered device allocations), its lookup and chip buffers as for a pitch-bound gadget.
 * hsw_gadget_region_tape works (host only).  hsw_gadget_download_region_distinct, hsw_gadget_replay_region,
 * hsw_gadget_download_region_compact, hsw_gadget_seek and hsw_gadget_place return HSW_ERR_UNSUPPORTED.
 * hsw_last_launch reports such a gadget's expansion launches with bit 2 of `split` set (split = 4 or 6): the wide
 * instantiations hsw_expand_table_kernel<.., true> / hsw_small_table_kernel<.., true>. */
int hsw_gadget_bind_columns(hsw_gadget *g, const hsw_region_binding *b, void *const *d_column_ptrs, size_t n_ptrs);
/* Like hsw_gadget_bind_columns, with the lookup-advice column and the chip columns by pointer table too: a prover
 * whose allocator hands out EVERY advice column one at a time (K lookup columns, 2 x K x ncols chip columns, ncols =
 * num_advice_columns) in no address order.  All tables are host arrays, copied by the call:
 *   d_column_ptrs, n_column_ptrs   K * b->columns_capacity, as hsw_gadget_bind_columns (required: without an image
 *                                  table this is hsw_gadget_bind_region)
 *   d_lookup_ptrs, n_lookup_ptrs   K: [c] = row 0 of proof c's lookup-advice column, an allocation of
 *                                  b->lookup_capacity cells.  NULL / 0: the pitch model of b
 *   d_chip_dense_ptrs,             K * ncols each: [c * ncols + k] = row 0 of chip column k of proof c, an allocation
 *   d_chip_spread_ptrs,            of b->chip_rows_capacity rows.  Both families or neither; NULL / 0: the pitch
 *   n_chip_ptrs                    model of b
 * The two families are independent: lookup pointers with pitch-model chips, or the other way round.  Where a table
 * is given the matching fields of b are ignored: d_lookup and lookup_pitch; d_chip_dense, d_chip_spread,
 * chip_col_stride and chip_context_pitch.  Gadget kinds, "fresh or reset gadget only", ownership, lifetime (the
 * binding survives hsw_gadget_reset and every layout call that still fits) and every refusal are those of
 * hsw_gadget_bind_columns; hsw_gadget_bind_region(g, NULL) unbinds.  Caller memory is never freed, grown, zeroed or
 * filled; unassigned cells keep the caller's content.
 * HSW_ERR_INVALID_ARG: t or the image table missing, a table of the wrong size, one chip family without the other, a
 * null table entry or one not 128-byte aligned; HSW_ERR_TOO_LARGE: lookup_capacity below Lp, chip_rows_capacity below
 * one proof's chip rows, columns_capacity below the layout's columns.  The whole call is validated before anything
 * changes: a failing call leaves the previous binding or the library's buffers in place.
 * Positions are unchanged (hsw_gadget_cell_position, hsw_gadget_result_cells, hsw_hash_result: binding changes
 * addresses, never positions).  hsw_gadget_streams reports proof 0's lookup pointer and chip column-0 pointers and
 * hsw_gadget_context_region(g, c) proof c's; hsw_gadget_region_binding reports proof 0's pointers with lookup_pitch,
 * respectively chip_col_stride and chip_context_pitch, = 0 for a family bound by table -- the further columns are
 * the caller's table's, no pitch describes them (the convention of context_pitch = 0).  hsw_gadget_verify reads
 * through the tables.  hsw_gadget_download_region lays its host `lookup`, `chip_dense` and `chip_spread` buffers out
 * as an UNBOUND gadget's (like `gate`): K lookup columns of Lp cells back to back, ncols chip columns of K x (one
 * proof's rows) each, proof c's rows after proof c-1's; used rows only, everything else in the host buffers is left
 * untouched. */
typedef struct hsw_column_tables {
    void *const *d_column_ptrs;      size_t n_column_ptrs;
    void *const *d_lookup_ptrs;      size_t n_lookup_ptrs;
    void *const *d_chip_dense_ptrs;
    void *const *d_chip_spread_ptrs; size_t n_chip_ptrs;
} hsw_column_tables;
int hsw_gadget_bind_column_tables(hsw_gadget *g, const hsw_region_binding *b, const hsw_column_tables *t);
/* Start the next synthesis pass with the same buffers and layout: every cursor back to
 * its initial value (cur_hash_idx, num_limb_sum, the stream cursors, the Context's zero
 * cell).  What the reference's harnesses do by cloning the config per synthesis
 * (lib.rs:440, benches/digest.rs:78).  Waits for outstanding work on the engine. */
int hsw_gadget_reset(hsw_gadget *g);
/* Host delivery of what the gadget has written so far (a CPU prover reads advice columns from host
 * memory).  Every pointer may be NULL (skipped).  Layouts equal the device ones: `gate` is the column
 * image (columns x max_rows cells; only the used rows of each column are copied) or, without
 * hsw_gadget_set_columns, the linear stream; `lookup` the lookup-advice stream (whole-digest contexts);
 * `chip_dense` / `chip_spread` ncols columns chip_col_stride cells apart (used rows copied).  One pass
 * of asynchronous copies on the engine's stream, then a synchronize; fastest into pinned memory
 * (hsw_host_alloc).  PCIe-bound: the bench circuit's region is 37 MB. */
typedef struct hsw_region_host {
    void *gate, *lookup, *chip_dense, *chip_spread;
} hsw_region_host;
int hsw_gadget_download_region(hsw_gadget *g, const hsw_region_host *dst);
/* The same delivery in the compact transport form: canonical cells travel as their low 64 bits (a quarter
 * of the bytes over PCIe) and the few cells of a region that do not fit -- the field negations of ch, -2^16,
 * the negative differences and is_zero inverses of the frames -- as a side list of (stream, cell index, four
 * limbs).  Layouts as in hsw_gadget_download_region with 8-byte cells (a column image travels in one piece:
 * the unassigned rows at the end of a column arrive as the zeros they are on the device); `wide` receives up to wide_cap entries
 * (in no particular order), n_wide how many the region has (HSW_ERR_TOO_LARGE if more than wide_cap: a block
 * has at most 256, a frame a few dozen).  hsw_region_widen rebuilds one stream's 32-byte cells on the host.
 * Canonical representation only (Montgomery cells are all full width). */
#define HSW_STREAM_GATE        0u
#define HSW_STREAM_LOOKUP      1u
#define HSW_STREAM_CHIP_DENSE  2u
#define HSW_STREAM_CHIP_SPREAD 3u
typedef struct hsw_wide_cell {
    uint64_t stream;               /* HSW_STREAM_* */
    uint64_t index;                /* cell index in that stream's buffer */
    uint64_t value[4];             /* canonical little-endian limbs */
} hsw_wide_cell;
typedef struct hsw_region_compact {
    uint64_t *gate, *lookup, *chip_dense, *chip_spread;     /* host buffers, 8 bytes per cell; NULL = skipped */
    hsw_wide_cell *wide;
    size_t wide_cap;
    size_t n_wide;                                          /* out */
} hsw_region_compact;
int hsw_gadget_download_region_compact(hsw_gadget *g, hsw_region_compact *dst);
/* Host helper: cells32[i] = compact[i] widened to 32 bytes, then the side-list entries of `stream_id`
 * (indices relative to the same buffer) copied over them. */
int hsw_region_widen(const uint64_t *compact, size_t n_cells, uint64_t stream_id, const hsw_wide_cell *wide,
                     size_t n_wide, void *cells32);
/* ---- distinct-value delivery of a whole region (HSW_GADGET_WHOLE_DIGEST contexts, 32-byte cells) ----
 * About 60 % of a region's cells repeat an earlier cell (QuantumCell::Existing, lookup-column copies, the
 * spread-chip cells tied to gate cells: spread.rs:209-210,226-227) or hold a gate constant, at positions that do not
 * depend on the input.  So only the NEW witnesses need to cross PCIe:
 *   hsw_gadget_region_tape              the input-independent half, built once per layout on the host: for every
 *                                       cell of the gate / lookup / chip streams assigned so far either
 *                                       HSW_TAPE_CONST | k (consts[k]) or the index of a distinct value -- copy
 *                                       chains already resolved, so cell i is simply  value(code[i])
 *   hsw_gadget_download_region_distinct packs the distinct values on the device (one gather launch) and copies
 *                                       them to `distinct` (cap_cells 32-byte cells, ideally pinned: hsw_host_alloc),
 *                                       in the gadget's representation (Montgomery for a halo2 prover)
 *   hsw_gadget_replay_region            rebuilds what hsw_gadget_download_region delivers -- column image (or
 *                                       linear stream), lookup column, chip columns; layouts and the
 *                                       "never touch the caller's cells" rules as there -- from the distinct
 *                                       values, with `threads` host threads (pure host work; a consumer that
 *                                       walks the region cell by cell anyway can read value(code[i]) itself)
 * The tape numbers STREAM cells, so it survives hsw_gadget_reset, a new column height and a new origin column /
 * row / lookup count (a prover that synthesizes one circuit pass after pass builds it once); its pointers stay
 * valid until hsw_gadget_set_origin is given a different zero_cell_loaded or the gadget is destroyed.  HSW_ERR_TOO_LARGE: cap_cells too small (*n_cells says how many), or a region of 2^30 cells or more. */
#define HSW_TAPE_CONST 0x80000000u
typedef struct hsw_region_tape {
    uint64_t n_distinct;                 /* distinct values of the digests assigned so far in this pass */
    uint64_t distinct_capacity;          /* ... of all digests of the gadget: size a reusable buffer with this */
    uint64_t gate_cells, lookup_cells, limb_calls;   /* entries of the code arrays that are assigned so far */
    const uint32_t *gate_code;           /* per gate-stream cell (hsw_gadget_cell_position gives its column / row) */
    const uint32_t *lookup_code;         /* per lookup entry of the gadget (entry j sits at d_lookup cell origin_lookups + j;
                                            shared contexts: after the caller's entries of every interlude before it) */
    const uint32_t *chip_dense_code, *chip_spread_code;   /* per limb call n: column n % ncols, row n / ncols */
    const void *consts;                  /* n_consts 32-byte cells in the gadget's current representation */
    uint64_t n_consts;
} hsw_region_tape;
int hsw_gadget_region_tape(hsw_gadget *g, hsw_region_tape *out);
int hsw_gadget_download_region_distinct(hsw_gadget *g, void *distinct, size_t cap_cells, size_t *n_cells);
int hsw_gadget_replay_region(hsw_gadget *g, const void *distinct, const hsw_region_host *dst, unsigned threads);

/* Buffer placement.  On MI355X the same HBM-bound batch runs up to 8 % faster or slower depending on which pair of
 * allocations its gate stream and its chip columns live in, and nothing in user space predicts it.
 * On a fresh or reset gadget: allocate the chip columns up to `candidates` (1..16) times, time the gadget's own batch
 * (every digest an empty message, through hsw_gadget_digest_batch) on each and keep the fastest; the others are
 * freed, the gadget is left reset.  ms_each (candidates floats, may be NULL) receives every candidate's batch time,
 * *kept (may be NULL) the index kept.  Worth calling once for gadgets of a few hundred blocks or more; a
 * latency-bound single digest does not care. */
int hsw_gadget_place(hsw_gadget *g, unsigned candidates, float *ms_each, unsigned *kept);

/* Position the context as if digests #0 .. #hash_idx-1 had already been assigned: every cursor
 * (cur_hash_idx, num_limb_sum, the gate / lookup stream cursors, the zero cell) takes the value it
 * would have then.  All of them follow from max_variable_byte_sizes alone -- never from the
 * messages -- so the digests of one circuit can be dealt to several GPUs (one gadget each, same
 * configuration): rank r seeks to its first digest and assigns its share into the same positions
 * the serial reference would use; no exchange is needed to agree on the layout. */
int hsw_gadget_seek(hsw_gadget *g, size_t hash_idx);
/* Check everything the gadget has written so far against the constraint system, on the device:
 * hsw_verify_blocks on every run of blocks + hsw_verify_frames on their frames (whole-digest contexts;
 * linear stream or column image), or hsw_verify_blocks alone (block-stream contexts).  Canonical or
 * Montgomery cells; the canonical-encoding rule of hsw_verify_blocks holds for every frame cell, the Context's zero
 * cell and every frame lookup entry too (HSW_VERIFY_RANGE / HSW_VERIFY_LOOKUP).  report->first_block counts the gadget's blocks (hsw_hash_result.first_block), whichever
 * launch found the failure. */
int hsw_gadget_verify(hsw_gadget *g, hsw_verify_report *report);
/* (column, row) of gate-stream cell `cell` (identity on row without set_columns). */
int hsw_gadget_cell_position(const hsw_gadget *g, uint64_t cell, uint64_t *column, uint64_t *row);
/* HSW_GADGET_CONTEXT_IMAGES: where proof h lives on the device -- what a prover batching K proofs hands to its h-th
 * proof.  32-byte cells in the gadget's representation.  HSW_ERR_INVALID_ARG without the flag or for h >= K. */
typedef struct hsw_context_region {
    void *d_image;                      /* columns x max_rows cells, column k = FlexGate column origin_column + k
                                           (without hsw_gadget_set_columns: the proof's linear stream) */
    void *d_lookup;                     /* lookup_cells cells; [0, origin_lookups) are the caller's */
    void *d_chip_dense, *d_chip_spread; /* the proof's chip row 0 of chip column 0; column c is c * chip_col_stride further */
    uint64_t columns, max_rows;
    uint64_t last_column_rows;          /* rows of image column columns - 1 the proof uses */
    uint64_t stream_cells;              /* gate-stream cells of one proof */
    uint64_t first_stream_cell;         /* h * stream_cells: the proof's first gadget-stream cell (hsw_hash_result) */
    uint64_t lookup_cells;              /* Lp */
    uint64_t chip_rows;                 /* chip rows of one proof */
    uint64_t chip_col_stride;
    uint64_t origin_column, origin_row, origin_lookups;
    uint32_t assigned;                  /* 1 once proof h has been digested in this synthesis pass */
    uint32_t reserved_;
} hsw_context_region;
/* (hsw_gadget_create_contexts gadgets: h counts Contexts; chip_rows are the rows of its M digests, assigned = all M are) */
int hsw_gadget_context_region(const hsw_gadget *g, size_t h, hsw_context_region *out);
/* Sha256DynamicConfig::digest (lib.rs:71-349); precomputed_input_len 0 = None.
 * Synchronous: returns once the streams of this hash are in HBM. */
int hsw_gadget_digest(hsw_gadget *g, const uint8_t *input, size_t input_len,
                      size_t precomputed_input_len, hsw_hash_result *result);
/* n consecutive digest() calls as ONE kernel launch (results as if sequential). */
int hsw_gadget_digest_batch(hsw_gadget *g, size_t n, const uint8_t *const *inputs,
                            const size_t *input_lens, const size_t *precomputed_input_lens,
                            hsw_hash_result *results);
/* hsw_gadget_digest_batch with the message bytes in DEVICE memory.  d_inputs, input_lens and
 * precomputed_input_lens are HOST arrays of n entries; d_inputs[i] is a device pointer of any byte alignment to
 * input_lens[i] readable bytes (may be NULL when input_lens[i] == 0).  The host never reads the bytes: ONE kernel
 * launch pads every message, hashes its precomputed prefix and stages its blocks, reading no 16-byte granule that
 * holds no byte of the message.
 * Synchronous, like hsw_gadget_digest_batch.  The bytes must be complete before the call: the caller has either
 * synchronised their producer or produced them on the stream the engine was created with.  The buffers must not
 * overlap anything the gadget writes, bound columns included.  Everything else is the host-fed call's, for every
 * kind of gadget and binding: results, cursors, hsw_gadget_result_cells, hsw_gadget_input_bytes (the padded bytes
 * come back with the states, 64 bytes per block), hsw_gadget_verify, seek, reset and every delivery.
 * Argument errors are the host-fed call's too, decided from the lengths alone before anything is launched or
 * committed: HSW_ERR_SHAPE (lib.rs:89), HSW_ERR_TOO_LARGE (lib.rs:90; also a message above 4 GiB),
 * HSW_ERR_INVALID_ARG for a NULL pointer with a non-zero length or a batch past the gadget's capacity. */
int hsw_gadget_digest_batch_device(hsw_gadget *g, size_t n, const void *const *d_inputs,
                                   const size_t *input_lens, const size_t *precomputed_input_lens,
                                   hsw_hash_result *results);
/* hsw_gadget_digest_batch_device for messages that DEPEND on each other's digests: a Merkle tree, an iterated hash,
 * a transcript that absorbs a digest -- in one call, with no host read between the dependency levels.
 * The n messages are the gadget's next n digests in digest order, exactly as for hsw_gadget_digest_batch_device.
 * levels (HOST array, n entries; NULL: every message is of level 0): levels[i] is message i's dependency level,
 * in any order and with gaps -- in a Context group the trees of the proofs interleave.
 * d_outputs (HOST array, n entries; NULL, or NULL entries: no destination): d_outputs[i] is a device pointer of any
 * byte alignment to 32 writable bytes that receive digest i, big-endian as in hsw_hash_result.output_bytes; no byte
 * outside those 32 is written, read or rewritten.
 * A message may read bytes that a message of a STRICTLY LOWER level of the same call writes: one hsw_ingest_kernel
 * launch per distinct level, in ascending order, back to back on the engine's stream, then the expansion once over
 * the whole batch.  Results, hsw_gadget_input_bytes, hsw_gadget_verify and everything else are the device-fed call's,
 * for every kind of gadget and binding.  Every level equal and d_outputs == NULL: hsw_gadget_digest_batch_device.
 * Refused with HSW_ERR_INVALID_ARG, from the pointers and lengths alone, before anything is launched or committed,
 * hsw_last_error naming the two messages: two outputs whose 32-byte ranges overlap; an input range
 * [d_inputs[i], + input_lens[i]) that overlaps the output of a message whose level is not strictly lower (the same
 * level is a race, a higher level reads stale bytes).  The argument errors of hsw_gadget_digest_batch_device apply
 * unchanged.  Outputs, like inputs, must not overlap anything the gadget writes, bound columns included: this is
 * NOT checked.  Bytes that no message of the call writes must be complete before the call, as above. */
int hsw_gadget_digest_levels_device(hsw_gadget *g, size_t n, const void *const *d_inputs,
                                    const size_t *input_lens, const size_t *precomputed_input_lens,
                                    const uint32_t *levels, void *const *d_outputs,
                                    hsw_hash_result *results);
int hsw_gadget_streams(hsw_gadget *g, hsw_gadget_view *view);
/* Where the cells of digest #hash_idx's AssignedHashResult (lib.rs:31-36, 342-346) sit -- what a shim
 * needs to hand back to the circuit (the reference's TestCircuit constrains output_bytes to its instance
 * column, lib.rs:480-482).  HSW_GADGET_WHOLE_DIGEST contexts only.  Cells are gate-stream indices;
 * positions (column, row) of the same cells in the FlexGate image (identity column 0 without set_columns). */
typedef struct hsw_result_cells {
    uint64_t input_len_cell;            /* load_witness(input_byte_size), lib.rs:124-125 */
    uint64_t input_bytes_cell0;         /* assigned_input_bytes[i] = cell input_bytes_cell0 + i (lib.rs:170-173) */
    uint64_t n_input_bytes;             /* max_variable_byte_size */
    uint64_t output_byte_cells[32];     /* the load_witness cells of the digest bytes (lib.rs:317-324) */
    uint64_t input_len_pos[2];          /* (column, row) */
    uint64_t input_bytes_pos0[2];       /* of input byte 0; byte i follows at i rows below unless a column break
                                           lies in between: hsw_gadget_cell_position(input_bytes_cell0 + i) */
    uint64_t output_byte_pos[32][2];
} hsw_result_cells;
int hsw_gadget_result_cells(const hsw_gadget *g, size_t hash_idx, hsw_result_cells *out);
/* ---- digest-to-digest copy constraints ("ties") of a pass: HSW_GADGET_WHOLE_DIGEST gadgets (else HSW_ERR_UNSUPPORTED) ----
 * hsw_block_structure / hsw_frame_structure give a replayer every copy constraint INSIDE a digest; what makes the
 * digests of a pass a Merkle tree or a hash chain is one more family: input-byte cell k of a parent equals
 * output-byte cell j of a child.  The gadget records them from what the device-fed calls were handed:
 *   - every destination d_outputs[i] of hsw_gadget_digest_levels_device, with the digest that wrote it; a later write
 *     of the same pass to the same bytes, in the same or a later call, replaces the earlier owner byte by byte;
 *   - every device-fed message (either device-fed call) is intersected with the destinations written before it -- a
 *     strictly lower level of the same call, any earlier call of the pass.  Every byte they share is one tie; partial
 *     overlaps and destinations of any byte alignment give exactly the shared bytes.
 * dst_byte indexes the digest's assigned input bytes (hsw_result_cells.input_bytes_cell0 + dst_byte), which start
 * AFTER the precomputed prefix: dst_byte = offset in the message - precomputed_input_len.  A shared byte inside the
 * prefix has no cell: it is not tied, it is counted in *prefix_bytes_untied.  Host-fed digests produce no ties.
 * hsw_gadget_reset clears the record; nothing of it lives on the device.  The list is what the circuit adds as
 * constrain_equal(src_cell, dst_cell); a caller that expects a tree asserts *n == 64 per inner node.
 * hsw_gadget_ties: ties in (dst_hash, dst_byte) order.  *n (may be NULL) is always set; out = NULL only queries;
 * cap < *n: HSW_ERR_TOO_LARGE, nothing written.  prefix_bytes_untied may be NULL.
 * (The four calls below came under HSW_ABI_MINOR 1 like the device-fed calls: probe for the symbol.) */
typedef struct hsw_cell_tie {
    uint64_t src_hash, dst_hash;     /* digests in gadget order (a Context group: c*M + m) */
    uint32_t src_byte, dst_byte;     /* output byte 0..31; index into input_bytes */
    uint64_t src_cell, dst_cell;     /* gate-stream cells: hsw_result_cells.output_byte_cells[src_byte],
                                        input_bytes_cell0 + dst_byte */
} hsw_cell_tie;
typedef struct hsw_tie_report {
    uint64_t violations, checks, first; /* first: lowest failing index (valid if violations) */
    float kernel_ms;
} hsw_tie_report;
int hsw_gadget_ties(const hsw_gadget *g, hsw_cell_tie *out, size_t cap, size_t *n, uint64_t *prefix_bytes_untied);
/* Device address of gate-stream cell `cell` in the layout and binding in force -- what hsw_gadget_cell_position plus
 * the binding's geometry give: the linear stream, a column image at its origin, a shared context after its jumps,
 * proof c's image of HSW_GADGET_CONTEXT_IMAGES or a Context group, a pitch binding (hsw_gadget_bind_region), the
 * caller's own column pointer (hsw_gadget_bind_columns / hsw_gadget_bind_column_tables) + row * 32.
 * HSW_ERR_INVALID_ARG: a cell out of range or of a digest not yet assigned in this pass. */
int hsw_gadget_cell_address(const hsw_gadget *g, uint64_t cell, void **d_cell);
/* On-device check of the recorded ties (hsw_gadget_verify_ties) or of the caller's own constrain_equal pairs between
 * any two assigned gate-stream cells (hsw_gadget_verify_equal: cells_a[i] against cells_b[i]), cell against cell in
 * every layout and binding: the two cells of a pair are compared as stored -- 32 bytes, canonical or Montgomery, like
 * the verifier's copies.  This is what hsw_gadget_verify does NOT see: it checks each digest against its own staging
 * arrays, so a parent that hashed stale bytes (a slot no message writes, a nodes buffer overlapping something else,
 * bytes changed between two calls of a pass) passes it and fails here.  checks = pairs compared; first = index of
 * the lowest failing tie / pair.  n == 0 (no ties): no launch, checks = 0.  An invalid cell anywhere:
 * HSW_ERR_INVALID_ARG before anything is launched.  Synchronous on the engine's stream. */
int hsw_gadget_verify_ties(hsw_gadget *g, hsw_tie_report *report);
int hsw_gadget_verify_equal(hsw_gadget *g, const uint64_t *cells_a, const uint64_t *cells_b, size_t n, hsw_tie_report *report);
/* ---- lookup-table multiplicities of a pass, counted on the device ----
 * The gadget's two lookup arguments, and what a prover needs first for either (halo2's permuted A'/S' pair or a logUp
 * sum): how often each table row is used by each proof.
 *   HSW_LOOKUP_RANGE   every entry the gadget queues into the lookup-advice column is a value below 2^16 (range_check
 *                      limbs, bytes, byte * 2^8): a row of the 2^16-row range table;
 *   HSW_LOOKUP_SPREAD  every (dense, spread) pair of the chip columns is row `dense` of the 2^num_bits_lookup-row
 *                      spread table (hsw_spread_table); the lookup has no selector: every row of every chip column.
 * hsw_gadget_lookup_runs LISTS the entries as runs of device cells (host only, no launch), exactly what the digests
 * committed so far in this pass have written, in (context, table, column, first) order:
 *   RANGE   one run per committed digest (its prologue, block and epilogue lookups are contiguous), neighbours merged
 *           where nothing of the caller's lies between them.  Never in a run: the caller's entries below
 *           lookups_queued / origin_lookups, the interlude entries of a shared context or Context group, anything of
 *           a proof that has not been digested.  A gadget without a lookup column (no HSW_GADGET_WHOLE_DIGEST) lists none;
 *   SPREAD  one run per (Context, chip column): column k holds the committed limb calls n = k (mod num_advice_columns),
 *           so with 3 columns the runs of one Context differ in length.
 * Addresses are those of the layout and binding in force (linear streams, column images, shared contexts, context
 * images, Context groups, hsw_gadget_bind_region pitches, hsw_gadget_bind_column_tables pointers).  *n (may be NULL)
 * is always set; out = NULL only queries; cap < *n: HSW_ERR_TOO_LARGE, nothing written.  hsw_gadget_reset empties it.
 * hsw_gadget_lookup_multiplicities COUNTS them (hsw_lookup_counts_kernel) into the caller's tables:
 *   d_range[c * range_pitch + t]   = listed RANGE entries of proof c whose value is t;
 *   d_spread[c * spread_pitch + t] = listed chip rows of proof c with dense == t and spread == spread(t);
 * with HSW_LOOKUP_ACCUMULATE the counters grow by that, else the tables of the Contexts that have at least one run
 * are zeroed first (2^16 / 2^num_bits_lookup counters each, not `pitch`) and no other counter is touched.  An entry is
 * in its table only if the WHOLE 32-byte cell (reduced from Montgomery form where the cells are HSW_REPR_MONTGOMERY)
 * equals a table row: a cell whose low limb fits and whose upper limbs are not zero is counted in not_in_table and in
 * no counter, and so is a Montgomery cell (dense or spread) whose stored limbs are >= p -- an encoding m + p reduces
 * to the value of m, but a cell is an encoding below p and nothing else is a row.  So per proof sum(counts) + its share of not_in_table = its listed entries.  The counters are the only
 * caller memory written.  Unassigned rows are the caller's: halo2 looks (0, 0) up there, so a prover adds
 * usable_rows - entries to row 0 of each table.  Synchronous on the engine's stream; an empty list is HSW_OK, a zero
 * report and no launch.  HSW_ERR_INVALID_ARG before any launch: both table pointers NULL, a pitch below the table
 * size, a counter pointer not 4-byte aligned.  HSW_ERR_UNSUPPORTED: d_range on a gadget without a lookup column,
 * HSW_REPR_COMPACT64 cells, a pass whose batches differ in representation.
 * (Both calls came under HSW_ABI_MINOR 1: probe for the symbol.) */
#define HSW_LOOKUP_RANGE 0u
#define HSW_LOOKUP_SPREAD 1u
#define HSW_LOOKUP_ACCUMULATE 1u      /* add to what the tables hold instead of zeroing the proofs' tables first */
typedef struct hsw_lookup_run {
    uint64_t context;      /* proof (Context) index; 0 for a single-Context gadget */
    uint32_t table;        /* HSW_LOOKUP_RANGE = 0 (lookup-advice column, 2^16 rows) | HSW_LOOKUP_SPREAD = 1 */
    uint32_t column;       /* chip column k for SPREAD, 0 for RANGE */
    uint64_t first;        /* RANGE: entry index in the proof's lookup column; SPREAD: the column's first row of this run */
    uint64_t n;            /* entries (cells of d_cells; for SPREAD also of d_spread) */
    void *d_cells;         /* device address of the first cell (RANGE: the entry; SPREAD: the dense cell) */
    void *d_spread;        /* SPREAD: the spread cell of the same row; NULL for RANGE */
} hsw_lookup_run;
int hsw_gadget_lookup_runs(const hsw_gadget *g, hsw_lookup_run *out, size_t cap, size_t *n);
typedef struct hsw_lookup_counts {
    uint32_t *d_range;     /* contexts x range_pitch u32, proof-major; counter t of proof c at c*range_pitch + t; NULL = skip */
    uint32_t *d_spread;    /* contexts x spread_pitch u32; NULL = skip */
    uint64_t range_pitch;  /* >= 65536;              0 = 65536 */
    uint64_t spread_pitch; /* >= 2^num_bits_lookup;  0 = 2^num_bits_lookup */
    uint32_t flags, reserved_;
} hsw_lookup_counts;
typedef struct hsw_lookup_report {
    uint64_t range_entries, spread_entries;   /* entries looked at, per table */
    uint64_t not_in_table;                    /* entries that are no row of their table; they are counted nowhere else */
    uint64_t first_context, first_entry;      /* the lowest failing entry in (context, table, column, entry) order */
    uint32_t first_table, first_column;
    float kernel_ms; uint32_t reserved_;
} hsw_lookup_report;
int hsw_gadget_lookup_multiplicities(hsw_gadget *g, const hsw_lookup_counts *out, hsw_lookup_report *report);
/* ---- halo2's permuted lookup columns A' and S', written on the device ----
 * An ARGUMENT is one lookup of one proof (Context):
 *   HSW_LOOKUP_RANGE   one per proof, a = c; T = 65536 table rows; the value of row t is val(t) = t;
 *   HSW_LOOKUP_SPREAD  one per proof and chip column (the reference configures one lookup per (dense_k, spread_k) pair),
 *                      a = c * num_advice_columns + k; T = 2^num_bits_lookup rows; val(t) = t * theta_c + spread(t) mod p,
 *                      halo2's fold acc * theta + expr over [dense, spread] (DESIGN.md assumption A6) -- with
 *                      HSW_PERMUTED_THETA_ON_SPREAD val(t) = t + spread(t) * theta_c.  thetas: HOST memory, contexts x 32
 *                      bytes in the representation of the cells, the stored limbs below p (NULL for RANGE).
 * d_input_columns / d_table_columns: HOST arrays (copied, not kept) of n_arguments DEVICE pointers, the A' and the S'
 * column of argument a: usable_rows cells of 32 bytes each, 16-byte aligned, in any address order.  n_arguments must
 * be contexts (RANGE) or contexts x num_advice_columns (SPREAD).  Cells are written in the representation of the pass (a
 * Montgomery cell is val * 2^256 mod p, below p).
 * With m[t] the argument's multiplicities, E = sum m and u = usable_rows: unassigned rows look row 0 up, m'[0] = m[0] +
 * (u - E), m'[t] = m[t] otherwise; off[t] is the exclusive prefix sum of m'.  Then, so that the output is fixed bit for bit:
 *   A'[i]      = val(t)  for off[t] <= i < off[t] + m'[t];
 *   S'[off[t]] = val(t)  for every t with m'[t] > 0;
 *   the remaining positions of S', ascending, take the leftover table rows in ascending row order: row 0 (u - T) +
 *   [m'[0] = 0] times (the table column's padding rows repeat row 0), every t > 0 [m'[t] = 0] times.
 * So A'[0] = S'[0] and A'[i] = S'[i] or A'[i] = A'[i-1] for i > 0, A' is a permutation of the padded input and S' of
 * the padded table.  Rows at or beyond u of either column, and every other byte of the caller's, are never written:
 * blinding rows are the prover's.  The order inside A' (by table row) is the library's; halo2's own is not pinned.
 * Where m comes from:
 *   counted (default)     from the argument's own runs as hsw_gadget_lookup_runs lists them (RANGE: the runs of the proof;
 *                         SPREAD: the run of chip column k alone), membership decided as hsw_gadget_lookup_multiplicities
 *                         decides it.  d_m (may be NULL) is an OUTPUT: the counted m, before the padding of row 0;
 *   HSW_PERMUTED_GIVEN_M  d_m is an INPUT (required): the caller's counters, e.g. of a prover with lookup entries of its own.
 * d_m: DEVICE memory, per-argument u32 tables [a * m_pitch + t], 4-byte aligned; m_pitch >= T, 0 = T.
 * Decided on the device, all or nothing: an entry that is no table row (counted) or sum m > usable_rows (given) sets a
 * flag in the first stage, and with the flag set the write stage stores nothing to any column: the status is HSW_OK,
 * report->written = 0, and not_in_table / first_* (as in hsw_lookup_report) / overflow_arguments say why.  The host reads
 * nothing between the stages.  An empty run list in counted mode is valid: every row is unassigned, A' is u x val(0) and
 * S' the table with its padding (row 0 and its u - T copies first, as the leftover rule orders them, then rows 1 .. T-1).  Synchronous on the engine's stream.
 * Refused before any launch -- HSW_ERR_INVALID_ARG: usable_rows < T, in counted mode an argument with more listed
 * entries than usable_rows (hsw_last_error names it), a NULL or misaligned column pointer, a wrong n_arguments, unknown
 * flags or table, d_m missing in given mode or misaligned, m_pitch below T, thetas missing for SPREAD or a theta >= p;
 * HSW_ERR_TOO_LARGE: usable_rows above 2^31, or d_m NULL and 4 T bytes x n_arguments above half of "permuted_scratch"
 * (pass d_m or raise the option); HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64 cells, a pass whose batches differ
 * in representation, RANGE on a gadget without a lookup column.
 * Scratch (index arrays of 12 T bytes per argument, value tables of 32 T bytes per proof, and 4 T bytes per argument for
 * m where d_m is NULL) is the gadget's: grown on demand, freed by hsw_gadget_destroy.  It is bounded by the engine option
 * "permuted_scratch": m of ALL arguments (it cannot be grouped: the flag must be known for every argument before the
 * first store) may take half of it at the most, and the arguments are processed in groups whose index and value arrays fit
 * the rest -- a group being at least one proof, so the bound is max(permuted_scratch, m + one proof's arrays) plus the
 * run table.
 * kernel_ms: the whole call on the device; prepare_ms (count, index arrays, value tables) + write_ms (the stores) = kernel_ms.
 * (The call came under HSW_ABI_MINOR 1: probe for the symbol.) */
#define HSW_PERMUTED_GIVEN_M 1u
#define HSW_PERMUTED_THETA_ON_SPREAD 2u
typedef struct hsw_lookup_permuted {
    uint32_t table;                  /* HSW_LOOKUP_RANGE | HSW_LOOKUP_SPREAD */
    uint32_t flags;
    uint64_t usable_rows;            /* u: T <= u <= 2^31 */
    size_t n_arguments;
    void *const *d_input_columns;    /* host array of n_arguments device pointers: A' */
    void *const *d_table_columns;    /* host array of n_arguments device pointers: S' */
    const void *thetas;              /* host, contexts x 32 bytes; SPREAD only */
    uint32_t *d_m;                   /* device, n_arguments x m_pitch u32; counted: output or NULL; given: input */
    uint64_t m_pitch;                /* >= T; 0 = T */
} hsw_lookup_permuted;
typedef struct hsw_permuted_report {
    uint64_t arguments;                       /* arguments processed */
    uint64_t entries;                         /* counted mode: lookup entries looked at */
    uint64_t written;                         /* cells written: 2 * usable_rows * arguments, or 0 */
    uint64_t not_in_table;                    /* counted mode: entries that are no row of their table */
    uint64_t first_context, first_entry;      /* the lowest of them in (context, table, column, entry) order */
    uint32_t first_table, first_column;
    uint64_t overflow_arguments;              /* given mode: arguments with sum m > usable_rows */
    float kernel_ms, prepare_ms, write_ms; uint32_t reserved_;
} hsw_permuted_report;
int hsw_gadget_lookup_permuted(hsw_gadget *g, const hsw_lookup_permuted *args, hsw_permuted_report *report);
/* ---- the lookup argument's grand-product column Z, written on the device ----
 * The third column of halo2's lookup argument, committed right after the permuted pair.  Per argument a (numbered as in
 * hsw_lookup_permuted) of proof c, over the usable rows, every value mod p:
 *   Z[0] = 1,   Z[i+1] = Z[i] * (A[i] + beta_c)(S[i] + gamma_c) / ((A'[i] + beta_c)(S'[i] + gamma_c)),   0 <= i < u
 *   A[i]   the unpermuted compressed input, READ from the caller's physical column(s): RANGE the cell of d_inputs[a];
 *          SPREAD d_inputs[a][i] * theta_c + d_inputs_spread[a][i], with HSW_PERMUTED_THETA_ON_SPREAD d_inputs[a][i] +
 *          d_inputs_spread[a][i] * theta_c (DESIGN.md assumption A6).  Rows i >= input_rows[a] are not read and count
 *          as 0: unassigned;
 *   S[i]   the unpermuted table column, NOT read: val(i) for i < T and val(0) for T <= i < u, val as in
 *          hsw_gadget_lookup_permuted (the table column's padding rows repeat row 0);
 *   A', S' d_permuted_inputs[a] / d_permuted_tables[a]: what hsw_gadget_lookup_permuted wrote, or any the caller has.
 * d_products[a] receives Z[0 .. u], u + 1 cells in the representation of the pass.  Z is one field element per row, so the
 * output is fixed bit for bit.  All pointer arrays are HOST arrays (copied, not kept) of n_arguments DEVICE pointers to
 * 32-byte cells, 16-byte aligned, in any address order; thetas (SPREAD only), betas, gammas: HOST memory, contexts x 32
 * bytes as stored (Montgomery cells: the challenge * 2^256 mod p), the stored limbs below p.
 * Decided on the device, per ARGUMENT (status[a], a host array of n_arguments words, may be NULL):
 *   HSW_PRODUCT_ZERO_DENOM        some (A'[i] + beta)(S'[i] + gamma) is 0;
 *   HSW_PRODUCT_CELL_NOT_BELOW_P  a stored cell that was read (input, A', S') is not an encoding below p;
 *                                 either one REFUSES the argument: none of its u + 1 cells is written;
 *   HSW_PRODUCT_OPEN              Z[u] != 1: the argument is written, its Z is what the recurrence gives.
 * The other arguments are written; the call returns HSW_OK in all these cases and the report counts them (first_open /
 * first_refused: the lowest such argument, ~0 where there is none; written: (u + 1) x the arguments not refused).  Every
 * row of every column is either fully written or untouched; nothing at or beyond row u + 1, no input cell and no other
 * byte of the caller's is ever written.  Blinding rows are the prover's; the commitment is hsw_gadget_msm.
 * Refused before any launch -- HSW_ERR_INVALID_ARG: usable_rows < T, a wrong n_arguments, unknown flags or table, a
 * pointer (array or column) that is NULL or not 16-byte aligned, input_rows[a] > usable_rows, a challenge that is missing
 * or not below p, a Z column that overlaps a column read or another Z column (byte intervals; hsw_last_error names the
 * argument); HSW_ERR_TOO_LARGE: usable_rows above 2^31, or more than 2^31 - 1 tiles in all; HSW_ERR_UNSUPPORTED:
 * HSW_REPR_COMPACT64 cells, a pass whose batches differ in representation.
 * Three launches on the engine's stream, the host reads nothing in between: tiles (products of tile_rows rows each, 64
 * bytes of scratch per tile), scan (per argument: prefix and suffix over the tiles, ONE inversion), write.  The scratch is
 * the gadget's: grown on demand, freed by hsw_gadget_destroy.  kernel_ms = tiles_ms + scan_ms + write_ms.  Synchronous.
 * (The call came under HSW_ABI_MINOR 1: probe for the symbol.) */
#define HSW_PRODUCT_OPEN          1u   /* Z[u] != 1 */
#define HSW_PRODUCT_ZERO_DENOM    2u   /* some (A'[i]+beta)(S'[i]+gamma) == 0 */
#define HSW_PRODUCT_CELL_NOT_BELOW_P 4u/* a stored cell that was read is not an encoding below p */
typedef struct hsw_lookup_product {
    uint32_t table, flags;                 /* HSW_LOOKUP_RANGE | HSW_LOOKUP_SPREAD; HSW_PERMUTED_THETA_ON_SPREAD */
    uint64_t usable_rows;                  /* u: T <= u <= 2^31 */
    size_t n_arguments;                    /* contexts (RANGE) or contexts x num_advice_columns (SPREAD), a as in hsw_lookup_permuted */
    const void *const *d_inputs;           /* host array of device pointers: RANGE the lookup-advice column, SPREAD the dense column */
    const void *const *d_inputs_spread;    /* SPREAD: the spread column; NULL for RANGE */
    const uint64_t *input_rows;            /* host, per argument, <= u; NULL = u everywhere */
    const void *const *d_permuted_inputs;  /* A', u cells */
    const void *const *d_permuted_tables;  /* S', u cells */
    void *const *d_products;               /* Z, u + 1 cells each */
    const void *thetas, *betas, *gammas;   /* host, contexts x 32 bytes as stored, below p; thetas as in hsw_lookup_permuted */
    uint32_t *status;                      /* host, n_arguments, output; may be NULL */
} hsw_lookup_product;
typedef struct hsw_product_report {
    uint64_t arguments, written;           /* written: (u + 1) x arguments actually stored */
    uint64_t open_arguments, first_open;
    uint64_t refused_arguments, first_refused;   /* ZERO_DENOM or CELL_NOT_BELOW_P */
    uint32_t tile_rows, reserved_;
    float kernel_ms, tiles_ms, scan_ms, write_ms;
} hsw_product_report;
int hsw_gadget_lookup_product(hsw_gadget *g, const hsw_lookup_product *args, hsw_product_report *report);
/* ---- the permutation argument's grand products Z, written on the device ----
 * What halo2 commits after the lookup permuted pairs and before the lookup Z (permutation::prover): the columns that
 * enforce the copy constraints, those hsw_gadget_ties lists among them.  The permutation has m = n_columns columns in its
 * own order, in S = ceil(m / L) chunks of L = chunk_columns (halo2's cs_degree - 2; the last chunk may be shorter).  For
 * proof c of contexts, over the u = usable_rows rows, every value mod p, chunk s holding the columns j with
 * s L <= j < min(m, (s + 1) L):
 *   num_s[i] = prod_j (v_{c,j}[i] + beta_c * delta^j * omega^i + gamma_c)
 *   den_s[i] = prod_j (v_{c,j}[i] + beta_c * sigma_j[i]         + gamma_c)
 *   Z_{c,0}[0] = 1,   Z_{c,s}[0] = Z_{c,s-1}[u]  (s > 0),   Z_{c,s}[i+1] = Z_{c,s}[i] * num_s[i] / den_s[i],   0 <= i < u
 *   v_{c,j}  the caller's physical column d_columns[c*m + j], 32-byte cells in the representation of the pass.  Rows
 *            i >= column_rows[c*m + j] are not read and count as 0 (a gadget's image columns are shorter than u);
 *   sigma_j  the key's permutation column d_sigmas[j], u cells in the representation of the pass, all read, SHARED by
 *            the proofs (K proofs of one circuit have one proving key).  Building it from copy constraints is keygen
 *            and stays the caller's;
 *   omega, delta  the caller's: the library does not check that omega is a root of unity and pins no constant of halo2's.
 * d_products[c*S + s] receives Z_{c,s}[0 .. u], u + 1 cells in the representation of the pass.  Z is one field element
 * per cell, so the output is fixed bit for bit.  All pointer arrays are HOST arrays (copied, not kept) of DEVICE pointers,
 * 16-byte aligned, in any address order; betas, gammas: HOST memory, contexts x 32 bytes as stored (Montgomery cells: the
 * challenge * 2^256 mod p); omega, delta: HOST memory, 32 bytes each as stored; all stored limbs below p.
 * Decided on the device, per PROOF, because the chunks of a proof chain (status[c], a host array of contexts words, may
 * be NULL), with the bits of hsw_gadget_lookup_product:
 *   HSW_PRODUCT_ZERO_DENOM        some den_s[i] is 0;
 *   HSW_PRODUCT_CELL_NOT_BELOW_P  a stored cell that was read (value or sigma) is not an encoding below p;
 *                                 either one REFUSES the proof: none of its S columns is written;
 *   HSW_PRODUCT_OPEN              Z_{c,S-1}[u] != 1: the proof is written, its Z is what the recurrence gives.
 * The other proofs are written; the call returns HSW_OK in all these cases and the report counts them (first_open /
 * first_refused: the lowest such proof, ~0 where there is none).  Every row of every Z column is either fully written or
 * untouched; nothing at or beyond row u + 1, no input cell and no other byte of the caller's is ever written.  Blinding
 * rows are the prover's; the commitment is hsw_gadget_msm.
 * Refused before any launch -- HSW_ERR_INVALID_ARG: usable_rows, n_columns or chunk_columns 0, unknown flags, a pointer
 * (array or column) that is NULL or not 16-byte aligned, column_rows[k] > usable_rows, a challenge, omega or delta that is
 * missing or not below p, a Z column that overlaps a column read or another Z column (byte intervals; hsw_last_error
 * names the proof); HSW_ERR_TOO_LARGE: usable_rows above 2^31, or more than 2^31 - 1 tiles (or columns) in all;
 * HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64 cells, a pass whose batches differ in representation.
 * Three launches on the engine's stream, the host reads nothing in between: tiles (per proof, chunk and tile_rows rows:
 * two products, 64 bytes of scratch), scan (per proof over the tiles of all its chunks, ONE inversion), write.  The
 * scratch is the gadget's: grown on demand, freed by hsw_gadget_destroy.  kernel_ms = tiles_ms + scan_ms + write_ms.
 * Synchronous.  (The call came under HSW_ABI_MINOR 1: probe for the symbol.) */
typedef struct hsw_permutation_product {
    uint32_t flags, chunk_columns;         /* flags: 0; chunk_columns: cs_degree - 2, >= 1 */
    uint64_t usable_rows;                  /* u: 1 <= u <= 2^31 */
    size_t n_columns;                      /* m, per proof, in the permutation's column order */
    const void *const *d_columns;          /* host array, contexts x m device pointers, [c*m + j] */
    const uint64_t *column_rows;           /* host, contexts x m, <= u; NULL = u everywhere */
    const void *const *d_sigmas;           /* host array, m device pointers, u cells each, shared by the proofs */
    void *const *d_products;               /* host array, contexts x S device pointers, [c*S + s], u + 1 cells each */
    const void *betas, *gammas;            /* host, contexts x 32 bytes as stored, below p */
    const void *omega, *delta;             /* host, 32 bytes each as stored, below p */
    uint32_t *status;                      /* host, contexts words, output; may be NULL */
} hsw_permutation_product;
typedef struct hsw_permutation_report {
    uint64_t proofs, products, written;    /* products = contexts x S; written = (u + 1) x S x proofs not refused */
    uint64_t open_proofs, first_open, refused_proofs, first_refused;   /* first_*: ~0 where there is none */
    uint32_t tile_rows, reserved_;
    float kernel_ms, tiles_ms, scan_ms, write_ms;
} hsw_permutation_report;
int hsw_gadget_permutation_product(hsw_gadget *g, const hsw_permutation_product *args, hsw_permutation_report *report);
/* ---- the Fr NTT of device columns: Lagrange, coefficient and coset form ----
 * What halo2 does next with every column above: lagrange_to_coeff, coeff_to_extended, extended_to_coeff.  For column b,
 * with a[j] the field element stored in cell j of d_inputs[b] for j < input_rows[b] and 0 from there on, every value mod
 * p, N = 2^log_n, natural order in and out:
 *   flags = 0:                    out[i] = c * sum_{j<N} a[j] * g^j * w^(i j)      0 <= i < N
 *   flags = HSW_NTT_SHIFT_AFTER:  out[i] = c * g^i * sum_{j<N} a[j] * w^(i j)
 * w = omega, g = shift (NULL: 1) and c = scale (NULL: 1) are the caller's: HOST memory, 32 bytes each as stored in the
 * representation of the pass, below p.  The library pins no constant of halo2's; it does check that w^(N/2) = p - 1, so
 * that w is a primitive N-th root of unity.  The three calls of halo2:
 *   lagrange_to_coeff   w = omega^-1,      c = n^-1, flags 0
 *   coeff_to_extended   w = omega_ext,     g = zeta, flags 0, input_rows = n, log_n = k + e
 *   extended_to_coeff   w = omega_ext^-1,  c = N^-1, g = zeta^-1, HSW_NTT_SHIFT_AFTER (the caller ignores the rows it truncates)
 * Cells are 32 bytes in the representation of the pass; the transform is linear and every constant is held in Montgomery
 * form, so canonical and Montgomery cells take the same kernel and the output is exact bit for bit in both.
 * d_inputs, d_outputs: HOST arrays (copied, not kept) of DEVICE pointers, 16-byte aligned, in any address order;
 * d_outputs[b] receives N cells.  Rows of an input at and beyond input_rows[b] are NOT READ.  d_outputs[b] ==
 * d_inputs[b] (in place) is allowed, and several columns may read one input; any other overlap of an output with an
 * input or with another output is refused.
 * Decided on the device, per column (status[b], a host array of n_columns words, may be NULL):
 *   HSW_NTT_CELL_NOT_BELOW_P  a stored cell that was read is not an encoding below p: the column is REFUSED, not one
 *                             byte of its output is written.
 * The other columns are written; the call returns HSW_OK and the report counts them (first_refused: the lowest such
 * column, ~0 where there is none).  input_rows[b] = 0 is legal: N zero cells, nothing of the input is read.  Nothing
 * outside rows [0, N) of the outputs of the columns not refused is ever written.
 * Refused before any launch -- HSW_ERR_INVALID_ARG: n_columns 0, log_n 0 or above 28, pass_log above 10, unknown flags, a
 * pointer (array or column) that is NULL or not 16-byte aligned, input_rows[b] > N, omega missing, not below p or not
 * primitive of order N, shift or scale not below p, an overlap as above (hsw_last_error names the column);
 * HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64 cells, a pass whose batches differ in representation.
 * The bits of the index go in digits, a launch per digit: one launch up to log_n = pass_log (0: 10, the points a
 * workgroup holds), else digits of at most max(1, pass_log - 2) bits, because a launch that reads or writes at a stride
 * keeps runs of four cells -- 2 launches up to log_n 16, 3 up to 24, 4 up to 28 by default.  Only a column's last launch
 * writes d_outputs[b]; before it the points live in the gadget's scratch (N cells per column; columns go in groups that
 * hold at most 1 GiB of it -- or what the engine option "round_scratch" lowers that to --, a group being at least one
 * column), grown on demand and freed by hsw_gadget_destroy.  The
 * table of the N / 2 powers of w is built on the device from O(log N) staged powers and cached by (w as a value,
 * log_n): four tables, the least recently used one evicted, all freed by hsw_gadget_destroy.  The host reads nothing
 * between launches.  Synchronous.  (The call came under HSW_ABI_MINOR 1: probe for the symbol.) */
#define HSW_NTT_SHIFT_AFTER 1u
#define HSW_NTT_CELL_NOT_BELOW_P 4u    /* status bit, the value of HSW_PRODUCT_CELL_NOT_BELOW_P */
typedef struct hsw_ntt {
    uint32_t flags, log_n;                 /* flags: 0 or HSW_NTT_SHIFT_AFTER; 1 <= log_n <= 28 */
    uint32_t pass_log, reserved_;          /* 0: the library's choice (10); else no launch transforms more than 2^pass_log points at a time, 1 .. 10 */
    size_t n_columns;
    const void *const *d_inputs;           /* host array, n_columns device pointers */
    const uint64_t *input_rows;            /* host, per column, 0 .. N; NULL = N everywhere */
    void *const *d_outputs;                /* host array, n_columns device pointers, N cells each */
    const void *omega, *shift, *scale;     /* host, 32 bytes each as stored, below p; shift, scale may be NULL */
    uint32_t *status;                      /* host, n_columns words, output; may be NULL */
} hsw_ntt;
typedef struct hsw_ntt_report {
    uint64_t columns, written, refused_columns, first_refused;   /* written = N x columns not refused; first_refused: ~0 where there is none */
    uint64_t twiddle_bytes, scratch_bytes; /* the table of this call's root; the points' scratch of a group */
    uint32_t launches, pass_log;           /* launches per column group; the pass_log used */
    float kernel_ms, twiddle_ms;           /* twiddle_ms: 0 when the table was cached */
} hsw_ntt_report;
int hsw_gadget_ntt(hsw_gadget *g, const hsw_ntt *args, hsw_ntt_report *report);
/* ---- commit device columns: the BN254 G1 multi-scalar multiplication on the device ----
 * What halo2 does between any two of the calls above: commit_lagrange (advice, A', S', Z) and commit (the pieces of h).
 * For column b, with a[j] the field element stored in cell j of d_scalars[b] for j < input_rows[b] and 0 from there on
 * -- the cell in the representation of the pass, canonical or Montgomery; the kernel reduces both to the canonical
 * integer below r -- and G[j] the point stored at d_bases + 64 j:
 *   out_points[b] = sum_{j < input_rows[b]} a[j] * G[j]      in BN254 G1 (y^2 = x^3 + 3 over Fq, prime order r = the Fr modulus)
 * Bases: ONE device array of n_bases affine points, 16-byte aligned, 64 bytes each: x then y, eight 32-bit limbs each,
 * little-endian, in MONTGOMERY form mod q whatever the representation of the pass, (0, 0) for the identity -- assumed to
 * be the in-memory form of halo2curves' G1Affine (assumption A7).  The caller uploads params.g_lagrange /
 * params.g once and reuses them across calls.  A (0, 0) base contributes nothing.  The library does not check that a
 * base is on the curve (the setup is the caller's); it does check that both coordinates of every base in rows
 * [0, max_b input_rows[b]) are below q.
 * Scalars: d_scalars is a HOST array (copied, not kept) of DEVICE pointers, 16-byte aligned, 32-byte cells; input_rows a
 * host array, NULL = n_bases everywhere.  Rows of a column at and beyond input_rows[b] are NOT READ.  input_rows[b] = 0
 * is legal and gives the identity.  Several columns may share one input.
 * Output: out_points is a HOST array of n_columns x 64 bytes in the stored form of a base; the identity is 64 zero
 * bytes.  The bytes are a function of the group element alone, hence the same whatever the schedule.  Nothing in
 * device memory other than the gadget's own scratch is written.
 * Decided on the device, per column (status[b], a host array of n_columns words, may be NULL); the call returns HSW_OK
 * in all of these cases:
 *   HSW_MSM_CELL_NOT_BELOW_P  a stored cell that was read is not an encoding below r: the column is REFUSED, not one
 *                             byte of out_points[b] is written; the other columns are.
 *   HSW_MSM_BASE_NOT_BELOW_Q  some base in the checked rows has a coordinate not below q: every column carries the bit
 *                             and nothing is written.  The report carries bad_bases and first_bad_base (~0 where
 *                             none).  Bases beyond the checked rows are not read.
 * Refused before any launch -- HSW_ERR_INVALID_ARG (hsw_last_error names the column): n_columns 0, n_bases 0 or above
 * 2^28, a pointer (array, column, bases, out_points) that is NULL or not 16-byte aligned (out_points: NULL), input_rows[b]
 * > n_bases, unknown flags, a window_bits or slice_rows outside its range; HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64
 * cells, a pass whose batches differ in representation.
 * The method is Pippenger's with unsigned digits of window_bits bits: W = ceil(254 / window_bits) windows, the rows in
 * slices of slice_rows rows; one launch checks the bases, then per group of columns one launch fills the 2^window_bits - 1
 * buckets of every (slice, window, column) and one sums the slices and forms a point per (window, column).  The host
 * copies W x 96 bytes per column, runs the Horner over the windows and the one inversion, and writes out_points.  Two
 * knobs exist so that small inputs reach every path: window_bits (0: the library's choice, 8; else 1 ..
 * HSW_MSM_MAX_WINDOW_BITS) and slice_rows (0: the library's choice, 4096, doubled until a column has at most 1024
 * slices; else a power of two from 64 to 2^28), the rows one workgroup accumulates; the report says what was used.
 * The partial buckets live in the gadget's scratch (columns go in groups that hold at most 1 GiB of them -- or what the
 * engine option "round_scratch" lowers that to --, a group being at least one column), grown on demand and
 * freed by hsw_gadget_destroy; nothing is allocated between the launches of a group.  The blinding term blind * W is a one-point addition and stays the prover's, as does the transcript.
 * Synchronous, on the engine's stream.  (The call came under HSW_ABI_MINOR 1: probe for the symbol.) */
#define HSW_MSM_CELL_NOT_BELOW_P 4u    /* status bit, the value of HSW_NTT_CELL_NOT_BELOW_P */
#define HSW_MSM_BASE_NOT_BELOW_Q 8u    /* status bit */
#define HSW_MSM_MAX_WINDOW_BITS 8u
typedef struct hsw_msm {
    uint32_t flags, window_bits;           /* flags: 0; window_bits: 0 or 1 .. HSW_MSM_MAX_WINDOW_BITS */
    uint32_t slice_rows, reserved_;        /* 0 or a power of two, 64 .. 2^28 */
    size_t n_columns;
    uint64_t n_bases;                      /* 1 .. 2^28 */
    const void *d_bases;                   /* device, n_bases x 64 bytes */
    const void *const *d_scalars;          /* host array, n_columns device pointers */
    const uint64_t *input_rows;            /* host, per column, 0 .. n_bases; NULL = n_bases everywhere */
    void *out_points;                      /* host, n_columns x 64 bytes, output */
    uint32_t *status;                      /* host, n_columns words, output; may be NULL */
} hsw_msm;
typedef struct hsw_msm_report {
    uint64_t columns, refused_columns, first_refused;   /* refused: either bit; first_refused: ~0 where there is none */
    uint64_t bad_bases, first_bad_base;    /* bases of the checked rows not below q; first_bad_base: ~0 where there is none */
    uint64_t scratch_bytes;                /* the partial buckets of a group */
    uint32_t window_bits, windows, slice_rows, slices;   /* what was used; slices: of the tallest column */
    uint32_t launches, reserved_;          /* the check (none when no row is read), and two per group of columns */
    float kernel_ms, finish_ms;            /* device: the launches; host: the Horner and the inversion of every column */
} hsw_msm_report;
int hsw_gadget_msm(hsw_gadget *g, const hsw_msm *args, hsw_msm_report *report);
/* ---- evaluate device columns at points, and open them: the quotients of the GWC multi-opening ----
 * What halo2 does after the last commitment with every polynomial in coefficient form (hsw_gadget_ntt's
 * lagrange_to_coeff leaves it on the device): eval_polynomial(p, x * omega^rot) for every query, and per distinct
 * opening point z of ProverGWC the fold of that point's polynomials with v, kate_division by (X - z), and the commitment
 * of the quotient (hsw_gadget_msm with n_bases = rows commits d_quotients[g] as it lies).  Every value mod p; column b
 * holds a_b[j] in cell j for j < input_rows[b] and 0 from there to `rows`; rows is 1 .. 2^28 and need not be a power of
 * two.
 *   hsw_gadget_evaluate, query i = (b, t) = (query_column[i], query_point[i]):
 *       out_evals[i] = sum_{j<rows} a_b[j] * z_t^j
 *   hsw_gadget_open, group g with columns b_0 .. b_{m-1} = group_columns[group_first[g] .. group_first[g+1]) in the
 *   caller's order, point z = points[g] and challenge v = challenges[g]:
 *       c[j] = sum_{i<m} v^(m-1-i) * a_{b_i}[j]         the fold acc * v + a: the FIRST column gets the highest power
 *       q[j] = sum_{j<i<rows} c[i] * z^(i-j-1)           0 <= j < rows, hence q[rows-1] = 0
 *       out_evals[g] = c(z) = c[0] + z * q[0]
 *   so that c(X) - c(z) = (X - z) * q(X).  Subtracting the evaluation from c changes c[0] alone, which q never reads:
 *   the quotient needs no evaluation first.
 * d_columns: a HOST array (copied, not kept) of DEVICE pointers, 16-byte aligned, 32-byte cells; input_rows a host
 * array, NULL = rows everywhere; input_rows[b] = 0 is legal.  Rows of a column at and beyond input_rows[b] are NOT
 * READ.  points, challenges: HOST memory, 32 bytes each as stored in the representation of the pass, below p.  A column
 * may sit in several groups and in several queries; duplicate queries are allowed; evaluate reads a column once for all
 * its points.  d_quotients: a host array of n_groups device pointers; d_quotients[g] receives exactly `rows` cells, the
 * last one zero.  out_evals: HOST, n_queries (n_groups) x 32 bytes as stored; for hsw_gadget_open it may be NULL.
 * Nothing in device memory but the gadget's scratch and, for open, the quotients is written.
 * Cells are in the representation of the pass; every constant is held in Montgomery form, so canonical and Montgomery
 * cells take the same kernel and the outputs are exact bit for bit in both.
 * Decided on the device (status: a host array of n_columns words for evaluate, of n_groups words for open; may be NULL):
 *   HSW_OPEN_CELL_NOT_BELOW_P  a stored cell that was read is not an encoding below p: the column with every query of
 *                              it, or the group, is REFUSED -- not one byte of its quotient or of its out_evals entries
 *                              is written.
 * The others are written; the call returns HSW_OK and the report counts the refusals (first_refused: the lowest such
 * column or group, ~0 where there is none).
 * Refused before any launch -- HSW_ERR_INVALID_ARG (hsw_last_error names the culprit): rows 0 or above 2^28; zero
 * columns, points, queries or groups, an empty group; an index out of range; a pointer (array, column, quotient,
 * out_evals of evaluate) that is NULL or a device pointer not 16-byte aligned; input_rows[b] > rows; a point or
 * challenge not below p; unknown flags; a tile_rows outside its range; a quotient that overlaps the `rows` cells of any
 * column (read or not), or another quotient; HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64 cells, a pass whose batches differ in
 * representation.
 * Three launches: tiles (a workgroup per tile of tile_rows rows folds, checks, and sums its rows by Horner's rule),
 * scan (the suffix over the tiles' sums: every tile's carry-in, and c(z)), write (open only: q, one multiply per row).
 * Every thread owns HSW_OPEN_THREAD_ROWS consecutive rows.  tile_rows: 0, the library's choice (2048), or a power of two
 * from HSW_OPEN_MIN_TILE_ROWS to 2^20 -- it exists so that small inputs reach the multi-tile and chunked-scan paths; the
 * output bytes do not depend on it, the report says what was used.  The folded column (groups of two columns or more),
 * a cell per thread and a cell per tile live in the gadget's scratch: groups (columns of evaluate) go in batches that
 * hold at most 1 GiB of it (or what the engine option "round_scratch" lowers that to), a batch being at least one group
 * (one column with all its points), three (two) launches per batch; grown on demand and
 * freed by hsw_gadget_destroy.  The host reads nothing between the launches of a call.  SHPLONK's multi-point opening
 * is hsw_gadget_shplonk_quotient / _open and h(X) is hsw_gadget_quotient (both below); the transcript and the blinding
 * terms stay the prover's.  Synchronous, on the engine's stream.  (The calls came
 * under HSW_ABI_MINOR 1: probe for the symbols.) */
#define HSW_OPEN_CELL_NOT_BELOW_P 4u   /* status bit, the value of HSW_NTT_CELL_NOT_BELOW_P */
#define HSW_OPEN_MIN_TILE_ROWS 256u
#define HSW_OPEN_THREAD_ROWS 8u
typedef struct hsw_evaluate {
    uint32_t flags, tile_rows;             /* flags: 0; tile_rows: 0 or a power of two, HSW_OPEN_MIN_TILE_ROWS .. 2^20 */
    uint64_t rows;                         /* 1 .. 2^28 */
    size_t n_columns;
    const void *const *d_columns;          /* host array, n_columns device pointers */
    const uint64_t *input_rows;            /* host, per column, 0 .. rows; NULL = rows everywhere */
    size_t n_points;
    const void *points;                    /* host, n_points x 32 bytes as stored, below p */
    size_t n_queries;
    const uint32_t *query_column;          /* host, n_queries indices below n_columns */
    const uint32_t *query_point;           /* host, n_queries indices below n_points */
    void *out_evals;                       /* host, n_queries x 32 bytes, output */
    uint32_t *status;                      /* host, n_columns words, output; may be NULL */
} hsw_evaluate;
typedef struct hsw_evaluate_report {
    uint64_t columns, queries, refused_columns, refused_queries, first_refused;   /* first_refused: a column; ~0 where there is none */
    uint64_t scratch_bytes;                /* the tiles' sums of a batch of columns */
    uint32_t tile_rows, tiles, thread_rows, launches;   /* what was used; launches: two per batch */
    float kernel_ms;
    uint32_t reserved_;
} hsw_evaluate_report;
int hsw_gadget_evaluate(hsw_gadget *g, const hsw_evaluate *args, hsw_evaluate_report *report);
typedef struct hsw_open {
    uint32_t flags, tile_rows;             /* flags: 0; tile_rows: 0 or a power of two, HSW_OPEN_MIN_TILE_ROWS .. 2^20 */
    uint64_t rows;                         /* 1 .. 2^28 */
    size_t n_columns;
    const void *const *d_columns;          /* host array, n_columns device pointers */
    const uint64_t *input_rows;            /* host, per column, 0 .. rows; NULL = rows everywhere */
    size_t n_groups;
    const uint64_t *group_first;           /* host, n_groups + 1 offsets into group_columns, increasing */
    const uint32_t *group_columns;         /* host, group_first[n_groups] indices below n_columns */
    const void *points, *challenges;       /* host, n_groups x 32 bytes each as stored, below p */
    void *const *d_quotients;              /* host array, n_groups device pointers, rows cells each */
    void *out_evals;                       /* host, n_groups x 32 bytes, output; may be NULL */
    uint32_t *status;                      /* host, n_groups words, output; may be NULL */
} hsw_open;
typedef struct hsw_open_report {
    uint64_t groups, written, refused_groups, first_refused;   /* written = rows x groups not refused; first_refused: ~0 where there is none */
    uint64_t scratch_bytes;                /* of the largest batch of groups */
    uint32_t tile_rows, tiles, thread_rows, launches;   /* what was used; launches: three per batch */
    uint32_t batches, reserved_;
    float kernel_ms, reserved2_;
} hsw_open_report;
int hsw_gadget_open(hsw_gadget *g, const hsw_open *args, hsw_open_report *report);
/* ---- SHPLONK's multi-point opening of device columns: the two polynomials of ProverSHPLONK ----
 * What halo2's ProverSHPLONK does after the evaluations with every polynomial in coefficient form: h(X), the y-fold of
 * every rotation set divided by the set's vanishing polynomial and folded with v, and -- after the prover has committed
 * h and squeezed u -- the linearisation L(X) divided by (X - u).  Both outputs are committed with hsw_gadget_msm (n_bases
 * = rows) as they lie: two G1 points however many rotations the circuit queries.  Every value mod p; column b holds
 * a_b[j] in cell j for j < input_rows[b] and 0 from there to `rows`; rows is 1 .. 2^28 and need not be a power of two.
 * T = points[0 .. n_points), the super point set: distinct field elements.  Rotation set i lists its columns b_{i,0 ..
 * m_i-1} = set_columns[set_first[i] .. set_first[i+1]) and its points S_i = { points[k] : k in
 * set_points[set_point_first[i] .. set_point_first[i+1]) }, t_i = |S_i| of them, z_{i,0 .. t_i-1} in the listed order.
 *   hsw_gadget_shplonk_quotient (y, v; u and d_h NULL), d_out = h:
 *       c_i[j] = sum_{k<m_i} y^k * a_{b_{i,k}}[j]           the FIRST listed column gets y^0
 *       Q_i(X) = floor( c_i(X) / Z_i(X) ),  Z_i(X) = prod_{z in S_i} (X - z)
 *       h[j]   = sum_i v^i * Q_i[j]                          0 <= j < rows; the first set gets v^0
 *   hsw_gadget_shplonk_open (y, v, u, d_h = the h of the first call), d_out = w:
 *       zd_i = prod_{z in T \ S_i} (u - z),   zt = prod_{z in T} (u - z)
 *       L[j] = sum_i v^i * zd_i * c_i[j]  -  zt * h[j]
 *       w[j] = zd_0^-1 * sum_{j<l<rows} L[l] * u^(l-j-1)     hence w[rows-1] = 0
 * No evaluation is needed in either call.  floor(c_i / Z_i) is what halo2 gets by first subtracting the interpolant R_i
 * of c_i over S_i: c_i = Z_i Q_i + R_i with deg R_i < t_i, and R_i agrees with c_i on S_i.  In the second call the terms
 * r_i = R_i(u) change L[0] alone, which w never reads (as in hsw_gadget_open): (X - u) w(X) = (L(X) - L(u)) / zd_0.  The
 * division by Z_i is done by partial fractions, lambda_{i,k} = 1 / prod_{l != k} (z_{i,k} - z_{i,l}):
 *       Q_i[j] = sum_k lambda_{i,k} * q_{i,k}[j],   q_{i,k}[j] = sum_{l>j} c_i[l] * z_{i,k}^(l-j-1)
 * the suffix Horner sums of hsw_gadget_open per (set, point); the top min(t_i, rows) cells of Q_i come out exactly 0.
 * The power orders (y^k in listed order within a set, v^i over sets in listed order) and the normalisation by zd_0^-1
 * are assumption A10: written from memory of halo2_proofs' shplonk prover, not pinned against its
 * source.  A fork that orders differently lists its columns or its sets in its order.
 * d_columns, input_rows: as hsw_gadget_open takes them; rows of a column at and beyond input_rows[b] are NOT READ, and a
 * column that no set lists is not read at all.  points, y, v, u: HOST memory, 32 bytes each as stored in the
 * representation of the pass, below p.  d_h: device, `rows` cells, all read.  d_out: device, receives exactly `rows`
 * cells.  Nothing in device memory but the gadget's scratch and d_out is written.  Cells are in the representation of
 * the pass; every constant is held in Montgomery form, so canonical and Montgomery cells take the same kernels and the
 * output is exact bit for bit in both.
 * Decided on the device (status: ONE host word; may be NULL):
 *   HSW_SHPLONK_CELL_NOT_BELOW_P  a stored cell that was read -- of a listed column, or of d_h -- is not an encoding
 *                                 below p: the call is REFUSED, not one byte of d_out is written.
 * The call still returns HSW_OK, and the report says refused = 1.
 * Refused before any launch -- HSW_ERR_INVALID_ARG (hsw_last_error names the culprit): rows 0 or above 2^28; zero
 * columns, points or sets; a set with no column or no point, or with more than HSW_SHPLONK_MAX_SET_POINTS points; more
 * than 65,535 sets; an index out of range; a column listed twice, in one set or in two; a point index twice in a set; two
 * entries of `points` equal in value; a point of T that no set uses; a pointer that is NULL or a device pointer not
 * 16-byte aligned; input_rows[b] > rows; a point or challenge not below p; unknown flags; a tile_rows outside its range;
 * d_out overlapping the `rows` cells of any column (read or not) or of d_h; quotient: u or d_h not NULL; open: u or d_h
 * NULL, or zd_0 = 0 (u is a point of T outside S_0).  HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64 cells, a pass whose batches
 * differ in representation.
 * Three launches per call: tiles (a workgroup per (set, tile): the fold with one staged weight per column, the check,
 * and per point of the set Horner and the workgroup scan), scan (hsw_gadget_open's, a workgroup per (set, point)),
 * write (a workgroup per tile: per (set, point) the recurrence down a thread's rows, the sum with the weights W_{i,k} =
 * v^i lambda_{i,k}, ONE store per output cell).  The second call is the same three launches over one set that holds
 * every listed column and h, with the weights v^i zd_i y^k / zd_0 and -zt / zd_0, the one point u and W = 1.  tile_rows:
 * as hsw_gadget_open's.  The scratch -- the staged points, weights and descriptors, c_i for every set of two columns or
 * more (rows cells), ceil(rows / 8) + tiles cells per (set, point), one status word -- lives in the gadget, is grown on
 * demand and freed by hsw_gadget_destroy.  It is NOT cut into batches: the write launch needs every set's c_i at once
 * (HSW_ERR_NOMEM if the device cannot hold it); report.scratch_bytes says how much.  The host reads nothing between
 * the launches.  One call is one proof's opening: K proofs are K calls.  The transcript, the blinding terms and the
 * evaluations written to the transcript (hsw_gadget_evaluate) stay the prover's.  Synchronous, on the engine's stream.
 * (The calls came under HSW_ABI_MINOR 1: probe for the symbols.) */
#define HSW_SHPLONK_CELL_NOT_BELOW_P 4u   /* status bit, the value of HSW_NTT_CELL_NOT_BELOW_P */
#define HSW_SHPLONK_MAX_SET_POINTS 16u    /* points of one rotation set */
typedef struct hsw_shplonk {
    uint32_t flags, tile_rows;             /* flags: 0; tile_rows: 0 or a power of two, HSW_OPEN_MIN_TILE_ROWS .. 2^20 */
    uint64_t rows;                         /* 1 .. 2^28 */
    size_t n_columns;
    const void *const *d_columns;          /* host array, n_columns device pointers */
    const uint64_t *input_rows;            /* host, per column, 0 .. rows; NULL = rows everywhere */
    size_t n_points;
    const void *points;                    /* host, n_points x 32 bytes as stored, below p, distinct: T */
    size_t n_sets;                         /* 1 .. 65,535 */
    const uint64_t *set_first;             /* host, n_sets + 1 offsets into set_columns, increasing from 0 */
    const uint32_t *set_columns;           /* host, set_first[n_sets] indices below n_columns, each at most once */
    const uint64_t *set_point_first;       /* host, n_sets + 1 offsets into set_points, increasing from 0 */
    const uint32_t *set_points;            /* host, set_point_first[n_sets] indices below n_points */
    const void *y, *v, *u;                 /* host, 32 bytes each as stored, below p; u: open only, NULL for quotient */
    const void *d_h;                       /* device, rows cells: open only, NULL for quotient */
    void *d_out;                           /* device, rows cells: h (quotient) or w (open) */
    uint32_t *status;                      /* host, one word, output; may be NULL */
} hsw_shplonk;
typedef struct hsw_shplonk_report {
    uint64_t sets, items, columns;         /* items: the (set, point) pairs; columns: the listed ones (open: and h) */
    uint64_t written, refused;             /* written = rows, or 0 when refused (1) */
    uint64_t scratch_bytes;                /* all of it: one call is one batch */
    uint32_t tile_rows, tiles, thread_rows, launches;   /* what was used; launches: three */
    float kernel_ms;
    uint32_t reserved_;
} hsw_shplonk_report;
int hsw_gadget_shplonk_quotient(hsw_gadget *g, const hsw_shplonk *args, hsw_shplonk_report *report);
int hsw_gadget_shplonk_open(hsw_gadget *g, const hsw_shplonk *args, hsw_shplonk_report *report);
/* ---- the quotient h(X) of device columns on the extended coset ----
 * What halo2's evaluate_h and vanishing argument do between the last grand product and the commitments of h: the
 * numerator -- every gate, permutation and lookup expression folded with y -- divided by the vanishing polynomial, row
 * by row on the extended coset, for K independent proofs of one circuit.  Every column already lies in device memory
 * in extended form (hsw_gadget_ntt's coeff_to_extended leaves it there); the caller brings h back with
 * extended_to_coeff, cuts it into n-row pieces and commits them with hsw_gadget_msm.
 * n = 2^log_rows, N = 2^log_n, e = log_n - log_rows, w = omega_ext, X_i = zeta * w^i; every value mod p.  Rotation r of
 * a base-domain query reads extended row (i + r * 2^e) mod N; u = usable_rows, and the last rotation -(blinding + 1) is
 * the shift +u in base rows.  Per proof c with its own theta, beta, gamma, y: V starts at 0 and every expression below
 * folds as V = V * y + expr, in exactly this order (assumption A9, DESIGN.md 5.5e: a fork that orders the gates or the
 * lookups differently changes only the order of the lists the caller passes):
 *   1. gates, in the listed order: gate_g[i] = sum_t coeff_t * prod_f col_{t,f}[(i + rot_{t,f} * 2^e) mod N]; a monomial
 *      with no factor is the constant coeff.  Columns share one index space: 0 .. m-1 the proof's own d_columns[c*m + j],
 *      m .. m+F-1 the shared d_fixed[j - m].  (The FlexGate gate q (a + b c - d) is the three monomials +1 q a(0),
 *      +1 q b(1) c(2), (p - 1) q d(3).)
 *   2. permutation (n_perm_columns > 0), S = ceil(n_perm_columns / L) sets:
 *        l0 * (1 - Z_0);   l_last * (Z_{S-1}^2 - Z_{S-1});   s = 1 .. S-1: l0 * (Z_s - Z_{s-1}[(i + u * 2^e) mod N]);
 *        s = 0 .. S-1: l_active * (Z_s[(i + 2^e) mod N] * prod_j (v_j + beta * sigma_j + gamma)
 *                                  - Z_s * prod_j (v_j + beta * delta^j * X_i + gamma))
 *      j over the set's columns, the exponent of delta the column's position in the whole permutation.
 *   3. lookups, in the listed order; A the fold acc * theta + col over the input columns, Sv over the table columns
 *      (the first listed column gets the highest power):
 *        l0 * (1 - Z);   l_last * (Z^2 - Z);
 *        l_active * (Z[(i + 2^e) mod N] * (A' + beta) * (S' + gamma) - Z * (A + beta) * (Sv + gamma));
 *        l0 * (A' - S');   l_active * (A' - S') * (A' - A'[(i - 2^e) mod N])
 *   h[i] = V[i] * t_inv[i mod 2^e],  t_inv[r] = (zeta^n * (w^n)^r - 1)^-1: 2^e constants, inverted on the host.
 * Every array of indices, offsets, coefficients and challenges is HOST memory (copied, not kept); d_columns, d_fixed,
 * d_sigmas, d_perm_products, the three lookup tables of pointers and d_h are HOST arrays of DEVICE pointers, 16-byte
 * aligned, N 32-byte cells each in the representation of the pass.  Coefficients and challenges: 32 bytes as stored in
 * that representation, below p.  V is held in the representation of the cells; the R factors that products of
 * canonical cells lose are absorbed into staged constants (coeff * R^d per monomial, one scaled l0 / l_last / l_active
 * per row), so the output is exact bit for bit in both forms.  Nothing in device memory but the gadget's scratch and
 * d_h is written.
 * Decided on the device (status: a host array of K words; may be NULL):
 *   HSW_QUOTIENT_CELL_NOT_BELOW_P  a stored cell that the proof read is not an encoding below p: the proof is REFUSED --
 *                                  not one byte of its d_h[c] is written.
 * The others are written; the call returns HSW_OK and the report counts the refusals.  Nothing outside rows [0, N) of
 * the d_h of written proofs is ever written.
 * Refused before any launch -- HSW_ERR_INVALID_ARG (hsw_last_error names the item): n_proofs 0; all three families
 * empty; log_n above 28; e outside 1 .. HSW_QUOTIENT_MAX_EXTENSION; usable_rows 0 or >= n; unknown flags; an offset
 * array that is not ascending or does not end at its count; a monomial of more than HSW_QUOTIENT_MAX_FACTORS factors; a
 * column index >= m + F; |rotation| >= n; a lookup without an input or a table column; a pointer (array or column) that
 * is NULL where it is needed or not 16-byte aligned; a coefficient, challenge, zeta or delta that is missing where
 * needed or not below p; omega_ext with w^(N/2) != p - 1; a zeta for which some zeta^n (w^n)^r - 1 is 0; a d_h[c]
 * whose N cells overlap any column the call reads or another d_h.  HSW_ERR_TOO_LARGE: counts that do not fit 32 bits.
 * HSW_ERR_UNSUPPORTED: HSW_REPR_COMPACT64 cells, a pass whose batches differ in representation.
 * One launch per family that is present (all gates; all sets; all lookups) and the finish, per batch of proofs; a
 * thread owns rows_per_thread consecutive rows.  V lives in the gadget's scratch, N cells per proof: proofs go in
 * batches whose scratch stays under 1 GiB (the engine option "quotient_scratch", 1 .. 2^30 bytes, lowers it: a test
 * knob), a batch being at least one proof; grown on demand and freed by hsw_gadget_destroy.  The host reads nothing
 * between the launches.  Synchronous, on the engine's stream.
 * Not built: lookup inputs and tables that are expressions (q * a) rather than single columns folded with theta;
 * halo2's fold of several circuit instances into one h under one transcript (K means K independent proofs); the domain
 * constants, l0 / l_last / l_active in extended form, the blinding rows, the split of h into pieces and the transcript
 * stay the prover's.  (The call came under HSW_ABI_MINOR 1: probe for the symbol.) */
#define HSW_QUOTIENT_CELL_NOT_BELOW_P 4u   /* status bit, the value of HSW_NTT_CELL_NOT_BELOW_P */
#define HSW_QUOTIENT_MAX_FACTORS 8u        /* factors of one monomial */
#define HSW_QUOTIENT_MAX_EXTENSION 8u      /* e = log_n - log_rows, 1 .. 8 */
typedef struct hsw_quotient_gates {        /* all HOST arrays, copied, not kept; n_gates 0: no gate */
    size_t n_gates, n_terms, n_factors;
    const uint32_t *gate_first_term;       /* n_gates + 1, ascending, [n_gates] == n_terms */
    const void *term_coeffs;               /* n_terms x 32 bytes as stored, below p */
    const uint32_t *term_first_factor;     /* n_terms + 1, ascending, [n_terms] == n_factors, <= MAX_FACTORS per term */
    const uint32_t *factor_column;         /* n_factors, < m + F */
    const int32_t *factor_rotation;        /* n_factors, |r| < n */
} hsw_quotient_gates;
typedef struct hsw_quotient_lookups {      /* n_lookups 0: none */
    size_t n_lookups;
    const uint32_t *first_input, *inputs;  /* n_lookups + 1 offsets; column indices < m + F, at least one per lookup */
    const uint32_t *first_table, *tables;  /* likewise */
    const void *const *d_permuted_inputs, *const *d_permuted_tables, *const *d_products;  /* contexts x n_lookups, [c*n_lookups + l], N cells, extended form */
    const void *thetas;                    /* host, contexts x 32 bytes */
} hsw_quotient_lookups;
typedef struct hsw_quotient {
    uint32_t flags, log_rows, log_n, chunk_columns;   /* flags 0; chunk_columns: L, >= 1 when n_perm_columns > 0 */
    uint64_t usable_rows;                  /* u, 1 <= u < n */
    size_t n_proofs, n_columns, n_fixed;   /* K, m, F */
    const void *const *d_columns;          /* host array, K x m device pointers, N cells each, extended form */
    const void *const *d_fixed;            /* host array, F device pointers, shared by the proofs; NULL when F == 0 */
    const void *d_l0, *d_l_last, *d_l_active;   /* device, N cells each, shared; required when a permutation or a lookup is listed */
    hsw_quotient_gates gates;
    size_t n_perm_columns;                 /* 0: no permutation argument */
    const uint32_t *perm_columns;          /* host, column indices < m + F in the permutation's order */
    const void *const *d_sigmas;           /* host array, n_perm_columns device pointers, N cells, shared */
    const void *const *d_perm_products;    /* host array, K x S, [c*S + s], N cells */
    hsw_quotient_lookups lookups;
    const void *betas, *gammas, *ys;       /* host, K x 32 bytes as stored, below p; betas/gammas needed only with a permutation or a lookup */
    const void *omega_ext, *zeta, *delta;  /* host, 32 bytes each as stored, below p; delta only with a permutation */
    void *const *d_h;                      /* host array, K device pointers, N cells each */
    uint32_t *status;                      /* host, K words, output; may be NULL */
} hsw_quotient;
typedef struct hsw_quotient_report {
    uint64_t proofs, written, refused_proofs, first_refused;   /* written = N x proofs not refused; first_refused ~0 where none */
    uint64_t expressions, scratch_bytes;   /* y-folds per proof; scratch of a batch */
    uint32_t launches, rows_per_thread;
    float kernel_ms, gates_ms, permutation_ms, lookups_ms, finish_ms;
} hsw_quotient_report;
int hsw_gadget_quotient(hsw_gadget *g, const hsw_quotient *args, hsw_quotient_report *report);
/* AssignedHashResult.input_bytes of digest #hash_idx (the padded variable part). */
int hsw_gadget_input_bytes(hsw_gadget *g, size_t hash_idx, uint8_t *out, size_t cap, size_t *len);
/* HSW_REPR_CANONICAL (default) or HSW_REPR_MONTGOMERY for subsequent digests. */
int hsw_gadget_set_repr(hsw_gadget *g, uint32_t repr);

/* Synchronous device-to-host copy on the engine's stream (for callers that hold
 * device pointers from hsw_gadget_streams but have no HIP binding of their own). */
int hsw_download(hsw_engine *e, void *host_dst, const void *d_src, size_t bytes);

/* Calibration: overwrites `bytes` of d_buf with a plain 16-byte-per-lane
 * streaming fill and returns its duration -- the practical HBM write ceiling
 * of this device/allocation, which bench.py reports next to the 8 TB/s spec. */
int hsw_fill_calibrate(hsw_engine *e, void *d_buf, size_t bytes, float *ms);

/* Tuning knobs (never change results).  "parts": waves per block, 0 = chosen
 * from the batch size (default), or 1, 2, 4, 8, 16.  "tile": cells per
 * contiguous run of one unit, 0 = chosen by the engine (default), 32, 64 or 128
 * (also 6416 = [16 rows][64 cells], the default of the compact form).  "split": how tiny batches
 * are dealt to waves -- -1 = the small-batch kernel (37 waves per block, one sub-unit program each) for
 * batches of <= 128 blocks (default), 0 = never, 1 = one phase program per wave (32 waves per block),
 * 2 = the small-batch kernel always.  "helpers": waves per workgroup (= role) of the small-batch kernel --
 * they share the write-out of every tile; 0 = chosen by the engine (default: 4 for Montgomery cells, else 4 / 2 / 1
 * up to 16 / 64 / 128 blocks), 1..4.  "verify_slices": workgroups per block of hsw_verify_blocks, 0 = default.
 * "mont_emit": where Montgomery cells of the streaming kernel are converted (8-bit table only) -- 0 = at
 * write-out always, 1 = at emit time for default-mode launches of 1,536 blocks or more (default; fewer VALU
 * instructions than the canonical kernel, but one wave per block), 2 = at emit time always (also internals mode).
 * "chunk_blocks": blocks per kernel launch of a long batch (default and maximum 2^20; a test knob).
 * "lookup_lds": hsw_gadget_lookup_multiplicities counts tables of up to 2^11 rows in LDS first (1, default) or every
 * table by global atomics (0; a measuring knob).
 * "permuted_scratch": bytes of scratch hsw_gadget_lookup_permuted holds at a time (default 256 MiB, 1 .. 2^32): the
 * multiplicities where the caller passes no d_m (at most half of it, else HSW_ERR_TOO_LARGE) and the index arrays and value
 * tables of a group of arguments; the arguments are processed in groups that fit, a group being at least one proof.
 * "quotient_scratch": bytes of accumulators hsw_gadget_quotient holds at a time (default and maximum 2^30, 1 .. 2^30):
 * the proofs of a call go in batches that fit, a batch being at least one proof (a test knob).
 * "round_scratch": bytes of scratch that hsw_gadget_ntt, hsw_gadget_msm, hsw_gadget_evaluate and hsw_gadget_open hold
 * between the launches of a group of columns or of a batch (default and maximum 2^30, 1 .. 2^30): the points of the NTT's
 * columns, the MSM's partial buckets, the tiles' sums of evaluate and the scratch of open's groups; a group or batch is
 * at least one column, one group, or one column with all its points (a test knob; the grid limits do not move). */
int hsw_engine_set_option(hsw_engine *e, const char *name, int64_t value);

const char *hsw_strerror(int status);
/* Detail of the last failure on this engine ("" if none); never NULL. */
const char *hsw_last_error(const hsw_engine *e);
uint32_t hsw_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HSW_H */
