// hsw_gadget.hpp -- host-side mirror of the reference's gadget front-end.
//
// Mirrors, by name and argument meaning, reference src/lib.rs:
//   AssignedHashResult            lib.rs:31-36
//   Sha256DynamicConfig           lib.rs:38-45
//     ::configure                 lib.rs:49-69
//     ::digest                    lib.rs:71-349
//     ::new_context               lib.rs:351-360
//     ::load                      lib.rs:366-368  (spread table, spread.rs:165-194)
// What differs is only where the per-block work happens: the block loop of
// lib.rs:180-238 becomes ONE hsw_witness_blocks call (HIP) for all blocks of
// a digest -- or of a whole batch of digests.
//
// SURVEY 8 f4 -- the cells digest() itself allocates around the block loop
// (length constraints lib.rs:122-151, inputs :162-178, is_equal/select :294-310,
// output bytes :311-341) -- are emitted by a context created with
// HSW_GADGET_WHOLE_DIGEST (hsw_frame.hpp / hsw_frame_kernel, assumption A4);
// without it only their *values* are produced (AssignedHashResult).
//
// Implemented in several translation units: hsw_gadget_sha.cpp (padding, host SHA, digest_plan / digest_prepare: no HIP
// call), hsw_gadget_context.cpp (Context: buffers, layouts, bind / unbind, the jump table), hsw_gadget_digest.cpp (the
// digest paths and the ties), hsw_gadget_lookup.cpp (the lookup entries of a pass, listed and counted),
// hsw_gadget_permuted.cpp (the permuted lookup columns of a pass), hsw_gadget_product.cpp (their grand product Z),
// hsw_gadget_permutation.cpp (the permutation argument's grand products), hsw_gadget_ntt.cpp (the Fr NTT of device
// columns), hsw_gadget_msm.cpp (their commitments: the G1 MSM), hsw_gadget_open.cpp (their evaluations and opening
// quotients), hsw_gadget_shplonk.cpp (SHPLONK's multi-point opening), hsw_gadget_quotient.cpp (the quotient h(X) on the
// extended coset) and hsw_gadget.cpp (the rest of the C ABI); hsw_gadget_launch.hpp is what only they share, and
// hsw_gadget_call.hpp what the calls of the round from hsw_gadget_permuted.cpp on share beyond it.
#ifndef HSW_GADGET_HPP
#define HSW_GADGET_HPP

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/hsw.h"
#include "hsw_gadget_layout.hpp"

namespace hsw {

// Value-level result of lib.rs:77-160 for one message.
struct DigestPlan {
    std::vector<uint8_t> blocks;   // padded_inputs[precomputed_input_len..]: max_variable_byte_size bytes
    uint32_t init_state[8];        // INIT_STATE after compress256 over the precomputed prefix (lib.rs:153-160)
    size_t num_round = 0;          // lib.rs:80-84
    size_t precomputed_round = 0;  // lib.rs:93
    size_t target_round = 0;       // num_round - precomputed_round (lib.rs:147-151): index into the state list
    size_t max_variable_round = 0; // lib.rs:87: compressions synthesised, always the maximum
};

// The part of lib.rs:77-93 that needs no bytes: the four round counts of *plan from the lengths alone, with the
// refusals below (blocks and init_state are left alone).
int digest_plan(size_t input_byte_size, size_t precomputed_input_len, size_t max_variable_byte_size, DigestPlan *plan);

// sha2::compress256 (lib.rs:160) of one block on the host, and whether it runs on the x86 SHA extensions
void plain_compress(uint32_t st[8], const uint8_t *block);
bool host_sha_is_fast();

// lib.rs:77-117,153-160.  Returns HSW_OK or the status the reference's
// assert!/debug_assert! maps to (HSW_ERR_SHAPE / HSW_ERR_TOO_LARGE).
int digest_prepare(const uint8_t *input, size_t input_byte_size, size_t precomputed_input_len,
                   size_t max_variable_byte_size, DigestPlan *plan);

// lib.rs:31-36 on values, plus where this hash's streams live.
struct AssignedHashResult {
    uint64_t input_len = 0;              // assigned_input_byte_size (lib.rs:124-125)
    std::vector<uint8_t> input_bytes;    // assigned_input_bytes (lib.rs:170-173): the padded variable part
    uint8_t output_bytes[32] = {0};      // lib.rs:311-341
    size_t first_block = 0;              // index of this hash's first block in the context's streams
    size_t n_blocks = 0;                 // max_variable_byte_size / 64
    uint64_t spread_cursor0 = 0;         // SpreadConfig.num_limb_sum when this digest started
    size_t num_round = 0, target_round = 0, precomputed_round = 0;   // (precomputed_round: lib.rs:93, hashed outside the circuit)
    // whole-digest contexts: where the sections of this digest start (cells)
    uint64_t prologue_cell = 0, block_cell = 0, epilogue_cell = 0, end_cell = 0;
    uint64_t zero_cell = ~0ull;          // the Context's zero cell, if this digest is the one that loads it (else ~0)
    uint64_t prologue_lookup = 0, block_lookup = 0, epilogue_lookup = 0;
};

class Context;

// a block of device memory that is replaced by a larger one on demand: the members are in hsw_gadget_call.hpp
struct DeviceScratch {
    void *d = nullptr;
    size_t cap = 0;                  // bytes
    int reserve(size_t bytes);
    void release();
};

// base + cells * cell_bytes, the offset taken modulo 2^64 as the kernels take it: a column given by pointer table may
// lie below entry 0 of its table
inline uint8_t *cell_ptr(const void *base, uint64_t cells, size_t cell_bytes = HSW_CELL_BYTES) {
    return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(base) + (uintptr_t)(cells * cell_bytes));
}

// The device jump table (Context::d_place, PlaceTable of hsw_kernels.h) in uint64 words, section by section:
//   [jump cells n][cumulative gaps n -- by pointer table a row per Context][lookup shifts per digest, at least one word]
//   and by pointer table too: [lookup rows K (PlaceTable::lk_row)][chip rows K * ncols * 2 (PlaceTable::chip_row)]
// n = the layout's jumps -- by pointer table one more, jump 0 at stream cell 0.  Context::upload_place writes the table
// through these offsets and Launch reads it through them
struct PlaceWords {
    size_t n = 0, cum = 0, shifts = 0, n_shifts = 0, lk_rows = 0, chip_rows = 0, total = 0;
};

// What a library-owned gadget holds (Context::owned), in cells: d_gate, d_lookup, each of d_chip_dense / d_chip_spread
// (chip_stride rows in each of their columns, 0 for a gadget without blocks)
struct OwnedCells { size_t image = 0, lookup = 0, chip = 0, chip_stride = 0; };

class Sha256DynamicConfig {
  public:
    std::vector<size_t> max_variable_byte_sizes;   // lib.rs:40
    size_t cur_hash_idx = 0;                       // lib.rs:43
    uint32_t num_bits_lookup = 8;                  // SpreadConfig (spread.rs:24-25)
    uint32_t num_advice_columns = 2;
    bool is_input_range_check = false;             // lib.rs:44 (the 8-bit range checks are halo2-base cells: emitted
                                                   // by whole-digest contexts only)

    // lib.rs:49-69.  HSW_ERR_SHAPE if a size is not a multiple of 64 (lib.rs:57-59)
    // or the spread shape is invalid (spread.rs:37).
    static int configure(const std::vector<size_t> &max_variable_byte_sizes, uint32_t num_bits_lookup,
                         uint32_t num_advice_columns, bool is_input_range_check, Sha256DynamicConfig *out);

    // lib.rs:351-360: a context sized for every hash this config will assign.
    // whole_digest: also lay out digest()'s own cells (HSW_GADGET_WHOLE_DIGEST)
    // group_m: a Context group (hsw_gadget_create_contexts) -- max_variable_byte_sizes holds K Contexts' group_m sizes each
    int new_context(hsw_engine *engine, Context **out, bool whole_digest = false, bool independent = false,
                    bool context_images = false, bool shared = false, size_t group_m = 0) const;

    // lib.rs:71-349.  precomputed_input_len = 0 is the reference's None.
    int digest(Context &ctx, const uint8_t *input, size_t input_len, size_t precomputed_input_len,
               AssignedHashResult *result);
    // n consecutive digest() calls with one kernel launch; results[i] as if called in order.
    int digest_batch(Context &ctx, size_t n, const uint8_t *const *inputs, const size_t *input_lens,
                     const size_t *precomputed_input_lens, AssignedHashResult *results);
    // digest_batch with the message bytes in DEVICE memory (hsw_gadget_digest_batch_device): d_inputs[i] is a device
    // pointer of any alignment, the lengths are host values, the host never reads a byte.  Results as digest_batch's.
    int digest_batch_device(Context &ctx, size_t n, const void *const *d_inputs, const size_t *input_lens,
                            const size_t *precomputed_input_lens, AssignedHashResult *results);
    // digest_batch_device over dependency levels (hsw_gadget_digest_levels_device): levels[i] (NULL: all 0) orders the
    // messages, d_outputs[i] (NULL table or entry: none) receives digest i's 32 bytes in DEVICE memory, and a message
    // may read what a message of a strictly lower level writes.  One hsw_ingest_kernel launch per distinct level,
    // back to back on the engine's stream, then the common tail once; the host reads neither inputs nor outputs.
    // Overlapping outputs, and an input that overlaps the output of a message not of a lower level, are refused
    // (HSW_ERR_INVALID_ARG, the engine's error text names the two messages) before anything is launched or committed.
    int digest_levels_device(Context &ctx, size_t n, const void *const *d_inputs, const size_t *input_lens,
                             const size_t *precomputed_input_lens, const uint32_t *levels, void *const *d_outputs,
                             AssignedHashResult *results);

    // lib.rs:366-368 -> spread.rs:165-194: the (dense, spread) lookup table rows.
    std::vector<std::pair<uint64_t, uint64_t>> load() const;

  private:
    // what digest_batch and digest_batch_device share once the batch's blocks and pre-states are staged (hsw_gadget_digest.cpp)
    template <class Stage>
    int digest_tail(Context &ctx, size_t n, const size_t *input_lens, std::vector<DigestPlan> &plans, size_t batch_blocks,
                    bool host_chain, bool device_fed, Stage &&stage, AssignedHashResult *results);
};

// The Region-owning context of lib.rs:351-360, re-imagined for HBM: it owns the
// device buffers the streams are written to and SpreadConfig's mutable cursor.
class Context {
  public:
    ~Context();
    hsw_engine *engine = nullptr;
    hsw_shape shape{};
    size_t capacity_blocks = 0;      // sum(max_variable_byte_sizes) / 64
    size_t blocks_done = 0;
    uint64_t num_limb_sum = 0;       // SpreadConfig.num_limb_sum (spread.rs:26), starts at 0 (spread.rs:70)
    size_t chip_col_stride = 0;      // rows per chip column buffer
    void *d_gate = nullptr;          // capacity_blocks * G cells
    void *d_chip_dense = nullptr;    // ncols * chip_col_stride cells
    void *d_chip_spread = nullptr;
    uint32_t *d_next_states = nullptr;   // capacity_blocks * 8
    uint8_t *d_blocks = nullptr;         // staging: capacity_blocks * 64
    uint32_t *d_pre_states = nullptr;    // capacity_blocks * 8
    uint32_t *d_init_states = nullptr;   // one per hash in flight
    uint32_t *d_offsets = nullptr;       // first block of every hash in flight (+ 1): hsw_chain_var_kernel
    size_t init_capacity = 0;
    void *d_ingest = nullptr;            // device-fed batches: a message descriptor per hash in flight (hsw_ingest_kernel), on first use
    // small batches: pinned, device-mapped host staging the kernels read directly (no H2D copies) and
    // the next states are copied back into (a truly asynchronous D2H): capacity_blocks * (64 + 32 + 32) bytes
    uint8_t *hp_blocks = nullptr;        // host views ...
    uint32_t *hp_pre = nullptr, *hp_next = nullptr;
    uint8_t *dp_blocks = nullptr;        // ... and the device addresses of the same memory
    uint32_t *dp_pre = nullptr, *dp_next = nullptr;
    // compact delivery (hsw_gadget_download_region_compact): 8-byte staging of the streams, side list, its counter
    void *d_c_gate = nullptr, *d_c_lookup = nullptr, *d_c_dense = nullptr, *d_c_spread = nullptr, *d_wide = nullptr;
    uint32_t *d_wide_count = nullptr, *hp_wide_count = nullptr;
    size_t wide_cap = 0;
    uint32_t repr_flags = HSW_REPR_CANONICAL;
    // HSW_GADGET_WHOLE_DIGEST: d_gate is one stream (prologue | zero cell | blocks | epilogue per
    // digest, back to back) and d_lookup the lookup-advice stream next to it
    bool whole = false;
    bool independent = false;        // HSW_GADGET_INDEPENDENT: every digest is a Context of its own (K proofs in flight)
    // HSW_GADGET_CONTEXT_IMAGES (with independent, all digests of one size): every Context has an origin, a column
    // image and a lookup column of its own, laid out alike -- Context h's image is cells [h*S, (h+1)*S) of d_gate,
    // its lookup column cells [h*Lp, (h+1)*Lp) of d_lookup; the layout's breaks are ONE Context's
    bool context_images = false;
    uint64_t ctx_digest_cells = 0, ctx_own_lookups = 0;   // one Context's digest cells (zero cell not counted) and lookups
    uint64_t ctx_stream() const { return ctx_digest_cells + (layout.origin_zero_loaded ? 0u : 1u); }   // C: stream cells per Context
    uint64_t ctx_lookups() const {                                                               // Lp
        return group_m && layout.max_rows ? layout.lookups_end : layout.origin_lookups + ctx_own_lookups;
    }
    // hsw_gadget_create_contexts (with shared): K Contexts of group_m digests each, every one laid out like ONE shared
    // context (its jumps, its interludes, the jump table on the device) and repeated like context images -- Context
    // c's image is cells [c*S, (c+1)*S) of d_gate, its lookup column cells [c*Lp, (c+1)*Lp) of d_lookup, its chip rows
    // follow Context c-1's.  Digest d of the pass is digest d % group_m of Context d / group_m; the layout, the
    // declarations and ctx_digest_cells / ctx_own_lookups are ONE Context's
    size_t group_m = 0;
    size_t ctx_blocks = 0;                                     // blocks of one Context
    size_t contexts() const { return context_images ? init_capacity : group_m ? init_capacity / group_m : 1; }
    size_t context_of(size_t d) const { return context_images ? d : group_m ? d / group_m : 0; }   // of digest d of the pass
    // hsw_gadget_bind_region: d_gate, d_lookup and the chip columns are the CALLER's memory -- never freed, grown,
    // zeroed or filled here -- at the caller's pitches: the image columns layout.pitch cells apart, and (K Contexts)
    // every Context's image, lookup column and chip rows in a place of its own: layout.image_pitch,
    // binding.lookup_pitch and binding.chip_context_pitch cells after the previous Context's.  Library-owned, these
    // three are columns x max_rows, Lp and "consecutive rows of the same columns".  `binding` is what the caller
    // declared; the layout calls check what they need against its capacities (adopt)
    bool bound = false;
    hsw_region_binding binding{};
    // hsw_gadget_bind_columns: a bound region whose image columns are one allocation each -- col_off[c *
    // binding.columns_capacity + k] = cells from proof 0's column 0 (d_gate) to column k of proof c, modulo 2^64.  Every
    // launch then goes through the table path (the jumps of a plain image, a Context per proof of context images) with a
    // cum row per Context (PlaceTable::cum_stride, upload_place); layout.pitch = binding.column_pitch keeps positions
    // and break gaps those of a pitch-bound region, layout.image_pitch is 0 and no code adds h * image_cells()
    bool by_pointer = false;
    std::vector<uint64_t> col_off;
    bool table_path() const { return (shared || by_pointer) && layout.max_rows != 0; }
    // cells from d_gate to row 0 of image column k of Context c
    uint64_t column_cell(uint64_t c, uint64_t k) const {
        return by_pointer ? col_off[(size_t)(c * binding.columns_capacity + k)] : c * layout.image_cells() + k * layout.column_pitch();
    }
    // cells from d_gate to gate-stream cell `cell` (whole-digest contexts) in the layout and binding in force, modulo
    // 2^64: the linear stream, the image after its jumps, the owning Context's image, the caller's pitches or its
    // own column pointer (hsw_gadget_cell_address)
    uint64_t cell_offset(uint64_t cell) const {
        const Layout &l = layout;
        if (!l.max_rows) return cell;
        if (!by_pointer) return l.image_cell(cell);
        const uint64_t h = l.period ? cell / l.period : 0, local = cell - h * l.period;
        const uint64_t at = local + l.origin_row + l.gap_at(local), P = l.column_pitch();
        return column_cell(h, at / P) + at % P;
    }
    // hsw_gadget_bind_column_tables: the lookup-advice column and / or the chip columns one allocation each as well (an
    // empty vector: that family keeps the pitch model).  lk_off[c] = cells from d_lookup (proof 0's column) to row 0
    // of proof c's; chip_dense_off / chip_spread_off[c * ncols + k] = cells from d_chip_dense / d_chip_spread (proof
    // 0's chip column 0) to row 0 of chip column k of proof c -- all modulo 2^64.  Positions (hsw_hash_result's
    // lookup cells, the cursors) stay an unbound gadget's: lookup_pitch() is Lp, and lookup_extra(c) is what the
    // addresses of Context c lie further (PlaceTable::lk_row; folded into the frames' lookup cells and Launch::run)
    std::vector<uint64_t> lk_off, chip_dense_off, chip_spread_off;
    bool lookup_by_table() const { return !lk_off.empty(); }
    bool chips_by_table() const { return !chip_dense_off.empty(); }
    uint64_t lookup_pitch() const { return bound && contexts() > 1 && !lookup_by_table() ? binding.lookup_pitch : ctx_lookups(); }
    uint64_t lookup_extra(uint64_t c) const { return lookup_by_table() ? lk_off[(size_t)c] - c * ctx_lookups() : 0; }
    // cells from d_lookup to row 0 of Context c's lookup column
    uint64_t lookup_cell(uint64_t c) const { return c * lookup_pitch() + lookup_extra(c); }
    size_t blocks_per_context() const { return context_images ? capacity_blocks / init_capacity : group_m ? ctx_blocks : capacity_blocks; }
    uint64_t ctx_limb_calls() const { return (uint64_t)blocks_per_context() * shape.limb_calls_per_block; }
    uint64_t ctx_chip_rows() const { return (ctx_limb_calls() + shape.num_advice_columns - 1) / shape.num_advice_columns; }
    // cells from where consecutive rows would put a Context's chip rows to where they lie, per Context (modulo 2^64;
    // ExpandParams::chip_ctx_extra)
    uint64_t chip_ctx_extra() const { return bound && contexts() > 1 && !chips_by_table() ? binding.chip_context_pitch - ctx_chip_rows() : 0; }
    // chip cell of limb call n (counted from the pass's first), from d_chip_dense / d_chip_spread: the pitch model
    uint64_t chip_cell(uint64_t n) const {
        const uint64_t ncols = shape.num_advice_columns, extra = chip_ctx_extra();
        return (n % ncols) * chip_col_stride + n / ncols + (extra ? n / ctx_limb_calls() * extra : 0);
    }
    // what a launch whose first limb call is n (a multiple of ncols) adds to d_chip_dense / d_chip_spread: the place
    // of n's row in column 0 -- by table, the columns' absolute row, which the Context's chip_row entries count from
    uint64_t chip_launch_cell(uint64_t n) const { return chips_by_table() ? n / shape.num_advice_columns : chip_cell(n); }
    // cells from d_chip_dense (spread: d_chip_spread) to the first chip row of Context c in chip column k
    uint64_t chip_column_cell(uint64_t c, uint64_t k, bool spread) const {
        if (chips_by_table()) return (spread ? chip_spread_off : chip_dense_off)[(size_t)(c * shape.num_advice_columns + k)];
        return k * chip_col_stride + c * (ctx_chip_rows() + chip_ctx_extra());
    }
    // the Contexts whose chip rows are counted apart (download_region): one run of rows per column otherwise
    bool chip_rows_per_context() const { return chip_ctx_extra() != 0 || (chips_by_table() && contexts() > 1); }
    // d_lookup cells ONE Context needs with layout l (Lp; one Context: the whole column)
    uint64_t lookups_needed(const Layout &l) const {
        return context_images ? l.origin_lookups + ctx_own_lookups : shared && l.max_rows ? l.lookups_end : l.origin_lookups + own_lookup_capacity;
    }
    // the library's own zeroed buffers again, sized for the layout without pitches (sizes / rc_inputs: the gadget's)
    int unbind(const std::vector<size_t> &sizes, bool rc_inputs);
    // t: NULL = hsw_gadget_bind_region; else the pointer tables of hsw_gadget_bind_columns (the image's only) or
    // hsw_gadget_bind_column_tables.  Validated in full before anything changes
    int bind(const std::vector<size_t> &sizes, bool rc_inputs, const hsw_region_binding &b, const hsw_column_tables *t = nullptr);
    bool zero_loaded = false;        // Context.zero_cell (first load_zero: compression.rs:34 of the first block)
    uint64_t gate_cursor = 0, gate_capacity = 0;       // cells
    void *d_lookup = nullptr;
    uint64_t lookup_cursor = 0, lookup_capacity = 0;
    uint64_t own_lookup_capacity = 0;                  // the gadget's own lookup entries (all Contexts)
    // what every digest_batch call wrote, for hsw_gadget_verify
    struct BatchRecord { size_t first_digest, n_digests, first_block, n_blocks; bool inputs_in_pinned; uint32_t repr_flags; };
    std::vector<BatchRecord> batches;
    // The origin and the stream-to-image map (hsw_gadget_layout.hpp).  With an image, d_gate is layout.columns
    // advice columns of layout.max_rows cells (context images: one such image per Context, back to back)
    Layout layout;
    // HSW_GADGET_SHARED_CONTEXT: the same Context for every digest of the pass, the caller's own cells in between
    // (interludes, hsw_gadget_set_digest_origin).  The layout's jumps are then column breaks and interludes, of any
    // number (up to HSW_GADGET_MAX_COLUMNS columns), and the kernels read them from a table on the device
    bool shared = false;
    std::vector<DigestOrigin> declared;                // per digest of the pass ([0] unused)
    std::vector<uint64_t> place_host;                  // what d_place holds (an unchanged table is not uploaded again)
    uint64_t image_columns = 0;                        // shared context: image columns allocated (>= layout.columns)
    void *d_place = nullptr;                           // device copy of the jump table (hsw_kernels.h PlaceTable)
    size_t place_cap = 0;                              // uint64 words of d_place
    bool place_dirty = true;                           // the layout changed since the last upload
    PlaceWords place_words() const;                    // where d_place's sections start, for the layout and binding in force
    int upload_place();                                // d_place from the layout, if it changed
    OwnedCells owned(const Layout &l) const;
    // the frame kernels' descriptor of digest d of the pass from its result: the generator and the verifier make it here
    hsw_frame_desc frame_desc(const AssignedHashResult &r, size_t d, bool rc_inputs) const;
    // The runs of the gate stream between two jumps, up to `cursor`, of every Context begun: fn(Context, lo, hi) with
    // [lo, hi) in the Context's own stream cells (one Context: the pass's).  Each run lies in one image column
    template <class Fn>
    void for_each_run(uint64_t cursor, Fn &&fn) const {
        const Layout &l = layout;
        const uint64_t K = l.period ? (cursor + l.period - 1) / l.period : 1;
        for (uint64_t h = 0; h < K; h++) {
            const uint64_t end = !l.period ? cursor : cursor < (h + 1) * l.period ? cursor - h * l.period : l.period;
            uint64_t lo = 0;
            for (size_t k = 0; k <= l.break_cell.size() && lo < end; k++) {
                const uint64_t hi = k < l.break_cell.size() && l.break_cell[k] < end ? l.break_cell[k] : end;
                if (hi > lo) { fn(h, lo, hi); lo = hi; }
            }
        }
    }
    // The layout this context would have with columns of `rows` cells (0: none) at the origin of *out, checked
    // against the limit of its kind (HSW_ERR_TOO_LARGE); decl: a shared context's declarations.  Touches nothing.
    int plan_layout(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t rows, const std::vector<DigestOrigin> &decl,
                    Layout *out) const;
    // Makes `nl` the layout.  fresh_image / fresh_lookup: the image / the lookup column is replaced by a zeroed
    // one sized for nl; a shared context's buffers grow instead, keeping what they hold, and if the map changed its
    // image cells [clear_from, end) -- what an earlier layout may have written there -- are zeroed again (unassigned
    // advice cells are 0).  Nothing is touched unless every allocation succeeded.  A bound region is the caller's:
    // nothing is allocated, grown or zeroed, and a layout that needs more columns or lookup cells than the binding
    // declares is HSW_ERR_TOO_LARGE.
    int adopt(Layout &nl, bool fresh_image, bool fresh_lookup, uint64_t clear_from);
    // hsw_gadget_set_origin: validated in full (layout included) before anything is freed or reallocated
    int set_origin(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t column, uint64_t row, bool zero_cell_loaded,
                   uint64_t lookups_queued);
    // device address of stream cell 0 (32-byte cells: whole-digest contexts have no compact form)
    void *gate_stream() const {
        return static_cast<uint8_t *>(d_gate) + (size_t)(layout.max_rows ? layout.origin_row : 0) * HSW_CELL_BYTES;
    }
    // Lay the whole-digest stream out as FlexGate (Vertical) advice columns of max_rows usable rows.
    // Only before the first digest.  HSW_ERR_TOO_LARGE: more than HSW_MAX_BREAKS + 1 columns.
    int set_columns(const std::vector<size_t> &max_variable_byte_sizes, bool is_input_range_check, uint64_t max_rows);
    void free_compact_staging();                       // the 8-byte staging follows the geometry: dropped when it changes
};

// The input-independent half of a whole region (hsw_replay.cpp): which cells are NEW witnesses, and for every other
// cell of the gate / lookup / chip streams which witness or constant it repeats.
struct RegionTape;
void free_region_tape(RegionTape *t);
void drop_region_tape_positions(RegionTape *t);

}  // namespace hsw

struct hsw_gadget {
    hsw::Sha256DynamicConfig cfg;
    hsw::Context *ctx = nullptr;
    std::vector<hsw::AssignedHashResult> results;   // one per digest so far (input_bytes kept for queries)
    hsw::RegionTape *tape = nullptr;                // built on first use, dropped when the layout changes
    // Digest-to-digest copy constraints of the pass (hsw_gadget_ties; whole-digest gadgets).  tie_owners: the device
    // bytes that hold a digest of the pass, as disjoint runs -- [start, start + len) holds output bytes byte0.. of
    // digest `hash` -- a later destination replacing what it covers.  Host memory only; hsw_gadget_reset clears it
    struct TieOwner { size_t len; uint64_t hash; uint32_t byte0; };
    struct Tie { uint64_t src_hash, dst_hash; uint32_t src_byte, dst_byte; };
    std::map<uintptr_t, TieOwner> tie_owners;
    std::vector<Tie> ties;                          // in (dst_hash, dst_byte) order: digests and bytes are walked ascending
    uint64_t tie_prefix_bytes = 0;                  // shared bytes inside a precomputed prefix: no cell, not tied
    // The cursors of a pass that starts at digest hash_idx (0: hsw_gadget_reset; else hsw_gadget_seek, the earlier
    // digests assigned elsewhere): nothing recorded, nothing to verify or to tie to
    void start_pass(size_t hash_idx, size_t blocks, uint64_t gate_cells, uint64_t lookup_cells) {
        hsw::Context &c = *ctx;
        c.blocks_done = blocks;
        c.num_limb_sum = (uint64_t)blocks * c.shape.limb_calls_per_block;       // spread.rs:70-71, 228-231
        c.gate_cursor = gate_cells;
        c.lookup_cursor = lookup_cells;
        c.zero_loaded = c.layout.origin_zero_loaded || hash_idx > 0;
        c.batches.clear();
        cfg.cur_hash_idx = hash_idx;            // lib.rs:66
        results.clear();
        results.resize(hash_idx);               // keeps hash_idx -> result indexing of hsw_gadget_input_bytes
        tie_owners.clear(); ties.clear(); tie_prefix_bytes = 0;   // the ties are the pass's
    }
    // the device-fed batch just committed as digests [first, first + n): its destinations, then its ties
    void record_ties(size_t first, size_t n, const void *const *d_inputs, const size_t *input_lens,
                     const size_t *precomputed_input_lens, void *const *d_outputs);
    void *d_pairs = nullptr;                        // hsw_gadget_verify_ties / _equal: address pairs on the device,
    size_t pairs_cap = 0;                           // grown on demand, freed by hsw_gadget_destroy
    void *d_lookup_runs = nullptr;                  // hsw_gadget_lookup_multiplicities (hsw_gadget_lookup.cpp): its report, run
    size_t lookup_runs_cap = 0;                     // table and zero lists on the device, in bytes; grown and freed like d_pairs
    // what the calls of the round from hsw_gadget_lookup_permuted to hsw_gadget_quotient stage and work in, one after the
    // other: each reserves what it needs, stages all it reads and leaves nothing a later call reads (hsw_gadget_call.hpp)
    hsw::DeviceScratch scratch;
    // the tables of the powers of the roots hsw_gadget_ntt was last called with: root in Montgomery form, log_n, the
    // device table (2^(log_n - 1) cells); stamp orders them by last use (0: free).  Freed by hsw_gadget_destroy
    struct NttTable { uint32_t root[8]; uint32_t log_n; void *d_table; size_t bytes; uint64_t stamp; };
    NttTable ntt_tables[4] = {};
    uint64_t ntt_stamp = 0;
    ~hsw_gadget() { hsw::free_region_tape(tape); }
};
#endif
