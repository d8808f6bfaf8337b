// hsw_kernels.h -- internal launch interface between the C ABI (hsw_api.cpp)
// and the gfx950 kernels (hsw_expand.hpp, hsw_kernels.hip).  Not part of the public boundary.
#ifndef HSW_KERNELS_H
#define HSW_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hsw {

enum : uint32_t {
    HSW_K_MONTGOMERY = 1u,   // mirrors HSW_REPR_MONTGOMERY
    HSW_K_SKIP_GATE = 2u,    // mirrors HSW_SKIP_GATE
    HSW_K_SKIP_CHIP = 4u,    // mirrors HSW_SKIP_CHIP
    HSW_K_COMPACT = 8u,      // HSW_REPR_COMPACT64: 8-byte cells
    HSW_K_INTERNALS = 16u,   // engine mode HSW_MODE_HALO2_INTERNALS: range_check cells + lookup stream
    HSW_K_SPLIT = 32u,       // 32 waves per block, each running one phase program (tiny batches: latency)
    HSW_K_CHAINED = 64u,     // small-batch kernel: the blocks are ONE message, pre_states holds its initial state only
    HSW_K_ROLE_MAJOR = 128u, // small-batch kernel: grid = role x block instead of block x role (hsw_small.hpp)
    HSW_K_M32 = 256u,        // with HSW_K_MONTGOMERY, streaming kernel, 8-bit table: Montgomery form built at EMIT time, tiles of
                             // finished 32-byte cells (hsw_expand.hpp Em::M32); else one conversion per cell at write-out
};
enum { HSW_K_MAX_BREAKS = 16 };
enum { HSW_M32_TILE = 8 };                     // cells per tile row of the emit-time Montgomery kernels (Em::M32): [64][8] x 32 B = 16 KiB
enum { HSW_CHAIN_WAVE_MAX_MESSAGES = 2048 };   // chain pre-pass: up to this many messages get a wave each (8 waves per CU), beyond
                                               // that one lane per message has the parallelism anyway
enum { HSW_SMALL_WAVES_PER_BLOCK = 37 };   // roles of the small-batch kernel (hsw_small.hpp)
enum { HSW_SMALL_AUTO_BLOCKS = 128 };      // the engine picks the small-batch kernel up to this many blocks per launch
                                           // (tools/small_n.py: faster than the streaming kernel up to ~190 canonical, ~250 Montgomery)
#ifndef HSW_SMALL_MAX_HELPERS
#define HSW_SMALL_MAX_HELPERS 4            // waves per role (workgroup): the emitter + up to 3 helper waves; a launch
                                           // bound of 512 threads made every wave of the kernel crawl (57 vs 33 us)
#endif

struct ExpandParams {
    const uint8_t *blocks;        // n_blocks * 64 bytes
    const uint32_t *pre_states;   // n_blocks * 8
    void *gate;                   // n_blocks * G cells of 32 B
    void *chip_dense;             // ncols columns, chip_col_stride cells apart
    void *chip_spread;
    uint32_t *next_states;        // n_blocks * 8, may be null
    size_t n_blocks;
    size_t chip_col_stride;       // cells
    uint64_t cursor0;             // SpreadConfig.num_limb_sum before block 0
    uint32_t ncols;               // num_advice_columns
    uint32_t flags;               // HSW_K_*
    uint32_t parts;               // waves per block: 1, 2, 4, 8 or 16
    void *lookup;                 // n_blocks * LOOKUP_CELLS cells (internals mode), may be null
    // FlexGate column packing: gate cell i is written at i + sum of break_gap[k] over break_cell[k] <= i
    uint32_t n_breaks;
    uint64_t break_cell[HSW_K_MAX_BREAKS];
    uint64_t break_gap[HSW_K_MAX_BREAKS];
    // whole-digest streams (internals mode): after every frame_every blocks the gate stream skips
    // frame_cells cells and the lookup stream frame_lookups cells (a digest's epilogue and the
    // next digest's prologue, written by hsw_frame_kernel); frame_every = 0: off
    uint64_t frame_every, frame_cells, frame_lookups;
    // context images (HSW_GADGET_CONTEXT_IMAGES): every frame_every blocks are one Context of their own whose gate
    // cells lie ctx_cells (= columns x max_rows) cells after the previous one's; block b of context b / frame_every
    // sits at (b / frame_every) * ctx_cells + (b % frame_every) * G + the gaps of ONE context's break table
    // (frame_cells unused; frame_lookups then includes the next context's caller-owned lookup cells).  0 = off
    uint64_t ctx_cells;
    uint32_t *next_states_host;   // small-batch kernel only: a second copy of next_states, in pinned host memory (may be null)
    const void *mont_tab;         // HSW_K_M32 only: 3 x 256 Montgomery-form cells -- i, spread(i), i << 8 for i < 256 (hsw_api.cpp)
    // bound regions (hsw_gadget_bind_region) with a Context per frame_every blocks: the chip rows of Context
    // b / frame_every start chip_ctx_extra cells further per Context than consecutive rows would put them
    // (= chip_context_pitch - rows of one Context, modulo 2^64).  0 = consecutive rows of the same columns
    uint64_t chip_ctx_extra;
};

// limbs = 16 / num_bits_lookup.  Returns hipErrorInvalidValue for a limb count
// this build has no instantiation for.
// tile = cells per tile row: 32 (64 units per wave), 64 (32 units, parts >= 2) or
// 128 (16 units, parts >= 4).
hipError_t launch_expand(const ExpandParams &p, int limbs, int tile, hipStream_t stream);
hipError_t launch_chain(const uint8_t *blocks, size_t n_messages, size_t blocks_per_message,
                        const uint32_t *init_states, uint32_t *pre_states, hipStream_t stream);

hipError_t launch_chain_var(const uint8_t *blocks, size_t n_messages, const uint32_t *offsets,
                            const uint32_t *init_states, uint32_t *pre_states, hipStream_t stream);
// One message of hsw_gadget_digest_levels_device for hsw_ingest_kernel: len bytes at the DEVICE address src (any
// alignment; never dereferenced when len == 0), padded to num_round rounds of which the first precomputed_round are
// only compressed and the next n_blocks (zero rounds past num_round included) are staged from block first_block on.
// msg: the message's index in the call (its row of init_states), whatever its place in the table.  dst: NULL, or the
// DEVICE address (any alignment) of the 32 bytes that receive the digest, the state after round num_round - 1.
struct IngestDesc {
    const uint8_t *src;
    uint64_t len;
    uint32_t first_block, n_blocks, num_round, precomputed_round;
    uint8_t *dst;
    uint32_t msg, reserved;
};
// Padding, prefix pre-hash, staging and chain in one launch over the n_messages descriptors at d_descs (the whole
// table of a call, or the part of it that forms one dependency level): blocks / pre_states are the staging buffers
// from their block 0, init_states[8 * msg] receives a message's state after its prefix.
hipError_t launch_ingest(const IngestDesc *d_descs, size_t n_messages, uint8_t *blocks, uint32_t *init_states,
                         uint32_t *pre_states, hipStream_t stream);
hipError_t launch_fill(void *dst, size_t bytes, hipStream_t stream);
// 32-byte canonical cells -> 8-byte cells + side list of the cells wider than 64 bits (6 u64 per entry)
hipError_t launch_pack64(const void *src32, void *dst8, size_t n_cells, uint64_t stream_id, uint64_t index0,
                         void *wide, uint32_t wide_cap, uint32_t *wide_count, hipStream_t stream);

// dst[w] = the 32-byte cell at image position pos[w] (distinct-value delivery, hsw_replay.cpp)
hipError_t launch_gather32(const void *image, const uint32_t *pos, void *dst, size_t n, hipStream_t stream);

// The period of a context-image launch (library-internal: the gadget passes it next to the public argument
// structs, whose layouts are fixed): a Context's gate stream is stream_cells cells long, its image image_cells.
struct PlaceTable;
struct ContextPeriod {
    uint64_t stream_cells, image_cells;
    const PlaceTable *place = nullptr;   // shared context (HSW_GADGET_SHARED_CONTEXT): the table path; stream_cells = image_cells = 0
    uint64_t chip_ctx_extra = 0;         // bound regions: ExpandParams / VerifyParams::chip_ctx_extra
    bool chip_rows_checked = false;      // bound regions: the gadget checked the chip capacities per Context itself
};

// Shared-context placement (HSW_GADGET_SHARED_CONTEXT, library-internal): the map from gate-stream cell to image
// cell as a device-resident table of jumps -- column breaks and interludes (the caller's own cells between two
// digests) -- of any length.  Stream cell i sits at i + cum[k], k the last jump with cell[k] <= i (0 before the
// first).  The table-path kernels take it as an extra kernel argument, so ExpandParams / SmallFrames / FrameBreaks
// and every existing launch keep their 16-entry break tables.
struct PlaceTable {
    const uint64_t *cell;       // n jump cells, ascending (equal cells allowed), absolute gate-stream cells
    const uint64_t *cum;        // cum[k]: the gaps of jumps 0..k summed
    const uint64_t *lk_shift;   // expansion: per digest of the launch (blk / frame_every), cumulative caller lookup entries
    uint64_t n;
    uint64_t base;              // expansion: gate-stream cell that ExpandParams::gate (no gaps added) stands for
    // Context groups (hsw_gadget_create_contexts; 0 = one Context): the table is ONE Context's and repeats with a
    // period -- a Context's gate stream is ctx_stream cells long, its image ctx_image cells (ExpandParams /
    // VerifyParams::ctx_cells carry ctx_image to the block kernels), and it owns ctx_blocks blocks.  An expansion or
    // verify launch then covers ONE digest index of several Contexts: block b is block b % frame_every of that digest
    // in Context b / frame_every, so its inputs, next states and chip cursor are those of block
    // (b / frame_every) * ctx_blocks + b % frame_every from the launch's first, its cells go through the table at
    // base + (b % frame_every) * G and land (b / frame_every) * ctx_image further, and its lookup entries follow the
    // launch's first by (b / frame_every) * (frame_every * LOOKUP_CELLS + frame_lookups), lk_shift unused
    uint64_t ctx_blocks, ctx_stream, ctx_image;
    // Columns by pointer table (hsw_gadget_bind_columns; 0 = the periodic case above): every image column is an
    // allocation of its own, so a jump lands at an arbitrary 64-bit distance and every Context has a cum row of its
    // own, cum_stride words after the previous one's -- Context c reads cum[c * cum_stride + k].  Jump 0 is then a
    // jump at stream cell 0 whose "gap" is the distance of the Context's column 0 from PlaceTable-less `gate`
    // (modulo 2^64, in cells), so every cell has a jump at or before it, and ctx_image is 0.  The wide
    // instantiations of the table-path kernels (template parameter WIDE) are launched for such a table.
    // ctx0: the Context of the launch's block 0 (block kernels; the frame kernels take the Context from the digest)
    uint64_t cum_stride, ctx0;
    // Lookup and chip columns by pointer table (hsw_gadget_bind_column_tables; read by the wide instantiations only,
    // null = the pitch model: ExpandParams / VerifyParams::frame_lookups, chip_col_stride and chip_ctx_extra).  Rows
    // per Context, in cells modulo 2^64 like cum:
    //   lk_row[c]    what Context c's lookup column lies further from the launch's `lookup` than c lookup columns of
    //                an unbound gadget (Lp cells each) would put it -- the launch's frame_lookups steps Lp
    //   chip_row[(c * ncols + k) * 2 + f]   f = 0 dense, 1 spread: chip column k of Context c, from the launch's
    //                `chip_dense` / `chip_spread` taken as the columns' absolute row cursor0 / ncols: limb call N
    //                (absolute) sits chip_row + N / ncols - cursor0 / ncols cells from that pointer
    // A launch's first block need not be its Context's first: c counts from the pass's first Context (ctx0 + ...).
    const uint64_t *lk_row, *chip_row;
};

struct FrameDesc;   // hsw_frame.hpp
struct FrameBreaks;
struct SmallFrames;
// The small-batch kernel (hsw_small.hpp; 8-bit table only): 37 waves per block, one sub-unit program each;
// with `frames` the digest frames are written by extra waves of the same launch.
hipError_t launch_small(const ExpandParams &p, const SmallFrames *frames, int limbs, hipStream_t stream);
// The same with a placement table (whole-digest launches only): hsw_small_table_kernel.
hipError_t launch_small_table(const ExpandParams &p, const SmallFrames *frames, const PlaceTable &t, hipStream_t stream);
// Whole-digest expansion with a placement table (8-bit table only): hsw_expand_table_kernel.
hipError_t launch_expand_table(const ExpandParams &p, const PlaceTable &t, int tile, hipStream_t stream);
// d_inv_tbl: k^-1 mod p for k = 0..(largest n_blocks), 4 x u64 each, in the output representation
hipError_t launch_frames(const FrameDesc *d_descs, size_t n, const uint8_t *blocks, const uint32_t *pre_states,
                         const uint32_t *next_states, const uint64_t *d_inv_tbl, void *gate, void *lookup,
                         const FrameBreaks &brk, unsigned slices, bool montgomery, hipStream_t stream);
// The same placed by a table (brk.n = 0): hsw_frame_table_kernel.
hipError_t launch_frames_table(const FrameDesc *d_descs, size_t n, const uint8_t *blocks, const uint32_t *pre_states,
                               const uint32_t *next_states, const uint64_t *d_inv_tbl, void *gate, void *lookup,
                               const PlaceTable &t, unsigned slices, bool montgomery, hipStream_t stream);

}  // namespace hsw
#endif
