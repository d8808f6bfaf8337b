// hsw_gadget_launch.hpp -- what the translation units of the gadget share beyond hsw_gadget.hpp (which tests include
// too): the engine behind the handle, hip_status, pass_repr, and the launch builder (Launch, Run, batch_runs) of the
// digest paths (hsw_gadget_digest.cpp) and of hsw_gadget_verify (hsw_gadget.cpp).  What the calls of the round over
// caller-owned device columns share beyond that is hsw_gadget_call.hpp.  Internal: not part of the boundary.
#ifndef HSW_GADGET_LAUNCH_HPP
#define HSW_GADGET_LAUNCH_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hsw_gadget.hpp"
#include "hsw_engine.hpp"
#include "hsw_kernels.h"
#include "hsw_permuted_value.hpp"

namespace hsw {

inline int hip_status(hipError_t he) { return he == hipSuccess ? HSW_OK : he == hipErrorOutOfMemory ? HSW_ERR_NOMEM : HSW_ERR_HIP; }

// the representation every batch of the pass was written in (HSW_OK), or HSW_ERR_UNSUPPORTED if they differ: what the
// calls that read the pass's cells back (hsw_gadget_lookup.cpp, hsw_gadget_permuted.cpp) decide membership in
inline int pass_repr(const Context &c, uint32_t *repr) {
    *repr = c.repr_flags;
    for (size_t i = 0; i < c.batches.size(); i++) {
        if (i == 0) *repr = c.batches[i].repr_flags;
        else if (c.batches[i].repr_flags != *repr) return HSW_ERR_UNSUPPORTED;
    }
    return HSW_OK;
}

// Where the launches of a batch write -- or, for hsw_gadget_verify, read: the generator and the verifier build
// their arguments here and nowhere else, so they agree in every kind of layout.  Made once per batch (what the
// frame launches need too), then filled in per launch.  `a`, `tbl` and `period` point at each other: not copyable.
struct Launch {
    const Context &c;
    const uint8_t *in_blocks;                 // the staging the batch's inputs are in, indexed by absolute block
    const uint32_t *in_pre;
    uint32_t flags;
    hsw_witness_args a{};
    hsw_pack_plan rel{};                      // plain image, context images: the breaks relative to the launch's first cell
    hsw_pack_plan abs{};                      // ... and as they are, for the frames (cell indices from stream cell 0)
    const hsw_pack_plan *frame_pack = nullptr;
    PlaceTable tbl{};                         // shared context: the jump table on the device (upload_place)
    PlaceWords words{};                       // ... and where its sections start
    ContextPeriod period{0, 0};
    const ContextPeriod *per = nullptr;       // context images: one Context's period; shared context: the table; else NULL

    Launch(const Context &ctx, bool inputs_in_pinned, uint32_t repr_flags)
        : c(ctx), in_blocks(inputs_in_pinned ? ctx.dp_blocks : ctx.d_blocks), in_pre(inputs_in_pinned ? ctx.dp_pre : ctx.d_pre_states),
          flags(repr_flags) {
        const Layout &l = c.layout;
        if (c.table_path()) {
            const uint64_t *d_place = static_cast<const uint64_t *>(c.d_place);
            words = c.place_words();
            tbl = PlaceTable{d_place, d_place + words.cum, d_place + words.shifts, words.n, 0};
            if (c.by_pointer) tbl.cum_stride = words.n;  // a cum row per Context
            if (c.lookup_by_table()) tbl.lk_row = d_place + words.lk_rows;
            if (c.chips_by_table()) tbl.chip_row = d_place + words.chip_rows;
            period.place = &tbl;
            per = &period;
            if (l.period) {                              // the periodic table: one Context's, every l.period stream cells
                const uint64_t image = c.by_pointer ? 0 : l.image_cells();      // (by pointer: the Context's cum row says where)
                tbl.ctx_blocks = c.blocks_per_context(); tbl.ctx_stream = l.period; tbl.ctx_image = image;
                period.stream_cells = l.period; period.image_cells = image;
            }
            period.chip_ctx_extra = c.chip_ctx_extra(); period.chip_rows_checked = c.bound;
        } else if (l.max_rows) {
            abs.n_breaks = (uint32_t)l.break_cell.size();
            for (size_t k = 0; k < abs.n_breaks; k++) { abs.break_cell[k] = l.break_cell[k]; abs.break_gap[k] = l.break_gap[k]; }
            frame_pack = &abs;
            if (l.period) { period = ContextPeriod{l.period, l.image_cells()}; per = &period; }
            period.chip_ctx_extra = c.chip_ctx_extra(); period.chip_rows_checked = c.bound;
        }
    }
    Launch(const Launch &) = delete;

    // n_blocks blocks from absolute block first_block on.  The chip cursor is the running num_limb_sum; column buffers
    // are addressed from absolute row 0 (cursor origin of the context).  Block-stream contexts: that is all
    void blocks(size_t first_block, size_t n_blocks) {
        const size_t cb = hsw_cell_bytes(flags);
        a = hsw_witness_args{};
        a.d_blocks = in_blocks + 64 * first_block; a.d_pre_states = in_pre + 8 * first_block; a.n_blocks = n_blocks;
        a.spread_cursor0 = (uint64_t)first_block * c.shape.limb_calls_per_block;
        // (a bound region: the chip rows of the launch's first Context, where the caller keeps that Context's)
        const size_t row_shift = (size_t)c.chip_launch_cell(a.spread_cursor0 - a.spread_cursor0 % c.shape.num_advice_columns);
        a.d_gate = static_cast<uint8_t *>(c.d_gate) + first_block * (size_t)c.shape.gate_cells_per_block * cb;
        a.d_chip_dense = static_cast<uint8_t *>(c.d_chip_dense) + row_shift * cb;
        a.d_chip_spread = static_cast<uint8_t *>(c.d_chip_spread) + row_shift * cb;
        a.chip_col_stride = c.chip_col_stride;
        a.d_next_states = c.d_next_states + 8 * first_block;
        a.flags = flags;
    }

    // Whole-digest contexts: the block streams of n_digests equally sized digests (shape fs) as ONE launch -- the
    // kernel skips the frame between two of them.  digest0: the first one's index in the pass, r0: its cells
    void run(size_t digest0, const AssignedHashResult &r0, size_t first_block, size_t n_digests, const hsw_frame_shape &fs) {
        blocks(first_block, (size_t)fs.n_blocks * n_digests);
        const size_t cb = hsw_cell_bytes(flags);
        const Layout &l = c.layout;
        // (context images: the run's first block in ITS Context's image; the breaks are that Context's)
        const uint64_t ctx0 = l.period ? r0.block_cell / l.period : 0, local = r0.block_cell - ctx0 * l.period;
        a.d_gate = static_cast<uint8_t *>(c.gate_stream()) + (size_t)((c.by_pointer ? 0 : ctx0 * l.image_cells()) + local) * cb;
        a.d_lookup = cell_ptr(c.d_lookup, r0.block_lookup + c.lookup_extra(ctx0), cb);   // (by table: the Context's own column)
        a.frame_every = fs.n_blocks;
        // between the block streams of two digests: one epilogue, the next prologue -- and the next Context's zero cell
        // when every digest is a Context of its own, and (context images) its caller-owned lookup cells
        a.frame_cells = fs.epilogue_cells + fs.prologue_cells + (c.independent && !l.origin_zero_loaded ? 1u : 0u);
        a.frame_lookups = fs.epilogue_lookups + fs.prologue_lookups + (c.context_images ? l.origin_lookups + (c.lookup_pitch() - c.ctx_lookups()) : 0u);
        // (a Context group: the "digests" of the run are the SAME digest index of consecutive Contexts, whose lookup
        //  columns lie ctx_lookups() apart and whose blocks ctx_blocks apart -- PlaceTable::ctx_blocks)
        if (c.group_m) a.frame_lookups = c.lookup_pitch() - (uint64_t)fs.n_blocks * c.shape.lookup_cells_per_block;
        if (period.place) {                              // the run's first block cell, its digests' lookup shifts
            tbl.base = local;
            tbl.lk_shift = tbl.cell + words.shifts + (c.group_m ? digest0 % c.group_m : c.context_images ? 0 : digest0);
            if (c.by_pointer && l.period) {
                // a pointer table's Contexts: block b of the launch is block b % frame_every of Context ctx0 + b / frame_every,
                // whose cells go through ITS cum row from the Context's own stream cell on -- no image offset (ctx_cells = 0),
                // and stepping a Context steps the stream back by the Context's blocks: frame_cells = -(frame_every * G), mod 2^64
                tbl.ctx0 = ctx0;
                a.frame_cells = 0 - (uint64_t)fs.n_blocks * c.shape.gate_cells_per_block;
            }
        } else if (frame_pack) {                         // breaks before the launch's first cell are pure offsets
            rel.n_breaks = abs.n_breaks;
            for (uint32_t k = 0; k < rel.n_breaks; k++) {
                rel.break_cell[k] = abs.break_cell[k] > local ? abs.break_cell[k] - local : 0;
                rel.break_gap[k] = abs.break_gap[k];
            }
            a.pack = &rel;
        }
    }
};

// The expansion (and verify) launches of a batch of n digests from digest d0 of the pass on, as runs of `count` digests
// `step` apart from batch index `first`: neighbours of equal size (blocks_of(i): digest i of the batch) -- or, in a
// Context group, digest index j of every Context the batch holds it of: M launches, not K * M
struct Run { size_t first, count, step; };
template <class BlocksOf>
std::vector<Run> batch_runs(const Context &c, size_t d0, size_t n, BlocksOf blocks_of) {
    std::vector<Run> runs;
    if (c.group_m) {
        const size_t M = c.group_m;
        for (size_t j = 0; j < M; j++) {
            const size_t c_lo = d0 > j ? (d0 - j + M - 1) / M : 0;      // the first Context whose digest j the batch holds
            const size_t first = c_lo * M + j;
            if (first >= d0 + n) continue;
            runs.push_back(Run{first - d0, (d0 + n - first + M - 1) / M, M});
        }
        return runs;
    }
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        while (j < n && blocks_of(j) == blocks_of(i)) j++;
        runs.push_back(Run{i, j - i, 1});
        i = j;
    }
    return runs;
}

}  // namespace hsw
#endif
