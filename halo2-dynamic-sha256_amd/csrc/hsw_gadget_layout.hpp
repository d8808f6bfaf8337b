// hsw_gadget_layout.hpp -- where the cells of a whole-digest gadget go: the map from gate-stream cell to FlexGate
// (column, row) / image cell and from the gadget's own lookup entries to d_lookup cells, and the ONE walk that
// computes it (assumption A3-iii of DESIGN.md).  Plain C++: no HIP call, nothing is allocated on a device.
#ifndef HSW_GADGET_LAYOUT_HPP
#define HSW_GADGET_LAYOUT_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/hsw.h"

namespace hsw {

// halo2-lib v0.2.x assign_region on one FlexGate (Vertical) advice column after the other: a call of `len` cells
// moves to the next column if row + len >= rows.  Every jump is recorded: break k before stream cell bc[k], leaving
// bg[k] cells of the image unused.  Image columns lie `pitch` cells apart (0: rows, the columns back to back): a
// jump to the next column also skips the pitch - rows cells between two columns.
struct ColumnWalk {
    uint64_t rows, col, row, cell;
    std::vector<uint64_t> &bc, &bg;
    uint64_t pitch = 0;
    void calls(const uint8_t *lens, size_t n);
    // one block (its call tape, G cells in all).  Its last call ends at row + G, no call ends further down: the block
    // stays in its column exactly if row + G < rows, and then the tape need not be walked
    void block(const std::vector<uint8_t> &tape, uint64_t G);
};

// Where the caller's Context stands just before a digest (hsw_gadget_set_digest_origin)
struct DigestOrigin { bool set = false; uint64_t column = 0, row = 0, lookups = 0; };

// The three kinds of layout differ by data: no jumps (max_rows = 0, the linear stream), the column breaks of a
// plain image, the breaks of ONE Context repeated every `period` stream cells (context images), or every jump of a
// shared context -- column breaks and interludes -- with the per-digest lookup tables next to them.
struct Layout {
    // Where the caller's halo2-base Context stood when it handed the region to the gadget (hsw_gadget_set_origin;
    // the reference's digest takes whatever Context it is given, lib.rs:71-76,351-360): stream cell 0 lands at
    // (origin_column, origin_row) = ctx.advice_alloc[0]; the Context may already cache its zero cell
    // (ctx.zero_cell, A4-iii: then no digest of this gadget assigns one) and may have queued
    // origin_lookups cells for the lookup-advice column (ctx.cells_to_lookup.len()).  With a column image,
    // image column k is FlexGate column origin_column + k and rows [0, origin_row) of image column 0 are
    // the caller's: never written, never delivered.
    uint64_t origin_column = 0, origin_row = 0, origin_lookups = 0;
    bool origin_zero_loaded = false;
    // FlexGate column image: `columns` advice columns of max_rows cells; stream cell i sits at i + the gaps of all
    // breaks at or before i (assumption A3-iii).  max_rows = 0: no image, the stream as it is
    uint64_t max_rows = 0, columns = 0;
    // Where the image columns lie in memory (hsw_gadget_bind_region; both 0 in a library-owned image): image column
    // k starts pitch cells after column k - 1 -- max_rows when 0 -- so every jump that changes column is pitch -
    // max_rows cells longer, and (a period) the image of Context h starts h * image_pitch cells after the first --
    // columns * column_pitch() when 0.  They change addresses (image_cell), never positions
    uint64_t pitch = 0, image_pitch = 0;
    uint64_t column_pitch() const { return pitch ? pitch : max_rows; }
    std::vector<uint64_t> break_cell, break_gap;
    std::vector<uint64_t> break_cum;                   // break_cum[k] = break_gap[0..k] summed (the search in gap_at)
    uint64_t period = 0;                               // context images with a column image: stream cells of one Context
    // shared context with a column image, per digest of the pass: its first gate-stream cell, its first entry among
    // the gadget's own lookup entries, the d_lookup cell of that entry; lookups_end: the d_lookup cells the pass needs
    std::vector<uint64_t> digest_cell0, digest_entry0, digest_lookup0;
    uint64_t lookups_end = 0;

    Layout origin() const {                            // a layout at the same origin in the same memory, nothing else
        Layout l;
        l.origin_column = origin_column; l.origin_row = origin_row; l.origin_lookups = origin_lookups; l.origin_zero_loaded = origin_zero_loaded;
        l.pitch = pitch; l.image_pitch = image_pitch;  // (the memory the image lives in does not move with the layout)
        return l;
    }
    // cells from one Context's image to the next = one image (0 without)
    uint64_t image_cells() const { return image_pitch ? image_pitch : columns * column_pitch(); }
    void set_breaks(std::vector<uint64_t> &bc, std::vector<uint64_t> &bg);   // swaps them in, rebuilds break_cum
    uint64_t gap_at(uint64_t cell) const;              // the gaps of all breaks at or before `cell`
    // (column, row) of stream cell i (context images: inside its own Context's image)
    void position(uint64_t cell, uint64_t *column, uint64_t *row) const;
    // offset of stream cell i from d_gate, in cells (origin row, jumps and, with context images, h * image_cells() included)
    uint64_t image_cell(uint64_t cell) const;
    uint64_t lookup_cell(uint64_t entry) const;        // d_lookup cell of the gadget's own lookup entry `entry`
    bool same_map(const Layout &o) const {             // (what a device copy of the jump table depends on)
        return break_cell == o.break_cell && break_gap == o.break_gap && digest_lookup0 == o.digest_lookup0 && columns == o.columns &&
               pitch == o.pitch && image_pitch == o.image_pitch;
    }
};

// The pass laid out digest by digest from out's origin in columns of `rows` cells: prologue | zero cell (the first
// time a Context needs one) | blocks | epilogue, with a jump wherever a call does not fit its column and -- decl[h]
// set -- wherever digest h's declared origin lies further on than the next free cell (an interlude; its gap may span
// columns), its lookup entries then starting at the declared queue length.  Columns lie out->pitch cells apart: every
// jump that changes column is pitch - rows cells longer, an interlude's once per column it crosses.  Fills max_rows,
// columns, the jumps, the per-digest tables and lookups_end of *out; the caller applies its own limit on breaks or columns.
// HSW_ERR_INVALID_ARG: a declaration behind the next free cell, before the origin column, with row >= rows or with a
// shorter lookup queue.
int layout_walk(const hsw_shape &shape, const size_t *sizes, size_t n, bool rc_inputs, uint64_t rows,
                const std::vector<DigestOrigin> *decl, Layout *out);

}  // namespace hsw
#endif
