// hsw_open.h -- launch interface of the evaluation and the opening of device columns (hsw_open.hip; hsw_gadget_evaluate
// and hsw_gadget_open in hsw_gadget_open.cpp are its callers; hsw_gadget_shplonk.cpp takes launch_open_scan as it is).
#ifndef HSW_OPEN_H
#define HSW_OPEN_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_open_value.hpp"

namespace hsw {

// One column (cells of two uint4 each, 16-byte aligned)
struct OpenColumn {
    const uint4 *cells;            // rows cells are read, the rest count as 0
    uint32_t rows;
    uint32_t item_first, n_items;  // evaluate: the column's (column, point) items; open: not used
    uint32_t status;               // evaluate: its status word
};

// One group of hsw_gadget_open
struct OpenGroup {
    uint32_t first, m;             // its columns: group_cols[first .. first + m)
    uint32_t src_rows, reserved_;  // the rows of src that are read: rows, or the column's own for m = 1
    PFe v;                         // the challenge, Montgomery form
    const uint4 *src;              // what the write launch reads: c in scratch, or for m = 1 the column itself
    uint4 *c;                      // scratch, rows cells (m = 1: NULL, nothing is stored)
    uint4 *seeds;                  // scratch, geometry.seeds cells: E of every thread
    uint4 *q;                      // the caller's quotient, rows cells
};

// What the scan launch walks: a group, or a (column, point) of evaluate.  Item i owns tiles [i n_tiles, (i + 1) n_tiles)
// of `tiles` and cell i of `evals`
struct OpenItem { uint32_t point, status; };

struct OpenParams {
    OpenGeometry geo;
    const OpenColumn *cols;
    const uint32_t *group_cols;
    const OpenGroup *groups;       // one per blockIdx.y of the open launches, from `base` on
    const OpenItem *items;
    const OpenPoint *points;
    uint4 *tiles;                  // scratch: n_tiles cells per item of this batch
    uint4 *evals;                  // one cell per item of the call
    uint32_t *status;              // zeroed by the caller
    uint32_t base;                 // the first group (open) or column (evaluate) of this batch
    uint32_t item_base;            // the first item of this batch: `tiles` starts with its tiles (open: base)
};

// tiles and write: n groups from p.base on; evaluate_tiles: n columns from p.base on; scan: n items from p.item_base on
hipError_t launch_open_tiles(const OpenParams &p, uint32_t n, hipStream_t stream);
hipError_t launch_open_write(const OpenParams &p, uint32_t n, hipStream_t stream);
hipError_t launch_evaluate_tiles(const OpenParams &p, uint32_t n, hipStream_t stream);
hipError_t launch_open_scan(const OpenParams &p, uint32_t n, hipStream_t stream);

}  // namespace hsw
#endif
