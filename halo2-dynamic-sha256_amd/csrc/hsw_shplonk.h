// hsw_shplonk.h -- launch interface of SHPLONK's multi-point opening of device columns (hsw_shplonk.hip;
// hsw_gadget_shplonk_quotient and hsw_gadget_shplonk_open in hsw_gadget_shplonk.cpp are its only callers).  The scan
// between the two launches declared here is launch_open_scan of hsw_open.h as it is, over the (set, point) items.
#ifndef HSW_SHPLONK_H
#define HSW_SHPLONK_H

#include "hsw_open.h"
#include "hsw_shplonk_value.hpp"

namespace hsw {

// One rotation set (open: the one set of every column and h)
struct ShplonkSet {
    uint32_t first, m;             // its columns set_cols[first .. first + m), their weights col_weights[first .. first + m)
    uint32_t item_first, n_items;  // its (set, point) items
    uint32_t src_rows, reserved_;  // the rows of src that are read: rows, or the column's own for m = 1
    const uint4 *src;              // what the write launch reads: c in scratch, or for m = 1 the column itself
    uint4 *c;                      // scratch, rows cells (m = 1: NULL, nothing is stored)
};

struct ShplonkParams {
    OpenGeometry geo;
    const OpenColumn *cols;        // cells and rows only
    const uint32_t *set_cols;
    const PFe *col_weights;        // Montgomery form; a set's first is 1 and is not read
    const ShplonkSet *sets;
    const OpenItem *items;         // item i: its point; owns tiles [i n_tiles, (i + 1) n_tiles) and seeds [i geo.seeds, ..)
    const PFe *item_weights;       // W, Montgomery form (unit: not read)
    const OpenPoint *points;
    uint4 *tiles;                  // scratch: n_tiles cells per item
    uint4 *seeds;                  // scratch: geo.seeds cells per item
    uint4 *out;                    // the caller's h or w, rows cells
    uint32_t *status;              // ONE word, zeroed by the caller
    uint32_t n_sets;
    uint32_t unit;                 // every W is 1 (open)
};

hipError_t launch_shplonk_tiles(const ShplonkParams &p, hipStream_t stream);
hipError_t launch_shplonk_write(const ShplonkParams &p, hipStream_t stream);

}  // namespace hsw
#endif
