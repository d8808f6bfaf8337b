// hsw_open_value.hpp -- the rules of evaluating and opening device columns (hsw_gadget_evaluate, hsw_gadget_open,
// include/hsw.h).
//
//   c[j] = sum_{i<m} v^(m-1-i) a_i[j]     the fold acc v + a over a group's columns, the first column the highest power
//   s[j] = sum_{i>=j} c[i] z^(i-j)        the suffix Horner sums:  s[j] = c[j] + z s[j+1],  s[rows] = 0
//   c(z) = s[0],   q[j] = s[j+1]          Kate division: c(X) - c(z) = (X - z) q(X), and q never reads c[0]
// Evaluation is the same recurrence with m = 1 and only s[0] kept.  The recurrence is a suffix scan of the affine maps
// x -> c[j] + z x, which all have the SAME multiplier, so a block of B consecutive rows composes to x -> S + z^B x with
// S its own Horner sum: a scan step costs one multiply by a constant power of z, staged by the host.
// The geometry: a TILE of tile_rows rows per workgroup, walked from its last SWEEP of `active` threads x OPEN_ROWS rows
// to its first; every thread owns OPEN_ROWS consecutive rows.
//   tiles   thread: fold, Horner over its rows (L_t).  Workgroup: inclusive suffix scan X_t = sum_{u>=t} L_u z^(R(u-t))
//           with the step multipliers z^(R 2^k).  E_t = X_{t+1} (what lies behind the thread inside its sweep) goes to
//           scratch, one cell per thread; the sweeps chain by carry = X_0 + z^(R active) carry; the tile's sum to scratch.
//   scan    per (group) or (column, point): every thread takes a chunk of tiles, Horner with z^tile_rows, a workgroup
//           scan with z^(tile_rows chunk 2^k); every tile's sum is replaced by its carry-in s[(tile + 1) tile_rows], and
//           s[0] = c(z) falls out of thread 0.
//   write   thread: seed = E_t + z^(R(active-1-t)) carry = s[row0 + R], then q[j] = s[j+1], s[j] = c[j] + z s[j+1] down
//           its rows: one multiply per row; the sweeps chain through thread 0's s[row0].
// Cells come in the representation of the pass (x, or x R); every constant -- z, v and the powers -- is held in
// Montgomery form, so fr_mont_mul(cell, constant) is the cell times the constant IN THE REPRESENTATION OF THE CELL, and
// additions are linear: the same code is exact for both forms.
// Host- and device-callable: hsw_open.hip is built from these, hsw_gadget_open.cpp stages with them,
// tests/cpp/open_value_check.cpp runs the launches thread for thread on the CPU against the plain recurrence.
#ifndef HSW_OPEN_VALUE_HPP
#define HSW_OPEN_VALUE_HPP
#include "hsw_fr_mul.hpp"

namespace hsw {

enum : uint32_t {
    OPEN_THREADS = 256,
    OPEN_THREADS_LOG = 8,
    OPEN_ROWS = 8,                   // consecutive rows of a thread: 256 contiguous bytes per column
    OPEN_SWEEP_ROWS = OPEN_THREADS * OPEN_ROWS,
    OPEN_MIN_TILE_ROWS = 256,        // HSW_OPEN_MIN_TILE_ROWS
    OPEN_MAX_TILE_LOG = 20,
    OPEN_DEFAULT_TILE_ROWS = OPEN_SWEEP_ROWS,
    OPEN_MAX_ROWS_LOG = 28,
    OPEN_CELL_NOT_BELOW_P = 4u,      // HSW_OPEN_CELL_NOT_BELOW_P
};

// What a call's launches share
struct OpenGeometry {
    uint32_t rows, tile_rows, n_tiles;
    uint32_t active, sweeps;         // threads that own rows, and sweeps of active * OPEN_ROWS rows per tile
    uint32_t chunk;                  // tiles per thread of the scan
    uint32_t seeds;                  // threads that own a row below `rows`: the cells of E
    uint32_t reserved_;
};

// The powers of one point, in Montgomery form
struct OpenPoint {
    PFe z;
    PFe zt;                          // z^tile_rows
    PFe zc[OPEN_THREADS_LOG];        // z^(tile_rows chunk 2^k): the steps of the scan launch
    PFe zr[OPEN_THREADS + 1];        // z^(OPEN_ROWS k): the steps of a workgroup (k = 2^s), the seeds, the sweeps (k = active)
};

HSW_PHD bool open_tile_rows_valid(uint32_t tile_rows) {
    return tile_rows == 0 || (tile_rows >= OPEN_MIN_TILE_ROWS && tile_rows <= (1u << OPEN_MAX_TILE_LOG) && (tile_rows & (tile_rows - 1)) == 0);
}
// false: rows or tile_rows out of range.  tile_rows 0 is OPEN_DEFAULT_TILE_ROWS
HSW_PHD bool open_geometry(uint64_t rows, uint32_t tile_rows, OpenGeometry &g) {
    if (rows < 1 || rows > (1ull << OPEN_MAX_ROWS_LOG) || !open_tile_rows_valid(tile_rows)) return false;
    g.rows = (uint32_t)rows;
    g.tile_rows = tile_rows ? tile_rows : (uint32_t)OPEN_DEFAULT_TILE_ROWS;
    g.n_tiles = (g.rows + g.tile_rows - 1) / g.tile_rows;
    g.active = g.tile_rows >= OPEN_SWEEP_ROWS ? (uint32_t)OPEN_THREADS : g.tile_rows / OPEN_ROWS;
    g.sweeps = g.tile_rows / (g.active * OPEN_ROWS);
    g.chunk = (g.n_tiles + OPEN_THREADS - 1) / OPEN_THREADS;
    g.seeds = (g.rows + OPEN_ROWS - 1) / OPEN_ROWS;
    g.reserved_ = 0;
    return true;
}
// the first row of thread t in a sweep of a tile
HSW_PHD uint32_t open_row0(const OpenGeometry &g, uint32_t tile, uint32_t sweep, uint32_t t) {
    return tile * g.tile_rows + (sweep * g.active + t) * OPEN_ROWS;
}
// the tiles [lo, hi) of thread t of the scan
HSW_PHD void open_chunk(const OpenGeometry &g, uint32_t t, uint32_t &lo, uint32_t &hi) {
    lo = t * g.chunk < g.n_tiles ? t * g.chunk : g.n_tiles;
    hi = g.n_tiles - lo < g.chunk ? g.n_tiles : lo + g.chunk;
}

// a stored constant (below p) in Montgomery form
HSW_PHD PFe open_to_mont(const PFe &stored, bool montgomery) { return montgomery ? stored : fr_to_mont(stored); }
// base^e by square and multiply, Montgomery form
HSW_PHD PFe open_power(const PFe &base_mont, uint64_t e) {
    PFe r = fr_one_mont(), b = base_mont;
    for (; e; e >>= 1) {
        if (e & 1u) r = fr_mont_mul(r, b);
        b = fr_mont_mul(b, b);
    }
    return r;
}
HSW_PHD void open_stage_point(const PFe &z_mont, const OpenGeometry &g, OpenPoint &pt) {
    pt.z = z_mont;
    pt.zt = open_power(z_mont, g.tile_rows);
    pt.zc[0] = open_power(pt.zt, g.chunk);
    for (uint32_t k = 1; k < OPEN_THREADS_LOG; k++) pt.zc[k] = fr_mont_mul(pt.zc[k - 1], pt.zc[k - 1]);
    pt.zr[0] = fr_one_mont();
    pt.zr[1] = open_power(z_mont, OPEN_ROWS);
    for (uint32_t k = 2; k <= OPEN_THREADS; k++) pt.zr[k] = fr_mont_mul(pt.zr[k - 1], pt.zr[1]);
}

// acc v + a: one more column of a group
HSW_PHD PFe open_fold(const PFe &acc, const PFe &v_mont, const PFe &a) { return fr_add(fr_mont_mul(acc, v_mont), a); }
// c + z s: one row of the recurrence, and one step of a scan (mine + power * behind)
HSW_PHD PFe open_step(const PFe &c, const PFe &z_mont, const PFe &s) { return fr_add(c, fr_mont_mul(z_mont, s)); }
// sum_k c[k] z^k over a thread's rows: OPEN_ROWS - 1 multiplies
HSW_PHD PFe open_horner(const PFe *c, const PFe &z_mont) {
    static_assert(OPEN_ROWS == 8, "one step per row below, written out so that c stays in registers");
    PFe s = open_step(c[6], z_mont, c[7]);
    s = open_step(c[5], z_mont, s); s = open_step(c[4], z_mont, s); s = open_step(c[3], z_mont, s);
    s = open_step(c[2], z_mont, s); s = open_step(c[1], z_mont, s);
    return open_step(c[0], z_mont, s);
}

}  // namespace hsw
#endif
