// hsw_open.hip -- device columns evaluated at points and opened: the fold of a group's columns with v, c(z), and the
// quotient (c(X) - c(z)) / (X - z), written on the device.
//
// hsw_gadget_evaluate and hsw_gadget_open (hsw_gadget_open.cpp).  Both are the suffix Horner recurrence s[j] = c[j] +
// z s[j+1] of hsw_open_value.hpp, in three launches on the stream and nothing read by the host in between:
//   tiles   a workgroup per (group or column, tile of tile_rows rows), a sweep of 2048 rows at a time from the tile's
//           last to its first: every thread loads OPEN_ROWS consecutive rows of each column (256 contiguous bytes per
//           column and lane, 16-byte loads), checks each stored cell against p, folds the columns with v (m - 1
//           multiplies per row, none for m = 1) and runs Horner in z over its rows; a workgroup suffix scan whose step
//           multipliers are the staged constants z^(8 2^k) combines the threads.  What lies behind each thread (one cell
//           per thread), the folded column c (m > 1 only: for m = 1 the column itself is c) and the tile's sum go to
//           scratch.  evaluate holds a column's rows in registers and repeats Horner and scan per point of the column.
//   scan    a workgroup per group or (column, point): every thread runs Horner with z^tile_rows over a chunk of tiles,
//           a workgroup scan with z^(tile_rows chunk 2^k); every tile's sum becomes its carry-in, thread 0 leaves c(z).
//   write   (open) tiles again: seed = E_t + z^(8 (active - 1 - t)) carry, then q[j] = s[j+1], s[j] = c[j] + z s[j+1]
//           down the thread's rows, two 16-byte stores per cell, one multiply per row.  A refused group stores nothing.
// Field elements travel through LDS limb-major (sh[limb][thread]): 4-byte accesses at stride 1, no bank conflict
// (hsw_open_device.hpp: the cell, LDS and scan helpers, shared with hsw_shplonk.hip).
// Vector loads, vector stores and vector atomics only.
#include "hsw_open.h"
#include "hsw_open_device.hpp"

namespace hsw {

typedef unsigned int u32;

namespace {

// q[row] = s[row+1], then s[row] = c[row] + z s[row+1]; rows at and beyond `rows` are no rows (there s is 0)
__device__ __forceinline__ void write_row(uint4 *q, u32 rows, u32 row, const PFe &c, const PFe &z, PFe &s) {
    if (row >= rows) return;
    store_cell(q, row, s);
    s = open_step(c, z, s);
}

}  // namespace

__global__ __launch_bounds__(OPEN_THREADS) void hsw_open_tiles_kernel(OpenParams p) {
    __shared__ u32 sh[8 * OPEN_THREADS];
    const u32 gi = p.base + blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const OpenGeometry geo = p.geo;
    const OpenGroup *grp = p.groups + gi;
    const OpenPoint *pt = p.points + p.items[gi].point;
    const u32 first = grp->first, m = grp->m;
    uint4 *c_out = grp->c, *seeds = grp->seeds;
    const PFe z = pt->z, v = grp->v;
    bool ok = true;
    PFe carry = fr_zero();                                            // (thread 0's: the sweeps behind this one)
    for (u32 sweep = geo.sweeps; sweep-- > 0;) {
        const u32 row0 = open_row0(geo, tile, sweep, t);
        const bool mine = t < geo.active && row0 < geo.rows;
        PFe L = fr_zero();
        if (mine) {
            PFe c[OPEN_ROWS];
            for (u32 i = 0; i < m; i++) {
                const OpenColumn *col = p.cols + p.group_cols[first + i];
                PFe a[OPEN_ROWS];
                ok = load_rows(col->cells, col->rows, row0, a) && ok;
#pragma unroll
                for (u32 k = 0; k < OPEN_ROWS; k++) c[k] = i ? open_fold(c[k], v, a[k]) : a[k];
            }
            if (c_out) {
#pragma unroll
                for (u32 k = 0; k < OPEN_ROWS; k++)
                    if (row0 + k < geo.rows) store_cell(c_out, row0 + k, c[k]);
            }
            L = open_horner(c, z);
        }
        suffix_scan<false>(sh, pt->zr, geo.active, L);
        if (mine) store_cell(seeds, row0 / OPEN_ROWS, t + 1 < geo.active ? lds_get(sh, t + 1) : fr_zero());
        if (t == 0) carry = sweep + 1 == geo.sweeps ? lds_get(sh, 0) : open_step(lds_get(sh, 0), pt->zr[geo.active], carry);
        __syncthreads();
    }
    if (!ok) atomicOr(&p.status[p.items[gi].status], OPEN_CELL_NOT_BELOW_P);
    if (t == 0) store_cell(p.tiles, (size_t)(gi - p.base) * geo.n_tiles + tile, carry);
}

__global__ __launch_bounds__(OPEN_THREADS) void hsw_evaluate_tiles_kernel(OpenParams p) {
    __shared__ u32 sh[8 * OPEN_THREADS];
    const u32 ci = p.base + blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const OpenGeometry geo = p.geo;
    const OpenColumn *col = p.cols + ci;
    const u32 item_first = col->item_first, n_items = col->n_items;
    bool ok = true;
    for (u32 sweep = geo.sweeps; sweep-- > 0;) {
        const u32 row0 = open_row0(geo, tile, sweep, t);
        const bool mine = t < geo.active && row0 < geo.rows;
        PFe a[OPEN_ROWS];
        if (mine) ok = load_rows(col->cells, col->rows, row0, a) && ok;
        for (u32 i = 0; i < n_items; i++) {                           // one pass over the column serves all its points
            const u32 item = item_first + i;
            const OpenPoint *pt = p.points + p.items[item].point;
            PFe L = fr_zero();
            if (mine) L = open_horner(a, pt->z);
            suffix_scan<false>(sh, pt->zr, geo.active, L);
            if (t == 0) {                                             // the sweeps chain through the tile's own cell
                const size_t at = (size_t)(item - p.item_base) * geo.n_tiles + tile;
                PFe x = lds_get(sh, 0);
                if (sweep + 1 != geo.sweeps) x = open_step(x, pt->zr[geo.active], load_cell(p.tiles, at));
                store_cell(p.tiles, at, x);
            }
            __syncthreads();
        }
    }
    if (!ok) atomicOr(&p.status[col->status], OPEN_CELL_NOT_BELOW_P);
}

__global__ __launch_bounds__(OPEN_THREADS) void hsw_open_scan_kernel(OpenParams p) {
    __shared__ u32 sh[8 * OPEN_THREADS];
    const u32 item = p.item_base + blockIdx.x, t = threadIdx.x;
    const OpenGeometry geo = p.geo;
    const OpenPoint *pt = p.points + p.items[item].point;
    uint4 *tiles = p.tiles + 2 * (size_t)blockIdx.x * geo.n_tiles;
    u32 lo, hi;
    open_chunk(geo, t, lo, hi);
    const PFe zt = pt->zt;
    PFe L = fr_zero();
    for (u32 k = hi; k-- > lo;) L = open_step(load_cell(tiles, k), zt, L);
    suffix_scan<true>(sh, pt->zc, OPEN_THREADS, L);
    PFe run = t + 1 < OPEN_THREADS ? lds_get(sh, t + 1) : fr_zero();  // what lies behind the chunk
    for (u32 k = hi; k-- > lo;) {                                     // every tile's carry-in, in place of its sum
        const PFe own = load_cell(tiles, k);
        store_cell(tiles, k, run);
        run = open_step(own, zt, run);
    }
    if (t == 0) store_cell(p.evals, item, run);                       // s[0] = c(z)
}

__global__ __launch_bounds__(OPEN_THREADS) void hsw_open_write_kernel(OpenParams p) {
    __shared__ u32 shc[8];
    const u32 gi = p.base + blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    if (p.status[p.items[gi].status] & OPEN_CELL_NOT_BELOW_P) return; // (workgroup-uniform: decided before this launch)
    const OpenGeometry geo = p.geo;
    const OpenGroup *grp = p.groups + gi;
    const OpenPoint *pt = p.points + p.items[gi].point;
    const uint4 *src = grp->src, *seeds = grp->seeds;
    uint4 *q = grp->q;
    const u32 src_rows = grp->src_rows;
    const PFe z = pt->z;
    PFe carry = load_cell(p.tiles, (size_t)(gi - p.base) * geo.n_tiles + tile);   // s[(tile + 1) tile_rows]
    for (u32 sweep = geo.sweeps; sweep-- > 0;) {
        const u32 row0 = open_row0(geo, tile, sweep, t);
        const bool mine = t < geo.active && row0 < geo.rows;
        PFe s = fr_zero();
        if (mine) {
            PFe c[OPEN_ROWS];
            (void)load_rows(src, src_rows, row0, c);
            s = open_step(load_cell(seeds, row0 / OPEN_ROWS), pt->zr[geo.active - 1 - t], carry);   // s[row0 + OPEN_ROWS]
            static_assert(OPEN_ROWS == 8, "one call per row below");
            write_row(q, geo.rows, row0 + 7, c[7], z, s); write_row(q, geo.rows, row0 + 6, c[6], z, s);
            write_row(q, geo.rows, row0 + 5, c[5], z, s); write_row(q, geo.rows, row0 + 4, c[4], z, s);
            write_row(q, geo.rows, row0 + 3, c[3], z, s); write_row(q, geo.rows, row0 + 2, c[2], z, s);
            write_row(q, geo.rows, row0 + 1, c[1], z, s); write_row(q, geo.rows, row0, c[0], z, s);
        }
        if (sweep) {                                                  // thread 0's s[row0] is the carry of the sweep before
            if (t == 0)
                for (int j = 0; j < 8; j++) shc[j] = s.l[j];
            __syncthreads();
            for (int j = 0; j < 8; j++) carry.l[j] = shc[j];
            __syncthreads();
        }
    }
}

hipError_t launch_open_tiles(const OpenParams &p, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_open_tiles_kernel, dim3(p.geo.n_tiles, n), dim3(OPEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_evaluate_tiles(const OpenParams &p, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_evaluate_tiles_kernel, dim3(p.geo.n_tiles, n), dim3(OPEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_open_scan(const OpenParams &p, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_open_scan_kernel, dim3(n), dim3(OPEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_open_write(const OpenParams &p, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_open_write_kernel, dim3(p.geo.n_tiles, n), dim3(OPEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
