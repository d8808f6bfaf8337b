// hsw_shplonk.hip -- SHPLONK's multi-point opening of device columns: the fold of every rotation set with its staged
// weights, one suffix Horner scan per (set, point) item, and the weighted sum of the items' scans, written on the device.
//
// hsw_gadget_shplonk_quotient and hsw_gadget_shplonk_open (hsw_gadget_shplonk.cpp).  Both are the recurrence s[j] = c[j] +
// z s[j+1] of hsw_open_value.hpp per item and the rules of hsw_shplonk_value.hpp, in three launches on the stream and
// nothing read by the host in between:
//   tiles   a workgroup per (set, tile of tile_rows rows), a sweep of 2048 rows at a time from the tile's last to its
//           first: every thread loads OPEN_ROWS consecutive rows of each column of the set, checks each stored cell
//           against p and forms c = sum_k w_k a_k (m - 1 multiplies per row; the first weight is 1).  c goes to scratch
//           for m >= 2; for m = 1 the column itself is c.  Then, with c[8] kept in registers, per point of the set:
//           Horner in z over the thread's rows and the workgroup suffix scan, as hsw_evaluate_tiles_kernel does; what
//           lies behind each thread (one cell per thread and item) and the tile's sum per item go to scratch.
//   scan    hsw_open_scan_kernel as it is, a workgroup per item: every tile's sum becomes its carry-in.
//   write   a workgroup per tile.  Per set it loads c once, per point of the set seed = E_t + z^(8 (active - 1 - t))
//           carry, then the recurrence down the thread's rows, acc[j] += W s[j+1] (W = 1: a plain add).  ONE store of acc
//           per cell of the output, which is never read.  With more than one sweep per tile an item's carry chains
//           through its own tile cell in scratch.  Any status bit set: nothing is stored.
// The cell, LDS and scan helpers are hsw_open_device.hpp's, shared with hsw_open.hip.
// Vector loads, vector stores and vector atomics only; every thread reaches every barrier (the loops and the early
// return of the write launch are workgroup-uniform).
#include "hsw_open_device.hpp"
#include "hsw_shplonk.h"

namespace hsw {

typedef unsigned int u32;

namespace {

// acc[row] += W s[row+1] (unit: += s[row+1]), then s[row] = c[row] + z s[row+1]; rows at and beyond `rows` are no rows
template <bool UNIT>
__device__ __forceinline__ void gather_row(u32 rows, u32 row, const PFe &c, const PFe &z, const PFe &W, PFe &s, PFe &acc) {
    if (row >= rows) return;
    acc = UNIT ? fr_add(acc, s) : shplonk_gather(acc, W, s);
    s = open_step(c, z, s);
}

template <bool UNIT>
__device__ __forceinline__ void write_body(const ShplonkParams &p) {
    const u32 tile = blockIdx.x, t = threadIdx.x;
    const OpenGeometry geo = p.geo;
    const bool chained = geo.sweeps > 1;                              // (workgroup-uniform)
    for (u32 sweep = geo.sweeps; sweep-- > 0;) {
        const u32 row0 = open_row0(geo, tile, sweep, t);
        const bool mine = t < geo.active && row0 < geo.rows;
        PFe acc[OPEN_ROWS];
#pragma unroll
        for (u32 k = 0; k < OPEN_ROWS; k++) acc[k] = fr_zero();
        for (u32 si = 0; si < p.n_sets; si++) {
            const ShplonkSet *set = p.sets + si;
            const u32 item_first = set->item_first, n_items = set->n_items;
            PFe c[OPEN_ROWS];
            if (mine) (void)load_rows(set->src, set->src_rows, row0, c);
            for (u32 i = 0; i < n_items; i++) {
                const u32 item = item_first + i;
                const OpenPoint *pt = p.points + p.items[item].point;
                const size_t at = (size_t)item * geo.n_tiles + tile;
                PFe s = fr_zero();
                if (mine) {
                    const PFe z = pt->z;
                    PFe W = fr_zero();
                    if (!UNIT) W = p.item_weights[item];
                    // s[row0 + OPEN_ROWS]: the carry is s[(tile + 1) tile_rows], or what the sweep before left
                    s = open_step(load_cell(p.seeds, (size_t)item * geo.seeds + row0 / OPEN_ROWS), pt->zr[geo.active - 1 - t], load_cell(p.tiles, at));
                    static_assert(OPEN_ROWS == 8, "one call per row below");
                    gather_row<UNIT>(geo.rows, row0 + 7, c[7], z, W, s, acc[7]); gather_row<UNIT>(geo.rows, row0 + 6, c[6], z, W, s, acc[6]);
                    gather_row<UNIT>(geo.rows, row0 + 5, c[5], z, W, s, acc[5]); gather_row<UNIT>(geo.rows, row0 + 4, c[4], z, W, s, acc[4]);
                    gather_row<UNIT>(geo.rows, row0 + 3, c[3], z, W, s, acc[3]); gather_row<UNIT>(geo.rows, row0 + 2, c[2], z, W, s, acc[2]);
                    gather_row<UNIT>(geo.rows, row0 + 1, c[1], z, W, s, acc[1]); gather_row<UNIT>(geo.rows, row0, c[0], z, W, s, acc[0]);
                }
                if (chained) {                                        // thread 0's s[row0] is the item's carry of the sweep before
                    __syncthreads();                                  // (every thread has read the cell)
                    if (t == 0) store_cell(p.tiles, at, s);
                }
            }
        }
        if (mine) {
#pragma unroll
            for (u32 k = 0; k < OPEN_ROWS; k++)
                if (row0 + k < geo.rows) store_cell(p.out, row0 + k, acc[k]);
        }
        if (chained) __syncthreads();                                 // (thread 0's cells, before the sweep before reads them)
    }
}

}  // namespace

// (two waves per SIMD: left to itself the compiler takes 286 registers for one; at two it needs 249 and spills nothing)
__global__ __launch_bounds__(OPEN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void hsw_shplonk_tiles_kernel(ShplonkParams p) {
    __shared__ u32 sh[8 * OPEN_THREADS];
    const u32 si = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const OpenGeometry geo = p.geo;
    const ShplonkSet *set = p.sets + si;
    const u32 first = set->first, m = set->m, item_first = set->item_first, n_items = set->n_items;
    uint4 *c_out = set->c;
    bool ok = true;
    for (u32 sweep = geo.sweeps; sweep-- > 0;) {
        const u32 row0 = open_row0(geo, tile, sweep, t);
        const bool mine = t < geo.active && row0 < geo.rows;
        PFe c[OPEN_ROWS];
        if (mine) {
            const OpenColumn *col0 = p.cols + p.set_cols[first];      // (its weight is 1)
            ok = load_rows(col0->cells, col0->rows, row0, c) && ok;
            for (u32 i = 1; i < m; i++) {
                const OpenColumn *col = p.cols + p.set_cols[first + i];
                const PFe w = p.col_weights[first + i];
                PFe a[OPEN_ROWS];
                ok = load_rows(col->cells, col->rows, row0, a) && ok;
                static_assert(OPEN_ROWS == 8, "one fold per row below, written out so that c stays in registers");
                c[0] = shplonk_fold(c[0], w, a[0]); c[1] = shplonk_fold(c[1], w, a[1]);
                c[2] = shplonk_fold(c[2], w, a[2]); c[3] = shplonk_fold(c[3], w, a[3]);
                c[4] = shplonk_fold(c[4], w, a[4]); c[5] = shplonk_fold(c[5], w, a[5]);
                c[6] = shplonk_fold(c[6], w, a[6]); c[7] = shplonk_fold(c[7], w, a[7]);
            }
            if (c_out) {
#pragma unroll
                for (u32 k = 0; k < OPEN_ROWS; k++)
                    if (row0 + k < geo.rows) store_cell(c_out, row0 + k, c[k]);
            }
        }
        for (u32 i = 0; i < n_items; i++) {                           // one pass over the set's columns serves all its points
            const u32 item = item_first + i;
            const OpenPoint *pt = p.points + p.items[item].point;
            PFe L = fr_zero();
            if (mine) L = open_horner(c, pt->z);
            suffix_scan<false>(sh, pt->zr, geo.active, L);
            if (mine) store_cell(p.seeds, (size_t)item * geo.seeds + row0 / OPEN_ROWS, t + 1 < geo.active ? lds_get(sh, t + 1) : fr_zero());
            if (t == 0) {                                             // the sweeps chain through the item's own tile cell
                const size_t at = (size_t)item * geo.n_tiles + tile;
                PFe x = lds_get(sh, 0);
                if (sweep + 1 != geo.sweeps) x = open_step(x, pt->zr[geo.active], load_cell(p.tiles, at));
                store_cell(p.tiles, at, x);
            }
            __syncthreads();
        }
    }
    if (!ok) atomicOr(p.status, SHPLONK_CELL_NOT_BELOW_P);
}

__global__ __launch_bounds__(OPEN_THREADS) void hsw_shplonk_write_kernel(ShplonkParams p) {
    if (*p.status & SHPLONK_CELL_NOT_BELOW_P) return;                 // (workgroup-uniform: decided before this launch)
    if (p.unit) write_body<true>(p);
    else write_body<false>(p);
}

hipError_t launch_shplonk_tiles(const ShplonkParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(hsw_shplonk_tiles_kernel, dim3(p.geo.n_tiles, p.n_sets), dim3(OPEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_shplonk_write(const ShplonkParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(hsw_shplonk_write_kernel, dim3(p.geo.n_tiles), dim3(OPEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
