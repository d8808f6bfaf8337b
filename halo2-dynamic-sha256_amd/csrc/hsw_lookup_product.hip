// hsw_lookup_product.hip -- the grand-product column Z of halo2's lookup argument, written on the device.
//
// hsw_gadget_lookup_product (hsw_gadget_product.cpp).  Z[i] = PN[i] SD[i] / D (hsw_product_value.hpp): no division per
// row, one inversion per argument, three launches on the stream and nothing read by the host in between:
//   tiles   a workgroup per (argument, tile of PRODUCT_TILE rows of Z): every thread loads PRODUCT_ROWS consecutive rows
//           of the input, A' and S' (128 contiguous bytes per column and lane), checks each stored cell against p, forms
//           num and den and multiplies them up; a tree in LDS leaves the tile's two products in scratch (64 B per tile).
//   scan    a workgroup per argument: every thread multiplies a chunk of tiles, a workgroup scan gives the prefix of the
//           numerators and the suffix of the denominators, lane 0 inverts D (fr_inv, about 380 multiplies) and sets
//           PRODUCT_ZERO_DENOM where D = 0; then every tile's factor (prefix) (suffix) / D replaces its numerator.
//   write   tiles again: num and den recomputed, a workgroup scan (prefix of num, suffix of den), two multiplies per row
//           and two 16-byte stores per cell.  A refused argument stores nothing; the lane of row u compares Z[u] with 1.
// Rows at or beyond u contribute the factor 1, so both tile stages walk the same ceil((u + 1) / PRODUCT_TILE) tiles.
// Field elements travel through LDS limb-major (sh[limb][thread]): 4-byte accesses at stride 1, no bank conflict.
// Vector loads, vector stores and vector atomics only.
#include "hsw_lookup_product.h"

namespace hsw {

typedef unsigned int u32;

namespace {

__device__ __forceinline__ PFe load_cell(const uint4 *col, u32 i) {
    const uint4 a = col[2 * (size_t)i], b = col[2 * (size_t)i + 1];
    return PFe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void store_cell(uint4 *col, u32 i, const PFe &v) {
    col[2 * (size_t)i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    col[2 * (size_t)i + 1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ void lds_put(u32 *sh, u32 t, const PFe &v) {
    for (int j = 0; j < 8; j++) sh[j * PRODUCT_THREADS + t] = v.l[j];
}
__device__ __forceinline__ PFe lds_get(const u32 *sh, u32 t) {
    PFe v;
    for (int j = 0; j < 8; j++) v.l[j] = sh[j * PRODUCT_THREADS + t];
    return v;
}

// num and den of row i (1 at and beyond u); false if a stored cell that was read is not below p
template <bool MONT>
__device__ __forceinline__ bool product_row(const ProductParams &p, const ProductArg &arg, const ProductChallenges &ch, u32 i, PFe &num, PFe &den) {
    if (i >= p.u) { num = den = fr_one_mont(); return true; }
    bool ok = true;
    PFe a = fr_zero();
    if (i < arg.input_rows) {
        const PFe d = load_cell(arg.in, i);
        ok = pfe_below_p(d);
        PFe s = fr_zero();
        if (p.kind != 0) { s = load_cell(arg.in_spread, i); ok = ok && pfe_below_p(s); }
        a = product_input(p.kind, d, s, ch.theta_mul);
    }
    const PFe pa = load_cell(arg.pin, i), ps = load_cell(arg.ptab, i);
    ok = ok && pfe_below_p(pa) && pfe_below_p(ps);
    num = product_term(a, product_table(p.kind, i, p.T, ch.theta, MONT), ch, MONT);
    den = product_term(pa, ps, ch, MONT);
    return ok;
}
// ... of the thread's PRODUCT_ROWS rows from row0 on, written out row by row so that num and den stay in registers
template <bool MONT>
__device__ __forceinline__ bool product_rows(const ProductParams &p, const ProductArg &arg, const ProductChallenges &ch, u32 row0,
                                             PFe *num, PFe *den) {
    static_assert(PRODUCT_ROWS == 4, "one call per row below");
    const bool ok0 = product_row<MONT>(p, arg, ch, row0, num[0], den[0]), ok1 = product_row<MONT>(p, arg, ch, row0 + 1, num[1], den[1]);
    const bool ok2 = product_row<MONT>(p, arg, ch, row0 + 2, num[2], den[2]), ok3 = product_row<MONT>(p, arg, ch, row0 + 3, num[3], den[3]);
    return ok0 && ok1 && ok2 && ok3;
}

// Inclusive scans over the workgroup's threads: shN[t] = n[0] ... n[t], and the mirrored one of d, shD[T-1-t] = d[t] ...
// d[T-1] (Hillis-Steele, 8 steps).  Ends synchronised
__device__ __forceinline__ void scan_pair(u32 *shN, u32 *shD, PFe n, PFe d) {
    const u32 t = threadIdx.x;
    lds_put(shN, t, n);
    lds_put(shD, PRODUCT_THREADS - 1 - t, d);
    __syncthreads();
    d = lds_get(shD, t);                                          // from here on thread t scans position t of both
    for (u32 s = 1; s < PRODUCT_THREADS; s <<= 1) {
        PFe on = fr_zero(), od = fr_zero();
        if (t >= s) { on = lds_get(shN, t - s); od = lds_get(shD, t - s); }
        __syncthreads();
        if (t >= s) {
            n = fr_mont_mul(on, n); d = fr_mont_mul(od, d);
            lds_put(shN, t, n); lds_put(shD, t, d);
        }
        __syncthreads();
    }
}

}  // namespace

template <bool MONT>
__global__ __launch_bounds__(PRODUCT_THREADS) void hsw_product_tiles_kernel(ProductParams p) {
    __shared__ u32 shN[8 * PRODUCT_THREADS], shD[8 * PRODUCT_THREADS];
    const u32 a = blockIdx.x / p.n_tiles, tile = blockIdx.x % p.n_tiles, t = threadIdx.x;
    const ProductArg arg = p.args[a];
    const ProductChallenges ch = p.ch[arg.context];
    PFe num[PRODUCT_ROWS], den[PRODUCT_ROWS];
    if (!product_rows<MONT>(p, arg, ch, tile * PRODUCT_TILE + t * PRODUCT_ROWS, num, den)) atomicOr(&p.status[a], PRODUCT_CELL_NOT_BELOW_P);
    const PFe n = fr_mont_mul(fr_mont_mul(num[0], num[1]), fr_mont_mul(num[2], num[3]));
    const PFe d = fr_mont_mul(fr_mont_mul(den[0], den[1]), fr_mont_mul(den[2], den[3]));
    lds_put(shN, t, n);
    lds_put(shD, t, d);
    __syncthreads();
    for (u32 s = PRODUCT_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            lds_put(shN, t, fr_mont_mul(lds_get(shN, t), lds_get(shN, t + s)));
            lds_put(shD, t, fr_mont_mul(lds_get(shD, t), lds_get(shD, t + s)));
        }
        __syncthreads();
    }
    if (t < 2) {                                                  // lane 0 the numerators' product, lane 1 the denominators'
        const PFe v = lds_get(t ? shD : shN, 0);
        store_cell(reinterpret_cast<uint4 *>(p.tiles + 2 * ((size_t)a * p.n_tiles + tile)), t, v);
    }
}

__global__ __launch_bounds__(PRODUCT_THREADS) void hsw_product_scan_kernel(ProductParams p) {
    __shared__ u32 shN[8 * PRODUCT_THREADS], shD[8 * PRODUCT_THREADS], shInv[8];
    const u32 a = blockIdx.x, t = threadIdx.x;
    uint4 *tiles = reinterpret_cast<uint4 *>(p.tiles + 2 * (size_t)a * p.n_tiles);   // cell 2 k: numerators, 2 k + 1: denominators
    const u32 chunk = (p.n_tiles + PRODUCT_THREADS - 1) / PRODUCT_THREADS;
    const u32 lo = t * chunk < p.n_tiles ? t * chunk : p.n_tiles, hi = p.n_tiles - lo < chunk ? p.n_tiles : lo + chunk;
    PFe n = fr_one_mont(), d = fr_one_mont();
    for (u32 k = lo; k < hi; k++) { n = fr_mont_mul(n, load_cell(tiles, 2 * k)); d = fr_mont_mul(d, load_cell(tiles, 2 * k + 1)); }
    scan_pair(shN, shD, n, d);
    if (t == 0) {
        const PFe D = lds_get(shD, PRODUCT_THREADS - 1);
        if (fr_is_zero(D)) atomicOr(&p.status[a], PRODUCT_ZERO_DENOM);
        const PFe inv = fr_inv(D);
        for (int j = 0; j < 8; j++) shInv[j] = inv.l[j];
    }
    __syncthreads();
    PFe inv;
    for (int j = 0; j < 8; j++) inv.l[j] = shInv[j];
    // what lies before the chunk (numerators, over D) and after it (denominators)
    PFe run_n = t ? fr_mont_mul(lds_get(shN, t - 1), inv) : inv;
    PFe run_d = t + 1 < PRODUCT_THREADS ? lds_get(shD, PRODUCT_THREADS - 2 - t) : fr_one_mont();
    for (u32 k = hi; k > lo; k--) {                               // the suffix, in place of the tile's denominators
        const PFe own = load_cell(tiles, 2 * (k - 1) + 1);
        store_cell(tiles, 2 * (k - 1) + 1, run_d);
        run_d = fr_mont_mul(run_d, own);
    }
    for (u32 k = lo; k < hi; k++) {                               // the factor, in place of the tile's numerators
        const PFe own = load_cell(tiles, 2 * k);
        store_cell(tiles, 2 * k, fr_mont_mul(run_n, load_cell(tiles, 2 * k + 1)));
        run_n = fr_mont_mul(run_n, own);
    }
}

// row i of Z, if there is one; the lane of row u decides whether the argument closes
template <bool MONT>
__device__ __forceinline__ void product_emit(const ProductParams &p, const ProductArg &arg, u32 a, u32 i, const PFe &z_mont) {
    if (i > p.u) return;
    const PFe z = product_cell(z_mont, MONT);
    store_cell(arg.z, i, z);
    if (i == p.u && !fr_equal(z, pfe_repr(1u, MONT))) atomicOr(&p.status[a], PRODUCT_OPEN);
}

template <bool MONT>
__global__ __launch_bounds__(PRODUCT_THREADS) void hsw_product_write_kernel(ProductParams p) {
    __shared__ u32 shN[8 * PRODUCT_THREADS], shD[8 * PRODUCT_THREADS];
    const u32 a = blockIdx.x / p.n_tiles, tile = blockIdx.x % p.n_tiles, t = threadIdx.x;
    if (p.status[a] & PRODUCT_REFUSED) return;                    // (workgroup-uniform: decided before this launch)
    const ProductArg arg = p.args[a];
    const ProductChallenges ch = p.ch[arg.context];
    const u32 row0 = tile * PRODUCT_TILE + t * PRODUCT_ROWS;
    PFe num[PRODUCT_ROWS], den[PRODUCT_ROWS];
    (void)product_rows<MONT>(p, arg, ch, row0, num, den);
    // in place: num[k] = num[0] ... num[k], den[k] = den[k] ... den[3]
    num[1] = fr_mont_mul(num[0], num[1]); num[2] = fr_mont_mul(num[1], num[2]); num[3] = fr_mont_mul(num[2], num[3]);
    den[2] = fr_mont_mul(den[2], den[3]); den[1] = fr_mont_mul(den[1], den[2]); den[0] = fr_mont_mul(den[0], den[1]);
    scan_pair(shN, shD, num[3], den[0]);
    PFe base = load_cell(reinterpret_cast<const uint4 *>(p.tiles + 2 * ((size_t)a * p.n_tiles + tile)), 0);
    if (t) base = fr_mont_mul(base, lds_get(shN, t - 1));
    if (t + 1 < PRODUCT_THREADS) base = fr_mont_mul(base, lds_get(shD, PRODUCT_THREADS - 2 - t));
    // Z[i] = base x (the thread's numerators before i) x (its denominators from i on)
    product_emit<MONT>(p, arg, a, row0, fr_mont_mul(base, den[0]));
    product_emit<MONT>(p, arg, a, row0 + 1, fr_mont_mul(fr_mont_mul(base, den[1]), num[0]));
    product_emit<MONT>(p, arg, a, row0 + 2, fr_mont_mul(fr_mont_mul(base, den[2]), num[1]));
    product_emit<MONT>(p, arg, a, row0 + 3, fr_mont_mul(fr_mont_mul(base, den[3]), num[2]));
}

hipError_t launch_product_tiles(const ProductParams &p, bool montgomery, hipStream_t stream) {
    if (p.n_args == 0) return hipSuccess;
    const dim3 grid(p.n_args * p.n_tiles), block(PRODUCT_THREADS);
    if (montgomery) hipLaunchKernelGGL(hsw_product_tiles_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(hsw_product_tiles_kernel<false>, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_product_scan(const ProductParams &p, hipStream_t stream) {
    if (p.n_args == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_product_scan_kernel, dim3(p.n_args), dim3(PRODUCT_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_product_write(const ProductParams &p, bool montgomery, hipStream_t stream) {
    if (p.n_args == 0) return hipSuccess;
    const dim3 grid(p.n_args * p.n_tiles), block(PRODUCT_THREADS);
    if (montgomery) hipLaunchKernelGGL(hsw_product_write_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(hsw_product_write_kernel<false>, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
