// hsw_permutation_product.hip -- the grand products Z of halo2's permutation argument, written on the device.
//
// hsw_gadget_permutation_product (hsw_gadget_permutation.cpp).  The scheme is hsw_lookup_product.hip's -- Z = (prefix of
// the numerators)(suffix of the denominators) / D, three launches, no host read in between -- with the permutation's
// terms (hsw_permutation_value.hpp) and ONE sequence of tiles per proof: chunk 0's tiles, then chunk 1's, ..., so that
// the prefix carries Z_{s-1}[u] into Z_s[0] and a proof has one inversion, one refusal and one OPEN bit.
//   tiles   a workgroup per (proof, chunk, tile of PRODUCT_TILE rows of Z): lane 0 multiplies up omega^(first row of the
//           tile) from the staged binary powers and shares it through LDS, a thread goes on from its table entry; then a
//           LOOP over the chunk's columns, PRODUCT_ROWS consecutive rows of the value and the sigma column per thread
//           (128 contiguous bytes per column and lane), every stored cell checked against p, num and den of the four
//           rows multiplied up in registers; a tree in LDS leaves the tile's two products in scratch.
//   scan    a workgroup per proof over its S x n_tiles tiles, as the lookup product's; lane 0 inverts D.
//   write   tiles again: num and den recomputed, the scan across the workgroup, two multiplies per row, two 16-byte
//           stores per cell.  A refused proof stores nothing; the lane of row u of the last chunk compares with 1.
// Rows at or beyond u contribute the factor 1.  A thread holds num[4], den[4] and omega^(its first row); the identity
// term of the next row is the last one times omega.  The LDS helpers and scan_pair are the lookup product's, repeated
// here so that its translation unit stays as it is.  Vector loads, vector stores and vector atomics only.
#include "hsw_permutation_product.h"

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

// where a workgroup works: proof c, chunk s, tile of the chunk, g = its place among the proof's tiles
struct Place { u32 c, s, tile, g; };
__device__ __forceinline__ Place place_of(const PermutationParams &p, u32 block) {
    const u32 per_proof = p.S * p.n_tiles, g = block % per_proof;
    return Place{block / per_proof, g / p.n_tiles, g % p.n_tiles, g};
}

// omega^(the thread's first row), in Montgomery form.  Ends synchronised
__device__ __forceinline__ PFe omega_row0(const PermutationParams &p, u32 tile, u32 *shW) {
    const u32 t = threadIdx.x;
    if (t == 0) {
        const PFe w = permutation_omega_tile(*p.powers, tile);
        for (int j = 0; j < 8; j++) shW[j] = w.l[j];
    }
    __syncthreads();
    PFe w;
    for (int j = 0; j < 8; j++) w.l[j] = shW[j];
    return permutation_omega_thread(*p.powers, w, t);
}

// row i of one column into num and den (nothing at and beyond u); false if a stored cell that was read is not below p
template <bool MONT>
__device__ __forceinline__ bool permutation_row(const PermutationParams &p, const PermutationColumn &col, const uint4 *sigma,
                                                const PermutationChallenges &ch, u32 i, const PFe &identity, bool first, PFe &num, PFe &den) {
    if (i >= p.u) return true;
    bool ok = true;
    PFe v = fr_zero();
    if (i < col.rows) { v = load_cell(col.v, i); ok = pfe_below_p(v); }
    const PFe s = load_cell(sigma, i);
    ok = ok && pfe_below_p(s);
    num = permutation_accumulate(num, permutation_factor(v, identity, ch.gamma), first, MONT);
    den = permutation_accumulate(den, permutation_factor(v, permutation_sigma_term(s, ch.beta_mul), ch.gamma), first, MONT);
    return ok;
}
// num and den of the thread's PRODUCT_ROWS rows of chunk s from row0 on (1 at and beyond u): a loop over the chunk's
// columns, the rows written out one by one so that num and den stay in registers
template <bool MONT>
__device__ __forceinline__ bool permutation_rows(const PermutationParams &p, u32 c, u32 s, u32 row0, const PFe &w0, PFe *num, PFe *den) {
    static_assert(PRODUCT_ROWS == 4, "one call per row below");
    const u32 j0 = s * p.L, j1 = p.m - j0 < p.L ? p.m : j0 + p.L;
    const PFe seed = j1 - j0 == p.L ? p.seed_full : p.seed_last, one = fr_one_mont();
    for (u32 r = 0; r < PRODUCT_ROWS; r++) num[r] = den[r] = row0 + r < p.u ? seed : one;
    const PermutationChallenges ch = p.ch[c];
    const PFe omega = p.powers->omega;
    bool ok = true;
    for (u32 j = j0; j < j1; j++) {
        const PermutationColumn col = p.cols[(size_t)c * p.m + j];
        const uint4 *sigma = p.sigmas[j];
        const bool first = j == j0;
        PFe id = permutation_identity_term(p.beta_delta[(size_t)c * p.m + j], w0);
        ok = permutation_row<MONT>(p, col, sigma, ch, row0, id, first, num[0], den[0]) && ok;
        id = fr_mont_mul(id, omega);
        ok = permutation_row<MONT>(p, col, sigma, ch, row0 + 1, id, first, num[1], den[1]) && ok;
        id = fr_mont_mul(id, omega);
        ok = permutation_row<MONT>(p, col, sigma, ch, row0 + 2, id, first, num[2], den[2]) && ok;
        id = fr_mont_mul(id, omega);
        ok = permutation_row<MONT>(p, col, sigma, ch, row0 + 3, id, first, num[3], den[3]) && ok;
    }
    return ok;
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
__global__ __launch_bounds__(PRODUCT_THREADS) void hsw_permutation_tiles_kernel(PermutationParams p) {
    __shared__ u32 shN[8 * PRODUCT_THREADS], shD[8 * PRODUCT_THREADS], shW[8];
    const Place at = place_of(p, blockIdx.x);
    const u32 t = threadIdx.x;
    const PFe w0 = omega_row0(p, at.tile, shW);
    PFe num[PRODUCT_ROWS], den[PRODUCT_ROWS];
    if (!permutation_rows<MONT>(p, at.c, at.s, at.tile * PRODUCT_TILE + t * PRODUCT_ROWS, w0, num, den)) atomicOr(&p.status[at.c], PRODUCT_CELL_NOT_BELOW_P);
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
        store_cell(reinterpret_cast<uint4 *>(p.tiles + 2 * ((size_t)at.c * p.S * p.n_tiles + at.g)), t, v);
    }
}

__global__ __launch_bounds__(PRODUCT_THREADS) void hsw_permutation_scan_kernel(PermutationParams p) {
    __shared__ u32 shN[8 * PRODUCT_THREADS], shD[8 * PRODUCT_THREADS], shInv[8];
    const u32 c = blockIdx.x, t = threadIdx.x, n_tiles = p.S * p.n_tiles;
    uint4 *tiles = reinterpret_cast<uint4 *>(p.tiles + 2 * (size_t)c * n_tiles);   // cell 2 k: numerators, 2 k + 1: denominators
    const u32 chunk = (n_tiles + PRODUCT_THREADS - 1) / PRODUCT_THREADS;
    const u32 lo = (uint64_t)t * chunk < n_tiles ? t * chunk : n_tiles, hi = n_tiles - lo < chunk ? n_tiles : lo + chunk;
    PFe n = fr_one_mont(), d = fr_one_mont();
    for (u32 k = lo; k < hi; k++) { n = fr_mont_mul(n, load_cell(tiles, 2 * k)); d = fr_mont_mul(d, load_cell(tiles, 2 * k + 1)); }
    scan_pair(shN, shD, n, d);
    if (t == 0) {
        const PFe D = lds_get(shD, PRODUCT_THREADS - 1);
        if (fr_is_zero(D)) atomicOr(&p.status[c], PRODUCT_ZERO_DENOM);
        const PFe inv = fr_inv(D);
        for (int j = 0; j < 8; j++) shInv[j] = inv.l[j];
    }
    __syncthreads();
    PFe inv;
    for (int j = 0; j < 8; j++) inv.l[j] = shInv[j];
    // what lies before the chunk of tiles (numerators, over D) and after it (denominators)
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

// row i of Z_s, if there is one; the lane of row u of the last chunk decides whether the proof closes
template <bool MONT>
__device__ __forceinline__ void permutation_emit(const PermutationParams &p, const Place &at, uint4 *z_col, u32 i, const PFe &z_mont) {
    if (i > p.u) return;
    const PFe z = product_cell(z_mont, MONT);
    store_cell(z_col, i, z);
    if (i == p.u && at.s + 1 == p.S && !fr_equal(z, pfe_repr(1u, MONT))) atomicOr(&p.status[at.c], PRODUCT_OPEN);
}

template <bool MONT>
__global__ __launch_bounds__(PRODUCT_THREADS) void hsw_permutation_write_kernel(PermutationParams p) {
    __shared__ u32 shN[8 * PRODUCT_THREADS], shD[8 * PRODUCT_THREADS], shW[8];
    const Place at = place_of(p, blockIdx.x);
    const u32 t = threadIdx.x;
    if (p.status[at.c] & PRODUCT_REFUSED) return;                 // (workgroup-uniform: decided before this launch)
    const u32 row0 = at.tile * PRODUCT_TILE + t * PRODUCT_ROWS;
    const PFe w0 = omega_row0(p, at.tile, shW);
    PFe num[PRODUCT_ROWS], den[PRODUCT_ROWS];
    (void)permutation_rows<MONT>(p, at.c, at.s, row0, w0, num, den);
    // in place: num[k] = num[0] ... num[k], den[k] = den[k] ... den[3]
    num[1] = fr_mont_mul(num[0], num[1]); num[2] = fr_mont_mul(num[1], num[2]); num[3] = fr_mont_mul(num[2], num[3]);
    den[2] = fr_mont_mul(den[2], den[3]); den[1] = fr_mont_mul(den[1], den[2]); den[0] = fr_mont_mul(den[0], den[1]);
    scan_pair(shN, shD, num[3], den[0]);
    PFe base = load_cell(reinterpret_cast<const uint4 *>(p.tiles + 2 * ((size_t)at.c * p.S * p.n_tiles + at.g)), 0);
    if (t) base = fr_mont_mul(base, lds_get(shN, t - 1));
    if (t + 1 < PRODUCT_THREADS) base = fr_mont_mul(base, lds_get(shD, PRODUCT_THREADS - 2 - t));
    // Z[i] = base x (the thread's numerators before i) x (its denominators from i on)
    uint4 *z_col = p.z[(size_t)at.c * p.S + at.s];
    permutation_emit<MONT>(p, at, z_col, row0, fr_mont_mul(base, den[0]));
    permutation_emit<MONT>(p, at, z_col, row0 + 1, fr_mont_mul(fr_mont_mul(base, den[1]), num[0]));
    permutation_emit<MONT>(p, at, z_col, row0 + 2, fr_mont_mul(fr_mont_mul(base, den[2]), num[1]));
    permutation_emit<MONT>(p, at, z_col, row0 + 3, fr_mont_mul(fr_mont_mul(base, den[3]), num[2]));
}

hipError_t launch_permutation_tiles(const PermutationParams &p, bool montgomery, hipStream_t stream) {
    if (p.n_proofs == 0) return hipSuccess;
    const dim3 grid(p.n_proofs * p.S * p.n_tiles), block(PRODUCT_THREADS);
    if (montgomery) hipLaunchKernelGGL(hsw_permutation_tiles_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(hsw_permutation_tiles_kernel<false>, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_permutation_scan(const PermutationParams &p, hipStream_t stream) {
    if (p.n_proofs == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_permutation_scan_kernel, dim3(p.n_proofs), dim3(PRODUCT_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_permutation_write(const PermutationParams &p, bool montgomery, hipStream_t stream) {
    if (p.n_proofs == 0) return hipSuccess;
    const dim3 grid(p.n_proofs * p.S * p.n_tiles), block(PRODUCT_THREADS);
    if (montgomery) hipLaunchKernelGGL(hsw_permutation_write_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(hsw_permutation_write_kernel<false>, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
