// hsw_open_device.hpp -- the device-side helpers that the kernels over the geometry of hsw_open_value.hpp share:
// hsw_open.hip (evaluate and the GWC opening) and hsw_shplonk.hip (SHPLONK's multi-point opening).  Cells as two 16-byte
// accesses, field elements through LDS limb-major (sh[limb][thread]): 4-byte accesses at stride 1, no bank conflict,
// a thread's rows of a column with the check against p, and the workgroup suffix scan.  Internal linkage: every
// translation unit that includes it gets its own inlined copies.
#ifndef HSW_OPEN_DEVICE_HPP
#define HSW_OPEN_DEVICE_HPP

#include <hip/hip_runtime.h>

#include "hsw_open_value.hpp"

namespace hsw {
namespace {

__device__ __forceinline__ PFe load_cell(const uint4 *col, size_t i) {
    const uint4 a = col[2 * i], b = col[2 * i + 1];
    return PFe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void store_cell(uint4 *col, size_t i, const PFe &v) {
    col[2 * i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    col[2 * i + 1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ void lds_put(unsigned int *sh, unsigned int t, const PFe &v) {
    for (int j = 0; j < 8; j++) sh[j * OPEN_THREADS + t] = v.l[j];
}
__device__ __forceinline__ PFe lds_get(const unsigned int *sh, unsigned int t) {
    PFe v;
    for (int j = 0; j < 8; j++) v.l[j] = sh[j * OPEN_THREADS + t];
    return v;
}

// a thread's rows of a column, 0 at and beyond col_rows; false if a stored cell that was read is not below p
__device__ __forceinline__ bool load_rows(const uint4 *cells, unsigned int col_rows, unsigned int row0, PFe *a) {
    bool ok = true;
#pragma unroll
    for (unsigned int k = 0; k < OPEN_ROWS; k++) {
        a[k] = fr_zero();
        if (row0 + k < col_rows) { a[k] = load_cell(cells, row0 + k); ok = ok && pfe_below_p(a[k]); }
    }
    return ok;
}

// The inclusive suffix scan over the first `active` threads: sh[t] = x[t] + M x[t+1] + M^2 x[t+2] + ..., with the step
// multipliers M^(2^k) = pow[k] (LOG) or pow[2^k].  Hillis-Steele, a multiply per step.  Ends synchronised
template <bool LOG>
__device__ __forceinline__ void suffix_scan(unsigned int *sh, const PFe *pow, unsigned int active, PFe x) {
    const unsigned int t = threadIdx.x;
    lds_put(sh, t, x);
    __syncthreads();
    unsigned int k = 0;
    for (unsigned int s = 1; s < active; s <<= 1, k++) {
        const bool on = t + s < active;
        PFe o = fr_zero();
        if (on) o = lds_get(sh, t + s);
        __syncthreads();
        if (on) {
            x = open_step(x, pow[LOG ? k : s], o);
            lds_put(sh, t, x);
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace hsw
#endif
