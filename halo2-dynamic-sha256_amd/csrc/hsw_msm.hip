// hsw_msm.hip -- the BN254 G1 multi-scalar multiplication of device columns against device-resident bases.
//
// hsw_gadget_msm (hsw_gadget_msm.cpp).  The rules -- digits, slices, chunks, where a partial bucket lies -- are
// hsw_msm_value.hpp's, the arithmetic hsw_g1.hpp's.  Three kernels of MSM_THREADS threads:
//   check        a base per thread of the checked rows, both coordinates against q; a workgroup counts in LDS and adds
//                its count and its lowest row to the report with one vector atomic each
//   accumulate   a workgroup per (slice, window, column).  Per chunk of its slice: cells loaded coalesced, checked
//                against r, brought to the canonical integer (one fr_from_mont for Montgomery cells), the window's
//                digit taken; an LDS atomic per row counts the digit and gives the row its rank in the digit's list;
//                thread d reads where list d starts (msm_bucket_start); the rows scatter their chunk-local index into
//                the sorted list; then thread d - 1 OWNS bucket d, held in registers across the chunks, and adds the
//                bases of its list with the complete mixed formula -- no branch but the skip of an affine (0, 0).  A
//                rank depends on the order of the atomics, a bucket's sum does not (the group is abelian).
//   reduce       a workgroup per (window, column): thread d - 1 sums bucket d of the column's slices, then the window's
//                sum_d d * B_d is the sum of the suffix sums: a suffix scan over the 256 places in LDS (8 steps) and a
//                tree sum (8 steps), every step one complete addition in every lane.  One point per (window, column).
// A slice at or beyond a column's rows returns at once, workgroup-uniform, and the reduce launch does not read it.
// Every thread of a workgroup that goes on reaches every barrier.  Cell indices are below 2^28 and stay 32-bit; byte
// offsets are formed from (size_t) products.  The LDS helpers are the NTT's, repeated so that its translation unit stays
// as it is.  Vector loads, vector stores, vector and LDS atomics only.
#include "hsw_msm.h"

namespace hsw {

typedef unsigned int u32;

namespace {

__device__ __forceinline__ PFe load_cell(const uint4 *col, u32 i) {
    const uint4 a = col[2 * (size_t)i], b = col[2 * (size_t)i + 1];
    return PFe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ Fq fq_of(const uint4 &a, const uint4 &b) { return Fq{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}}; }
__device__ __forceinline__ G1Affine load_base(const uint4 *bases, u32 i) {
    const uint4 *b = bases + 4 * (size_t)i;
    return G1Affine{fq_of(b[0], b[1]), fq_of(b[2], b[3])};
}
__device__ __forceinline__ G1 load_point(const uint4 *points, uint64_t i) {
    const uint4 *b = points + 6 * (size_t)i;
    return G1{fq_of(b[0], b[1]), fq_of(b[2], b[3]), fq_of(b[4], b[5])};
}
__device__ __forceinline__ void store_fq(uint4 *at, const Fq &v) {
    at[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    at[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ void store_point(uint4 *points, uint64_t i, const G1 &v) {
    uint4 *b = points + 6 * (size_t)i;
    store_fq(b, v.x); store_fq(b + 2, v.y); store_fq(b + 4, v.z);
}
// a point in LDS, limb-major: every access 4 bytes at lane stride one
__device__ __forceinline__ void lds_put(u32 *sh, u32 l, const G1 &v) {
    for (int j = 0; j < 8; j++) {
        sh[j * MSM_THREADS + l] = v.x.l[j];
        sh[(8 + j) * MSM_THREADS + l] = v.y.l[j];
        sh[(16 + j) * MSM_THREADS + l] = v.z.l[j];
    }
}
__device__ __forceinline__ G1 lds_get(const u32 *sh, u32 l) {
    G1 v;
    for (int j = 0; j < 8; j++) {
        v.x.l[j] = sh[j * MSM_THREADS + l];
        v.y.l[j] = sh[(8 + j) * MSM_THREADS + l];
        v.z.l[j] = sh[(16 + j) * MSM_THREADS + l];
    }
    return v;
}

}  // namespace

__global__ __launch_bounds__(MSM_THREADS) void hsw_msm_check_kernel(const uint4 *bases, u32 rows, MsmCheck *check) {
    __shared__ u32 shBad, shFirst;
    const u32 t = threadIdx.x, i = blockIdx.x * MSM_THREADS + t;
    if (t == 0) { shBad = 0; shFirst = ~0u; }
    __syncthreads();
    if (i < rows) {
        const G1Affine b = load_base(bases, i);
        if (!fq_below_q(b.x) || !fq_below_q(b.y)) { atomicAdd(&shBad, 1u); atomicMin(&shFirst, i); }
    }
    __syncthreads();
    if (t == 0 && shBad) { atomicAdd(&check->bad, shBad); atomicMin(&check->first, shFirst); }
}

__global__ __launch_bounds__(MSM_THREADS) void hsw_msm_accumulate_kernel(MsmParams p) {
    __shared__ u32 hist[MSM_THREADS];                  // rows of the chunk per digit; [0] stays 0: digit 0 is dropped
    __shared__ u32 start[MSM_THREADS];                 // where a digit's list starts in sorted[]
    __shared__ u32 digit_rank[MSM_CHUNK_ROWS];         // digit << 16 | rank in the digit's list, per row of the chunk
    __shared__ unsigned short sorted[MSM_CHUNK_ROWS];  // chunk-local rows, by digit
    __shared__ u32 shBad;
    const u32 t = threadIdx.x, slice = blockIdx.x, w = blockIdx.y, gb = blockIdx.z;
    const MsmPlan &g = p.plan;
    const MsmColumn col = p.cols[gb];
    const u32 row0 = slice * g.slice_rows;
    if (row0 >= col.rows) return;                      // (workgroup-uniform, before any barrier)
    const u32 row_end = col.rows - row0 < g.slice_rows ? col.rows : row0 + g.slice_rows;
    if (t == 0) shBad = 0;
    G1 bucket = g1_identity();
    for (u32 chunk0 = row0; chunk0 < row_end; chunk0 += g.chunk_rows) {
        const u32 n = row_end - chunk0 < g.chunk_rows ? row_end - chunk0 : g.chunk_rows;
        hist[t] = 0;
        __syncthreads();
        for (u32 l = t; l < n; l += MSM_THREADS) {
            const PFe cell = load_cell(col.cells, chunk0 + l);
            PFe a;
            u32 d = 0;
            if (msm_canonical(cell, p.montgomery != 0, a)) d = msm_digit(a, w, g.window_bits);
            else atomicOr(&shBad, 1u);
            const u32 rank = d ? atomicAdd(&hist[d], 1u) : 0u;
            digit_rank[l] = d << 16 | rank;
        }
        __syncthreads();
        start[t] = t ? msm_bucket_start(hist, t) : 0u;
        __syncthreads();
        for (u32 l = t; l < n; l += MSM_THREADS) {
            const u32 dr = digit_rank[l];
            if (dr >> 16) sorted[start[dr >> 16] + (dr & 0xffffu)] = (unsigned short)l;
        }
        __syncthreads();
        if (t < g.buckets) {
            const u32 s = start[t + 1], count = hist[t + 1];
            for (u32 j = 0; j < count; j++) {
                const G1Affine b = load_base(p.bases, chunk0 + sorted[s + j]);
                if (!g1_affine_is_identity(b)) bucket = g1_add_mixed(bucket, b);
            }
        }
        __syncthreads();                               // (the lists are read: the next chunk may overwrite them)
    }
    if (t < g.buckets) store_point(p.partial, msm_partial_index(g, gb, w, slice, t + 1), bucket);
    if (t == 0 && shBad) atomicOr(&p.status[gb], (u32)MSM_CELL_NOT_BELOW_P);
}

__global__ __launch_bounds__(MSM_THREADS) void hsw_msm_reduce_kernel(MsmParams p) {
    __shared__ u32 sh[24 * MSM_THREADS];
    const u32 t = threadIdx.x, w = blockIdx.x, gb = blockIdx.y;
    const MsmPlan &g = p.plan;
    const u32 n_slices = msm_slices(p.cols[gb].rows, g.slice_rows);
    G1 mine = g1_identity();                           // place t holds bucket t + 1; the places beyond the buckets the identity
    if (t < g.buckets)
        for (u32 s = 0; s < n_slices; s++) mine = g1_add(mine, load_point(p.partial, msm_partial_index(g, gb, w, s, t + 1)));
    lds_put(sh, t, mine);
    __syncthreads();
    for (u32 off = 1; off < MSM_THREADS; off <<= 1) {  // the suffix sums T_t = sum of the places from t on
        const G1 other = t + off < MSM_THREADS ? lds_get(sh, t + off) : g1_identity();
        __syncthreads();
        mine = g1_add(mine, other);
        lds_put(sh, t, mine);
        __syncthreads();
    }
    for (u32 off = MSM_THREADS / 2; off >= 1; off >>= 1) {   // their sum: places [off, 2 off) onto [0, off)
        if (t < off) {
            mine = g1_add(mine, lds_get(sh, t + off));
            lds_put(sh, t, mine);
        }
        __syncthreads();
    }
    if (t == 0) store_point(p.windows, (uint64_t)gb * g.windows + w, mine);
}

hipError_t launch_msm_check(const uint4 *bases, uint32_t rows, MsmCheck *check, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_msm_check_kernel, dim3((rows + MSM_THREADS - 1) / MSM_THREADS), dim3(MSM_THREADS), 0, stream, bases, rows, check);
    return hipGetLastError();
}

hipError_t launch_msm_accumulate(const MsmParams &p, uint32_t n_columns, hipStream_t stream) {
    hipLaunchKernelGGL(hsw_msm_accumulate_kernel, dim3(p.plan.slices, p.plan.windows, n_columns), dim3(MSM_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_msm_reduce(const MsmParams &p, uint32_t n_columns, hipStream_t stream) {
    hipLaunchKernelGGL(hsw_msm_reduce_kernel, dim3(p.plan.windows, n_columns), dim3(MSM_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
