// hsw_lookup_permuted.hip -- halo2's permuted lookup columns A' and S', written on the device from multiplicities.
//
// hsw_gadget_lookup_permuted (hsw_gadget_permuted.cpp): per argument the multiplicities m[t] are already counted
// (hsw_lookup_counts_kernel, one table per argument) or given.  No field element is sorted:
//   prepare   one workgroup per argument.  E = sum m; m'[0] = m[0] + (u - E); every thread walks a chunk of four table
//             rows twice -- its sums, a workgroup scan, then its entries of the three compact arrays of
//             hsw_permuted_index.hpp (the used rows with their offsets, the spare rows).
//   values    the cell of every table row, once per table (hsw_permuted_value.hpp): the write stage copies cells.
//   write     split by tiles of PERMUTED_TILE OUTPUT rows, not by table rows: m'[0] is most of a column.  A tile
//             searches the offsets once for its first row (workgroup-uniform), stages the at most PERMUTED_TILE + 1
//             offsets its rows can fall into in LDS, and every lane resolves its row there.  A lane writes the A'
//             and the S' cell of its row as two 16-byte stores each; consecutive lanes write consecutive cells, so a
//             wave writes 2 KiB contiguous per column.  With the report's flag set (an entry that is no table row,
//             multiplicities that exceed the usable rows) no tile stores anything: all or nothing, no host read
//             between the stages.
// Vector loads and plain vector stores only.
#include "hsw_lookup_permuted.h"

#include "hsw_permuted_value.hpp"

namespace hsw {

typedef unsigned int u32;
typedef unsigned long long u64;

namespace {
constexpr u32 PREPARE_THREADS = 1024, PREPARE_ROWS = 4;
}

__global__ __launch_bounds__(256) void hsw_permuted_zero_kernel(u32 *m, u64 pitch, u32 T) {
    const u32 t = blockIdx.y * 256u + threadIdx.x;
    if (t < T) m[(u64)blockIdx.x * pitch + t] = 0;
}

// the sum of table blockIdx.x into sum[0] (every thread returns it)
__device__ __forceinline__ u64 table_sum(const u32 *m, u32 T, u64 *scratch) {
    u64 s = 0;
    for (u32 t = threadIdx.x; t < T; t += blockDim.x) s += m[t];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63u) == 0) scratch[threadIdx.x >> 6] = s;
    __syncthreads();
    u64 all = 0;
    for (u32 w = 0; w < (blockDim.x + 63u) / 64u; w++) all += scratch[w];
    __syncthreads();
    return all;
}

__global__ __launch_bounds__(256) void hsw_permuted_sums_kernel(const u32 *m, u64 pitch, u32 T, u32 u, PermutedReport *report) {
    __shared__ u64 scratch[4];
    const u64 E = table_sum(m + (u64)blockIdx.x * pitch, T, scratch);
    if (threadIdx.x == 0 && E > u) atomicAdd(reinterpret_cast<u64 *>(&report->overflow), 1ull);
}

__global__ __launch_bounds__(PREPARE_THREADS) void hsw_permuted_prepare_kernel(PermutedParams p) {
    __shared__ u64 scratch[PREPARE_THREADS / 64];
    __shared__ PermutedSums wave_sums[PREPARE_THREADS / 64];
    const u32 a = blockIdx.x;
    const u32 *m = p.args[a].m;
    u32 *used_off = p.index + (size_t)a * permuted_index_words(p.T), *used_row = used_off + p.T + 1, *spare_row = used_row + p.T;
    const u64 E = table_sum(m, p.T, scratch);
    if (E > p.u) {                                               // (the flag is set: nothing reads this argument's arrays)
        if (threadIdx.x == 0) p.heads[a] = PermutedHead{0, 0, 0, 0};
        return;
    }
    const u32 pad0 = p.u - (u32)E;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // PREPARE_ROWS consecutive rows per thread, so that a wave reads 1 KiB contiguous; the chunk bases from a scan over
    // the workgroup (shuffles inside a wave, the wave sums through LDS), carried from one sweep of 4,096 rows to the next
    PermutedSums carry{0, 0, 0};
    for (u32 r0 = 0; r0 < p.T; r0 += PREPARE_THREADS * PREPARE_ROWS) {
        const u32 at = r0 + threadIdx.x * PREPARE_ROWS;
        const u32 lo = at < p.T ? at : p.T, hi = lo + PREPARE_ROWS < p.T ? lo + PREPARE_ROWS : p.T;
        const PermutedSums mine = permuted_chunk_sums(m, lo, hi, pad0);
        PermutedSums inc = mine;
        for (u32 d = 1; d < 64; d <<= 1) {
            const u32 r = __shfl_up(inc.rows, d, 64), us = __shfl_up(inc.used, d, 64), sp = __shfl_up(inc.spare, d, 64);
            if (lane >= d) { inc.rows += r; inc.used += us; inc.spare += sp; }
        }
        if (lane == 63) wave_sums[wave] = inc;
        __syncthreads();
        PermutedSums base{carry.rows + inc.rows - mine.rows, carry.used + inc.used - mine.used, carry.spare + inc.spare - mine.spare};
        for (u32 w = 0; w < PREPARE_THREADS / 64; w++) {
            const PermutedSums t = wave_sums[w];
            if (w < wave) { base.rows += t.rows; base.used += t.used; base.spare += t.spare; }
            carry.rows += t.rows; carry.used += t.used; carry.spare += t.spare;
        }
        permuted_chunk_write(m, lo, hi, pad0, base, used_off, used_row, spare_row);
        __syncthreads();                                         // (wave_sums is written again)
    }
    if (threadIdx.x == 0) {
        p.heads[a] = permuted_head(m, p.T, p.u, pad0, carry);
        used_off[carry.used] = p.u;                              // the sentinel: carry.used <= T
    }
}

template <bool MONT>
__global__ __launch_bounds__(256) void hsw_permuted_values_kernel(uint4 *values, const u32 *thetas, u32 kind, u32 T) {
    const u32 t = blockIdx.y * 256u + threadIdx.x;
    if (t >= T) return;
    PFe theta{{0, 0, 0, 0, 0, 0, 0, 0}};
    if (kind != PERMUTED_VALUE_RANGE)
        for (int j = 0; j < 8; j++) theta.l[j] = thetas[(size_t)blockIdx.x * 8u + j];
    const PFe v = permuted_value(kind, t, theta, MONT);
    uint4 *out = values + 2 * ((size_t)blockIdx.x * T + t);
    out[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    out[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

__global__ __launch_bounds__(256) void hsw_permuted_write_kernel(PermutedParams p) {
    __shared__ u32 win[PERMUTED_TILE + 1];
    if (p.report->count.not_in_table | p.report->overflow) return;          // all or nothing
    const u32 a = blockIdx.y;
    const PermutedHead head = p.heads[a];
    const u32 i0 = blockIdx.x * PERMUTED_TILE;
    if (!head.ok || !head.used || i0 >= p.u) return;              // (never: the flag covers the first, u >= T >= 1 the second)
    const u32 i1 = p.u - i0 < PERMUTED_TILE ? p.u : i0 + PERMUTED_TILE;
    const PermutedArg arg = p.args[a];
    const u32 *used_off = p.index + (size_t)a * permuted_index_words(p.T), *used_row = used_off + p.T + 1, *spare_row = used_row + p.T;
    // the run of the tile's first row, and the offsets its rows can fall into: every run has at least one row, so row
    // i0 + k lies in run j0 + k at the latest.  win[n] is the next run's offset or the sentinel used_off[used] = u
    const u32 j0 = permuted_find(used_off, 0, head.used, i0);
    const u32 n = head.used - j0 < PERMUTED_TILE ? head.used - j0 : PERMUTED_TILE;
    for (u32 k = threadIdx.x; k <= n; k += 256) win[k] = used_off[j0 + k];
    __syncthreads();
    const bool one_run = win[1] >= i1;                            // the whole tile inside run j0: the usual case under m'[0]
    uint4 *in = static_cast<uint4 *>(arg.input), *tab = static_cast<uint4 *>(arg.table);
    for (u32 i = i0 + threadIdx.x; i < i1; i += 256) {
        u32 t, r;                                                 // the table rows of A'[i] and S'[i]
        permuted_rows(win, one_run ? 1u : n, j0, i, used_row, spare_row, head.zeros, &t, &r);
        const uint4 v0 = arg.values[2 * (size_t)t], v1 = arg.values[2 * (size_t)t + 1];
        const uint4 s0 = arg.values[2 * (size_t)r], s1 = arg.values[2 * (size_t)r + 1];
        in[2 * (size_t)i] = v0; in[2 * (size_t)i + 1] = v1;
        tab[2 * (size_t)i] = s0; tab[2 * (size_t)i + 1] = s1;
    }
}

hipError_t launch_permuted_zero(uint32_t *m, uint64_t pitch, uint32_t T, size_t n_tables, hipStream_t stream) {
    if (n_tables == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_permuted_zero_kernel, dim3((unsigned)n_tables, (T + 255u) / 256u), dim3(256), 0, stream, m, pitch, T);
    return hipGetLastError();
}

hipError_t launch_permuted_sums(const uint32_t *m, uint64_t pitch, uint32_t T, uint32_t u, size_t n_tables, PermutedReport *report,
                                hipStream_t stream) {
    if (n_tables == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_permuted_sums_kernel, dim3((unsigned)n_tables), dim3(256), 0, stream, m, pitch, T, u, report);
    return hipGetLastError();
}

hipError_t launch_permuted_prepare(const PermutedParams &p, hipStream_t stream) {
    if (p.n_args == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_permuted_prepare_kernel, dim3(p.n_args), dim3(PREPARE_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_permuted_values(uint4 *values, const uint32_t *thetas, uint32_t kind, uint32_t T, size_t n_tables, bool montgomery,
                                  hipStream_t stream) {
    if (n_tables == 0) return hipSuccess;
    const dim3 grid((unsigned)n_tables, (T + 255u) / 256u);
    if (montgomery) hipLaunchKernelGGL(hsw_permuted_values_kernel<true>, grid, dim3(256), 0, stream, values, thetas, kind, T);
    else hipLaunchKernelGGL(hsw_permuted_values_kernel<false>, grid, dim3(256), 0, stream, values, thetas, kind, T);
    return hipGetLastError();
}

hipError_t launch_permuted_write(const PermutedParams &p, hipStream_t stream) {
    if (p.n_args == 0 || p.u == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_permuted_write_kernel, dim3((p.u + PERMUTED_TILE - 1) / PERMUTED_TILE, p.n_args), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
