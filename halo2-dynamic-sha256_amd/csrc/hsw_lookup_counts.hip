// hsw_lookup_counts.hip -- lookup-table multiplicities of a pass, counted where the cells already are.
//
// hsw_gadget_lookup_multiplicities: the host has listed the pass's lookup entries as runs of device cells
// (hsw_gadget_lookup_runs: every layout, image, pitch and pointer table is in the addresses), so the kernel knows no
// layout -- like hsw_verify_pairs_kernel it is handed addresses.  A work item is `chunk` consecutive entries of one
// run, one workgroup each: one long run and many short ones fill the chip alike.  A lane loads its cell as two
// 16-byte pieces (a spread row: the dense and the spread cell), reduces a Montgomery cell to its value (a stored
// encoding >= p is no cell of the field and hence no table row), decides
// whether the WHOLE 32-byte value is a row of its table, and counts it.  A table of up to LOOKUP_LDS_BINS rows (the
// spread table of up to 11 bits) is counted in an LDS histogram per workgroup that is flushed with one global atomic
// per non-zero bin; a 2^16-row table (the range table always, the 16-bit spread table) does not fit a workgroup's
// LDS as u32 and its entries go straight to the caller's table with a global atomic each: they are 16-bit limbs for
// the most part (a tenth of a proof's range entries lie below 2^11), sparse over 65,536 bins.  Entries that are no
// row of their table are counted once per wave from the ballot, the lowest of them offered with one 64-bit atomic min.
// Vector loads, vector stores and atomics only.
#include "hsw_lookup_counts.h"

namespace hsw {

typedef unsigned int u32;
typedef unsigned long long u64;
#define DEV __device__ __forceinline__

namespace {

struct Cell { u64 l[4]; };

DEV Cell load_cell(const uint4 *base, u64 idx) {
    const uint4 a = base[2 * idx], b = base[2 * idx + 1];
    Cell c;
    c.l[0] = (u64)a.x | ((u64)a.y << 32); c.l[1] = (u64)a.z | ((u64)a.w << 32);
    c.l[2] = (u64)b.x | ((u64)b.y << 32); c.l[3] = (u64)b.z | ((u64)b.w << 32);
    return c;
}
// m = x * 2^256 mod p -> x: the reduction hsw_verify.hip applies on load (from_mont there; the verify kernels keep
// theirs in their own translation unit, so that their code objects do not depend on this one)
DEV Cell from_mont(const Cell &a) {
    const u64 P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    const u64 INV = 0xc2e1f593efffffffull;                       // -p^-1 mod 2^64
    u64 t[5] = {a.l[0], a.l[1], a.l[2], a.l[3], 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 m = t[0] * INV;
        unsigned __int128 s = (unsigned __int128)m * P[0] + t[0];
        u64 carry = (u64)(s >> 64);
#pragma unroll
        for (int j = 1; j < 4; j++) {
            s = (unsigned __int128)m * P[j] + t[j] + carry;
            t[j - 1] = (u64)s;
            carry = (u64)(s >> 64);
        }
        s = (unsigned __int128)t[4] + carry;
        t[3] = (u64)s;
        t[4] = (u64)(s >> 64);
    }
    Cell r;
    r.l[0] = t[0]; r.l[1] = t[1]; r.l[2] = t[2]; r.l[3] = t[3];
    // r < 2p: one conditional subtraction
    bool ge = t[4] != 0;
    if (!ge) { ge = true; for (int i = 3; i >= 0; i--) { if (r.l[i] > P[i]) break; if (r.l[i] < P[i]) { ge = false; break; } } }
    if (ge) { u64 br = 0; for (int i = 0; i < 4; i++) { const unsigned __int128 d = (unsigned __int128)r.l[i] - P[i] - br; r.l[i] = (u64)d; br = (u64)(d >> 64) & 1; } }
    return r;
}
DEV bool narrow(const Cell &c) { return (c.l[1] | c.l[2] | c.l[3]) == 0; }
DEV bool geq_p(const Cell &a) {
    const u64 P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    for (int i = 3; i >= 0; i--) { if (a.l[i] > P[i]) return true; if (a.l[i] < P[i]) return false; }
    return true;
}
// spread.rs:169-189 for a dense value below 2^16: bit b of t at bit 2 b
DEV u32 spread_of(u32 t) {
    t = (t | (t << 8)) & 0x00ff00ffu;
    t = (t | (t << 4)) & 0x0f0f0f0fu;
    t = (t | (t << 2)) & 0x33333333u;
    return (t | (t << 1)) & 0x55555555u;
}

constexpr u32 UNROLL = 4;         // cells a lane has in flight before it classifies the first

}  // namespace

template <bool MONT>
__global__ __launch_bounds__(256) void hsw_lookup_counts_kernel(LookupCountParams p) {
    __shared__ u32 hist[LOOKUP_LDS_BINS];
    // the work item's run: the last one that starts at or before it (workgroup-uniform)
    u32 lo = 0, hi = p.n_runs;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (p.runs[mid].chunk0 <= blockIdx.x) lo = mid; else hi = mid;
    }
    const LookupRun run = p.runs[lo];
    const u64 i0 = ((u64)blockIdx.x - run.chunk0) * p.chunk;
    if (i0 >= run.n) return;                                     // (never: the host counts the chunks of every run)
    const u32 cnt = run.n - i0 < p.chunk ? (u32)(run.n - i0) : p.chunk;
    const bool is_spread = run.spread != nullptr;
    const u32 rows = is_spread ? 1u << p.bits : 65536u;
    u32 *table = is_spread ? p.spread + run.context * p.spread_pitch : p.range + run.context * p.range_pitch;
    const u32 lds_bins = rows <= p.lds_bins ? rows : 0;       // the whole table in LDS, or none of it
    for (u32 t = threadIdx.x; t < lds_bins; t += 256) hist[t] = 0;
    __syncthreads();
    const uint4 *dense = static_cast<const uint4 *>(run.cells) + 2 * i0;
    const uint4 *spread = is_spread ? static_cast<const uint4 *>(run.spread) + 2 * i0 : nullptr;
    const u32 lane = threadIdx.x & 63u;
    for (u32 base = 0; base < cnt; base += 256 * UNROLL) {
        Cell d[UNROLL], s[UNROLL];
#pragma unroll
        for (u32 u = 0; u < UNROLL; u++) {
            const u32 i = base + u * 256 + threadIdx.x;
            d[u] = Cell{{0, 0, 0, 0}}; s[u] = Cell{{0, 0, 0, 0}};
            if (i < cnt) {
                d[u] = load_cell(dense, i);
                if (is_spread) s[u] = load_cell(spread, i);
            }
        }
#pragma unroll
        for (u32 u = 0; u < UNROLL; u++) {
            const u32 i = base + u * 256 + threadIdx.x;
            const bool active = i < cnt;
            bool ok = false;
            u32 t = 0;
            if (active) {
                // a Montgomery cell is an encoding m < p: m + p reduces to the same value, and is no table row (decided
                // before the reduction, which is the last use of the stored limbs)
                const bool enc = !MONT || !(geq_p(d[u]) || (is_spread && geq_p(s[u])));
                const Cell v = MONT ? from_mont(d[u]) : d[u];
                ok = enc && narrow(v) && v.l[0] < rows;
                t = (u32)v.l[0];
                if (ok && is_spread) {
                    const Cell w = MONT ? from_mont(s[u]) : s[u];
                    ok = narrow(w) && w.l[0] == spread_of(t);
                }
            }
            if (ok) {
                if (t < lds_bins) atomicAdd(&hist[t], 1u);
                else atomicAdd(&table[t], 1u);
            }
            const u64 bad = __ballot(active && !ok);
            if (bad && lane == (u32)__ffsll((long long)bad) - 1u) {       // the wave's lowest failing lane: its lowest entry
                atomicAdd(reinterpret_cast<u64 *>(&p.report->not_in_table), (u64)__popcll(bad));
                atomicMin(reinterpret_cast<u64 *>(&p.report->first_key), ((u64)lo << 40) | (i0 + i));
            }
        }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < lds_bins; t += 256) {
        const u32 c = hist[t];
        if (c) atomicAdd(&table[t], c);
    }
}

// the tables of the proofs that have runs, before a count that does not accumulate: blockIdx.x = the proof's place in
// the list, blockIdx.y = 1,024 counters of its table; 16-byte stores where the table is aligned for them
__global__ __launch_bounds__(256) void hsw_lookup_zero_kernel(u32 *table, u64 pitch, u32 counters, const u32 *contexts) {
    u32 *t = table + (u64)contexts[blockIdx.x] * pitch;
    const u32 i = (blockIdx.y * 256u + threadIdx.x) * 4u;
    if (i >= counters) return;
    if ((reinterpret_cast<uintptr_t>(t) & 15u) == 0 && i + 4 <= counters) {
        *reinterpret_cast<uint4 *>(t + i) = make_uint4(0, 0, 0, 0);
    } else {
        for (u32 j = i; j < i + 4 && j < counters; j++) t[j] = 0;
    }
}

hipError_t launch_lookup_counts(const LookupCountParams &p, size_t n_chunks, bool montgomery, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    if (montgomery) hipLaunchKernelGGL(hsw_lookup_counts_kernel<true>, dim3((unsigned)n_chunks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(hsw_lookup_counts_kernel<false>, dim3((unsigned)n_chunks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_lookup_zero(uint32_t *table, uint64_t pitch, uint32_t counters, const uint32_t *d_contexts, size_t n_contexts,
                              hipStream_t stream) {
    if (n_contexts == 0 || counters == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_lookup_zero_kernel, dim3((unsigned)n_contexts, (counters + 1023u) / 1024u), dim3(256), 0, stream, table, pitch,
                       counters, d_contexts);
    return hipGetLastError();
}

}  // namespace hsw
