// hsw_lookup_counts.h -- launch interface of the lookup-multiplicity count (hsw_lookup_counts.hip;
// hsw_gadget_lookup_multiplicities in hsw_gadget_lookup.cpp is its only caller).
#ifndef HSW_LOOKUP_COUNTS_H
#define HSW_LOOKUP_COUNTS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hsw {

// One run of the uploaded run table: n consecutive 32-byte cells (16-byte aligned) -- and, for a run of the spread
// table, the n spread cells of the same rows.  The runs are in (context, table, column, first) order
struct LookupRun {
    const void *cells, *spread;    // spread NULL: entries of the range table
    uint64_t n;
    uint64_t chunk0;               // the run's first work item among all of the launch (ascending)
    uint64_t context;
};

struct LookupReport {              // device memory
    uint64_t not_in_table;
    uint64_t first_key;            // (run << 40) | entry in the run, of the lowest failing entry; ~0 = none
};

enum : uint32_t { LOOKUP_LDS_BINS = 2048 };   // the largest table a workgroup counts in LDS

struct LookupCountParams {
    const LookupRun *runs;
    uint32_t n_runs;
    uint32_t chunk;                // entries per work item (one workgroup each): a multiple of 256
    uint32_t *range, *spread;      // the caller's counters; the table of proof c starts c * pitch counters in
    uint64_t range_pitch, spread_pitch;
    uint32_t bits;                 // the spread table has 2^bits rows
    uint32_t lds_bins;             // tables of up to this many rows are counted in LDS first (<= LOOKUP_LDS_BINS; 0: global atomics only)
    LookupReport *report;
};

// n_chunks work items; montgomery: the cells are x * 2^256 mod p, reduced on load
hipError_t launch_lookup_counts(const LookupCountParams &p, size_t n_chunks, bool montgomery, hipStream_t stream);
// zeroes `counters` counters of the table of every listed proof: table[contexts[i] * pitch + 0 .. counters)
hipError_t launch_lookup_zero(uint32_t *table, uint64_t pitch, uint32_t counters, const uint32_t *d_contexts, size_t n_contexts,
                              hipStream_t stream);

}  // namespace hsw
#endif
