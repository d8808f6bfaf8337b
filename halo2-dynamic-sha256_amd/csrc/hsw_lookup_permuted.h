// hsw_lookup_permuted.h -- launch interface of the permuted lookup pair (hsw_lookup_permuted.hip;
// hsw_gadget_lookup_permuted in hsw_gadget_permuted.cpp is its only caller).
#ifndef HSW_LOOKUP_PERMUTED_H
#define HSW_LOOKUP_PERMUTED_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_lookup_counts.h"
#include "hsw_permuted_index.hpp"

namespace hsw {

// The call's report on the device.  Its head is the count's own (LookupReport: hsw_lookup_counts_kernel writes there);
// a non-zero not_in_table or overflow is the flag that keeps the write stage from storing anything
struct PermutedReport {
    LookupReport count;
    uint64_t overflow;             // arguments whose multiplicities sum to more than usable_rows
    uint64_t reserved_;
};

// One argument of a group, as the prepare and write stages take it
struct PermutedArg {
    const uint32_t *m;             // its T multiplicities
    void *input, *table;           // A' and S': usable_rows cells each, 16-byte aligned
    const uint4 *values;           // its value table: T cells (two uint4 each) in the representation of the pass
};

enum : uint32_t { PERMUTED_TILE = 1024 };      // output rows per workgroup of the write stage

struct PermutedParams {
    const PermutedArg *args;       // the group's arguments
    uint32_t n_args;
    uint32_t T;                    // table rows
    uint32_t u;                    // usable rows
    uint32_t *index;               // n_args x permuted_index_words(T)
    PermutedHead *heads;           // n_args
    PermutedReport *report;
};

enum : uint32_t { PERMUTED_VALUE_RANGE = 0, PERMUTED_VALUE_SPREAD = 1, PERMUTED_VALUE_THETA_ON_SPREAD = 2 };

// zeroes T counters of n_tables tables `pitch` counters apart
hipError_t launch_permuted_zero(uint32_t *m, uint64_t pitch, uint32_t T, size_t n_tables, hipStream_t stream);
// given multiplicities: counts the tables whose sum exceeds u into report->overflow
hipError_t launch_permuted_sums(const uint32_t *m, uint64_t pitch, uint32_t T, uint32_t u, size_t n_tables, PermutedReport *report,
                                hipStream_t stream);
// the index arrays and heads of a group from its multiplicities
hipError_t launch_permuted_prepare(const PermutedParams &p, hipStream_t stream);
// n_tables value tables of T cells: val(t) = t (RANGE), t * theta + spread(t) (SPREAD) or t + spread(t) * theta
// (THETA_ON_SPREAD); thetas: n_tables x 8 u32, as stored (unused for RANGE)
hipError_t launch_permuted_values(uint4 *values, const uint32_t *thetas, uint32_t kind, uint32_t T, size_t n_tables, bool montgomery,
                                  hipStream_t stream);
// A' and S' of the group, tile by tile -- or nothing at all where the report carries the flag
hipError_t launch_permuted_write(const PermutedParams &p, hipStream_t stream);

}  // namespace hsw
#endif
