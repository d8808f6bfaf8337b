// hsw_msm.h -- launch interface of the G1 multi-scalar multiplication of device columns (hsw_msm.hip; hsw_gadget_msm in
// hsw_gadget_msm.cpp is its only caller).
#ifndef HSW_MSM_H
#define HSW_MSM_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_msm_value.hpp"

namespace hsw {

static_assert(MSM_MAX_BUCKETS == (1u << MSM_MAX_WINDOW_BITS) - 1 && MSM_MAX_BUCKETS <= MSM_THREADS, "a thread owns a bucket");
static_assert(sizeof(G1) == 96 && sizeof(G1Affine) == 64, "points are 6 and 4 uint4");

// One column (cells of two uint4 each, 16-byte aligned)
struct MsmColumn {
    const uint4 *cells;            // rows cells are read
    uint32_t rows, reserved_;
};

// what the check launch leaves: the bases of the checked rows with a coordinate not below q, and the lowest of them
struct MsmCheck { uint32_t bad, first; };

struct MsmParams {
    MsmPlan plan;
    const MsmColumn *cols;         // one per column of the group
    uint32_t *status;              // likewise, zeroed by the caller
    const uint4 *bases;            // four uint4 per point: x, y
    uint4 *partial;                // the group's partial buckets, six uint4 per point, at msm_partial_index
    uint4 *windows;                // the group's window points, [column of the group][window]
    uint32_t montgomery, reserved_;
};

// counts the bases of rows [0, rows) with a coordinate not below q into *check ({0, ~0} before)
hipError_t launch_msm_check(const uint4 *bases, uint32_t rows, MsmCheck *check, hipStream_t stream);
// the buckets of every (slice, window, column) of the group
hipError_t launch_msm_accumulate(const MsmParams &p, uint32_t n_columns, hipStream_t stream);
// the window points of every (window, column) of the group
hipError_t launch_msm_reduce(const MsmParams &p, uint32_t n_columns, hipStream_t stream);

}  // namespace hsw
#endif
