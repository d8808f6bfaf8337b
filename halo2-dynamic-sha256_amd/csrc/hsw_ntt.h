// hsw_ntt.h -- launch interface of the Fr NTT of device columns (hsw_ntt.hip; hsw_gadget_ntt in hsw_gadget_ntt.cpp is
// its only caller).
#ifndef HSW_NTT_H
#define HSW_NTT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_ntt_value.hpp"

namespace hsw {

static_assert(NTT_THREADS * NTT_POINTS == 1u << NTT_TILE_LOG, "a thread's points fill the tile");

// One column (cells of two uint4 each, 16-byte aligned)
struct NttColumn {
    const uint4 *in;               // rows cells are read, the rest count as 0
    uint4 *out;                    // N cells, written by the last launch only
    uint4 *scratch;                // N cells between the launches (one launch: not used)
    uint32_t rows, reserved_;
};

enum : uint32_t { NTT_OUT_PLAIN = 0, NTT_OUT_SCALE = 1, NTT_OUT_TABLE = 2 };

struct NttParams {
    NttPlan plan;
    NttPass pass;
    const NttColumn *cols;         // one per blockIdx.y
    uint32_t *status;              // likewise, zeroed by the caller
    const PFe *twiddle;            // w^e, e < N / 2, Montgomery form
    const NttWindows *shift;       // g's windows: launch 0 with shift_in, the last launch with NTT_OUT_TABLE
    const PFe *tile_in;            // launch 0 with shift_in: g^(ntt_offset(l))
    const PFe *tile_out;           // NTT_OUT_TABLE: c g^(output offset of the lam-th store)
    PFe scale;                     // NTT_OUT_SCALE: c, Montgomery form
    uint32_t shift_in, out_mode;
};

// T[e] = w^e for e < count from w's windows
hipError_t launch_ntt_twiddles(PFe *table, const NttWindows *windows, uint32_t count, hipStream_t stream);
// launch p.pass.k of the transform of n_columns columns
hipError_t launch_ntt_pass(const NttParams &p, uint32_t n_columns, hipStream_t stream);

}  // namespace hsw
#endif
