// hsw_msm_value.hpp -- the rules of the G1 multi-scalar multiplication of device columns (hsw_gadget_msm, include/hsw.h).
//
//   out = sum_{j < rows} a[j] * G[j],  a[j] the canonical integer below r of cell j, by Pippenger's bucket method:
// the 254 bits of a scalar are cut into W = ceil(254 / c) unsigned DIGITS of c bits, digit 0 the lowest (the top one may
// be short), and the rows into SLICES of slice_rows rows.  Then, with B[w][s][d] = the sum of the bases of slice s whose
// digit w is d (digit 0 is dropped),
//   accumulate   a workgroup per (slice, window, column) forms its 2^c - 1 buckets B[w][s][1 ..], walking the slice in
//                CHUNKS of at most MSM_CHUNK_ROWS rows: the chunk's rows are counting-sorted by digit (histogram,
//                msm_bucket_start, scatter), bucket d then adds the bases of its list with the mixed formula
//   reduce       a workgroup per (window, column) sums the slices' buckets, B[w][d] = sum_s B[w][s][d], and forms the
//                window's point S[w] = sum_d d * B[w][d] as the sum of the suffix sums (msm_weighted_sum)
//   finish       Horner over the windows from the top one down -- c doublings, one addition -- and one inversion
// Everything here is a value or an index, never a memory access: hsw_msm.hip is built from these, hsw_gadget_msm.cpp
// plans and finishes with them, and tests/cpp/msm_value_check.cpp runs the launches on the CPU against double-and-add.
#ifndef HSW_MSM_VALUE_HPP
#define HSW_MSM_VALUE_HPP
#include "hsw_fr_mul.hpp"
#include "hsw_g1.hpp"

namespace hsw {

enum : uint32_t {
    MSM_SCALAR_BITS = 254,           // r < 2^254
    MSM_MAX_WINDOW_BITS = 8,         // HSW_MSM_MAX_WINDOW_BITS: a thread owns one bucket, 2^c - 1 <= MSM_THREADS
    MSM_THREADS = 256,
    MSM_MAX_BUCKETS = 255,
    MSM_MIN_SLICE_ROWS = 64,
    MSM_CHUNK_ROWS = 4096,           // rows counting-sorted in LDS at a time
    MSM_MAX_LOG_BASES = 28,
    MSM_DEFAULT_WINDOW_BITS = 8,
    MSM_DEFAULT_SLICE_ROWS = 4096,
    MSM_DEFAULT_MAX_SLICES = 1024,   // the default slice doubles until a column has no more slices than this
    MSM_CELL_NOT_BELOW_P = 4u,       // HSW_MSM_CELL_NOT_BELOW_P
    MSM_BASE_NOT_BELOW_Q = 8u,       // HSW_MSM_BASE_NOT_BELOW_Q
};

struct MsmPlan {
    uint32_t window_bits, windows, buckets;    // c, W = ceil(254 / c), 2^c - 1
    uint32_t slice_rows, slices, chunk_rows;   // slices of the tallest column (at least 1); chunk = min(slice, MSM_CHUNK_ROWS)
};

HSW_PHD uint32_t msm_slices(uint32_t rows, uint32_t slice_rows) { return (uint32_t)(((uint64_t)rows + slice_rows - 1) / slice_rows); }

// false: window_bits or slice_rows outside its range.  max_rows: the tallest column; 0 picks the library's choice
HSW_PHD bool msm_plan(uint32_t max_rows, uint32_t window_bits, uint32_t slice_rows, MsmPlan &plan) {
    if (window_bits > MSM_MAX_WINDOW_BITS) return false;
    if (slice_rows && (slice_rows < MSM_MIN_SLICE_ROWS || slice_rows > (1u << MSM_MAX_LOG_BASES) || (slice_rows & (slice_rows - 1)))) return false;
    const uint32_t c = window_bits ? window_bits : (uint32_t)MSM_DEFAULT_WINDOW_BITS;
    uint32_t s = slice_rows;
    if (!s) for (s = MSM_DEFAULT_SLICE_ROWS; msm_slices(max_rows, s) > MSM_DEFAULT_MAX_SLICES; s *= 2) {}
    plan.window_bits = c;
    plan.windows = (MSM_SCALAR_BITS + c - 1) / c;
    plan.buckets = (1u << c) - 1;
    plan.slice_rows = s;
    plan.slices = max_rows ? msm_slices(max_rows, s) : 1u;
    plan.chunk_rows = s < MSM_CHUNK_ROWS ? s : (uint32_t)MSM_CHUNK_ROWS;
    return true;
}

// the canonical integer of a stored cell; false if the cell is not an encoding below r
HSW_PHD bool msm_canonical(const PFe &cell, bool montgomery, PFe &a) {
    if (!pfe_below_p(cell)) return false;
    a = montgomery ? fr_from_mont(cell) : cell;
    return true;
}

// digit w of a canonical scalar: bits [w c, w c + c), those at and above 256 being 0
HSW_PHD uint32_t msm_digit(const PFe &a, uint32_t w, uint32_t c) {
    const uint32_t bit = w * c, limb = bit >> 5, sh = bit & 31u;
    uint32_t lo = 0, hi = 0;                                               // (selected, not indexed: the limbs stay in registers)
    for (uint32_t j = 0; j < 8; j++) {
        if (j == limb) lo = a.l[j];
        if (j == limb + 1) hi = a.l[j];
    }
    return (uint32_t)(((uint64_t)hi << 32 | lo) >> sh) & ((1u << c) - 1);
}

// where the list of bucket d (1 <= d) starts in a chunk's sorted rows: the rows of the digits 1 .. d - 1 before it
HSW_PHD uint32_t msm_bucket_start(const uint32_t *hist, uint32_t d) {
    uint32_t s = 0;
    for (uint32_t k = 1; k < d; k++) s += hist[k];
    return s;
}

// points (96 bytes each) from the start of the partial buckets to bucket d (1 <= d <= buckets) of slice s, window w of
// the group's column gb: slices side by side under a window, so that the reduce launch walks them at one stride
HSW_PHD uint64_t msm_partial_index(const MsmPlan &p, uint32_t gb, uint32_t w, uint32_t s, uint32_t d) {
    return (((uint64_t)gb * p.windows + w) * p.slices + s) * p.buckets + (d - 1);
}
HSW_PHD uint64_t msm_partial_points(const MsmPlan &p) { return (uint64_t)p.windows * p.slices * p.buckets; }   // per column

// sum_d d * B[d - 1] over n buckets: the sum of the suffix sums T_j = sum_{d >= j} B_d
HSW_PHD G1 msm_weighted_sum(const G1 *buckets, uint32_t n) {
    G1 running = g1_identity(), total = g1_identity();
    for (uint32_t d = n; d >= 1; d--) {
        running = g1_add(running, buckets[d - 1]);
        total = g1_add(total, running);
    }
    return total;
}

// sum_w 2^(w c) S[w], from the top window down
HSW_PHD G1 msm_horner(const G1 *windows, uint32_t n_windows, uint32_t c) {
    G1 acc = windows[n_windows - 1];
    for (uint32_t w = n_windows - 1; w-- > 0;) {
        for (uint32_t k = 0; k < c; k++) acc = g1_double(acc);
        acc = g1_add(acc, windows[w]);
    }
    return acc;
}

// the stored form of the result: 64 bytes, zero for the identity
HSW_PHD G1Affine msm_normalise(const G1 &p) { return g1_to_affine(p); }

}  // namespace hsw
#endif
