// hsw_permuted_index.hpp -- the index rules of halo2's permuted lookup pair (hsw_gadget_lookup_permuted, include/hsw.h).
//
// One argument: a table of T rows, u usable rows, multiplicities m[t] with E = sum m <= u.  Unassigned rows look row 0
// up: m'[0] = m[0] + (u - E), m'[t] = m[t] otherwise, off[t] the exclusive prefix sum of m' (off[T] = u).
//   A'[i]      = row t                   for off[t] <= i < off[t] + m'[t]
//   S'[off[t]] = row t                   for every used row (m'[t] > 0): the FIRST position of its run
//   S'[i]      = the r-th spare row      for the r-th REPEATED position i (every other one), both ascending; the spare
//                rows are row 0 (u - T) + [m'[0] = 0] times (the table column's padding repeats row 0), then every
//                t > 0 with m'[t] = 0 once.
// Nothing is sorted: the pair is described by three compact arrays, built from m in one pass,
//   used_off[j], used_row[j]   the j-th used row (ascending) and the off of it; used_off[used] = u
//   spare_row[q]               the q-th row t > 0 with m'[t] = 0
// and a position is resolved by the three functions at the end: the search position -> run, the rank of a repeated
// position, the rank -> spare row map.  Plain integer functions, host- and device-callable like hsw_flush_bounds.hpp:
// hsw_lookup_permuted.hip builds and reads the arrays through them (a chunk of rows per thread, the chunk bases from a
// workgroup scan), tests/cpp/permuted_index_check.cpp runs the same functions against a brute-force model.
#ifndef HSW_PERMUTED_INDEX_HPP
#define HSW_PERMUTED_INDEX_HPP
#include <cstddef>
#include <cstdint>
#if defined(__HIPCC__)
#define HSW_PHD __host__ __device__ __forceinline__
#else
#define HSW_PHD inline
#endif

namespace hsw {

// What one argument's arrays hold: `used` runs, `zeros` copies of row 0 at the head of the spare rows
struct PermutedHead { uint32_t used, zeros, ok, reserved_; };

// u32 words of one argument's arrays, back to back: used_off[T + 1], used_row[T], spare_row[T]
HSW_PHD size_t permuted_index_words(uint32_t T) { return 3 * (size_t)T + 4; }

// m'[t]: pad0 = u - E goes to row 0
HSW_PHD uint32_t permuted_mprime(const uint32_t *m, uint32_t t, uint32_t pad0) { return m[t] + (t == 0 ? pad0 : 0u); }

// Rows [lo, hi) of the table: the positions they take, how many of them are used, how many are spare (t > 0, m' = 0)
struct PermutedSums { uint32_t rows, used, spare; };
HSW_PHD PermutedSums permuted_chunk_sums(const uint32_t *m, uint32_t lo, uint32_t hi, uint32_t pad0) {
    PermutedSums s{0, 0, 0};
    for (uint32_t t = lo; t < hi; t++) {
        const uint32_t mp = permuted_mprime(m, t, pad0);
        s.rows += mp;
        if (mp) s.used++; else if (t) s.spare++;
    }
    return s;
}
// ... and their entries of the three arrays, `base` being the sums of the rows [0, lo)
HSW_PHD void permuted_chunk_write(const uint32_t *m, uint32_t lo, uint32_t hi, uint32_t pad0, PermutedSums base, uint32_t *used_off,
                                  uint32_t *used_row, uint32_t *spare_row) {
    for (uint32_t t = lo; t < hi; t++) {
        const uint32_t mp = permuted_mprime(m, t, pad0);
        if (mp) { used_off[base.used] = base.rows; used_row[base.used] = t; base.used++; base.rows += mp; }
        else if (t) spare_row[base.spare++] = t;
    }
}
// the head, from the sums of the whole table: used_off[used] = u is the caller's to write
HSW_PHD PermutedHead permuted_head(const uint32_t *m, uint32_t T, uint32_t u, uint32_t pad0, PermutedSums all) {
    return PermutedHead{all.used, (u - T) + (permuted_mprime(m, 0, pad0) == 0 ? 1u : 0u), 1u, 0u};
}

// position -> run: the last j of [lo, hi) with used_off[j] <= i (used_off[lo] <= i is the caller's to know)
HSW_PHD uint32_t permuted_find(const uint32_t *used_off, uint32_t lo, uint32_t hi, uint32_t i) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (used_off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// the rank of position i of run j among the repeated positions (i != used_off[j]): j + 1 first positions lie at or before it
HSW_PHD uint32_t permuted_rank(uint32_t i, uint32_t j) { return i - (j + 1u); }
// rank -> spare row
HSW_PHD uint32_t permuted_spare(uint32_t rank, uint32_t zeros, const uint32_t *spare_row) {
    return rank < zeros ? 0u : spare_row[rank - zeros];
}
// Row i of a tile of output rows that starts in run j0, through the window win[0 .. n] = used_off[j0 .. j0 + n] (n >= 1
// runs; win[n] is the next run's offset or the sentinel): the table row of A'[i] and of S'[i].  Every run has at least
// one row, so a tile of R rows needs n = min(R, used - j0) runs
HSW_PHD void permuted_rows(const uint32_t *win, uint32_t n, uint32_t j0, uint32_t i, const uint32_t *used_row, const uint32_t *spare_row,
                           uint32_t zeros, uint32_t *input_row, uint32_t *table_row) {
    const uint32_t k = permuted_find(win, 0, n, i);
    const uint32_t t = used_row[j0 + k];
    *input_row = t;
    *table_row = i == win[k] ? t : permuted_spare(permuted_rank(i, j0 + k), zeros, spare_row);
}

}  // namespace hsw
#endif
