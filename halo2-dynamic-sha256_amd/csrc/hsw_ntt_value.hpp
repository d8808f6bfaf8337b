// hsw_ntt_value.hpp -- the index rules of the Fr NTT of device columns (hsw_gadget_ntt, include/hsw.h).
//
//   out[i] = sum_{j<N} a[j] w^(i j),  N = 2^L, natural order in and out, in n launches over the L bits of j.
// The bits of j are cut into DIGITS, digit 0 the top one: j = sum_k j_k S_k with S_k = 2^(bits below digit k), and the
// output index is the digits in reverse: i = sum_k i_k T_k with T_k = 2^(bits of the digits before k).  Then
//   i j = sum_k i_k j_k (N / N_k)  +  sum_{m<k} i_m T_m j_k S_k      (mod N; the terms with m > k are multiples of N)
// so launch k is a DFT of size N_k = 2^(bits of digit k) over digit k with the root w^(N / N_k), after every point was
// multiplied by the inter-launch twiddle w^(S_k j_k I), I = sum_{m<k} i_m T_m -- launch 0 has none.
// Between launches a point lies where it lay: launch k leaves i_k (in natural bit order) in the address bits that held
// j_k.  Only the last launch moves points, to the digit-reversed address, which is the natural output index.
// A workgroup holds a TILE of up to 2^NTT_TILE_LOG points, local index l = (hi << lo_bits) | lo:
//   launch k, not the last   hi = digit k, all of it (address bits from hs on); lo = as many of the lowest address bits
//                            as still fit, so that loads and stores go in runs of 2^lo_bits cells; the DFT is over hi
//   the last launch          lo = the last digit, all of it: the DFT is over lo; hi = as many of the lowest bits of
//                            digit 0 as fit (address bits from hs on).  These are the lowest bits of the OUTPUT index,
//                            so that the stores go in runs of 2^hi_bits cells
// and the workgroup's index is spread over the address bits the tile leaves free.  Inside the tile the DFT is radix-2
// decimation in frequency over the bits of the field, top bit first: at field bit fb the pair (l, l + bit) becomes
// (x + y, (x - y) w^(pos << (L - 1 - fb))) with pos the field's bits below fb; field bit 0 multiplies by 1.  That leaves
// the field bit-reversed, which the store undoes by reading the tile at the reversed place.
// The digits: L <= pass_log is ONE digit.  Otherwise every launch reads or writes at a stride, and runs of four cells
// cost two bits of the tile: digits of at most max(1, pass_log - 2) bits, as few as it takes, sizes balanced.
// Host- and device-callable: hsw_ntt.hip is built from these, hsw_gadget_ntt.cpp stages with them,
// tests/cpp/ntt_value_check.cpp runs the launches point for point on the CPU against the sum above.
#ifndef HSW_NTT_VALUE_HPP
#define HSW_NTT_VALUE_HPP
#include "hsw_fr_mul.hpp"

namespace hsw {

enum : uint32_t {
    NTT_MAX_LOG = 28,            // the two-adicity of Fr
    NTT_TILE_LOG = 10,           // points of a workgroup's tile, log2; the greatest pass_log
    NTT_THREADS = 256,
    NTT_POINTS = 4,              // points of a thread: NTT_THREADS * NTT_POINTS = 2^NTT_TILE_LOG
    NTT_WINDOWS = 7,             // 4-bit windows of an exponent below 2^28
    NTT_SHIFT_AFTER = 1u,        // HSW_NTT_SHIFT_AFTER
    NTT_CELL_NOT_BELOW_P = 4u,   // HSW_NTT_CELL_NOT_BELOW_P
};

// The digits of a transform, the top one first
struct NttPlan {
    uint32_t log_n, n_pass;
    uint8_t bits[NTT_MAX_LOG];
};

// The geometry of one launch
struct NttPass {
    uint32_t log_n, k, n_pass;
    uint32_t field_bits, field_shift;      // the DFT is over bits [field_shift, field_shift + field_bits) of l
    uint32_t lo_bits, hi_bits, hs;         // address = base + lo + (hi << hs)
    uint32_t below;                        // log2 S_k
    uint32_t reserved_;
};

// base^(v << 4 w) for the 4-bit windows of an exponent, in Montgomery form
struct NttWindows { PFe v[NTT_WINDOWS][16]; };

HSW_PHD uint32_t ntt_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// false: log_n or pass_log out of range.  pass_log 0 is NTT_TILE_LOG
HSW_PHD bool ntt_plan(uint32_t log_n, uint32_t pass_log, NttPlan &plan) {
    if (log_n < 1 || log_n > NTT_MAX_LOG || pass_log > NTT_TILE_LOG) return false;
    const uint32_t p = pass_log ? pass_log : (uint32_t)NTT_TILE_LOG;
    plan.log_n = log_n;
    for (uint32_t k = 0; k < NTT_MAX_LOG; k++) plan.bits[k] = 0;
    if (log_n <= p) { plan.n_pass = 1; plan.bits[0] = (uint8_t)log_n; return true; }
    const uint32_t s = p > 3 ? p - 2 : 1u, n = (log_n + s - 1) / s;
    plan.n_pass = n;
    for (uint32_t k = 0; k < n; k++) plan.bits[k] = (uint8_t)(log_n / n + (k < log_n % n ? 1u : 0u));
    return true;
}

HSW_PHD NttPass ntt_pass(const NttPlan &plan, uint32_t k) {
    NttPass g{};
    g.log_n = plan.log_n; g.k = k; g.n_pass = plan.n_pass;
    uint32_t above = 0;
    for (uint32_t m = 0; m < k; m++) above += plan.bits[m];
    const uint32_t d = plan.bits[k];
    g.below = plan.log_n - above - d;
    g.field_bits = d;
    if (k + 1 < plan.n_pass) {
        g.lo_bits = ntt_min(NTT_TILE_LOG - d, g.below);
        g.hi_bits = d; g.hs = g.below; g.field_shift = g.lo_bits;
    } else {
        g.lo_bits = d; g.field_shift = 0;
        g.hi_bits = k ? ntt_min(NTT_TILE_LOG - d, plan.bits[0]) : 0u;
        g.hs = k ? plan.log_n - plan.bits[0] : plan.log_n;
    }
    return g;
}

HSW_PHD uint32_t ntt_tile_log(const NttPass &g) { return g.lo_bits + g.hi_bits; }
HSW_PHD uint32_t ntt_workgroups(const NttPass &g) { return 1u << (g.log_n - ntt_tile_log(g)); }
// the address of local index 0 of a workgroup: its index spread over the bits between lo and hi, then above hi
HSW_PHD uint32_t ntt_base(const NttPass &g, uint32_t wg) {
    const uint32_t mid = g.hs - g.lo_bits;
    return ((wg & ((1u << mid) - 1u)) << g.lo_bits) | ((wg >> mid) << (g.hs + g.hi_bits));
}
HSW_PHD uint32_t ntt_offset(const NttPass &g, uint32_t l) { return (l & ((1u << g.lo_bits) - 1u)) + ((l >> g.lo_bits) << g.hs); }
HSW_PHD uint32_t ntt_field(const NttPass &g, uint32_t l) { return (l >> g.field_shift) & ((1u << g.field_bits) - 1u); }

HSW_PHD uint32_t ntt_reverse(uint32_t x, uint32_t bits) {
    x = ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
    x = ((x & 0x33333333u) << 2) | ((x >> 2) & 0x33333333u);
    x = ((x & 0x0f0f0f0fu) << 4) | ((x >> 4) & 0x0f0f0f0fu);
    x = ((x & 0x00ff00ffu) << 8) | ((x >> 8) & 0x00ff00ffu);
    x = (x << 16) | (x >> 16);
    return bits ? x >> (32 - bits) : 0u;
}
// l with its field reversed
HSW_PHD uint32_t ntt_reverse_field(const NttPass &g, uint32_t l) {
    const uint32_t mask = ((1u << g.field_bits) - 1u) << g.field_shift;
    return (l & ~mask) | (ntt_reverse(ntt_field(g, l), g.field_bits) << g.field_shift);
}
// The local index (field in natural order) that the lam-th store of a workgroup writes: consecutive lam are consecutive
// cells of the destination -- lo, except in the last launch of several, where the runs of the output go along hi
HSW_PHD uint32_t ntt_store_local(const NttPass &g, uint32_t lam) {
    if (g.k + 1 < g.n_pass || g.k == 0) return lam;
    return ((lam & ((1u << g.hi_bits) - 1u)) << g.lo_bits) | (lam >> g.hi_bits);
}

// I = sum_{m<k} i_m T_m of the point at `addr` before launch k
HSW_PHD uint32_t ntt_done_index(const NttPlan &plan, uint32_t k, uint32_t addr) {
    uint32_t I = 0, above = 0;
    for (uint32_t m = 0; m < k; m++) {
        const uint32_t d = plan.bits[m];
        I |= ((addr >> (plan.log_n - above - d)) & ((1u << d) - 1u)) << above;
        above += d;
    }
    return I;
}
// the digits of addr in reverse: where the last launch stores
HSW_PHD uint32_t ntt_out_index(const NttPlan &plan, uint32_t addr) { return ntt_done_index(plan, plan.n_pass, addr); }
// the exponent of the inter-launch twiddle of a point, below N
HSW_PHD uint32_t ntt_twiddle_exponent(const NttPass &g, uint32_t digit, uint32_t done) { return (digit * done) << g.below; }
// the exponent, below N / 2, of the butterfly at field bit fb whose lower point is l
HSW_PHD uint32_t ntt_stage_exponent(const NttPass &g, uint32_t l, uint32_t fb) { return (ntt_field(g, l) & ((1u << fb) - 1u)) << (g.log_n - 1 - fb); }
// the first of a thread's four points of a step whose lower free bit is ql: t with two zero bits let in there
HSW_PHD uint32_t ntt_step_local(uint32_t t, uint32_t ql) { return ((t >> ql) << (ql + 2)) | (t & ((1u << ql) - 1u)); }

HSW_PHD void ntt_stage_windows(const PFe &base_mont, NttWindows &win) {
    PFe step = base_mont;                                          // base^(2^(4 w))
    for (uint32_t w = 0; w < NTT_WINDOWS; w++) {
        win.v[w][0] = fr_one_mont();
        for (uint32_t v = 1; v < 16; v++) win.v[w][v] = fr_mont_mul(win.v[w][v - 1], step);
        step = fr_mont_mul(win.v[w][15], step);
    }
}
// base^e, e < 2^28: a multiply per window of e that is not 0, but the lowest
HSW_PHD PFe ntt_power(const NttWindows &win, uint32_t e) {
    PFe r = win.v[0][e & 15u];
    for (uint32_t w = 1; w < NTT_WINDOWS; w++) {
        const uint32_t nib = (e >> (4 * w)) & 15u;
        if (nib) r = fr_mont_mul(r, win.v[w][nib]);
    }
    return r;
}
// w^e, e < N, from the table of the N / 2 first powers (N = 2: its one entry is 1)
HSW_PHD PFe ntt_twiddle(const PFe *table, uint32_t log_n, uint32_t e) {
    const uint32_t half = 1u << (log_n - 1);
    if (e < half) return table[e];
    return fr_sub(fr_zero(), table[e - half]);
}
HSW_PHD void ntt_butterfly(PFe &x, PFe &y, const PFe *table, uint32_t e, bool multiply) {
    const PFe u = fr_add(x, y), v = fr_sub(x, y);
    x = u;
    y = multiply ? fr_mont_mul(v, table[e]) : v;
}

// a stored constant (below p) in Montgomery form
HSW_PHD PFe ntt_to_mont(const PFe &stored, bool montgomery) { return montgomery ? stored : fr_to_mont(stored); }
// whether w (Montgomery form) is a primitive 2^log_n-th root of unity: w^(N / 2) = p - 1
HSW_PHD bool ntt_root_is_primitive(const PFe &w_mont, uint32_t log_n) {
    PFe x = w_mont;
    for (uint32_t b = 1; b < log_n; b++) x = fr_mont_mul(x, x);
    return fr_equal(x, fr_sub(fr_zero(), fr_one_mont()));
}

}  // namespace hsw
#endif
