// hsw_permuted_value.hpp -- the compressed value of a table row in a permuted lookup pair (hsw_gadget_lookup_permuted).
//
// halo2 folds the expressions of a lookup argument with the challenge theta, acc * theta + expr.  The spread argument
// has [dense, spread], so row t is val(t) = t * theta + spread(t); the range argument has one expression, val(t) = t.
// Both factors next to theta are small (t < 2^16, spread(t) < 2^32), so a value costs ONE 32 x 256-bit multiply with
// reduction mod p -- mont_from_u64's problem (hsw_expand.hpp) with the stored theta in place of R -- and one add of
// the other term in the representation of the cells:  repr(s * theta + x) = s * repr(theta) + repr(x), where repr(x)
// is x itself (canonical) or x * R mod p (Montgomery: the same multiply with R for theta).  The same routine serves
// both representations.  Host- and device-callable: tests/cpp/permuted_index_check.cpp checks it against shift-and-add.
#ifndef HSW_PERMUTED_VALUE_HPP
#define HSW_PERMUTED_VALUE_HPP
#include <cstdint>

#include "hsw_permuted_index.hpp"

namespace hsw {

struct PFe { uint32_t l[8]; };     // little-endian 32-bit limbs, a value below p

#define HSW_PV_P {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}

HSW_PHD bool pfe_below_p(const PFe &a) {
    const uint32_t P[8] = HSW_PV_P;
    for (int j = 7; j >= 0; j--) if (a.l[j] != P[j]) return a.l[j] < P[j];
    return false;
}
// a - p if a >= p (a < 2p)
HSW_PHD PFe pfe_reduce_once(const PFe &a) {
    const uint32_t P[8] = HSW_PV_P;
    PFe d;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] - P[j] - br;
        d.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    return br ? a : d;
}
// a + b mod p for a, b < p (the sum is below 2p < 2^255: no carry out)
HSW_PHD PFe pfe_add(const PFe &a, const PFe &b) {
    PFe s;
    uint64_t cy = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] + b.l[j] + cy;
        s.l[j] = (uint32_t)x;
        cy = x >> 32;
    }
    return pfe_reduce_once(s);
}
// s * a mod p for a < p and any 32-bit s.  t = s * a < 2^32 p; one Barrett step with mu = floor(2^288 / p) on the top
// 64 bits of t gives q^ = q or q - 1 (t / p - (t >> 224) mu / 2^64 < 2^-29 + 2^-2.4 < 1), so t - q^ p < 2p: exactly one
// conditional subtraction -- mont_from_u64's argument, which never used that its multiplicand is R.
HSW_PHD PFe pfe_mul_small(uint32_t s, const PFe &a) {
    const uint32_t P[8] = HSW_PV_P;
    uint32_t t[9];
    uint64_t acc = 0;
    for (int j = 0; j < 8; j++) { acc = (uint64_t)s * a.l[j] + (acc >> 32); t[j] = (uint32_t)acc; }
    t[8] = (uint32_t)(acc >> 32);
    // q = floor((t >> 224) * mu / 2^64), mu = 5 * 2^32 + MU0
    const uint32_t MU0 = 0x4a474626u;
    uint64_t mid = (uint64_t)t[7] * MU0;
    mid = (uint64_t)t[8] * MU0 + (mid >> 32);
    mid = (uint64_t)t[7] * 5u + mid;
    const uint32_t q = t[8] * 5u + (uint32_t)(mid >> 32);
    PFe r;
    acc = 0;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {                                // (t - q p) mod 2^256: the true value is below 2p
        acc = (uint64_t)q * P[j] + (acc >> 32);
        const uint64_t x = (uint64_t)t[j] - (uint32_t)acc - br;
        r.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    return pfe_reduce_once(r);
}
// spread.rs:169-189 for a dense value below 2^16: bit b of t at bit 2 b
HSW_PHD uint32_t pfe_spread_of(uint32_t t) {
    t = (t | (t << 8)) & 0x00ff00ffu;
    t = (t | (t << 4)) & 0x0f0f0f0fu;
    t = (t | (t << 2)) & 0x33333333u;
    return (t | (t << 1)) & 0x55555555u;
}
// a small integer in the representation of the cells
HSW_PHD PFe pfe_repr(uint32_t x, bool montgomery) {
    const PFe R{{0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}};   // 2^256 mod p
    if (montgomery) return pfe_mul_small(x, R);
    return PFe{{x, 0, 0, 0, 0, 0, 0, 0}};
}
// The cell of table row t.  kind: 0 = t, 1 = t * theta + spread(t), 2 = t + spread(t) * theta (PERMUTED_VALUE_* of
// hsw_lookup_permuted.h); theta as stored (below p)
HSW_PHD PFe permuted_value(uint32_t kind, uint32_t t, const PFe &theta, bool montgomery) {
    if (kind == 0) return pfe_repr(t, montgomery);
    const uint32_t sp = pfe_spread_of(t);
    if (kind == 1) return pfe_add(pfe_mul_small(t, theta), pfe_repr(sp, montgomery));
    return pfe_add(pfe_mul_small(sp, theta), pfe_repr(t, montgomery));
}

}  // namespace hsw
#endif
