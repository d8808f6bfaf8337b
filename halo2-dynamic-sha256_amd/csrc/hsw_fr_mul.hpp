// hsw_fr_mul.hpp -- BN254 Fr arithmetic with a full 256 x 256-bit Montgomery multiply, host- and device-callable.
//
// hsw_mont.hpp and hsw_permuted_value.hpp multiply a field element by a 32/64-bit one; hsw_fr.hpp multiplies two, on the
// host only.  This is the device's: the same element type as hsw_permuted_value.hpp (PFe, eight 32-bit limbs, below p)
// and plain C++ -- (uint64_t)a * b + c + d cannot overflow (2^64 - 1 at the most) and compiles to one v_mad_u64_u32 with
// a 64-bit add on gfx950, so a multiply is 2 x 64 of them in two interleaved carry chains (CIOS: one row of a * b[i],
// one row of m * p, the accumulator shifted by a limb).  p < 2^254, so for a, b < p the accumulator stays below 2p and
// ONE conditional subtraction ends it; inputs that are not below p give garbage, never an out-of-range access.
//   fr_mont_mul(a, b) = a b 2^-256 mod p        fr_add, fr_sub        fr_to_mont / fr_from_mont
//   fr_inv(a)         = a^(p-2) in Montgomery form: for a = x R it is x^-1 R; fr_inv(0) = 0
// Nothing here knows of a kernel: hsw_product_value.hpp (the lookup argument's grand product) is its first user, the
// permutation argument's product the next.  tests/cpp/fr_mul_check.cpp checks every routine against shift-and-add.
#ifndef HSW_FR_MUL_HPP
#define HSW_FR_MUL_HPP
#include <cstdint>

#include "hsw_permuted_value.hpp"

namespace hsw {

#define HSW_FR_R {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}    // 2^256 mod p
#define HSW_FR_R2 {0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u}   // 2^512 mod p
#define HSW_FR_R3 {0xb4bf0040u, 0x5e94d8e1u, 0x1cfbb6b8u, 0x2a489cbeu, 0xa19fcfedu, 0x893cc664u, 0x7fcc657cu, 0x0cf8594bu}   // 2^768 mod p

HSW_PHD PFe fr_zero() { return PFe{{0, 0, 0, 0, 0, 0, 0, 0}}; }
HSW_PHD PFe fr_one_mont() { return PFe{HSW_FR_R}; }                     // 1 in Montgomery form
HSW_PHD bool fr_is_zero(const PFe &a) {
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x |= a.l[j];
    return x == 0;
}
HSW_PHD bool fr_equal(const PFe &a, const PFe &b) {
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x |= a.l[j] ^ b.l[j];
    return x == 0;
}
HSW_PHD PFe fr_add(const PFe &a, const PFe &b) { return pfe_add(a, b); }
// a - b mod p for a, b < p
HSW_PHD PFe fr_sub(const PFe &a, const PFe &b) {
    const uint32_t P[8] = HSW_PV_P;
    PFe d;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] - b.l[j] - br;
        d.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    const uint32_t mask = 0u - (uint32_t)br;                             // a < b: add p back
    uint64_t cy = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)d.l[j] + (P[j] & mask) + cy;
        d.l[j] = (uint32_t)x;
        cy = x >> 32;
    }
    return d;
}
// a b 2^-256 mod p for a, b < p (CIOS, Koc et al. 1996: the accumulator t has 8 limbs and two carry words)
HSW_PHD PFe fr_mont_mul(const PFe &a, const PFe &b) {
    const uint32_t P[8] = HSW_PV_P;
    const uint32_t NP0 = 0xefffffffu;                                     // -p^-1 mod 2^32
    uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t t8 = 0;
    for (int i = 0; i < 8; i++) {
        uint64_t acc = 0;
        for (int j = 0; j < 8; j++) {                                     // t += a * b[i]
            acc = (uint64_t)a.l[j] * b.l[i] + t[j] + (acc >> 32);
            t[j] = (uint32_t)acc;
        }
        acc = (uint64_t)t8 + (acc >> 32);
        const uint32_t t8n = (uint32_t)acc, t9 = (uint32_t)(acc >> 32);
        const uint32_t m = t[0] * NP0;                                    // t += m * p, then t >>= 32: the low limb is 0
        acc = (uint64_t)m * P[0] + t[0];
        for (int j = 1; j < 8; j++) {
            acc = (uint64_t)m * P[j] + t[j] + (acc >> 32);
            t[j - 1] = (uint32_t)acc;
        }
        acc = (uint64_t)t8n + (acc >> 32);
        t[7] = (uint32_t)acc;
        t8 = t9 + (uint32_t)(acc >> 32);
    }
    PFe r;                                                                // below 2p < 2^255: t8 == 0
    for (int j = 0; j < 8; j++) r.l[j] = t[j];
    return pfe_reduce_once(r);
}
HSW_PHD PFe fr_to_mont(const PFe &a) { return fr_mont_mul(a, PFe{HSW_FR_R2}); }
HSW_PHD PFe fr_from_mont(const PFe &a) { return fr_mont_mul(a, PFe{{1, 0, 0, 0, 0, 0, 0, 0}}); }
// a^(p-2) for a in Montgomery form, the result in Montgomery form: 253 squarings and one multiply per set bit of p - 2
// below its top one (about 380 multiplies).  No branch on a: the exponent is a constant
HSW_PHD PFe fr_inv(const PFe &a) {
    const uint32_t E[8] = {0xefffffffu, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};   // p - 2
    PFe r = a;                                                            // bit 253, the top one
    for (int bit = 252; bit >= 0; bit--) {
        r = fr_mont_mul(r, r);
        if ((E[bit >> 5] >> (bit & 31)) & 1u) r = fr_mont_mul(r, a);
    }
    return r;
}

}  // namespace hsw
#endif
