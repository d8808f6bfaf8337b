// hsw_fq.hpp -- BN254 Fq, the base field of G1, host- and device-callable.
//
// hsw_fr_mul.hpp's routines over the other modulus: q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47 is
// odd and below 2^254 like p, so the CIOS multiply's bound argument holds word for word (for a, b < q the accumulator
// stays below 2q < 2^255 and ONE conditional subtraction ends it).  Repeated here rather than shared, as hsw_ntt.hip
// repeats the LDS helpers, so that hsw_fr_mul.hpp and every translation unit that includes it stay as they are.
//   fq_mont_mul(a, b) = a b 2^-256 mod q        fq_add, fq_sub, fq_neg        fq_to_mont / fq_from_mont
//   fq_inv(a)         = a^(q-2) in Montgomery form: for a = x R it is x^-1 R; fq_inv(0) = 0
// An element is eight 32-bit limbs, low first, below q.  tests/cpp/g1_check.cpp checks every routine against
// shift-and-add.  hsw_g1.hpp (the curve) is its only user.
#ifndef HSW_FQ_HPP
#define HSW_FQ_HPP
#include <cstdint>

#include "hsw_permuted_index.hpp"

namespace hsw {

struct Fq { uint32_t l[8]; };      // little-endian 32-bit limbs, a value below q

#define HSW_FQ_Q {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}
#define HSW_FQ_R {0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}    // 2^256 mod q
#define HSW_FQ_R2 {0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u}   // 2^512 mod q

HSW_PHD Fq fq_zero() { return Fq{{0, 0, 0, 0, 0, 0, 0, 0}}; }
HSW_PHD Fq fq_one_mont() { return Fq{HSW_FQ_R}; }                        // 1 in Montgomery form
HSW_PHD bool fq_is_zero(const Fq &a) {
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x |= a.l[j];
    return x == 0;
}
HSW_PHD bool fq_equal(const Fq &a, const Fq &b) {
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x |= a.l[j] ^ b.l[j];
    return x == 0;
}
HSW_PHD bool fq_below_q(const Fq &a) {
    const uint32_t Q[8] = HSW_FQ_Q;
    for (int j = 7; j >= 0; j--) if (a.l[j] != Q[j]) return a.l[j] < Q[j];
    return false;
}
// a - q if a >= q (a < 2q)
HSW_PHD Fq fq_reduce_once(const Fq &a) {
    const uint32_t Q[8] = HSW_FQ_Q;
    Fq d;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] - Q[j] - br;
        d.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    return br ? a : d;
}
// a + b mod q for a, b < q (the sum is below 2q < 2^255: no carry out)
HSW_PHD Fq fq_add(const Fq &a, const Fq &b) {
    Fq s;
    uint64_t cy = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] + b.l[j] + cy;
        s.l[j] = (uint32_t)x;
        cy = x >> 32;
    }
    return fq_reduce_once(s);
}
// a - b mod q for a, b < q
HSW_PHD Fq fq_sub(const Fq &a, const Fq &b) {
    const uint32_t Q[8] = HSW_FQ_Q;
    Fq d;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] - b.l[j] - br;
        d.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    const uint32_t mask = 0u - (uint32_t)br;                             // a < b: add q back
    uint64_t cy = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)d.l[j] + (Q[j] & mask) + cy;
        d.l[j] = (uint32_t)x;
        cy = x >> 32;
    }
    return d;
}
HSW_PHD Fq fq_neg(const Fq &a) { return fq_sub(fq_zero(), a); }
// a b 2^-256 mod q for a, b < q (CIOS, as fr_mont_mul)
HSW_PHD Fq fq_mont_mul(const Fq &a, const Fq &b) {
    const uint32_t Q[8] = HSW_FQ_Q;
    const uint32_t NQ0 = 0xe4866389u;                                     // -q^-1 mod 2^32
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
        const uint32_t m = t[0] * NQ0;                                    // t += m * q, then t >>= 32: the low limb is 0
        acc = (uint64_t)m * Q[0] + t[0];
        for (int j = 1; j < 8; j++) {
            acc = (uint64_t)m * Q[j] + t[j] + (acc >> 32);
            t[j - 1] = (uint32_t)acc;
        }
        acc = (uint64_t)t8n + (acc >> 32);
        t[7] = (uint32_t)acc;
        t8 = t9 + (uint32_t)(acc >> 32);
    }
    Fq r;                                                                 // below 2q < 2^255: t8 == 0
    for (int j = 0; j < 8; j++) r.l[j] = t[j];
    return fq_reduce_once(r);
}
HSW_PHD Fq fq_to_mont(const Fq &a) { return fq_mont_mul(a, Fq{HSW_FQ_R2}); }
HSW_PHD Fq fq_from_mont(const Fq &a) { return fq_mont_mul(a, Fq{{1, 0, 0, 0, 0, 0, 0, 0}}); }
// a^(q-2) for a in Montgomery form, the result in Montgomery form (Fermat; no branch on a: the exponent is a constant)
HSW_PHD Fq fq_inv(const Fq &a) {
    const uint32_t E[8] = {0xd87cfd45u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};   // q - 2
    Fq r = a;                                                             // bit 253, the top one
    for (int bit = 252; bit >= 0; bit--) {
        r = fq_mont_mul(r, r);
        if ((E[bit >> 5] >> (bit & 31)) & 1u) r = fq_mont_mul(r, a);
    }
    return r;
}

}  // namespace hsw
#endif
