// hsw_g1.hpp -- BN254 G1 (y^2 = x^3 + 3 over Fq, prime order r = the Fr modulus), host- and device-callable.
//
// A point in flight is homogeneous projective (X : Y : Z) with the identity (0 : 1 : 0); a stored point is affine
// (x, y) with (0, 0) for the identity (assumption A7 of DESIGN.md: the in-memory form of halo2curves' G1Affine).  Every
// coordinate is in Montgomery form mod q.  The three formulas are the COMPLETE ones of Renes, Costello and Batina
// ("Complete addition formulas for prime order elliptic curves", Eurocrypt 2016, algorithms 7, 8 and 9: a = 0) with
// b3 = 3 b = 9: G1 has prime order, so they have no exceptional case -- P + P, P + (-P) and the identity on either side
// take the same instructions as any other sum, and a bucket needs no branch.  The one predicated case is the caller's:
// an affine (0, 0) has no projective reading in the mixed formula and is skipped (g1_affine_is_identity).
// 9 x is three doublings and an add, not a multiply.  tests/cpp/g1_check.cpp checks all of it against affine
// chord-and-tangent arithmetic.
#ifndef HSW_G1_HPP
#define HSW_G1_HPP
#include "hsw_fq.hpp"

namespace hsw {

struct G1Affine { Fq x, y; };      // as stored: 64 bytes, (0, 0) = the identity
struct G1 { Fq x, y, z; };         // (X : Y : Z), identity (0 : 1 : 0)

HSW_PHD G1 g1_identity() { return G1{fq_zero(), fq_one_mont(), fq_zero()}; }
HSW_PHD bool g1_is_identity(const G1 &p) { return fq_is_zero(p.z); }
HSW_PHD bool g1_affine_is_identity(const G1Affine &p) {
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x |= p.x.l[j] | p.y.l[j];
    return x == 0;
}
HSW_PHD G1 g1_from_affine(const G1Affine &p) {
    if (g1_affine_is_identity(p)) return g1_identity();
    return G1{p.x, p.y, fq_one_mont()};
}
HSW_PHD Fq fq_mul_b3(const Fq &a) {                                      // 9 a
    Fq t = fq_add(a, a);
    t = fq_add(t, t);
    t = fq_add(t, t);
    return fq_add(t, a);
}

// (X1 : Y1 : Z1) + affine (X2, Y2), which is not (0, 0)
HSW_PHD G1 g1_add_mixed(const G1 &p, const G1Affine &q) {
    Fq t0 = fq_mont_mul(p.x, q.x), t1 = fq_mont_mul(p.y, q.y), t3 = fq_add(q.x, q.y), t4 = fq_add(p.x, p.y);
    t3 = fq_mont_mul(t3, t4); t4 = fq_add(t0, t1); t3 = fq_sub(t3, t4); t4 = fq_mont_mul(q.y, p.z); t4 = fq_add(t4, p.y);
    Fq y3 = fq_mont_mul(q.x, p.z); y3 = fq_add(y3, p.x);
    Fq x3 = fq_add(t0, t0); t0 = fq_add(x3, t0);
    Fq t2 = fq_mul_b3(p.z), z3 = fq_add(t1, t2); t1 = fq_sub(t1, t2); y3 = fq_mul_b3(y3); x3 = fq_mont_mul(t4, y3);
    t2 = fq_mont_mul(t3, t1); x3 = fq_sub(t2, x3); y3 = fq_mont_mul(y3, t0); t1 = fq_mont_mul(t1, z3); y3 = fq_add(t1, y3);
    t0 = fq_mont_mul(t0, t3); z3 = fq_mont_mul(z3, t4); z3 = fq_add(z3, t0);
    return G1{x3, y3, z3};
}

// (X1 : Y1 : Z1) + (X2 : Y2 : Z2)
HSW_PHD G1 g1_add(const G1 &p, const G1 &q) {
    Fq t0 = fq_mont_mul(p.x, q.x), t1 = fq_mont_mul(p.y, q.y), t2 = fq_mont_mul(p.z, q.z), t3 = fq_add(p.x, p.y), t4 = fq_add(q.x, q.y);
    t3 = fq_mont_mul(t3, t4); t4 = fq_add(t0, t1); t3 = fq_sub(t3, t4); t4 = fq_add(p.y, p.z);
    Fq x3 = fq_add(q.y, q.z); t4 = fq_mont_mul(t4, x3); x3 = fq_add(t1, t2); t4 = fq_sub(t4, x3); x3 = fq_add(p.x, p.z);
    Fq y3 = fq_add(q.x, q.z); x3 = fq_mont_mul(x3, y3); y3 = fq_add(t0, t2); y3 = fq_sub(x3, y3);
    x3 = fq_add(t0, t0); t0 = fq_add(x3, t0); t2 = fq_mul_b3(t2);
    Fq z3 = fq_add(t1, t2); t1 = fq_sub(t1, t2); y3 = fq_mul_b3(y3); x3 = fq_mont_mul(t4, y3); t2 = fq_mont_mul(t3, t1); x3 = fq_sub(t2, x3);
    y3 = fq_mont_mul(y3, t0); t1 = fq_mont_mul(t1, z3); y3 = fq_add(t1, y3); t0 = fq_mont_mul(t0, t3); z3 = fq_mont_mul(z3, t4); z3 = fq_add(z3, t0);
    return G1{x3, y3, z3};
}

// 2 (X : Y : Z)
HSW_PHD G1 g1_double(const G1 &p) {
    Fq t0 = fq_mont_mul(p.y, p.y), z3 = fq_add(t0, t0); z3 = fq_add(z3, z3); z3 = fq_add(z3, z3);
    Fq t1 = fq_mont_mul(p.y, p.z), t2 = fq_mont_mul(p.z, p.z); t2 = fq_mul_b3(t2);
    Fq x3 = fq_mont_mul(t2, z3), y3 = fq_add(t0, t2);
    z3 = fq_mont_mul(t1, z3); t1 = fq_add(t2, t2); t2 = fq_add(t1, t2); t0 = fq_sub(t0, t2); y3 = fq_mont_mul(t0, y3); y3 = fq_add(x3, y3);
    t1 = fq_mont_mul(p.x, p.y); x3 = fq_mont_mul(t0, t1); x3 = fq_add(x3, x3);
    return G1{x3, y3, z3};
}

// (X / Z, Y / Z) as stored, (0, 0) for the identity: one inversion
HSW_PHD G1Affine g1_to_affine(const G1 &p) {
    if (g1_is_identity(p)) return G1Affine{fq_zero(), fq_zero()};
    const Fq zi = fq_inv(p.z);
    return G1Affine{fq_mont_mul(p.x, zi), fq_mont_mul(p.y, zi)};
}

}  // namespace hsw
#endif
