// hsw_product_value.hpp -- the row rules of the lookup argument's grand product Z (hsw_gadget_lookup_product, include/hsw.h).
//
//   Z[0] = 1,  Z[i+1] = Z[i] num[i] / den[i],   num[i] = (A[i] + beta)(S[i] + gamma),  den[i] = (A'[i] + beta)(S'[i] + gamma)
// without a division per row:  Z[i] = PN[i] SD[i] / D  with PN the exclusive prefix product of num, SD the suffix
// product of den (SD[i] = den[i] ... den[u-1], SD[u] = 1) and D = SD[0], inverted once per argument.
// Cells come in the representation of the pass (canonical x, or Montgomery x R); inside, every product is held in
// Montgomery form (v R), so one fr_mont_mul multiplies two of them.  The way in and out, both exact:
//   Montgomery cells   (x R)(y R) R^-1 = (x y) R: one multiply;         Z as it is
//   canonical cells    (x y R^-1)(R^3) R^-1 = (x y) R: two multiplies;  Z times 1 (fr_from_mont)
// theta_mul is the factor that keeps a cell times theta in the representation of the cells under fr_mont_mul: theta as
// stored for Montgomery cells ((d R)(theta R) R^-1 = d theta R), theta R for canonical ones (d (theta R) R^-1 = d theta).
// Host- and device-callable: hsw_lookup_product.hip is built from these, tests/cpp/fr_mul_check.cpp runs the same
// routines against the recurrence with an inversion per row.
#ifndef HSW_PRODUCT_VALUE_HPP
#define HSW_PRODUCT_VALUE_HPP
#include "hsw_fr_mul.hpp"

namespace hsw {

// The challenges of one proof, as the kernels take them (32-byte cells as stored, below p)
struct ProductChallenges { PFe theta, theta_mul, beta, gamma; };

HSW_PHD PFe product_theta_mul(const PFe &theta, bool montgomery) { return montgomery ? theta : fr_to_mont(theta); }

// The unpermuted compressed input A[i] from the caller's cell(s), in the representation of the cells.
// kind: PERMUTED_VALUE_* (0 = the cell, 1 = dense * theta + spread, 2 = dense + spread * theta)
HSW_PHD PFe product_input(uint32_t kind, const PFe &dense, const PFe &spread, const PFe &theta_mul) {
    if (kind == 0) return dense;
    if (kind == 1) return fr_add(fr_mont_mul(dense, theta_mul), spread);
    return fr_add(dense, fr_mont_mul(spread, theta_mul));
}
// The unpermuted table column S[i]: row i of the table, and row 0 on the padding rows T <= i < u
HSW_PHD PFe product_table(uint32_t kind, uint32_t i, uint32_t T, const PFe &theta, bool montgomery) {
    return permuted_value(kind, i < T ? i : 0u, theta, montgomery);
}
// (a + beta)(s + gamma) of cells in the representation of the pass, in Montgomery form
HSW_PHD PFe product_term(const PFe &a, const PFe &s, const ProductChallenges &ch, bool montgomery) {
    const PFe t = fr_mont_mul(fr_add(a, ch.beta), fr_add(s, ch.gamma));
    return montgomery ? t : fr_mont_mul(t, PFe{HSW_FR_R3});
}
// a Montgomery-form value as a cell of the pass
HSW_PHD PFe product_cell(const PFe &z, bool montgomery) { return montgomery ? z : fr_from_mont(z); }

}  // namespace hsw
#endif
