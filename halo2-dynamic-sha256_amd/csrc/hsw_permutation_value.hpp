// hsw_permutation_value.hpp -- the row rules of the permutation argument's grand products Z (hsw_gadget_permutation_product,
// include/hsw.h), after halo2's permutation::prover.
//
// The m columns of the permutation go in chunks of L; per row i < u of chunk s (columns j, sL <= j < min(m, (s+1)L)):
//   num_s[i] = prod_j (v_j[i] + beta delta^j omega^i + gamma),   den_s[i] = prod_j (v_j[i] + beta sigma_j[i] + gamma)
//   Z_0[0] = 1,  Z_s[0] = Z_{s-1}[u],  Z_s[i+1] = Z_s[i] num_s[i] / den_s[i]
// Cells come in the representation of the pass (canonical x, or Montgomery x R); inside, every product is held in
// Montgomery form (hsw_product_value.hpp), and a FACTOR v + term + gamma stays in the representation of the cells, so the
// three addends need no conversion.  What is staged on the host makes that exact with one multiply per term:
//   omega^i          always in Montgomery form (w R): a cell-form x times it under fr_mont_mul stays in cell form;
//   beta delta^j     in cell form, so (beta delta^j)(omega^i R) R^-1 = beta delta^j omega^i in cell form: the identity term;
//   beta_mul         beta R for canonical cells, beta as stored for Montgomery ones (product_theta_mul): sigma times it
//                    is beta sigma in cell form: the sigma term.
// A chunk's product: Montgomery factors (f R) multiply up as they are.  n canonical factors under fr_mont_mul lose one
// R each, so the product starts from the seed R^(n+1): seed f_1 ... f_n R^-n = (f_1 ... f_n) R -- one multiply more per
// row and chunk, not per column.  Out again with product_cell.
// omega^i without a power per row: row = tile * TILE + t * ROWS + r; the host stages omega^(ROWS t) for the workgroup's
// threads and the binary powers of omega^TILE, a workgroup multiplies those of its tile's set bits, a thread multiplies
// by its table entry, and from there on by omega per row.  Nothing here checks that omega is a root of unity.
// Host- and device-callable: hsw_permutation_product.hip is built from these, hsw_gadget_permutation.cpp stages with
// them, tests/cpp/permutation_value_check.cpp runs them against a shift-and-add model.
#ifndef HSW_PERMUTATION_VALUE_HPP
#define HSW_PERMUTATION_VALUE_HPP
#include "hsw_product_value.hpp"

namespace hsw {

enum : uint32_t { PERMUTATION_TABLE = 256, PERMUTATION_TILE_BITS = 22 };   // threads of a workgroup; tile indices below 2^22 (u <= 2^31)

// The challenges of one proof, as the kernels take them
struct PermutationChallenges { PFe beta_mul, gamma; };

// omega's powers, all in Montgomery form: rows per thread and rows per tile are the staging call's
struct PermutationPowers {
    PFe omega;
    PFe thread[PERMUTATION_TABLE];          // omega^(rows_per_thread t)
    PFe tile[PERMUTATION_TILE_BITS];        // omega^(rows_per_tile 2^b)
};

// a stored challenge or constant (below p) in Montgomery form
HSW_PHD PFe permutation_to_mont(const PFe &stored, bool montgomery) { return montgomery ? stored : fr_to_mont(stored); }

// rows_per_tile = PERMUTATION_TABLE * rows_per_thread
HSW_PHD void permutation_stage_powers(const PFe &omega_mont, uint32_t rows_per_thread, PermutationPowers &pw) {
    pw.omega = omega_mont;
    PFe step = fr_one_mont();
    for (uint32_t r = 0; r < rows_per_thread; r++) step = fr_mont_mul(step, omega_mont);
    pw.thread[0] = fr_one_mont();
    for (uint32_t t = 1; t < PERMUTATION_TABLE; t++) pw.thread[t] = fr_mont_mul(pw.thread[t - 1], step);
    pw.tile[0] = fr_mont_mul(pw.thread[PERMUTATION_TABLE - 1], step);
    for (uint32_t b = 1; b < PERMUTATION_TILE_BITS; b++) pw.tile[b] = fr_mont_mul(pw.tile[b - 1], pw.tile[b - 1]);
}
// omega^(rows_per_tile tile), tile < 2^PERMUTATION_TILE_BITS: one multiply per set bit
HSW_PHD PFe permutation_omega_tile(const PermutationPowers &pw, uint32_t tile) {
    PFe w = fr_one_mont();
    for (uint32_t b = 0; b < PERMUTATION_TILE_BITS; b++)
        if ((tile >> b) & 1u) w = fr_mont_mul(w, pw.tile[b]);
    return w;
}
// omega^(first row of thread t of that tile)
HSW_PHD PFe permutation_omega_thread(const PermutationPowers &pw, const PFe &omega_tile, uint32_t t) { return fr_mont_mul(omega_tile, pw.thread[t]); }

// beta delta^j in cell form from the one of column j - 1 (column 0: beta as stored)
HSW_PHD PFe permutation_next_beta_delta(const PFe &beta_delta, const PFe &delta_mont) { return fr_mont_mul(beta_delta, delta_mont); }
// where a chunk of n columns starts its product: 1 in Montgomery form, or R^(n+1) for canonical factors
HSW_PHD PFe permutation_seed(uint32_t n, bool montgomery) {
    if (montgomery) return fr_one_mont();
    PFe s = PFe{HSW_FR_R2};
    for (uint32_t k = 1; k < n; k++) s = fr_mont_mul(s, PFe{HSW_FR_R2});
    return s;
}
// beta delta^j omega^i in cell form; the next row's is this one times omega (Montgomery form) again
HSW_PHD PFe permutation_identity_term(const PFe &beta_delta, const PFe &omega_i_mont) { return fr_mont_mul(beta_delta, omega_i_mont); }
// beta sigma in cell form
HSW_PHD PFe permutation_sigma_term(const PFe &sigma, const PFe &beta_mul) { return fr_mont_mul(sigma, beta_mul); }
// v + term + gamma, all in cell form
HSW_PHD PFe permutation_factor(const PFe &v, const PFe &term, const PFe &gamma) { return fr_add(fr_add(v, term), gamma); }
// the product so far times a factor; a Montgomery chunk's first factor IS the product so far (its seed is 1)
HSW_PHD PFe permutation_accumulate(const PFe &acc, const PFe &factor, bool first, bool montgomery) {
    if (montgomery && first) return factor;
    return fr_mont_mul(acc, factor);
}

}  // namespace hsw
#endif
