// hsw_quotient_value.hpp -- the row rules of the quotient h(X) on the extended coset (hsw_gadget_quotient, include/hsw.h),
// after halo2's evaluate_h and vanishing argument (the order of the expressions: assumption A9).
//
// n = 2^log_rows, N = 2^log_n, e = log_n - log_rows, w = omega_ext, X_i = zeta w^i.  A base-domain rotation r reads
// extended row (i + r 2^e) mod N; u = usable_rows, and the rotation -(blinding + 1) is the shift +u in base rows.  Per
// proof the accumulator V starts at 0 and every expression folds as V = V y + expr:
//   gates        sum_t coeff_t prod_f col_{t,f}[(i + rot_{t,f} 2^e) mod N], in the caller's order
//   permutation  l0 (1 - Z_0);  l_last (Z_{S-1}^2 - Z_{S-1});  s = 1 .. S-1: l0 (Z_s - Z_{s-1}[i + u 2^e]);
//                s = 0 .. S-1: l_active (Z_s[i + 2^e] prod_j (v_j + beta sigma_j + gamma) - Z_s prod_j (v_j + beta delta^j X_i + gamma))
//   lookups      l0 (1 - Z);  l_last (Z^2 - Z);  l_active (Z[i + 2^e] (A' + beta)(S' + gamma) - Z (A + beta)(Sv + gamma));
//                l0 (A' - S');  l_active (A' - S')(A' - A'[i - 2^e]);   A, Sv: the fold acc theta + col of the columns
//   h[i] = V[i] t_inv[i mod 2^e],  t_inv[r] = (zeta^n (w^n)^r - 1)^-1
// Cells come in the representation of the pass (canonical x, or Montgomery x R) and V is held IN THAT REPRESENTATION, so
// it leaves as a cell with no conversion.  What makes every addend exact under fr_mont_mul (a b R^-1):
//   y, theta, t_inv, w^i      in Montgomery form: a cell-form value times one of them stays in cell form;
//   beta, gamma, 1            in cell form, as addends; beta_mul (beta R for canonical cells) for beta sigma, and
//                             beta delta^j zeta in cell form for the identity term, as hsw_permutation_value.hpp has them;
//   a product of k cells      k - 1 multiplies lose k - 1 factors R of canonical cells (none of Montgomery ones, whose
//                             own R's pay for them).  They are put back ONCE per product, by one multiply of its first
//                             factor with the constant R^k (quotient_scaled): a gate monomial of d factors starts from
//                             coeff R^d (coeff as stored for Montgomery cells, which is coeff R), the fixed families
//                             scale l0 / l_last / l_active by R^2 / R^3 / R^4 and R^(n_j + 2) for a set of n_j columns.
// w^i comes from PermutationPowers (hsw_permutation_value.hpp), staged for QUOTIENT_ROWS rows per thread.
// The bodies below are what one thread of hsw_quotient.hip runs; tests/cpp/quotient_value_check.cpp runs them thread for
// thread on the CPU against the plain definition.  Host- and device-callable.
#ifndef HSW_QUOTIENT_VALUE_HPP
#define HSW_QUOTIENT_VALUE_HPP
#include "hsw_permutation_value.hpp"

namespace hsw {

enum : uint32_t {
    QUOTIENT_THREADS = PERMUTATION_TABLE,
    QUOTIENT_ROWS = 2,                   // consecutive extended rows of a thread: 64 contiguous bytes per column
    QUOTIENT_TILE = QUOTIENT_THREADS * QUOTIENT_ROWS,
    QUOTIENT_MAX_FACTORS = 8,            // HSW_QUOTIENT_MAX_FACTORS
    QUOTIENT_MAX_EXTENSION = 8,          // HSW_QUOTIENT_MAX_EXTENSION
    QUOTIENT_MAX_LOG = 28,
    QUOTIENT_CELL_NOT_BELOW_P = 4u,      // HSW_QUOTIENT_CELL_NOT_BELOW_P
};

// The challenges of one proof, as the kernels take them
struct QuotientProof {
    PFe y, theta;                        // Montgomery form
    PFe beta, gamma;                     // as stored: addends in cell form
    PFe beta_mul;                        // product_theta_mul of beta: sigma times it is beta sigma in cell form
};

// The constants of a call
struct QuotientConstants {
    PFe one;                             // 1 in cell form
    PFe r2, r3, r4, seed_full, seed_last;   // R^2, R^3, R^4, R^(L + 2), R^(columns of the last set + 2)
};

// What the launches of a call share.  Every pointer is device memory (host memory where the CPU runs the bodies); the
// descriptor tables are read with indices that do not depend on the thread
struct QuotientParams {
    uint32_t N, mask, ext, u_off;        // N, N - 1, 2^e, (u 2^e) mod N
    uint32_t m, F, first, reserved_;     // columns of a proof, shared columns; first: this launch starts V at 0
    const PFe *const *cols;              // K x m
    const PFe *const *fixed;             // F
    const PFe *l0, *l_last, *l_active;
    // gates
    uint32_t n_gates, n_perm, L, S;
    const uint32_t *gate_first_term, *term_first_factor, *factor_column, *factor_offset;   // offset: (rot 2^e) mod N
    const PFe *term_coeff;               // coeff R^d for canonical cells, as stored for Montgomery ones
    // permutation
    const uint32_t *perm_columns;
    const PFe *const *sigmas;            // n_perm
    const PFe *const *perm_z;            // K x S
    const PFe *beta_delta;               // K x n_perm: beta delta^j zeta in cell form
    const PermutationPowers *powers;     // of w, QUOTIENT_ROWS rows per thread
    // lookups
    uint32_t n_lookups, reserved2_;
    const uint32_t *first_input, *inputs, *first_table, *tables;
    const PFe *const *lk_a, *const *lk_s, *const *lk_z;   // K x n_lookups: A', S', Z
    // all
    const QuotientProof *proofs;         // K
    const PFe *t_inv;                    // 2^e, Montgomery form
    PFe *const *h;                       // K
    PFe *V;                              // the scratch of the batch: N cells per proof of it
    uint32_t *status;                    // K words, zeroed by the caller
    const QuotientConstants *k;
};

// a stored challenge or constant (below p) in Montgomery form
HSW_PHD PFe quotient_to_mont(const PFe &stored, bool montgomery) { return permutation_to_mont(stored, montgomery); }
// R^k, k >= 1
HSW_PHD PFe quotient_r_power(uint32_t k) {
    PFe s = fr_one_mont();
    for (uint32_t i = 1; i < k; i++) s = fr_mont_mul(s, PFe{HSW_FR_R2});
    return s;
}
// the coefficient of a monomial of d factors as the kernels take it
HSW_PHD PFe quotient_coeff(const PFe &stored, uint32_t d, bool montgomery) {
    PFe c = stored;
    if (!montgomery)
        for (uint32_t i = 0; i < d; i++) c = fr_mont_mul(c, PFe{HSW_FR_R2});
    return c;
}
// the first factor of a product of k cells: l R^(k-1) for canonical cells (r_k = R^k), l itself for Montgomery ones
template <bool MONT>
HSW_PHD PFe quotient_scaled(const PFe &l, const PFe &r_k) { return MONT ? l : fr_mont_mul(l, r_k); }
// V y + expr
HSW_PHD PFe quotient_fold(const PFe &V, const PFe &y_mont, const PFe &expr) { return fr_add(fr_mont_mul(V, y_mont), expr); }
// acc theta + col
HSW_PHD PFe quotient_theta_fold(const PFe &acc, const PFe &theta_mont, const PFe &col) { return fr_add(fr_mont_mul(acc, theta_mont), col); }
// l0 (1 - z), l0 (a - b): l0s = quotient_scaled(l0, R^2)
HSW_PHD PFe quotient_difference(const PFe &l0s, const PFe &a, const PFe &b) { return fr_mont_mul(l0s, fr_sub(a, b)); }
// l_last (z^2 - z): lls = quotient_scaled(l_last, R^3)
HSW_PHD PFe quotient_boolean(const PFe &lls, const PFe &z, const PFe &one) { return fr_mont_mul(fr_mont_mul(lls, fr_sub(z, one)), z); }
// h = V t_inv
HSW_PHD PFe quotient_finish(const PFe &V, const PFe &t_inv_mont) { return fr_mont_mul(V, t_inv_mont); }

// t_inv[r] = (zeta^n (w^n)^r - 1)^-1 for r < 2^e, Montgomery form; false if one of them has no inverse
HSW_PHD bool quotient_stage_t_inv(const PFe &zeta_mont, const PFe &w_mont, uint32_t log_rows, uint32_t e, PFe *t_inv) {
    PFe zn = zeta_mont, wn = w_mont;
    for (uint32_t k = 0; k < log_rows; k++) { zn = fr_mont_mul(zn, zn); wn = fr_mont_mul(wn, wn); }
    for (uint32_t r = 0; r < (1u << e); r++) {
        const PFe t = fr_sub(zn, fr_one_mont());
        if (fr_is_zero(t)) return false;
        t_inv[r] = fr_inv(t);
        zn = fr_mont_mul(zn, wn);
    }
    return true;
}

// One cell: on the device two 16-byte loads (columns are 16-byte aligned)
HSW_PHD PFe quotient_load(const PFe *col, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 *q = reinterpret_cast<const uint4 *>(col) + 2 * (size_t)i;
    const uint4 a = q[0], b = q[1];
    return PFe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
#else
    return col[i];
#endif
}
HSW_PHD void quotient_store(PFe *col, uint32_t i, const PFe &v) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *q = reinterpret_cast<uint4 *>(col) + 2 * (size_t)i;
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
#else
    col[i] = v;
#endif
}
// a stored cell, checked
HSW_PHD PFe quotient_cell(const PFe *col, uint32_t i, bool &ok) {
    const PFe x = quotient_load(col, i);
    ok = ok && pfe_below_p(x);
    return x;
}
// column j of the shared index space for proof c
HSW_PHD const PFe *quotient_column(const QuotientParams &p, uint32_t c, uint32_t j) {
    return j < p.m ? p.cols[(size_t)c * p.m + j] : p.fixed[j - p.m];
}

// V of the thread's rows as the launch finds it (Vb: the proof's N cells of scratch)
HSW_PHD void quotient_begin(const QuotientParams &p, const PFe *Vb, uint32_t row0, PFe *V) {
    for (uint32_t r = 0; r < QUOTIENT_ROWS; r++) V[r] = p.first ? fr_zero() : quotient_load(Vb, row0 + r);
}
HSW_PHD void quotient_end(PFe *Vb, uint32_t row0, const PFe *V) {
    for (uint32_t r = 0; r < QUOTIENT_ROWS; r++) quotient_store(Vb, row0 + r, V[r]);
}

// The gates of proof c folded into V for rows row0 .. row0 + QUOTIENT_ROWS; false: a stored cell not below p was read
HSW_PHD bool quotient_gates_rows(const QuotientParams &p, uint32_t c, uint32_t row0, PFe *V) {
    static_assert(QUOTIENT_ROWS == 2, "two rows written out below so that nothing is indexed at run time");
    const PFe y = p.proofs[c].y;
    bool ok = true;
    for (uint32_t g = 0; g < p.n_gates; g++) {
        PFe s0 = fr_zero(), s1 = fr_zero();
        for (uint32_t t = p.gate_first_term[g]; t < p.gate_first_term[g + 1]; t++) {
            PFe a0 = p.term_coeff[t], a1 = a0;
            for (uint32_t f = p.term_first_factor[t]; f < p.term_first_factor[t + 1]; f++) {
                const PFe *col = quotient_column(p, c, p.factor_column[f]);
                const uint32_t off = p.factor_offset[f];
                a0 = fr_mont_mul(a0, quotient_cell(col, (row0 + off) & p.mask, ok));
                a1 = fr_mont_mul(a1, quotient_cell(col, (row0 + 1 + off) & p.mask, ok));
            }
            s0 = fr_add(s0, a0);
            s1 = fr_add(s1, a1);
        }
        V[0] = quotient_fold(V[0], y, s0);
        V[1] = quotient_fold(V[1], y, s1);
    }
    return ok;
}

// One row of the permutation argument; x: w^row in Montgomery form
template <bool MONT>
HSW_PHD bool quotient_permutation_row(const QuotientParams &p, uint32_t c, uint32_t row, const PFe &x, PFe &V) {
    const QuotientProof &pr = p.proofs[c];
    const PFe *const *Z = p.perm_z + (size_t)c * p.S;
    bool ok = true;
    {
        const PFe l0s = quotient_scaled<MONT>(quotient_cell(p.l0, row, ok), p.k->r2);
        V = quotient_fold(V, pr.y, quotient_difference(l0s, p.k->one, quotient_cell(Z[0], row, ok)));
        const PFe lls = quotient_scaled<MONT>(quotient_cell(p.l_last, row, ok), p.k->r3);
        V = quotient_fold(V, pr.y, quotient_boolean(lls, quotient_cell(Z[p.S - 1], row, ok), p.k->one));
        for (uint32_t s = 1; s < p.S; s++)
            V = quotient_fold(V, pr.y, quotient_difference(l0s, quotient_cell(Z[s], row, ok), quotient_cell(Z[s - 1], (row + p.u_off) & p.mask, ok)));
    }
    const PFe la = quotient_cell(p.l_active, row, ok);
    for (uint32_t s = 0; s < p.S; s++) {
        const uint32_t j0 = s * p.L, j1 = p.n_perm - j0 < p.L ? p.n_perm : j0 + p.L;
        const PFe las = quotient_scaled<MONT>(la, j1 - j0 == p.L ? p.k->seed_full : p.k->seed_last);
        PFe left = fr_mont_mul(las, quotient_cell(Z[s], (row + p.ext) & p.mask, ok));
        PFe right = fr_mont_mul(las, quotient_cell(Z[s], row, ok));
        for (uint32_t j = j0; j < j1; j++) {
            const PFe v = quotient_cell(quotient_column(p, c, p.perm_columns[j]), row, ok);
            const PFe sg = quotient_cell(p.sigmas[j], row, ok);
            left = fr_mont_mul(left, permutation_factor(v, permutation_sigma_term(sg, pr.beta_mul), pr.gamma));
            right = fr_mont_mul(right, permutation_factor(v, permutation_identity_term(p.beta_delta[(size_t)c * p.n_perm + j], x), pr.gamma));
        }
        V = quotient_fold(V, pr.y, fr_sub(left, right));
    }
    return ok;
}
// The thread's rows; x0: w^row0 in Montgomery form
template <bool MONT>
HSW_PHD bool quotient_permutation_rows(const QuotientParams &p, uint32_t c, uint32_t row0, const PFe &x0, PFe *V) {
    static_assert(QUOTIENT_ROWS == 2, "one call per row below");
    bool ok = quotient_permutation_row<MONT>(p, c, row0, x0, V[0]);
    ok = quotient_permutation_row<MONT>(p, c, row0 + 1, fr_mont_mul(x0, p.powers->omega), V[1]) && ok;
    return ok;
}

// One row of the lookup arguments
template <bool MONT>
HSW_PHD bool quotient_lookups_row(const QuotientParams &p, uint32_t c, uint32_t row, PFe &V) {
    const QuotientProof &pr = p.proofs[c];
    bool ok = true;
    const PFe l0s = quotient_scaled<MONT>(quotient_cell(p.l0, row, ok), p.k->r2);
    const PFe lls = quotient_scaled<MONT>(quotient_cell(p.l_last, row, ok), p.k->r3);
    const PFe la = quotient_cell(p.l_active, row, ok);
    for (uint32_t l = 0; l < p.n_lookups; l++) {
        const size_t at = (size_t)c * p.n_lookups + l;
        PFe A = fr_zero(), Sv = fr_zero();
        for (uint32_t k = p.first_input[l]; k < p.first_input[l + 1]; k++) A = quotient_theta_fold(A, pr.theta, quotient_cell(quotient_column(p, c, p.inputs[k]), row, ok));
        for (uint32_t k = p.first_table[l]; k < p.first_table[l + 1]; k++) Sv = quotient_theta_fold(Sv, pr.theta, quotient_cell(quotient_column(p, c, p.tables[k]), row, ok));
        const PFe z = quotient_cell(p.lk_z[at], row, ok), ap = quotient_cell(p.lk_a[at], row, ok), sp = quotient_cell(p.lk_s[at], row, ok);
        V = quotient_fold(V, pr.y, quotient_difference(l0s, p.k->one, z));
        V = quotient_fold(V, pr.y, quotient_boolean(lls, z, p.k->one));
        {
            const PFe la4 = quotient_scaled<MONT>(la, p.k->r4);
            PFe left = fr_mont_mul(la4, quotient_cell(p.lk_z[at], (row + p.ext) & p.mask, ok));
            left = fr_mont_mul(fr_mont_mul(left, fr_add(ap, pr.beta)), fr_add(sp, pr.gamma));
            PFe right = fr_mont_mul(la4, z);
            right = fr_mont_mul(fr_mont_mul(right, fr_add(A, pr.beta)), fr_add(Sv, pr.gamma));
            V = quotient_fold(V, pr.y, fr_sub(left, right));
        }
        const PFe d = fr_sub(ap, sp);
        V = quotient_fold(V, pr.y, fr_mont_mul(l0s, d));
        const PFe la3 = quotient_scaled<MONT>(la, p.k->r3);
        V = quotient_fold(V, pr.y, fr_mont_mul(fr_mont_mul(la3, d), fr_sub(ap, quotient_cell(p.lk_a[at], (row - p.ext) & p.mask, ok))));
    }
    return ok;
}
template <bool MONT>
HSW_PHD bool quotient_lookups_rows(const QuotientParams &p, uint32_t c, uint32_t row0, PFe *V) {
    static_assert(QUOTIENT_ROWS == 2, "one call per row below");
    bool ok = quotient_lookups_row<MONT>(p, c, row0, V[0]);
    ok = quotient_lookups_row<MONT>(p, c, row0 + 1, V[1]) && ok;
    return ok;
}

// h of the thread's rows
HSW_PHD void quotient_finish_rows(const QuotientParams &p, const PFe *Vb, PFe *h, uint32_t row0) {
    for (uint32_t r = 0; r < QUOTIENT_ROWS; r++)
        quotient_store(h, row0 + r, quotient_finish(quotient_load(Vb, row0 + r), p.t_inv[(row0 + r) & (p.ext - 1)]));
}

}  // namespace hsw
#endif
