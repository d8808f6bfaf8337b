// hsw_shplonk_value.hpp -- the rules of SHPLONK's multi-point opening of device columns (hsw_gadget_shplonk_quotient,
// hsw_gadget_shplonk_open, include/hsw.h).
//
//   c_i[j] = sum_{k<m_i} y^k a_{b_{i,k}}[j]          the fold of rotation set i: the first listed column gets y^0
//   Q_i    = floor(c_i / Z_i),  Z_i = prod_{z in S_i} (X - z)
//   h[j]   = sum_i v^i Q_i[j]
//   L[j]   = sum_i v^i zd_i c_i[j] - zt h[j],  zd_i = prod_{z in T \ S_i} (u - z),  zt = prod_{z in T} (u - z)
//   w[j]   = zd_0^-1 sum_{l>j} L[l] u^(l-j-1)
// Partial fractions make the division by Z_i a weighted sum of divisions by one root each, which are the suffix Horner
// sums of hsw_open_value.hpp:
//   lambda_{i,k} = 1 / prod_{l != k} (z_{i,k} - z_{i,l}),   Q_i[j] = sum_k lambda_{i,k} q_{i,k}[j],
//   q_{i,k}[j]   = sum_{l>j} c_i[l] z_{i,k}^(l-j-1)
// (1 / Z_i(X) = sum_k lambda_{i,k} / (X - z_{i,k}); the remainders of the single divisions are constants and sum to
// R_i(X) / Z_i(X)'s polynomial part, which is 0.)  sum_k lambda_{i,k} = 0 for t_i >= 2, so the top cells of Q_i come out
// exactly 0.  Both calls are therefore the same three launches: a fold with one staged weight per column, one scan per
// (set, point) item, and a write that sums the items' scans with one staged weight W per item:
//   quotient   column weights y^k, item weights W_{i,k} = v^i lambda_{i,k}
//   open       ONE set that holds every listed column and h, column weights v^i zd_i y^k / zd_0 and -zt / zd_0, the one
//              point u, W = 1 (no multiply)
// Every constant is held in Montgomery form, so the same code is exact for canonical and Montgomery cells
// (hsw_open_value.hpp).  Host- and device-callable: hsw_shplonk.hip is built from these, hsw_gadget_shplonk.cpp stages
// with them, tests/cpp/shplonk_value_check.cpp runs the launches thread for thread on the CPU.
#ifndef HSW_SHPLONK_VALUE_HPP
#define HSW_SHPLONK_VALUE_HPP
#include "hsw_open_value.hpp"

namespace hsw {

enum : uint32_t {
    SHPLONK_MAX_SET_POINTS = 16,     // HSW_SHPLONK_MAX_SET_POINTS
    SHPLONK_MAX_SETS = 65535,
    SHPLONK_CELL_NOT_BELOW_P = 4u,   // HSW_SHPLONK_CELL_NOT_BELOW_P
};

// lambda_k = 1 / prod_{l != k} (z[k] - z[l]) over the t points of a set, Montgomery form in and out; the points are
// distinct, so no factor is 0.  t = 1: the empty product, 1
HSW_PHD PFe shplonk_lambda(const PFe *z_mont, uint32_t t, uint32_t k) {
    PFe d = fr_one_mont();
    for (uint32_t l = 0; l < t; l++)
        if (l != k) d = fr_mont_mul(d, fr_sub(z_mont[k], z_mont[l]));
    return fr_inv(d);
}

// prod (u - z) over the points of T whose `skip` entry is 0 (skip NULL: all of T), Montgomery form
HSW_PHD PFe shplonk_vanish(const PFe &u_mont, const PFe *points_mont, uint32_t n_points, const uint8_t *skip) {
    PFe d = fr_one_mont();
    for (uint32_t i = 0; i < n_points; i++)
        if (!skip || !skip[i]) d = fr_mont_mul(d, fr_sub(u_mont, points_mont[i]));
    return d;
}

// The weights of one set's columns: out[k] = scale y^k.  quotient: scale 1; open: scale v^i zd_i / zd_0
HSW_PHD void shplonk_column_weights(const PFe &scale_mont, const PFe &y_mont, uint32_t m, PFe *out) {
    PFe w = scale_mont;
    for (uint32_t k = 0; k < m; k++) {
        out[k] = w;
        w = fr_mont_mul(w, y_mont);
    }
}

// one column into the fold: c + w a (the first column of a set always has weight 1 and is taken as it is)
HSW_PHD PFe shplonk_fold(const PFe &c, const PFe &w_mont, const PFe &a) { return fr_add(c, fr_mont_mul(a, w_mont)); }
// one item's share of an output cell: acc + W s
HSW_PHD PFe shplonk_gather(const PFe &acc, const PFe &W_mont, const PFe &s) { return fr_add(acc, fr_mont_mul(s, W_mont)); }

}  // namespace hsw
#endif
