// hsw_gadget_quotient.cpp -- the quotient h(X) of device columns on the extended coset (include/hsw.h, "the quotient
// h(X) of device columns"): every refusal decided on the host, the descriptor tables, the challenges and the constants
// staged as hsw_quotient_value.hpp takes them (rotations as row offsets, coefficients with their R factors, t_inv by
// fr_inv), the proofs cut into batches whose accumulators fit the scratch, then the launches of hsw_quotient.hip batch
// by batch.  A translation unit of its own: only the entry point below refers to those kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_nounwind.hpp"
#include "hsw_ntt_value.hpp"
#include "hsw_quotient.h"

namespace {

using hsw::fail_at;
using hsw::Interval;
using hsw::load_below_p;
using hsw::PFe;

const size_t QUOTIENT_GRID_Y = 65535;                          // blockIdx.y

// offsets[0 .. n] ascending from 0 to `end`
bool offsets_ok(const uint32_t *off, size_t n, size_t end) {
    if (off[0] != 0 || off[n] != end) return false;
    for (size_t i = 0; i < n; i++)
        if (off[i] > off[i + 1]) return false;
    return true;
}

// the kinds of columns a call reads, for the overlap message
const char *const KIND[] = {"column", "fixed column", "l0", "l_last", "l_active", "sigma", "permutation product", "permuted input", "permuted table", "lookup product"};

}  // namespace

extern "C" int hsw_gadget_quotient(hsw_gadget *g, const hsw_quotient *args, hsw_quotient_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->first_refused = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const hsw_quotient &a = *args;
    const hsw_quotient_gates &ga = a.gates;
    const hsw_quotient_lookups &lk = a.lookups;
    const size_t K = a.n_proofs, m = a.n_columns, F = a.n_fixed, n_perm = a.n_perm_columns, n_lk = lk.n_lookups;
    if (a.flags) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    if (K == 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_proofs is at least 1");
    if (ga.n_gates == 0 && n_perm == 0 && n_lk == 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "no gate, no permutation and no lookup: nothing to fold");
    if (a.log_n > hsw::QUOTIENT_MAX_LOG) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "log_n is at most 28");
    if (a.log_rows >= a.log_n || a.log_n - a.log_rows > HSW_QUOTIENT_MAX_EXTENSION)
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "the extension log_n - log_rows is 1 .. 8");
    const uint32_t ext_log = a.log_n - a.log_rows;
    const uint64_t n = 1ull << a.log_rows, N = 1ull << a.log_n;
    if (a.usable_rows < 1 || a.usable_rows >= n) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "usable_rows is 1 .. 2^log_rows - 1");
    const size_t big[] = {K, m, F, ga.n_gates, ga.n_terms, ga.n_factors, n_perm, n_lk};
    for (size_t x : big)
        if (x > 0xFFFFFFFFull) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "a count does not fit 32 bits");
    if ((uint64_t)K * std::max<size_t>(m, 1) > 0xFFFFFFFFull) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "n_proofs x n_columns does not fit 32 bits");
    const size_t width = m + F;
    const bool fixed_family = n_perm || n_lk;                    // l0, l_last, l_active, beta, gamma
    // ---- the descriptor tables ----
    if (m && !a.d_columns) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "d_columns is NULL");
    if (F && !a.d_fixed) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "d_fixed is NULL");
    if (!a.d_h) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "d_h is NULL");
    if (!a.ys) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "ys is NULL");
    if (!a.omega_ext || !a.zeta) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega_ext or zeta is NULL");
    if (fixed_family && (!a.betas || !a.gammas)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "betas or gammas is NULL");
    if (fixed_family && (!a.d_l0 || !a.d_l_last || !a.d_l_active)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "d_l0, d_l_last or d_l_active is NULL");
    std::vector<uint32_t> factor_offset(ga.n_factors);
    if (ga.n_gates) {
        if (!ga.gate_first_term || !ga.term_first_factor || (ga.n_terms && !ga.term_coeffs) || (ga.n_factors && (!ga.factor_column || !ga.factor_rotation)))
            return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "an array of the gates is NULL");
        if (!offsets_ok(ga.gate_first_term, ga.n_gates, ga.n_terms)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "gate_first_term is not ascending from 0 to n_terms");
        if (!offsets_ok(ga.term_first_factor, ga.n_terms, ga.n_factors)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "term_first_factor is not ascending from 0 to n_factors");
        for (size_t t = 0; t < ga.n_terms; t++)
            if (ga.term_first_factor[t + 1] - ga.term_first_factor[t] > HSW_QUOTIENT_MAX_FACTORS) return fail_at(e, HSW_ERR_INVALID_ARG, "term", t, "more than HSW_QUOTIENT_MAX_FACTORS factors");
        for (size_t f = 0; f < ga.n_factors; f++) {
            if (ga.factor_column[f] >= width) return fail_at(e, HSW_ERR_INVALID_ARG, "factor", f, "its column index is out of range");
            const int64_t r = ga.factor_rotation[f];
            if (r <= -(int64_t)n || r >= (int64_t)n) return fail_at(e, HSW_ERR_INVALID_ARG, "factor", f, "a rotation of 2^log_rows rows or more");
            factor_offset[f] = (uint32_t)(((uint64_t)(r + (int64_t)n) << ext_log) & (N - 1));
        }
    } else if (ga.n_terms || ga.n_factors) {
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "terms or factors without a gate");
    }
    size_t S = 0;
    const uint32_t L = n_perm ? (uint32_t)std::min<size_t>(std::max<uint32_t>(a.chunk_columns, 1), n_perm) : 1u;   // (a set never holds more than all columns)
    if (n_perm) {
        if (a.chunk_columns < 1) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "chunk_columns is at least 1");
        if (!a.perm_columns || !a.d_sigmas || !a.d_perm_products) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "an array of the permutation is NULL");
        if (!a.delta) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "delta is NULL");
        S = (n_perm + L - 1) / L;
        for (size_t j = 0; j < n_perm; j++)
            if (a.perm_columns[j] >= width) return fail_at(e, HSW_ERR_INVALID_ARG, "permutation column", j, "its column index is out of range");
    }
    if (n_lk) {
        if (!lk.first_input || !lk.inputs || !lk.first_table || !lk.tables || !lk.d_permuted_inputs || !lk.d_permuted_tables || !lk.d_products || !lk.thetas)
            return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "an array of the lookups is NULL");
        if (lk.first_input[0] != 0 || lk.first_table[0] != 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "first_input[0] and first_table[0] are 0");
        for (size_t l = 0; l < n_lk; l++) {
            if (lk.first_input[l + 1] <= lk.first_input[l]) return fail_at(e, HSW_ERR_INVALID_ARG, "lookup", l, "no input column (first_input must increase)");
            if (lk.first_table[l + 1] <= lk.first_table[l]) return fail_at(e, HSW_ERR_INVALID_ARG, "lookup", l, "no table column (first_table must increase)");
            for (uint32_t k = lk.first_input[l]; k < lk.first_input[l + 1]; k++)
                if (lk.inputs[k] >= width) return fail_at(e, HSW_ERR_INVALID_ARG, "lookup", l, "an input column index out of range");
            for (uint32_t k = lk.first_table[l]; k < lk.first_table[l + 1]; k++)
                if (lk.tables[k] >= width) return fail_at(e, HSW_ERR_INVALID_ARG, "lookup", l, "a table column index out of range");
        }
    }
    // ---- the pointers: present, aligned, and no d_h over anything read or over another d_h ----
    std::vector<Interval> iv;
    const uintptr_t col_bytes = (uintptr_t)N * HSW_CELL_BYTES;
    bool bad_ptr = false;
    size_t bad_kind = 0, bad_index = 0;
    auto reads = [&](const void *ptr, size_t kind, size_t index) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(ptr);
        if ((!x || (x & 15u)) && !bad_ptr) { bad_ptr = true; bad_kind = kind; bad_index = index; }
        iv.push_back(Interval{x, x + col_bytes, index, false, kind});
    };
    for (size_t i = 0; i < K * m; i++) reads(a.d_columns[i], 0, i);
    for (size_t i = 0; i < F; i++) reads(a.d_fixed[i], 1, i);
    if (fixed_family) { reads(a.d_l0, 2, 0); reads(a.d_l_last, 3, 0); reads(a.d_l_active, 4, 0); }
    for (size_t i = 0; i < n_perm; i++) reads(a.d_sigmas[i], 5, i);
    for (size_t i = 0; i < (n_perm ? K * S : 0); i++) reads(a.d_perm_products[i], 6, i);
    for (size_t i = 0; i < K * n_lk; i++) { reads(lk.d_permuted_inputs[i], 7, i); reads(lk.d_permuted_tables[i], 8, i); reads(lk.d_products[i], 9, i); }
    if (bad_ptr) return fail_at(e, HSW_ERR_INVALID_ARG, KIND[bad_kind], bad_index, "a pointer that is NULL or not 16-byte aligned");
    for (size_t k = 0; k < K; k++) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(a.d_h[k]);
        if (!x || (x & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a d_h pointer that is NULL or not 16-byte aligned");
        iv.push_back(Interval{x, x + col_bytes, k, true, 0});
    }
    {
        Interval writer{}, with{};
        if (hsw::output_overlaps(iv, &writer, &with)) {
            const std::string what = std::string("its d_h overlaps ") + (with.out ? "the d_h of proof" : KIND[with.other]) + " " + std::to_string(with.index);
            return fail_at(e, HSW_ERR_INVALID_ARG, "proof", writer.index, what.c_str());
        }
    }
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    // ---- coefficients, challenges and constants ----
    std::vector<PFe> coeff(ga.n_terms);
    for (size_t t = 0; t < ga.n_terms; t++) {
        if (!load_below_p(coeff[t], static_cast<const uint8_t *>(ga.term_coeffs) + 32 * t)) return fail_at(e, HSW_ERR_INVALID_ARG, "term", t, "a coefficient whose stored limbs are not below p");
        coeff[t] = hsw::quotient_coeff(coeff[t], ga.term_first_factor[t + 1] - ga.term_first_factor[t], mont);
    }
    PFe w, zeta, delta = hsw::fr_zero();
    if (!load_below_p(w, a.omega_ext) || !load_below_p(zeta, a.zeta) || (n_perm && !load_below_p(delta, a.delta)))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega_ext, zeta or delta whose stored limbs are not below p");
    w = hsw::quotient_to_mont(w, mont);
    if (!hsw::ntt_root_is_primitive(w, a.log_n)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega_ext is not a primitive 2^log_n-th root of unity");
    const PFe zeta_mont = hsw::quotient_to_mont(zeta, mont), delta_mont = hsw::quotient_to_mont(delta, mont);
    std::vector<PFe> t_inv((size_t)1 << ext_log);
    if (!hsw::quotient_stage_t_inv(zeta_mont, w, a.log_rows, ext_log, t_inv.data()))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "zeta: the vanishing polynomial is 0 on its coset (some zeta^n (w^n)^r - 1 is 0)");
    std::vector<hsw::QuotientProof> proofs(K);
    std::vector<PFe> beta_delta(K * n_perm);
    for (size_t k = 0; k < K; k++) {
        hsw::QuotientProof &pr = proofs[k];
        std::memset(&pr, 0, sizeof pr);
        PFe y, theta = hsw::fr_zero();
        if (!load_below_p(y, static_cast<const uint8_t *>(a.ys) + 32 * k)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a y whose stored limbs are not below p");
        if (n_lk && !load_below_p(theta, static_cast<const uint8_t *>(lk.thetas) + 32 * k)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a theta whose stored limbs are not below p");
        pr.y = hsw::quotient_to_mont(y, mont);
        pr.theta = hsw::quotient_to_mont(theta, mont);
        if (fixed_family) {
            if (!load_below_p(pr.beta, static_cast<const uint8_t *>(a.betas) + 32 * k)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a beta whose stored limbs are not below p");
            if (!load_below_p(pr.gamma, static_cast<const uint8_t *>(a.gammas) + 32 * k)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a gamma whose stored limbs are not below p");
            pr.beta_mul = hsw::product_theta_mul(pr.beta, mont);
        }
        PFe bd = hsw::fr_mont_mul(pr.beta, zeta_mont);           // beta zeta in cell form, then times delta per column
        for (size_t j = 0; j < n_perm; j++) {
            beta_delta[k * n_perm + j] = bd;
            bd = hsw::permutation_next_beta_delta(bd, delta_mont);
        }
    }
    hsw::QuotientConstants kc;
    kc.one = hsw::pfe_repr(1u, mont);
    kc.r2 = hsw::quotient_r_power(2); kc.r3 = hsw::quotient_r_power(3); kc.r4 = hsw::quotient_r_power(4);
    kc.seed_full = hsw::quotient_r_power(L + 2);
    kc.seed_last = hsw::quotient_r_power((uint32_t)(n_perm ? n_perm - (S - 1) * L : 0) + 2);
    hsw::PermutationPowers powers;
    hsw::permutation_stage_powers(w, hsw::QUOTIENT_ROWS, powers);
    // ---- batches of proofs whose accumulators fit the scratch ----
    const size_t v_bytes = (size_t)N * sizeof(PFe);
    const size_t per_batch = std::min(std::min(K, QUOTIENT_GRID_Y), std::max<size_t>(1, e->quotient_scratch / v_bytes));
    const size_t scratch_bytes = per_batch * v_bytes;
    // ---- device staging: [status words][tables ...][the accumulators of a batch] ----
    hsw::Staging st;
    st.zeroed(K * sizeof(uint32_t));                      // (the status words start at 0)
    const size_t o_cols = st.add(a.d_columns, K * m * sizeof(void *)), o_fixed = st.add(a.d_fixed, F * sizeof(void *));
    const size_t o_gft = st.add(ga.gate_first_term, ga.n_gates ? (ga.n_gates + 1) * 4 : 0), o_tff = st.add(ga.term_first_factor, ga.n_gates ? (ga.n_terms + 1) * 4 : 0);
    const size_t o_fc = st.add(ga.factor_column, ga.n_factors * 4), o_fo = st.add(factor_offset.data(), ga.n_factors * 4);
    const size_t o_coeff = st.add(coeff.data(), ga.n_terms * sizeof(PFe));
    const size_t o_pc = st.add(a.perm_columns, n_perm * 4), o_sig = st.add(a.d_sigmas, n_perm * sizeof(void *));
    const size_t o_pz = st.add(a.d_perm_products, (n_perm ? K * S : 0) * sizeof(void *)), o_bd = st.add(beta_delta.data(), beta_delta.size() * sizeof(PFe));
    const size_t o_pw = st.add(&powers, sizeof powers);
    const size_t o_fi = st.add(lk.first_input, n_lk ? (n_lk + 1) * 4 : 0), o_in = st.add(lk.inputs, n_lk ? lk.first_input[n_lk] * 4 : 0);
    const size_t o_ft = st.add(lk.first_table, n_lk ? (n_lk + 1) * 4 : 0), o_tb = st.add(lk.tables, n_lk ? lk.first_table[n_lk] * 4 : 0);
    const size_t o_la = st.add(lk.d_permuted_inputs, K * n_lk * sizeof(void *)), o_ls = st.add(lk.d_permuted_tables, K * n_lk * sizeof(void *));
    const size_t o_lz = st.add(lk.d_products, K * n_lk * sizeof(void *));
    const size_t o_pr = st.add(proofs.data(), K * sizeof(hsw::QuotientProof)), o_ti = st.add(t_inv.data(), t_inv.size() * sizeof(PFe));
    const size_t o_h = st.add(a.d_h, K * sizeof(void *)), o_k = st.add(&kc, sizeof kc);
    const size_t o_v = st.work(scratch_bytes);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    hsw::QuotientParams p{};
    p.N = (uint32_t)N; p.mask = (uint32_t)(N - 1); p.ext = 1u << ext_log; p.u_off = (uint32_t)((a.usable_rows << ext_log) & (N - 1));
    p.m = (uint32_t)m; p.F = (uint32_t)F;
    p.cols = hsw::at<const PFe *const>(d, o_cols); p.fixed = hsw::at<const PFe *const>(d, o_fixed);
    p.l0 = static_cast<const PFe *>(a.d_l0); p.l_last = static_cast<const PFe *>(a.d_l_last); p.l_active = static_cast<const PFe *>(a.d_l_active);
    p.n_gates = (uint32_t)ga.n_gates; p.n_perm = (uint32_t)n_perm; p.L = L; p.S = (uint32_t)S;
    p.gate_first_term = hsw::at<const uint32_t>(d, o_gft); p.term_first_factor = hsw::at<const uint32_t>(d, o_tff);
    p.factor_column = hsw::at<const uint32_t>(d, o_fc); p.factor_offset = hsw::at<const uint32_t>(d, o_fo);
    p.term_coeff = hsw::at<const PFe>(d, o_coeff);
    p.perm_columns = hsw::at<const uint32_t>(d, o_pc); p.sigmas = hsw::at<const PFe *const>(d, o_sig);
    p.perm_z = hsw::at<const PFe *const>(d, o_pz); p.beta_delta = hsw::at<const PFe>(d, o_bd);
    p.powers = hsw::at<const hsw::PermutationPowers>(d, o_pw);
    p.n_lookups = (uint32_t)n_lk;
    p.first_input = hsw::at<const uint32_t>(d, o_fi); p.inputs = hsw::at<const uint32_t>(d, o_in);
    p.first_table = hsw::at<const uint32_t>(d, o_ft); p.tables = hsw::at<const uint32_t>(d, o_tb);
    p.lk_a = hsw::at<const PFe *const>(d, o_la); p.lk_s = hsw::at<const PFe *const>(d, o_ls); p.lk_z = hsw::at<const PFe *const>(d, o_lz);
    p.proofs = hsw::at<const hsw::QuotientProof>(d, o_pr); p.t_inv = hsw::at<const PFe>(d, o_ti);
    p.h = hsw::at<PFe *const>(d, o_h); p.V = hsw::at<PFe>(d, o_v);
    p.status = hsw::at<uint32_t>(d, 0); p.k = hsw::at<const hsw::QuotientConstants>(d, o_k);
    const hipStream_t stream = es.stream;
    // the families of every batch, then its finish: an event at every boundary, summed per family afterwards
    hsw::Events ev;
    std::vector<int> stage;                                      // what ran between event i and i + 1: 0 gates, 1 permutation, 2 lookups, 3 finish
    hipError_t he = hsw::upload(st, d, stream, ev);
    uint32_t launches = 0;
    for (size_t k0 = 0; he == hipSuccess && k0 < K; k0 += per_batch) {
        const uint32_t nb = (uint32_t)std::min(per_batch, K - k0), base = (uint32_t)k0;
        p.first = 1;
        for (int family = 0; he == hipSuccess && family < 4; family++) {
            if (family == 0 && !ga.n_gates) continue;
            if (family == 1 && !n_perm) continue;
            if (family == 2 && !n_lk) continue;
            if (family == 0) he = hsw::launch_quotient_gates(p, base, nb, stream);
            else if (family == 1) he = hsw::launch_quotient_permutation(p, base, nb, mont, stream);
            else if (family == 2) he = hsw::launch_quotient_lookups(p, base, nb, mont, stream);
            else he = hsw::launch_quotient_finish(p, base, nb, stream);
            p.first = 0;
            launches++;
            stage.push_back(family);
            if (he == hipSuccess) he = ev.record(stream);
        }
    }
    std::vector<uint32_t> status(K, 0);
    std::vector<float> between;
    const int frc = hsw::finish(e, he, stream, ev, d, status.data(), K * sizeof(uint32_t), between);
    if (frc != HSW_OK) return frc;
    float ms[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < stage.size(); i++) ms[stage[i]] += between[i];
    for (size_t k = 0; k < K; k++) {
        status[k] &= hsw::QUOTIENT_CELL_NOT_BELOW_P;
        if (status[k]) { if (!report->refused_proofs++) report->first_refused = k; }
        else report->written += N;
    }
    report->proofs = K;
    report->expressions = ga.n_gates + (n_perm ? 2 * S + 1 : 0) + 5 * n_lk;
    report->scratch_bytes = scratch_bytes;
    report->launches = launches;
    report->rows_per_thread = hsw::QUOTIENT_ROWS;
    report->gates_ms = ms[0]; report->permutation_ms = ms[1]; report->lookups_ms = ms[2]; report->finish_ms = ms[3];
    report->kernel_ms = ms[0] + ms[1] + ms[2] + ms[3];
    if (a.status) std::memcpy(a.status, status.data(), K * sizeof(uint32_t));
    return HSW_OK;
} HSW_NO_UNWIND
