// hsw_gadget_permutation.cpp -- the grand products Z of halo2's permutation argument (include/hsw.h, "permutation
// argument's grand products"): every refusal decided on the host, the caller's pointers staged with beta delta^j per
// column and omega's powers (hsw_permutation_value.hpp), then the three launches of hsw_permutation_product.hip.  A
// translation unit of its own: only the entry point below refers to those kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_nounwind.hpp"
#include "hsw_permutation_product.h"

namespace {

using hsw::fail_at;
using hsw::Interval;

const size_t NO_PROOF = ~(size_t)0;                            // a sigma column is every proof's

bool load_below_p(hsw::PFe &x, const void *stored, size_t k) { return hsw::load_below_p(x, static_cast<const uint8_t *>(stored) + 32 * k); }

}  // namespace

extern "C" int hsw_gadget_permutation_product(hsw_gadget *g, const hsw_permutation_product *args, hsw_permutation_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->tile_rows = hsw::PRODUCT_TILE;
    report->first_open = report->first_refused = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const uint64_t u = args->usable_rows;
    const size_t K = (size_t)c.contexts(), m = args->n_columns, L = args->chunk_columns;
    if (u == 0 || m == 0 || L == 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "usable_rows, n_columns and chunk_columns are at least 1");
    if (args->flags) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    if (u > (1ull << 31)) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "usable_rows above 2^31");
    if (m > 0x7fffffffull / K) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "too many columns");
    if (!args->d_columns || !args->d_sigmas || !args->d_products) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a column pointer array is NULL");
    const size_t S = (m + L - 1) / L;
    std::vector<Interval> iv;
    iv.reserve(K * (m + S) + m);
    const auto column = [&](const void *ptr, uint64_t cells, size_t proof, bool z) {
        const uintptr_t at = reinterpret_cast<uintptr_t>(ptr);
        if (!at || (at & 15u)) return false;
        if (cells) iv.push_back(Interval{at, at + (uintptr_t)cells * HSW_CELL_BYTES, proof, z, 0});
        return true;
    };
    for (size_t j = 0; j < m; j++)
        if (!column(args->d_sigmas[j], u, NO_PROOF, false)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a sigma column pointer that is NULL or not 16-byte aligned");
    for (size_t k = 0; k < K; k++) {
        for (size_t j = 0; j < m; j++) {
            const uint64_t rows = args->column_rows ? args->column_rows[k * m + j] : u;
            if (rows > u) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "column_rows above usable_rows");
            if (!column(args->d_columns[k * m + j], rows, k, false)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a column pointer that is NULL or not 16-byte aligned");
        }
        for (size_t s = 0; s < S; s++)
            if (!column(args->d_products[k * S + s], u + 1, k, true)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", k, "a Z column pointer that is NULL or not 16-byte aligned");
    }
    // a Z column may overlap neither a column that is read nor another Z column: the proof named is the Z column's
    Interval writer{}, with{};
    if (hsw::output_overlaps(iv, &writer, &with)) return fail_at(e, HSW_ERR_INVALID_ARG, "proof", writer.index, "a Z column of its overlaps a column read or another Z column");
    if (!args->betas || !args->gammas || !args->omega || !args->delta) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a challenge, omega or delta is NULL");
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    hsw::PFe omega, delta;
    if (!load_below_p(omega, args->omega, 0) || !load_below_p(delta, args->delta, 0))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega or delta whose stored limbs are not below p");
    const hsw::PFe delta_mont = hsw::permutation_to_mont(delta, mont);
    std::vector<hsw::PermutationChallenges> ch(K);
    std::vector<hsw::PFe> beta_delta(K * m);
    for (size_t k = 0; k < K; k++) {
        hsw::PFe beta;
        if (!load_below_p(beta, args->betas, k) || !load_below_p(ch[k].gamma, args->gammas, k))
            return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a challenge whose stored limbs are not below p");
        ch[k].beta_mul = hsw::product_theta_mul(beta, mont);
        for (size_t j = 0; j < m; j++) beta_delta[k * m + j] = j ? hsw::permutation_next_beta_delta(beta_delta[k * m + j - 1], delta_mont) : beta;
    }
    const uint64_t n_tiles = (u + 1 + hsw::PRODUCT_TILE - 1) / hsw::PRODUCT_TILE;
    if (S > 0x7fffffffull / n_tiles || K > 0x7fffffffull / (S * n_tiles)) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "too many tiles for one launch");
    hsw::PermutationPowers powers;
    hsw::permutation_stage_powers(hsw::permutation_to_mont(omega, mont), hsw::PRODUCT_ROWS, powers);
    // device staging: [status words][columns][beta delta^j][sigma pointers][Z pointers][challenges][omega's powers][tile products]
    hsw::Staging st;
    st.zeroed(K * sizeof(uint32_t));
    const size_t off_cols = st.zeroed(K * m * sizeof(hsw::PermutationColumn)), off_bd = st.add(beta_delta.data(), beta_delta.size() * sizeof(hsw::PFe));
    const size_t off_sig = st.add(args->d_sigmas, m * sizeof(void *)), off_z = st.add(args->d_products, K * S * sizeof(void *));
    const size_t off_ch = st.add(ch.data(), ch.size() * sizeof(hsw::PermutationChallenges)), off_pw = st.add(&powers, sizeof powers);
    const size_t off_tiles = st.work(K * S * (size_t)n_tiles * 2 * sizeof(hsw::PFe));
    for (size_t k = 0; k < K * m; k++)
        st.image<hsw::PermutationColumn>(off_cols)[k] = hsw::PermutationColumn{static_cast<const uint4 *>(args->d_columns[k]), (uint32_t)(args->column_rows ? args->column_rows[k] : u), 0};
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    hsw::PermutationParams p{};
    p.cols = hsw::at<const hsw::PermutationColumn>(d, off_cols);
    p.beta_delta = hsw::at<const hsw::PFe>(d, off_bd);
    p.sigmas = hsw::at<const uint4 *const>(d, off_sig);
    p.z = hsw::at<uint4 *const>(d, off_z);
    p.ch = hsw::at<const hsw::PermutationChallenges>(d, off_ch);
    p.powers = hsw::at<const hsw::PermutationPowers>(d, off_pw);
    p.seed_full = hsw::permutation_seed((uint32_t)std::min(L, m), mont);
    p.seed_last = hsw::permutation_seed((uint32_t)(m - (S - 1) * L), mont);
    p.n_proofs = (uint32_t)K; p.m = (uint32_t)m; p.L = (uint32_t)std::min(L, m); p.S = (uint32_t)S;
    p.n_tiles = (uint32_t)n_tiles; p.u = (uint32_t)u;
    p.tiles = hsw::at<hsw::PFe>(d, off_tiles);
    p.status = hsw::at<uint32_t>(d, 0);
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    if (he == hipSuccess) he = hsw::launch_permutation_tiles(p, mont, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_permutation_scan(p, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_permutation_write(p, mont, stream);
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint32_t> status(K, 0);
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, status.data(), K * sizeof(uint32_t), ms);
    if (frc != HSW_OK) return frc;
    report->tiles_ms = ms[0]; report->scan_ms = ms[1]; report->write_ms = ms[2];
    report->kernel_ms = ms[0] + ms[1] + ms[2];
    report->proofs = K; report->products = K * S;
    for (size_t k = 0; k < K; k++) {
        const uint32_t s = status[k];
        if (s & hsw::PRODUCT_REFUSED) {
            if (!report->refused_proofs++) report->first_refused = k;
            status[k] = s & hsw::PRODUCT_REFUSED;            // (nothing was written: whether it closes was never looked at)
        } else {
            report->written += (u + 1) * S;
            if ((s & hsw::PRODUCT_OPEN) && !report->open_proofs++) report->first_open = k;
        }
    }
    if (args->status) std::memcpy(args->status, status.data(), K * sizeof(uint32_t));
    return HSW_OK;
} HSW_NO_UNWIND
