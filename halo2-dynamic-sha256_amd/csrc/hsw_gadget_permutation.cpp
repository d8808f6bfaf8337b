// hsw_gadget_permutation.cpp -- the grand products Z of halo2's permutation argument (include/hsw.h, "permutation
// argument's grand products"): every refusal decided on the host, the caller's pointers staged with beta delta^j per
// column and omega's powers (hsw_permutation_value.hpp), then the three launches of hsw_permutation_product.hip.  A
// translation unit of its own: only the entry point below refers to those kernels.
#include "hsw_gadget_launch.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "hsw_nounwind.hpp"
#include "hsw_permutation_product.h"

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Events {                                     // the stage boundaries of one call
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    hipError_t record(hipStream_t s) {
        hipEvent_t e = nullptr;
        hipError_t he = hipEventCreate(&e);
        if (he != hipSuccess) return he;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
};

const size_t NO_PROOF = ~(size_t)0;                            // a sigma column is every proof's
struct Interval { uintptr_t lo, hi; size_t proof; bool z; };   // bytes [lo, hi) of a Z column of the proof or of a column it reads

int fail_proof(hsw_engine *e, int status, const char *what, size_t c) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "proof %zu: %s", c, what);
    return hsw_engine_fail(e, status, buf);
}

bool load_below_p(hsw::PFe &x, const void *stored, size_t k) {
    std::memcpy(&x, static_cast<const uint8_t *>(stored) + 32 * k, 32);
    return hsw::pfe_below_p(x);
}

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
        if (cells) iv.push_back(Interval{at, at + (uintptr_t)cells * HSW_CELL_BYTES, proof, z});
        return true;
    };
    for (size_t j = 0; j < m; j++)
        if (!column(args->d_sigmas[j], u, NO_PROOF, false)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a sigma column pointer that is NULL or not 16-byte aligned");
    for (size_t k = 0; k < K; k++) {
        for (size_t j = 0; j < m; j++) {
            const uint64_t rows = args->column_rows ? args->column_rows[k * m + j] : u;
            if (rows > u) return fail_proof(e, HSW_ERR_INVALID_ARG, "column_rows above usable_rows", k);
            if (!column(args->d_columns[k * m + j], rows, k, false)) return fail_proof(e, HSW_ERR_INVALID_ARG, "a column pointer that is NULL or not 16-byte aligned", k);
        }
        for (size_t s = 0; s < S; s++)
            if (!column(args->d_products[k * S + s], u + 1, k, true)) return fail_proof(e, HSW_ERR_INVALID_ARG, "a Z column pointer that is NULL or not 16-byte aligned", k);
    }
    // a Z column may overlap neither a column that is read nor another Z column: one sweep in address order, with the
    // furthest end of the Z columns (and whose it is) and of all columns seen so far
    std::sort(iv.begin(), iv.end(), [](const Interval &x, const Interval &y) { return x.lo < y.lo; });
    uintptr_t end_z = 0, end_any = 0;
    size_t z_proof = 0;
    for (const Interval &x : iv) {
        if (x.z ? x.lo < end_any : x.lo < end_z)
            return fail_proof(e, HSW_ERR_INVALID_ARG, "a Z column of its overlaps a column read or another Z column", x.z ? x.proof : z_proof);
        if (x.z && x.hi > end_z) { end_z = x.hi; z_proof = x.proof; }
        end_any = std::max(end_any, x.hi);
    }
    if (!args->betas || !args->gammas || !args->omega || !args->delta) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a challenge, omega or delta is NULL");
    uint32_t repr = 0;
    if (hsw::pass_repr(c, &repr) != HSW_OK) return hsw_engine_fail(e, HSW_ERR_UNSUPPORTED, "the batches of the pass differ in representation");
    if ((repr | c.repr_flags) & HSW_REPR_COMPACT64) return hsw_engine_fail(e, HSW_ERR_UNSUPPORTED, "32-byte cells only");
    const bool mont = (repr & HSW_REPR_MONTGOMERY) != 0;
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
    // device staging: [status words][columns][beta delta^j][sigma pointers][Z pointers][challenges][omega's powers][tile products]
    const size_t off_cols = align256(K * sizeof(uint32_t)), off_bd = align256(off_cols + K * m * sizeof(hsw::PermutationColumn));
    const size_t off_sig = align256(off_bd + K * m * sizeof(hsw::PFe)), off_z = align256(off_sig + m * sizeof(void *));
    const size_t off_ch = align256(off_z + K * S * sizeof(void *)), off_pw = align256(off_ch + K * sizeof(hsw::PermutationChallenges));
    const size_t off_tiles = align256(off_pw + sizeof(hsw::PermutationPowers));
    const size_t bytes = off_tiles + K * S * (size_t)n_tiles * 2 * sizeof(hsw::PFe);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    if (bytes > g->permutation_cap) {                        // (every earlier call has been waited for: nothing reads the old one)
        void *p = nullptr;
        const hipError_t he = hipMalloc(&p, bytes);
        if (he != hipSuccess) return hsw::hip_status(he);
        (void)hipFree(g->d_permutation);
        g->d_permutation = p; g->permutation_cap = bytes;
    }
    uint8_t *d = static_cast<uint8_t *>(g->d_permutation);
    std::vector<uint8_t> host(off_tiles, 0);                 // (the status words start at 0)
    for (size_t k = 0; k < K * m; k++) {
        const hsw::PermutationColumn pc{static_cast<const uint4 *>(args->d_columns[k]), (uint32_t)(args->column_rows ? args->column_rows[k] : u), 0};
        std::memcpy(host.data() + off_cols + k * sizeof pc, &pc, sizeof pc);
    }
    std::memcpy(host.data() + off_bd, beta_delta.data(), beta_delta.size() * sizeof(hsw::PFe));
    std::memcpy(host.data() + off_sig, args->d_sigmas, m * sizeof(void *));
    std::memcpy(host.data() + off_z, args->d_products, K * S * sizeof(void *));
    std::memcpy(host.data() + off_ch, ch.data(), ch.size() * sizeof(hsw::PermutationChallenges));
    hsw::PermutationPowers powers;
    hsw::permutation_stage_powers(hsw::permutation_to_mont(omega, mont), hsw::PRODUCT_ROWS, powers);
    std::memcpy(host.data() + off_pw, &powers, sizeof powers);
    hsw::PermutationParams p{};
    p.cols = reinterpret_cast<const hsw::PermutationColumn *>(d + off_cols);
    p.beta_delta = reinterpret_cast<const hsw::PFe *>(d + off_bd);
    p.sigmas = reinterpret_cast<const uint4 *const *>(d + off_sig);
    p.z = reinterpret_cast<uint4 *const *>(d + off_z);
    p.ch = reinterpret_cast<const hsw::PermutationChallenges *>(d + off_ch);
    p.powers = reinterpret_cast<const hsw::PermutationPowers *>(d + off_pw);
    p.seed_full = hsw::permutation_seed((uint32_t)std::min(L, m), mont);
    p.seed_last = hsw::permutation_seed((uint32_t)(m - (S - 1) * L), mont);
    p.n_proofs = (uint32_t)K; p.m = (uint32_t)m; p.L = (uint32_t)std::min(L, m); p.S = (uint32_t)S;
    p.n_tiles = (uint32_t)n_tiles; p.u = (uint32_t)u;
    p.tiles = reinterpret_cast<hsw::PFe *>(d + off_tiles);
    p.status = reinterpret_cast<uint32_t *>(d);
    const hipStream_t stream = es.stream;
    Events ev;
    hipError_t he = hipMemcpyAsync(d, host.data(), host.size(), hipMemcpyHostToDevice, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_permutation_tiles(p, mont, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_permutation_scan(p, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_permutation_write(p, mont, stream);
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint32_t> status(K, 0);
    if (he == hipSuccess) he = hipMemcpyAsync(status.data(), d, K * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    float ms[3] = {0, 0, 0};
    for (size_t i = 0; he == hipSuccess && i < 3; i++) he = hipEventElapsedTime(&ms[i], ev.ev[i], ev.ev[i + 1]);
    e->timed = false;
    if (he != hipSuccess) return hsw_engine_fail(e, HSW_ERR_HIP, hipGetErrorString(he));
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
