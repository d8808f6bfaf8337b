// hsw_gadget_product.cpp -- the grand-product column Z of halo2's lookup argument (include/hsw.h, "grand-product column"):
// every refusal decided on the host, the caller's pointers and challenges staged, then the three launches of
// hsw_lookup_product.hip.  A translation unit of its own: only the entry point below refers to those kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_lookup_permuted.h"
#include "hsw_lookup_product.h"
#include "hsw_nounwind.hpp"

static_assert(hsw::PRODUCT_OPEN == HSW_PRODUCT_OPEN && hsw::PRODUCT_ZERO_DENOM == HSW_PRODUCT_ZERO_DENOM &&
                  hsw::PRODUCT_CELL_NOT_BELOW_P == HSW_PRODUCT_CELL_NOT_BELOW_P,
              "the device's status bits are the public ones");

using hsw::fail_at;
using hsw::Interval;

extern "C" int hsw_gadget_lookup_product(hsw_gadget *g, const hsw_lookup_product *args, hsw_product_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->tile_rows = hsw::PRODUCT_TILE;
    report->first_open = report->first_refused = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const bool spread = args->table == HSW_LOOKUP_SPREAD;
    if (args->table != HSW_LOOKUP_RANGE && !spread) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown table");
    if (args->flags & ~HSW_PERMUTED_THETA_ON_SPREAD) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    const uint64_t K = c.contexts(), ncols = c.shape.num_advice_columns;
    const uint64_t T = spread ? 1ull << c.shape.num_bits_lookup : 65536, u = args->usable_rows;
    const size_t n_args = (size_t)(spread ? K * ncols : K);
    if (args->n_arguments != n_args) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_arguments is not the number of arguments of the pass");
    if (u < T) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "usable_rows below the table size");
    if (u > (1ull << 31)) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "usable_rows above 2^31");
    if (!args->d_inputs || !args->d_permuted_inputs || !args->d_permuted_tables || !args->d_products || (spread && !args->d_inputs_spread))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a column pointer array is NULL");
    std::vector<Interval> iv;
    iv.reserve(5 * n_args);
    for (size_t a = 0; a < n_args; a++) {
        const uint64_t rows = args->input_rows ? args->input_rows[a] : u;
        if (rows > u) return fail_at(e, HSW_ERR_INVALID_ARG, "argument", a, "input_rows above usable_rows");
        const uintptr_t col[5] = {reinterpret_cast<uintptr_t>(args->d_inputs[a]), spread ? reinterpret_cast<uintptr_t>(args->d_inputs_spread[a]) : 16,
                                  reinterpret_cast<uintptr_t>(args->d_permuted_inputs[a]), reinterpret_cast<uintptr_t>(args->d_permuted_tables[a]),
                                  reinterpret_cast<uintptr_t>(args->d_products[a])};
        const uint64_t cells[5] = {rows, spread ? rows : 0, u, u, u + 1};
        for (int k = 0; k < 5; k++) {
            if (!col[k] || (col[k] & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "argument", a, "a column pointer that is NULL or not 16-byte aligned");
            if (cells[k]) iv.push_back(Interval{col[k], col[k] + (uintptr_t)cells[k] * HSW_CELL_BYTES, a, k == 4, 0});
        }
    }
    // a Z column may overlap neither a column that is read nor another Z column; the argument named is the one whose
    // interval comes later in address order (of two that start together, the later argument)
    Interval writer{}, with{};
    if (hsw::output_overlaps(iv, &writer, &with)) {
        const bool writer_later = with.out || writer.lo > with.lo || (writer.lo == with.lo && writer.index > with.index);
        return fail_at(e, HSW_ERR_INVALID_ARG, "argument", writer_later ? writer.index : with.index, "its Z column overlaps a column read or another Z column, or its columns overlap another argument's Z");
    }
    if (!args->betas || !args->gammas || (spread && !args->thetas)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a challenge array is NULL");
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    std::vector<hsw::ProductChallenges> ch((size_t)K);
    for (size_t k = 0; k < (size_t)K; k++) {
        hsw::ProductChallenges &x = ch[k];
        x.theta = hsw::fr_zero();
        if (spread) std::memcpy(&x.theta, static_cast<const uint8_t *>(args->thetas) + 32 * k, 32);
        std::memcpy(&x.beta, static_cast<const uint8_t *>(args->betas) + 32 * k, 32);
        std::memcpy(&x.gamma, static_cast<const uint8_t *>(args->gammas) + 32 * k, 32);
        if (!hsw::pfe_below_p(x.theta) || !hsw::pfe_below_p(x.beta) || !hsw::pfe_below_p(x.gamma))
            return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a challenge whose stored limbs are not below p");
        x.theta_mul = hsw::product_theta_mul(x.theta, mont);
    }
    const uint64_t n_tiles = (u + 1 + hsw::PRODUCT_TILE - 1) / hsw::PRODUCT_TILE;
    if (n_tiles * n_args > 0x7fffffffull) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "too many tiles for one launch");
    // device staging: [status words][arguments][challenges][tile products]
    hsw::Staging st;
    st.zeroed(n_args * sizeof(uint32_t));
    const size_t off_args = st.zeroed(n_args * sizeof(hsw::ProductArg)), off_ch = st.add(ch.data(), ch.size() * sizeof(hsw::ProductChallenges));
    const size_t off_tiles = st.work(n_args * (size_t)n_tiles * 2 * sizeof(hsw::PFe));
    for (size_t a = 0; a < n_args; a++)
        st.image<hsw::ProductArg>(off_args)[a] = hsw::ProductArg{static_cast<const uint4 *>(args->d_inputs[a]), spread ? static_cast<const uint4 *>(args->d_inputs_spread[a]) : nullptr,
                                                                 static_cast<const uint4 *>(args->d_permuted_inputs[a]), static_cast<const uint4 *>(args->d_permuted_tables[a]),
                                                                 static_cast<uint4 *>(args->d_products[a]), (uint32_t)(args->input_rows ? args->input_rows[a] : u),
                                                                 (uint32_t)(spread ? a / ncols : a)};
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    hsw::ProductParams p{};
    p.args = hsw::at<const hsw::ProductArg>(d, off_args);
    p.ch = hsw::at<const hsw::ProductChallenges>(d, off_ch);
    p.n_args = (uint32_t)n_args; p.n_tiles = (uint32_t)n_tiles;
    p.T = (uint32_t)T; p.u = (uint32_t)u;
    p.kind = !spread ? hsw::PERMUTED_VALUE_RANGE
                     : args->flags & HSW_PERMUTED_THETA_ON_SPREAD ? hsw::PERMUTED_VALUE_THETA_ON_SPREAD : hsw::PERMUTED_VALUE_SPREAD;
    p.tiles = hsw::at<hsw::PFe>(d, off_tiles);
    p.status = hsw::at<uint32_t>(d, 0);
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    if (he == hipSuccess) he = hsw::launch_product_tiles(p, mont, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_product_scan(p, stream);
    if (he == hipSuccess) he = ev.record(stream);
    if (he == hipSuccess) he = hsw::launch_product_write(p, mont, stream);
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint32_t> status(n_args, 0);
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, status.data(), n_args * sizeof(uint32_t), ms);
    if (frc != HSW_OK) return frc;
    report->tiles_ms = ms[0]; report->scan_ms = ms[1]; report->write_ms = ms[2];
    report->kernel_ms = ms[0] + ms[1] + ms[2];
    report->arguments = n_args;
    for (size_t a = 0; a < n_args; a++) {
        const uint32_t s = status[a];
        if (s & hsw::PRODUCT_REFUSED) {
            if (!report->refused_arguments++) report->first_refused = a;
            status[a] = s & hsw::PRODUCT_REFUSED;            // (nothing was written: whether it closes was never looked at)
        } else {
            report->written += u + 1;
            if ((s & hsw::PRODUCT_OPEN) && !report->open_arguments++) report->first_open = a;
        }
    }
    if (args->status) std::memcpy(args->status, status.data(), n_args * sizeof(uint32_t));
    return HSW_OK;
} HSW_NO_UNWIND
