// hsw_gadget_ntt.cpp -- the Fr NTT of device columns (include/hsw.h, "the Fr NTT of device columns"): every refusal
// decided on the host, omega, shift and scale brought into Montgomery form and staged as windows and tile tables
// (hsw_ntt_value.hpp), the table of omega's powers built or found in the gadget's cache, then the launches of
// hsw_ntt.hip, group of columns by group.  A translation unit of its own: only the entry point below refers to those
// kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_nounwind.hpp"
#include "hsw_ntt.h"

namespace {

const size_t NTT_GRID_COLUMNS = 65535;                         // blockIdx.y

using hsw::fail_at;
using hsw::Interval;
using hsw::load_below_p;

}  // namespace

extern "C" int hsw_gadget_ntt(hsw_gadget *g, const hsw_ntt *args, hsw_ntt_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->first_refused = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const size_t n = args->n_columns;
    const uint32_t L = args->log_n;
    if (n == 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_columns is at least 1");
    if (args->flags & ~HSW_NTT_SHIFT_AFTER) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    if (L < 1 || L > hsw::NTT_MAX_LOG) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "log_n is 1 .. 28");
    hsw::NttPlan plan;
    if (!hsw::ntt_plan(L, args->pass_log, plan)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "pass_log is 0 .. 10");
    if (!args->d_inputs || !args->d_outputs) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a column pointer array is NULL");
    const uint64_t N = 1ull << L;
    std::vector<Interval> iv;
    iv.reserve(2 * n);
    for (size_t b = 0; b < n; b++) {
        const uint64_t rows = args->input_rows ? args->input_rows[b] : N;
        if (rows > N) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "input_rows above 2^log_n");
        const uintptr_t in = reinterpret_cast<uintptr_t>(args->d_inputs[b]), out = reinterpret_cast<uintptr_t>(args->d_outputs[b]);
        if (!in || (in & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "an input pointer that is NULL or not 16-byte aligned");
        if (!out || (out & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "an output pointer that is NULL or not 16-byte aligned");
        iv.push_back(Interval{out, out + (uintptr_t)N * HSW_CELL_BYTES, b, true, 0});
        if (rows && in != out) iv.push_back(Interval{in, in + (uintptr_t)rows * HSW_CELL_BYTES, b, false, 0});   // (in place: the output's interval stands for both)
    }
    // an output may overlap neither another output nor an input that is not its own in place
    Interval writer{}, with{};
    if (hsw::output_overlaps(iv, &writer, &with))
        return fail_at(e, HSW_ERR_INVALID_ARG, "column", writer.index, "its output overlaps an input that is not its own in place, or another output");
    if (!args->omega) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega is NULL");
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    hsw::PFe omega, shift = hsw::fr_zero(), scale = hsw::fr_zero();
    if (!load_below_p(omega, args->omega) || (args->shift && !load_below_p(shift, args->shift)) || (args->scale && !load_below_p(scale, args->scale)))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega, shift or scale whose stored limbs are not below p");
    omega = hsw::ntt_to_mont(omega, mont);
    if (!hsw::ntt_root_is_primitive(omega, L)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "omega is not a primitive 2^log_n-th root of unity");
    if (args->shift) shift = hsw::ntt_to_mont(shift, mont);
    if (args->scale) scale = hsw::ntt_to_mont(scale, mont);
    const bool shift_in = args->shift && !(args->flags & HSW_NTT_SHIFT_AFTER);
    const uint32_t out_mode = args->shift && (args->flags & HSW_NTT_SHIFT_AFTER) ? hsw::NTT_OUT_TABLE : args->scale ? hsw::NTT_OUT_SCALE : hsw::NTT_OUT_PLAIN;
    const uint32_t n_pass = plan.n_pass;
    const hsw::NttPass pass0 = hsw::ntt_pass(plan, 0), pass_last = hsw::ntt_pass(plan, n_pass - 1);
    // columns in groups whose points between launches fit the scratch (1 GiB, or what the option "round_scratch" lowers it to)
    const size_t column_bytes = (size_t)N * HSW_CELL_BYTES;
    size_t group = std::min(n, NTT_GRID_COLUMNS);
    if (n_pass > 1) group = std::min(group, std::max<size_t>(1, e->round_scratch / column_bytes));
    // device staging: [status words][columns][shift's windows][tile table in][tile table out][omega's windows][points]
    const size_t tile = (size_t)1 << hsw::NTT_TILE_LOG;
    hsw::Staging st;
    st.zeroed(n * sizeof(uint32_t));
    const size_t off_cols = st.zeroed(n * sizeof(hsw::NttColumn)), off_win = st.zeroed(sizeof(hsw::NttWindows));
    const size_t off_in = st.zeroed(tile * sizeof(hsw::PFe)), off_out = st.zeroed(tile * sizeof(hsw::PFe)), off_tw = st.zeroed(sizeof(hsw::NttWindows));
    const size_t scratch_bytes = n_pass > 1 ? group * column_bytes : 0, off_points = st.work(scratch_bytes);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    // the table of omega's powers: the cache's, or a new one in the slot that is free or was used longest ago
    const size_t table_cells = (size_t)1 << (L - 1);
    hsw_gadget::NttTable *table = nullptr;
    for (hsw_gadget::NttTable &t : g->ntt_tables)
        if (t.stamp && t.log_n == L && std::memcmp(t.root, omega.l, 32) == 0) table = &t;
    const bool cached = table != nullptr;
    if (!cached) {
        table = &g->ntt_tables[0];
        for (hsw_gadget::NttTable &t : g->ntt_tables)
            if (t.stamp < table->stamp) table = &t;
        void *p = nullptr;                                   // (first the new one: a failure loses no table that is still good)
        const hipError_t he = hipMalloc(&p, table_cells * sizeof(hsw::PFe));
        if (he != hipSuccess) return hsw::hip_status(he);
        (void)hipFree(table->d_table);
        *table = hsw_gadget::NttTable{};
        table->d_table = p; table->bytes = table_cells * sizeof(hsw::PFe); table->log_n = L;
        std::memcpy(table->root, omega.l, 32);
    }
    table->stamp = ++g->ntt_stamp;
    void *d = g->scratch.d;
    for (size_t b = 0; b < n; b++) {
        hsw::NttColumn &nc = st.image<hsw::NttColumn>(off_cols)[b];
        nc.in = static_cast<const uint4 *>(args->d_inputs[b]);
        nc.out = static_cast<uint4 *>(args->d_outputs[b]);
        nc.scratch = hsw::at<uint4>(d, off_points + (b % group) * column_bytes);
        nc.rows = (uint32_t)(args->input_rows ? args->input_rows[b] : N);
    }
    if (shift_in || out_mode == hsw::NTT_OUT_TABLE) {
        hsw::NttWindows &win = *st.image<hsw::NttWindows>(off_win);
        hsw::ntt_stage_windows(shift, win);
        // g^(offset) of every place of a tile: where launch 0 loads from, or where the last launch stores to (times c)
        hsw::PFe *tab = st.image<hsw::PFe>(shift_in ? off_in : off_out);
        for (uint32_t l = 0; l < tile; l++) {
            if (shift_in) tab[l] = hsw::ntt_power(win, hsw::ntt_offset(pass0, l));
            else {
                const uint32_t i = hsw::ntt_out_index(plan, hsw::ntt_offset(pass_last, hsw::ntt_store_local(pass_last, l)));
                tab[l] = hsw::ntt_power(win, i & (uint32_t)(N - 1));
                if (args->scale) tab[l] = hsw::fr_mont_mul(tab[l], scale);
            }
        }
    }
    if (!cached) hsw::ntt_stage_windows(omega, *st.image<hsw::NttWindows>(off_tw));
    hsw::NttParams p{};
    p.plan = plan;
    p.twiddle = static_cast<const hsw::PFe *>(table->d_table);
    p.shift = hsw::at<const hsw::NttWindows>(d, off_win);
    p.tile_in = hsw::at<const hsw::PFe>(d, off_in);
    p.tile_out = hsw::at<const hsw::PFe>(d, off_out);
    p.scale = scale;
    p.shift_in = shift_in ? 1u : 0u;
    p.out_mode = out_mode;
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    if (he == hipSuccess && !cached)
        he = hsw::launch_ntt_twiddles(static_cast<hsw::PFe *>(table->d_table), hsw::at<const hsw::NttWindows>(d, off_tw), (uint32_t)table_cells, stream);
    if (he == hipSuccess) he = ev.record(stream);
    for (size_t b0 = 0; he == hipSuccess && b0 < n; b0 += group) {
        p.cols = hsw::at<const hsw::NttColumn>(d, off_cols) + b0;
        p.status = hsw::at<uint32_t>(d, 0) + b0;
        for (uint32_t k = 0; he == hipSuccess && k < n_pass; k++) {
            p.pass = hsw::ntt_pass(plan, k);
            he = hsw::launch_ntt_pass(p, (uint32_t)std::min(group, n - b0), stream);
        }
    }
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint32_t> status(n, 0);
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, status.data(), n * sizeof(uint32_t), ms);
    if (frc != HSW_OK) {
        if (!cached) table->stamp = 0;                       // (the table may not have been built: not to be found again)
        return frc;
    }
    report->twiddle_ms = cached ? 0.0f : ms[0];
    report->kernel_ms = ms[1];
    report->columns = n;
    report->twiddle_bytes = table->bytes;
    report->scratch_bytes = scratch_bytes;
    report->launches = n_pass;
    report->pass_log = args->pass_log ? args->pass_log : (uint32_t)hsw::NTT_TILE_LOG;
    for (size_t b = 0; b < n; b++) {
        status[b] &= hsw::NTT_CELL_NOT_BELOW_P;
        if (status[b]) { if (!report->refused_columns++) report->first_refused = b; }
        else report->written += N;
    }
    if (args->status) std::memcpy(args->status, status.data(), n * sizeof(uint32_t));
    return HSW_OK;
} HSW_NO_UNWIND
