// hsw_gadget_permuted.cpp -- halo2's permuted lookup columns of a pass (include/hsw.h, "permuted lookup columns"): the
// arguments' multiplicities counted by hsw_lookup_counts_kernel from the runs hsw_gadget_lookup_runs lists -- one table
// per ARGUMENT, where hsw_gadget_lookup_multiplicities counts one per proof -- or given, then expanded into A' and S' by
// the kernels of hsw_lookup_permuted.hip.  A translation unit of its own: only the entry point below refers to them.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_lookup_permuted.h"
#include "hsw_nounwind.hpp"
#include "hsw_permuted_value.hpp"

extern "C" int hsw_gadget_lookup_permuted(hsw_gadget *g, const hsw_lookup_permuted *args, hsw_permuted_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const bool spread = args->table == HSW_LOOKUP_SPREAD, given = (args->flags & HSW_PERMUTED_GIVEN_M) != 0;
    if (args->table != HSW_LOOKUP_RANGE && !spread) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown table");
    if (args->flags & ~(HSW_PERMUTED_GIVEN_M | HSW_PERMUTED_THETA_ON_SPREAD)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    const uint64_t K = c.contexts(), ncols = c.shape.num_advice_columns;
    const uint64_t T = spread ? 1ull << c.shape.num_bits_lookup : 65536, u = args->usable_rows;
    const size_t n_args = (size_t)(spread ? K * ncols : K);
    if (args->n_arguments != n_args) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_arguments is not the number of arguments of the pass");
    if (u < T) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "usable_rows below the table size");
    if (u > (1ull << 31)) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "usable_rows above 2^31");
    if (!args->d_input_columns || !args->d_table_columns) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a column pointer array is NULL");
    for (size_t a = 0; a < n_args; a++) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(args->d_input_columns[a]), y = reinterpret_cast<uintptr_t>(args->d_table_columns[a]);
        if (!x || !y || ((x | y) & 15u)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a column pointer that is NULL or not 16-byte aligned");
    }
    const uint64_t m_pitch = args->d_m && args->m_pitch ? args->m_pitch : T;
    if (given && !args->d_m) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "HSW_PERMUTED_GIVEN_M without d_m");
    if (m_pitch < T) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "m_pitch below the table size");
    if (reinterpret_cast<uintptr_t>(args->d_m) & 3u) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "d_m is not 4-byte aligned");
    if (!spread && !(c.whole && c.d_lookup)) return hsw_engine_fail(e, HSW_ERR_UNSUPPORTED, "this gadget has no lookup column");
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    std::vector<hsw::PFe> thetas;
    if (spread) {
        if (!args->thetas) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "the spread argument needs thetas");
        thetas.resize((size_t)K);
        std::memcpy(thetas.data(), args->thetas, (size_t)K * sizeof(hsw::PFe));
        for (const hsw::PFe &t : thetas)
            if (!hsw::pfe_below_p(t)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a theta whose stored limbs are not below p");
    }
    // ---- counted mode: the runs of the table asked for, one counter table per argument
    std::vector<hsw_lookup_run> runs;                // (in list order: the kernel's run index counts these)
    std::vector<hsw::LookupRun> dev;
    if (!given) {
        size_t n = 0;
        int rc = hsw_gadget_lookup_runs(g, nullptr, 0, &n);
        if (rc != HSW_OK) return rc;
        std::vector<hsw_lookup_run> all(n);
        if (n && (rc = hsw_gadget_lookup_runs(g, all.data(), n, nullptr)) != HSW_OK) return rc;
        std::vector<uint64_t> per_arg(n_args, 0);
        for (const hsw_lookup_run &r : all) {
            if (r.table != args->table || r.n == 0) continue;
            if ((reinterpret_cast<uintptr_t>(r.d_cells) | reinterpret_cast<uintptr_t>(r.d_spread)) & 15u)
                return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a cell address that is not 16-byte aligned");
            const uint64_t a = spread ? r.context * ncols + r.column : r.context;
            per_arg[(size_t)a] += r.n;
            report->entries += r.n;
            runs.push_back(r);
            dev.push_back(hsw::LookupRun{r.d_cells, r.d_spread, r.n, 0, a});
        }
        for (size_t a = 0; a < n_args; a++)
            if (per_arg[a] > u)
                return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, ("argument " + std::to_string(a) + " has " + std::to_string(per_arg[a]) + " lookup entries, more than usable_rows").c_str());
        if (dev.size() >= (1u << 24)) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "more than 2^24 lookup runs");
    }
    uint64_t chunk = (report->entries / 2048 + 255) / 256 * 256;
    chunk = std::min<uint64_t>(std::max<uint64_t>(chunk, 256), 4096);
    uint64_t n_chunks = 0;
    for (hsw::LookupRun &r : dev) { r.chunk0 = n_chunks; n_chunks += (r.n + chunk - 1) / chunk; }
    if (n_chunks > 0x7fffffffull) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "too many lookup entries for one launch");
    // ---- groups of arguments whose index arrays and value tables fit the budget: whole proofs (SPREAD: a value table
    // per proof), at least one, at most what one grid holds
    const size_t index_bytes = hsw::permuted_index_words((uint32_t)T) * 4, value_bytes = (size_t)T * 32;
    // (m, where it is not the caller's, cannot be grouped -- the flag must be known for every argument before the first
    //  store -- so it is charged to the same budget and may take half of it at the most)
    const size_t m_bytes = args->d_m ? 0 : n_args * (size_t)T * 4;
    if (m_bytes > e->permuted_scratch / 2)
        return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "the multiplicities of all arguments exceed half of permuted_scratch: pass d_m or raise the option");
    const size_t budget = e->permuted_scratch - m_bytes;
    size_t group = spread ? (size_t)ncols * std::max<size_t>(1, budget / (ncols * index_bytes + value_bytes))
                          : std::max<size_t>(1, budget > value_bytes ? (budget - value_bytes) / index_bytes : 1);
    group = std::min(std::min(group, n_args), spread ? (size_t)(65535 / ncols * ncols) : (size_t)65535);
    const size_t group_tables = spread ? group / (size_t)ncols : 1;
    // device staging: [report][thetas][runs][arguments][heads of a group][m, where it is not the caller's][index arrays
    // of a group][value tables of a group]
    const hsw::PermutedReport none{{0, ~0ull}, 0, 0};
    hsw::Staging st;
    st.add(&none, sizeof none);
    const size_t off_thetas = st.add(thetas.data(), thetas.size() * sizeof(hsw::PFe)), off_runs = st.add(dev.data(), dev.size() * sizeof(hsw::LookupRun));
    const size_t off_args = st.zeroed(n_args * sizeof(hsw::PermutedArg));
    const size_t off_heads = st.work(group * sizeof(hsw::PermutedHead)), off_m = st.work(m_bytes), off_index = st.work(group * index_bytes);
    const size_t off_values = st.work(group_tables * value_bytes);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    uint32_t *m_base = args->d_m ? args->d_m : hsw::at<uint32_t>(d, off_m);
    uint4 *d_values = hsw::at<uint4>(d, off_values);
    for (size_t a = 0; a < n_args; a++) {
        const size_t table = spread ? (a % group) / (size_t)ncols : 0;    // its value table among the group's
        st.image<hsw::PermutedArg>(off_args)[a] = hsw::PermutedArg{m_base + a * m_pitch, args->d_input_columns[a], args->d_table_columns[a], d_values + 2 * table * (size_t)T};
    }
    hsw::PermutedReport *d_report = hsw::at<hsw::PermutedReport>(d, 0);
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    // ---- stage 1, all arguments: the multiplicities and the flag
    if (he == hipSuccess && given) he = hsw::launch_permuted_sums(m_base, m_pitch, (uint32_t)T, (uint32_t)u, n_args, d_report, stream);
    if (he == hipSuccess && !given) he = hsw::launch_permuted_zero(m_base, m_pitch, (uint32_t)T, n_args, stream);
    if (he == hipSuccess && !given && !dev.empty()) {
        hsw::LookupCountParams p{};
        p.runs = hsw::at<const hsw::LookupRun>(d, off_runs);
        p.n_runs = (uint32_t)dev.size();
        p.chunk = (uint32_t)chunk;
        p.range = p.spread = m_base;                          // (the kernel's "proof" is the argument: LookupRun::context)
        p.range_pitch = p.spread_pitch = m_pitch;
        p.bits = c.shape.num_bits_lookup;
        p.lds_bins = e->lookup_lds ? hsw::LOOKUP_LDS_BINS : 0;
        p.report = &d_report->count;
        he = hsw::launch_lookup_counts(p, (size_t)n_chunks, mont, stream);
    }
    // ---- stage 2, group by group: index arrays, value tables, the stores (none where the flag is set)
    const uint32_t kind = !spread ? hsw::PERMUTED_VALUE_RANGE
                                  : args->flags & HSW_PERMUTED_THETA_ON_SPREAD ? hsw::PERMUTED_VALUE_THETA_ON_SPREAD : hsw::PERMUTED_VALUE_SPREAD;
    for (size_t a0 = 0; a0 < n_args && he == hipSuccess; a0 += group) {
        hsw::PermutedParams p{};
        p.args = hsw::at<const hsw::PermutedArg>(d, off_args) + a0;
        p.n_args = (uint32_t)std::min(group, n_args - a0);
        p.T = (uint32_t)T; p.u = (uint32_t)u;
        p.index = hsw::at<uint32_t>(d, off_index);
        p.heads = hsw::at<hsw::PermutedHead>(d, off_heads);
        p.report = d_report;
        he = hsw::launch_permuted_prepare(p, stream);
        const size_t tables = spread ? p.n_args / (size_t)ncols : 1;
        if (he == hipSuccess && (spread || a0 == 0))          // (RANGE: one table for every group)
            he = hsw::launch_permuted_values(d_values, hsw::at<const uint32_t>(d, off_thetas) + (spread ? a0 / ncols * 8 : 0), kind,
                                             (uint32_t)T, tables, mont, stream);
        if (he == hipSuccess) he = ev.record(stream);
        if (he == hipSuccess) he = hsw::launch_permuted_write(p, stream);
        if (he == hipSuccess) he = ev.record(stream);
    }
    hsw::PermutedReport got{};
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, &got, sizeof got, ms);
    if (frc != HSW_OK) return frc;
    for (size_t i = 0; i < ms.size(); i++) (i % 2 ? report->write_ms : report->prepare_ms) += ms[i];
    report->kernel_ms = report->prepare_ms + report->write_ms;
    report->arguments = n_args;
    report->not_in_table = got.count.not_in_table;
    report->overflow_arguments = got.overflow;
    report->written = got.count.not_in_table || got.overflow ? 0 : 2 * u * n_args;
    if (got.count.not_in_table && got.count.first_key != ~0ull) {
        const size_t k = (size_t)(got.count.first_key >> 40);
        if (k < runs.size()) {
            const hsw_lookup_run &r = runs[k];
            report->first_context = r.context; report->first_table = r.table; report->first_column = r.column;
            report->first_entry = r.first + (got.count.first_key & ((1ull << 40) - 1));
        }
    }
    return HSW_OK;
} HSW_NO_UNWIND
