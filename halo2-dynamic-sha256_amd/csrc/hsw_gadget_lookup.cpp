// hsw_gadget_lookup.cpp -- the lookup entries of a pass (include/hsw.h, "lookup-table multiplicities"): listed as runs
// of device cells from the accessors the launches and deliveries use (Context::lookup_extra, chip_column_cell), and
// counted on the device by hsw_lookup_counts_kernel.  A translation unit of its own next to hsw_gadget.cpp: only the
// two entry points below refer to the new kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_lookup_counts.h"
#include "hsw_nounwind.hpp"

namespace {

int list_runs(const hsw_gadget *g, std::vector<hsw_lookup_run> &runs) {
    const hsw::Context &c = *g->ctx;
    runs.clear();
    const uint64_t K = c.contexts();
    // ---- RANGE: every committed digest's own lookup entries, prologue to epilogue; positions are those of
    // hsw_hash_result (Context cx's column starts at cx * lookup_pitch()), addresses lookup_extra(cx) further
    if (c.whole && c.d_lookup) {
        for (const hsw::Context::BatchRecord &b : c.batches) {
            if (b.n_blocks == 0) continue;                      // (nothing was launched: nothing was written)
            for (size_t d = b.first_digest; d < b.first_digest + b.n_digests && d < g->results.size(); d++) {
                const hsw::AssignedHashResult &r = g->results[d];
                hsw_frame_shape fs;
                const int rc = hsw_frame_query(&c.shape, g->cfg.max_variable_byte_sizes[d], g->cfg.is_input_range_check ? 1 : 0, &fs);
                if (rc != HSW_OK) return rc;
                const uint64_t cx = c.context_of(d), col0 = K > 1 ? cx * c.lookup_pitch() : 0;
                const uint64_t lo = r.prologue_lookup, hi = r.epilogue_lookup + fs.epilogue_lookups;
                if (hi <= lo) continue;
                if (!runs.empty() && runs.back().context == cx && runs.back().first + runs.back().n == lo - col0) {
                    runs.back().n += hi - lo;                   // nothing of the caller's in between
                    continue;
                }
                hsw_lookup_run o{};
                o.context = cx; o.table = HSW_LOOKUP_RANGE; o.column = 0;
                o.first = lo - col0; o.n = hi - lo;
                o.d_cells = hsw::cell_ptr(c.d_lookup, lo + c.lookup_extra(cx));
                runs.push_back(o);
            }
        }
    }
    // ---- SPREAD: the committed limb calls [n0, n1) of the pass, per Context and chip column
    uint64_t n0 = c.num_limb_sum;
    for (const hsw::Context::BatchRecord &b : c.batches)
        if (b.n_blocks) n0 = std::min<uint64_t>(n0, (uint64_t)b.first_block * c.shape.limb_calls_per_block);
    const uint64_t n1 = c.num_limb_sum, ncols = c.shape.num_advice_columns;
    const uint64_t L = K > 1 ? c.ctx_limb_calls() : n1;           // (K > 1: a whole number of rows per Context)
    for (uint64_t cx = L ? n0 / L : 0; n0 < n1 && cx < K && cx * L < n1; cx++) {
        const uint64_t base = K > 1 ? cx * L : 0;
        const uint64_t lo = std::max(n0, base), hi = K > 1 ? std::min(n1, base + L) : n1;
        for (uint64_t k = 0; k < ncols; k++) {
            const uint64_t nk = lo + (k + ncols - lo % ncols) % ncols;    // the first limb call of column k at or after lo
            if (nk >= hi) continue;
            hsw_lookup_run o{};
            o.context = cx; o.table = HSW_LOOKUP_SPREAD; o.column = (uint32_t)k;
            o.first = (nk - base) / ncols;
            o.n = (hi - nk + ncols - 1) / ncols;
            o.d_cells = hsw::cell_ptr(c.d_chip_dense, c.chip_column_cell(cx, k, false) + o.first);
            o.d_spread = hsw::cell_ptr(c.d_chip_spread, c.chip_column_cell(cx, k, true) + o.first);
            runs.push_back(o);
        }
    }
    std::stable_sort(runs.begin(), runs.end(), [](const hsw_lookup_run &a, const hsw_lookup_run &b) {
        if (a.context != b.context) return a.context < b.context;
        if (a.table != b.table) return a.table < b.table;
        if (a.column != b.column) return a.column < b.column;
        return a.first < b.first;
    });
    return HSW_OK;
}

}  // namespace

extern "C" {

int hsw_gadget_lookup_runs(const hsw_gadget *g, hsw_lookup_run *out, size_t cap, size_t *n) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    std::vector<hsw_lookup_run> runs;
    const int rc = list_runs(g, runs);
    if (rc != HSW_OK) return rc;
    if (n) *n = runs.size();
    if (!out) return HSW_OK;
    if (cap < runs.size()) return HSW_ERR_TOO_LARGE;
    if (!runs.empty()) std::memcpy(out, runs.data(), runs.size() * sizeof runs[0]);
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_lookup_multiplicities(hsw_gadget *g, const hsw_lookup_counts *out, hsw_lookup_report *report) try {
    if (!g || !out || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const uint64_t spread_rows = 1ull << c.shape.num_bits_lookup;
    const uint64_t range_pitch = out->range_pitch ? out->range_pitch : 65536, spread_pitch = out->spread_pitch ? out->spread_pitch : spread_rows;
    if (!out->d_range && !out->d_spread) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "both counter tables are NULL");
    if (out->flags & ~HSW_LOOKUP_ACCUMULATE) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    if ((out->d_range && range_pitch < 65536) || (out->d_spread && spread_pitch < spread_rows))
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a pitch below the table size");
    if ((reinterpret_cast<uintptr_t>(out->d_range) | reinterpret_cast<uintptr_t>(out->d_spread)) & 3u)
        return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a counter table that is not 4-byte aligned");
    if (out->d_range && !(c.whole && c.d_lookup)) return hsw_engine_fail(e, HSW_ERR_UNSUPPORTED, "this gadget has no lookup column");
    bool mont = false;
    const int prc = hsw::pass_cells(c, &mont);
    if (prc != HSW_OK) return prc;
    std::vector<hsw_lookup_run> runs;
    int rc = list_runs(g, runs);
    if (rc != HSW_OK) return rc;
    // the runs of the tables asked for, as the kernel takes them; the proofs whose tables are zeroed first
    std::vector<hsw::LookupRun> dev;
    std::vector<uint32_t> zero_ctx[2];
    uint64_t entries = 0;
    for (const hsw_lookup_run &r : runs) {
        if (!(r.table == HSW_LOOKUP_RANGE ? out->d_range : out->d_spread) || r.n == 0) continue;
        if ((reinterpret_cast<uintptr_t>(r.d_cells) | reinterpret_cast<uintptr_t>(r.d_spread)) & 15u)
            return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a cell address that is not 16-byte aligned");   // (two 16-byte loads per cell)
        (r.table == HSW_LOOKUP_RANGE ? report->range_entries : report->spread_entries) += r.n;
        entries += r.n;
        std::vector<uint32_t> &z = zero_ctx[r.table];
        if (z.empty() || z.back() != (uint32_t)r.context) z.push_back((uint32_t)r.context);   // (context order: once each)
        dev.push_back(hsw::LookupRun{r.d_cells, r.d_spread, r.n, 0, r.context});
    }
    if (dev.empty()) return HSW_OK;
    if (dev.size() >= (1u << 24)) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "more than 2^24 lookup runs");
    // work items of `chunk` entries: small enough that a single proof still fills the chip, large enough that the
    // flush of a workgroup's LDS histogram is a fraction of its loads
    uint64_t chunk = (entries / 2048 + 255) / 256 * 256;
    chunk = std::min<uint64_t>(std::max<uint64_t>(chunk, 256), 4096);
    uint64_t n_chunks = 0;
    for (hsw::LookupRun &r : dev) { r.chunk0 = n_chunks; n_chunks += (r.n + chunk - 1) / chunk; }
    if (n_chunks > 0x7fffffffull) return hsw_engine_fail(e, HSW_ERR_TOO_LARGE, "too many lookup entries for one launch");
    const bool zero = !(out->flags & HSW_LOOKUP_ACCUMULATE);
    // device staging: [report][runs][proofs to zero: range][proofs to zero: spread]
    const size_t off_runs = sizeof(hsw::LookupReport), off_z0 = off_runs + dev.size() * sizeof(hsw::LookupRun);
    const size_t off_z1 = off_z0 + ((zero_ctx[0].size() + 1) / 2) * 8, bytes = off_z1 + ((zero_ctx[1].size() + 1) / 2) * 8;
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    if (bytes > g->lookup_runs_cap) {                        // (every earlier count has been waited for: nothing reads the old one)
        void *p = nullptr;
        const size_t cap = std::max(bytes, 2 * g->lookup_runs_cap);
        const hipError_t he = hipMalloc(&p, cap);
        if (he != hipSuccess) return hsw::hip_status(he);
        (void)hipFree(g->d_lookup_runs);
        g->d_lookup_runs = p; g->lookup_runs_cap = cap;
    }
    std::vector<uint8_t> host(bytes, 0);
    const hsw::LookupReport none{0, ~0ull};
    std::memcpy(host.data(), &none, sizeof none);
    std::memcpy(host.data() + off_runs, dev.data(), dev.size() * sizeof(hsw::LookupRun));
    if (!zero_ctx[0].empty()) std::memcpy(host.data() + off_z0, zero_ctx[0].data(), zero_ctx[0].size() * 4);
    if (!zero_ctx[1].empty()) std::memcpy(host.data() + off_z1, zero_ctx[1].data(), zero_ctx[1].size() * 4);
    uint8_t *d = static_cast<uint8_t *>(g->d_lookup_runs);
    hsw::LookupCountParams p{};
    p.runs = reinterpret_cast<const hsw::LookupRun *>(d + off_runs);
    p.n_runs = (uint32_t)dev.size();
    p.chunk = (uint32_t)chunk;
    p.range = out->d_range; p.spread = out->d_spread;
    p.range_pitch = range_pitch; p.spread_pitch = spread_pitch;
    p.bits = c.shape.num_bits_lookup;
    p.lds_bins = e->lookup_lds ? hsw::LOOKUP_LDS_BINS : 0;
    p.report = reinterpret_cast<hsw::LookupReport *>(d);
    const hipStream_t stream = es.stream;
    hipError_t he = hipMemcpyAsync(d, host.data(), bytes, hipMemcpyHostToDevice, stream);
    if (he == hipSuccess) he = hipEventRecord(e->ev0, stream);
    if (he == hipSuccess && zero && out->d_range)
        he = hsw::launch_lookup_zero(out->d_range, range_pitch, 65536, reinterpret_cast<const uint32_t *>(d + off_z0), zero_ctx[0].size(), stream);
    if (he == hipSuccess && zero && out->d_spread)
        he = hsw::launch_lookup_zero(out->d_spread, spread_pitch, (uint32_t)spread_rows, reinterpret_cast<const uint32_t *>(d + off_z1),
                                     zero_ctx[1].size(), stream);
    if (he == hipSuccess) he = hsw::launch_lookup_counts(p, (size_t)n_chunks, mont, stream);
    if (he == hipSuccess) he = hipEventRecord(e->ev1, stream);
    hsw::LookupReport got{};
    if (he == hipSuccess) he = hipMemcpyAsync(&got, d, sizeof got, hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he == hipSuccess) he = hipEventElapsedTime(&report->kernel_ms, e->ev0, e->ev1);
    e->timed = false;
    if (he != hipSuccess) return hsw_engine_fail(e, HSW_ERR_HIP, hipGetErrorString(he));
    report->not_in_table = got.not_in_table;
    if (got.not_in_table && got.first_key != ~0ull) {
        // (the kernel's run index counts the runs it was given: those of the tables asked for, in list order)
        size_t k = (size_t)(got.first_key >> 40), seen = 0;
        for (const hsw_lookup_run &r : runs) {
            if (!(r.table == HSW_LOOKUP_RANGE ? out->d_range : out->d_spread) || r.n == 0) continue;
            if (seen++ != k) continue;
            report->first_context = r.context; report->first_table = r.table; report->first_column = r.column;
            report->first_entry = r.first + (got.first_key & ((1ull << 40) - 1));
            break;
        }
    }
    return HSW_OK;
} HSW_NO_UNWIND

}  // extern "C"
