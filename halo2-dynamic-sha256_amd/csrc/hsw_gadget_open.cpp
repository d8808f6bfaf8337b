// hsw_gadget_open.cpp -- device columns evaluated at points and opened (include/hsw.h, "evaluate device columns at
// points, and open them"): every refusal decided on the host, the points and challenges brought into Montgomery form
// and staged with their powers (hsw_open_value.hpp), the groups (or the columns of evaluate) cut into batches whose
// scratch stays under 1 GiB (the engine option "round_scratch" lowers it), then the launches of hsw_open.hip batch by
// batch.  A translation unit of its own: only the two entry points below refer to those kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <cstring>

#include "hsw_nounwind.hpp"
#include "hsw_open.h"

namespace {

const size_t OPEN_GRID_Y = 65535;                              // blockIdx.y

using hsw::align256;
using hsw::fail_at;
using hsw::Interval;
using hsw::load_below_p;

// what both calls ask of rows, tile_rows, the columns and the representation; 0 or the status to return
int check_common(hsw_engine *e, hsw::Context &c, uint32_t flags, uint64_t rows, uint32_t tile_rows, size_t n_columns,
                 const void *const *d_columns, const uint64_t *input_rows, hsw::OpenGeometry &geo, bool &mont) {
    if (flags) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "unknown flag");
    if (rows < 1 || rows > (1ull << hsw::OPEN_MAX_ROWS_LOG)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "rows is 1 .. 2^28");
    if (!hsw::open_geometry(rows, tile_rows, geo)) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "tile_rows 0 or a power of two, 256 .. 2^20");
    if (n_columns == 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_columns is at least 1");
    if (n_columns > 0xFFFFFFFFull) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_columns is below 2^32");
    if (!d_columns) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "the column pointer array is NULL");
    for (size_t b = 0; b < n_columns; b++) {
        if (input_rows && input_rows[b] > rows) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "input_rows above rows");
        const uintptr_t in = reinterpret_cast<uintptr_t>(d_columns[b]);
        if (!in || (in & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "a pointer that is NULL or not 16-byte aligned");
    }
    return hsw::pass_cells(c, &mont);
}

}  // namespace

extern "C" int hsw_gadget_evaluate(hsw_gadget *g, const hsw_evaluate *args, hsw_evaluate_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->first_refused = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const size_t n = args->n_columns, n_points = args->n_points, n_queries = args->n_queries;
    hsw::OpenGeometry geo;
    bool mont = false;
    const int rc = check_common(e, c, args->flags, args->rows, args->tile_rows, n, args->d_columns, args->input_rows, geo, mont);
    if (rc != HSW_OK) return rc;
    if (n_points == 0 || n_points > 0xFFFFFFFFull) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_points is at least 1");
    if (n_queries == 0 || n_queries > 0xFFFFFFFFull) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_queries is at least 1");
    if (!args->points) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "points is NULL");
    if (!args->query_column || !args->query_point) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a query index array is NULL");
    if (!args->out_evals) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "out_evals is NULL");
    std::vector<hsw::PFe> z(n_points);
    for (size_t t = 0; t < n_points; t++)
        if (!load_below_p(z[t], static_cast<const uint8_t *>(args->points) + 32 * t)) return fail_at(e, HSW_ERR_INVALID_ARG, "point", t, "its stored limbs are not below p");
    // the items: the distinct (column, point) pairs, by column
    std::vector<uint64_t> pairs(n_queries);
    for (size_t i = 0; i < n_queries; i++) {
        if (args->query_column[i] >= n) return fail_at(e, HSW_ERR_INVALID_ARG, "query", i, "its column index is out of range");
        if (args->query_point[i] >= n_points) return fail_at(e, HSW_ERR_INVALID_ARG, "query", i, "its point index is out of range");
        pairs[i] = ((uint64_t)args->query_column[i] << 32) | args->query_point[i];
    }
    const std::vector<uint64_t> query_pair(pairs);
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const size_t n_items = pairs.size();
    std::vector<uint32_t> query_item(n_queries);                 // where a query's evaluation will lie
    for (size_t i = 0; i < n_queries; i++) query_item[i] = (uint32_t)(std::lower_bound(pairs.begin(), pairs.end(), query_pair[i]) - pairs.begin());
    std::vector<hsw::OpenColumn> cols;                           // the columns that have a query
    std::vector<hsw::OpenItem> items(n_items);
    for (size_t i = 0; i < n_items; i++) {
        const uint32_t b = (uint32_t)(pairs[i] >> 32);
        items[i] = hsw::OpenItem{(uint32_t)pairs[i], b};
        if (cols.empty() || cols.back().status != b) {
            hsw::OpenColumn oc{};
            oc.cells = static_cast<const uint4 *>(args->d_columns[b]);
            oc.rows = (uint32_t)(args->input_rows ? args->input_rows[b] : args->rows);
            oc.item_first = (uint32_t)i; oc.n_items = 0; oc.status = b;
            cols.push_back(oc);
        }
        cols.back().n_items++;
    }
    // batches of columns whose tiles' sums fit the scratch
    const size_t item_bytes = (size_t)geo.n_tiles * sizeof(hsw::PFe);
    std::vector<size_t> batch_first{0};
    size_t scratch_bytes = 0, acc = 0;
    for (size_t k = 0; k < cols.size(); k++) {
        const size_t need = cols[k].n_items * item_bytes;
        if (k > batch_first.back() && (acc + need > e->round_scratch || k - batch_first.back() >= OPEN_GRID_Y)) { batch_first.push_back(k); acc = 0; }
        acc += need;
        scratch_bytes = std::max(scratch_bytes, acc);
    }
    batch_first.push_back(cols.size());
    // device staging: [status words][evaluations][columns][items][points][the tiles' sums]
    hsw::Staging st;
    st.zeroed(n * sizeof(uint32_t));
    const size_t off_evals = st.zeroed(n_items * sizeof(hsw::PFe)), off_cols = st.add(cols.data(), cols.size() * sizeof(hsw::OpenColumn));
    const size_t off_items = st.add(items.data(), n_items * sizeof(hsw::OpenItem)), off_points = st.zeroed(n_points * sizeof(hsw::OpenPoint));
    const size_t off_tiles = st.work(scratch_bytes);
    for (size_t t = 0; t < n_points; t++) hsw::open_stage_point(hsw::open_to_mont(z[t], mont), geo, st.image<hsw::OpenPoint>(off_points)[t]);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    hsw::OpenParams p{};
    p.geo = geo;
    p.cols = hsw::at<const hsw::OpenColumn>(d, off_cols);
    p.items = hsw::at<const hsw::OpenItem>(d, off_items);
    p.points = hsw::at<const hsw::OpenPoint>(d, off_points);
    p.tiles = hsw::at<uint4>(d, off_tiles);
    p.evals = hsw::at<uint4>(d, off_evals);
    p.status = hsw::at<uint32_t>(d, 0);
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    uint32_t launches = 0;
    for (size_t k = 0; he == hipSuccess && k + 1 < batch_first.size(); k++) {
        const size_t c0 = batch_first[k], c1 = batch_first[k + 1];
        p.base = (uint32_t)c0;
        p.item_base = cols[c0].item_first;
        const uint32_t batch_items = (c1 < cols.size() ? cols[c1].item_first : (uint32_t)n_items) - p.item_base;
        he = hsw::launch_evaluate_tiles(p, (uint32_t)(c1 - c0), stream);
        if (he == hipSuccess) he = hsw::launch_open_scan(p, batch_items, stream);
        launches += 2;
    }
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint8_t> back(off_cols);
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, back.data(), back.size(), ms);
    if (frc != HSW_OK) return frc;
    std::vector<uint32_t> status(n);
    std::memcpy(status.data(), back.data(), n * sizeof(uint32_t));
    for (size_t b = 0; b < n; b++) {
        status[b] &= hsw::OPEN_CELL_NOT_BELOW_P;
        if (status[b] && !report->refused_columns++) report->first_refused = b;
    }
    for (size_t i = 0; i < n_queries; i++) {
        const uint32_t b = args->query_column[i];
        if (status[b]) { report->refused_queries++; continue; }
        const size_t item = query_item[i];
        std::memcpy(static_cast<uint8_t *>(args->out_evals) + 32 * i, back.data() + off_evals + 32 * item, 32);
    }
    report->columns = n;
    report->queries = n_queries;
    report->scratch_bytes = scratch_bytes;
    report->tile_rows = geo.tile_rows;
    report->tiles = geo.n_tiles;
    report->thread_rows = hsw::OPEN_ROWS;
    report->launches = launches;
    report->kernel_ms = ms[0];
    if (args->status) std::memcpy(args->status, status.data(), n * sizeof(uint32_t));
    return HSW_OK;
} HSW_NO_UNWIND

extern "C" int hsw_gadget_open(hsw_gadget *g, const hsw_open *args, hsw_open_report *report) try {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    report->first_refused = ~0ull;
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const size_t n = args->n_columns, n_groups = args->n_groups;
    hsw::OpenGeometry geo;
    bool mont = false;
    const int rc = check_common(e, c, args->flags, args->rows, args->tile_rows, n, args->d_columns, args->input_rows, geo, mont);
    if (rc != HSW_OK) return rc;
    if (n_groups == 0 || n_groups > 0xFFFFFFFFull) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "n_groups is at least 1");
    if (!args->group_first || !args->group_columns) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "a group index array is NULL");
    if (!args->points || !args->challenges) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "points or challenges is NULL");
    if (!args->d_quotients) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "the quotient pointer array is NULL");
    if (args->group_first[0] != 0) return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, "group_first[0] is 0");
    const uint64_t rows = args->rows;
    std::vector<hsw::PFe> z(n_groups), v(n_groups);
    std::vector<Interval> iv;
    iv.reserve(n + n_groups);
    for (size_t b = 0; b < n; b++) {                             // (a column counts with all its `rows` cells, read or not)
        const uintptr_t in = reinterpret_cast<uintptr_t>(args->d_columns[b]);
        iv.push_back(Interval{in, in + (uintptr_t)rows * HSW_CELL_BYTES, b, false, 0});
    }
    for (size_t k = 0; k < n_groups; k++) {
        const uint64_t f0 = args->group_first[k], f1 = args->group_first[k + 1];
        if (f1 <= f0) return fail_at(e, HSW_ERR_INVALID_ARG, "group", k, "an empty group (group_first must increase)");
        if (f1 > 0xFFFFFFFFull) return fail_at(e, HSW_ERR_INVALID_ARG, "group", k, "group_first is below 2^32");
        for (uint64_t i = f0; i < f1; i++)
            if (args->group_columns[i] >= n) return fail_at(e, HSW_ERR_INVALID_ARG, "group", k, "a column index out of range");
        if (!load_below_p(z[k], static_cast<const uint8_t *>(args->points) + 32 * k)) return fail_at(e, HSW_ERR_INVALID_ARG, "group", k, "a point whose stored limbs are not below p");
        if (!load_below_p(v[k], static_cast<const uint8_t *>(args->challenges) + 32 * k)) return fail_at(e, HSW_ERR_INVALID_ARG, "group", k, "a challenge whose stored limbs are not below p");
        const uintptr_t q = reinterpret_cast<uintptr_t>(args->d_quotients[k]);
        if (!q || (q & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "group", k, "a quotient pointer that is NULL or not 16-byte aligned");
        iv.push_back(Interval{q, q + (uintptr_t)rows * HSW_CELL_BYTES, k, true, 0});
    }
    // a quotient may overlap neither the `rows` cells of a column nor another quotient
    Interval writer{}, with{};
    if (hsw::output_overlaps(iv, &writer, &with)) return fail_at(e, HSW_ERR_INVALID_ARG, "group", writer.index, "its quotient overlaps a column or another quotient");
    // batches of groups whose scratch fits: per group the tiles' sums, a cell per thread and, for two columns or more, c
    const size_t n_refs = (size_t)args->group_first[n_groups];
    const size_t tile_bytes = (size_t)geo.n_tiles * sizeof(hsw::PFe), seed_bytes = align256((size_t)geo.seeds * sizeof(hsw::PFe));
    const size_t c_bytes = align256((size_t)rows * sizeof(hsw::PFe));
    std::vector<size_t> batch_first{0};
    size_t scratch_bytes = 0, acc = 0;
    for (size_t k = 0; k < n_groups; k++) {
        const bool folded = args->group_first[k + 1] - args->group_first[k] > 1;
        const size_t need = tile_bytes + seed_bytes + (folded ? c_bytes : 0);
        if (k > batch_first.back() && (acc + need > e->round_scratch || k - batch_first.back() >= OPEN_GRID_Y)) { batch_first.push_back(k); acc = 0; }
        acc += need;
        scratch_bytes = std::max(scratch_bytes, align256(acc));
    }
    batch_first.push_back(n_groups);
    // device staging: [status words][evaluations][columns][group columns][groups][items][points][the scratch of a batch]
    hsw::Staging st;
    st.zeroed(n_groups * sizeof(uint32_t));
    const size_t off_evals = st.zeroed(n_groups * sizeof(hsw::PFe)), off_cols = st.zeroed(n * sizeof(hsw::OpenColumn));
    const size_t off_refs = st.add(args->group_columns, n_refs * sizeof(uint32_t)), off_groups = st.zeroed(n_groups * sizeof(hsw::OpenGroup));
    const size_t off_items = st.zeroed(n_groups * sizeof(hsw::OpenItem)), off_points = st.zeroed(n_groups * sizeof(hsw::OpenPoint));
    const size_t off_scratch = st.work(scratch_bytes);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(st.bytes);
    if (grc != HSW_OK) return grc;
    void *d = g->scratch.d;
    for (size_t b = 0; b < n; b++) {
        hsw::OpenColumn &oc = st.image<hsw::OpenColumn>(off_cols)[b];
        oc.cells = static_cast<const uint4 *>(args->d_columns[b]);
        oc.rows = (uint32_t)(args->input_rows ? args->input_rows[b] : rows);
    }
    for (size_t bk = 0; bk + 1 < batch_first.size(); bk++) {
        const size_t g0 = batch_first[bk], g1 = batch_first[bk + 1];
        size_t off = (g1 - g0) * tile_bytes;                     // the tiles' sums of the batch come first, group after group
        for (size_t k = g0; k < g1; k++) {
            hsw::OpenGroup og{};
            og.first = (uint32_t)args->group_first[k];
            og.m = (uint32_t)(args->group_first[k + 1] - args->group_first[k]);
            og.v = hsw::open_to_mont(v[k], mont);
            og.seeds = hsw::at<uint4>(d, off_scratch + off);
            off += seed_bytes;
            if (og.m > 1) {
                og.c = hsw::at<uint4>(d, off_scratch + off);
                off += c_bytes;
                og.src = og.c; og.src_rows = (uint32_t)rows;
            } else {                                             // one column: it is its own c
                const uint32_t b = args->group_columns[og.first];
                og.src = static_cast<const uint4 *>(args->d_columns[b]);
                og.src_rows = (uint32_t)(args->input_rows ? args->input_rows[b] : rows);
            }
            og.q = static_cast<uint4 *>(args->d_quotients[k]);
            st.image<hsw::OpenGroup>(off_groups)[k] = og;
            st.image<hsw::OpenItem>(off_items)[k] = hsw::OpenItem{(uint32_t)k, (uint32_t)k};
            hsw::open_stage_point(hsw::open_to_mont(z[k], mont), geo, st.image<hsw::OpenPoint>(off_points)[k]);
        }
    }
    hsw::OpenParams p{};
    p.geo = geo;
    p.cols = hsw::at<const hsw::OpenColumn>(d, off_cols);
    p.group_cols = hsw::at<const uint32_t>(d, off_refs);
    p.groups = hsw::at<const hsw::OpenGroup>(d, off_groups);
    p.items = hsw::at<const hsw::OpenItem>(d, off_items);
    p.points = hsw::at<const hsw::OpenPoint>(d, off_points);
    p.tiles = hsw::at<uint4>(d, off_scratch);
    p.evals = hsw::at<uint4>(d, off_evals);
    p.status = hsw::at<uint32_t>(d, 0);
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    uint32_t launches = 0;
    for (size_t bk = 0; he == hipSuccess && bk + 1 < batch_first.size(); bk++) {
        const uint32_t nb = (uint32_t)(batch_first[bk + 1] - batch_first[bk]);
        p.base = p.item_base = (uint32_t)batch_first[bk];
        he = hsw::launch_open_tiles(p, nb, stream);
        if (he == hipSuccess) he = hsw::launch_open_scan(p, nb, stream);
        if (he == hipSuccess) he = hsw::launch_open_write(p, nb, stream);
        launches += 3;
    }
    if (he == hipSuccess) he = ev.record(stream);
    std::vector<uint8_t> back(off_cols);
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, back.data(), back.size(), ms);
    if (frc != HSW_OK) return frc;
    std::vector<uint32_t> status(n_groups);
    std::memcpy(status.data(), back.data(), n_groups * sizeof(uint32_t));
    for (size_t k = 0; k < n_groups; k++) {
        status[k] &= hsw::OPEN_CELL_NOT_BELOW_P;
        if (status[k]) { if (!report->refused_groups++) report->first_refused = k; continue; }
        report->written += rows;
        if (args->out_evals) std::memcpy(static_cast<uint8_t *>(args->out_evals) + 32 * k, back.data() + off_evals + 32 * k, 32);
    }
    report->groups = n_groups;
    report->scratch_bytes = scratch_bytes;
    report->tile_rows = geo.tile_rows;
    report->tiles = geo.n_tiles;
    report->thread_rows = hsw::OPEN_ROWS;
    report->launches = launches;
    report->batches = (uint32_t)(batch_first.size() - 1);
    report->kernel_ms = ms[0];
    if (args->status) std::memcpy(args->status, status.data(), n_groups * sizeof(uint32_t));
    return HSW_OK;
} HSW_NO_UNWIND
