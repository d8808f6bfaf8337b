// hsw_gadget_shplonk.cpp -- SHPLONK's multi-point opening of device columns (include/hsw.h, "SHPLONK's multi-point
// opening of device columns"): every refusal decided on the host, the points and challenges brought into Montgomery
// form, lambda, zd, zt and the weight tables made with hsw_shplonk_value.hpp, the points staged with their powers
// (open_stage_point), then the three launches: the tiles and the write of hsw_shplonk.hip around the scan of hsw_open.hip.
// Both entry points are one routine: the second call is the first over ONE set that holds every listed column and h.
// The scratch is not cut into batches: the write launch needs every set's c at once.  A translation unit of its own:
// only the two entry points below refer to those kernels.
#include "hsw_gadget_call.hpp"

#include <algorithm>
#include <array>
#include <cstring>

#include "hsw_nounwind.hpp"
#include "hsw_shplonk.h"

namespace {

using hsw::align256;
using hsw::fail_at;
using hsw::Interval;
using hsw::load_below_p;
using hsw::PFe;

int fail(hsw_engine *e, const char *what) { return hsw_engine_fail(e, HSW_ERR_INVALID_ARG, what); }

int shplonk_call(hsw_gadget *g, const hsw_shplonk *args, hsw_shplonk_report *report, bool open) {
    if (!g || !args || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    hsw::Context &c = *g->ctx;
    hsw_engine *e = c.engine;
    const size_t n = args->n_columns, n_points = args->n_points, n_sets = args->n_sets;
    const uint64_t rows = args->rows;
    hsw::OpenGeometry geo;
    if (args->flags) return fail(e, "unknown flag");
    if (rows < 1 || rows > (1ull << hsw::OPEN_MAX_ROWS_LOG)) return fail(e, "rows is 1 .. 2^28");
    if (!hsw::open_geometry(rows, args->tile_rows, geo)) return fail(e, "tile_rows 0 or a power of two, 256 .. 2^20");
    if (n == 0) return fail(e, "n_columns is at least 1");
    if (n >= 0xFFFFFFFFull) return fail(e, "n_columns is below 2^32 - 1");
    if (!args->d_columns) return fail(e, "the column pointer array is NULL");
    for (size_t b = 0; b < n; b++) {
        if (args->input_rows && args->input_rows[b] > rows) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "input_rows above rows");
        const uintptr_t in = reinterpret_cast<uintptr_t>(args->d_columns[b]);
        if (!in || (in & 15u)) return fail_at(e, HSW_ERR_INVALID_ARG, "column", b, "a pointer that is NULL or not 16-byte aligned");
    }
    bool mont = false;
    const int rc = hsw::pass_cells(c, &mont);
    if (rc != HSW_OK) return rc;
    if (n_points == 0 || n_points > 0xFFFFFFFFull) return fail(e, "n_points is at least 1");
    if (n_sets == 0) return fail(e, "n_sets is at least 1");
    if (n_sets > hsw::SHPLONK_MAX_SETS) return fail(e, "n_sets is at most 65535");
    if (!args->points) return fail(e, "points is NULL");
    if (!args->set_first || !args->set_columns || !args->set_point_first || !args->set_points) return fail(e, "a set index array is NULL");
    if (!args->y || !args->v) return fail(e, "y or v is NULL");
    const uintptr_t out = reinterpret_cast<uintptr_t>(args->d_out), dh = reinterpret_cast<uintptr_t>(args->d_h);
    if (!out || (out & 15u)) return fail(e, "d_out is NULL or not 16-byte aligned");
    if (open) {
        if (!args->u) return fail(e, "u is NULL: the second call takes the challenge u");
        if (!dh || (dh & 15u)) return fail(e, "d_h is NULL or not 16-byte aligned: the second call reads the h of the first");
    } else if (args->u || args->d_h) {
        return fail(e, "u and d_h are NULL for hsw_gadget_shplonk_quotient");
    }
    std::vector<PFe> z(n_points);
    for (size_t t = 0; t < n_points; t++)
        if (!load_below_p(z[t], static_cast<const uint8_t *>(args->points) + 32 * t)) return fail_at(e, HSW_ERR_INVALID_ARG, "point", t, "its stored limbs are not below p");
    PFe y, v, u = hsw::fr_zero();
    if (!load_below_p(y, args->y)) return fail(e, "y: its stored limbs are not below p");
    if (!load_below_p(v, args->v)) return fail(e, "v: its stored limbs are not below p");
    if (open && !load_below_p(u, args->u)) return fail(e, "u: its stored limbs are not below p");
    // the sets: their columns (each listed once in the whole call) and their points (each of T used, none twice in a set)
    if (args->set_first[0] != 0 || args->set_point_first[0] != 0) return fail(e, "set_first[0] and set_point_first[0] are 0");
    std::vector<uint8_t> col_used(n, 0), point_used(n_points, 0);
    for (size_t i = 0; i < n_sets; i++) {
        const uint64_t f0 = args->set_first[i], f1 = args->set_first[i + 1], p0 = args->set_point_first[i], p1 = args->set_point_first[i + 1];
        if (f1 <= f0) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "no column (set_first must increase)");
        if (p1 <= p0) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "no point (set_point_first must increase)");
        if (f1 - f0 > n) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "a column listed twice");
        if (p1 - p0 > hsw::SHPLONK_MAX_SET_POINTS) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "more than HSW_SHPLONK_MAX_SET_POINTS points");
        for (uint64_t k = f0; k < f1; k++) {
            const uint32_t b = args->set_columns[k];
            if (b >= n) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "a column index out of range");
            if (col_used[b]) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "a column listed twice");
            col_used[b] = 1;
        }
        for (uint64_t k = p0; k < p1; k++) {
            const uint32_t t = args->set_points[k];
            if (t >= n_points) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "a point index out of range");
            for (uint64_t l = p0; l < k; l++)
                if (args->set_points[l] == t) return fail_at(e, HSW_ERR_INVALID_ARG, "set", i, "a point index twice");
            point_used[t] = 1;
        }
    }
    for (size_t t = 0; t < n_points; t++)
        if (!point_used[t]) return fail_at(e, HSW_ERR_INVALID_ARG, "point", t, "no set uses it");
    {   // T is a set: no two entries equal in value (one representation: equal values are equal limbs)
        std::vector<std::pair<std::array<uint32_t, 8>, size_t>> sorted(n_points);
        for (size_t t = 0; t < n_points; t++) {
            for (int j = 0; j < 8; j++) sorted[t].first[j] = z[t].l[j];
            sorted[t].second = t;
        }
        std::sort(sorted.begin(), sorted.end());
        for (size_t t = 1; t < n_points; t++)
            if (sorted[t].first == sorted[t - 1].first) return fail_at(e, HSW_ERR_INVALID_ARG, "point", sorted[t].second, "equal in value to another point");
    }
    {   // d_out may overlap neither the `rows` cells of a column (read or not) nor h
        std::vector<Interval> iv;
        iv.reserve(n + 2);
        for (size_t b = 0; b < n; b++) {
            const uintptr_t in = reinterpret_cast<uintptr_t>(args->d_columns[b]);
            iv.push_back(Interval{in, in + (uintptr_t)rows * HSW_CELL_BYTES, b, false, 0});
        }
        if (open) iv.push_back(Interval{dh, dh + (uintptr_t)rows * HSW_CELL_BYTES, n, false, 0});
        iv.push_back(Interval{out, out + (uintptr_t)rows * HSW_CELL_BYTES, 0, true, 0});
        Interval writer{}, with{};
        if (hsw::output_overlaps(iv, &writer, &with)) {
            if (open && with.index == n) return fail(e, "d_out overlaps d_h");
            return fail_at(e, HSW_ERR_INVALID_ARG, "column", with.index, "d_out overlaps it");
        }
    }
    // every constant in Montgomery form
    std::vector<PFe> zm(n_points);
    for (size_t t = 0; t < n_points; t++) zm[t] = hsw::open_to_mont(z[t], mont);
    const PFe ym = hsw::open_to_mont(y, mont), vm = hsw::open_to_mont(v, mont), um = hsw::open_to_mont(u, mont);
    const size_t n_listed = (size_t)args->set_first[n_sets], n_set_points = (size_t)args->set_point_first[n_sets];
    // what the launches walk: the caller's sets, or the one set of the second call
    const size_t k_sets = open ? 1 : n_sets, k_refs = open ? n_listed + 1 : n_listed, k_items = open ? 1 : n_set_points;
    const size_t k_cols = open ? n + 1 : n, k_points = open ? 1 : n_points;
    std::vector<uint32_t> refs(k_refs);
    std::vector<PFe> col_weights(k_refs), item_weights(k_items);
    std::vector<hsw::OpenItem> items(k_items);
    std::vector<hsw::ShplonkSet> sets(k_sets);
    std::memcpy(refs.data(), args->set_columns, n_listed * sizeof(uint32_t));
    if (open) {
        std::vector<PFe> zd(n_sets);
        std::vector<uint8_t> in_set(n_points);
        for (size_t i = 0; i < n_sets; i++) {
            std::fill(in_set.begin(), in_set.end(), 0);
            for (uint64_t k = args->set_point_first[i]; k < args->set_point_first[i + 1]; k++) in_set[args->set_points[k]] = 1;
            zd[i] = hsw::shplonk_vanish(um, zm.data(), (uint32_t)n_points, in_set.data());
        }
        if (hsw::fr_is_zero(zd[0])) return fail(e, "zd_0 = 0: u is a point of T outside the first set");
        const PFe zd0_inv = hsw::fr_inv(zd[0]);
        PFe vi = hsw::fr_one_mont();                             // v^i
        for (size_t i = 0; i < n_sets; i++) {
            const uint64_t f0 = args->set_first[i], m = args->set_first[i + 1] - f0;
            const PFe scale = i ? hsw::fr_mont_mul(vi, hsw::fr_mont_mul(zd[i], zd0_inv)) : hsw::fr_one_mont();
            hsw::shplonk_column_weights(scale, ym, (uint32_t)m, col_weights.data() + f0);
            vi = hsw::fr_mont_mul(vi, vm);
        }
        const PFe zt = hsw::shplonk_vanish(um, zm.data(), (uint32_t)n_points, nullptr);
        refs[n_listed] = (uint32_t)n;                            // h, the last column of the one set
        col_weights[n_listed] = hsw::fr_sub(hsw::fr_zero(), hsw::fr_mont_mul(zt, zd0_inv));
        items[0] = hsw::OpenItem{0, 0};
        item_weights[0] = hsw::fr_one_mont();
        sets[0] = hsw::ShplonkSet{0, (uint32_t)k_refs, 0, 1, (uint32_t)rows, 0, nullptr, nullptr};
    } else {
        PFe vi = hsw::fr_one_mont();
        for (size_t i = 0; i < n_sets; i++) {
            const uint64_t f0 = args->set_first[i], m = args->set_first[i + 1] - f0;
            const uint64_t p0 = args->set_point_first[i], t = args->set_point_first[i + 1] - p0;
            hsw::shplonk_column_weights(hsw::fr_one_mont(), ym, (uint32_t)m, col_weights.data() + f0);
            PFe zs[hsw::SHPLONK_MAX_SET_POINTS];
            for (uint64_t k = 0; k < t; k++) zs[k] = zm[args->set_points[p0 + k]];
            for (uint64_t k = 0; k < t; k++) {
                items[p0 + k] = hsw::OpenItem{args->set_points[p0 + k], 0};
                item_weights[p0 + k] = hsw::fr_mont_mul(vi, hsw::shplonk_lambda(zs, (uint32_t)t, (uint32_t)k));
            }
            sets[i] = hsw::ShplonkSet{(uint32_t)f0, (uint32_t)m, (uint32_t)p0, (uint32_t)t, (uint32_t)rows, 0, nullptr, nullptr};
            vi = hsw::fr_mont_mul(vi, vm);
        }
    }
    // device staging: [the status word][the scan's s[0] per item][columns][set columns][their weights][sets][items]
    // [their weights][points][the tiles' sums][a cell per thread and item][c of every set of two columns or more]
    const size_t cell = sizeof(PFe), c_bytes = align256((size_t)rows * cell);
    hsw::Staging st;
    st.zeroed(sizeof(uint32_t));
    const size_t off_evals = st.zeroed(k_items * cell), off_cols = st.zeroed(k_cols * sizeof(hsw::OpenColumn));
    const size_t off_refs = st.add(refs.data(), k_refs * sizeof(uint32_t)), off_cw = st.add(col_weights.data(), k_refs * cell);
    const size_t off_sets = st.zeroed(k_sets * sizeof(hsw::ShplonkSet)), off_items = st.add(items.data(), k_items * sizeof(hsw::OpenItem));
    const size_t off_iw = st.add(item_weights.data(), k_items * cell), off_points = st.zeroed(k_points * sizeof(hsw::OpenPoint));
    const size_t off_tiles = st.work(k_items * (size_t)geo.n_tiles * cell), off_seeds = st.work(k_items * (size_t)geo.seeds * cell);
    size_t off_c = st.work(0);
    for (size_t i = 0; i < k_sets; i++)
        if (sets[i].m > 1) st.work(c_bytes);
    const size_t total = st.bytes;
    for (size_t b = 0; b < k_cols; b++) {
        hsw::OpenColumn &oc = st.image<hsw::OpenColumn>(off_cols)[b];
        oc.cells = static_cast<const uint4 *>(b < n ? args->d_columns[b] : args->d_h);
        oc.rows = (uint32_t)(b < n && args->input_rows ? args->input_rows[b] : rows);
    }
    for (size_t t = 0; t < k_points; t++) hsw::open_stage_point(open ? um : zm[t], geo, st.image<hsw::OpenPoint>(off_points)[t]);
    EngineScope es(e);
    if (!es.ok) return hsw_engine_fail(e, HSW_ERR_NO_DEVICE, "hipSetDevice failed");
    const int grc = g->scratch.reserve(total);
    if (grc != HSW_OK) return hsw_engine_fail(e, grc, "the scratch of the SHPLONK opening does not fit the device");
    void *d = g->scratch.d;
    for (size_t i = 0; i < k_sets; i++) {
        if (sets[i].m > 1) {
            sets[i].c = hsw::at<uint4>(d, off_c);
            sets[i].src = sets[i].c;
            off_c += c_bytes;
        } else {                                                 // one column: it is its own c
            const uint32_t b = refs[sets[i].first];
            sets[i].src = static_cast<const uint4 *>(args->d_columns[b]);
            sets[i].src_rows = (uint32_t)(args->input_rows ? args->input_rows[b] : rows);
        }
    }
    std::memcpy(st.image<hsw::ShplonkSet>(off_sets), sets.data(), k_sets * sizeof(hsw::ShplonkSet));
    hsw::ShplonkParams p{};
    p.geo = geo;
    p.cols = hsw::at<const hsw::OpenColumn>(d, off_cols);
    p.set_cols = hsw::at<const uint32_t>(d, off_refs);
    p.col_weights = hsw::at<const PFe>(d, off_cw);
    p.sets = hsw::at<const hsw::ShplonkSet>(d, off_sets);
    p.items = hsw::at<const hsw::OpenItem>(d, off_items);
    p.item_weights = hsw::at<const PFe>(d, off_iw);
    p.points = hsw::at<const hsw::OpenPoint>(d, off_points);
    p.tiles = hsw::at<uint4>(d, off_tiles);
    p.seeds = hsw::at<uint4>(d, off_seeds);
    p.out = static_cast<uint4 *>(args->d_out);
    p.status = hsw::at<uint32_t>(d, 0);
    p.n_sets = (uint32_t)k_sets;
    p.unit = open ? 1u : 0u;
    hsw::OpenParams sp{};                                      // the scan of hsw_open.hip over the items
    sp.geo = geo;
    sp.items = p.items;
    sp.points = p.points;
    sp.tiles = p.tiles;
    sp.evals = hsw::at<uint4>(d, off_evals);
    sp.status = p.status;
    const hipStream_t stream = es.stream;
    hsw::Events ev;
    hipError_t he = hsw::upload(st, d, stream, ev);
    if (he == hipSuccess) he = hsw::launch_shplonk_tiles(p, stream);
    if (he == hipSuccess) he = hsw::launch_open_scan(sp, (uint32_t)k_items, stream);
    if (he == hipSuccess) he = hsw::launch_shplonk_write(p, stream);
    if (he == hipSuccess) he = ev.record(stream);
    uint32_t status = 0;
    std::vector<float> ms;
    const int frc = hsw::finish(e, he, stream, ev, d, &status, sizeof status, ms);
    if (frc != HSW_OK) return frc;
    status &= hsw::SHPLONK_CELL_NOT_BELOW_P;
    report->sets = n_sets;
    report->items = n_set_points;
    report->columns = k_refs;
    report->refused = status ? 1 : 0;
    report->written = status ? 0 : rows;
    report->scratch_bytes = total;
    report->tile_rows = geo.tile_rows;
    report->tiles = geo.n_tiles;
    report->thread_rows = hsw::OPEN_ROWS;
    report->launches = 3;
    report->kernel_ms = ms[0];
    if (args->status) *args->status = status;
    return HSW_OK;
}

}  // namespace

extern "C" int hsw_gadget_shplonk_quotient(hsw_gadget *g, const hsw_shplonk *args, hsw_shplonk_report *report) try {
    return shplonk_call(g, args, report, false);
} HSW_NO_UNWIND

extern "C" int hsw_gadget_shplonk_open(hsw_gadget *g, const hsw_shplonk *args, hsw_shplonk_report *report) try {
    return shplonk_call(g, args, report, true);
} HSW_NO_UNWIND
