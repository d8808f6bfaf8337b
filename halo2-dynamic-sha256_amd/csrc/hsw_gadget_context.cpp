// hsw_gadget_context.cpp -- the Context of hsw_gadget.hpp: its buffers, its layouts, bind and unbind, the device jump
// table; and Sha256DynamicConfig::configure / load / new_context.
#include "hsw_gadget_launch.hpp"

#include <algorithm>
#include <memory>
#include <new>

namespace hsw {

namespace {

// A zeroed device buffer of `bytes` (at least one cell; unassigned advice cells are 0) whose first `keep` bytes are
// those of `old`.  `old` itself is left alone: a caller can get several buffers and commit only when it has them all.
hipError_t fresh_zeroed(void **out, size_t bytes, const void *old = nullptr, size_t keep = 0) {
    if (!bytes) bytes = HSW_CELL_BYTES;
    void *p = nullptr;
    hipError_t he = hipMalloc(&p, bytes);
    if (he == hipSuccess) he = hipMemset(p, 0, bytes);
    if (he == hipSuccess && old && keep) he = hipMemcpy(p, old, keep, hipMemcpyDeviceToDevice);
    if (he != hipSuccess) { (void)hipFree(p); p = nullptr; }
    *out = p;
    return he;
}

}  // namespace

int Sha256DynamicConfig::configure(const std::vector<size_t> &sizes, uint32_t num_bits_lookup,
                                   uint32_t num_advice_columns, bool is_input_range_check,
                                   Sha256DynamicConfig *out) {
    if (!out) return HSW_ERR_INVALID_ARG;
    for (size_t b : sizes)
        if (b % 64 != 0) return HSW_ERR_SHAPE;                                // lib.rs:57-59
    hsw_shape s;
    const int rc = hsw_shape_query(num_bits_lookup, num_advice_columns, &s);  // SpreadConfig::configure, spread.rs:37
    if (rc != HSW_OK) return rc;
    out->max_variable_byte_sizes = sizes;
    out->cur_hash_idx = 0;                                                    // lib.rs:66
    out->num_bits_lookup = num_bits_lookup;
    out->num_advice_columns = num_advice_columns;
    out->is_input_range_check = is_input_range_check;
    return HSW_OK;
}

std::vector<std::pair<uint64_t, uint64_t>> Sha256DynamicConfig::load() const {
    std::vector<std::pair<uint64_t, uint64_t>> rows;                          // spread.rs:169-189
    for (uint64_t idx = 0; idx < (1ull << num_bits_lookup); idx++) {
        uint64_t sp = 0;
        for (int b = 0; b < 32; b++) sp |= ((idx >> b) & 1ull) << (2 * b);
        rows.emplace_back(idx, sp);
    }
    return rows;
}

Context::~Context() {
    if (!bound) { (void)hipFree(d_gate); (void)hipFree(d_chip_dense); (void)hipFree(d_chip_spread); (void)hipFree(d_lookup); }
    (void)hipFree(d_next_states); (void)hipFree(d_blocks); (void)hipFree(d_pre_states);
    (void)hipFree(d_init_states); (void)hipFree(d_offsets); (void)hipFree(d_place); (void)hipFree(d_ingest);
    if (hp_blocks) (void)hipHostFree(hp_blocks);
    free_compact_staging();
}

void Context::free_compact_staging() {
    (void)hipFree(d_c_gate); (void)hipFree(d_c_lookup); (void)hipFree(d_c_dense); (void)hipFree(d_c_spread);
    (void)hipFree(d_wide); (void)hipFree(d_wide_count);
    if (hp_wide_count) (void)hipHostFree(hp_wide_count);
    d_c_gate = d_c_lookup = d_c_dense = d_c_spread = d_wide = nullptr;
    d_wide_count = hp_wide_count = nullptr;
    wide_cap = 0;
}

int Sha256DynamicConfig::new_context(hsw_engine *engine, Context **out, bool whole_digest, bool independent,
                                     bool context_images, bool shared, size_t group_m) const {
    if (!engine || !out) return HSW_ERR_INVALID_ARG;
    *out = nullptr;
    hsw_shape s;
    int rc = hsw_engine_shape(engine, &s);
    if (rc != HSW_OK) return rc;
    if (s.num_bits_lookup != num_bits_lookup || s.num_advice_columns != num_advice_columns)
        return HSW_ERR_SHAPE;
    EngineScope es(engine);                                   // the context's buffers live on the engine's GPU
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    std::unique_ptr<Context> c(new (std::nothrow) Context());
    if (!c) return HSW_ERR_NOMEM;
    c->engine = engine;
    c->shape = s;
    size_t total = 0;
    for (size_t b : max_variable_byte_sizes) total += b / 64;
    c->capacity_blocks = total;
    c->init_capacity = max_variable_byte_sizes.size();
    const size_t nb = total ? total : 1, nh = c->init_capacity ? c->init_capacity : 1;
    if (whole_digest) {
        if (s.mode != HSW_MODE_HALO2_INTERNALS) return HSW_ERR_INVALID_ARG;
        c->whole = true;
        c->independent = independent;
        c->context_images = context_images;
        c->shared = shared;
        if (shared) c->declared.resize(group_m ? group_m : max_variable_byte_sizes.size());
        c->group_m = group_m;
        // the Context's zero cell: one, or one per digest when every digest is a Context of its own
        uint64_t cells = independent ? max_variable_byte_sizes.size() : 1, lookups = 0;
        for (size_t b : max_variable_byte_sizes) {
            if (independent && ((b / 64) * (uint64_t)s.limb_calls_per_block) % s.num_advice_columns != 0)
                return HSW_ERR_UNSUPPORTED;                   // a context's chip rows must start on a row of their own
            hsw_frame_shape fs;
            rc = hsw_frame_query(&s, b, is_input_range_check ? 1 : 0, &fs);
            if (rc == HSW_OK && fs.n_blocks == 0) rc = HSW_ERR_UNSUPPORTED;
            if (rc != HSW_OK) return rc;
            cells += fs.digest_cells;
            lookups += fs.digest_lookups;
            c->ctx_digest_cells = fs.digest_cells;            // (context images: every digest has this shape)
            c->ctx_own_lookups = fs.digest_lookups;
        }
        if (group_m) {                                        // K Contexts alike: a zero cell each, one Context's sums
            const uint64_t K = max_variable_byte_sizes.size() / group_m;
            c->ctx_digest_cells = (cells - 1) / K;
            c->ctx_own_lookups = lookups / K;
            c->ctx_blocks = total / (size_t)K;
            cells += K - 1;
            if (((uint64_t)c->ctx_blocks * s.limb_calls_per_block) % s.num_advice_columns != 0)
                return HSW_ERR_UNSUPPORTED;                   // a Context's chip rows must start on a row of their own
        }
        c->gate_capacity = cells;
        c->lookup_capacity = c->own_lookup_capacity = lookups;
    }
    const OwnedCells own = c->owned(c->layout);
    c->chip_col_stride = own.chip_stride;
    const size_t gate_bytes = own.image * HSW_CELL_BYTES, col_bytes = own.chip * HSW_CELL_BYTES;
    hipError_t he = hipMalloc(&c->d_gate, gate_bytes);
    // touch the stream buffers once: the first write into fresh device memory is several times slower
    // (measured: 16-block digests 266 us instead of 54 us while a context's buffer was still untouched)
    if (he == hipSuccess) he = hipMemset(c->d_gate, 0, gate_bytes);
    if (he == hipSuccess && whole_digest) {
        const size_t lbytes = (own.lookup ? own.lookup : 1) * HSW_CELL_BYTES;
        he = hipMalloc(&c->d_lookup, lbytes);
        if (he == hipSuccess) he = hipMemset(c->d_lookup, 0, lbytes);
    }
    if (he == hipSuccess) he = hipMalloc(&c->d_chip_dense, col_bytes);
    if (he == hipSuccess) he = hipMalloc(&c->d_chip_spread, col_bytes);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_next_states, nb * 32);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_blocks, nb * 64);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_pre_states, nb * 32);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_init_states, nh * 32);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_offsets, (nh + 1) * sizeof(uint32_t));
    if (he == hipSuccess) {
        void *pin = nullptr, *dpin = nullptr;
        he = hipHostMalloc(&pin, nb * 128, hipHostMallocMapped);
        if (he == hipSuccess) {
            c->hp_blocks = static_cast<uint8_t *>(pin);
            he = hipHostGetDevicePointer(&dpin, pin, 0);
        }
        if (he == hipSuccess) {
            c->hp_pre = reinterpret_cast<uint32_t *>(c->hp_blocks + nb * 64);
            c->hp_next = reinterpret_cast<uint32_t *>(c->hp_blocks + nb * 96);
            c->dp_blocks = static_cast<uint8_t *>(dpin);
            c->dp_pre = reinterpret_cast<uint32_t *>(c->dp_blocks + nb * 64);
            c->dp_next = reinterpret_cast<uint32_t *>(c->dp_blocks + nb * 96);
        }
    }
    if (he == hipSuccess) he = hipMemset(c->d_chip_dense, 0, col_bytes);
    if (he == hipSuccess) he = hipMemset(c->d_chip_spread, 0, col_bytes);
    if (he != hipSuccess) return hip_status(he);
    *out = c.release();
    return HSW_OK;
}

// What a library-owned gadget with layout l holds, in cells: new_context allocates it, adopt and unbind size the
// buffers they replace by it
OwnedCells Context::owned(const Layout &l) const {
    const size_t K = contexts(), ncols = shape.num_advice_columns;
    OwnedCells o;
    // K images; without one the whole-digest stream, or the block streams
    o.image = l.max_rows ? K * (size_t)l.image_cells() : whole ? (size_t)gate_capacity
                                                               : (capacity_blocks ? capacity_blocks : 1) * (size_t)shape.gate_cells_per_block;
    // the lookup-advice stream is indexed from the Context's first queued cell: [0, origin_lookups) are the caller's;
    // a shared context's holds the interludes' entries too -- a group's K columns of them
    if (shared && l.max_rows) o.lookup = group_m ? K * (size_t)l.lookups_end : (size_t)std::max(l.lookups_end, own_lookup_capacity);
    else o.lookup = (size_t)own_lookup_capacity + K * (size_t)l.origin_lookups;
    o.chip_stride = (size_t)hsw_chip_rows(&shape, 0, capacity_blocks);
    o.chip = ncols * (o.chip_stride ? o.chip_stride : 1);
    return o;
}

int Context::plan_layout(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t rows, const std::vector<DigestOrigin> &decl,
                         Layout *out) const {
    if (!rows) return HSW_OK;                             // no image: the stream as it is, from the origin
    // context images: ONE Context's walk (every Context is laid out alike), K images of it
    // (a Context group: ONE Context's group_m digests, with the declarations)
    const size_t n = context_images && !sizes.empty() ? 1 : group_m ? group_m : sizes.size();
    const int rc = layout_walk(shape, sizes.data(), n, rc_inputs, rows, shared ? &decl : nullptr, out);
    if (rc != HSW_OK) return rc;
    if (group_m) out->period = ctx_digest_cells + (out->origin_zero_loaded ? 0u : 1u);
    if (shared) return out->columns > HSW_GADGET_MAX_COLUMNS ? HSW_ERR_TOO_LARGE : HSW_OK;
    out->digest_cell0.clear(); out->digest_entry0.clear(); out->digest_lookup0.clear();   // (one lookup run, no table)
    if (context_images) out->period = ctx_digest_cells + (out->origin_zero_loaded ? 0u : 1u);
    return out->break_cell.size() > HSW_MAX_BREAKS ? HSW_ERR_TOO_LARGE : HSW_OK;
}

int Context::adopt(Layout &nl, bool fresh_image, bool fresh_lookup, uint64_t clear_from) {
    const size_t K = contexts(), none = ~(size_t)0;
    const bool table = (shared || by_pointer) && nl.max_rows, changed = !nl.same_map(layout);
    if (bound) {                                          // the caller's memory: it fits what was declared, or it does not
        if (nl.columns > binding.columns_capacity || lookups_needed(nl) > binding.lookup_capacity) return HSW_ERR_TOO_LARGE;
        layout = std::move(nl);
        lookup_capacity = (uint64_t)(K - 1) * lookup_pitch() + binding.lookup_capacity;
        place_dirty = place_dirty || changed || lookup_by_table();      // (the table's lookup rows count from Lp, the layout's)
        return HSW_OK;
    }
    const OwnedCells own = owned(nl);
    size_t img_cells = none, img_keep = 0, lk_cells = none, lk_keep = 0;
    if (table && group_m) {
        // a Context group: K images and K lookup columns whose places follow from one Context's size -- a layout
        // that differs gets fresh, zeroed ones (the same layout again, pass after pass, keeps them)
        if (fresh_image || changed || nl.max_rows != layout.max_rows) img_cells = own.image;
        if (fresh_lookup || nl.lookups_end != layout.lookups_end || own.lookup != lookup_capacity) lk_cells = own.lookup;
        fresh_lookup = false;
    } else if (table) {                                   // the image grows: the columns so far are copied over
        const uint64_t have = nl.max_rows == layout.max_rows ? image_columns : 0;   // (another column height: a fresh image)
        if (nl.columns > have) { img_cells = own.image; img_keep = (size_t)(have * nl.max_rows); }
    } else if (fresh_image) {
        img_cells = own.image;
    }
    // the lookup-advice stream is indexed from the Context's first queued cell: [0, origin_lookups) are the caller's
    if (fresh_lookup) lk_cells = own.lookup;
    else if (table && !group_m && nl.lookups_end > lookup_capacity) { lk_cells = own.lookup; lk_keep = (size_t)lookup_capacity; }   // the interludes' entries
    const bool clear = table && changed && !group_m;
    if (img_cells != none || lk_cells != none || clear) {
        EngineScope es(engine);
        if (!es.ok) return HSW_ERR_NO_DEVICE;
        // (the callers run on a drained engine: nothing still writes the buffers replaced here)
        void *img = nullptr, *lk = nullptr;
        hipError_t he = hipSuccess;
        if (img_cells != none) he = fresh_zeroed(&img, img_cells * HSW_CELL_BYTES, d_gate, img_keep * HSW_CELL_BYTES);
        if (he == hipSuccess && lk_cells != none) he = fresh_zeroed(&lk, lk_cells * HSW_CELL_BYTES, d_lookup, lk_keep * HSW_CELL_BYTES);
        if (he != hipSuccess) { (void)hipFree(img); return hip_status(he); }
        if (img) { (void)hipFree(d_gate); d_gate = img; image_columns = nl.columns; }
        if (lk) { (void)hipFree(d_lookup); d_lookup = lk; lookup_capacity = lk_cells; }
        if (img || lk) free_compact_staging();            // sized for the old geometry
        const uint64_t end = image_columns * nl.max_rows;
        if (clear && clear_from < end)                    // cells an earlier layout wrote past the unchanged part
            (void)hipMemset(static_cast<uint8_t *>(d_gate) + (size_t)clear_from * HSW_CELL_BYTES, 0, (size_t)(end - clear_from) * HSW_CELL_BYTES);
    }
    layout = std::move(nl);
    place_dirty = place_dirty || changed;
    return HSW_OK;
}

int Context::set_columns(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t rows) {
    if (!whole || blocks_done != 0 || gate_cursor != 0) return HSW_ERR_INVALID_ARG;
    if (independent && !context_images) return HSW_ERR_UNSUPPORTED;   // K regions in one stream: linear only
    const uint64_t G = shape.gate_cells_per_block;
    if (rows < G + 16) return HSW_ERR_INVALID_ARG;        // keeps a block inside <= 2 columns (kernel: <= 2 breaks per block)
    if (layout.origin_row >= rows) return HSW_ERR_INVALID_ARG;   // the Context's next free row lies inside its column
    if (bound && rows > layout.pitch) return HSW_ERR_TOO_LARGE;  // a bound column holds column_pitch cells at most
    Layout nl = layout.origin();
    // (shared context -- a new layout: the declarations made for the old one are dropped)
    const std::vector<DigestOrigin> none(declared.size());
    int rc = plan_layout(sizes, rc_inputs, rows, none, &nl);
    if (rc == HSW_OK) rc = adopt(nl, true, false, 0);
    if (rc == HSW_OK) declared = none;
    return rc;
}

PlaceWords Context::place_words() const {
    PlaceWords w;
    const size_t K = by_pointer ? contexts() : 1, ncols = shape.num_advice_columns;
    w.n = layout.break_cell.size() + (by_pointer ? 1 : 0);
    w.cum = w.n;
    w.shifts = w.cum + K * w.n;
    w.n_shifts = shared ? layout.digest_lookup0.size() : by_pointer ? init_capacity : 0;
    w.lk_rows = w.shifts + (w.n_shifts ? w.n_shifts : 1);
    w.chip_rows = w.lk_rows + (lookup_by_table() ? K : 0);
    w.total = w.chip_rows + (chips_by_table() ? K * ncols * 2 : 0);
    return w;
}

int Context::upload_place() {
    if (!place_dirty && d_place) return HSW_OK;
    const Layout &l = layout;
    const PlaceWords w = place_words();
    const size_t nb = l.break_cell.size(), K = contexts(), ncols = shape.num_advice_columns;
    std::vector<uint64_t> h(w.total, 0);
    for (size_t k = 0; k < nb; k++) h[w.n - nb + k] = l.break_cell[k];      // (by pointer: after jump 0 at stream cell 0)
    if (by_pointer) {
        // A jump into image column k of Context c lands break_cum (columns one pitch apart) + what column k really
        // lies from there: col_off - k * pitch, modulo 2^64 (PlaceTable::cum_stride)
        std::vector<uint64_t> col(w.n, 0);
        for (size_t k = 0; k < nb; k++) {
            uint64_t c = 0;
            l.position(l.break_cell[k], &c, nullptr);
            col[1 + k] = c - l.origin_column;
        }
        for (size_t c = 0; c < K; c++)
            for (size_t k = 0; k < w.n; k++)
                h[w.cum + c * w.n + k] = (k ? l.break_cum[k - 1] : 0) + column_cell(c, col[k]) - col[k] * l.column_pitch();
    } else {
        for (size_t k = 0; k < nb; k++) h[w.cum + k] = l.break_cum[k];
    }
    for (size_t d = 0; d < w.n_shifts && shared; d++) h[w.shifts + d] = l.digest_lookup0[d] - l.origin_lookups - l.digest_entry0[d];
    for (size_t c = 0; c < K && lookup_by_table(); c++) h[w.lk_rows + c] = lookup_extra(c);      // PlaceTable::lk_row
    for (size_t c = 0; c < K && chips_by_table(); c++)                                          // PlaceTable::chip_row
        for (size_t k = 0; k < ncols; k++) {
            h[w.chip_rows + (c * ncols + k) * 2] = chip_column_cell(c, k, false) - c * ctx_chip_rows();
            h[w.chip_rows + (c * ncols + k) * 2 + 1] = chip_column_cell(c, k, true) - c * ctx_chip_rows();
        }
    if (d_place && h == place_host) { place_dirty = false; return HSW_OK; }   // the device already holds this table
    EngineScope es(engine);
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    hipError_t he = hipSuccess;
    if (h.size() > place_cap) {
        void *p = nullptr;
        he = hipMalloc(&p, h.size() * sizeof(uint64_t));
        if (he != hipSuccess) return hip_status(he);
        (void)hipFree(d_place);
        d_place = p;
        place_cap = h.size();
    }
    he = hipMemcpy(d_place, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) return HSW_ERR_HIP;
    place_host.swap(h);
    place_dirty = false;
    return HSW_OK;
}

hsw_frame_desc Context::frame_desc(const AssignedHashResult &r, size_t d, bool rc_inputs) const {
    // (lookup columns by pointer table: the frame kernels address through the Context's offset, positions stay)
    const uint64_t lx = lookup_extra(context_of(d));
    hsw_frame_desc f{};
    f.input_len = r.input_len;
    f.first_block = r.first_block;
    f.prologue_cell = r.prologue_cell; f.epilogue_cell = r.epilogue_cell;
    f.prologue_lookup = r.prologue_lookup + lx; f.epilogue_lookup = r.epilogue_lookup + lx;
    f.zero_cell = r.zero_cell;
    f.n_blocks = (uint32_t)r.n_blocks;
    f.num_round = (uint32_t)r.num_round;
    f.precomputed_round = (uint32_t)r.precomputed_round;
    f.is_input_range_check = rc_inputs ? 1u : 0u;
    return f;
}

int Context::set_origin(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t column, uint64_t row, bool zero_cell_loaded,
                        uint64_t lookups_queued) {
    if (!whole || blocks_done != 0 || gate_cursor != 0 || lookup_cursor != layout.origin_lookups) return HSW_ERR_INVALID_ARG;
    if (independent && !context_images) return HSW_ERR_UNSUPPORTED;
    if (layout.max_rows && row >= layout.max_rows) return HSW_ERR_INVALID_ARG;
    // the new layout, checked in full: nothing is touched if it cannot be had.  The column breaks follow from where
    // the stream starts: a new row, or a zero cell that comes or goes, lays the image out again (a fresh image); a
    // shared context drops its declarations and has every cell of an earlier layout zeroed
    Layout nl = layout.origin();                          // (in the same memory: a bound region's pitches stay)
    nl.origin_column = column; nl.origin_row = row; nl.origin_lookups = lookups_queued; nl.origin_zero_loaded = zero_cell_loaded;
    const std::vector<DigestOrigin> none(declared.size());
    const int rc = plan_layout(sizes, rc_inputs, layout.max_rows, none, &nl);
    if (rc != HSW_OK) return rc;
    const bool fresh_image = layout.max_rows && (row != layout.origin_row || zero_cell_loaded != layout.origin_zero_loaded);
    const int rc2 = adopt(nl, fresh_image, lookups_queued != layout.origin_lookups, 0);
    if (rc2 != HSW_OK) return rc2;
    declared = none;
    lookup_cursor = lookups_queued;
    zero_loaded = zero_cell_loaded;                       // (without the zero cell the stream is one cell shorter)
    return HSW_OK;
}

int Context::bind(const std::vector<size_t> &sizes, bool rc_inputs, const hsw_region_binding &b_in, const hsw_column_tables *t) {
    const uint64_t K = contexts();
    const size_t ncols = shape.num_advice_columns;
    hsw_region_binding b = b_in;
    void *const *col_ptrs = t ? t->d_column_ptrs : nullptr;
    const size_t n_ptrs = t ? t->n_column_ptrs : 0;
    const bool lk_tab = t && t->d_lookup_ptrs, chip_tab = t && (t->d_chip_dense_ptrs || t->d_chip_spread_ptrs);
    auto entries_ok = [](void *const *p, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (!p[i] || ((uintptr_t)p[i] & 127u)) return false;
        return true;
    };
    if (t && !col_ptrs) return HSW_ERR_INVALID_ARG;       // (without an image table: hsw_gadget_bind_region)
    if (col_ptrs) {                                       // columns by pointer table: one pointer per column per proof
        if (b.columns_capacity == 0 || b.columns_capacity > ~(size_t)0 / (size_t)K || n_ptrs != (size_t)K * (size_t)b.columns_capacity) return HSW_ERR_INVALID_ARG;
        if (!entries_ok(col_ptrs, n_ptrs)) return HSW_ERR_INVALID_ARG;
        b.d_columns = col_ptrs[0];
        b.context_pitch = 0;
    }
    if (t && t->n_lookup_ptrs != (lk_tab ? (size_t)K : 0)) return HSW_ERR_INVALID_ARG;
    if (lk_tab) {                                         // ... and one per lookup-advice column
        if (!entries_ok(t->d_lookup_ptrs, (size_t)K)) return HSW_ERR_INVALID_ARG;
        b.d_lookup = t->d_lookup_ptrs[0];
        b.lookup_pitch = 0;
    }
    if (chip_tab && (!t->d_chip_dense_ptrs || !t->d_chip_spread_ptrs)) return HSW_ERR_INVALID_ARG;   // both families or neither
    if (t && t->n_chip_ptrs != (chip_tab ? (size_t)K * ncols : 0)) return HSW_ERR_INVALID_ARG;
    if (chip_tab) {                                       // ... and two per chip column
        if (!entries_ok(t->d_chip_dense_ptrs, (size_t)K * ncols) || !entries_ok(t->d_chip_spread_ptrs, (size_t)K * ncols)) return HSW_ERR_INVALID_ARG;
        b.d_chip_dense = t->d_chip_dense_ptrs[0]; b.d_chip_spread = t->d_chip_spread_ptrs[0];
        b.chip_col_stride = b.chip_context_pitch = 0;
    }
    const void *ptrs[4] = {b.d_columns, b.d_lookup, b.d_chip_dense, b.d_chip_spread};
    // (128 bytes: a column that starts on a line boundary keeps the realigned write-out on whole lines)
    for (const void *p : ptrs)
        if (!p || ((uintptr_t)p & 127u)) return HSW_ERR_INVALID_ARG;
    // (a block's cells are addressed by 32-bit byte offsets from its first, the gaps of <= 2 column breaks included)
    if (b.column_pitch < layout.max_rows || b.column_pitch > (1ull << 24)) return HSW_ERR_INVALID_ARG;
    if (!chip_tab && b.chip_col_stride < b.chip_rows_capacity) return HSW_ERR_INVALID_ARG;
    if (K > 1) {
        if (!col_ptrs && (b.columns_capacity > ~0ull / b.column_pitch || b.context_pitch < b.columns_capacity * b.column_pitch)) return HSW_ERR_INVALID_ARG;
        if (!lk_tab && b.lookup_pitch < b.lookup_capacity) return HSW_ERR_INVALID_ARG;
        if (b.context_pitch > ~0ull / (K * HSW_CELL_BYTES) || b.lookup_pitch > ~0ull / (K * HSW_CELL_BYTES) ||
            b.chip_context_pitch > ~0ull / (K * HSW_CELL_BYTES))
            return HSW_ERR_INVALID_ARG;
    }
    Layout nl = layout.origin();
    nl.pitch = b.column_pitch;
    nl.image_pitch = K > 1 ? b.context_pitch : 0;
    const int rc = plan_layout(sizes, rc_inputs, layout.max_rows, declared, &nl);
    if (rc != HSW_OK) return rc;
    // (cells from entry 0, modulo 2^64: an entry below entry 0 wraps, and wraps back when the kernels scale by the cell size)
    auto offsets = [](void *const *p, size_t n) {
        std::vector<uint64_t> o(n);
        for (size_t i = 0; i < n; i++) o[i] = (uint64_t)((uintptr_t)p[i] - (uintptr_t)p[0]) / HSW_CELL_BYTES;
        return o;
    };
    std::vector<uint64_t> off, lko, cdo, cso;
    if (col_ptrs) off = offsets(col_ptrs, n_ptrs);
    if (lk_tab) lko = offsets(t->d_lookup_ptrs, (size_t)K);
    if (chip_tab) { cdo = offsets(t->d_chip_dense_ptrs, (size_t)K * ncols); cso = offsets(t->d_chip_spread_ptrs, (size_t)K * ncols); }
    if (nl.columns > b.columns_capacity || lookups_needed(nl) > b.lookup_capacity || ctx_chip_rows() > b.chip_rows_capacity) return HSW_ERR_TOO_LARGE;
    // (the caller ran on a drained engine: nothing still writes the buffers given up here)
    if (!bound) {
        EngineScope es(engine);
        if (!es.ok) return HSW_ERR_NO_DEVICE;
        (void)hipFree(d_gate); (void)hipFree(d_lookup); (void)hipFree(d_chip_dense); (void)hipFree(d_chip_spread);
    }
    free_compact_staging();
    bound = true;
    binding = b;
    by_pointer = col_ptrs != nullptr;
    col_off.swap(off);
    lk_off.swap(lko); chip_dense_off.swap(cdo); chip_spread_off.swap(cso);
    d_gate = b.d_columns; d_lookup = b.d_lookup; d_chip_dense = b.d_chip_dense; d_chip_spread = b.d_chip_spread;
    chip_col_stride = (size_t)b.chip_col_stride;
    image_columns = b.columns_capacity;
    layout = std::move(nl);
    lookup_capacity = (K - 1) * lookup_pitch() + b.lookup_capacity;
    place_dirty = true;
    return HSW_OK;
}

int Context::unbind(const std::vector<size_t> &sizes, bool rc_inputs) {
    if (!bound) return HSW_OK;
    Layout nl = layout.origin();
    nl.pitch = nl.image_pitch = 0;
    const int rc = plan_layout(sizes, rc_inputs, layout.max_rows, declared, &nl);
    if (rc != HSW_OK) return rc;
    EngineScope es(engine);
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    const OwnedCells own = owned(nl);                     // what a fresh gadget with this layout owns
    void *img = nullptr, *lk = nullptr, *cd = nullptr, *cs = nullptr;
    hipError_t he = fresh_zeroed(&img, own.image * HSW_CELL_BYTES);
    if (he == hipSuccess) he = fresh_zeroed(&lk, own.lookup * HSW_CELL_BYTES);
    if (he == hipSuccess) he = fresh_zeroed(&cd, own.chip * HSW_CELL_BYTES);
    if (he == hipSuccess) he = fresh_zeroed(&cs, own.chip * HSW_CELL_BYTES);
    if (he != hipSuccess) { (void)hipFree(img); (void)hipFree(lk); (void)hipFree(cd); (void)hipFree(cs); return hip_status(he); }
    bound = false;
    by_pointer = false;
    col_off.clear();
    lk_off.clear(); chip_dense_off.clear(); chip_spread_off.clear();
    binding = hsw_region_binding{};
    d_gate = img; d_lookup = lk; d_chip_dense = cd; d_chip_spread = cs;
    chip_col_stride = own.chip_stride;
    image_columns = nl.columns;
    lookup_capacity = own.lookup;
    layout = std::move(nl);
    place_dirty = true;
    return HSW_OK;
}

}  // namespace hsw
