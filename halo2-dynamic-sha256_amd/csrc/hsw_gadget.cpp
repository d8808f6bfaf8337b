// hsw_gadget.cpp -- the C ABI of the gadget front-end (include/hsw.h) over Sha256DynamicConfig and Context
// (hsw_gadget.hpp; hsw_gadget_sha.cpp, hsw_gadget_context.cpp, hsw_gadget_digest.cpp).
#include "hsw_gadget_launch.hpp"

#include <chrono>
#include <cstring>
#include <new>

#include "hsw_nounwind.hpp"
#include "hsw_frame.hpp"

extern "C" {

int hsw_digest_prepare(const uint8_t *input, size_t input_len, size_t precomputed_input_len,
                       size_t max_variable_byte_size, uint8_t *blocks_out, uint32_t init_state_out[8],
                       hsw_digest_info *info) try {
    hsw::DigestPlan plan;
    const int rc = hsw::digest_prepare(input, input_len, precomputed_input_len, max_variable_byte_size, &plan);
    if (rc != HSW_OK) return rc;
    if (blocks_out && !plan.blocks.empty()) std::memcpy(blocks_out, plan.blocks.data(), plan.blocks.size());
    if (init_state_out) std::memcpy(init_state_out, plan.init_state, 32);
    if (info) {
        info->num_round = plan.num_round;
        info->precomputed_round = plan.precomputed_round;
        info->target_round = plan.target_round;
        info->n_blocks = plan.max_variable_round;
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_create(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t n_hashes,
                      int is_input_range_check, hsw_gadget **out) try {
    return hsw_gadget_create_ex(e, max_variable_byte_sizes, n_hashes, is_input_range_check, 0, out);
} HSW_NO_UNWIND

int hsw_gadget_create_ex(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t n_hashes,
                         int is_input_range_check, uint32_t flags, hsw_gadget **out) try {
    if (!e || !out || (!max_variable_byte_sizes && n_hashes)) return HSW_ERR_INVALID_ARG;
    if (flags & ~(HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES | HSW_GADGET_SHARED_CONTEXT))
        return HSW_ERR_INVALID_ARG;
    const bool shared = (flags & HSW_GADGET_SHARED_CONTEXT) != 0;
    if (shared && (!(flags & HSW_GADGET_WHOLE_DIGEST) || (flags & (HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES))))
        return HSW_ERR_INVALID_ARG;
    if ((flags & HSW_GADGET_INDEPENDENT) && !(flags & HSW_GADGET_WHOLE_DIGEST)) return HSW_ERR_INVALID_ARG;
    const bool images = (flags & HSW_GADGET_CONTEXT_IMAGES) != 0;
    if (images && !(flags & HSW_GADGET_INDEPENDENT)) return HSW_ERR_INVALID_ARG;
    *out = nullptr;
    for (size_t i = 1; images && i < n_hashes; i++)        // K proofs of ONE circuit: every Context laid out alike
        if (max_variable_byte_sizes[i] != max_variable_byte_sizes[0]) return HSW_ERR_UNSUPPORTED;
    hsw_shape s;
    int rc = hsw_engine_shape(e, &s);
    if (rc != HSW_OK) return rc;
    if (shared && s.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;   // the table-path kernels: the 8-bit spread table
    hsw_gadget *g = new (std::nothrow) hsw_gadget();
    if (!g) return HSW_ERR_NOMEM;
    std::vector<size_t> sizes(max_variable_byte_sizes, max_variable_byte_sizes + n_hashes);
    rc = hsw::Sha256DynamicConfig::configure(sizes, s.num_bits_lookup, s.num_advice_columns,
                                             is_input_range_check != 0, &g->cfg);
    if (rc == HSW_OK) rc = g->cfg.new_context(e, &g->ctx, (flags & HSW_GADGET_WHOLE_DIGEST) != 0, (flags & HSW_GADGET_INDEPENDENT) != 0,
                                              images, shared);
    if (rc != HSW_OK) { delete g; return rc; }
    *out = g;
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_create_contexts(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t digests_per_context,
                               size_t n_contexts, int is_input_range_check, uint32_t flags, hsw_gadget **out) try {
    if (!e || !out || !max_variable_byte_sizes || digests_per_context == 0 || n_contexts == 0) return HSW_ERR_INVALID_ARG;
    // (HSW_GADGET_SHARED_CONTEXT may be named: every Context of a group is one; the K-proof flags of create_ex are not this)
    if (!(flags & HSW_GADGET_WHOLE_DIGEST) || (flags & ~(HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_SHARED_CONTEXT))) return HSW_ERR_INVALID_ARG;
    *out = nullptr;
    hsw_shape s;
    int rc = hsw_engine_shape(e, &s);
    if (rc != HSW_OK) return rc;
    if (s.mode != HSW_MODE_HALO2_INTERNALS) return HSW_ERR_INVALID_ARG;
    if (s.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;              // the table-path kernels: the 8-bit spread table
    if (n_contexts > (~(size_t)0 >> 8) / digests_per_context) return HSW_ERR_TOO_LARGE;
    hsw_gadget *g = new (std::nothrow) hsw_gadget();
    if (!g) return HSW_ERR_NOMEM;
    std::vector<size_t> sizes;                               // digest d of the pass: digest d % M of Context d / M
    sizes.reserve(digests_per_context * n_contexts);
    for (size_t c = 0; c < n_contexts; c++) sizes.insert(sizes.end(), max_variable_byte_sizes, max_variable_byte_sizes + digests_per_context);
    rc = hsw::Sha256DynamicConfig::configure(sizes, s.num_bits_lookup, s.num_advice_columns, is_input_range_check != 0, &g->cfg);
    if (rc == HSW_OK) rc = g->cfg.new_context(e, &g->ctx, true, false, false, true, digests_per_context);
    if (rc != HSW_OK) { delete g; return rc; }
    *out = g;
    return HSW_OK;
} HSW_NO_UNWIND

void hsw_gadget_destroy(hsw_gadget *g) {
    if (!g) return;
    if (g->scratch.d || g->d_pairs || g->d_lookup_runs || g->ntt_stamp) {   // (every call that used them was synchronous)
        EngineScope es(g->ctx->engine);
        (void)hipFree(g->scratch.d);
        (void)hipFree(g->d_pairs);
        (void)hipFree(g->d_lookup_runs);
        for (hsw_gadget::NttTable &t : g->ntt_tables) (void)hipFree(t.d_table);
    }
    delete g->ctx;
    delete g;
}

// What the three digest entry points do with a committed batch: the ties of a device-fed one (d_inputs; nothing to
// intersect without a destination in this call or earlier in the pass: no bookkeeping), the public results, the gadget's own
static int finish_batch(hsw_gadget *g, int rc, std::vector<hsw::AssignedHashResult> &rs, const void *const *d_inputs,
                        const size_t *input_lens, const size_t *precomputed_input_lens, void *const *d_outputs, hsw_hash_result *results) {
    if (rc != HSW_OK) return rc;
    if (d_inputs && g->ctx->whole && (d_outputs || !g->tie_owners.empty()))
        g->record_ties(g->results.size(), rs.size(), d_inputs, input_lens, precomputed_input_lens, d_outputs);
    for (hsw::AssignedHashResult &r : rs) {
        hsw_hash_result *o = results++;
        o->input_len = r.input_len;
        o->first_block = r.first_block;
        o->n_blocks = r.n_blocks;
        o->spread_cursor0 = r.spread_cursor0;
        o->num_round = r.num_round;
        o->target_round = r.target_round;
        std::memcpy(o->output_bytes, r.output_bytes, 32);
        o->prologue_cell = r.prologue_cell; o->block_cell = r.block_cell;
        o->epilogue_cell = r.epilogue_cell; o->end_cell = r.end_cell;
        o->prologue_lookup = r.prologue_lookup; o->block_lookup = r.block_lookup;
        o->epilogue_lookup = r.epilogue_lookup;
        g->results.push_back(std::move(r));
    }
    return HSW_OK;
}

int hsw_gadget_digest_batch(hsw_gadget *g, size_t n, const uint8_t *const *inputs, const size_t *input_lens,
                            const size_t *precomputed_input_lens, hsw_hash_result *results) try {
    if (!g || !results) return HSW_ERR_INVALID_ARG;
    std::vector<hsw::AssignedHashResult> rs(n);
    return finish_batch(g, g->cfg.digest_batch(*g->ctx, n, inputs, input_lens, precomputed_input_lens, rs.data()), rs, nullptr,
                        input_lens, precomputed_input_lens, nullptr, results);
} HSW_NO_UNWIND

int hsw_gadget_digest_batch_device(hsw_gadget *g, size_t n, const void *const *d_inputs, const size_t *input_lens,
                                   const size_t *precomputed_input_lens, hsw_hash_result *results) try {
    return hsw_gadget_digest_levels_device(g, n, d_inputs, input_lens, precomputed_input_lens, nullptr, nullptr, results);
} HSW_NO_UNWIND

int hsw_gadget_digest_levels_device(hsw_gadget *g, size_t n, const void *const *d_inputs, const size_t *input_lens,
                                    const size_t *precomputed_input_lens, const uint32_t *levels, void *const *d_outputs,
                                    hsw_hash_result *results) try {
    if (!g || !results) return HSW_ERR_INVALID_ARG;
    std::vector<hsw::AssignedHashResult> rs(n);
    return finish_batch(g, g->cfg.digest_levels_device(*g->ctx, n, d_inputs, input_lens, precomputed_input_lens, levels, d_outputs, rs.data()),
                        rs, d_inputs, input_lens, precomputed_input_lens, d_outputs, results);
} HSW_NO_UNWIND

int hsw_gadget_digest(hsw_gadget *g, const uint8_t *input, size_t input_len, size_t precomputed_input_len,
                      hsw_hash_result *result) try {
    return hsw_gadget_digest_batch(g, 1, &input, &input_len, &precomputed_input_len, result);
} HSW_NO_UNWIND

int hsw_gadget_streams(hsw_gadget *g, hsw_gadget_view *view) try {
    if (!g || !view) return HSW_ERR_INVALID_ARG;
    view->d_gate = g->ctx->d_gate;
    view->d_chip_dense = g->ctx->d_chip_dense;
    view->d_chip_spread = g->ctx->d_chip_spread;
    view->d_next_states = g->ctx->d_next_states;
    view->chip_col_stride = g->ctx->chip_col_stride;
    view->blocks_done = g->ctx->blocks_done;
    view->capacity_blocks = g->ctx->capacity_blocks;
    view->num_limb_sum = g->ctx->num_limb_sum;
    view->cur_hash_idx = g->cfg.cur_hash_idx;
    view->gate_cells = g->ctx->gate_cursor;
    view->gate_capacity = g->ctx->gate_capacity;
    view->d_lookup = g->ctx->d_lookup;
    view->lookup_cells = g->ctx->lookup_cursor;
    view->lookup_capacity = g->ctx->lookup_capacity;
    view->max_rows = g->ctx->layout.max_rows;
    view->columns = g->ctx->layout.columns;
    view->origin_column = g->ctx->layout.origin_column;
    view->origin_row = g->ctx->layout.origin_row;
    view->origin_lookups = g->ctx->layout.origin_lookups;
    view->origin_zero_loaded = g->ctx->layout.origin_zero_loaded ? 1u : 0u;
    view->reserved_ = 0;
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_input_bytes(hsw_gadget *g, size_t hash_idx, uint8_t *out, size_t cap, size_t *len) try {
    if (!g || hash_idx >= g->results.size()) return HSW_ERR_INVALID_ARG;
    const std::vector<uint8_t> &b = g->results[hash_idx].input_bytes;
    if (len) *len = b.size();
    if (out) {
        if (cap < b.size()) return HSW_ERR_INVALID_ARG;
        if (!b.empty()) std::memcpy(out, b.data(), b.size());
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_result_cells(const hsw_gadget *g, size_t hash_idx, hsw_result_cells *out) try {
    if (!g || !out || hash_idx >= g->results.size()) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_INVALID_ARG;                  // block-stream contexts hold no frame cells
    const hsw::AssignedHashResult &r = g->results[hash_idx];
    std::memset(out, 0, sizeof *out);
    out->input_len_cell = r.prologue_cell + hsw::frame::P_LEN;
    out->input_bytes_cell0 = r.prologue_cell + hsw::frame::P_BYTES;
    out->n_input_bytes = (uint64_t)r.n_blocks * 64;
    g->ctx->layout.position(out->input_len_cell, &out->input_len_pos[0], &out->input_len_pos[1]);
    g->ctx->layout.position(out->input_bytes_cell0, &out->input_bytes_pos0[0], &out->input_bytes_pos0[1]);
    for (uint32_t w = 0; w < 8; w++)
        for (uint32_t i = 0; i < 4; i++) {
            const uint64_t cell = r.epilogue_cell + (uint64_t)hsw::frame::E_STATE * (r.n_blocks + 1) +
                                  (uint64_t)hsw::frame::E_WORD * w + 5u * i;
            out->output_byte_cells[4 * w + i] = cell;
            g->ctx->layout.position(cell, &out->output_byte_pos[4 * w + i][0], &out->output_byte_pos[4 * w + i][1]);
        }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_set_columns(hsw_gadget *g, uint64_t max_rows, uint64_t *n_columns) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    int rc = hsw_engine_synchronize(g->ctx->engine);          // the image is reallocated: nothing may still write the old one
    if (rc == HSW_OK) rc = g->ctx->set_columns(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, max_rows);
    if (rc == HSW_OK && n_columns) *n_columns = g->ctx->layout.columns;
    if (rc == HSW_OK) hsw::drop_region_tape_positions(g->tape);     // the codes are per stream cell; image positions follow the layout
    return rc;
} HSW_NO_UNWIND

int hsw_gadget_set_origin(hsw_gadget *g, uint64_t column, uint64_t row, int zero_cell_loaded,
                          uint64_t lookups_already_queued) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (!c.whole || g->cfg.cur_hash_idx != 0) return HSW_ERR_INVALID_ARG;   // before the first digest of a synthesis pass
    int rc = hsw_engine_synchronize(c.engine);
    if (rc != HSW_OK) return rc;
    const uint64_t old_row = c.layout.origin_row;
    const bool old_zero = c.layout.origin_zero_loaded;
    rc = c.set_origin(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, column, row, zero_cell_loaded != 0,
                      lookups_already_queued);
    if (rc != HSW_OK) return rc;                                  // (nothing was touched: origin, layout and tape as before)
    // the region tape (hsw_replay.cpp) numbers stream cells: only a zero cell that comes or goes changes it; a new
    // origin row moves the witnesses' image positions; column and queued lookups are offsets applied at delivery.
    // A prover that synthesizes the same circuit pass after pass keeps its tape.
    if (old_zero != (zero_cell_loaded != 0)) { hsw::free_region_tape(g->tape); g->tape = nullptr; }
    else if (old_row != row) hsw::drop_region_tape_positions(g->tape);
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_set_digest_origin(hsw_gadget *g, size_t h, uint64_t column, uint64_t row, uint64_t lookups_queued) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    const size_t n = c.group_m ? c.group_m : g->cfg.max_variable_byte_sizes.size();   // (a group: digest h of every Context alike)
    if (!c.shared || !c.layout.max_rows || h < 1 || h >= n || h < g->cfg.cur_hash_idx || row >= c.layout.max_rows)
        return HSW_ERR_INVALID_ARG;
    const hsw::DigestOrigin &was = c.declared[h];
    // the same declaration again (the next pass declaring what the last one did) changes nothing: the later digests'
    // layout depends on it only, so their declarations stay too
    if (was.set && was.column == column && was.row == row && was.lookups == lookups_queued) return HSW_OK;
    // digest h's declaration replaces the old one and drops the later ones (their layout follows from it)
    std::vector<hsw::DigestOrigin> decl(c.declared.begin(), c.declared.begin() + (ptrdiff_t)h);
    decl.resize(n);
    decl[h].set = true; decl[h].column = column; decl[h].row = row; decl[h].lookups = lookups_queued;
    int rc = hsw_engine_synchronize(c.engine);           // the image may grow: nothing may still write the old one
    if (rc != HSW_OK) return rc;
    // (cells past digest h-1's end: the same in both layouts up to there, stale beyond it if the layout changes)
    const uint64_t clear_from = c.layout.image_cell(c.layout.digest_cell0[h] - 1) + 1;
    hsw::Layout nl = c.layout.origin();
    rc = c.plan_layout(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, c.layout.max_rows, decl, &nl);
    if (rc == HSW_OK) rc = c.adopt(nl, false, false, clear_from);
    if (rc != HSW_OK) return rc;
    c.declared.swap(decl);
    hsw::drop_region_tape_positions(g->tape);           // the witnesses' image positions follow the layout
    return HSW_OK;
} HSW_NO_UNWIND

// What the three bind entry points share once their own arguments are checked.  b = NULL: unbind (t = NULL then);
// t: the pointer tables, whose kernels are the table path's
static int rebind(hsw_gadget *g, const hsw_region_binding *b, const hsw_column_tables *t) {
    hsw::Context &c = *g->ctx;
    // a whole-digest gadget with a column image (K linear regions in one stream, block streams: nothing to bind)
    if (!c.whole || !c.layout.max_rows) return HSW_ERR_UNSUPPORTED;
    if (g->cfg.cur_hash_idx != 0 || c.blocks_done != 0 || c.gate_cursor != 0) return HSW_ERR_INVALID_ARG;   // a fresh or reset gadget
    if (t && c.shape.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;   // (the table-path kernels: the 8-bit spread table, as for shared contexts)
    int rc = hsw_engine_synchronize(c.engine);           // buffers change hands: nothing may still write the old ones
    if (rc != HSW_OK) return rc;
    rc = b ? c.bind(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, *b, t)
           : c.unbind(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check);
    if (rc == HSW_OK) hsw::drop_region_tape_positions(g->tape);     // image positions follow the pitches
    return rc;
}

int hsw_gadget_bind_region(hsw_gadget *g, const hsw_region_binding *b) try {
    return g ? rebind(g, b, nullptr) : HSW_ERR_INVALID_ARG;
} HSW_NO_UNWIND

int hsw_gadget_bind_columns(hsw_gadget *g, const hsw_region_binding *b, void *const *d_column_ptrs, size_t n_ptrs) try {
    if (!g || !b || !d_column_ptrs) return HSW_ERR_INVALID_ARG;
    hsw_column_tables t{};
    t.d_column_ptrs = d_column_ptrs; t.n_column_ptrs = n_ptrs;
    return rebind(g, b, &t);
} HSW_NO_UNWIND

int hsw_gadget_bind_column_tables(hsw_gadget *g, const hsw_region_binding *b, const hsw_column_tables *t) try {
    if (!g || !b || !t || !t->d_column_ptrs) return HSW_ERR_INVALID_ARG;
    return rebind(g, b, t);
} HSW_NO_UNWIND

int hsw_gadget_region_binding(const hsw_gadget *g, hsw_region_binding *out) try {
    if (!g || !out) return HSW_ERR_INVALID_ARG;
    const hsw::Context &c = *g->ctx;
    if (c.bound) { *out = c.binding; return HSW_OK; }
    const bool many = c.contexts() > 1;
    std::memset(out, 0, sizeof *out);
    out->d_columns = c.d_gate;
    out->column_pitch = c.layout.column_pitch();
    out->columns_capacity = c.shared && !c.group_m && c.image_columns ? c.image_columns : c.layout.columns;
    out->context_pitch = c.layout.image_cells();
    out->d_lookup = c.d_lookup;
    out->lookup_capacity = many ? c.ctx_lookups() : c.lookup_capacity;
    out->lookup_pitch = c.lookup_pitch();
    out->d_chip_dense = c.d_chip_dense; out->d_chip_spread = c.d_chip_spread;
    out->chip_col_stride = c.chip_col_stride;
    out->chip_rows_capacity = many ? c.ctx_chip_rows() : c.chip_col_stride;
    out->chip_context_pitch = c.ctx_chip_rows();         // consecutive rows of the same columns
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_reset(hsw_gadget *g) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    const int rc = hsw_engine_synchronize(g->ctx->engine);
    if (rc != HSW_OK) return rc;
    g->start_pass(0, 0, 0, g->ctx->layout.origin_lookups);   // the Context as the caller hands it over (hsw_gadget_set_origin)
    return HSW_OK;
} HSW_NO_UNWIND

// Which allocations the chip columns live in, relative to the gate stream, is worth up to 8 % of an HBM-bound
// batch on MI355X and nothing in user space predicts it: try `candidates` allocations, timing the
// gadget's own batch (every digest an empty message) on each, and keep the fastest.
int hsw_gadget_place(hsw_gadget *g, unsigned candidates, float *ms_each, unsigned *kept) try {
    if (!g || candidates == 0 || candidates > 16) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (c.shared) return HSW_ERR_UNSUPPORTED;                     // (its trial batch would run over the declared interludes)
    if (c.bound) return HSW_ERR_UNSUPPORTED;                      // (the chip columns are the caller's: nothing to place)
    if (g->cfg.cur_hash_idx != 0 || c.blocks_done != 0) return HSW_ERR_INVALID_ARG;      // a fresh or reset gadget
    const size_t n = g->cfg.max_variable_byte_sizes.size();
    if (n == 0) return HSW_ERR_INVALID_ARG;
    EngineScope es(c.engine);
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    const hipStream_t stream = es.stream;
    int rc = HSW_OK;
    const size_t col_bytes = c.owned(c.layout).chip * HSW_CELL_BYTES;
    const uint8_t nothing = 0;
    std::vector<const uint8_t *> in(n, &nothing);
    std::vector<size_t> lens(n, 0), pres(n, 0);
    std::vector<hsw_hash_result> res(n);
    struct Cand { void *dense, *spread; float ms; };
    std::vector<Cand> cands;
    auto restore = [&](size_t keep) {                        // install candidate `keep`, free the others
        for (size_t k = 0; k < cands.size(); k++)
            if (k != keep) { (void)hipFree(cands[k].dense); (void)hipFree(cands[k].spread); }
        c.d_chip_dense = cands[keep].dense;
        c.d_chip_spread = cands[keep].spread;
    };
    for (unsigned k = 0; k < candidates; k++) {
        Cand cd{c.d_chip_dense, c.d_chip_spread, 0.f};
        if (k > 0) {
            cd.dense = cd.spread = nullptr;
            hipError_t he = hipMalloc(&cd.dense, col_bytes);
            if (he == hipSuccess) he = hipMalloc(&cd.spread, col_bytes);
            if (he == hipSuccess) he = hipMemset(cd.dense, 0, col_bytes);
            if (he == hipSuccess) he = hipMemset(cd.spread, 0, col_bytes);
            if (he != hipSuccess) {                               // out of memory: judge the candidates there are
                (void)hipFree(cd.dense); (void)hipFree(cd.spread);
                (void)hipGetLastError();
                break;
            }
        }
        cands.push_back(cd);
        c.d_chip_dense = cd.dense;
        c.d_chip_spread = cd.spread;
        float best = 0.f;
        for (int rep = 0; rep < 3 && rc == HSW_OK; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            rc = hsw_gadget_digest_batch(g, n, in.data(), lens.data(), pres.data(), res.data());
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc == HSW_OK && (rep == 1 || (rep > 1 && ms < best))) best = ms;
            const int rr = hsw_gadget_reset(g);
            if (rc == HSW_OK) rc = rr;
        }
        if (rc != HSW_OK) { restore(0); return rc; }
        cands.back().ms = best;
    }
    size_t keep = 0;
    for (size_t k = 1; k < cands.size(); k++)
        if (cands[k].ms < cands[keep].ms) keep = k;
    for (size_t k = 0; k < cands.size() && ms_each; k++) ms_each[k] = cands[k].ms;
    for (size_t k = cands.size(); k < candidates && ms_each; k++) ms_each[k] = 0.f;
    if (kept) *kept = (unsigned)keep;
    restore(keep);
    hipError_t he = hipMemsetAsync(c.d_chip_dense, 0, col_bytes, stream);       // as a fresh gadget has them
    if (he == hipSuccess) he = hipMemsetAsync(c.d_chip_spread, 0, col_bytes, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    return he == hipSuccess ? HSW_OK : HSW_ERR_HIP;
} HSW_NO_UNWIND

int hsw_gadget_download_region(hsw_gadget *g, const hsw_region_host *dst) try {
    if (!g || !dst) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    EngineScope es(c.engine);
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    const hipStream_t stream = es.stream;
    const size_t cb = hsw_cell_bytes(c.repr_flags);
    hipError_t he = hipSuccess;
    // `cells` cells from cell d0 of device buffer d to cell h0 of host buffer h
    auto copy = [&](void *h, size_t h0, const void *d, uint64_t d0, size_t cells) {
        if (h && he == hipSuccess && cells)
            he = hipMemcpyAsync(static_cast<uint8_t *>(h) + h0 * cb, hsw::cell_ptr(d, d0, cb), cells * cb, hipMemcpyDeviceToHost, stream);
    };
    const hsw::Layout &l = c.layout;
    if (dst->gate && c.whole && l.max_rows) {
        // the runs of the stream between two jumps up to the cursor, for every Context begun: each lies in one column
        // and is one copy.  Rows above the origin, the gaps at column ends and the interludes' cells are the caller's
        // or nobody's: never touched.  Host layout = device layout -- but columns by pointer table, where the host
        // buffer is an UNBOUND gadget's: K images of columns x max_rows cells back to back
        c.for_each_run(c.gate_cursor, [&](uint64_t h, uint64_t lo, uint64_t hi) {
            const uint64_t dev = c.cell_offset(h * l.period + lo), at = lo + l.origin_row + l.gap_at(lo), P = l.column_pitch();
            copy(dst->gate, (size_t)(c.by_pointer ? (h * l.columns + at / P) * l.max_rows + at % P : dev), c.d_gate, dev, (size_t)(hi - lo));
        });
    } else if (dst->gate) {
        copy(dst->gate, 0, c.d_gate, 0, c.whole ? (size_t)c.gate_cursor : c.blocks_done * (size_t)c.shape.gate_cells_per_block);
    }
    // (lookup columns by pointer table: the host buffer is an unbound gadget's, Context cx's device cells lookup_extra(cx) further)
    auto copy_lookup = [&](uint64_t cx, uint64_t cell0, uint64_t cells) {
        copy(dst->lookup, (size_t)cell0, c.d_lookup, cell0 + c.lookup_extra(cx), (size_t)cells);
    };
    if (dst->lookup && c.d_lookup && c.context_images) {
        const uint64_t Lp = c.lookup_pitch();              // Context h: its own entries after the caller's queued cells
        for (uint64_t h = 0; h < g->cfg.cur_hash_idx; h++)
            copy_lookup(h, h * Lp + l.origin_lookups, c.ctx_own_lookups);
    } else if (dst->lookup && c.d_lookup && c.shared && !l.digest_lookup0.empty()) {
        const size_t M = c.group_m ? c.group_m : l.digest_entry0.size();
        const uint64_t own = c.group_m ? c.ctx_own_lookups : c.own_lookup_capacity, Lp = c.group_m ? c.lookup_pitch() : 0;
        for (size_t d = 0; d < g->cfg.cur_hash_idx; d++) {     // every digest's own entries; the interludes' are the caller's
            const size_t h = d % M, cx = d / M;                 // (a Context group: digest h of Context cx, in its own lookup column)
            const uint64_t end = h + 1 < l.digest_entry0.size() ? l.digest_entry0[h + 1] : own;
            copy_lookup(cx, cx * Lp + l.digest_lookup0[h], end - l.digest_entry0[h]);
        }
    } else if (dst->lookup && c.d_lookup) {
        copy_lookup(0, l.origin_lookups, c.lookup_cursor - l.origin_lookups);
    }
    const uint32_t ncols = c.shape.num_advice_columns;
    // the used rows of every chip column -- of every Context begun, where each has chip rows of its own (a bound region)
    // (chip columns by pointer table: the host buffers are an unbound gadget's -- ncols columns of all Contexts' rows,
    //  Context cx's after Context cx-1's -- and every column of every Context is one copy from its own allocation)
    const uint64_t per = c.chip_rows_per_context() ? c.ctx_limb_calls() : c.num_limb_sum ? c.num_limb_sum : 1;
    const size_t host_stride = c.chips_by_table() ? (size_t)hsw_chip_rows(&c.shape, 0, c.capacity_blocks) : c.chip_col_stride;
    for (uint64_t n0 = 0; n0 < c.num_limb_sum; n0 += per) {
        const uint64_t n1 = n0 + per < c.num_limb_sum ? n0 + per : c.num_limb_sum, cx = n0 / per;
        const size_t rows = (size_t)((n1 - n0 + ncols - 1) / ncols);
        for (uint32_t k = 0; k < ncols; k++) {
            const size_t hcell = c.chips_by_table() ? k * host_stride + (size_t)(n0 / ncols) : (size_t)c.chip_column_cell(cx, k, false);
            copy(dst->chip_dense, hcell, c.d_chip_dense, c.chip_column_cell(cx, k, false), rows);
            copy(dst->chip_spread, hcell, c.d_chip_spread, c.chip_column_cell(cx, k, true), rows);
        }
    }
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    return he == hipSuccess ? HSW_OK : HSW_ERR_HIP;
} HSW_NO_UNWIND

int hsw_gadget_download_region_compact(hsw_gadget *g, hsw_region_compact *dst) try {
    if (!g || !dst) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (c.repr_flags != HSW_REPR_CANONICAL) return HSW_ERR_UNSUPPORTED;      // packs canonical 32-byte cells
    if (c.context_images) return HSW_ERR_UNSUPPORTED;                         // one image per Context: not packed here
    if ((c.shared && c.layout.max_rows) || c.group_m) return HSW_ERR_UNSUPPORTED;    // shared context: interludes are the caller's
    if (c.bound) return HSW_ERR_UNSUPPORTED;                                  // a bound region: the cells between columns are the caller's
    if (!dst->wide && dst->wide_cap) return HSW_ERR_INVALID_ARG;
    EngineScope es(c.engine);
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    const hipStream_t stream = es.stream;
    const uint32_t ncols = c.shape.num_advice_columns;
    const size_t chip_cells = c.owned(c.layout).chip;
    const size_t gate_cells = c.whole ? (c.layout.max_rows ? (size_t)(c.layout.max_rows * (c.layout.break_cell.size() + 1)) : (size_t)c.gate_capacity)
                                      : c.capacity_blocks * (size_t)c.shape.gate_cells_per_block;
    hipError_t he = hipSuccess;
    if (!c.d_wide) {        // first use (or the geometry changed: set_columns / set_origin drop the staging):
                            // the 8-byte staging of every stream, the side list and its counter
        // wide cells: 4 ch negations per round (256 per block) + a few dozen per digest frame
        c.wide_cap = c.capacity_blocks * 256 + 128 * (c.init_capacity + 1) + 4 * c.capacity_blocks + 64;
        he = hipMalloc(&c.d_c_gate, (gate_cells ? gate_cells : 1) * 8);
        if (he == hipSuccess && c.d_lookup) he = hipMalloc(&c.d_c_lookup, (size_t)(c.lookup_capacity ? c.lookup_capacity : 1) * 8);
        if (he == hipSuccess) he = hipMalloc(&c.d_c_dense, chip_cells * 8);
        if (he == hipSuccess) he = hipMalloc(&c.d_c_spread, chip_cells * 8);
        if (he == hipSuccess) he = hipMalloc((void **)&c.d_wide_count, sizeof(uint32_t));
        if (he == hipSuccess) he = hipHostMalloc((void **)&c.hp_wide_count, sizeof(uint32_t), hipHostMallocDefault);
        if (he == hipSuccess) he = hipMalloc(&c.d_wide, c.wide_cap * 48);
        if (he != hipSuccess) { c.free_compact_staging(); return hsw::hip_status(he); }
    }
    he = hipMemsetAsync(c.d_wide_count, 0, sizeof(uint32_t), stream);
    auto pack = [&](uint64_t *h, void *d8, const void *d32, uint64_t sid, size_t cell0, size_t cells) {
        if (he != hipSuccess || !cells || !h) return;
        he = hsw::launch_pack64(static_cast<const uint8_t *>(d32) + cell0 * 32, static_cast<uint8_t *>(d8) + cell0 * 8, cells, sid,
                                cell0, c.d_wide, (uint32_t)c.wide_cap, c.d_wide_count, stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(h + cell0, static_cast<uint8_t *>(d8) + cell0 * 8, cells * 8, hipMemcpyDeviceToHost, stream);
    };
    if (c.whole && c.layout.max_rows) {
        // ONE pass over the image from (column 0, row 0) to the last assigned cell: the few unassigned rows at
        // the end of every column are zero on the device and travel as zeros (a launch and a copy per column
        // would cost more than the bytes they save)
        uint64_t last_col = 0, last_row = 0;
        if (c.gate_cursor) { c.layout.position(c.gate_cursor - 1, &last_col, &last_row); last_row += 1; last_col -= c.layout.origin_column; }
        // (from the origin row on: the rows above it in image column 0 are the caller's cells)
        pack(dst->gate, c.d_c_gate, c.d_gate, HSW_STREAM_GATE, (size_t)c.layout.origin_row,
             c.gate_cursor ? (size_t)(last_col * c.layout.max_rows + last_row - c.layout.origin_row) : 0);
    } else {
        pack(dst->gate, c.d_c_gate, c.d_gate, HSW_STREAM_GATE, 0,
             c.whole ? (size_t)c.gate_cursor : c.blocks_done * (size_t)c.shape.gate_cells_per_block);
    }
    if (c.d_lookup)
        pack(dst->lookup, c.d_c_lookup, c.d_lookup, HSW_STREAM_LOOKUP, (size_t)c.layout.origin_lookups, (size_t)(c.lookup_cursor - c.layout.origin_lookups));
    const size_t rows = (size_t)((c.num_limb_sum + ncols - 1) / ncols);
    if (rows == c.chip_col_stride) {         // every column full: one pass per family
        pack(dst->chip_dense, c.d_c_dense, c.d_chip_dense, HSW_STREAM_CHIP_DENSE, 0, rows * ncols);
        pack(dst->chip_spread, c.d_c_spread, c.d_chip_spread, HSW_STREAM_CHIP_SPREAD, 0, rows * ncols);
    } else {
        for (uint32_t k = 0; k < ncols; k++) {
            pack(dst->chip_dense, c.d_c_dense, c.d_chip_dense, HSW_STREAM_CHIP_DENSE, k * c.chip_col_stride, rows);
            pack(dst->chip_spread, c.d_c_spread, c.d_chip_spread, HSW_STREAM_CHIP_SPREAD, k * c.chip_col_stride, rows);
        }
    }
    // the side list: the counter and as many entries as the caller has room for, in one pass of copies
    const size_t take = dst->wide_cap < c.wide_cap ? dst->wide_cap : c.wide_cap;
    if (he == hipSuccess) he = hipMemcpyAsync(c.hp_wide_count, c.d_wide_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess && take) he = hipMemcpyAsync(dst->wide, c.d_wide, take * 48, hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return HSW_ERR_HIP;
    dst->n_wide = *c.hp_wide_count;
    if (dst->n_wide > take) return HSW_ERR_TOO_LARGE;         // n_wide says how many entries the region has
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_region_widen(const uint64_t *compact, size_t n_cells, uint64_t stream_id, const hsw_wide_cell *wide, size_t n_wide,
                     void *cells32) try {
    if ((!compact || !cells32) && n_cells) return HSW_ERR_INVALID_ARG;
    if (!wide && n_wide) return HSW_ERR_INVALID_ARG;
    uint64_t *out = static_cast<uint64_t *>(cells32);
    for (size_t i = 0; i < n_cells; i++) { out[4 * i] = compact[i]; out[4 * i + 1] = 0; out[4 * i + 2] = 0; out[4 * i + 3] = 0; }
    for (size_t k = 0; k < n_wide; k++) {
        if (wide[k].stream != stream_id) continue;
        if (wide[k].index >= n_cells) return HSW_ERR_INVALID_ARG;
        std::memcpy(out + 4 * wide[k].index, wide[k].value, 32);
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_seek(hsw_gadget *g, size_t hash_idx) try {
    if (!g || hash_idx > g->cfg.max_variable_byte_sizes.size()) return HSW_ERR_INVALID_ARG;
    if (g->ctx->context_images) return HSW_ERR_UNSUPPORTED;       // K proofs of one circuit: nothing to deal out
    if (g->ctx->shared) return HSW_ERR_UNSUPPORTED;               // shared context: the layout follows the declared origins
    if (g->ctx->bound) return HSW_ERR_UNSUPPORTED;                // a bound region is one prover's own slabs
    int rc = hsw_engine_synchronize(g->ctx->engine);
    if (rc != HSW_OK) return rc;
    hsw::Context &c = *g->ctx;
    size_t blocks = 0;
    uint64_t gate = 0, lookup = c.layout.origin_lookups;
    for (size_t h = 0; h < hash_idx; h++) {
        const size_t b = g->cfg.max_variable_byte_sizes[h];
        blocks += b / 64;
        if (c.whole) {
            hsw_frame_shape fs;
            rc = hsw_frame_query(&c.shape, b, g->cfg.is_input_range_check ? 1 : 0, &fs);
            if (rc != HSW_OK) return rc;
            gate += fs.digest_cells + (c.independent || (h == 0 && !c.layout.origin_zero_loaded) ? 1 : 0);   // + the Context's zero cell, loaded by digest #0
            lookup += fs.digest_lookups;
        }
    }
    g->start_pass(hash_idx, blocks, gate, lookup);       // (digests assigned elsewhere: nothing to tie to)
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_verify(hsw_gadget *g, hsw_verify_report *report) try {
    if (!g || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    hsw::Context &c = *g->ctx;
    if (c.repr_flags & HSW_REPR_COMPACT64) return HSW_ERR_UNSUPPORTED;         // 32-byte cells only
    // shared context: every launch checks through the jump table (the layout of the digests so far is final)
    if (c.table_path()) {
        const int rc0 = c.upload_place();
        if (rc0 != HSW_OK) return rc0;
    }
    // block0: a block launch reports blocks counted from its own first one (the frames report the pass's), the
    // gadget's report names blocks of the pass
    auto merge = [&](const hsw_verify_report &r, uint64_t block0) {
        if (r.violations && !report->violations) {
            report->first_block = r.first_block + block0; report->first_cell = r.first_cell; report->first_class = r.first_class;
        }
        report->violations += r.violations; report->checks += r.checks; report->kernel_ms += r.kernel_ms;
    };
    for (const hsw::Context::BatchRecord &b : c.batches) {
        hsw::Launch L(c, b.inputs_in_pinned, b.repr_flags);
        hsw_verify_report r;
        if (!c.whole) {
            L.blocks(b.first_block, b.n_blocks);
            const int rc = hsw_verify_blocks(c.engine, &L.a, &r);
            if (rc != HSW_OK) return rc;
            merge(r, b.first_block);
            continue;
        }
        // the launches of the batch as it was generated: runs of equally sized digests, or a group's digest indices
        for (const hsw::Run &run : hsw::batch_runs(c, b.first_digest, b.n_digests, [&](size_t k) { return g->results[b.first_digest + k].n_blocks; })) {
            const hsw::AssignedHashResult &r0 = g->results[b.first_digest + run.first];
            hsw_frame_shape fs;
            int rc = hsw_frame_query(&c.shape, r0.n_blocks * 64, g->cfg.is_input_range_check ? 1 : 0, &fs);
            if (rc != HSW_OK) return rc;
            L.run(b.first_digest + run.first, r0, r0.first_block, run.count, fs);
            rc = hsw_verify_blocks_impl(c.engine, &L.a, &r, L.per);
            if (rc != HSW_OK) return rc;
            merge(r, r0.first_block);
            std::vector<hsw_frame_desc> descs(run.count);
            for (size_t k = 0; k < run.count; k++) {
                const size_t dk = b.first_digest + run.first + k * run.step;
                descs[k] = c.frame_desc(g->results[dk], dk, g->cfg.is_input_range_check);
            }
            rc = hsw_verify_frames_impl(c.engine, descs.data(), descs.size(), L.in_blocks, L.in_pre, c.d_next_states, c.gate_stream(),
                                        c.d_lookup, L.frame_pack, b.repr_flags, &r, L.per);
            if (rc != HSW_OK) return rc;
            merge(r, 0);
        }
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_context_region(const hsw_gadget *g, size_t h, hsw_context_region *out) try {
    if (!g || !out) return HSW_ERR_INVALID_ARG;
    const hsw::Context &c = *g->ctx;
    if (!(c.context_images || c.group_m) || h >= c.contexts()) return HSW_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    const uint32_t ncols = c.shape.num_advice_columns;
    // (a Context group: Context h holds group_m digests, ctx_blocks blocks)
    const uint64_t nb = c.group_m ? c.ctx_blocks : g->cfg.max_variable_byte_sizes[h] / 64, C = c.ctx_stream();
    out->stream_cells = C;
    out->first_stream_cell = h * C;
    out->columns = c.layout.columns;
    out->max_rows = c.layout.max_rows;
    if (c.layout.max_rows) {
        uint64_t col = 0, row = 0;
        c.layout.position(C - 1, &col, &row);
        out->last_column_rows = row + 1;
        out->d_image = hsw::cell_ptr(c.d_gate, c.column_cell(h, 0));   // (by pointer table: proof h's column 0)
    } else {
        out->d_image = hsw::cell_ptr(c.d_gate, h * C);           // linear: the Context's stream
    }
    out->lookup_cells = c.ctx_lookups();
    out->d_lookup = hsw::cell_ptr(c.d_lookup, c.lookup_cell(h));   // (by pointer table: proof h's own column)
    out->chip_rows = nb * c.shape.limb_calls_per_block / ncols;
    out->chip_col_stride = c.chip_col_stride;
    // (a whole number of rows per Context; by pointer table: proof h's chip column 0 of each family)
    out->d_chip_dense = hsw::cell_ptr(c.d_chip_dense, c.chip_column_cell(h, 0, false));
    out->d_chip_spread = hsw::cell_ptr(c.d_chip_spread, c.chip_column_cell(h, 0, true));
    out->origin_column = c.layout.origin_column;
    out->origin_row = c.layout.origin_row;
    out->origin_lookups = c.layout.origin_lookups;
    out->assigned = (h + 1) * (c.group_m ? c.group_m : 1) <= g->cfg.cur_hash_idx ? 1u : 0u;   // every digest of the Context
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_cell_position(const hsw_gadget *g, uint64_t cell, uint64_t *column, uint64_t *row) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    g->ctx->layout.position(cell, column, row);
    return HSW_OK;
} HSW_NO_UNWIND

// ---- digest-to-digest copy constraints (include/hsw.h, "ties")

// gate-stream cells of one recorded tie: the child's output-byte cell (hsw_gadget_result_cells), the parent's input-byte cell
static void tie_cells(const hsw_gadget *g, const hsw_gadget::Tie &t, uint64_t *src_cell, uint64_t *dst_cell) {
    const hsw::AssignedHashResult &s = g->results[(size_t)t.src_hash], &d = g->results[(size_t)t.dst_hash];
    *src_cell = s.epilogue_cell + (uint64_t)hsw::frame::E_STATE * (s.n_blocks + 1) + (uint64_t)hsw::frame::E_WORD * (t.src_byte / 4) +
                5u * (t.src_byte % 4);
    *dst_cell = d.prologue_cell + hsw::frame::P_BYTES + t.dst_byte;
}

// a gate-stream cell some digest of this pass has been assigned (the pass order is the stream order)
static bool cell_assigned(const hsw_gadget *g, uint64_t cell) {
    const hsw::Context &c = *g->ctx;
    if (!c.whole || c.batches.empty() || c.batches[0].first_digest >= g->results.size()) return false;
    return cell >= g->results[c.batches[0].first_digest].prologue_cell && cell < c.gate_cursor;
}

static uint64_t cell_device_address(const hsw::Context &c, uint64_t cell) {
    return (uint64_t)reinterpret_cast<uintptr_t>(c.d_gate) + c.cell_offset(cell) * HSW_CELL_BYTES;   // (pointer tables: modulo 2^64)
}

int hsw_gadget_ties(const hsw_gadget *g, hsw_cell_tie *out, size_t cap, size_t *n, uint64_t *prefix_bytes_untied) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;                  // block-stream contexts have no byte cells
    if (n) *n = g->ties.size();
    if (prefix_bytes_untied) *prefix_bytes_untied = g->tie_prefix_bytes;
    if (!out) return HSW_OK;
    if (cap < g->ties.size()) return HSW_ERR_TOO_LARGE;
    for (size_t i = 0; i < g->ties.size(); i++) {
        const hsw_gadget::Tie &t = g->ties[i];
        hsw_cell_tie &o = out[i];
        o.src_hash = t.src_hash; o.dst_hash = t.dst_hash; o.src_byte = t.src_byte; o.dst_byte = t.dst_byte;
        tie_cells(g, t, &o.src_cell, &o.dst_cell);
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_cell_address(const hsw_gadget *g, uint64_t cell, void **d_cell) try {
    if (!g || !d_cell) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;
    if (!cell_assigned(g, cell)) return HSW_ERR_INVALID_ARG;
    *d_cell = reinterpret_cast<void *>((uintptr_t)cell_device_address(*g->ctx, cell));
    return HSW_OK;
} HSW_NO_UNWIND

// n pairs (cells[2 i], cells[2 i + 1]): every cell validated and resolved before anything is launched
static int verify_pairs(hsw_gadget *g, size_t n, const std::vector<uint64_t> &cells, hsw_tie_report *report) {
    hsw::Context &c = *g->ctx;
    std::memset(report, 0, sizeof *report);
    if (n == 0) return HSW_OK;
    std::vector<uint64_t> addr(2 * n);
    for (size_t i = 0; i < 2 * n; i++) {
        const uint64_t cell = cells[i];
        if (!cell_assigned(g, cell)) return hsw_engine_fail(c.engine, HSW_ERR_INVALID_ARG, "a cell out of range or not assigned in this pass");
        addr[i] = cell_device_address(c, cell);
    }
    if (n > g->pairs_cap) {                                  // (every earlier check has been waited for: nothing reads the old one)
        EngineScope es(c.engine);
        if (!es.ok) return HSW_ERR_NO_DEVICE;
        void *p = nullptr;
        const size_t cap = n > 2 * g->pairs_cap ? n : 2 * g->pairs_cap;
        const hipError_t he = hipMalloc(&p, cap * 16);
        if (he != hipSuccess) return hsw::hip_status(he);
        (void)hipFree(g->d_pairs);
        g->d_pairs = p; g->pairs_cap = cap;
    }
    return hsw_verify_pairs_impl(c.engine, addr.data(), g->d_pairs, n, report);
}

int hsw_gadget_verify_ties(hsw_gadget *g, hsw_tie_report *report) try {
    if (!g || !report) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;
    std::vector<uint64_t> cells(2 * g->ties.size());
    for (size_t i = 0; i < g->ties.size(); i++) tie_cells(g, g->ties[i], &cells[2 * i], &cells[2 * i + 1]);
    return verify_pairs(g, g->ties.size(), cells, report);
} HSW_NO_UNWIND

int hsw_gadget_verify_equal(hsw_gadget *g, const uint64_t *cells_a, const uint64_t *cells_b, size_t n, hsw_tie_report *report) try {
    if (!g || !report || ((!cells_a || !cells_b) && n)) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;
    std::vector<uint64_t> cells(2 * n);
    for (size_t i = 0; i < n; i++) { cells[2 * i] = cells_a[i]; cells[2 * i + 1] = cells_b[i]; }
    return verify_pairs(g, n, cells, report);
} HSW_NO_UNWIND

int hsw_gadget_set_repr(hsw_gadget *g, uint32_t repr) try {
    if (!g || (repr & ~HSW_REPR_MASK) || repr == HSW_REPR_MASK) return HSW_ERR_INVALID_ARG;
    if (g->ctx->whole && (repr & HSW_REPR_COMPACT64)) return HSW_ERR_UNSUPPORTED;   // frames hold full-width cells
    if (g->ctx->blocks_done != 0 && hsw_cell_bytes(repr) != hsw_cell_bytes(g->ctx->repr_flags))
        return HSW_ERR_INVALID_ARG;               // the cell size of a context's streams cannot change midway
    g->ctx->repr_flags = repr;
    return HSW_OK;
} HSW_NO_UNWIND

}  // extern "C"
