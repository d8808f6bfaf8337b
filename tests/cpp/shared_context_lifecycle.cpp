// HSW_GADGET_SHARED_CONTEXT on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in
// HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): flag validation, layouts past 17
// columns, every hsw_gadget_set_digest_origin refusal (each leaving the positions unchanged), an interlude that
// grows the image, host deliveries that leave the interlude's cells alone, destroy without a leak.
// Built and run by tests/test_shared_context_host.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/hsw.h"

extern "C" {
size_t hip_stub_live_device_allocations();
size_t hip_stub_live_pinned_allocations();
size_t hip_stub_live_events();
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static const uint32_t SHARED = HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_SHARED_CONTEXT;
static const uint64_t MAX_ROWS = (1u << 17) - 9;

static void pos(hsw_gadget *g, uint64_t cell, uint64_t *col, uint64_t *row) {
    CHECK(hsw_gadget_cell_position(g, cell, col, row) == HSW_OK);
}

int main() {
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    size_t sizes[4] = {1024, 1024, 1024, 1024};
    hsw_gadget *g = nullptr;
    // the flag needs whole-digest, and goes with neither independent contexts nor context images
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, HSW_GADGET_SHARED_CONTEXT, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, SHARED | HSW_GADGET_INDEPENDENT, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, SHARED | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g) ==
          HSW_ERR_INVALID_ARG && !g);

    // four bench-circuit digests need about 35 columns: too large without the flag, accepted with it
    uint64_t columns = 0;
    CHECK(hsw_gadget_create_ex(e, sizes, 4, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_ERR_TOO_LARGE);
    CHECK(hsw_gadget_set_digest_origin(g, 1, 0, 0, 0) == HSW_ERR_INVALID_ARG);        // not a shared context
    hsw_gadget_destroy(g);
    CHECK(hsw_gadget_create_ex(e, sizes, 4, 1, SHARED, &g) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, 0, 0, 0) == HSW_ERR_INVALID_ARG);        // no column image yet
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_OK && columns > HSW_MAX_BREAKS + 1 && columns < 40);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns == columns);
    hsw_gadget_destroy(g);
    g = nullptr;

    // two digests; digest 0 at origin (2, 131000) with 7 queued lookups
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, SHARED, &g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 2, 131000, 0, 7) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_OK);
    std::vector<uint8_t> msg(100, 3);
    const uint8_t *in[1] = {msg.data()};
    size_t len[1] = {msg.size()}, pre[1] = {0};
    hsw_hash_result r0, r1;
    CHECK(hsw_gadget_digest_batch(g, 1, in, len, pre, &r0) == HSW_OK);
    CHECK(r0.prologue_lookup == 7);
    uint64_t c = 0, rw = 0, c_last = 0, r_last = 0, c_e = 0, r_e = 0;
    pos(g, r0.prologue_cell, &c, &rw);
    CHECK(c == 2 && rw == 131000);
    pos(g, r0.end_cell - 1, &c_last, &r_last);                   // next free cell: (c_last, r_last + 1)
    pos(g, r0.end_cell, &c_e, &r_e);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint64_t lk_after0 = v.lookup_cells, cols0 = v.columns;
    // every refusal leaves the layout as it was
    CHECK(hsw_gadget_set_digest_origin(g, 0, c_last + 1, 0, lk_after0) == HSW_ERR_INVALID_ARG);          // h = 0
    CHECK(hsw_gadget_set_digest_origin(g, 2, c_last + 1, 0, lk_after0) == HSW_ERR_INVALID_ARG);          // h >= n_hashes
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last + 1, MAX_ROWS, lk_after0) == HSW_ERR_INVALID_ARG);   // row outside
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last, r_last, lk_after0) == HSW_ERR_INVALID_ARG);         // before the free cell
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last - 1, r_last + 5, lk_after0) == HSW_ERR_INVALID_ARG); // earlier column
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last + 1, 0, lk_after0 - 1) == HSW_ERR_INVALID_ARG);      // lookups below
    CHECK(hsw_gadget_set_digest_origin(g, 1, 0, 5, lk_after0) == HSW_ERR_INVALID_ARG);                   // before the origin column
    CHECK(hsw_gadget_set_digest_origin(g, 1, 2 + HSW_GADGET_MAX_COLUMNS, 0, lk_after0) == HSW_ERR_TOO_LARGE);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == c_e && rw == r_e);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns == cols0);
    // the next free cell itself is no interlude: the layout stays as it is
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last, r_last + 1, lk_after0) == HSW_OK);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == c_e && rw == r_e);
    // an interlude into column 40: the image grows, earlier device pointers are stale
    void *old_gate = v.d_gate;
    CHECK(hsw_gadget_set_digest_origin(g, 1, 40, 17, lk_after0 + 11) == HSW_OK);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == 40 && rw == 17);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns > 39 && v.d_gate != old_gate);
    // reset keeps the declarations; set_columns clears them
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == 40 && rw == 17);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_OK);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == c_e && rw == r_e);
    // a pass with the interlude declared up front, as ONE batch (the stub runs no kernel)
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last + 1, 3, lk_after0 + 11) == HSW_OK);
    const uint8_t *in2[2] = {msg.data(), msg.data()};
    size_t len2[2] = {msg.size(), 55}, pre2[2] = {0, 0};
    hsw_hash_result rr[2];
    CHECK(hsw_gadget_digest_batch(g, 2, in2, len2, pre2, rr) == HSW_OK);
    r1 = rr[1];
    CHECK(r1.prologue_cell == r0.end_cell && r1.prologue_lookup == lk_after0 + 11);
    pos(g, r1.prologue_cell, &c, &rw);
    CHECK(c == c_last + 1 && rw == 3);
    hsw_result_cells rc;
    CHECK(hsw_gadget_result_cells(g, 1, &rc) == HSW_OK && rc.input_len_pos[0] == c_last + 1);
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last + 2, 0, lk_after0 + 11) == HSW_ERR_INVALID_ARG);     // already assigned
    // deliveries into exact-size buffers: the interlude's cells and lookup entries keep the caller's sentinel
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint64_t base = (uint64_t)(v.columns) * v.max_rows;
    std::vector<uint64_t> gate(base * 4, 0x5a5a5a5a5a5a5a5aull), lookup(v.lookup_capacity * 4, 0x5a5a5a5a5a5a5a5aull);
    std::vector<uint64_t> cd(2 * v.chip_col_stride * 4), cs(2 * v.chip_col_stride * 4);
    hsw_region_host dst = {gate.data(), lookup.data(), cd.data(), cs.data()};
    CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
    const uint64_t free_at = (c_last - 2) * MAX_ROWS + r_last + 1, land = (c_last + 1 - 2) * MAX_ROWS + 3;
    for (uint64_t i = free_at; i < land; i += 997) CHECK(gate[4 * i] == 0x5a5a5a5a5a5a5a5aull);
    for (uint64_t i = lk_after0; i < lk_after0 + 11; i++) CHECK(lookup[4 * i] == 0x5a5a5a5a5a5a5a5aull);
    CHECK(gate[4 * land] == 0 && lookup[4 * (lk_after0 + 11)] == 0);
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK);
    std::vector<uint64_t> distinct(tape.n_distinct * 4 + 4);
    size_t n = 0;
    CHECK(hsw_gadget_download_region_distinct(g, distinct.data(), tape.n_distinct, &n) == HSW_OK);
    std::fill(gate.begin(), gate.end(), 0x5a5a5a5a5a5a5a5aull);
    std::fill(lookup.begin(), lookup.end(), 0x5a5a5a5a5a5a5a5aull);
    CHECK(hsw_gadget_replay_region(g, distinct.data(), &dst, 3) == HSW_OK);
    for (uint64_t i = free_at; i < land; i += 997) CHECK(gate[4 * i] == 0x5a5a5a5a5a5a5a5aull);
    for (uint64_t i = lk_after0; i < lk_after0 + 11; i++) CHECK(lookup[4 * i] == 0x5a5a5a5a5a5a5a5aull);
    // the calls that refuse in this mode
    hsw_region_compact cdst = {};
    CHECK(hsw_gadget_download_region_compact(g, &cdst) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_seek(g, 1) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_place(g, 2, nullptr, nullptr) == HSW_ERR_UNSUPPORTED);
    hsw_verify_report vrep;
    CHECK(hsw_gadget_verify(g, &vrep) == HSW_OK);                                  // the table-path verifier
    // the same declaration again changes nothing; set_origin at the same place drops the declaration
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_last + 1, 3, lk_after0 + 11) == HSW_OK);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == c_last + 1 && rw == 3);
    CHECK(hsw_gadget_set_origin(g, 2, 131000, 0, 7) == HSW_OK);
    pos(g, r0.end_cell, &c, &rw);
    CHECK(c == c_e && rw == r_e);
    hsw_gadget_destroy(g);
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::puts("shared context lifecycle ok");
    return 0;
}
