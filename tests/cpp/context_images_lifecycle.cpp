// HSW_GADGET_CONTEXT_IMAGES on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in
// HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): flag validation, the layout
// calls, hsw_gadget_context_region for every proof, a failing hsw_gadget_set_columns / hsw_gadget_set_origin that
// must leave the layout and its buffers intact, host deliveries into EXACT-size buffers, destroy without a leak.
// Built and run by tests/test_context_images_host.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
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

static const uint32_t IMAGES = HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES;
static const uint64_t MAX_ROWS = (1u << 17) - 9;

static void same_region(const hsw_context_region &a, const hsw_context_region &b) {
    CHECK(a.d_image == b.d_image && a.d_lookup == b.d_lookup && a.columns == b.columns && a.max_rows == b.max_rows &&
          a.last_column_rows == b.last_column_rows && a.lookup_cells == b.lookup_cells && a.origin_row == b.origin_row &&
          a.origin_column == b.origin_column && a.origin_lookups == b.origin_lookups && a.stream_cells == b.stream_cells);
}

int main() {
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    const size_t K = 5;
    size_t sizes[K] = {1024, 1024, 1024, 1024, 1024};
    hsw_gadget *g = nullptr;
    // the flag needs whole-digest + independent, and K proofs of one size
    CHECK(hsw_gadget_create_ex(e, sizes, K, 1, HSW_GADGET_CONTEXT_IMAGES, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_ex(e, sizes, K, 1, HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_CONTEXT_IMAGES, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_ex(e, sizes, K, 1, HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g) == HSW_ERR_INVALID_ARG && !g);
    sizes[3] = 512;
    CHECK(hsw_gadget_create_ex(e, sizes, K, 1, IMAGES, &g) == HSW_ERR_UNSUPPORTED && !g);
    sizes[3] = 1024;
    // without the flag nothing changes: an independent gadget refuses columns, origins and context_region
    CHECK(hsw_gadget_create_ex(e, sizes, K, 1, HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT, &g) == HSW_OK);
    uint64_t columns = 0;
    hsw_context_region reg;
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_set_origin(g, 1, 2, 0, 3) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_context_region(g, 0, &reg) == HSW_ERR_INVALID_ARG);
    hsw_gadget_destroy(g);
    g = nullptr;

    // create -> set_origin -> set_columns -> context_region for every proof
    CHECK(hsw_gadget_create_ex(e, sizes, K, 1, IMAGES, &g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 2, 69000, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_OK && columns >= 9 && columns <= HSW_MAX_BREAKS + 1);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns == columns && v.lookup_capacity % K == 0);
    std::vector<hsw_context_region> regs(K);
    for (size_t h = 0; h < K; h++) {
        CHECK(hsw_gadget_context_region(g, h, &regs[h]) == HSW_OK);
        const hsw_context_region &r = regs[h];
        CHECK(r.columns == columns && r.max_rows == MAX_ROWS && r.origin_column == 2 && r.origin_row == 69000);
        CHECK(r.d_image == (uint8_t *)v.d_gate + h * columns * MAX_ROWS * HSW_CELL_BYTES);
        CHECK(r.lookup_cells * K == v.lookup_capacity && r.origin_lookups == 5);
        CHECK(r.d_lookup == (uint8_t *)v.d_lookup + h * r.lookup_cells * HSW_CELL_BYTES);
        CHECK(r.stream_cells == 1116315 && r.first_stream_cell == h * r.stream_cells && r.chip_rows == 16 * 4120 / 2);
        CHECK(r.d_chip_dense == (uint8_t *)v.d_chip_dense + h * r.chip_rows * HSW_CELL_BYTES && r.assigned == 0);
        CHECK(r.last_column_rows > 0 && r.last_column_rows <= MAX_ROWS);
    }
    CHECK(hsw_gadget_context_region(g, K, &reg) == HSW_ERR_INVALID_ARG);
    // failing calls leave the layout (and its buffers) intact
    CHECK(hsw_gadget_set_columns(g, 69348 + 16, &columns) == HSW_ERR_TOO_LARGE);        // G + 16 rows: more than 17 columns
    CHECK(hsw_gadget_set_origin(g, 0, MAX_ROWS, 0, 9) == HSW_ERR_INVALID_ARG);          // row outside the column
    for (size_t h = 0; h < K; h++) {
        CHECK(hsw_gadget_context_region(g, h, &reg) == HSW_OK);
        same_region(reg, regs[h]);
    }
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns == regs[0].columns && v.max_rows == MAX_ROWS);

    // a synthesis pass (the stub runs no kernel) and every host delivery into exact-size buffers
    std::vector<uint8_t> msg(56, 1);
    std::vector<const uint8_t *> in(K, msg.data());
    std::vector<size_t> lens(K, msg.size()), pre(K, 0);
    std::vector<hsw_hash_result> res(K);
    CHECK(hsw_gadget_digest_batch(g, K, in.data(), lens.data(), pre.data(), res.data()) == HSW_OK);
    CHECK(res[K - 1].prologue_cell == (K - 1) * regs[0].stream_cells && res[K - 1].end_cell == K * regs[0].stream_cells);
    CHECK(res[1].prologue_lookup == regs[0].lookup_cells + 5);
    CHECK(hsw_gadget_context_region(g, K - 1, &reg) == HSW_OK && reg.assigned == 1);
    uint64_t col = 0, row = 0;
    CHECK(hsw_gadget_cell_position(g, res[3].prologue_cell, &col, &row) == HSW_OK && col == 2 && row == 69000);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const size_t img_cells = K * (size_t)(v.columns * v.max_rows), chip_cells = 2 * v.chip_col_stride;
    std::vector<uint64_t> gate(img_cells * 4), lookup(v.lookup_capacity * 4), cd(chip_cells * 4), cs(chip_cells * 4);
    hsw_region_host dst = {gate.data(), lookup.data(), cd.data(), cs.data()};
    CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK && tape.gate_cells == K * regs[0].stream_cells);
    std::vector<uint64_t> distinct(tape.n_distinct * 4);
    size_t n = 0;
    CHECK(hsw_gadget_download_region_distinct(g, distinct.data(), tape.n_distinct, &n) == HSW_OK && n == tape.n_distinct);
    CHECK(hsw_gadget_replay_region(g, distinct.data(), &dst, 3) == HSW_OK);
    hsw_region_compact cdst = {};
    CHECK(hsw_gadget_download_region_compact(g, &cdst) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_seek(g, 1) == HSW_ERR_UNSUPPORTED);
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);

    // the next pass at another origin: a Context with its zero cell and queued lookups -- new layout, one cell less
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 1, 40000, 1, 1234) == HSW_OK);
    CHECK(hsw_gadget_context_region(g, 2, &reg) == HSW_OK && reg.stream_cells == 1116314 && reg.origin_lookups == 1234);
    CHECK(hsw_gadget_digest_batch(g, K, in.data(), lens.data(), pre.data(), res.data()) == HSW_OK);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    std::vector<uint64_t> gate2(K * (size_t)(v.columns * v.max_rows) * 4), lookup2(v.lookup_capacity * 4);
    hsw_region_host dst2 = {gate2.data(), lookup2.data(), cd.data(), cs.data()};
    CHECK(hsw_gadget_download_region(g, &dst2) == HSW_OK);
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK && tape.gate_cells == K * 1116314);
    distinct.assign(tape.n_distinct * 4, 0);
    CHECK(hsw_gadget_download_region_distinct(g, distinct.data(), tape.n_distinct, &n) == HSW_OK);
    CHECK(hsw_gadget_replay_region(g, distinct.data(), &dst2, 2) == HSW_OK);
    hsw_gadget_destroy(g);
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::puts("context images lifecycle ok");
    return 0;
}
