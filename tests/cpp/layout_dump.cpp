// Prints, as text, where a fixed list of gadgets puts every digest: hsw_gadget_streams, every hsw_hash_result,
// hsw_gadget_cell_position around every jump of the stream-to-image map, hsw_gadget_context_region, which host cells
// hsw_gadget_download_region writes, and hsw_pack_plan_query.  Runs against the stand-in HIP runtime of hip_stub.cpp
// (no kernel runs: device cells stay zero), under ASan + UBSan + LeakSanitizer.  tests/test_layout_golden.py compares
// the text with tests/golden/gadget_layouts.txt, recorded from the commit named there.
// output_bytes of a result is not printed: without kernels it is whatever the pinned staging held.
// With the argument `tables` it prints a second list instead -- the smallest gadgets that reach every form of the
// device jump table (Context::place_host): the table's words, the binding, the context regions, the device offsets of
// the cells around every jump and the delivered host cells, unbound, bound by pitch and bound by pointer table
// (tests/golden/gadget_place_tables.txt).
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_gadget.hpp"   // (hsw.h + Context::upload_place / place_host)

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

typedef unsigned long long ull;
static const uint32_t WHOLE = HSW_GADGET_WHOLE_DIGEST;
static const uint32_t SHARED = HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_SHARED_CONTEXT;
static const uint32_t IMAGES = HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES;
static const uint64_t MAX_ROWS = (1u << 17) - 9;
static const uint64_t SENTINEL = 0x5a5a5a5a5a5a5a5aull;
static hsw_engine *E = nullptr;

static hsw_gadget *create(const std::vector<size_t> &sizes, int rc_inputs, uint32_t flags) {
    hsw_gadget *g = nullptr;
    CHECK(hsw_gadget_create_ex(E, sizes.data(), sizes.size(), rc_inputs, flags, &g) == HSW_OK);
    return g;
}

static void streams(hsw_gadget *g) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    std::printf("  streams: max_rows %llu columns %llu gate %llu/%llu lookup %llu/%llu blocks %zu/%zu limbs %llu hash %zu "
                "origin (%llu,%llu) lookups %llu zero %u stride %zu\n",
                (ull)v.max_rows, (ull)v.columns, (ull)v.gate_cells, (ull)v.gate_capacity, (ull)v.lookup_cells,
                (ull)v.lookup_capacity, v.blocks_done, v.capacity_blocks, (ull)v.num_limb_sum, v.cur_hash_idx,
                (ull)v.origin_column, (ull)v.origin_row, (ull)v.origin_lookups, v.origin_zero_loaded, v.chip_col_stride);
}

// digests [first, first + n) of the pass as one batch: messages of 3 + 61 * index bytes (cut to what the size takes)
static std::vector<hsw_hash_result> digest(hsw_gadget *g, const std::vector<size_t> &sizes, size_t first, size_t n) {
    std::vector<std::vector<uint8_t>> msgs;
    std::vector<const uint8_t *> in;
    std::vector<size_t> len, pre(n, 0);
    for (size_t i = 0; i < n; i++) {
        size_t l = 3 + 61 * (first + i);
        if (l + 9 > sizes[first + i]) l = sizes[first + i] - 9;
        msgs.emplace_back(l, (uint8_t)(first + i + 1));
    }
    for (size_t i = 0; i < n; i++) { in.push_back(msgs[i].data()); len.push_back(msgs[i].size()); }
    std::vector<hsw_hash_result> r(n);
    CHECK(hsw_gadget_digest_batch(g, n, in.data(), len.data(), pre.data(), r.data()) == HSW_OK);
    for (size_t i = 0; i < n; i++)
        std::printf("  result %zu: len %llu first_block %zu n_blocks %zu spread %llu rounds %zu/%zu cells %llu %llu %llu %llu "
                    "lookups %llu %llu %llu\n", first + i, (ull)r[i].input_len, r[i].first_block, r[i].n_blocks,
                    (ull)r[i].spread_cursor0, r[i].num_round, r[i].target_round, (ull)r[i].prologue_cell, (ull)r[i].block_cell,
                    (ull)r[i].epilogue_cell, (ull)r[i].end_cell, (ull)r[i].prologue_lookup, (ull)r[i].block_lookup,
                    (ull)r[i].epilogue_lookup);
    return r;
}

static uint64_t fnv(uint64_t sum, std::initializer_list<uint64_t> words) {
    for (uint64_t w : words) sum = (sum ^ w) * 0x100000001b3ull;
    return sum;
}
static const uint64_t FNV0 = 0xcbf29ce484222325ull;
static const int SHOWN = 4;      // lines printed one by one per list; the whole list goes into its FNV-1a sum

// every jump of the map (a cell that is not one row below the cell before it) with the cell before it, and every
// 4,099th cell: the first of them as text, all of them in a sum (the text stays a few hundred lines)
static void positions(hsw_gadget *g) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    uint64_t pc = 0, pr = 0, cells = FNV0, jumps = FNV0;
    int n_jumps = 0, n_cells = 0;
    for (uint64_t i = 0; i < v.gate_capacity; i++) {
        uint64_t c = 0, r = 0;
        CHECK(hsw_gadget_cell_position(g, i, &c, &r) == HSW_OK);
        if (i && !(c == pc && r == pr + 1)) {
            if (n_jumps++ < SHOWN)
                std::printf("  jump before cell %llu: (%llu,%llu) -> (%llu,%llu)\n", (ull)i, (ull)pc, (ull)pr, (ull)c, (ull)r);
            jumps = fnv(jumps, {i, pc, pr, c, r});
        }
        if (i % 4099 == 0) {
            if (n_cells++ < SHOWN) std::printf("  cell %llu: (%llu,%llu)\n", (ull)i, (ull)c, (ull)r);
            cells = fnv(cells, {i, c, r});
        }
        pc = c; pr = r;
    }
    std::printf("  %d jumps: sum %016llx; every 4099th of %llu cells: sum %016llx\n", n_jumps, (ull)jumps, (ull)v.gate_capacity, (ull)cells);
}

static void runs(const char *what, const std::vector<uint64_t> &cells) {
    const size_t n = cells.size() / 4;
    uint64_t sum = FNV0;
    int n_runs = 0;
    for (size_t i = 0; i < n;) {
        if (cells[4 * i] == SENTINEL) { i++; continue; }
        size_t j = i;
        while (j < n && cells[4 * j] != SENTINEL) j++;
        if (n_runs++ < SHOWN) std::printf("  delivered %s [%zu, %zu)\n", what, i, j);
        sum = fnv(sum, {i, j});
        i = j;
    }
    std::printf("  %d runs of %s delivered: sum %016llx\n", n_runs, what, (ull)sum);
}

// hsw_gadget_download_region into exact-size buffers full of a sentinel: the cells it writes (zeros here)
static void delivery_into(hsw_gadget *g, uint64_t gate_cells, uint64_t chip_stride) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    std::vector<uint64_t> gate(gate_cells * 4, SENTINEL), lookup((v.lookup_capacity ? v.lookup_capacity : 1) * 4, SENTINEL);
    std::vector<uint64_t> cd(2 * chip_stride * 4, SENTINEL), cs(2 * chip_stride * 4, SENTINEL);
    hsw_region_host dst = {gate.data(), v.d_lookup ? lookup.data() : nullptr, cd.data(), cs.data()};
    CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
    runs("gate", gate);
    if (v.d_lookup) runs("lookup", lookup);
    runs("chip", cd);
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);                 // (the launch builder under the sanitizers; no kernel runs)
}

static void delivery(hsw_gadget *g, uint64_t n_images) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    delivery_into(g, v.max_rows ? v.columns * v.max_rows * n_images : v.gate_capacity, v.chip_col_stride);
}

static void context_regions(hsw_gadget *g, size_t k) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    for (size_t h = 0; h < k; h++) {
        hsw_context_region r;
        CHECK(hsw_gadget_context_region(g, h, &r) == HSW_OK);
        std::printf("  context %zu: image +%lld lookup +%lld dense +%lld spread +%lld columns %llu rows %llu last %llu stream %llu "
                    "first %llu lookups %llu chip %llu/%llu origin (%llu,%llu) %llu assigned %u\n", h,
                    (long long)((uint8_t *)r.d_image - (uint8_t *)v.d_gate), (long long)((uint8_t *)r.d_lookup - (uint8_t *)v.d_lookup),
                    (long long)((uint8_t *)r.d_chip_dense - (uint8_t *)v.d_chip_dense),
                    (long long)((uint8_t *)r.d_chip_spread - (uint8_t *)v.d_chip_spread), (ull)r.columns, (ull)r.max_rows,
                    (ull)r.last_column_rows, (ull)r.stream_cells, (ull)r.first_stream_cell, (ull)r.lookup_cells, (ull)r.chip_rows,
                    (ull)r.chip_col_stride, (ull)r.origin_column, (ull)r.origin_row, (ull)r.origin_lookups, r.assigned);
    }
}

static void next_free(hsw_gadget *g, const hsw_hash_result &r, uint64_t *col, uint64_t *row) {
    CHECK(hsw_gadget_cell_position(g, r.end_cell - 1, col, row) == HSW_OK);
    *row += 1;
}

static void plain(const char *name, uint32_t flags, const std::vector<size_t> &sizes, int rc_inputs, bool columns_first,
                  const uint64_t *origin, uint64_t rows) {
    std::printf("%s\n", name);
    hsw_gadget *g = create(sizes, rc_inputs, flags);
    uint64_t cols = 0;
    if (rows && columns_first) CHECK(hsw_gadget_set_columns(g, rows, &cols) == HSW_OK);
    if (origin) CHECK(hsw_gadget_set_origin(g, origin[0], origin[1], (int)origin[2], origin[3]) == HSW_OK);
    if (rows && !columns_first) CHECK(hsw_gadget_set_columns(g, rows, &cols) == HSW_OK);
    std::printf("  set_columns: %llu\n", (ull)cols);
    streams(g);
    digest(g, sizes, 0, sizes.size());
    streams(g);
    if (flags & HSW_GADGET_WHOLE_DIGEST) positions(g);
    if (flags & HSW_GADGET_CONTEXT_IMAGES) context_regions(g, sizes.size());
    delivery(g, (flags & HSW_GADGET_CONTEXT_IMAGES) ? sizes.size() : 1);
    hsw_gadget_destroy(g);
}

// the interludes of tests/test_gpu_shared_context.py: digest 1 lands (dcol, drow) past the next free cell after digest 0
static void interlude(const char *name, uint64_t dcol, uint64_t drow, bool absolute, bool batch) {
    std::printf("shared context, interlude %s, %s\n", name, batch ? "one batch" : "per digest");
    const std::vector<size_t> sizes = {1024, 1024};
    hsw_gadget *g = create(sizes, 1, SHARED);
    uint64_t cols = 0, fc = 0, fr = 0;
    CHECK(hsw_gadget_set_origin(g, 2, 131000, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &cols) == HSW_OK);
    std::vector<hsw_hash_result> r = digest(g, sizes, 0, 1);
    next_free(g, r[0], &fc, &fr);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint64_t lk = v.lookup_cells + 9;
    const uint64_t col = absolute ? dcol : fc + dcol, row = absolute || dcol ? drow : fr + drow;
    if (batch) CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, col, row, lk) == HSW_OK);
    streams(g);
    if (batch) digest(g, sizes, 0, 2);
    else digest(g, sizes, 1, 1);
    streams(g);
    positions(g);
    delivery(g, 1);
    hsw_gadget_destroy(g);
}

// 4 and 9 bench-circuit digests as one batch (about 35 and 77 columns), with and without an interlude in the middle
static void wide(size_t k, bool with_interlude) {
    std::printf("shared context, %zu digests, %s\n", k, with_interlude ? "interlude" : "back to back");
    const std::vector<size_t> sizes(k, 1024);
    hsw_gadget *g = create(sizes, 1, SHARED);
    uint64_t cols = 0;
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &cols) == HSW_OK);
    std::printf("  set_columns: %llu\n", (ull)cols);
    if (with_interlude) {
        std::vector<hsw_hash_result> r = digest(g, sizes, 0, k / 2);
        uint64_t fc = 0, fr = 0;
        next_free(g, r.back(), &fc, &fr);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_set_digest_origin(g, k / 2, fc + 3, 500, v.lookup_cells + 100) == HSW_OK);
    }
    digest(g, sizes, 0, k);
    streams(g);
    positions(g);
    delivery(g, 1);
    hsw_gadget_destroy(g);
}

static void layout_changes() {
    std::printf("plain image, another column height and origin between two passes\n");
    const std::vector<size_t> sizes = {128, 128};
    hsw_gadget *g = create(sizes, 1, WHOLE);
    uint64_t cols = 0;
    CHECK(hsw_gadget_set_origin(g, 0, 130, 0, 0) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &cols) == HSW_OK);
    digest(g, sizes, 0, 2);
    streams(g);
    positions(g);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS - 1000, &cols) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 3, 129990, 1, 11) == HSW_OK);
    digest(g, sizes, 0, 2);
    streams(g);
    positions(g);
    delivery(g, 1);
    // a layout that cannot be had: refused
    std::printf("  set_origin to the last row: %d\n", hsw_gadget_set_origin(g, 0, MAX_ROWS - 1001, 0, 0));
    hsw_gadget_destroy(g);

    std::printf("shared context, other declarations between two passes\n");
    const std::vector<size_t> three = {1024, 128, 1024};
    g = create(three, 1, SHARED);
    CHECK(hsw_gadget_set_origin(g, 2, 131000, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &cols) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, 40, 17, 60000) == HSW_OK);         // grows the image
    CHECK(hsw_gadget_set_digest_origin(g, 2, 41, 130000, 70000) == HSW_OK);
    digest(g, three, 0, 3);
    streams(g);
    positions(g);
    delivery(g, 1);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, 12, 100, 56000) == HSW_OK);        // replaces digest 1's, drops digest 2's
    digest(g, three, 0, 2);
    CHECK(hsw_gadget_set_digest_origin(g, 2, 14, 0, 66000) == HSW_OK);
    digest(g, three, 2, 1);
    streams(g);
    positions(g);
    delivery(g, 1);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 1, 17, 1, 3) == HSW_OK);                    // every declaration dropped
    digest(g, three, 0, 3);
    streams(g);
    positions(g);
    delivery(g, 1);
    hsw_gadget_destroy(g);
}

static void pack_plans() {
    struct Case { size_t n_blocks; uint64_t start_row, max_rows; uint32_t mode; };
    const Case cases[6] = {{1, 0, 1u << 20, HSW_MODE_DEFAULT}, {2, 100, 131000, HSW_MODE_HALO2_INTERNALS},
                           {16, 5000, 131063, HSW_MODE_HALO2_INTERNALS}, {4, 0, 92000, HSW_MODE_DEFAULT},
                           {3, 69000, 70000, HSW_MODE_HALO2_INTERNALS}, {5, 17, 20011, HSW_MODE_DEFAULT}};
    for (const Case &c : cases) {
        hsw_shape s;
        CHECK(hsw_shape_query_ex(8, 2, c.mode, &s) == HSW_OK);
        hsw_pack_plan p;
        const int rc = hsw_pack_plan_query(&s, c.n_blocks, c.start_row, c.max_rows, &p);
        std::printf("pack plan %zu blocks from row %llu of %llu, mode %u: rc %d breaks %u columns %u span %llu end_row %llu\n",
                    c.n_blocks, (ull)c.start_row, (ull)c.max_rows, c.mode, rc, p.n_breaks, p.columns_touched, (ull)p.span_cells,
                    (ull)p.end_row);
        for (uint32_t k = 0; k < p.n_breaks; k++) std::printf("  break %u: cell %llu gap %llu\n", k, (ull)p.break_cell[k], (ull)p.break_gap[k]);
    }
    hsw_shape s;
    CHECK(hsw_shape_query_ex(8, 2, HSW_MODE_HALO2_INTERNALS, &s) == HSW_OK);
    hsw_pack_plan p;
    std::printf("pack plan 40 blocks of 131063 rows: rc %d\n", hsw_pack_plan_query(&s, 40, 0, 131063, &p));
}


// ---- the second list (`tables`): the device jump table in every form

static uint64_t up4(uint64_t cells) { return (cells + 3) & ~3ull; }   // 128-byte lines
enum Bind { UNBOUND, BY_PITCH, BY_COLUMNS, BY_TABLES };

// Every column of one gadget out of ONE zeroed allocation, at fixed offsets (a table entry is an address difference:
// two allocations would make it differ from run to run), the columns of a table in descending address order: column 1
// lies below column 0, and the offsets are taken modulo 2^64
struct Carved {
    uint64_t *mem = nullptr;
    std::vector<void *> img, lk, cd, cs;
    hsw_region_binding b{};
    ~Carved() { std::free(mem); }
};

static void bind(hsw_gadget *g, Bind how, size_t K, uint64_t pitch, Carved *s) {
    hsw_region_binding need;
    CHECK(hsw_gadget_region_binding(g, &need) == HSW_OK);
    const uint64_t cols = need.columns_capacity, lk = need.lookup_capacity, rows = need.chip_rows_capacity;
    const uint64_t col_slot = up4(pitch), lk_slot = up4(lk), chip_col = up4(rows + 1), chip_slot = 2 * chip_col;
    const uint64_t o_lk = K * cols * col_slot, o_cd = o_lk + K * lk_slot, o_cs = o_cd + K * chip_slot, total = o_cs + K * chip_slot;
    s->mem = static_cast<uint64_t *>(std::aligned_alloc(128, total * 32));
    CHECK(s->mem);
    std::memset(s->mem, 0, total * 32);
    auto at = [&](uint64_t cell) { return static_cast<void *>(s->mem + 4 * cell); };
    for (size_t i = 0; i < K * cols; i++) s->img.push_back(at((K * cols - 1 - i) * col_slot));
    for (size_t i = 0; i < K; i++) s->lk.push_back(at(o_lk + (K - 1 - i) * lk_slot));
    for (size_t i = 0; i < 2 * K; i++) {
        s->cd.push_back(at(o_cd + (2 * K - 1 - i) * chip_col));
        s->cs.push_back(at(o_cs + (2 * K - 1 - i) * chip_col));
    }
    // the pitch model: ascending, a Context per slot
    s->b = hsw_region_binding{at(0), pitch, cols, cols * col_slot, at(o_lk), lk, lk_slot, at(o_cd), at(o_cs), rows + 1, rows, chip_slot};
    if (how == BY_PITCH) CHECK(hsw_gadget_bind_region(g, &s->b) == HSW_OK);
    if (how == BY_COLUMNS) CHECK(hsw_gadget_bind_columns(g, &s->b, s->img.data(), s->img.size()) == HSW_OK);
    if (how == BY_TABLES) {
        const hsw_column_tables t = {s->img.data(), s->img.size(), s->lk.data(), s->lk.size(), s->cd.data(), s->cs.data(), s->cd.size()};
        CHECK(hsw_gadget_bind_column_tables(g, &s->b, &t) == HSW_OK);
    }
}

static long long cells_between(const void *p, const void *from) {
    return (long long)((intptr_t)p - (intptr_t)from) / (long long)HSW_CELL_BYTES;
}

static void place_table(hsw_gadget *g) {
    CHECK(g->ctx->upload_place() == HSW_OK);
    const std::vector<uint64_t> &w = g->ctx->place_host;
    uint64_t sum = FNV0;
    for (uint64_t x : w) sum = fnv(sum, {x});
    std::printf("  place table: %zu words, sum %016llx\n   first", w.size(), (ull)sum);
    for (size_t i = 0; i < w.size() && i < 8; i++) std::printf(" %llu", (ull)w[i]);
    std::printf("\n   last");
    for (size_t i = w.size() > 8 ? w.size() - 8 : 0; i < w.size(); i++) std::printf(" %llu", (ull)w[i]);
    std::printf("\n");
}

// the binding in force: pointers as cells from the allocation the columns were carved from (unbound: from the view's)
static void binding(hsw_gadget *g, const Carved *s) {
    hsw_gadget_view v;
    hsw_region_binding b;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && hsw_gadget_region_binding(g, &b) == HSW_OK);
    std::printf("  binding: columns %+lld pitch %llu capacity %llu context_pitch %llu lookup %+lld capacity %llu pitch %llu "
                "dense %+lld spread %+lld stride %llu rows %llu context_pitch %llu\n",
                cells_between(b.d_columns, s ? s->mem : v.d_gate), (ull)b.column_pitch, (ull)b.columns_capacity, (ull)b.context_pitch,
                cells_between(b.d_lookup, s ? s->mem : v.d_lookup), (ull)b.lookup_capacity, (ull)b.lookup_pitch,
                cells_between(b.d_chip_dense, s ? s->mem : v.d_chip_dense), cells_between(b.d_chip_spread, s ? s->mem : v.d_chip_spread),
                (ull)b.chip_col_stride, (ull)b.chip_rows_capacity, (ull)b.chip_context_pitch);
}

// hsw_gadget_cell_address, in cells from d_gate, of the first and the last assigned cell and of the two cells around
// every jump of the map
static void addresses(hsw_gadget *g) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    auto address = [&](uint64_t cell) {
        void *p = nullptr;
        CHECK(hsw_gadget_cell_address(g, cell, &p) == HSW_OK);
        return cells_between(p, v.d_gate);
    };
    uint64_t pc = 0, pr = 0, sum = FNV0;
    int n_jumps = 0;
    std::printf("  address of cell 0: %+lld, of cell %llu: %+lld\n", address(0), (ull)(v.gate_cells - 1), address(v.gate_cells - 1));
    for (uint64_t i = 0; i < v.gate_cells; i++) {
        uint64_t c = 0, r = 0;
        CHECK(hsw_gadget_cell_position(g, i, &c, &r) == HSW_OK);
        if (i && !(c == pc && r == pr + 1)) {
            std::printf("  jump before cell %llu: (%llu,%llu) %+lld -> (%llu,%llu) %+lld\n", (ull)i, (ull)pc, (ull)pr, address(i - 1),
                        (ull)c, (ull)r, address(i));
            sum = fnv(sum, {i, (uint64_t)address(i - 1), (uint64_t)address(i)});
            n_jumps++;
        }
        if (i % 4099 == 0) sum = fnv(sum, {i, (uint64_t)address(i)});
        pc = c; pr = r;
    }
    std::printf("  %d jumps; their addresses and every 4099th cell's: sum %016llx\n", n_jumps, (ull)sum);
}

// contexts: what hsw_gadget_context_region counts (0: the gadget has no such regions); n: digests of the pass
static void table_case(const char *name, hsw_gadget *g, const std::vector<size_t> &sizes, size_t contexts, uint64_t rows, Bind how,
                       bool with_interlude) {
    std::printf("%s\n", name);
    const size_t K = contexts ? contexts : 1;
    uint64_t cols = 0;
    CHECK(hsw_gadget_set_origin(g, 1, 33, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, rows, &cols) == HSW_OK);
    if (with_interlude) {                                         // digest 1 starts two columns after digest 0's last, 11 caller lookups
        hsw_shape sh;
        hsw_frame_shape fs;
        uint64_t c = 0, r = 0;
        CHECK(hsw_engine_shape(E, &sh) == HSW_OK && hsw_frame_query(&sh, sizes[0], 1, &fs) == HSW_OK);
        CHECK(hsw_gadget_cell_position(g, fs.digest_cells, &c, &r) == HSW_OK);
        CHECK(hsw_gadget_set_digest_origin(g, 1, c + 2, 41, 5 + fs.digest_lookups + 11) == HSW_OK);
    }
    const uint64_t pitch = rows + 128;
    Carved s;
    if (how != UNBOUND) bind(g, how, K, pitch, &s);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    std::printf("  set_columns: %llu\n", (ull)cols);
    digest(g, sizes, 0, sizes.size());
    streams(g);
    place_table(g);
    binding(g, how != UNBOUND ? &s : nullptr);
    context_regions(g, contexts);
    addresses(g);
    // host buffers: a pitch-bound image or chip column is delivered where it lies, every other one as an unbound gadget's
    hsw_shape sh;
    CHECK(hsw_engine_shape(E, &sh) == HSW_OK);
    const uint64_t image = how == BY_PITCH ? (K - 1) * s.b.context_pitch + v.columns * pitch : K * v.columns * rows;
    const uint64_t stride = how == BY_TABLES ? hsw_chip_rows(&sh, 0, v.capacity_blocks) : v.chip_col_stride;   // (by table: chip_col_stride is 0)
    delivery_into(g, image, stride);
    hsw_gadget_destroy(g);
    for (uint64_t i = 0; s.mem && i < 4; i++) CHECK(s.mem[i] == 0);   // (launches do nothing here)
}

static void tables() {
    hsw_shape sh;
    CHECK(hsw_shape_query(8, 2, &sh) == HSW_OK);
    const uint64_t rows = 2 * (uint64_t)sh.gate_cells_per_block + 100;   // every second block crosses a column
    const std::vector<size_t> shared = {64, 128, 64}, image = {128, 64}, images(3, 128), group = {64, 128, 64, 128};
    hsw_gadget *g = nullptr;
    table_case("(a) shared context, an interlude, unbound", create(shared, 1, SHARED), shared, 0, rows, UNBOUND, true);
    table_case("(b) shared context, an interlude, bound by pitch", create(shared, 1, SHARED), shared, 0, rows, BY_PITCH, true);
    table_case("(c) plain image, columns by pointer table", create(image, 1, WHOLE), image, 0, rows, BY_COLUMNS, false);
    table_case("(d) context images, K = 3, image, lookup and chip columns by pointer table", create(images, 1, IMAGES), images, 3, rows,
               BY_TABLES, false);
    for (Bind how : {UNBOUND, BY_TABLES}) {
        CHECK(hsw_gadget_create_contexts(E, group.data(), 2, 2, 1, WHOLE, &g) == HSW_OK);
        table_case(how == UNBOUND ? "(e) Context group, K = 2, M = 2, unbound" : "(f) Context group, K = 2, M = 2, all columns by pointer table",
                   g, group, 2, rows, how, false);
    }
}

int main(int argc, char **argv) {
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &E) == HSW_OK);
    if (argc > 1 && std::strcmp(argv[1], "tables") == 0) {
        tables();
        hsw_engine_destroy(E);
        std::puts("place table dump done");
        return 0;
    }
    const uint64_t origins[6][4] = {{0, 17, 0, 0}, {2, 131000, 0, 5}, {1, 40000, 1, 1234}, {0, MAX_ROWS - 1, 0, 0},
                                    {3, 1000, 1, 9}, {4, 69990, 0, 3}};
    plain("block stream", 0, {128, 64, 192}, 0, false, nullptr, 0);
    plain("linear whole-digest stream", WHOLE, {128, 128}, 1, false, nullptr, 0);
    plain("linear whole-digest stream, independent contexts", WHOLE | HSW_GADGET_INDEPENDENT, {128, 64, 192}, 1, false, nullptr, 0);
    plain("linear whole-digest stream, origin (3,1000), zero cell loaded, 9 lookups queued", WHOLE, {128, 64, 192}, 1, false, origins[4], 0);
    plain("column image, origin (0,0)", WHOLE, {128, 128}, 1, false, nullptr, MAX_ROWS);
    plain("column image, origin (0,17)", WHOLE, {128, 128}, 1, false, origins[0], MAX_ROWS);
    plain("column image, origin (2,131000), 5 lookups queued", WHOLE, {128, 128}, 1, false, origins[1], MAX_ROWS);
    plain("column image, origin (1,40000), zero cell loaded, 1234 lookups queued", WHOLE, {128, 128}, 1, false, origins[2], MAX_ROWS);
    plain("column image, origin (0,last row)", WHOLE, {128, 128}, 1, false, origins[3], MAX_ROWS);
    plain("column image of 70000 rows, then origin (4,69990)", WHOLE, {64, 64, 64, 64, 64}, 0, true,
          origins[5], 70000);
    plain("one bench-circuit digest, 9 columns", WHOLE, {1024}, 1, false, nullptr, MAX_ROWS);
    plain("context images, K = 8, origin (2,131000), 5 lookups queued", IMAGES, std::vector<size_t>(8, 1024), 1, false, origins[1], MAX_ROWS);
    plain("context images, K = 9, origin (2,131000), 5 lookups queued", IMAGES, std::vector<size_t>(9, 1024), 1, false, origins[1], MAX_ROWS);
    plain("context images, K = 9, columns then origin (1,40000), zero cell loaded", IMAGES, std::vector<size_t>(9, 1024), 1, true, origins[2], MAX_ROWS);
    plain("context images, K = 8, linear", IMAGES, std::vector<size_t>(8, 1024), 1, false, origins[1], 0);
    for (int batch = 0; batch < 2; batch++) {
        interlude("rows_down", 0, 7, false, batch != 0);
        interlude("other_column", 2, 1000, false, batch != 0);
        interlude("last_row", 1, MAX_ROWS - 1, false, batch != 0);
        interlude("column 40 (the image grows)", 40, 17, true, batch != 0);
    }
    wide(4, false);
    wide(4, true);
    wide(9, false);
    wide(9, true);
    layout_changes();
    pack_plans();
    hsw_engine_destroy(E);
    std::puts("layout dump done");
    return 0;
}
