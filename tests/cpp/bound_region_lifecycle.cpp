// hsw_gadget_bind_region on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP
// runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): the argument rules (every refusal
// leaves the geometry hsw_gadget_region_binding reports as it was), bind / reset / layout calls that fit and that do
// not / unbind / bind again / destroy for the four kinds of layout, and every position of a bound gadget against an
// unbound twin: the same (FlexGate column, row), the image cell at column * column_pitch + row (+ c * context_pitch).
// The caller's memory is exactly as large as the binding declares, so a copy past it is a sanitizer report.
// Built and run by tests/test_bound_region_host.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_gadget.hpp"   // (hsw.h + the layout: image_cell is not public)

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

static const uint32_t WHOLE = HSW_GADGET_WHOLE_DIGEST;
static const uint64_t FILL = 0x5a5a5a5a5a5a5a5aull, HOST = 0xa5a5a5a5a5a5a5a5ull;
static uint64_t up4(uint64_t cells) { return (cells + 3) & ~3ull; }   // 128-byte lines

// One slab per proof: [columns | lookup | dense | spread], every area on a line boundary, every cell = FILL
struct Slabs {
    uint64_t *mem = nullptr;
    uint64_t cells = 0;
    hsw_region_binding b{};
    ~Slabs() { std::free(mem); }
    uint64_t *cell(uint64_t i) const { return mem + 4 * i; }
};

// the needs of `g` as it stands (library-owned geometry), `extra_cols` columns and `extra_lk` lookup cells to spare
static void make_slabs(hsw_gadget *g, size_t K, uint64_t pitch, uint64_t extra_cols, uint64_t extra_lk, Slabs *s) {
    hsw_region_binding need;
    CHECK(hsw_gadget_region_binding(g, &need) == HSW_OK);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint64_t cols = v.columns + extra_cols, lk = need.lookup_capacity + extra_lk, rows = need.chip_rows_capacity;
    const uint64_t o_lk = up4(cols * pitch), o_cd = o_lk + up4(lk), o_cs = o_cd + up4(2 * rows + 2), slab = o_cs + up4(2 * rows + 2);
    s->cells = K * slab;
    s->mem = static_cast<uint64_t *>(std::aligned_alloc(128, s->cells * 32));
    CHECK(s->mem);
    for (uint64_t i = 0; i < 4 * s->cells; i++) s->mem[i] = FILL;
    s->b = hsw_region_binding{s->cell(0), pitch, cols, slab, s->cell(o_lk), lk, slab, s->cell(o_cd), s->cell(o_cs), rows + 1, rows, slab};
}

static void digests(hsw_gadget *g, size_t n) {
    std::vector<uint8_t> msg(150, 7);
    std::vector<const uint8_t *> in(n, msg.data());
    std::vector<size_t> len(n), pre(n, 0);
    for (size_t i = 0; i < n; i++) len[i] = (i * 37) % 55;
    std::vector<hsw_hash_result> r(n);
    CHECK(hsw_gadget_digest_batch(g, n, in.data(), len.data(), pre.data(), r.data()) == HSW_OK);
}

static bool same(const hsw_region_binding &a, const hsw_region_binding &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// Every gate-stream cell of a bound gadget against its unbound twin, then the deliveries into a host buffer of the
// slabs' geometry: exactly the image cells of the stream are touched, by the download and by the replay alike
static void compare_positions(hsw_gadget *twin, hsw_gadget *g, const Slabs &s, size_t K, size_t n_digests) {
    hsw_gadget_view vt, vg;
    CHECK(hsw_gadget_streams(twin, &vt) == HSW_OK && hsw_gadget_streams(g, &vg) == HSW_OK);
    CHECK(vt.columns == vg.columns && vt.max_rows == vg.max_rows && vt.gate_capacity == vg.gate_capacity);
    CHECK(vg.d_gate == s.b.d_columns && vg.d_lookup == s.b.d_lookup && vg.d_chip_dense == s.b.d_chip_dense && vg.chip_col_stride == s.b.chip_col_stride);
    hsw_region_binding q;
    CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, s.b));
    const uint64_t C = vg.gate_capacity / K;                      // stream cells of one Context
    digests(twin, n_digests);
    digests(g, n_digests);
    CHECK(hsw_gadget_streams(g, &vg) == HSW_OK && vg.gate_cells == vg.gate_capacity);
    std::vector<uint64_t> host(4 * s.cells, HOST), host2(4 * s.cells, HOST);
    const uint64_t o_lk = (uint64_t *)s.b.d_lookup - s.mem, o_cd = (uint64_t *)s.b.d_chip_dense - s.mem, o_cs = (uint64_t *)s.b.d_chip_spread - s.mem;
    hsw_region_host dst = {host.data(), host.data() + o_lk, host.data() + o_cd, host.data() + o_cs};
    CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
    uint64_t touched = 0;
    for (uint64_t cell = 0; cell < vg.gate_cells; cell++) {
        uint64_t ct = 0, rt = 0, cg = 0, rg = 0;
        CHECK(hsw_gadget_cell_position(twin, cell, &ct, &rt) == HSW_OK && hsw_gadget_cell_position(g, cell, &cg, &rg) == HSW_OK);
        CHECK(ct == cg && rt == rg && rg < vg.max_rows);
        const uint64_t at = g->ctx->layout.image_cell(cell);
        const uint64_t want = (cg - vg.origin_column) * s.b.column_pitch + rg + (K > 1 ? (cell / C) * s.b.context_pitch : 0);
        CHECK(at == want);
        CHECK(host[4 * at] == FILL);                              // delivered (the stub's launches write nothing: the slab's fill)
        host[4 * at] = HOST;
        touched++;
    }
    CHECK(touched == vg.gate_cells);
    // nothing else of the image area was touched, in any proof: rows >= max_rows, rows above the origin, interludes, tails
    for (size_t c = 0; c < K; c++)
        for (uint64_t i = 0; i < s.b.columns_capacity * s.b.column_pitch; i++) CHECK(host[4 * (c * s.b.context_pitch + i)] == HOST);
    // lookup column and chip rows: inside every proof's own capacity, the caller's queued entries untouched
    hsw_context_region reg{};
    if (K > 1) CHECK(hsw_gadget_context_region(g, 0, &reg) == HSW_OK);
    const uint64_t Lp = K > 1 ? reg.lookup_cells : vg.lookup_cells;
    const uint64_t rows = vg.num_limb_sum / 2 / K;
    for (size_t c = 0; c < K; c++) {
        const uint64_t *lk = host.data() + o_lk + 4 * c * s.b.lookup_pitch;
        for (uint64_t i = 0; i < vg.origin_lookups; i++) CHECK(lk[4 * i] == HOST);
        CHECK(lk[4 * vg.origin_lookups] == FILL && lk[4 * (Lp - 1)] == FILL);
        for (uint64_t i = Lp; i < s.b.lookup_capacity; i++) CHECK(lk[4 * i] == HOST);
        for (int k = 0; k < 2; k++) {
            const uint64_t *cd = host.data() + o_cd + 4 * (c * s.b.chip_context_pitch + k * s.b.chip_col_stride);
            const uint64_t *cs = host.data() + o_cs + 4 * (c * s.b.chip_context_pitch + k * s.b.chip_col_stride);
            CHECK(cd[0] == FILL && cd[4 * (rows - 1)] == FILL && cd[4 * rows] == HOST);
            CHECK(cs[0] == FILL && cs[4 * (rows - 1)] == FILL && cs[4 * rows] == HOST);
        }
    }
    if (K > 1) {
        CHECK(hsw_gadget_context_region(g, K - 1, &reg) == HSW_OK && reg.assigned == 1);
        CHECK(reg.d_image == (uint8_t *)s.b.d_columns + (K - 1) * s.b.context_pitch * 32);
        CHECK(reg.d_lookup == (uint8_t *)s.b.d_lookup + (K - 1) * s.b.lookup_pitch * 32);
        CHECK(reg.d_chip_dense == (uint8_t *)s.b.d_chip_dense + (K - 1) * s.b.chip_context_pitch * 32);
        CHECK(reg.d_chip_spread == (uint8_t *)s.b.d_chip_spread + (K - 1) * s.b.chip_context_pitch * 32);
        CHECK(reg.chip_col_stride == s.b.chip_col_stride && reg.chip_rows == rows);
    }
    // the distinct delivery replayed into a sentinel-filled buffer of the same geometry writes exactly the same cells
    CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK && tape.gate_cells == vg.gate_cells);
    std::vector<uint64_t> distinct(tape.n_distinct * 4 + 4);
    size_t n = 0;
    CHECK(hsw_gadget_download_region_distinct(g, distinct.data(), tape.n_distinct, &n) == HSW_OK && n == tape.n_distinct);
    hsw_region_host dst2 = {host2.data(), host2.data() + o_lk, host2.data() + o_cd, host2.data() + o_cs};
    CHECK(hsw_gadget_replay_region(g, distinct.data(), &dst2, 3) == HSW_OK);
    for (uint64_t i = 0; i < s.cells; i++) CHECK((host[4 * i] == HOST) == (host2[4 * i] == HOST));
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
    // the refusals of a bound gadget
    hsw_region_compact cdst = {};
    CHECK(hsw_gadget_download_region_compact(g, &cdst) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_seek(g, 0) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_place(g, 2, nullptr, nullptr) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, s.b));         // survives the reset
    // the slab itself: no call wrote, zeroed or filled a cell of it (launches do nothing here)
    for (uint64_t i = 0; i < 4 * s.cells; i++) CHECK(s.mem[i] == FILL);
}

enum Kind { SINGLE, SHARED, IMAGES, GROUP };
static hsw_gadget *create(hsw_engine *e, Kind kind, const size_t *sizes, size_t n, size_t K, uint64_t col, uint64_t row, uint64_t rows,
                          bool interlude) {
    hsw_gadget *g = nullptr;
    if (kind == GROUP) CHECK(hsw_gadget_create_contexts(e, sizes, n, K, 1, WHOLE, &g) == HSW_OK);
    else if (kind == IMAGES) {
        std::vector<size_t> all(K, sizes[0]);
        CHECK(hsw_gadget_create_ex(e, all.data(), K, 1, WHOLE | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g) == HSW_OK);
    } else CHECK(hsw_gadget_create_ex(e, sizes, n, 1, WHOLE | (kind == SHARED ? HSW_GADGET_SHARED_CONTEXT : 0u), &g) == HSW_OK);
    uint64_t columns = 0;
    CHECK(hsw_gadget_set_origin(g, col, row, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, rows, &columns) == HSW_OK);
    if (interlude) {                                              // digest 1 starts three columns after digest 0's last, 11 caller lookups
        hsw_shape sh;
        hsw_frame_shape fs;
        CHECK(hsw_engine_shape(e, &sh) == HSW_OK && hsw_frame_query(&sh, sizes[0], 1, &fs) == HSW_OK);
        uint64_t c = 0, r = 0;
        CHECK(hsw_gadget_cell_position(g, fs.digest_cells, &c, &r) == HSW_OK);
        CHECK(hsw_gadget_set_digest_origin(g, 1, c + 3, 41, 5 + fs.digest_lookups + 11) == HSW_OK);
    }
    return g;
}

// a bound gadget of `kind` and its unbound twin at both pitches
static void positions(hsw_engine *e, Kind kind, const size_t *sizes, size_t n, size_t K, uint64_t col, uint64_t row, uint64_t rows,
                      bool interlude) {
    const uint64_t pitches[2] = {rows + 3, 1ull << 17};
    for (uint64_t pitch : pitches) {
        hsw_gadget *twin = create(e, kind, sizes, n, K, col, row, rows, interlude), *g = create(e, kind, sizes, n, K, col, row, rows, interlude);
        Slabs s;
        make_slabs(g, K, pitch, 1, 7, &s);
        CHECK(hsw_gadget_bind_region(g, &s.b) == HSW_OK);
        compare_positions(twin, g, s, K, kind == IMAGES ? K : n * K);
        hsw_gadget_destroy(twin);
        hsw_gadget_destroy(g);
    }
}

int main() {
    hsw_engine *e = nullptr, *edef = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    CHECK(hsw_abi_version() == 3);
    const uint64_t ROWS = 70001;                                  // odd
    size_t sizes[2] = {128, 64};
    hsw_gadget *g = nullptr;

    // ---- which gadgets
    CHECK(hsw_gadget_bind_region(nullptr, nullptr) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, WHOLE, &g) == HSW_OK);
    hsw_region_binding junk{};
    CHECK(hsw_gadget_bind_region(g, &junk) == HSW_ERR_UNSUPPORTED);                 // linear: no hsw_gadget_set_columns
    CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_ERR_UNSUPPORTED);
    hsw_gadget_destroy(g);
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_DEFAULT, &edef) == HSW_OK);
    CHECK(hsw_gadget_create_ex(edef, sizes, 2, 1, 0, &g) == HSW_OK);
    CHECK(hsw_gadget_bind_region(g, &junk) == HSW_ERR_UNSUPPORTED);                 // block streams
    hsw_gadget_destroy(g);
    hsw_engine_destroy(edef);
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, WHOLE | HSW_GADGET_INDEPENDENT, &g) == HSW_OK);
    CHECK(hsw_gadget_bind_region(g, &junk) == HSW_ERR_UNSUPPORTED);                 // K linear regions
    hsw_gadget_destroy(g);

    // ---- the argument rules, on K = 3 context images: every refusal leaves the geometry in force
    {
        const size_t K = 3;
        g = create(e, IMAGES, sizes, 1, K, 2, 17, ROWS, false);
        hsw_region_binding owned, q;
        CHECK(hsw_gadget_region_binding(g, &owned) == HSW_OK);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        CHECK(owned.d_columns == v.d_gate && owned.column_pitch == ROWS && owned.columns_capacity == v.columns && owned.context_pitch == v.columns * ROWS);
        CHECK(owned.lookup_pitch == owned.lookup_capacity && owned.chip_context_pitch == owned.chip_rows_capacity && owned.chip_col_stride == v.chip_col_stride);
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_OK);                        // unbound already: nothing to do
        Slabs s;
        make_slabs(g, K, ROWS + 3, 0, 0, &s);
        for (int round = 0; round < 2; round++) {                                   // library-owned, then bound
            const hsw_region_binding before = round ? s.b : owned;
            auto refused = [&](hsw_region_binding b, int want) {
                CHECK(hsw_gadget_bind_region(g, &b) == want);
                CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
            };
            hsw_region_binding b = s.b;
            b.d_columns = nullptr; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.d_lookup = nullptr; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.d_chip_dense = nullptr; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.d_chip_spread = nullptr; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.d_columns = (uint8_t *)b.d_columns + 64; refused(b, HSW_ERR_INVALID_ARG);          // not 128-byte aligned
            b = s.b; b.d_lookup = (uint8_t *)b.d_lookup + 32; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.d_chip_spread = (uint8_t *)b.d_chip_spread + 96; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.column_pitch = ROWS - 1; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.context_pitch = b.columns_capacity * b.column_pitch - 1; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.lookup_pitch = b.lookup_capacity - 1; refused(b, HSW_ERR_INVALID_ARG);
            b = s.b; b.columns_capacity -= 1; refused(b, HSW_ERR_TOO_LARGE);
            b = s.b; b.lookup_capacity -= 1; refused(b, HSW_ERR_TOO_LARGE);
            b = s.b; b.chip_rows_capacity -= 1; refused(b, HSW_ERR_TOO_LARGE);
            if (round == 0) CHECK(hsw_gadget_bind_region(g, &s.b) == HSW_OK);       // odd pitch: accepted
        }
        // after the first digest of a pass: refused, bound or not; allowed again after the reset
        digests(g, 1);
        CHECK(hsw_gadget_bind_region(g, &s.b) == HSW_ERR_INVALID_ARG && hsw_gadget_bind_region(g, nullptr) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_bind_region(g, &s.b) == HSW_OK);
        // ---- lifecycle: layout calls that fit, one that does not, unbind, bind again, destroy while bound
        CHECK(hsw_gadget_set_origin(g, 4, 100, 0, 5) == HSW_OK);                     // fits: the same columns, the same Lp
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, s.b));
        uint64_t col = 0, row = 0, columns = 0;
        CHECK(hsw_gadget_cell_position(g, 0, &col, &row) == HSW_OK && col == 4 && row == 100);
        CHECK(hsw_gadget_set_origin(g, 4, 100, 0, 6) == HSW_ERR_TOO_LARGE);          // one lookup cell more than declared
        CHECK(hsw_gadget_set_columns(g, ROWS + 4, &columns) == HSW_ERR_TOO_LARGE);   // a column higher than the pitch
        CHECK(hsw_gadget_set_origin(g, 4, ROWS - 1, 0, 5) == HSW_ERR_TOO_LARGE);     // a column more than declared
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.max_rows == ROWS && v.origin_lookups == 5 && v.d_gate == s.b.d_columns);
        CHECK(hsw_gadget_cell_position(g, 0, &col, &row) == HSW_OK && col == 4 && row == 100);
        CHECK(hsw_gadget_set_columns(g, ROWS + 2, &columns) == HSW_OK && columns <= s.b.columns_capacity);   // fits
        CHECK(hsw_gadget_set_columns(g, ROWS, &columns) == HSW_OK);
        digests(g, K);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_OK);                         // library-owned, zeroed buffers again
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_columns != s.b.d_columns && q.column_pitch == ROWS && q.context_pitch == q.columns_capacity * ROWS);
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.d_gate == q.d_columns && ((uint64_t *)v.d_gate)[0] == 0);
        digests(g, K);
        std::vector<uint64_t> gate(K * q.context_pitch * 4), look(K * q.lookup_pitch * 4), cd(2 * q.chip_col_stride * 4), cs(2 * q.chip_col_stride * 4);
        hsw_region_host dst = {gate.data(), look.data(), cd.data(), cs.data()};
        CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);                        // exact-size buffers of the library's geometry
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_bind_region(g, &s.b) == HSW_OK);
        digests(g, 2);
        hsw_gadget_destroy(g);                                                       // bound, a pass half issued: the slab stays the caller's
        for (uint64_t i = 0; i < 4 * s.cells; i++) CHECK(s.mem[i] == FILL);
    }

    // ---- a shared context that would have grown its image
    {
        g = create(e, SHARED, sizes, 2, 1, 1, 777, ROWS, false);
        Slabs s;
        make_slabs(g, 1, ROWS + 3, 0, 20, &s);
        CHECK(hsw_gadget_bind_region(g, &s.b) == HSW_OK);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        const uint64_t cols = v.columns;
        hsw_shape sh;
        hsw_frame_shape fs;
        CHECK(hsw_engine_shape(e, &sh) == HSW_OK && hsw_frame_query(&sh, sizes[0], 1, &fs) == HSW_OK);
        uint64_t c = 0, r = 0, c2 = 0, r2 = 0;
        CHECK(hsw_gadget_cell_position(g, fs.digest_cells + 1, &c, &r) == HSW_OK);
        CHECK(hsw_gadget_set_digest_origin(g, 1, c + 2, 0, 5 + fs.digest_lookups) == HSW_ERR_TOO_LARGE);     // two columns more
        CHECK(hsw_gadget_set_digest_origin(g, 1, c, r + 9, 5 + fs.digest_lookups + 21) == HSW_ERR_TOO_LARGE); // lookups past the capacity
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns == cols && v.d_gate == s.b.d_columns);
        CHECK(hsw_gadget_cell_position(g, fs.digest_cells + 1, &c2, &r2) == HSW_OK && c2 == c && r2 == r);
        CHECK(hsw_gadget_set_digest_origin(g, 1, c, r + 9, 5 + fs.digest_lookups + 20) == HSW_OK);           // fits
        CHECK(hsw_gadget_cell_position(g, fs.digest_cells + 1, &c2, &r2) == HSW_OK && c2 == c && r2 == r + 9);
        digests(g, 2);
        hsw_gadget_destroy(g);
        for (uint64_t i = 0; i < 4 * s.cells; i++) CHECK(s.mem[i] == FILL);
    }

    // ---- positions: the four kinds of layout, two pitches each
    size_t test_circuit[2] = {128, 128}, bench[1] = {1024}, big[2] = {1024, 1024};
    positions(e, SINGLE, test_circuit, 2, 1, 0, 17, ROWS, false);                    // TestCircuit shape
    positions(e, SINGLE, bench, 1, 1, 2, 131000, (1u << 17) - 9, false);             // bench-circuit shape
    positions(e, SHARED, big, 2, 1, 1, 777, (1u << 17) - 9, true);                   // > 17 columns, an interlude that spans columns
    positions(e, IMAGES, bench, 1, 3, 2, 131000, (1u << 17) - 9, false);
    positions(e, GROUP, sizes, 2, 3, 1, 777, ROWS, true);                            // M = 2
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::puts("bound region lifecycle ok");
    return 0;
}
