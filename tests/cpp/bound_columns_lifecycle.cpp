// hsw_gadget_bind_columns on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP
// runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): the argument rules (every refusal
// leaves the geometry hsw_gadget_region_binding reports as it was), bind / reset / layout calls that fit and that do
// not / unbind, the five refusals, and every stream cell's position against an unbound twin for a 3-column single image
// and a K = 3 Context group with an interlude.  Every column is a heap allocation of its own, exactly column_pitch
// cells long, so a copy past it is a sanitizer report.  Built and run by tests/test_bound_columns_host.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hsw.h"

extern "C" {
size_t hip_stub_live_device_allocations();
size_t hip_stub_live_pinned_allocations();
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static const uint64_t FILL = 0x5a5a5a5a5a5a5a5aull, HOST = 0xa5a5a5a5a5a5a5a5ull;
static const uint64_t ROWS = (1u << 17) - 9, PITCH = ROWS + 12;

static void *cells(uint64_t n) {
    uint64_t *p = static_cast<uint64_t *>(std::aligned_alloc(128, (n * 32 + 127) & ~127ull));
    CHECK(p);
    for (uint64_t i = 0; i < 4 * n; i++) p[i] = FILL;
    return p;
}

// K x cols columns, each an allocation of its own (allocated in reverse column order), + pitch-model lookup / chip areas
struct Columns {
    std::vector<void *> ptrs, all;
    hsw_region_binding b{};
    ~Columns() { for (void *p : all) std::free(p); }
};
static void make_columns(hsw_gadget *g, size_t K, uint64_t extra_cols, Columns *s) {
    hsw_region_binding need;
    CHECK(hsw_gadget_region_binding(g, &need) == HSW_OK);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint64_t cols = v.columns + extra_cols, lk = need.lookup_capacity, rows = need.chip_rows_capacity, chip = 2 * (rows + 1);
    s->ptrs.assign(K * cols, nullptr);
    for (size_t i = K * cols; i-- > 0;) { s->ptrs[i] = cells(PITCH); s->all.push_back(s->ptrs[i]); }
    void *l = cells(K * ((lk + 3) & ~3ull)), *cd = cells(K * ((chip + 3) & ~3ull)), *cs = cells(K * ((chip + 3) & ~3ull));
    s->all.push_back(l); s->all.push_back(cd); s->all.push_back(cs);
    s->b = hsw_region_binding{nullptr, PITCH, cols, 0, l, lk, (lk + 3) & ~3ull, cd, cs, rows + 1, rows, (chip + 3) & ~3ull};
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

static hsw_gadget *single(hsw_engine *e) {
    const size_t sizes[2] = {128, 128};
    hsw_gadget *g = nullptr;
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 0, 17, 0, 0) == HSW_OK);
    return g;
}
static hsw_gadget *group(hsw_engine *e, uint64_t decl_col) {
    const size_t sizes[2] = {192, 64};
    hsw_gadget *g = nullptr;
    CHECK(hsw_gadget_create_contexts(e, sizes, 2, 3, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 1, 777, 0, 5) == HSW_OK);
    uint64_t n = 0;
    CHECK(hsw_gadget_set_columns(g, ROWS, &n) == HSW_OK);
    if (decl_col) CHECK(hsw_gadget_set_digest_origin(g, 1, decl_col, 41, 100000) == HSW_OK);
    return g;
}

// every stream cell's position equals the twin's; the download touches exactly those cells of the unbound-layout buffer
static void compare(hsw_gadget *twin, hsw_gadget *g, const Columns &s, size_t K, size_t n) {
    hsw_gadget_view vt, vg;
    digests(twin, n);
    digests(g, n);
    CHECK(hsw_gadget_streams(twin, &vt) == HSW_OK && hsw_gadget_streams(g, &vg) == HSW_OK);
    CHECK(vt.columns == vg.columns && vt.gate_cells == vg.gate_cells && vg.gate_cells == vg.gate_capacity && vg.d_gate == s.ptrs[0]);
    const uint64_t C = vg.gate_capacity / K;
    std::vector<uint64_t> host(4 * K * vg.columns * ROWS, HOST);
    hsw_region_host dst = {host.data(), nullptr, nullptr, nullptr};
    CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
    for (uint64_t cell = 0; cell < vg.gate_cells; cell++) {
        uint64_t ct = 0, rt = 0, cg = 0, rg = 0;
        CHECK(hsw_gadget_cell_position(twin, cell, &ct, &rt) == HSW_OK && hsw_gadget_cell_position(g, cell, &cg, &rg) == HSW_OK);
        CHECK(ct == cg && rt == rg && rg < ROWS);
        const uint64_t at = ((cell / C) * vg.columns + (cg - vg.origin_column)) * ROWS + rg;
        CHECK(host[4 * at] == FILL);
        host[4 * at] = HOST;
    }
    for (uint64_t i = 0; i < host.size(); i += 4) CHECK(host[i] == HOST);
    hsw_hash_result a, b;
    hsw_result_cells ra, rb;
    for (size_t h = 0; h < n; h++) {
        CHECK(hsw_gadget_result_cells(twin, h, &ra) == HSW_OK && hsw_gadget_result_cells(g, h, &rb) == HSW_OK);
        CHECK(std::memcmp(&ra, &rb, sizeof ra) == 0);
    }
    (void)a; (void)b;
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK);
    // the five refusals
    uint64_t one[4];
    size_t got = 0;
    hsw_region_compact rc{};
    float ms[2];
    unsigned kept = 0;
    CHECK(hsw_gadget_download_region_distinct(g, one, 1, &got) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_replay_region(g, one, &dst, 1) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_download_region_compact(g, &rc) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_seek(g, 0) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_place(g, 2, ms, &kept) == HSW_ERR_UNSUPPORTED);
}

int main() {
    CHECK(hsw_abi_version() == 3 && sizeof(hsw_region_binding) == 96);
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- single image, 3 columns: argument rules, lifecycle, positions
        hsw_gadget *g = single(e), *twin = single(e);
        Columns s;
        hsw_region_binding before, q;
        // no column image yet
        void *dummy[1] = {nullptr};
        hsw_region_binding zero{};
        CHECK(hsw_gadget_bind_columns(g, &zero, dummy, 1) == HSW_ERR_UNSUPPORTED);
        uint64_t n = 0;
        CHECK(hsw_gadget_set_columns(g, ROWS, &n) == HSW_OK && n == 3);
        CHECK(hsw_gadget_set_columns(twin, ROWS, &n) == HSW_OK);
        make_columns(g, 1, 1, &s);                               // 4 columns reserved
        CHECK(hsw_gadget_region_binding(g, &before) == HSW_OK);
        auto refused = [&](const hsw_region_binding &b, void *const *p, size_t np, int want) {
            CHECK(hsw_gadget_bind_columns(g, &b, p, np) == want);
            CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        };
        CHECK(hsw_gadget_bind_columns(nullptr, &s.b, s.ptrs.data(), s.ptrs.size()) == HSW_ERR_INVALID_ARG);
        refused(s.b, nullptr, s.ptrs.size(), HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_bind_columns(g, nullptr, s.ptrs.data(), s.ptrs.size()) == HSW_ERR_INVALID_ARG);
        refused(s.b, s.ptrs.data(), s.ptrs.size() - 1, HSW_ERR_INVALID_ARG);          // n_ptrs != K * columns_capacity
        std::vector<void *> p = s.ptrs;
        p[2] = nullptr;
        refused(s.b, p.data(), p.size(), HSW_ERR_INVALID_ARG);                         // a null entry
        p[2] = (uint8_t *)s.ptrs[2] + 32;
        refused(s.b, p.data(), p.size(), HSW_ERR_INVALID_ARG);                         // not on a 128-byte line
        hsw_region_binding b = s.b;
        b.d_lookup = (uint8_t *)s.b.d_lookup + 64;
        refused(b, s.ptrs.data(), s.ptrs.size(), HSW_ERR_INVALID_ARG);
        b = s.b; b.d_chip_dense = nullptr;
        refused(b, s.ptrs.data(), s.ptrs.size(), HSW_ERR_INVALID_ARG);
        b = s.b; b.column_pitch = ROWS - 1;
        refused(b, s.ptrs.data(), s.ptrs.size(), HSW_ERR_INVALID_ARG);
        b = s.b; b.column_pitch = (1ull << 24) + 1;
        refused(b, s.ptrs.data(), s.ptrs.size(), HSW_ERR_INVALID_ARG);
        b = s.b; b.columns_capacity = 2;
        refused(b, s.ptrs.data(), 2, HSW_ERR_TOO_LARGE);                               // fewer columns than the layout
        b = s.b; b.lookup_capacity -= 1;
        refused(b, s.ptrs.data(), s.ptrs.size(), HSW_ERR_TOO_LARGE);
        b = s.b; b.chip_rows_capacity -= 1;
        refused(b, s.ptrs.data(), s.ptrs.size(), HSW_ERR_TOO_LARGE);
        // bind: d_columns reported as proof 0 column 0, context_pitch 0
        CHECK(hsw_gadget_bind_columns(g, &s.b, s.ptrs.data(), s.ptrs.size()) == HSW_OK);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_columns == s.ptrs[0] && q.context_pitch == 0 && q.column_pitch == PITCH && q.columns_capacity == 4);
        before = q;
        p[2] = nullptr;
        refused(s.b, p.data(), p.size(), HSW_ERR_INVALID_ARG);                         // a refusal keeps the previous binding
        compare(twin, g, s, 1, 2);                                                     // (ends with a reset)
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));          // survives the reset
        CHECK(hsw_gadget_set_origin(g, 0, 40, 0, 0) == HSW_OK);                        // a layout call that fits
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        hsw_gadget_view v0, v1;
        CHECK(hsw_gadget_streams(g, &v0) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, PITCH + 1, &n) == HSW_ERR_TOO_LARGE);          // taller than a column allocation
        const int rc_cols = hsw_gadget_set_columns(g, 69500, &n);                       // more columns than reserved
        if (rc_cols != HSW_ERR_TOO_LARGE) std::fprintf(stderr, "set_columns(69500) = %d, columns %llu\n", rc_cols, (unsigned long long)n);
        CHECK(rc_cols == HSW_ERR_TOO_LARGE);
        CHECK(hsw_gadget_streams(g, &v1) == HSW_OK && std::memcmp(&v0, &v1, sizeof v0) == 0);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        digests(g, 2);
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_ERR_INVALID_ARG);              // not in the middle of a pass
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_OK);                           // unbind
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_columns != s.ptrs[0] && q.column_pitch == ROWS);
        digests(g, 2);
        size_t got = 0;
        hsw_region_tape tape;
        CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK);
        std::vector<uint64_t> distinct(tape.n_distinct * 4 + 4);
        CHECK(hsw_gadget_download_region_distinct(g, distinct.data(), tape.n_distinct, &got) == HSW_OK);   // works again
        for (void *c : s.ptrs) CHECK(*static_cast<uint64_t *>(c) == FILL);
        hsw_gadget_destroy(g);
        hsw_gadget_destroy(twin);
    }
    {   // ---- K = 3 Context group with an interlude
        hsw_gadget *probe = group(e, 0);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(probe, &v) == HSW_OK);
        const uint64_t decl_col = v.origin_column + v.columns + 1;
        hsw_gadget_destroy(probe);
        hsw_gadget *g = group(e, decl_col), *twin = group(e, decl_col);
        Columns s;
        make_columns(g, 3, 0, &s);
        CHECK(hsw_gadget_bind_columns(g, &s.b, s.ptrs.data(), s.ptrs.size() - 1) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_bind_columns(g, &s.b, s.ptrs.data(), s.ptrs.size()) == HSW_OK);
        hsw_context_region reg;
        for (size_t c = 0; c < 3; c++)
            CHECK(hsw_gadget_context_region(g, c, &reg) == HSW_OK && reg.d_image == s.ptrs[c * s.b.columns_capacity]);
        hsw_region_binding before, q;
        CHECK(hsw_gadget_region_binding(g, &before) == HSW_OK && before.context_pitch == 0);
        compare(twin, g, s, 3, 6);
        CHECK(hsw_gadget_set_digest_origin(g, 1, decl_col + 2, 41, 100000) == HSW_ERR_TOO_LARGE);   // needs more columns
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_OK);
        hsw_gadget_destroy(g);
        hsw_gadget_destroy(twin);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0);
    std::printf("bound columns lifecycle ok\n");
    return 0;
}
