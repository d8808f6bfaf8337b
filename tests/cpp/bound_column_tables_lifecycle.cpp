// hsw_gadget_bind_column_tables on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in
// HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): every refusal (each leaves the
// geometry hsw_gadget_region_binding reports and the pointers hsw_gadget_streams reports as they were), bind / reset /
// rebind with other tables / unbind / destroy while bound, the reports of hsw_gadget_region_binding, hsw_gadget_streams
// and hsw_gadget_context_region, and hsw_gadget_download_region into host buffers laid out as an unbound twin's.  Every
// column -- image, lookup, chip dense, chip spread -- is a heap allocation of its own, exactly as long as the capacity
// the binding declares, so a copy past it is a sanitizer report; launches do nothing here, so at the end every caller
// cell must still hold the fill: the library itself never writes caller memory.
// Built and run by tests/test_bound_column_tables_host.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
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
static const size_t NCOLS = 2;

struct Alloc { uint64_t *p; uint64_t cells; };
static std::vector<Alloc> g_all;
static void *cells(uint64_t n) {
    uint64_t *p = static_cast<uint64_t *>(std::aligned_alloc(128, (n * 32 + 127) & ~127ull));
    CHECK(p);
    for (uint64_t i = 0; i < 4 * n; i++) p[i] = FILL;
    g_all.push_back(Alloc{p, n});
    return p;
}
static void all_untouched_then_free() {
    for (const Alloc &a : g_all) {
        for (uint64_t i = 0; i < 4 * a.cells; i++) CHECK(a.p[i] == FILL);
        std::free(a.p);
    }
    g_all.clear();
}

// every advice column an allocation of its own, allocated in reverse order; the pitch-model areas too (for the mixed cases)
struct Tables {
    std::vector<void *> img, lk, cd, cs;
    hsw_region_binding b{};
    hsw_column_tables t{};
};
static void make_tables(hsw_gadget *g, size_t K, Tables *s) {
    hsw_region_binding need;
    CHECK(hsw_gadget_region_binding(g, &need) == HSW_OK);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint64_t cols = v.columns, lk = need.lookup_capacity, rows = need.chip_rows_capacity;
    s->img.assign(K * cols, nullptr); s->lk.assign(K, nullptr); s->cd.assign(K * NCOLS, nullptr); s->cs.assign(K * NCOLS, nullptr);
    for (size_t i = K * NCOLS; i-- > 0;) { s->cs[i] = cells(rows); s->cd[i] = cells(rows); }
    for (size_t i = K; i-- > 0;) s->lk[i] = cells(lk);
    for (size_t i = K * cols; i-- > 0;) s->img[i] = cells(PITCH);
    // the pitch-model areas (ignored where a table is given)
    const uint64_t lkp = (lk + 3) & ~3ull, chip = (NCOLS * (rows + 1) + 3) & ~3ull;
    void *l = cells(K * lkp), *d = cells(K * chip), *sp = cells(K * chip);
    s->b = hsw_region_binding{nullptr, PITCH, cols, 0, l, lk, lkp, d, sp, rows + 1, rows, chip};
    s->t = hsw_column_tables{s->img.data(), s->img.size(), s->lk.data(), s->lk.size(), s->cd.data(), s->cs.data(), s->cd.size()};
}

static void digests(hsw_gadget *g, size_t n, std::vector<hsw_hash_result> *out = nullptr) {
    std::vector<uint8_t> msg(150, 7);
    std::vector<const uint8_t *> in(n, msg.data());
    std::vector<size_t> len(n), pre(n, 0);
    for (size_t i = 0; i < n; i++) len[i] = (i * 37) % 55;
    std::vector<hsw_hash_result> r(n);
    CHECK(hsw_gadget_digest_batch(g, n, in.data(), len.data(), pre.data(), r.data()) == HSW_OK);
    if (out) *out = r;
}

static bool same(const hsw_region_binding &a, const hsw_region_binding &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static hsw_gadget *single(hsw_engine *e) {
    const size_t sizes[2] = {128, 128};
    hsw_gadget *g = nullptr;
    CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 0, 17, 0, 0) == HSW_OK);
    return g;
}
static hsw_gadget *group(hsw_engine *e) {
    const size_t sizes[2] = {192, 64};
    hsw_gadget *g = nullptr;
    CHECK(hsw_gadget_create_contexts(e, sizes, 2, 3, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
    CHECK(hsw_gadget_set_origin(g, 1, 777, 0, 5) == HSW_OK);
    uint64_t n = 0;
    CHECK(hsw_gadget_set_columns(g, ROWS, &n) == HSW_OK);
    return g;
}

// Positions and results are the twin's; hsw_gadget_download_region touches, in host buffers laid out as the unbound
// twin's, exactly the cells the twin's own download touches (the twin delivers its zeroed memory, g the callers' fill).
// lk_tab / chip_tab: which families of g are bound by table (the others: host layout = the pitch model, checked elsewhere)
static void compare(hsw_gadget *twin, hsw_gadget *g, size_t n, bool lk_tab, bool chip_tab) {
    std::vector<hsw_hash_result> rt, rg;
    digests(twin, n, &rt);
    digests(g, n, &rg);
    for (size_t h = 0; h < n; h++) {
        CHECK(rt[h].prologue_cell == rg[h].prologue_cell && rt[h].block_cell == rg[h].block_cell && rt[h].end_cell == rg[h].end_cell);
        if (lk_tab)
            CHECK(rt[h].prologue_lookup == rg[h].prologue_lookup && rt[h].block_lookup == rg[h].block_lookup && rt[h].epilogue_lookup == rg[h].epilogue_lookup);
        hsw_result_cells ra, rb;
        CHECK(hsw_gadget_result_cells(twin, h, &ra) == HSW_OK && hsw_gadget_result_cells(g, h, &rb) == HSW_OK);
        CHECK(std::memcmp(&ra, &rb, sizeof ra) == 0);
    }
    hsw_gadget_view vt, vg;
    CHECK(hsw_gadget_streams(twin, &vt) == HSW_OK && hsw_gadget_streams(g, &vg) == HSW_OK);
    CHECK(vt.columns == vg.columns && vt.gate_cells == vg.gate_cells && vt.num_limb_sum == vg.num_limb_sum);
    CHECK(!lk_tab || vt.lookup_cells == vg.lookup_cells);       // (a pitch-bound lookup column counts its cells at the pitch)
    for (uint64_t cell = 0; cell < vg.gate_cells; cell += 997) {
        uint64_t ct = 0, rowt = 0, cg = 0, rowg = 0;
        CHECK(hsw_gadget_cell_position(twin, cell, &ct, &rowt) == HSW_OK && hsw_gadget_cell_position(g, cell, &cg, &rowg) == HSW_OK);
        CHECK(ct == cg && rowt == rowg);
    }
    const size_t lk_cells = (size_t)vt.lookup_capacity, chip_cells = NCOLS * (size_t)vt.chip_col_stride;
    std::vector<uint64_t> tl(4 * lk_cells, HOST), td(4 * chip_cells, HOST), ts(4 * chip_cells, HOST);
    std::vector<uint64_t> gl(4 * lk_cells, HOST), gd(4 * chip_cells, HOST), gs(4 * chip_cells, HOST);
    hsw_region_host dt = {nullptr, tl.data(), td.data(), ts.data()};
    hsw_region_host dg = {nullptr, lk_tab ? gl.data() : nullptr, chip_tab ? gd.data() : nullptr, chip_tab ? gs.data() : nullptr};
    CHECK(hsw_gadget_download_region(twin, &dt) == HSW_OK && hsw_gadget_download_region(g, &dg) == HSW_OK);
    size_t touched = 0;
    auto same_cells = [&](const std::vector<uint64_t> &t, const std::vector<uint64_t> &x) {
        for (size_t i = 0; i < t.size(); i++) {
            CHECK(x[i] == (t[i] != HOST ? FILL : HOST));
            touched += t[i] != HOST;
        }
    };
    if (lk_tab) same_cells(tl, gl);
    if (chip_tab) { same_cells(td, gd); same_cells(ts, gs); }
    CHECK(touched != 0);
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK);
    // the refusals of a gadget bound by pointer table
    uint64_t one[4];
    size_t got = 0;
    hsw_region_compact rc{};
    float ms[2];
    unsigned kept = 0;
    CHECK(hsw_gadget_download_region_distinct(g, one, 1, &got) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_replay_region(g, one, &dg, 1) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_download_region_compact(g, &rc) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_seek(g, 0) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_reset(twin) == HSW_OK);
    CHECK(hsw_gadget_place(g, 2, ms, &kept) == HSW_ERR_UNSUPPORTED);
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR >= 1 && sizeof(hsw_region_binding) == 96 && sizeof(hsw_column_tables) == 7 * sizeof(void *));
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- single image: every refusal, the reports, the lifecycle
        hsw_gadget *g = single(e), *twin = single(e);
        Tables s, s2;
        hsw_region_binding before, q;
        hsw_gadget_view v0, v1;
        // no column image yet
        void *dummy[1] = {nullptr};
        hsw_region_binding zero{};
        hsw_column_tables tz{dummy, 1, nullptr, 0, nullptr, nullptr, 0};
        CHECK(hsw_gadget_bind_column_tables(g, &zero, &tz) == HSW_ERR_UNSUPPORTED);
        uint64_t n = 0;
        CHECK(hsw_gadget_set_columns(g, ROWS, &n) == HSW_OK && n == 3);
        CHECK(hsw_gadget_set_columns(twin, ROWS, &n) == HSW_OK);
        make_tables(g, 1, &s);
        make_tables(g, 1, &s2);
        CHECK(hsw_gadget_region_binding(g, &before) == HSW_OK && hsw_gadget_streams(g, &v0) == HSW_OK);
        auto refused = [&](const hsw_region_binding &b, const hsw_column_tables &t, int want) {
            CHECK(hsw_gadget_bind_column_tables(g, &b, &t) == want);
            CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
            CHECK(hsw_gadget_streams(g, &v1) == HSW_OK && std::memcmp(&v0, &v1, sizeof v0) == 0);
        };
        auto refusals = [&]() {
            CHECK(hsw_gadget_bind_column_tables(nullptr, &s.b, &s.t) == HSW_ERR_INVALID_ARG);
            CHECK(hsw_gadget_bind_column_tables(g, nullptr, &s.t) == HSW_ERR_INVALID_ARG);
            CHECK(hsw_gadget_bind_column_tables(g, &s.b, nullptr) == HSW_ERR_INVALID_ARG);
            hsw_column_tables t = s.t;
            t.d_column_ptrs = nullptr;
            refused(s.b, t, HSW_ERR_INVALID_ARG);                                          // the image table is required
            t = s.t; t.n_column_ptrs -= 1;
            refused(s.b, t, HSW_ERR_INVALID_ARG);
            t = s.t; t.n_lookup_ptrs = 2;
            refused(s.b, t, HSW_ERR_INVALID_ARG);                                          // wrong n_lookup_ptrs
            t = s.t; t.d_lookup_ptrs = nullptr;
            refused(s.b, t, HSW_ERR_INVALID_ARG);                                          // ... a count without a table
            t = s.t; t.n_chip_ptrs = NCOLS + 1;
            refused(s.b, t, HSW_ERR_INVALID_ARG);                                          // wrong n_chip_ptrs
            t = s.t; t.n_chip_ptrs = 1;
            refused(s.b, t, HSW_ERR_INVALID_ARG);
            t = s.t; t.d_chip_spread_ptrs = nullptr;
            refused(s.b, t, HSW_ERR_INVALID_ARG);                                          // one chip family without the other
            t = s.t; t.d_chip_dense_ptrs = nullptr;
            refused(s.b, t, HSW_ERR_INVALID_ARG);
            // a null or misaligned entry, in each table
            std::vector<void *> *tabs[4] = {&s.img, &s.lk, &s.cd, &s.cs};
            for (std::vector<void *> *tab : tabs) {
                void *keep = tab->back();
                tab->back() = nullptr;
                refused(s.b, s.t, HSW_ERR_INVALID_ARG);
                tab->back() = static_cast<uint8_t *>(keep) + 32;
                refused(s.b, s.t, HSW_ERR_INVALID_ARG);
                tab->back() = keep;
            }
            // capacities below what the layout needs
            hsw_region_binding b = s.b;
            b.lookup_capacity -= 1;
            refused(b, s.t, HSW_ERR_TOO_LARGE);
            b = s.b; b.chip_rows_capacity -= 1;
            refused(b, s.t, HSW_ERR_TOO_LARGE);
            b = s.b; b.columns_capacity -= 1;
            t = s.t; t.n_column_ptrs -= 1;
            refused(b, t, HSW_ERR_TOO_LARGE);
            // a pitch-model family still obeys the pitch rules: lookup by table, chips by pitch with a null area
            b = s.b; b.d_chip_dense = nullptr;
            t = s.t; t.d_chip_dense_ptrs = t.d_chip_spread_ptrs = nullptr; t.n_chip_ptrs = 0;
            refused(b, t, HSW_ERR_INVALID_ARG);
        };
        refusals();                                                                        // ... on the library's own buffers
        // the ignored fields really are: garbage in them does not matter
        hsw_region_binding b = s.b;
        b.d_lookup = nullptr; b.lookup_pitch = 1; b.d_chip_dense = b.d_chip_spread = dummy; b.chip_col_stride = 1; b.chip_context_pitch = 7;
        CHECK(hsw_gadget_bind_column_tables(g, &b, &s.t) == HSW_OK);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK);
        CHECK(q.d_columns == s.img[0] && q.context_pitch == 0 && q.column_pitch == PITCH && q.columns_capacity == 3);
        CHECK(q.d_lookup == s.lk[0] && q.lookup_pitch == 0 && q.lookup_capacity == s.b.lookup_capacity);
        CHECK(q.d_chip_dense == s.cd[0] && q.d_chip_spread == s.cs[0] && q.chip_col_stride == 0 && q.chip_context_pitch == 0 &&
              q.chip_rows_capacity == s.b.chip_rows_capacity);
        CHECK(hsw_gadget_streams(g, &v0) == HSW_OK);
        CHECK(v0.d_gate == s.img[0] && v0.d_lookup == s.lk[0] && v0.d_chip_dense == s.cd[0] && v0.d_chip_spread == s.cs[0]);
        before = q;
        refusals();                                                                        // ... and on a previous binding
        compare(twin, g, 2, true, true);                                                   // (ends with a reset)
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));              // survives the reset
        CHECK(hsw_gadget_set_origin(g, 0, 40, 0, 0) == HSW_OK && hsw_gadget_set_origin(twin, 0, 40, 0, 0) == HSW_OK);   // a layout call that fits
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        CHECK(hsw_gadget_set_origin(g, 0, 40, 0, 1) == HSW_ERR_TOO_LARGE);                // one lookup cell more than an allocation holds
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        compare(twin, g, 2, true, true);
        // bind -> reset -> rebind with other tables
        digests(g, 1);
        CHECK(hsw_gadget_bind_column_tables(g, &s2.b, &s2.t) == HSW_ERR_INVALID_ARG);     // not after the first digest of a pass
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && same(q, before));
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_bind_column_tables(g, &s2.b, &s2.t) == HSW_OK);
        CHECK(hsw_gadget_streams(g, &v1) == HSW_OK && v1.d_gate == s2.img[0] && v1.d_lookup == s2.lk[0] && v1.d_chip_dense == s2.cd[0] && v1.d_chip_spread == s2.cs[0]);
        compare(twin, g, 2, true, true);
        // mixed: lookup by table and chips by pitch, then the reverse; then the image table alone through the new entry point
        hsw_column_tables t = s.t;
        t.d_chip_dense_ptrs = t.d_chip_spread_ptrs = nullptr; t.n_chip_ptrs = 0;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_OK);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_lookup == s.lk[0] && q.lookup_pitch == 0 && q.d_chip_dense == s.b.d_chip_dense &&
              q.chip_col_stride == s.b.chip_col_stride);
        compare(twin, g, 2, true, false);
        t = s.t; t.d_lookup_ptrs = nullptr; t.n_lookup_ptrs = 0;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_OK);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_lookup == s.b.d_lookup && q.d_chip_dense == s.cd[0] && q.chip_col_stride == 0);
        compare(twin, g, 2, false, true);
        t.d_chip_dense_ptrs = t.d_chip_spread_ptrs = nullptr; t.n_chip_ptrs = 0;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_OK);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_lookup == s.b.d_lookup && q.d_chip_dense == s.b.d_chip_dense && q.context_pitch == 0);
        // bind -> unbind: the library's own buffers again, every delivery works again
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &s.t) == HSW_OK);
        digests(g, 2);
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_ERR_INVALID_ARG);                  // not in the middle of a pass
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_bind_region(g, nullptr) == HSW_OK);
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.d_columns != s.img[0] && q.d_lookup != s.lk[0] && q.d_chip_dense != s.cd[0] &&
              q.column_pitch == ROWS && q.chip_col_stride != 0);
        digests(g, 2);
        size_t got = 0;
        hsw_region_tape tape;
        CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK);
        std::vector<uint64_t> distinct(tape.n_distinct * 4 + 4);
        CHECK(hsw_gadget_download_region_distinct(g, distinct.data(), tape.n_distinct, &got) == HSW_OK);
        hsw_gadget_destroy(g);
        hsw_gadget_destroy(twin);
    }
    {   // ---- K = 3 Context group: per-proof reports, a batch split inside a Context, destroy while bound
        hsw_gadget *g = group(e), *twin = group(e);
        Tables s;
        make_tables(g, 3, &s);
        hsw_column_tables t = s.t;
        t.n_lookup_ptrs = 1;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_ERR_INVALID_ARG);         // K entries, not 1
        t = s.t; t.n_chip_ptrs = NCOLS;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_ERR_INVALID_ARG);         // K * ncols entries
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &s.t) == HSW_OK);
        hsw_context_region reg;
        for (size_t c = 0; c < 3; c++) {
            CHECK(hsw_gadget_context_region(g, c, &reg) == HSW_OK);
            CHECK(reg.d_image == s.img[c * s.b.columns_capacity] && reg.d_lookup == s.lk[c] && reg.d_chip_dense == s.cd[c * NCOLS] &&
                  reg.d_chip_spread == s.cs[c * NCOLS]);
        }
        hsw_region_binding q;
        CHECK(hsw_gadget_region_binding(g, &q) == HSW_OK && q.context_pitch == 0 && q.lookup_pitch == 0 && q.chip_col_stride == 0 &&
              q.chip_context_pitch == 0 && q.d_lookup == s.lk[0] && q.d_chip_spread == s.cs[0]);
        compare(twin, g, 6, true, true);
        digests(g, 3);                                                                     // ends inside Context 1
        digests(g, 3);
        digests(twin, 6);
        hsw_verify_report rep;
        CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_reset(twin) == HSW_OK);
        // mixed, K > 1: the pitch-model family at its pitches
        t = s.t; t.d_lookup_ptrs = nullptr; t.n_lookup_ptrs = 0;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_OK);
        for (size_t c = 0; c < 3; c++) {
            CHECK(hsw_gadget_context_region(g, c, &reg) == HSW_OK);
            CHECK(reg.d_lookup == static_cast<uint8_t *>(s.b.d_lookup) + c * s.b.lookup_pitch * 32 && reg.d_chip_dense == s.cd[c * NCOLS]);
        }
        compare(twin, g, 6, false, true);
        t = s.t; t.d_chip_dense_ptrs = t.d_chip_spread_ptrs = nullptr; t.n_chip_ptrs = 0;
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &t) == HSW_OK);
        for (size_t c = 0; c < 3; c++) {
            CHECK(hsw_gadget_context_region(g, c, &reg) == HSW_OK);
            CHECK(reg.d_lookup == s.lk[c] && reg.d_chip_dense == static_cast<uint8_t *>(s.b.d_chip_dense) + c * s.b.chip_context_pitch * 32);
        }
        compare(twin, g, 6, true, false);
        CHECK(hsw_gadget_bind_column_tables(g, &s.b, &s.t) == HSW_OK);
        digests(g, 6);
        hsw_gadget_destroy(g);                                                             // destroy while bound, mid-pass
        hsw_gadget_destroy(twin);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0);
    all_untouched_then_free();
    std::printf("bound column tables lifecycle ok\n");
    return 0;
}
