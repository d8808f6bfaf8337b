// hsw_gadget_lookup_runs / hsw_gadget_lookup_multiplicities on the host side under AddressSanitizer + UBSan +
// LeakSanitizer, against the stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing).
// Every case prints what the library's public geometry calls say about the pass -- DIG lines (a committed digest: its
// Context, where its own lookup entries start in the Context's column, its size), CALLER lines (lookup entries that are
// the caller's), CTX lines (where a Context's lookup column and chip columns start on the device: from hsw_gadget_streams,
// hsw_gadget_context_region or the program's own pointer tables) -- and the run list (RUN lines).
// tests/test_lookup_counts_host.py checks every run against a model of its own.  Checked here: the cap / NULL rules,
// the refusals, no launch for an empty list, the launches of a count, no leak of the run table.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hsw.h"

extern "C" {
size_t hip_stub_live_device_allocations();
size_t hip_stub_live_pinned_allocations();
int hip_stub_launches();
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static const uint64_t ROWS = (1u << 17) - 9;
static const uint32_t WHOLE = HSW_GADGET_WHOLE_DIGEST;
typedef unsigned long long ull;

static std::vector<void *> g_mine;
static void *cells(uint64_t n) {
    void *p = std::aligned_alloc(128, (size_t)((n * 32 + 127) & ~127ull));
    CHECK(p);
    std::memset(p, 0x5a, (size_t)(n * 32));
    g_mine.push_back(p);
    return p;
}
static void free_mine() { for (void *p : g_mine) std::free(p); g_mine.clear(); }

static std::vector<hsw_hash_result> digests(hsw_gadget *g, size_t n) {
    std::vector<uint8_t> msg(150, 7);
    std::vector<const uint8_t *> in(n, msg.data());
    std::vector<size_t> len(n), pre(n, 0);
    for (size_t i = 0; i < n; i++) len[i] = (i * 37) % 55;
    std::vector<hsw_hash_result> r(n);
    CHECK(hsw_gadget_digest_batch(g, n, in.data(), len.data(), pre.data(), r.data()) == HSW_OK);
    return r;
}

// the list, with the cap / NULL rules on the way
static std::vector<hsw_lookup_run> dump(hsw_gadget *g, const char *name) {
    size_t n = ~(size_t)0;
    CHECK(hsw_gadget_lookup_runs(g, nullptr, 0, &n) == HSW_OK && n != ~(size_t)0);
    CHECK(hsw_gadget_lookup_runs(g, nullptr, 0, nullptr) == HSW_OK);
    std::vector<hsw_lookup_run> r(n + 1);
    std::memset(r.data(), 0xee, r.size() * sizeof r[0]);
    CHECK(hsw_gadget_lookup_runs(g, r.data(), n, nullptr) == HSW_OK);
    CHECK(reinterpret_cast<const uint8_t *>(&r[n])[0] == 0xee);              // nothing past n
    if (n) {                                                                 // a cap that is too small: *n still set, nothing written
        std::vector<hsw_lookup_run> u(n);
        std::memset(u.data(), 0xee, u.size() * sizeof u[0]);
        size_t n2 = 0;
        CHECK(hsw_gadget_lookup_runs(g, u.data(), n - 1, &n2) == HSW_ERR_TOO_LARGE && n2 == n);
        for (size_t i = 0; i < n * sizeof u[0]; i++) CHECK(reinterpret_cast<const uint8_t *>(u.data())[i] == 0xee);
    }
    r.resize(n);
    for (size_t i = 0; i < n; i++) {
        const hsw_lookup_run &x = r[i];
        CHECK(x.n > 0 && x.d_cells && (x.table == HSW_LOOKUP_SPREAD) == (x.d_spread != nullptr));
        std::printf("RUN %llu %u %u %llu %llu %llu %llu\n", (ull)x.context, x.table, x.column, (ull)x.first, (ull)x.n,
                    (ull)(uintptr_t)x.d_cells, (ull)(uintptr_t)x.d_spread);
    }
    std::printf("CASE %s %zu\n", name, n);
    return r;
}

// DIG context first_entry n_blocks max_variable_byte_size is_input_range_check
static void print_digests(hsw_gadget *g, const std::vector<hsw_hash_result> &r, const size_t *sizes, size_t M, uint64_t lookup_pitch) {
    (void)g;
    for (size_t d = 0; d < r.size(); d++) {
        const uint64_t cx = lookup_pitch ? d / M : 0;
        std::printf("DIG %llu %llu %llu %zu 1\n", (ull)cx, (ull)(r[d].prologue_lookup - cx * lookup_pitch), (ull)r[d].n_blocks, sizes[d % M]);
    }
}
static void print_ctx(uint64_t cx, const void *lookup, const void *const *dense, const void *const *spread, size_t ncols) {
    std::printf("CTX %llu %llu", (ull)cx, (ull)(uintptr_t)lookup);
    for (size_t k = 0; k < ncols; k++) std::printf(" %llu", (ull)(uintptr_t)dense[k]);
    for (size_t k = 0; k < ncols; k++) std::printf(" %llu", (ull)(uintptr_t)spread[k]);
    std::printf("\n");
}
// a Context's columns from the public geometry: hsw_gadget_streams (one Context) or hsw_gadget_context_region
static void print_ctx_public(hsw_gadget *g, uint64_t cx, bool multi) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    const uint8_t *lk = static_cast<const uint8_t *>(v.d_lookup), *cd = static_cast<const uint8_t *>(v.d_chip_dense), *cs = static_cast<const uint8_t *>(v.d_chip_spread);
    uint64_t stride = v.chip_col_stride;
    if (multi) {
        hsw_context_region r;
        CHECK(hsw_gadget_context_region(g, (size_t)cx, &r) == HSW_OK);
        lk = static_cast<const uint8_t *>(r.d_lookup); cd = static_cast<const uint8_t *>(r.d_chip_dense); cs = static_cast<const uint8_t *>(r.d_chip_spread);
        stride = r.chip_col_stride;
    }
    const void *d[2] = {cd, cd + stride * 32}, *s[2] = {cs, cs + stride * 32};
    print_ctx(cx, lk, d, s, 2);
}

static hsw_gadget *group(hsw_engine *e, const size_t *sizes, hsw_frame_shape *fs0) {
    hsw_gadget *g = nullptr;
    CHECK(hsw_gadget_create_contexts(e, sizes, 2, 2, 1, WHOLE, &g) == HSW_OK);
    uint64_t columns = 0, c = 0, r = 0;
    CHECK(hsw_gadget_set_origin(g, 1, 777, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, ROWS, &columns) == HSW_OK);
    hsw_shape sh;
    CHECK(hsw_engine_shape(e, &sh) == HSW_OK && hsw_frame_query(&sh, sizes[0], 1, fs0) == HSW_OK);
    CHECK(hsw_gadget_cell_position(g, fs0->digest_cells, &c, &r) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, c + 1, 41, 5 + fs0->digest_lookups + 11) == HSW_OK);     // an interlude of 11 caller lookups
    return g;
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_lookup_run) == 48 && sizeof(hsw_lookup_counts) == 40 && sizeof(hsw_lookup_report) == 56);
    hsw_lookup_report rep;
    uint32_t *counters = static_cast<uint32_t *>(std::calloc(3 * 70000, 4));
    CHECK(counters);
    {   // ---- a linear block-stream gadget, 3 chip columns, 2 blocks: SPREAD only, columns of unequal length
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        CHECK(dump(g, "fresh").empty());
        digests(g, 1);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        const uint8_t *cd = static_cast<const uint8_t *>(v.d_chip_dense), *cs = static_cast<const uint8_t *>(v.d_chip_spread);
        const void *d[3] = {cd, cd + v.chip_col_stride * 32, cd + 2 * v.chip_col_stride * 32};
        const void *s[3] = {cs, cs + v.chip_col_stride * 32, cs + 2 * v.chip_col_stride * 32};
        print_ctx(0, nullptr, d, s, 3);
        std::printf("LIMBS 0 %llu 3\n", (ull)v.num_limb_sum);
        CHECK(dump(g, "block_stream").size() == 3);
        // no lookup column: the range table is refused, the spread table alone is counted
        hsw_lookup_counts both{counters, counters, 0, 0, 0, 0}, sp{nullptr, counters, 0, 0, 0, 0};
        const int l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_multiplicities(g, &both, &rep) == HSW_ERR_UNSUPPORTED && hip_stub_launches() == l0);
        CHECK(hsw_gadget_lookup_multiplicities(g, &sp, &rep) == HSW_OK && rep.spread_entries == v.num_limb_sum && rep.range_entries == 0);
        CHECK(hip_stub_launches() == l0 + 2);                                // the zeroing and the count
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    hsw_shape sh;
    CHECK(hsw_engine_shape(e, &sh) == HSW_OK);
    {   // ---- a whole digest at an origin with lookups_queued = 5; the argument rules; after hsw_gadget_reset
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        uint64_t columns = 0;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, WHOLE, &g) == HSW_OK);
        CHECK(hsw_gadget_set_origin(g, 2, 131000, 0, 5) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, ROWS, &columns) == HSW_OK);
        hsw_lookup_counts both{counters, counters + 70000, 0, 0, 0, 0};
        int l0 = hip_stub_launches();
        std::memset(&rep, 0xee, sizeof rep);
        CHECK(hsw_gadget_lookup_multiplicities(g, &both, &rep) == HSW_OK);   // nothing digested: an empty list
        CHECK(rep.range_entries == 0 && rep.spread_entries == 0 && rep.not_in_table == 0 && rep.kernel_ms == 0.f && hip_stub_launches() == l0);
        const std::vector<hsw_hash_result> r = digests(g, 1);
        print_digests(g, r, sizes, 1, 0);
        std::printf("CALLER 0 0 5\n");
        print_ctx_public(g, 0, false);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        std::printf("LIMBS 0 %llu 2\n", (ull)v.num_limb_sum);
        const std::vector<hsw_lookup_run> runs = dump(g, "origin");
        CHECK(runs.size() == 3 && runs[0].table == HSW_LOOKUP_RANGE && runs[0].first == 5);
        // refusals, each before any launch
        l0 = hip_stub_launches();
        hsw_lookup_counts bad = both;
        CHECK(hsw_gadget_lookup_multiplicities(nullptr, &both, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_lookup_multiplicities(g, nullptr, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_lookup_multiplicities(g, &both, nullptr) == HSW_ERR_INVALID_ARG);
        bad.d_range = bad.d_spread = nullptr;
        CHECK(hsw_gadget_lookup_multiplicities(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = both; bad.range_pitch = 65535;
        CHECK(hsw_gadget_lookup_multiplicities(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = both; bad.spread_pitch = 255;
        CHECK(hsw_gadget_lookup_multiplicities(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = both; bad.d_spread = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(counters) + 2);
        CHECK(hsw_gadget_lookup_multiplicities(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = both; bad.flags = 2;
        CHECK(hsw_gadget_lookup_multiplicities(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hip_stub_launches() == l0 && hip_stub_live_device_allocations() > 0);
        // a count: two tables zeroed, one count launch; accumulating: the count launch alone; one table: its runs alone
        const size_t live = hip_stub_live_device_allocations();
        CHECK(hsw_gadget_lookup_multiplicities(g, &both, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
        CHECK(rep.range_entries == runs[0].n && rep.spread_entries == runs[1].n + runs[2].n && rep.not_in_table == 0);
        CHECK(hip_stub_live_device_allocations() == live + 1);               // the run table
        both.flags = HSW_LOOKUP_ACCUMULATE; both.range_pitch = 70000;
        CHECK(hsw_gadget_lookup_multiplicities(g, &both, &rep) == HSW_OK && hip_stub_launches() == l0 + 4);
        CHECK(hip_stub_live_device_allocations() == live + 1);
        hsw_lookup_counts only{counters, nullptr, 0, 0, 0, 0};
        CHECK(hsw_gadget_lookup_multiplicities(g, &only, &rep) == HSW_OK && rep.spread_entries == 0 && rep.range_entries == runs[0].n);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(dump(g, "after_reset").empty());
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_multiplicities(g, &both, &rep) == HSW_OK && rep.range_entries == 0 && hip_stub_launches() == l0);
        hsw_gadget_destroy(g);                                               // frees the run table: the leak check at the end
    }
    {   // ---- a shared context, an interlude that queues 11 caller lookups between its two digests
        const size_t sizes[2] = {64, 128};
        hsw_gadget *g = nullptr;
        uint64_t columns = 0, c = 0, r = 0;
        CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, WHOLE | HSW_GADGET_SHARED_CONTEXT, &g) == HSW_OK);
        CHECK(hsw_gadget_set_origin(g, 1, 777, 0, 5) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, ROWS, &columns) == HSW_OK);
        hsw_frame_shape fs;
        CHECK(hsw_frame_query(&sh, sizes[0], 1, &fs) == HSW_OK);
        CHECK(hsw_gadget_cell_position(g, fs.digest_cells, &c, &r) == HSW_OK);
        CHECK(hsw_gadget_set_digest_origin(g, 1, c + 1, 41, 5 + fs.digest_lookups + 11) == HSW_OK);
        const std::vector<hsw_hash_result> rs = digests(g, 2);
        print_digests(g, rs, sizes, 2, 0);
        std::printf("CALLER 0 0 5\nCALLER 0 %llu %llu\n", (ull)(5 + fs.digest_lookups), (ull)(5 + fs.digest_lookups + 11));
        print_ctx_public(g, 0, false);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        std::printf("LIMBS 0 %llu 2\n", (ull)v.num_limb_sum);
        CHECK(dump(g, "shared_interlude").size() == 4);
        hsw_gadget_destroy(g);
    }
    {   // ---- K = 3 context images, only 2 proofs digested
        const size_t sizes[3] = {64, 64, 64};
        hsw_gadget *g = nullptr;
        uint64_t columns = 0;
        CHECK(hsw_gadget_create_ex(e, sizes, 3, 1, WHOLE | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g) == HSW_OK);
        CHECK(hsw_gadget_set_origin(g, 2, 131000, 0, 5) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, ROWS, &columns) == HSW_OK);
        const std::vector<hsw_hash_result> rs = digests(g, 2);
        hsw_context_region r0;
        CHECK(hsw_gadget_context_region(g, 0, &r0) == HSW_OK);
        print_digests(g, rs, sizes, 1, r0.lookup_cells);
        for (uint64_t cx = 0; cx < 3; cx++) { std::printf("CALLER %llu 0 5\n", (ull)cx); print_ctx_public(g, cx, true); }
        for (uint64_t cx = 0; cx < 2; cx++) std::printf("LIMBS %llu %llu 2\n", (ull)cx, (ull)sh.limb_calls_per_block);
        const std::vector<hsw_lookup_run> runs = dump(g, "images_2_of_3");
        CHECK(runs.size() == 6 && runs.back().context == 1);
        hsw_gadget_destroy(g);
    }
    for (int tables = 0; tables < 2; tables++) {
        // ---- a Context group, M = 2 and K = 2: bound by pitch (pitches larger than needed), then by pointer tables in
        //      shuffled address order
        const size_t sizes[2] = {64, 128};
        hsw_frame_shape fs0;
        hsw_gadget *g = group(e, sizes, &fs0);
        hsw_region_binding need;
        hsw_gadget_view v;
        CHECK(hsw_gadget_region_binding(g, &need) == HSW_OK && hsw_gadget_streams(g, &v) == HSW_OK);
        const uint64_t K = 2, cols = v.columns, lk = need.lookup_capacity, rows = need.chip_rows_capacity, PITCH = ROWS + 12;
        const uint64_t lkp = lk + 7, chip_pitch = rows + 9, stride = K * chip_pitch + 3;
        std::vector<void *> img(K * cols), lks(K), cd(K * 2), cs(K * 2);
        hsw_region_binding b{};
        if (!tables) {
            b = hsw_region_binding{cells(K * cols * PITCH), PITCH, cols, cols * PITCH, cells(K * lkp), lk, lkp,
                                   cells(2 * stride), cells(2 * stride), stride, rows, chip_pitch};
            CHECK(hsw_gadget_bind_region(g, &b) == HSW_OK);
        } else {
            // one slab per family, the entries dealt from its far end and interleaved: addresses descend and alternate
            //  (every entry on a 128-byte line, as the binding asks)
            const uint64_t ip = (PITCH + 8) & ~3ull, lp = (lk + 8) & ~3ull, rp = (rows + 8) & ~3ull;
            uint8_t *si = static_cast<uint8_t *>(cells(K * cols * ip)), *sl = static_cast<uint8_t *>(cells(K * lp));
            uint8_t *sd = static_cast<uint8_t *>(cells(2 * K * rp)), *ss = static_cast<uint8_t *>(cells(2 * K * rp));
            for (uint64_t i = 0; i < K * cols; i++) img[i] = si + (K * cols - 1 - i) * ip * 32;
            for (uint64_t i = 0; i < K; i++) lks[i] = sl + (K - 1 - i) * lp * 32;
            const uint64_t order[4] = {2, 0, 3, 1};
            for (uint64_t i = 0; i < 2 * K; i++) { cd[i] = sd + order[i] * rp * 32; cs[i] = ss + order[3 - i] * rp * 32; }
            b = hsw_region_binding{nullptr, PITCH, cols, 0, nullptr, lk, 0, nullptr, nullptr, rows, rows, 0};
            hsw_column_tables t{img.data(), img.size(), lks.data(), lks.size(), cd.data(), cs.data(), cd.size()};
            CHECK(hsw_gadget_bind_column_tables(g, &b, &t) == HSW_OK);
        }
        const std::vector<hsw_hash_result> rs = digests(g, 4);
        hsw_context_region r0, r1;
        CHECK(hsw_gadget_context_region(g, 0, &r0) == HSW_OK && hsw_gadget_context_region(g, 1, &r1) == HSW_OK);
        // (positions stay an unbound gadget's by table; a pitch-bound column counts its cells at the pitch)
        print_digests(g, rs, sizes, 2, tables ? r0.lookup_cells : lkp);
        for (uint64_t cx = 0; cx < K; cx++) {
            std::printf("CALLER %llu 0 5\nCALLER %llu %llu %llu\n", (ull)cx, (ull)cx, (ull)(5 + fs0.digest_lookups), (ull)(5 + fs0.digest_lookups + 11));
            std::printf("LIMBS %llu %llu 2\n", (ull)cx, (ull)(3 * sh.limb_calls_per_block));
            if (tables) {
                const void *d[2] = {cd[cx * 2], cd[cx * 2 + 1]}, *s[2] = {cs[cx * 2], cs[cx * 2 + 1]};
                print_ctx(cx, lks[cx], d, s, 2);
            } else {                                          // the binding's own arithmetic
                const uint8_t *bd = static_cast<const uint8_t *>(b.d_chip_dense), *bs = static_cast<const uint8_t *>(b.d_chip_spread);
                const void *d[2] = {bd + cx * chip_pitch * 32, bd + (stride + cx * chip_pitch) * 32};
                const void *s[2] = {bs + cx * chip_pitch * 32, bs + (stride + cx * chip_pitch) * 32};
                print_ctx(cx, static_cast<const uint8_t *>(b.d_lookup) + cx * lkp * 32, d, s, 2);
                CHECK((cx ? r1 : r0).d_lookup == static_cast<const uint8_t *>(b.d_lookup) + cx * lkp * 32 && (cx ? r1 : r0).d_chip_dense == d[0]);
            }
        }
        CHECK(dump(g, tables ? "group_tables" : "group_pitch").size() == 2 * (2 + 2));
        hsw_gadget_destroy(g);                                // while bound
        free_mine();
    }
    hsw_engine_destroy(e);
    std::free(counters);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0);
    std::printf("lookup counts lifecycle ok\n");
    return 0;
}
