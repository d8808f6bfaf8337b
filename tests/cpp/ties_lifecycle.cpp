// hsw_gadget_ties / hsw_gadget_cell_address / hsw_gadget_verify_ties / hsw_gadget_verify_equal on the host side under
// AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP runtime of hip_stub.cpp ("device" memory = heap
// memory, launches do nothing).  Every case prints what it handed to the device-fed calls (MSG lines) and the ties the
// library derived from it (TIE lines): tests/test_ties_host.py replays the MSG lines through a model of its own and
// compares.  Checked here: the counts, the cap / NULL rules, the refusals, the cells of a tie against
// hsw_gadget_result_cells, hsw_gadget_cell_address against position arithmetic and against the caller's own column
// pointers, no launch for a refused or empty check, no leak.  Inputs and destinations are poisoned heap blocks: the
// host may use their addresses and nothing else.
#include <hip/hip_runtime.h>
#include <sanitizer/asan_interface.h>

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

struct Arena {
    std::vector<std::pair<void *, size_t>> blocks;
    uint8_t *get(size_t bytes) {
        void *p = std::malloc(bytes ? bytes : 1);
        CHECK(p);
        ASAN_POISON_MEMORY_REGION(p, bytes ? bytes : 1);
        blocks.emplace_back(p, bytes ? bytes : 1);
        return static_cast<uint8_t *>(p);
    }
    ~Arena() {
        for (auto &b : blocks) { ASAN_UNPOISON_MEMORY_REGION(b.first, b.second); std::free(b.first); }
    }
};

struct Msg { const void *src; size_t len; uint32_t level; void *dst; size_t pre; };

static size_t g_hash = 0, g_call = 0;      // of the pass being printed

// kind: 0 = hsw_gadget_digest_levels_device, 1 = hsw_gadget_digest_batch_device (no levels, no destinations),
// 2 = hsw_gadget_digest_batch (host-fed: zeros of the same lengths)
static void call(hsw_gadget *g, const std::vector<Msg> &m, int kind = 0) {
    std::vector<const void *> p;
    std::vector<size_t> len, pre;
    std::vector<uint32_t> lv;
    std::vector<void *> dst;
    for (const Msg &x : m) { p.push_back(x.src); len.push_back(x.len); pre.push_back(x.pre); lv.push_back(x.level); dst.push_back(x.dst); }
    std::vector<hsw_hash_result> r(m.size());
    if (kind == 0) CHECK(hsw_gadget_digest_levels_device(g, m.size(), p.data(), len.data(), pre.data(), lv.data(), dst.data(), r.data()) == HSW_OK);
    if (kind == 1) CHECK(hsw_gadget_digest_batch_device(g, m.size(), p.data(), len.data(), pre.data(), r.data()) == HSW_OK);
    if (kind == 2) {
        std::vector<uint8_t> zeros(256, 0);
        std::vector<const uint8_t *> hp(m.size(), zeros.data());
        CHECK(hsw_gadget_digest_batch(g, m.size(), hp.data(), len.data(), pre.data(), r.data()) == HSW_OK);
    }
    for (const Msg &x : m)
        std::printf("MSG %zu %zu %u %d %llu %zu %zu %llu\n", g_hash++, g_call, kind == 0 ? x.level : 0u, kind != 2 ? 1 : 0,
                    (unsigned long long)(uintptr_t)x.src, x.len, x.pre, (unsigned long long)(kind == 0 ? (uintptr_t)x.dst : 0));
    g_call++;
}

static std::vector<hsw_cell_tie> dump(hsw_gadget *g, const char *name, size_t want, uint64_t want_prefix = 0) {
    size_t n = ~(size_t)0;
    uint64_t pre = ~0ull;
    CHECK(hsw_gadget_ties(g, nullptr, 0, &n, &pre) == HSW_OK);
    CHECK(n == want && pre == want_prefix);
    std::vector<hsw_cell_tie> t(n + 1);
    std::memset(t.data(), 0xee, t.size() * sizeof t[0]);
    CHECK(hsw_gadget_ties(g, t.data(), n, nullptr, nullptr) == HSW_OK);
    if (n) {                                                 // a cap that is too small: *n still set, nothing written
        std::vector<hsw_cell_tie> u(n);
        std::memset(u.data(), 0xee, u.size() * sizeof u[0]);
        size_t n2 = 0;
        CHECK(hsw_gadget_ties(g, u.data(), n - 1, &n2, nullptr) == HSW_ERR_TOO_LARGE && n2 == n);
        for (size_t i = 0; i < n * sizeof u[0]; i++) CHECK(reinterpret_cast<const uint8_t *>(u.data())[i] == 0xee);
    }
    CHECK(reinterpret_cast<const uint8_t *>(&t[n])[0] == 0xee);     // nothing past n
    t.resize(n);
    for (size_t i = 0; i < n; i++) {
        hsw_result_cells src, dst;
        CHECK(hsw_gadget_result_cells(g, (size_t)t[i].src_hash, &src) == HSW_OK && hsw_gadget_result_cells(g, (size_t)t[i].dst_hash, &dst) == HSW_OK);
        CHECK(t[i].src_byte < 32 && t[i].dst_byte < dst.n_input_bytes);
        CHECK(t[i].src_cell == src.output_byte_cells[t[i].src_byte] && t[i].dst_cell == dst.input_bytes_cell0 + t[i].dst_byte);
        if (i) CHECK(t[i - 1].dst_hash < t[i].dst_hash || (t[i - 1].dst_hash == t[i].dst_hash && t[i - 1].dst_byte < t[i].dst_byte));
        std::printf("TIE %llu %llu %u %u\n", (unsigned long long)t[i].src_hash, (unsigned long long)t[i].dst_hash, t[i].src_byte, t[i].dst_byte);
    }
    std::printf("CASE %s %zu %llu\n", name, n, (unsigned long long)pre);
    // the recorded ties through the pair check: one launch, every tie compared (the stub's kernels find nothing)
    const int l0 = hip_stub_launches();
    hsw_tie_report rep;
    std::memset(&rep, 0xee, sizeof rep);
    CHECK(hsw_gadget_verify_ties(g, &rep) == HSW_OK);
    CHECK(rep.checks == n && rep.violations == 0 && hip_stub_launches() - l0 == (n ? 1 : 0));
    return t;
}

static void next_pass(hsw_gadget *g) {
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    g_hash = g_call = 0;
}

static const uint64_t ROWS = (1u << 17) - 9;

// sizes {128} * 7, whole digest, a column image
static void cases(hsw_engine *e, hsw_gadget *g) {
    Arena a;
    uint8_t *nodes = a.get(32 * 7 + 64);
    auto leaf = [&](size_t len, void *dst) { return Msg{a.get(len), len, 0, dst, 0}; };
    // ---- a 2-leaf tree
    call(g, {leaf(10, nodes), leaf(119, nodes + 32), Msg{nodes, 64, 1, nodes + 64, 0}});
    std::vector<hsw_cell_tie> t = dump(g, "tree2", 64);
    CHECK(t[0].src_hash == 0 && t[0].dst_hash == 2 && t[63].src_hash == 1 && t[63].src_byte == 31 && t[63].dst_byte == 63);
    // ---- ties gone after hsw_gadget_reset
    next_pass(g);
    dump(g, "after_reset", 0);
    // ---- a 4-leaf tree
    std::vector<Msg> tree = {leaf(0, nodes), leaf(55, nodes + 32), leaf(64, nodes + 64), leaf(119, nodes + 96),
                             Msg{nodes, 64, 1, nodes + 128, 0}, Msg{nodes + 64, 64, 1, nodes + 160, 0}, Msg{nodes + 128, 64, 2, nodes + 192, 0}};
    tree[0].src = nullptr;
    call(g, tree);
    dump(g, "tree4", 192);
    // ---- the same tree, its messages shuffled and its levels with gaps
    next_pass(g);
    std::vector<Msg> sh = {tree[6], tree[0], tree[4], tree[1], tree[5], tree[2], tree[3]};
    for (Msg &m : sh) m.level = 10 * m.level + 7;
    call(g, sh);
    t = dump(g, "shuffled", 192);
    CHECK(t[0].dst_hash == 0 && t[0].src_hash == 2);         // the root is digest 0, its left child digest 2
    // ---- partial overlaps at odd alignments: bytes 5..31 of one child and 0..9 of the next
    next_pass(g);
    call(g, {leaf(3, nodes + 3), leaf(4, nodes + 35), Msg{nodes + 8, 37, 1, nullptr, 0}});
    t = dump(g, "partial", 37);
    CHECK(t[0].src_byte == 5 && t[0].dst_byte == 0 && t[26].src_byte == 31 && t[27].src_hash == 1 && t[27].src_byte == 0 && t[36].src_byte == 9);
    // ---- a precomputed prefix of 64 bytes over a 96-byte message reading three digests
    next_pass(g);
    call(g, {leaf(1, nodes), leaf(2, nodes + 32), leaf(3, nodes + 64), Msg{nodes, 96, 1, nullptr, 64}});
    t = dump(g, "prefix", 32, 64);
    CHECK(t[0].src_hash == 2 && t[0].src_byte == 0 && t[0].dst_byte == 0 && t[31].dst_byte == 31);
    // ---- a parent aimed at a slot nobody writes
    next_pass(g);
    call(g, {leaf(1, nodes), leaf(2, nodes + 32), Msg{nodes + 64, 64, 1, nodes + 128, 0}});
    dump(g, "unwritten_slot", 0);
    // ---- two calls in one pass: the second (the device-fed call without levels) reads the first's destinations;
    //      a host-fed digest in between takes a digest index and produces no tie
    next_pass(g);
    call(g, {leaf(7, nodes), leaf(8, nodes + 32)});
    call(g, {Msg{nullptr, 64, 0, nullptr, 0}}, 2);
    call(g, {Msg{nodes, 64, 0, nullptr, 0}}, 1);
    t = dump(g, "two_calls", 64);
    CHECK(t[0].dst_hash == 3 && t[32].src_hash == 1);
    // ---- a destination rewritten by a later digest, byte by byte: bytes 16..47 now belong to digest 2
    next_pass(g);
    call(g, {leaf(7, nodes), leaf(8, nodes + 32)});
    call(g, {leaf(9, nodes + 16), Msg{nodes, 64, 1, nullptr, 0}});
    t = dump(g, "rewritten", 64);
    CHECK(t[15].src_hash == 0 && t[15].src_byte == 15 && t[16].src_hash == 2 && t[16].src_byte == 0 && t[47].src_byte == 31 &&
          t[48].src_hash == 1 && t[48].src_byte == 16);

    // ---- hsw_gadget_cell_address, unbound image: d_gate + ((column - origin column) * max_rows + row) cells
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns >= 2 && v.gate_cells > ROWS);
    uint64_t columns_seen = 0;
    auto at_position = [&](uint64_t cell) {
        uint64_t col = 0, row = 0;
        void *q = nullptr;
        CHECK(hsw_gadget_cell_position(g, cell, &col, &row) == HSW_OK && hsw_gadget_cell_address(g, cell, &q) == HSW_OK);
        CHECK(q == static_cast<uint8_t *>(v.d_gate) + ((col - v.origin_column) * v.max_rows + row) * 32);
        columns_seen |= 1ull << col;
    };
    for (uint64_t cell = 0; cell < v.gate_cells; cell += 4999) at_position(cell);
    for (uint64_t cell = ROWS - 60; cell < ROWS + 60; cell++) at_position(cell);              // across the first column break
    at_position(v.gate_cells - 1);
    CHECK(columns_seen == (1ull << v.columns) - 1 || columns_seen > 3);
    void *p = nullptr;
    CHECK(hsw_gadget_cell_address(g, v.gate_cells, &p) == HSW_ERR_INVALID_ARG);              // the next digest's: not assigned yet
    CHECK(hsw_gadget_cell_address(g, ~0ull, &p) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_cell_address(g, 0, nullptr) == HSW_ERR_INVALID_ARG && hsw_gadget_cell_address(nullptr, 0, &p) == HSW_ERR_INVALID_ARG);
    // ---- hsw_gadget_verify_equal: refused before anything is launched; n = 0 launches nothing
    const int l0 = hip_stub_launches();
    hsw_tie_report rep;
    uint64_t ca[3] = {0, 5, v.gate_cells - 1}, cb[3] = {1, v.gate_cells, 7};
    CHECK(hsw_gadget_verify_equal(g, ca, cb, 3, &rep) == HSW_ERR_INVALID_ARG);
    cb[1] = ~0ull;
    CHECK(hsw_gadget_verify_equal(g, ca, cb, 3, &rep) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_verify_equal(g, nullptr, cb, 3, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_verify_equal(g, ca, cb, 3, nullptr) == HSW_ERR_INVALID_ARG);
    std::memset(&rep, 0xee, sizeof rep);
    CHECK(hsw_gadget_verify_equal(g, nullptr, nullptr, 0, &rep) == HSW_OK && rep.checks == 0 && rep.violations == 0);
    CHECK(hip_stub_launches() == l0);
    cb[1] = 6;
    CHECK(hsw_gadget_verify_equal(g, ca, cb, 3, &rep) == HSW_OK && rep.checks == 3 && hip_stub_launches() == l0 + 1);
    std::vector<uint64_t> many(5000, 3);                     // the staging grows
    CHECK(hsw_gadget_verify_equal(g, many.data(), many.data(), many.size(), &rep) == HSW_OK && rep.checks == 5000);
    (void)e;
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1 && sizeof(hsw_cell_tie) == 40 && sizeof(hsw_tie_report) == 32);
    const size_t sizes[7] = {128, 128, 128, 128, 128, 128, 128};
    {   // a block-stream gadget has no byte cells
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 2, &e) == HSW_OK);
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 7, 0, &g) == HSW_OK);
        Arena a;
        uint8_t *o = a.get(64);
        g_hash = g_call = 0;
        call(g, {Msg{a.get(5), 5, 0, o, 0}, Msg{o, 32, 1, o + 32, 0}});
        size_t n = 0;
        void *p = nullptr;
        hsw_tie_report rep;
        uint64_t c0 = 0;
        CHECK(hsw_gadget_ties(g, nullptr, 0, &n, nullptr) == HSW_ERR_UNSUPPORTED);
        CHECK(hsw_gadget_cell_address(g, 0, &p) == HSW_ERR_UNSUPPORTED);
        CHECK(hsw_gadget_verify_ties(g, &rep) == HSW_ERR_UNSUPPORTED);
        CHECK(hsw_gadget_verify_equal(g, &c0, &c0, 1, &rep) == HSW_ERR_UNSUPPORTED);
        CHECK(hsw_gadget_ties(nullptr, nullptr, 0, &n, nullptr) == HSW_ERR_INVALID_ARG && hsw_gadget_verify_ties(nullptr, &rep) == HSW_ERR_INVALID_ARG &&
              hsw_gadget_verify_ties(g, nullptr) == HSW_ERR_INVALID_ARG);
        std::printf("CASE block_stream 0 0\n");
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    hsw_gadget *g = nullptr;
    uint64_t ncol = 0;
    CHECK(hsw_gadget_create_ex(e, sizes, 7, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, ROWS, &ncol) == HSW_OK);
    g_hash = g_call = 0;
    cases(e, g);
    hsw_gadget_destroy(g);
    {   // a Context group, K = 2 proofs of M = 3 digests (two leaves and their root), both trees in one nodes block:
        // no tie crosses proofs, the digests are c * M + m
        CHECK(hsw_gadget_create_contexts(e, sizes, 3, 2, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, ROWS, &ncol) == HSW_OK);
        Arena a;
        uint8_t *nodes = a.get(32 * 6);
        std::vector<Msg> m;
        for (size_t c = 0; c < 2; c++) {
            uint8_t *t = nodes + 96 * c;
            m.push_back(Msg{a.get(10 + c), 10 + c, 0, t, 0});
            m.push_back(Msg{a.get(119), 119, 0, t + 32, 0});
            m.push_back(Msg{t, 64, 1, t + 64, 0});
        }
        g_hash = g_call = 0;
        call(g, m);
        const std::vector<hsw_cell_tie> t = dump(g, "context_group", 128);
        for (const hsw_cell_tie &x : t) CHECK(x.src_hash / 3 == x.dst_hash / 3 && x.dst_hash % 3 == 2 && x.src_hash % 3 == x.dst_byte / 32);
        // a cell of proof 1 lies in proof 1's image: one image further than the same cell of proof 0
        hsw_context_region r0, r1;
        CHECK(hsw_gadget_context_region(g, 0, &r0) == HSW_OK && hsw_gadget_context_region(g, 1, &r1) == HSW_OK);
        void *p0 = nullptr, *p1 = nullptr;
        CHECK(hsw_gadget_cell_address(g, t[0].dst_cell, &p0) == HSW_OK && hsw_gadget_cell_address(g, t[64].dst_cell, &p1) == HSW_OK);
        CHECK(t[64].dst_cell == t[0].dst_cell + r0.stream_cells);
        CHECK(static_cast<uint8_t *>(p1) - static_cast<uint8_t *>(p0) == static_cast<uint8_t *>(r1.d_image) - static_cast<uint8_t *>(r0.d_image));
        hsw_gadget_destroy(g);
    }
    {   // columns by pointer table, the columns in DESCENDING address order: the caller's own pointer + row * 32
        const size_t two[3] = {128, 128, 128};
        CHECK(hsw_gadget_create_ex(e, two, 3, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        CHECK(hsw_gadget_set_origin(g, 2, 17, 0, 0) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, ROWS, &ncol) == HSW_OK && ncol >= 2);
        hsw_region_binding need;
        CHECK(hsw_gadget_region_binding(g, &need) == HSW_OK);
        const uint64_t PITCH = ROWS + 12, lk = need.lookup_capacity, rows = need.chip_rows_capacity;
        std::vector<void *> mine;
        auto cells = [&](uint64_t n) { void *q = std::aligned_alloc(128, (size_t)((n * 32 + 127) & ~127ull)); CHECK(q); mine.push_back(q); return q; };
        // ONE slab, column k at its far end first: addresses descend with k whatever the allocator does
        uint8_t *slab = static_cast<uint8_t *>(cells(ncol * (PITCH + 5)));
        std::vector<void *> img(ncol);
        for (uint64_t k = 0; k < ncol; k++) img[k] = slab + (ncol - 1 - k) * (PITCH + 5) * 32;
        for (uint64_t k = 1; k < ncol; k++) CHECK(img[k] < img[k - 1]);
        const uint64_t chip = (2 * (rows + 1) + 3) & ~3ull;
        hsw_region_binding b{nullptr, PITCH, ncol, 0, cells(lk), lk, lk, cells(chip), cells(chip), rows + 1, rows, chip};
        CHECK(hsw_gadget_bind_columns(g, &b, img.data(), img.size()) == HSW_OK);
        Arena a;
        uint8_t *nodes = a.get(96);
        g_hash = g_call = 0;
        call(g, {Msg{a.get(10), 10, 0, nodes, 0}, Msg{a.get(11), 11, 0, nodes + 32, 0}, Msg{nodes, 64, 1, nodes + 64, 0}});
        const std::vector<hsw_cell_tie> t = dump(g, "pointer_table", 64);
        hsw_gadget_view v;
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        uint64_t last_col = 0;
        for (uint64_t cell = 0; cell < v.gate_cells; cell += 997) {
            uint64_t col = 0, row = 0;
            void *p = nullptr;
            CHECK(hsw_gadget_cell_position(g, cell, &col, &row) == HSW_OK && hsw_gadget_cell_address(g, cell, &p) == HSW_OK);
            CHECK(col >= 2 && col - 2 < ncol && p == static_cast<uint8_t *>(img[col - 2]) + row * 32);
            last_col = col;
        }
        CHECK(last_col > 2);                                 // more than one column was reached
        void *p = nullptr;
        CHECK(hsw_gadget_cell_address(g, t[0].src_cell, &p) == HSW_OK);
        hsw_gadget_destroy(g);                               // while bound, with pair staging allocated
        for (void *q : mine) std::free(q);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0);
    std::printf("ties lifecycle ok\n");
    return 0;
}
