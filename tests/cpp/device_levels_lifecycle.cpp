// hsw_gadget_digest_levels_device on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the
// stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): the refusals that follow
// from pointers, lengths and levels alone (nothing launched, nothing committed, hsw_last_error naming the two
// messages), one ingest launch per distinct level, levels in shuffled order, a Context group, destroy without a leak.
// Inputs are malloc'ed blocks exactly as long as the messages and outputs blocks of exactly 32 bytes, all of them
// POISONED while the library runs: under the stub no kernel runs, so any read or write of an input or an output --
// inside its block or past it -- is the host's and a sanitizer report.  Built and run by
// tests/test_device_levels_host.py.
#include <hip/hip_runtime.h>
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

// "device" memory of the caller's: exact-size heap blocks nobody on the host may touch
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

struct State { size_t cur_hash_idx, blocks_done; uint64_t num_limb_sum, gate_cells, lookup_cells; };
static State state(hsw_gadget *g) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    return State{(size_t)v.cur_hash_idx, (size_t)v.blocks_done, v.num_limb_sum, v.gate_cells, v.lookup_cells};
}
static bool same(const State &a, const State &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Msg { const void *src; size_t len; uint32_t level; void *dst; size_t pre; };

static int levels_call(hsw_gadget *g, const std::vector<Msg> &m, std::vector<hsw_hash_result> *out = nullptr,
                       bool null_levels = false, bool null_outputs = false) {
    std::vector<const void *> p;
    std::vector<size_t> len, pre;
    std::vector<uint32_t> lv;
    std::vector<void *> dst;
    for (const Msg &x : m) { p.push_back(x.src); len.push_back(x.len); pre.push_back(x.pre); lv.push_back(x.level); dst.push_back(x.dst); }
    std::vector<hsw_hash_result> r(m.size() + 1);
    const int rc = hsw_gadget_digest_levels_device(g, m.size(), p.data(), len.data(), pre.data(), null_levels ? nullptr : lv.data(),
                                                   null_outputs ? nullptr : dst.data(), r.data());
    if (out) *out = r;
    return rc;
}

static bool names(hsw_engine *e, const char *a, const char *b) {
    const std::string s = hsw_last_error(e);
    return s.find(a) != std::string::npos && s.find(b) != std::string::npos;
}

// A 4-leaf tree in one nodes block: leaves 0..3 (level 0), inner 4, 5 (level 1), root 6 (level 2); message k's output
// is nodes + 32 k, inner message j reads its two children in place.
static std::vector<Msg> tree(Arena &a, uint8_t *nodes) {
    const size_t leaf_len[4] = {0, 55, 64, 119};
    std::vector<Msg> m;
    for (size_t i = 0; i < 4; i++) m.push_back(Msg{leaf_len[i] ? a.get(leaf_len[i]) : nullptr, leaf_len[i], 0, nodes + 32 * i, 0});
    m.push_back(Msg{nodes + 0, 64, 1, nodes + 128, 0});
    m.push_back(Msg{nodes + 64, 64, 1, nodes + 160, 0});
    m.push_back(Msg{nodes + 128, 64, 2, nodes + 192, 0});
    return m;
}

// sizes: {128} * 7
static void exercise(hsw_engine *e, hsw_gadget *g) {
    Arena a;
    const State fresh = state(g);
    CHECK(fresh.cur_hash_idx == 0 && fresh.blocks_done == 0);
    uint8_t *nodes = a.get(32 * 7);
    const std::vector<Msg> t = tree(a, nodes);

    // ---- argument refusals
    hsw_hash_result one;
    const void *p0 = t[1].src;
    size_t l0 = 5;
    CHECK(hsw_gadget_digest_levels_device(nullptr, 1, &p0, &l0, nullptr, nullptr, nullptr, &one) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_digest_levels_device(g, 1, &p0, &l0, nullptr, nullptr, nullptr, nullptr) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_digest_levels_device(g, 1, nullptr, &l0, nullptr, nullptr, nullptr, &one) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_digest_levels_device(g, 1, &p0, nullptr, nullptr, nullptr, nullptr, &one) == HSW_ERR_INVALID_ARG);
    const int launches0 = hip_stub_launches();
    // ---- the device-fed call's refusals, unchanged
    uint8_t *x = a.get(200), *o = a.get(32);
    CHECK(levels_call(g, {{x, 120, 0, o, 0}}) == HSW_ERR_TOO_LARGE);                           // lib.rs:90
    CHECK(levels_call(g, {{x, 100, 0, o, 100}}) == HSW_ERR_SHAPE);                             // lib.rs:89
    CHECK(levels_call(g, {{x, 5, 0, o, 0}, {nullptr, 3, 1, nullptr, 0}}) == HSW_ERR_INVALID_ARG);   // NULL with a length
    CHECK(levels_call(g, std::vector<Msg>(8, Msg{nullptr, 0, 0, nullptr, 0})) == HSW_ERR_INVALID_ARG);   // an eighth hash
    // ---- overlaps: byte ranges, decided before anything is launched
    uint8_t *w = a.get(96);                                   // never dereferenced: only its addresses matter
    CHECK(levels_call(g, {{x, 5, 0, w, 0}, {x, 7, 0, w + 31, 0}}) == HSW_ERR_INVALID_ARG && names(e, "messages 0", "and 1"));   // by one byte
    CHECK(levels_call(g, {{x, 5, 1, w + 40, 0}, {x, 7, 0, w + 40, 0}}) == HSW_ERR_INVALID_ARG);     // the same 32 bytes, any levels
    CHECK(levels_call(g, {{x, 5, 0, w, 0}, {w + 31, 7, 0, nullptr, 0}}) == HSW_ERR_INVALID_ARG && names(e, "message 1", "message 0"));   // same level: a race
    CHECK(levels_call(g, {{w + 60, 5, 0, nullptr, 0}, {x, 7, 1, w + 32, 0}}) == HSW_ERR_INVALID_ARG && names(e, "message 0", "message 1"));   // a higher level: stale bytes
    CHECK(levels_call(g, {{w, 64, 0, w + 63, 0}}) == HSW_ERR_INVALID_ARG && names(e, "message 0", "message 0"));   // its own output
    CHECK(levels_call(g, {{x, 5, 0, w, 0}, {x, 5, 0, w + 32, 0}, {w, 65, 1, w + 64, 0}}) == HSW_ERR_INVALID_ARG && names(e, "message 2", "message 2"));
    CHECK(levels_call(g, {{x, 5, 3, w, 0}, {x, 5, 0, w + 32, 0}, {w, 64, 2, w + 64, 0}}) == HSW_ERR_INVALID_ARG && names(e, "message 2", "message 0"));
    CHECK(same(state(g), fresh) && hip_stub_launches() == launches0);
    // ---- ranges that only touch are fine (same level): an input that ends where an output begins, and vice versa
    std::vector<hsw_hash_result> r;
    CHECK(levels_call(g, {{x, 5, 0, w + 32, 0}, {w, 32, 0, nullptr, 0}, {w + 64, 32, 0, nullptr, 0}}, &r) == HSW_OK);
    CHECK(state(g).cur_hash_idx == 3 && r[2].first_block == 4);
    CHECK(hsw_gadget_reset(g) == HSW_OK && same(state(g), fresh));

    // ---- one launch more per distinct level more than the device-fed call of the same messages
    std::vector<const void *> p;
    std::vector<size_t> len;
    for (const Msg &m : t) { p.push_back(m.src); len.push_back(m.len); }
    std::vector<hsw_hash_result> flat(7);
    int l1 = hip_stub_launches();
    CHECK(hsw_gadget_digest_batch_device(g, 7, p.data(), len.data(), nullptr, flat.data()) == HSW_OK);
    const int flat_launches = hip_stub_launches() - l1;
    const State full = state(g);
    CHECK(full.cur_hash_idx == 7 && full.blocks_done == 14 && flat_launches >= 2);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    l1 = hip_stub_launches();
    CHECK(levels_call(g, t, &r) == HSW_OK);
    CHECK(hip_stub_launches() - l1 == flat_launches + 2);                                      // 3 levels
    CHECK(same(state(g), full));
    for (size_t i = 0; i < 7; i++)
        CHECK(r[i].first_block == flat[i].first_block && r[i].n_blocks == 2 && r[i].num_round == flat[i].num_round &&
              r[i].input_len == t[i].len && r[i].block_cell == flat[i].block_cell);
    CHECK(levels_call(g, {{x, 1, 0, nullptr, 0}}) == HSW_ERR_INVALID_ARG);                     // the gadget is full
    // every level equal and no outputs, by NULL tables: the device-fed call's launches
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    l1 = hip_stub_launches();
    CHECK(levels_call(g, t, &r, /*null_levels=*/true, /*null_outputs=*/true) == HSW_OK);
    CHECK(hip_stub_launches() - l1 == flat_launches && same(state(g), full));
    // levels with gaps, in shuffled digest order: root first, then a leaf, an inner node, ...
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    std::vector<Msg> sh = {t[6], t[0], t[4], t[1], t[5], t[2], t[3]};
    for (Msg &m : sh) m.level = 10 * m.level + 7;
    l1 = hip_stub_launches();
    CHECK(levels_call(g, sh, &r) == HSW_OK);
    CHECK(hip_stub_launches() - l1 == flat_launches + 2 && same(state(g), full));
    for (size_t i = 0; i < 7; i++) CHECK(r[i].first_block == 2 * i && r[i].input_len == sh[i].len);
    // ... and a shuffled order that is wrong about who reads whom is refused, the pass stays where it is
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    sh[0].level = 7;                                                                           // the root at the leaves' level
    CHECK(levels_call(g, sh) == HSW_ERR_INVALID_ARG && names(e, "message 0", "message 2") && same(state(g), fresh));
    // a prefix (target_round == 0) and a host-fed digest in the same pass
    CHECK(levels_call(g, {{x, 100, 0, o, 128}, {o, 32, 1, nullptr, 0}}, &r) == HSW_OK);
    CHECK(r[0].num_round == 2 && r[0].target_round == 0 && r[1].first_block == 2);
    std::vector<uint8_t> msg(119, 3);
    const uint8_t *hp = msg.data();
    size_t hl = 119;
    CHECK(hsw_gadget_digest_batch(g, 1, &hp, &hl, nullptr, &one) == HSW_OK && one.first_block == 4);
    size_t n_in = 0;
    CHECK(hsw_gadget_input_bytes(g, 1, nullptr, 0, &n_in) == HSW_OK && n_in == 128);
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    const size_t sizes[7] = {128, 128, 128, 128, 128, 128, 128};
    {   // plain gadget, default-mode engine
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 2, &e) == HSW_OK);
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 7, 0, &g) == HSW_OK);
        exercise(e, g);
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    {   // whole-digest gadget with a column image, internals engine
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 7, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        uint64_t n = 0;
        CHECK(hsw_gadget_set_columns(g, (1u << 17) - 9, &n) == HSW_OK);
        exercise(e, g);
        hsw_gadget_destroy(g);
        // a Context group: K = 2 proofs of a circuit with M = 3 digests (two leaves and their root), the levels
        // interleaved in digest order
        CHECK(hsw_gadget_create_contexts(e, sizes, 3, 2, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        CHECK(hsw_gadget_set_columns(g, (1u << 17) - 9, &n) == HSW_OK);
        {
            Arena a;
            uint8_t *nodes = a.get(32 * 6);
            std::vector<Msg> m;
            for (size_t c = 0; c < 2; c++) {
                uint8_t *t = nodes + 96 * c;
                m.push_back(Msg{a.get(10 + c), 10 + c, 0, t, 0});
                m.push_back(Msg{a.get(119), 119, 0, t + 32, 0});
                m.push_back(Msg{t, 64, 1, t + 64, 0});
            }
            std::vector<const void *> p;
            std::vector<size_t> len;
            for (const Msg &x : m) { p.push_back(x.src); len.push_back(x.len); }
            std::vector<hsw_hash_result> flat(6), r;
            int l1 = hip_stub_launches();
            CHECK(hsw_gadget_digest_batch_device(g, 6, p.data(), len.data(), nullptr, flat.data()) == HSW_OK);
            const int flat_launches = hip_stub_launches() - l1;
            const State full = state(g);
            CHECK(full.cur_hash_idx == 6 && full.blocks_done == 12);
            CHECK(hsw_gadget_reset(g) == HSW_OK);
            l1 = hip_stub_launches();
            CHECK(levels_call(g, m, &r) == HSW_OK);
            CHECK(hip_stub_launches() - l1 == flat_launches + 1 && same(state(g), full));      // 2 levels
            for (size_t i = 0; i < 6; i++) CHECK(r[i].first_block == flat[i].first_block && r[i].block_cell == flat[i].block_cell);
            hsw_context_region reg;
            CHECK(hsw_gadget_context_region(g, 1, &reg) == HSW_OK && reg.assigned == 1);
            CHECK(hsw_gadget_reset(g) == HSW_OK);
            m[5].level = 0;                                                                    // proof 1's root races its leaves
            CHECK(levels_call(g, m) == HSW_ERR_INVALID_ARG && names(e, "message 5", "message 3") && state(g).cur_hash_idx == 0);
        }
        hsw_gadget_destroy(g);
        // a gadget destroyed right after its first levels call
        CHECK(hsw_gadget_create_ex(e, sizes, 7, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        {
            Arena a;
            uint8_t *o = a.get(32);
            CHECK(levels_call(g, {{a.get(64), 64, 0, o, 0}, {o, 32, 5, nullptr, 0}}) == HSW_OK);
        }
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0);
    std::printf("device levels lifecycle ok\n");
    return 0;
}
