// hsw_gadget_digest_batch_device on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the
// stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): the refusals that
// follow from the lengths alone (nothing committed), NULL-with-length and over-capacity, the size of what
// hsw_gadget_input_bytes returns, reset / re-digest / destroy without a leak -- for a plain and a whole-digest
// gadget.  Every d_inputs entry with a non-zero length is an address nothing is mapped at: under the stub no kernel
// runs, so ANY read of a message byte is the host's and a sanitizer report.  Built and run by
// tests/test_device_inputs_host.py.
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

// addresses in the unmapped first page, each misaligned differently
static const void *nowhere(size_t i) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(16 * (i + 1) + (2 * i + 1) % 16)); }

struct State { size_t cur_hash_idx, blocks_done; uint64_t num_limb_sum, gate_cells, lookup_cells; };
static State state(hsw_gadget *g) {
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    return State{(size_t)v.cur_hash_idx, (size_t)v.blocks_done, v.num_limb_sum, v.gate_cells, v.lookup_cells};
}
static bool same(const State &a, const State &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int digest(hsw_gadget *g, const std::vector<const void *> &p, const std::vector<size_t> &len, const std::vector<size_t> &pre,
                  std::vector<hsw_hash_result> *out = nullptr) {
    std::vector<hsw_hash_result> r(p.size() + 1);
    const int rc = hsw_gadget_digest_batch_device(g, p.size(), p.data(), len.data(), pre.empty() ? nullptr : pre.data(), r.data());
    if (out) *out = r;
    return rc;
}

// sizes: {128, 64, 192}
static void exercise(hsw_gadget *g, bool whole) {
    const State fresh = state(g);
    CHECK(fresh.cur_hash_idx == 0 && fresh.blocks_done == 0);
    hsw_hash_result one;
    const void *p0 = nowhere(0);
    size_t l0 = 5;
    // ---- argument refusals
    CHECK(hsw_gadget_digest_batch_device(nullptr, 1, &p0, &l0, nullptr, &one) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_digest_batch_device(g, 1, &p0, &l0, nullptr, nullptr) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_digest_batch_device(g, 1, nullptr, &l0, nullptr, &one) == HSW_ERR_INVALID_ARG);
    CHECK(hsw_gadget_digest_batch_device(g, 1, &p0, nullptr, nullptr, &one) == HSW_ERR_INVALID_ARG);
    const int launches0 = hip_stub_launches();
    // ---- refusals decided from the lengths alone: nothing launched, nothing committed
    CHECK(digest(g, {nowhere(0), nowhere(1)}, {5, 56}, {}) == HSW_ERR_TOO_LARGE);            // 56 + 9 > 64 (lib.rs:90)
    CHECK(digest(g, {nowhere(0)}, {120}, {}) == HSW_ERR_TOO_LARGE);
    CHECK(digest(g, {nowhere(0)}, {100}, {100}) == HSW_ERR_SHAPE);                             // lib.rs:89
    CHECK(digest(g, {nowhere(0)}, {10}, {128}) == HSW_ERR_TOO_LARGE);                          // prefix past the padded message
    CHECK(digest(g, {nowhere(0)}, {(size_t)1 << 33}, {(size_t)1 << 33}) == HSW_ERR_TOO_LARGE); // above 4 GiB
    CHECK(digest(g, {nowhere(0), nullptr}, {5, 3}, {}) == HSW_ERR_INVALID_ARG);                // NULL with a length
    CHECK(digest(g, {nowhere(0), nowhere(1), nowhere(2), nowhere(3)}, {1, 1, 1, 1}, {}) == HSW_ERR_INVALID_ARG);   // a fourth hash
    CHECK(same(state(g), fresh) && hip_stub_launches() == launches0);
    // ---- a batch of unreadable addresses succeeds: the host never dereferences a message
    std::vector<hsw_hash_result> r;
    CHECK(digest(g, {nowhere(0), nullptr}, {119, 0}, {}, &r) == HSW_OK);                       // (NULL with length 0 is fine)
    CHECK(hip_stub_launches() > launches0);
    State s = state(g);
    CHECK(s.cur_hash_idx == 2 && s.blocks_done == 3);
    CHECK(r[0].n_blocks == 2 && r[0].num_round == 2 && r[0].target_round == 2 && r[0].input_len == 119 && r[0].first_block == 0);
    CHECK(r[1].n_blocks == 1 && r[1].num_round == 1 && r[1].first_block == 2);
    CHECK(digest(g, {nowhere(2)}, {200}, {}) == HSW_ERR_TOO_LARGE && same(state(g), s));      // a refusal mid-pass
    CHECK(digest(g, {nowhere(2)}, {250}, {128}, &r) == HSW_OK);                                // 5 rounds, 2 of them the prefix
    CHECK(r[0].num_round == 5 && r[0].target_round == 3 && r[0].n_blocks == 3 && r[0].first_block == 3);
    CHECK(digest(g, {nowhere(3)}, {1}, {}) == HSW_ERR_INVALID_ARG);                            // the gadget is full
    // ---- hsw_gadget_input_bytes: max_variable_byte_size bytes each
    const size_t sizes[3] = {128, 64, 192};
    for (size_t h = 0; h < 3; h++) {
        size_t len = 0;
        CHECK(hsw_gadget_input_bytes(g, h, nullptr, 0, &len) == HSW_OK && len == sizes[h]);
        std::vector<uint8_t> buf(len);
        CHECK(hsw_gadget_input_bytes(g, h, buf.data(), len, nullptr) == HSW_OK);
        CHECK(hsw_gadget_input_bytes(g, h, buf.data(), len - 1, nullptr) == HSW_ERR_INVALID_ARG);
    }
    if (whole) {
        hsw_result_cells rc;
        CHECK(hsw_gadget_result_cells(g, 2, &rc) == HSW_OK && rc.n_input_bytes == 192);
    }
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
    // ---- reset and the same pass again, host-fed and device-fed batches mixed
    CHECK(hsw_gadget_reset(g) == HSW_OK && same(state(g), fresh));
    std::vector<uint8_t> msg(119, 3);
    const uint8_t *hp = msg.data();
    size_t hl = 119;
    CHECK(hsw_gadget_digest_batch(g, 1, &hp, &hl, nullptr, &one) == HSW_OK);
    CHECK(digest(g, {nullptr, nowhere(5)}, {0, 183}, {}, &r) == HSW_OK && r[0].first_block == 2 && r[1].first_block == 3);
    s = state(g);
    CHECK(s.cur_hash_idx == 3 && s.blocks_done == 6);
    size_t len = 0;
    CHECK(hsw_gadget_input_bytes(g, 0, nullptr, 0, &len) == HSW_OK && len == 128);
    CHECK(hsw_gadget_input_bytes(g, 2, nullptr, 0, &len) == HSW_OK && len == 192);
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    {   // plain gadget, default-mode engine
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 2, &e) == HSW_OK);
        const size_t sizes[3] = {128, 64, 192};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 3, 0, &g) == HSW_OK);
        exercise(g, false);
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    {   // whole-digest gadget with a column image, internals engine
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
        const size_t sizes[3] = {128, 64, 192};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 3, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        uint64_t n = 0;
        CHECK(hsw_gadget_set_columns(g, (1u << 17) - 9, &n) == HSW_OK);
        exercise(g, true);
        hsw_gadget_destroy(g);
        // a gadget destroyed before its first device-fed batch, and one destroyed right after it
        CHECK(hsw_gadget_create_ex(e, sizes, 3, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        hsw_gadget_destroy(g);
        CHECK(hsw_gadget_create_ex(e, sizes, 3, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        CHECK(digest(g, {nowhere(7)}, {64}, {}) == HSW_OK);
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0);
    std::printf("device inputs lifecycle ok\n");
    return 0;
}
