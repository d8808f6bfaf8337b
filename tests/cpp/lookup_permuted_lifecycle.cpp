// hsw_gadget_lookup_permuted on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP
// runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every refusal that is
// decided before a launch (and that it launches nothing), the number of arguments of a single Context, a Context group
// and a gadget with 3 chip columns, the launches of a call in both modes and for groups of arguments, the growth of the
// gadget's scratch and its release (no device allocation and no event left at the end).
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
int hip_stub_launches();
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static const uint32_t WHOLE = HSW_GADGET_WHOLE_DIGEST;
static const uint64_t P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

static void digests(hsw_engine *e, hsw_gadget *g, size_t n) {
    std::vector<uint8_t> msg(150, 7);
    std::vector<const uint8_t *> in(n, msg.data());
    std::vector<size_t> len(n), pre(n, 0);
    for (size_t i = 0; i < n; i++) len[i] = (i * 37) % 55;
    std::vector<hsw_hash_result> r(n);
    const int rc = hsw_gadget_digest_batch(g, n, in.data(), len.data(), pre.data(), r.data());
    if (rc != HSW_OK) std::fprintf(stderr, "hsw_gadget_digest_batch: %s (%s)\n", hsw_strerror(rc), hsw_last_error(e));
    CHECK(rc == HSW_OK);
}

// the caller's columns: n_args x 2 columns of u cells, exact size, and the two pointer arrays
struct Columns {
    std::vector<void *> in, tab;
    std::vector<void *> mine;
    Columns(size_t n_args, uint64_t u) {
        for (size_t a = 0; a < 2 * n_args; a++) {
            void *p = std::aligned_alloc(32, (size_t)u * 32);
            CHECK(p);
            std::memset(p, 0x5a, (size_t)u * 32);
            mine.push_back(p);
            (a < n_args ? in : tab).push_back(p);
        }
    }
    ~Columns() { for (void *p : mine) std::free(p); }
};

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_lookup_permuted) == 64 && sizeof(hsw_permuted_report) == 80);
    hsw_permuted_report rep;
    uint64_t theta[3][4] = {{5, 0, 0, 0}, {P[0] - 1, P[1], P[2], P[3]}, {7, 7, 7, ~0ull}};   // (p - 1; a value above p)
    std::vector<uint32_t> m(6 * 70000, 0);
    {   // ---- a linear block-stream gadget, 3 chip columns, no lookup column: 3 spread arguments, RANGE refused
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        digests(e, g, 1);
        Columns col(3, 3000);
        hsw_lookup_permuted a{HSW_LOOKUP_SPREAD, 0, 3000, 3, col.in.data(), col.tab.data(), theta, nullptr, 0};
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &a, &rep) == HSW_OK);
        CHECK(rep.arguments == 3 && rep.entries == 2 * 4120 && rep.written == 2 * 3000 * 3 && rep.not_in_table == 0 && rep.overflow_arguments == 0);
        CHECK(hip_stub_launches() == l0 + 5);                                // zero, count; prepare, values, write
        hsw_lookup_permuted bad = a;
        l0 = hip_stub_launches();
        bad.n_arguments = 2;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // one argument per chip column
        bad = a; bad.usable_rows = 2746;                                      // columns 0 and 1 hold 2,747 rows
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "argument 0"));
        bad = a; bad.table = HSW_LOOKUP_RANGE; bad.n_arguments = 1; bad.usable_rows = 70000;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_UNSUPPORTED);               // no lookup column
        CHECK(hip_stub_launches() == l0);
        // 8-byte cells (a block-stream gadget takes them before the first block of a pass): refused, nothing launched
        CHECK(hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_ERR_INVALID_ARG);              // (not in the middle of a pass)
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &a, &rep) == HSW_ERR_UNSUPPORTED && std::strstr(hsw_last_error(e), "32-byte"));
        CHECK(hip_stub_launches() == l0);
        digests(e, g, 1);                                                    // a pass written in 8-byte cells
        l0 = hip_stub_launches();
        bad = a; bad.flags = HSW_PERMUTED_GIVEN_M; bad.d_m = m.data();
        CHECK(hsw_gadget_lookup_permuted(g, &a, &rep) == HSW_ERR_UNSUPPORTED && hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_UNSUPPORTED);
        CHECK(hip_stub_launches() == l0 && rep.written == 0);
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- a single Context: 1 range argument, 2 spread arguments; every refusal; both modes; scratch growth
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, WHOLE, &g) == HSW_OK);
        const uint64_t u = 66000;
        Columns col(2, u);
        hsw_lookup_permuted sp{HSW_LOOKUP_SPREAD, 0, u, 2, col.in.data(), col.tab.data(), theta, nullptr, 0};
        hsw_lookup_permuted rg{HSW_LOOKUP_RANGE, 0, u, 1, col.in.data(), col.tab.data(), nullptr, nullptr, 0};
        const size_t live0 = hip_stub_live_device_allocations();
        int l0 = hip_stub_launches();
        // nothing digested: an empty run list is valid -- no count launch
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_OK && rep.entries == 0 && rep.written == 2 * u * 2);
        CHECK(hip_stub_launches() == l0 + 4 && hip_stub_live_device_allocations() == live0 + 1);
        digests(e, g, 1);
        const size_t live = hip_stub_live_device_allocations();
        // refusals, each before any launch
        l0 = hip_stub_launches();
        hsw_lookup_permuted bad = sp;
        CHECK(hsw_gadget_lookup_permuted(nullptr, &sp, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_lookup_permuted(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_lookup_permuted(g, &sp, nullptr) == HSW_ERR_INVALID_ARG);
        bad.table = 2;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.flags = 4;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // unknown flag
        bad = sp; bad.usable_rows = 255;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // u < T
        bad = rg; bad.usable_rows = 65535;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.usable_rows = (1ull << 31) + 1;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_TOO_LARGE);
        bad = sp; bad.usable_rows = 4000;                                     // 2 blocks: 4,120 rows per column
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "argument 0"));
        bad = sp; bad.n_arguments = 1;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = rg; bad.n_arguments = 2;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.d_input_columns = nullptr;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        {
            std::vector<void *> p2(col.tab);
            p2[1] = nullptr;
            bad = sp; bad.d_table_columns = p2.data();
            CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);           // a NULL column
            p2[1] = static_cast<uint8_t *>(col.tab[1]) + 8;
            CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);           // not 16-byte aligned
        }
        bad = sp; bad.thetas = nullptr;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.thetas = P;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // theta = p
        bad = sp; bad.thetas = theta[2];
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // above p
        bad = sp; bad.flags = HSW_PERMUTED_GIVEN_M;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // given mode without d_m
        bad = sp; bad.d_m = m.data(); bad.m_pitch = 255;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.d_m = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(m.data()) + 2);
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live);
        // counted: zero, count, prepare, values, write; theta = p - 1 is a field element
        bad = sp; bad.thetas = theta[1];
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_OK && hip_stub_launches() == l0 + 5);
        CHECK(rep.arguments == 2 && rep.entries == 2 * 4120 && rep.written == 2 * u * 2);
        // given: sums, prepare, values, write
        bad = sp; bad.flags = HSW_PERMUTED_GIVEN_M | HSW_PERMUTED_THETA_ON_SPREAD; bad.d_m = m.data(); bad.m_pitch = 70000;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_OK && hip_stub_launches() == l0 + 9 && rep.entries == 0);
        CHECK(hip_stub_live_device_allocations() == live);                   // the scratch was large enough
        // the range argument needs more: the scratch grows, once
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_OK && hip_stub_launches() == l0 + 14);
        CHECK(rep.arguments == 1 && rep.written == 2 * u && rep.entries == 3 + 2 * 128 + 2 * 3184 + 64);
        CHECK(hip_stub_live_device_allocations() == live);                   // (replaced, not added)
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_OK && hip_stub_live_device_allocations() == live);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_OK && rep.entries == 0 && hip_stub_launches() == l0 + 4);
        CHECK(hip_stub_live_events() > 0);                                    // (the engine's own)
        hsw_gadget_destroy(g);                                                // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live);
    }
    {   // ---- a pass whose batches differ in representation: refused in both modes, nothing launched; a reset clears it
        const size_t sizes[2] = {64, 64};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, WHOLE, &g) == HSW_OK);
        const uint64_t u = 65536 + 5;
        Columns col(2, u);
        hsw_lookup_permuted sp{HSW_LOOKUP_SPREAD, 0, u, 2, col.in.data(), col.tab.data(), theta, nullptr, 0};
        hsw_lookup_permuted rg{HSW_LOOKUP_RANGE, HSW_PERMUTED_GIVEN_M, u, 1, col.in.data(), col.tab.data(), nullptr, m.data(), 0};
        digests(e, g, 1);
        CHECK(hsw_gadget_set_repr(g, HSW_REPR_MONTGOMERY) == HSW_OK);
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_OK && hip_stub_launches() == l0 + 5);   // one batch so far: canonical
        digests(e, g, 1);
        l0 = hip_stub_launches();
        const size_t live = hip_stub_live_device_allocations();
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_ERR_UNSUPPORTED && std::strstr(hsw_last_error(e), "differ in representation"));
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_ERR_UNSUPPORTED && rep.written == 0);
        CHECK(hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        digests(e, g, 2);                                                    // both in Montgomery form
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_OK && hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_OK);
        CHECK(hip_stub_launches() == l0 + 5 + 4);
        hsw_gadget_destroy(g);
    }
    {   // ---- a Context group, M = 2 and K = 3: 3 range and 6 spread arguments, in groups of one proof
        const size_t sizes[2] = {64, 128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_contexts(e, sizes, 2, 3, 1, WHOLE, &g) == HSW_OK);
        uint64_t columns = 0;
        CHECK(hsw_gadget_set_columns(g, (1u << 17) - 9, &columns) == HSW_OK);   // (a Context group is laid out in columns)
        digests(e, g, 6);
        const uint64_t u = 65536 + 9;
        Columns col(6, u);
        hsw_lookup_permuted sp{HSW_LOOKUP_SPREAD, 0, u, 6, col.in.data(), col.tab.data(), theta, m.data(), 0};
        hsw_lookup_permuted rg{HSW_LOOKUP_RANGE, 0, u, 3, col.in.data(), col.tab.data(), nullptr, nullptr, 0};
        const size_t events = hip_stub_live_events();
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_ERR_INVALID_ARG && hip_stub_launches() == l0);   // theta[2] is above p
        theta[2][3] = 1;
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_OK && rep.arguments == 6 && rep.entries == 3 * 3 * 4120);
        CHECK(hip_stub_launches() == l0 + 5);
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_OK && rep.arguments == 3 && hip_stub_launches() == l0 + 10);
        hsw_lookup_permuted bad = sp;
        bad.n_arguments = 3;
        CHECK(hsw_gadget_lookup_permuted(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_engine_set_option(e, "permuted_scratch", 0) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_engine_set_option(e, "permuted_scratch", 1) == HSW_OK);   // a group is at least one proof
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_permuted(g, &sp, &rep) == HSW_OK && hip_stub_launches() == l0 + 2 + 3 * 3);
        // without d_m the multiplicities of all arguments are scratch too, charged to the same budget: refused, no launch
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_ERR_TOO_LARGE && std::strstr(hsw_last_error(e), "d_m") && hip_stub_launches() == l0 + 11);
        CHECK(hsw_engine_set_option(e, "permuted_scratch", 2 * 3 * 65536 * 4) == HSW_OK);     // exactly twice m: accepted, groups of one proof
        CHECK(hsw_engine_set_option(e, "permuted_scratch", 2 * 3 * 65536 * 4 - 1) == HSW_OK);
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_ERR_TOO_LARGE && hip_stub_launches() == l0 + 11);
        CHECK(hsw_engine_set_option(e, "permuted_scratch", 1) == HSW_OK);
        rg.d_m = m.data();
        CHECK(hsw_gadget_lookup_permuted(g, &rg, &rep) == HSW_OK && hip_stub_launches() == l0 + 11 + 2 + 3 * 2 + 1);   // one value table
        CHECK(rep.written == 2 * u * 3);
        CHECK(hsw_engine_set_option(e, "permuted_scratch", 256 << 20) == HSW_OK);
        CHECK(hip_stub_live_events() == events);                              // the calls' own events are gone
        hsw_gadget_destroy(g);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("lookup permuted lifecycle ok\n");
    return 0;
}
