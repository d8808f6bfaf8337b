// hsw_gadget_lookup_product on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP
// runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every refusal that is
// decided before a launch (and that it launches nothing and allocates nothing), the number of arguments of a single
// Context, a Context group and a gadget with 3 chip columns, the three launches of a call, the growth of the gadget's
// scratch and its release (no device allocation and no event left at the end).
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

// the caller's columns: per argument the dense and spread inputs, A', S' (u cells each) and Z (u + 1 cells), exact size
struct Columns {
    std::vector<const void *> in, in_spread, pin, ptab;
    std::vector<void *> z, mine;
    void *cells(uint64_t n) {
        void *p = std::aligned_alloc(32, (size_t)n * 32);
        CHECK(p);
        std::memset(p, 0, (size_t)n * 32);
        mine.push_back(p);
        return p;
    }
    Columns(size_t n_args, uint64_t u) {
        for (size_t a = 0; a < n_args; a++) {
            in.push_back(cells(u)); in_spread.push_back(cells(u)); pin.push_back(cells(u)); ptab.push_back(cells(u));
            z.push_back(cells(u + 1));
        }
    }
    ~Columns() { for (void *p : mine) std::free(p); }
    hsw_lookup_product args(uint32_t table, uint64_t u, size_t n_args, const void *thetas, const void *betas, const void *gammas, uint32_t *status) const {
        return hsw_lookup_product{table, 0, u, n_args, in.data(), table == HSW_LOOKUP_SPREAD ? in_spread.data() : nullptr, nullptr,
                                  pin.data(), ptab.data(), z.data(), thetas, betas, gammas, status};
    }
};

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_lookup_product) == 104 && sizeof(hsw_product_report) == 72);
    CHECK(HSW_PRODUCT_OPEN == 1 && HSW_PRODUCT_ZERO_DENOM == 2 && HSW_PRODUCT_CELL_NOT_BELOW_P == 4);
    hsw_product_report rep;
    uint64_t ch[3][4] = {{5, 0, 0, 0}, {P[0] - 1, P[1], P[2], P[3]}, {7, 7, 7, 1}};            // (p - 1 is a field element)
    const uint64_t above[3][4] = {{5, 0, 0, 0}, {1, 0, 0, 0}, {7, 7, 7, ~0ull}};               // the third is above p
    uint32_t status[8];
    {   // ---- a linear block-stream gadget, 3 chip columns, no lookup column: 3 spread arguments; RANGE has one: the
        //      caller brings its column, whatever the gadget holds
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        digests(e, g, 1);
        Columns col(3, 3000);
        hsw_lookup_product a = col.args(HSW_LOOKUP_SPREAD, 3000, 3, ch, ch, ch, status);
        int l0 = hip_stub_launches();
        const size_t live0 = hip_stub_live_device_allocations();
        CHECK(hsw_gadget_lookup_product(g, &a, &rep) == HSW_OK);
        CHECK(rep.arguments == 3 && rep.written == 3 * 3001 && rep.open_arguments == 0 && rep.refused_arguments == 0);
        CHECK(rep.first_open == ~0ull && rep.first_refused == ~0ull && rep.tile_rows >= 64);
        CHECK(hip_stub_launches() == l0 + 3);                                // tiles, scan, write
        CHECK(hip_stub_live_device_allocations() == live0 + 1);              // the scratch
        hsw_lookup_product bad = a;
        l0 = hip_stub_launches();
        bad.n_arguments = 2;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // one argument per chip column
        Columns big(1, 70000);
        bad = big.args(HSW_LOOKUP_RANGE, 70000, 1, nullptr, ch, ch, nullptr);                  // (no status array: allowed)
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_OK && rep.arguments == 1 && rep.written == 70001);
        CHECK(hip_stub_launches() == l0 + 3);
        // 8-byte cells: refused, nothing launched
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_product(g, &a, &rep) == HSW_ERR_UNSUPPORTED && std::strstr(hsw_last_error(e), "32-byte"));
        digests(e, g, 1);                                                    // a pass written in 8-byte cells
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_product(g, &a, &rep) == HSW_ERR_UNSUPPORTED && hip_stub_launches() == l0 && rep.written == 0);
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- a single Context: 1 range argument, 2 spread arguments; every refusal; scratch growth
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, WHOLE, &g) == HSW_OK);
        const uint64_t u = 66000;
        Columns col(2, u);
        const hsw_lookup_product sp = col.args(HSW_LOOKUP_SPREAD, u, 2, ch, ch, ch, status);
        const hsw_lookup_product rg = col.args(HSW_LOOKUP_RANGE, u, 1, nullptr, ch, ch, status);
        const size_t live0 = hip_stub_live_device_allocations();
        int l0 = hip_stub_launches();
        // refusals, each before any launch and before the scratch exists
        hsw_lookup_product bad = sp;
        CHECK(hsw_gadget_lookup_product(nullptr, &sp, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_lookup_product(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_lookup_product(g, &sp, nullptr) == HSW_ERR_INVALID_ARG);
        bad.table = 2;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.flags = 1;                                              // HSW_PERMUTED_GIVEN_M is not this call's
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.flags = 4;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.usable_rows = 255;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);               // u < T
        bad = rg; bad.usable_rows = 65535;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.usable_rows = (1ull << 31) + 1;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_TOO_LARGE);
        bad = sp; bad.n_arguments = 1;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = rg; bad.n_arguments = 2;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        // a NULL pointer array, one by one
        bad = sp; bad.d_inputs = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.d_inputs_spread = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.d_permuted_inputs = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.d_permuted_tables = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.d_products = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        // a NULL or misaligned column, in every family; the text names the argument
        for (int family = 0; family < 5; family++)
            for (int how = 0; how < 2; how++) {
                std::vector<const void *> cp(family == 0 ? col.in : family == 1 ? col.in_spread : family == 2 ? col.pin : col.ptab);
                std::vector<void *> zp(col.z);
                if (family < 4) cp[1] = how ? static_cast<const uint8_t *>(cp[1]) + 8 : nullptr;
                else zp[1] = how ? static_cast<uint8_t *>(zp[1]) + 8 : nullptr;
                bad = sp;
                if (family == 0) bad.d_inputs = cp.data();
                if (family == 1) bad.d_inputs_spread = cp.data();
                if (family == 2) bad.d_permuted_inputs = cp.data();
                if (family == 3) bad.d_permuted_tables = cp.data();
                if (family == 4) bad.d_products = zp.data();
                CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "argument 1"));
            }
        {
            uint64_t rows[2] = {u, u + 1};
            bad = sp; bad.input_rows = rows;
            CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "argument 1"));
        }
        // challenges: missing, equal to p, above p -- in each of the three arrays
        bad = sp; bad.thetas = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.betas = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = rg; bad.gammas = nullptr;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.thetas = P;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = sp; bad.betas = P;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        bad = rg; bad.gammas = above[2];
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        // overlaps: Z on another Z, Z on its own input, Z on another argument's A', Z's last cell (row u) on S'
        {
            std::vector<void *> zp(col.z);
            zp[1] = static_cast<uint8_t *>(zp[0]) + 32 * u;                    // argument 1's row 0 is argument 0's row u
            bad = sp; bad.d_products = zp.data();
            CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "overlaps"));
            zp = col.z; zp[0] = const_cast<void *>(col.in[0]);
            bad.d_products = zp.data();
            CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "overlaps"));
            std::vector<const void *> pp(col.pin);
            pp[1] = static_cast<const uint8_t *>(col.z[0]) + 32 * 100;
            bad = sp; bad.d_permuted_inputs = pp.data();
            CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "overlaps"));
            std::vector<const void *> tp(col.ptab);
            tp[0] = static_cast<const uint8_t *>(col.z[1]) + 32 * u;
            bad = sp; bad.d_permuted_tables = tp.data();
            CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "overlaps"));
            // ... while columns that are only read may be one and the same, and an input with no assigned row lies anywhere
            pp = col.pin; pp[1] = col.pin[0];
            const uint64_t rows[2] = {0, 17};
            std::vector<const void *> ip(col.in);
            ip[0] = col.z[0];
            bad = sp; bad.d_permuted_inputs = pp.data(); bad.d_inputs = ip.data(); bad.input_rows = rows;
            const std::vector<const void *> is{col.z[1], col.in_spread[1]};
            bad.d_inputs_spread = is.data();
            CHECK(hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live0);
            CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
        }
        l0 = hip_stub_launches();
        const size_t live = hip_stub_live_device_allocations();
        CHECK(live == live0 + 1);
        digests(e, g, 1);
        const size_t live1 = hip_stub_live_device_allocations();
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_product(g, &sp, &rep) == HSW_OK && hip_stub_launches() == l0 + 3 && rep.arguments == 2 && rep.written == 2 * (u + 1));
        CHECK(hsw_gadget_lookup_product(g, &rg, &rep) == HSW_OK && hip_stub_launches() == l0 + 6 && rep.arguments == 1 && rep.written == u + 1);
        CHECK(hip_stub_live_device_allocations() == live1);                  // the scratch was large enough
        // twice the rows: the scratch grows, once (replaced, not added)
        Columns wide(2, 2 * u);
        const hsw_lookup_product sp2 = wide.args(HSW_LOOKUP_SPREAD, 2 * u, 2, ch, ch, ch, status);
        CHECK(hsw_gadget_lookup_product(g, &sp2, &rep) == HSW_OK && hip_stub_live_device_allocations() == live1);
        CHECK(hsw_gadget_lookup_product(g, &sp2, &rep) == HSW_OK && hsw_gadget_lookup_product(g, &sp, &rep) == HSW_OK);
        CHECK(hip_stub_live_device_allocations() == live1);
        CHECK(hip_stub_live_events() > 0);                                    // (the engine's own)
        hsw_gadget_destroy(g);                                                // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live1);
    }
    {   // ---- a pass whose batches differ in representation: refused, nothing launched; a reset clears it
        const size_t sizes[2] = {64, 64};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, WHOLE, &g) == HSW_OK);
        const uint64_t u = 65536 + 5;
        Columns col(2, u);
        const hsw_lookup_product sp = col.args(HSW_LOOKUP_SPREAD, u, 2, ch, ch, ch, status);
        const hsw_lookup_product rg = col.args(HSW_LOOKUP_RANGE, u, 1, nullptr, ch, ch, status);
        digests(e, g, 1);
        CHECK(hsw_gadget_set_repr(g, HSW_REPR_MONTGOMERY) == HSW_OK);
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_product(g, &sp, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);   // one batch so far: canonical
        digests(e, g, 1);
        l0 = hip_stub_launches();
        const size_t live = hip_stub_live_device_allocations();
        CHECK(hsw_gadget_lookup_product(g, &sp, &rep) == HSW_ERR_UNSUPPORTED && std::strstr(hsw_last_error(e), "differ in representation"));
        CHECK(hsw_gadget_lookup_product(g, &rg, &rep) == HSW_ERR_UNSUPPORTED && rep.written == 0);
        CHECK(hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live);
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        digests(e, g, 2);                                                    // both in Montgomery form
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_lookup_product(g, &sp, &rep) == HSW_OK && hsw_gadget_lookup_product(g, &rg, &rep) == HSW_OK);
        CHECK(hip_stub_launches() == l0 + 6);
        hsw_gadget_destroy(g);
    }
    {   // ---- a Context group, M = 2 and K = 3: 3 range and 6 spread arguments, a challenge per Context
        const size_t sizes[2] = {64, 128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_contexts(e, sizes, 2, 3, 1, WHOLE, &g) == HSW_OK);
        uint64_t columns = 0;
        CHECK(hsw_gadget_set_columns(g, (1u << 17) - 9, &columns) == HSW_OK);   // (a Context group is laid out in columns)
        digests(e, g, 6);
        const uint64_t u = 65536 + 9;
        Columns col(6, u);
        hsw_lookup_product sp = col.args(HSW_LOOKUP_SPREAD, u, 6, ch, ch, ch, status);
        const hsw_lookup_product rg = col.args(HSW_LOOKUP_RANGE, u, 3, nullptr, ch, ch, status);
        const size_t events = hip_stub_live_events();
        int l0 = hip_stub_launches();
        sp.gammas = above;
        CHECK(hsw_gadget_lookup_product(g, &sp, &rep) == HSW_ERR_INVALID_ARG && hip_stub_launches() == l0);   // the third Context's is above p
        sp.gammas = ch;
        CHECK(hsw_gadget_lookup_product(g, &sp, &rep) == HSW_OK && rep.arguments == 6 && rep.written == 6 * (u + 1));
        CHECK(hip_stub_launches() == l0 + 3);
        CHECK(hsw_gadget_lookup_product(g, &rg, &rep) == HSW_OK && rep.arguments == 3 && hip_stub_launches() == l0 + 6);
        hsw_lookup_product bad = sp;
        bad.n_arguments = 3;
        CHECK(hsw_gadget_lookup_product(g, &bad, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hip_stub_live_events() == events);                              // the calls' own events are gone
        hsw_gadget_destroy(g);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("lookup product lifecycle ok\n");
    return 0;
}
