// hsw_gadget_ntt on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP runtime of
// hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every refusal that is decided
// before a launch, with its status and its hsw_last_error (and that it launches nothing and allocates nothing), among
// them an omega of order N / 2 and one of order 2 N; the launches per (log_n, pass_log); the groups of columns and the
// growth of the scratch; the cache of twiddle tables (a hit launches no table kernel, a fifth root evicts the one used
// longest ago, all freed); the overlap rules (in place accepted, every other overlap refused); the groups of columns
// under the engine option "round_scratch", launch by launch; no device allocation and no event left at the end.  The columns are addresses only: no launch runs, so nothing reads them.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_gadget.hpp"
#include "../../halo2-dynamic-sha256_amd/csrc/hsw_ntt.h"
#include "../../halo2-dynamic-sha256_amd/csrc/hsw_ntt_value.hpp"
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

using hsw::PFe;

// base^((p - 1) / 2^log_n) as a canonical cell: base 7 gives a primitive 2^log_n-th root of unity
static PFe root(uint32_t log_n, uint32_t base = 7) {
    const uint32_t pm1[8] = {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    PFe r = hsw::fr_one_mont();
    const PFe b = hsw::fr_to_mont(PFe{{base, 0, 0, 0, 0, 0, 0, 0}});
    for (int bit = 255; bit >= 0; bit--) {
        r = hsw::fr_mont_mul(r, r);
        const int at = bit + (int)log_n;                                   // bit `bit` of (p - 1) >> log_n
        if (at < 256 && ((pm1[at >> 5] >> (at & 31)) & 1u)) r = hsw::fr_mont_mul(r, b);
    }
    return hsw::fr_from_mont(r);
}

struct Columns {
    std::vector<const void *> in;
    std::vector<void *> out;
    Columns(size_t n, uint32_t log_n) {
        const uintptr_t pitch = (uintptr_t)64 << log_n;                     // a column, and as much room after it
        for (size_t b = 0; b < n; b++) {
            in.push_back(reinterpret_cast<const void *>((uintptr_t)0x100000000000ull + 2 * b * pitch));
            out.push_back(reinterpret_cast<void *>((uintptr_t)0x100000000000ull + (2 * b + 1) * pitch));
        }
    }
    hsw_ntt args(uint32_t log_n, const void *omega, uint32_t *status) const {
        return hsw_ntt{0, log_n, 0, 0, in.size(), in.data(), nullptr, out.data(), omega, nullptr, nullptr, status};
    }
};

static bool refused(hsw_engine *e, hsw_gadget *g, const hsw_ntt &a, int status, const char *text) {
    hsw_ntt_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    const int rc = hsw_gadget_ntt(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "got %d (%s), expected %d (...%s...)\n", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.written == 0;
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_ntt) == 80 && sizeof(hsw_ntt_report) == 64);
    CHECK(HSW_NTT_SHIFT_AFTER == hsw::NTT_SHIFT_AFTER && HSW_NTT_CELL_NOT_BELOW_P == hsw::NTT_CELL_NOT_BELOW_P && HSW_NTT_CELL_NOT_BELOW_P == HSW_PRODUCT_CELL_NOT_BELOW_P);
    hsw_ntt_report rep;
    uint32_t status[8];
    const uint64_t above[4] = {7, 7, 7, ~0ull}, five[4] = {5, 0, 0, 0};
    const PFe w8 = root(8);
    {   // ---- a linear block-stream gadget transforms too; in 8-byte cells: refused, nothing launched
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        const Columns col(2, 8);
        const hsw_ntt a = col.args(8, &w8, status);
        CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.columns == 2 && rep.written == 512 && rep.launches == 1 && rep.scratch_bytes == 0);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        CHECK(refused(e, g, a, HSW_ERR_UNSUPPORTED, "32-byte"));
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- every refusal
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const Columns col(3, 8);
        const hsw_ntt ok = col.args(8, &w8, status);
        hsw_ntt bad = ok;
        CHECK(hsw_gadget_ntt(nullptr, &ok, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_ntt(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_ntt(g, &ok, nullptr) == HSW_ERR_INVALID_ARG);
        bad.n_columns = 0;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "at least 1"));
        bad = ok; bad.flags = 2;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "unknown flag"));
        bad = ok; bad.log_n = 0;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "log_n is 1 .. 28"));
        bad = ok; bad.log_n = 29;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "log_n is 1 .. 28"));
        bad = ok; bad.pass_log = 11;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "pass_log is 0 .. 10"));
        bad = ok; bad.d_inputs = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        bad = ok; bad.d_outputs = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        for (int family = 0; family < 2; family++)
            for (int how = 0; how < 2; how++) {
                std::vector<const void *> ip(col.in);
                std::vector<void *> op(col.out);
                if (family == 0) ip[1] = how ? static_cast<const uint8_t *>(ip[1]) + 8 : nullptr;
                else op[1] = how ? static_cast<uint8_t *>(op[1]) + 8 : nullptr;
                bad = ok; bad.d_inputs = ip.data(); bad.d_outputs = op.data();
                CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, family == 0 ? "column 1: an input pointer" : "column 1: an output pointer"));
                CHECK(std::strstr(hsw_last_error(e), "NULL or not 16-byte aligned"));
            }
        {
            uint64_t rows[3] = {256, 0, 257};
            bad = ok; bad.input_rows = rows;
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "column 2: input_rows above 2^log_n"));
        }
        bad = ok; bad.omega = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "omega is NULL"));
        bad = ok; bad.omega = above;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "not below p"));
        bad = ok; bad.shift = above;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "not below p"));
        bad = ok; bad.scale = above;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "not below p"));
        const PFe w7 = root(7), w9 = root(9);
        bad = ok; bad.omega = &w7;                                          // of order N / 2
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "not a primitive"));
        bad = ok; bad.omega = &w9;                                          // of order 2 N
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "not a primitive"));
        bad = ok; bad.omega = five;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "not a primitive"));
        // ---- the overlap rules
        {
            std::vector<const void *> ip(col.in);
            std::vector<void *> op(col.out);
            op[1] = const_cast<void *>(ip[1]);                               // in place: accepted
            bad = ok; bad.d_inputs = ip.data(); bad.d_outputs = op.data();
            CHECK(hsw_gadget_ntt(g, &bad, &rep) == HSW_OK && rep.written == 3 * 256);
            ip[2] = ip[0];                                                   // two columns read one input: accepted
            CHECK(hsw_gadget_ntt(g, &bad, &rep) == HSW_OK && rep.written == 3 * 256);
            op[1] = static_cast<uint8_t *>(const_cast<void *>(ip[1])) + 32;  // its own input, a cell further: refused
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "column 1: its output overlaps"));
            op[1] = const_cast<void *>(ip[0]);                               // another column's input: refused
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "its output overlaps"));
            op[1] = static_cast<uint8_t *>(op[0]) + 255 * 32;                // the last cell of another output: refused
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "its output overlaps"));
            op[1] = static_cast<uint8_t *>(op[0]) + 256 * 32;                // adjacent: accepted
            CHECK(hsw_gadget_ntt(g, &bad, &rep) == HSW_OK);
            uint64_t rows[3] = {256, 0, 256};                                // an input of no rows overlaps nothing
            ip[1] = op[0];
            bad.input_rows = rows;
            CHECK(hsw_gadget_ntt(g, &bad, &rep) == HSW_OK);
            rows[1] = 1;
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "its output overlaps"));
        }
        hsw_gadget_destroy(g);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- launches per (log_n, pass_log); the cache of tables; groups and scratch
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        const uint32_t logs[6] = {1, 10, 11, 16, 17, 20}, want[6] = {1, 1, 2, 2, 3, 3};
        size_t tables = 0;
        for (int k = 0; k < 6; k++) {
            const Columns col(2, logs[k]);
            const PFe w = root(logs[k]);
            hsw_ntt a = col.args(logs[k], &w, status);
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.launches == want[k] && rep.pass_log == 10);
            CHECK(hip_stub_launches() == l0 + 1 + (int)want[k]);             // the table, then the launches of the one group
            CHECK(rep.twiddle_bytes == 32ull << (logs[k] - 1) && rep.scratch_bytes == (want[k] > 1 ? 2 * (32ull << logs[k]) : 0));
            tables = tables < 4 ? tables + 1 : 4;
            CHECK(hip_stub_live_device_allocations() == live0 + 1 + tables);  // the staging and scratch, and at most four tables
            for (uint32_t p = 1; p <= 10; p++) {                             // the same root: no table kernel
                a.pass_log = p;
                const uint32_t s = p > 3 ? p - 2 : 1, n = logs[k] <= p ? 1 : (logs[k] + s - 1) / s;
                const int l1 = hip_stub_launches();
                CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.launches == n && rep.pass_log == p && rep.twiddle_ms == 0);
                CHECK(hip_stub_launches() == l1 + (int)n);
            }
        }
        {   // the tables of 16, 17, 20 and 11 are held (10 went when 20 came): 11 hits, 10 misses and evicts 16 ...
            const Columns col(1, 20);
            const PFe w11 = root(11), w10 = root(10), w16 = root(16), w17 = root(17), w11b = root(11, 5);
            hsw_ntt a = col.args(11, &w11, status);
            int l0 = hip_stub_launches();
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 2);
            a = col.args(10, &w10, status); l0 = hip_stub_launches();
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 2);
            a = col.args(17, &w17, status); l0 = hip_stub_launches();       // ... 17 is still there ...
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
            a = col.args(16, &w16, status); l0 = hip_stub_launches();       // ... and 16 is not
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
            a = col.args(11, &w11b, status); l0 = hip_stub_launches();      // another root of the same order: a table of its own
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
            CHECK(hip_stub_live_device_allocations() == live0 + 5);
        }
        {   // five columns of 256 MiB: groups of four, a scratch of 1 GiB
            const Columns col(5, 23);
            const PFe w = root(23);
            const hsw_ntt a = col.args(23, &w, status);
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.launches == 3 && rep.scratch_bytes == 1ull << 30 && rep.written == 5ull << 23);
            CHECK(hip_stub_launches() == l0 + 1 + 2 * 3);
            CHECK(hip_stub_live_device_allocations() == live0 + 5);
        }
        hsw_gadget_destroy(g);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- "round_scratch": five columns of 64 KiB (log_n 11, two launches a group) on a gadget of their own
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        CHECK(hsw_engine_set_option(e, "round_scratch", 0) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "round_scratch must be 1 .. 2^30 bytes"));
        CHECK(hsw_engine_set_option(e, "round_scratch", ((int64_t)1 << 30) + 1) == HSW_ERR_INVALID_ARG);
        const Columns col(5, 11);
        const PFe w = root(11);
        const hsw_ntt a = col.args(11, &w, status);
        CHECK(hsw_engine_set_option(e, "round_scratch", 2 * 65536 + 31) == HSW_OK);   // two columns and a little: groups of 2, 2 and 1
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.launches == 2 && rep.scratch_bytes == 2 * 65536 && rep.written == 5 * 2048);
        CHECK(hip_stub_launches() == l0 + 1 + 3 * 2);                           // the table, then two launches for each of three groups
        const size_t cap2 = g->scratch.cap;
        const void *d2 = g->scratch.d;
        CHECK(cap2 >= 2 * 65536 && hip_stub_live_device_allocations() == live0 + 2);
        {   // the staged columns (behind the status words' 256 bytes): column b keeps its points in slot b modulo 2, and the
            // second slot ends where the scratch ends
            const hsw::NttColumn *nc = reinterpret_cast<const hsw::NttColumn *>(static_cast<const uint8_t *>(d2) + 256);
            const size_t slot[5] = {0, 1, 0, 1, 0};
            for (size_t b = 0; b < 5; b++)
                CHECK(nc[b].in == col.in[b] && nc[b].out == col.out[b] && reinterpret_cast<const uint8_t *>(nc[b].scratch) == static_cast<const uint8_t *>(d2) + cap2 - (2 - slot[b]) * 65536);
        }
        CHECK(hsw_engine_set_option(e, "round_scratch", 1) == HSW_OK);          // below one column: five groups of one
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.launches == 2 && rep.scratch_bytes == 65536 && hip_stub_launches() == l0 + 5 * 2);
        CHECK(g->scratch.cap == cap2 && g->scratch.d == d2);                    // (a smaller need: the scratch as it was)
        for (size_t b = 0; b < 5; b++)                                          // one slot, and every column in it
            CHECK(reinterpret_cast<const hsw::NttColumn *>(static_cast<const uint8_t *>(d2) + 256)[b].scratch == reinterpret_cast<const hsw::NttColumn *>(static_cast<const uint8_t *>(d2) + 256)[0].scratch);
        {   // one launch holds nothing between launches: the option cuts nothing
            const Columns one(3, 8);
            const hsw_ntt b = one.args(8, &w8, status);
            l0 = hip_stub_launches();
            CHECK(hsw_gadget_ntt(g, &b, &rep) == HSW_OK && rep.launches == 1 && rep.scratch_bytes == 0 && hip_stub_launches() == l0 + 1 + 1);
        }
        CHECK(hsw_engine_set_option(e, "round_scratch", (int64_t)1 << 30) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.launches == 2 && rep.scratch_bytes == 5 * 65536 && hip_stub_launches() == l0 + 2);
        const size_t cap5 = g->scratch.cap;
        const void *d5 = g->scratch.d;
        CHECK(cap5 == cap2 + 3 * 65536 && hip_stub_live_device_allocations() == live0 + 3);   // grown by three columns: replaced, not added to
        CHECK(hsw_engine_set_option(e, "round_scratch", 2 * 65536) == HSW_OK);  // exactly two columns
        CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.scratch_bytes == 2 * 65536 && g->scratch.cap == cap5 && g->scratch.d == d5);
        CHECK(hsw_engine_set_option(e, "round_scratch", 2 * 65536 - 1) == HSW_OK);   // a byte short of two: groups of one
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_ntt(g, &a, &rep) == HSW_OK && rep.scratch_bytes == 65536 && hip_stub_launches() == l0 + 5 * 2);
        CHECK(hsw_engine_set_option(e, "round_scratch", (int64_t)1 << 30) == HSW_OK);
        hsw_gadget_destroy(g);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("ntt lifecycle ok\n");
    return 0;
}
