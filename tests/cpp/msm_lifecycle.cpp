// hsw_gadget_msm on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP runtime of
// hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every refusal that is decided
// before a launch, with its status and its hsw_last_error (and that it launches nothing, allocates nothing and writes
// neither out_points nor status); what the report says of the plan per (n_bases, window_bits, slice_rows); the launches
// -- the check and two per group of columns; the growth and the reuse of the scratch; the groups of columns under 1 GiB
// of partial buckets, and under what the engine option "round_scratch" lowers that to; no device allocation and no event left at the end.  The columns and the bases are addresses only:
// no launch runs, so nothing reads them, and the points the host tail makes of the unwritten scratch are not looked at.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_gadget.hpp"
#include "../../halo2-dynamic-sha256_amd/csrc/hsw_msm_value.hpp"
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

static const void *BASES = reinterpret_cast<const void *>((uintptr_t)0x200000000000ull);

struct Columns {
    std::vector<const void *> in;
    std::vector<uint8_t> out;
    std::vector<uint32_t> status;
    Columns(size_t n, uint64_t n_bases) : out(64 * n, 0xA5), status(n, 0xFFFFFFFFu) {
        for (size_t b = 0; b < n; b++) in.push_back(reinterpret_cast<const void *>((uintptr_t)0x100000000000ull + b * 32 * n_bases));
    }
    hsw_msm args(uint64_t n_bases, uint32_t window_bits = 0, uint32_t slice_rows = 0) {
        return hsw_msm{0, window_bits, slice_rows, 0, in.size(), n_bases, BASES, in.data(), nullptr, out.data(), status.data()};
    }
    bool untouched() const {
        for (uint8_t x : out) if (x != 0xA5) return false;
        for (uint32_t x : status) if (x != 0xFFFFFFFFu) return false;
        return true;
    }
};

static bool refused(hsw_engine *e, hsw_gadget *g, const hsw_msm &a, const Columns &col, int status, const char *text) {
    hsw_msm_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    const int rc = hsw_gadget_msm(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "got %d (%s), expected %d (...%s...)\n", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.launches == 0 && rep.columns == 0 && col.untouched();
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_msm) == 72 && sizeof(hsw_msm_report) == 80);
    CHECK(HSW_MSM_CELL_NOT_BELOW_P == hsw::MSM_CELL_NOT_BELOW_P && HSW_MSM_BASE_NOT_BELOW_Q == hsw::MSM_BASE_NOT_BELOW_Q);
    CHECK(HSW_MSM_CELL_NOT_BELOW_P == HSW_NTT_CELL_NOT_BELOW_P && HSW_MSM_MAX_WINDOW_BITS == hsw::MSM_MAX_WINDOW_BITS && HSW_MSM_MAX_WINDOW_BITS >= 8);
    hsw_msm_report rep;
    {   // ---- a linear block-stream gadget commits too; in 8-byte cells: refused, nothing launched
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        Columns col(2, 300);
        const hsw_msm a = col.args(300);
        CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.columns == 2 && rep.launches == 3 && rep.window_bits == 8 && rep.windows == 32 && rep.slice_rows == 4096 && rep.slices == 1);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        Columns fresh(2, 300);
        CHECK(refused(e, g, fresh.args(300), fresh, HSW_ERR_UNSUPPORTED, "32-byte"));
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
        Columns col(3, 300);
        const hsw_msm ok = col.args(300, 8, 64);
        hsw_msm bad = ok;
        CHECK(hsw_gadget_msm(nullptr, &ok, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_msm(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_msm(g, &ok, nullptr) == HSW_ERR_INVALID_ARG && col.untouched());
        bad.n_columns = 0;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "at least 1"));
        bad = ok; bad.flags = 1;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "unknown flag"));
        bad = ok; bad.n_bases = 0;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "n_bases is 1 .. 2^28"));
        bad = ok; bad.n_bases = (1ull << 28) + 1;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "n_bases is 1 .. 2^28"));
        bad = ok; bad.d_bases = nullptr;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "d_bases is NULL or not 16-byte aligned"));
        bad = ok; bad.d_bases = static_cast<const uint8_t *>(BASES) + 8;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "d_bases is NULL or not 16-byte aligned"));
        bad = ok; bad.d_scalars = nullptr;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        bad = ok; bad.out_points = nullptr;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "out_points is NULL"));
        for (int how = 0; how < 2; how++) {
            std::vector<const void *> ip(col.in);
            ip[1] = how ? static_cast<const uint8_t *>(ip[1]) + 8 : nullptr;
            bad = ok; bad.d_scalars = ip.data();
            CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "column 1: a scalar pointer that is NULL or not 16-byte aligned"));
        }
        {
            const uint64_t rows[3] = {300, 0, 301};
            bad = ok; bad.input_rows = rows;
            CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "column 2: input_rows above n_bases"));
        }
        const uint32_t slices[4] = {32, 63, 96, 1u << 29};
        bad = ok; bad.window_bits = HSW_MSM_MAX_WINDOW_BITS + 1;
        CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "window_bits is 0 .. 8"));
        for (uint32_t s : slices) {
            bad = ok; bad.slice_rows = s;
            CHECK(refused(e, g, bad, col, HSW_ERR_INVALID_ARG, "slice_rows 0 or a power of two"));
        }
        CHECK(hip_stub_live_device_allocations() > 0);                       // (the gadget's own)
        hsw_gadget_destroy(g);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- the plan in the report; launches; the scratch grows once and is reused; groups
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        for (uint32_t c = 1; c <= HSW_MSM_MAX_WINDOW_BITS; c++) {
            Columns col(3, 300);
            const uint64_t rows[3] = {300, 299, 1};
            hsw_msm a = col.args(300, c, 64);
            a.input_rows = rows;
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3 && rep.launches == 3);
            CHECK(rep.window_bits == c && rep.windows == (254 + c - 1) / c && rep.slice_rows == 64 && rep.slices == 5 && rep.columns == 3);
            CHECK(rep.scratch_bytes == 3ull * rep.windows * 5 * ((1u << c) - 1) * 96 && rep.first_refused == ~0ull && rep.first_bad_base == ~0ull);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);          // one scratch, replaced when it grows
            for (uint32_t s : col.status) CHECK(s == 0);
        }
        {   // no row at all: no check launch, the identity everywhere
            Columns col(2, 300);
            const uint64_t rows[2] = {0, 0};
            hsw_msm a = col.args(300);
            a.input_rows = rows;
            a.status = nullptr;                                              // (no status array: allowed)
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 2 && rep.launches == 2 && rep.slices == 1);
        }
        {   // the default slice doubles until a column has at most 1024 of them
            Columns col(1, 1ull << 23);
            const hsw_msm a = col.args(1ull << 23);
            CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.slice_rows == 8192 && rep.slices == 1024 && rep.launches == 3);
            CHECK(rep.scratch_bytes == 32ull * 1024 * 255 * 96);
            const size_t live1 = hip_stub_live_device_allocations();
            Columns small(2, 300);                                           // a smaller call: the scratch is large enough
            const hsw_msm b = small.args(300);
            CHECK(hsw_gadget_msm(g, &b, &rep) == HSW_OK && hip_stub_live_device_allocations() == live1);
        }
        {   // 2^20 rows in slices of 4096: 191 MiB of partial buckets per column -- seven columns go in groups of five
            Columns col(7, 1ull << 20);
            const hsw_msm a = col.args(1ull << 20);
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.slices == 256 && rep.launches == 5 && hip_stub_launches() == l0 + 5);
            CHECK(rep.scratch_bytes == 5ull * 32 * 256 * 255 * 96 && rep.scratch_bytes <= 1ull << 30 && rep.columns == 7);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);
        }
        CHECK(hip_stub_live_events() > 0);                                   // (the engine's own)
        hsw_gadget_destroy(g);                                               // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live0 + 1);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- "round_scratch": six columns of 5 slices x 32 windows x 255 buckets x 96 bytes on a gadget of their own
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        const int64_t column = 5 * 32 * 255 * 96;                            // 3,916,800 bytes
        CHECK(hsw_engine_set_option(e, "round_scratch", 0) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "round_scratch must be 1 .. 2^30 bytes"));
        CHECK(hsw_engine_set_option(e, "round_scratch", ((int64_t)1 << 30) + 1) == HSW_ERR_INVALID_ARG);
        Columns col(6, 300);
        const uint64_t rows[6] = {300, 65, 300, 0, 1, 299};
        hsw_msm a = col.args(300, 8, 64);
        a.input_rows = rows;
        CHECK(hsw_engine_set_option(e, "round_scratch", 2 * column) == HSW_OK);      // exactly two columns: three groups
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.launches == 1 + 2 * 3 && hip_stub_launches() == l0 + 7 && rep.scratch_bytes == 7833600 && rep.columns == 6);
        const size_t cap2 = g->scratch.cap;
        const void *d2 = g->scratch.d;
        CHECK(cap2 >= 7833600 && cap2 < 3 * (size_t)column && hip_stub_live_device_allocations() == live0 + 1);
        CHECK(hsw_engine_set_option(e, "round_scratch", 2 * column - 1) == HSW_OK);  // a byte short of two: six groups of one
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.launches == 1 + 2 * 6 && hip_stub_launches() == l0 + 13 && rep.scratch_bytes == 3916800);
        CHECK(g->scratch.cap == cap2 && g->scratch.d == d2);                 // (a smaller need: the scratch as it was)
        CHECK(hsw_engine_set_option(e, "round_scratch", 1) == HSW_OK);               // below one column: a group is one column still
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.launches == 13 && hip_stub_launches() == l0 + 13 && rep.scratch_bytes == 3916800);
        CHECK(hsw_engine_set_option(e, "round_scratch", (int64_t)1 << 30) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.launches == 3 && hip_stub_launches() == l0 + 3 && rep.scratch_bytes == 23500800);
        const size_t cap6 = g->scratch.cap;
        const void *d6 = g->scratch.d;
        CHECK(cap6 == cap2 + 4 * (size_t)column && hip_stub_live_device_allocations() == live0 + 1);   // grown by four columns: replaced, not added to
        CHECK(hsw_engine_set_option(e, "round_scratch", 2 * column) == HSW_OK);
        CHECK(hsw_gadget_msm(g, &a, &rep) == HSW_OK && rep.launches == 7 && rep.scratch_bytes == 7833600 && g->scratch.cap == cap6 && g->scratch.d == d6);
        CHECK(hsw_engine_set_option(e, "round_scratch", (int64_t)1 << 30) == HSW_OK);
        for (uint32_t s : col.status) CHECK(s == 0);
        hsw_gadget_destroy(g);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("msm lifecycle ok\n");
    return 0;
}
