// hsw_gadget_shplonk_quotient and hsw_gadget_shplonk_open on the host side under AddressSanitizer + UBSan +
// LeakSanitizer, against the stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing).
// Checked here: every refusal that is decided before a launch, with its status and its hsw_last_error (and that it
// launches nothing, allocates nothing and does not write the status word); what the report says of the geometry per
// (rows, tile_rows); three launches per call; the size, the growth and the reuse of the scratch; no device allocation
// and no event left at the end.  The columns, h and the output are addresses only: no launch runs, so nothing reads or
// writes them.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_shplonk_value.hpp"
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

static const uint8_t P_BYTES[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                    0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};   // p itself: not below p

// n columns of `rows` cells as addresses; the sets ({0, 1} at {z0}), ({2} at {z0, z1}), ({3} at {z0, z1, z2}) by default
struct Call {
    uint64_t rows;
    std::vector<const void *> in;
    std::vector<uint8_t> points, y, v, u;
    std::vector<uint64_t> first, pfirst;
    std::vector<uint32_t> cols, pts;
    void *h, *out;
    uint32_t status;
    explicit Call(uint64_t rows_, size_t n = 4) : rows(rows_), points(32 * 3, 0), y(32, 0), v(32, 0), u(32, 0), first{0, 2, 3, 4}, pfirst{0, 1, 3, 6},
                                                 cols{0, 1, 2, 3}, pts{0, 0, 1, 0, 1, 2}, status(0xFFFFFFFFu) {
        for (size_t b = 0; b < n; b++) in.push_back(reinterpret_cast<const void *>((uintptr_t)0x100000000000ull + b * 32 * rows));
        h = reinterpret_cast<void *>((uintptr_t)0x200000000000ull);
        out = reinterpret_cast<void *>((uintptr_t)0x300000000000ull);
        for (int k = 0; k < 3; k++) points[32 * k] = (uint8_t)(k + 2);
        y[0] = 7; v[0] = 9; u[0] = 11;
    }
    hsw_shplonk quotient(uint32_t tile_rows = 0) {
        return hsw_shplonk{0, tile_rows, rows, in.size(), in.data(), nullptr, points.size() / 32, points.data(), first.size() - 1, first.data(), cols.data(),
                           pfirst.data(), pts.data(), y.data(), v.data(), nullptr, nullptr, out, &status};
    }
    hsw_shplonk open(uint32_t tile_rows = 0) {
        hsw_shplonk a = quotient(tile_rows);
        a.u = u.data(); a.d_h = h;
        return a;
    }
};

static bool refused(hsw_engine *e, hsw_gadget *g, const hsw_shplonk &a, bool open, int status, const char *text) {
    hsw_shplonk_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    if (a.status) *a.status = 0xFFFFFFFFu;
    const int rc = open ? hsw_gadget_shplonk_open(g, &a, &rep) : hsw_gadget_shplonk_quotient(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "%s: got %d (%s), expected %d (...%s...)\n", open ? "open" : "quotient", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.launches == 0 && rep.sets == 0 && (!a.status || *a.status == 0xFFFFFFFFu);
}
// refused by both calls alike
static bool refused_both(hsw_engine *e, hsw_gadget *g, hsw_shplonk q, hsw_shplonk o, int status, const char *text) {
    return refused(e, g, q, false, status, text) && refused(e, g, o, true, status, text);
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_shplonk) == 144 && sizeof(hsw_shplonk_report) == 72);
    CHECK(HSW_SHPLONK_CELL_NOT_BELOW_P == hsw::SHPLONK_CELL_NOT_BELOW_P && HSW_SHPLONK_CELL_NOT_BELOW_P == HSW_NTT_CELL_NOT_BELOW_P);
    CHECK(HSW_SHPLONK_MAX_SET_POINTS == hsw::SHPLONK_MAX_SET_POINTS && HSW_OPEN_THREAD_ROWS == hsw::OPEN_ROWS);
    hsw_shplonk_report rep;
    {   // ---- a linear block-stream gadget opens too; in 8-byte cells: refused, nothing launched
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        Call call(300);
        const hsw_shplonk qa = call.quotient(), oa = call.open();
        CHECK(hsw_gadget_shplonk_quotient(g, &qa, &rep) == HSW_OK && rep.sets == 3 && rep.items == 6 && rep.columns == 4 && rep.launches == 3 && rep.tile_rows == 2048);
        CHECK(rep.tiles == 1 && rep.written == 300 && rep.refused == 0 && rep.thread_rows == 8 && call.status == 0);
        CHECK(hsw_gadget_shplonk_open(g, &oa, &rep) == HSW_OK && rep.sets == 3 && rep.items == 6 && rep.columns == 5 && rep.launches == 3 && rep.written == 300);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        Call fresh(300);
        CHECK(refused_both(e, g, fresh.quotient(), fresh.open(), HSW_ERR_UNSUPPORTED, "32-byte"));
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
        Call call(300);
        const hsw_shplonk qok = call.quotient(256), ook = call.open(256);
        hsw_shplonk qb = qok, ob = ook;
        CHECK(hsw_gadget_shplonk_quotient(nullptr, &qok, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_shplonk_quotient(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_shplonk_quotient(g, &qok, nullptr) == HSW_ERR_INVALID_ARG && hsw_gadget_shplonk_open(nullptr, &ook, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_shplonk_open(g, nullptr, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_shplonk_open(g, &ook, nullptr) == HSW_ERR_INVALID_ARG);
        for (uint64_t rows : {(uint64_t)0, ((uint64_t)1 << 28) + 1}) {
            qb = qok; qb.rows = rows; ob = ook; ob.rows = rows;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "rows is 1 .. 2^28"));
        }
        for (uint32_t t : {128u, 255u, 384u, 1u << 21}) {
            qb = qok; qb.tile_rows = t; ob = ook; ob.tile_rows = t;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "tile_rows 0 or a power of two"));
        }
        qb = qok; qb.flags = 1; ob = ook; ob.flags = 2;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "unknown flag"));
        qb = qok; qb.n_columns = 0; ob = ook; ob.n_columns = 0;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "n_columns is at least 1"));
        qb = qok; qb.d_columns = nullptr; ob = ook; ob.d_columns = nullptr;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        for (int how = 0; how < 2; how++) {
            std::vector<const void *> ip(call.in);
            ip[1] = how ? static_cast<const uint8_t *>(ip[1]) + 8 : nullptr;
            qb = qok; qb.d_columns = ip.data(); ob = ook; ob.d_columns = ip.data();
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "column 1: a pointer that is NULL or not 16-byte aligned"));
        }
        {
            const uint64_t rows[4] = {300, 0, 301, 300};
            qb = qok; qb.input_rows = rows; ob = ook; ob.input_rows = rows;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "column 2: input_rows above rows"));
        }
        qb = qok; qb.n_points = 0; ob = ook; ob.n_points = 0;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "n_points is at least 1"));
        qb = qok; qb.n_sets = 0; ob = ook; ob.n_sets = 0;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "n_sets is at least 1"));
        qb = qok; qb.n_sets = 65536; ob = ook; ob.n_sets = 65536;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "n_sets is at most 65535"));
        qb = qok; qb.points = nullptr; ob = ook; ob.points = nullptr;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "points is NULL"));
        qb = qok; qb.set_first = nullptr; ob = ook; ob.set_columns = nullptr;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "a set index array is NULL"));
        qb = qok; qb.set_point_first = nullptr; ob = ook; ob.set_points = nullptr;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "a set index array is NULL"));
        qb = qok; qb.y = nullptr; ob = ook; ob.v = nullptr;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "y or v is NULL"));
        qb = qok; qb.d_out = nullptr; ob = ook; ob.d_out = static_cast<uint8_t *>(call.out) + 8;
        CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "d_out is NULL or not 16-byte aligned"));
        // what tells the two calls apart
        qb = qok; qb.u = call.u.data();
        CHECK(refused(e, g, qb, false, HSW_ERR_INVALID_ARG, "u and d_h are NULL for hsw_gadget_shplonk_quotient"));
        qb = qok; qb.d_h = call.h;
        CHECK(refused(e, g, qb, false, HSW_ERR_INVALID_ARG, "u and d_h are NULL for hsw_gadget_shplonk_quotient"));
        ob = ook; ob.u = nullptr;
        CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "u is NULL"));
        ob = ook; ob.d_h = nullptr;
        CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "d_h is NULL or not 16-byte aligned"));
        ob = ook; ob.d_h = static_cast<uint8_t *>(call.h) + 4;
        CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "d_h is NULL or not 16-byte aligned"));
        {   // points and challenges not below p
            std::vector<uint8_t> bad(call.points);
            std::memcpy(bad.data() + 32, P_BYTES, 32);
            qb = qok; qb.points = bad.data(); ob = ook; ob.points = bad.data();
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "point 1: its stored limbs are not below p"));
            qb = qok; qb.y = P_BYTES; ob = ook; ob.y = P_BYTES;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "y: its stored limbs are not below p"));
            qb = qok; qb.v = P_BYTES; ob = ook; ob.v = P_BYTES;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "v: its stored limbs are not below p"));
            ob = ook; ob.u = P_BYTES;
            CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "u: its stored limbs are not below p"));
        }
        {   // the sets
            const uint64_t shifted[4] = {1, 2, 3, 4}, empty[4] = {0, 2, 2, 4}, no_point[4] = {0, 1, 1, 6};
            qb = qok; qb.set_first = shifted; ob = ook; ob.set_point_first = shifted;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set_first[0] and set_point_first[0] are 0"));
            qb = qok; qb.set_first = empty; ob = ook; ob.set_first = empty;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 1: no column"));
            qb = qok; qb.set_point_first = no_point; ob = ook; ob.set_point_first = no_point;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 1: no point"));
            const uint32_t range[4] = {0, 1, 4, 3}, twice_in_one[4] = {0, 0, 2, 3}, twice_in_two[4] = {0, 1, 2, 1};
            qb = qok; qb.set_columns = range; ob = ook; ob.set_columns = range;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 1: a column index out of range"));
            qb = qok; qb.set_columns = twice_in_one; ob = ook; ob.set_columns = twice_in_one;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 0: a column listed twice"));
            qb = qok; qb.set_columns = twice_in_two; ob = ook; ob.set_columns = twice_in_two;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 2: a column listed twice"));
            const uint32_t p_range[6] = {0, 0, 3, 0, 1, 2}, p_twice[6] = {0, 0, 1, 0, 2, 0}, p_unused[6] = {0, 0, 1, 0, 1, 1};
            qb = qok; qb.set_points = p_range; ob = ook; ob.set_points = p_range;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 1: a point index out of range"));
            qb = qok; qb.set_points = p_twice; ob = ook; ob.set_points = p_twice;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 2: a point index twice"));
            qb = qok; qb.set_points = p_unused; ob = ook; ob.set_points = p_unused;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 2: a point index twice"));
            const uint32_t p_two[6] = {0, 0, 1, 0, 1, 1};
            const uint64_t pf_two[4] = {0, 1, 3, 5};                          // the third set: {z0, z1}; z2 is used by none
            qb = qok; qb.set_points = p_two; qb.set_point_first = pf_two; ob = ook; ob.set_points = p_two; ob.set_point_first = pf_two;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "point 2: no set uses it"));
            std::vector<uint8_t> same(call.points);
            std::memcpy(same.data() + 64, same.data(), 32);
            qb = qok; qb.points = same.data(); ob = ook; ob.points = same.data();
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "equal in value to another point"));
            // seventeen points in one set
            std::vector<uint8_t> many(32 * 17, 0);
            for (int k = 0; k < 17; k++) many[32 * k] = (uint8_t)(k + 1);
            const uint64_t f1[2] = {0, 1}, pf1[2] = {0, 17};
            uint32_t p17[17];
            for (uint32_t k = 0; k < 17; k++) p17[k] = k;
            qb = qok; qb.n_sets = 1; qb.set_first = f1; qb.set_point_first = pf1; qb.set_points = p17; qb.n_points = 17; qb.points = many.data();
            ob = qb; ob.u = call.u.data(); ob.d_h = call.h;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "set 0: more than HSW_SHPLONK_MAX_SET_POINTS points"));
            const uint64_t pf16[2] = {0, 16};
            qb.set_point_first = pf16; qb.n_points = 16;                      // sixteen: allowed
            CHECK(hsw_gadget_shplonk_quotient(g, &qb, &rep) == HSW_OK && rep.items == 16 && rep.sets == 1);
        }
        {   // overlaps: with the last row of a column (read or not), with h; right behind a column: allowed
            qb = qok; qb.d_out = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.in[2]) + 32 * 299);
            ob = ook; ob.d_out = qb.d_out;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "column 2: d_out overlaps it"));
            const uint64_t rows[4] = {300, 300, 0, 300};
            qb.input_rows = rows; ob.input_rows = rows;
            CHECK(refused_both(e, g, qb, ob, HSW_ERR_INVALID_ARG, "column 2: d_out overlaps it"));
            ob = ook; ob.d_out = static_cast<uint8_t *>(call.h) + 32 * 299;
            CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "d_out overlaps d_h"));
            ob = ook; ob.d_h = static_cast<uint8_t *>(call.out) + 32 * 299;
            CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "d_out overlaps d_h"));
            qb = qok; qb.d_out = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.in[3]) + 32 * 300); qb.status = nullptr;   // (no status word: allowed)
            CHECK(hsw_gadget_shplonk_quotient(g, &qb, &rep) == HSW_OK && rep.launches == 3);
        }
        {   // zd_0 = 0: u is a point of T outside the first set (z1 = 3); u = z0, inside it, is allowed
            std::vector<uint8_t> u(32, 0);
            u[0] = 3;
            ob = ook; ob.u = u.data();
            CHECK(refused(e, g, ob, true, HSW_ERR_INVALID_ARG, "zd_0 = 0"));
            u[0] = 2;
            CHECK(hsw_gadget_shplonk_open(g, &ob, &rep) == HSW_OK && rep.launches == 3);
        }
        CHECK(hip_stub_live_device_allocations() > 0);                       // (the gadget's own)
        hsw_gadget_destroy(g);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- the geometry in the report; launches; the scratch: its size, grown once, reused
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        const auto a256 = [](uint64_t x) { return (x + 255) & ~255ull; };
        const uint32_t tiles[] = {0, 256, 512, 4096, 1u << 20};
        uint64_t largest = 0;
        for (uint32_t t : tiles) {
            Call call(70000);
            const hsw_shplonk qa = call.quotient(t), oa = call.open(t);
            const uint32_t used = t ? t : 2048, n_tiles = (70000 + used - 1) / used;
            int l0 = hip_stub_launches();
            CHECK(hsw_gadget_shplonk_quotient(g, &qa, &rep) == HSW_OK && hip_stub_launches() == l0 + 3 && rep.launches == 3);
            CHECK(rep.tile_rows == used && rep.tiles == n_tiles && rep.thread_rows == 8 && rep.sets == 3 && rep.items == 6 && rep.columns == 4);
            CHECK(rep.written == 70000 && rep.refused == 0 && call.status == 0);
            // six items of tiles and seeds, ONE folded set (the first, of two columns), staging in front
            const uint64_t scratch = a256(6ull * n_tiles * 32) + a256(6ull * 8750 * 32) + a256(70000ull * 32);
            CHECK(rep.scratch_bytes >= scratch && rep.scratch_bytes < scratch + 3 * sizeof(hsw::OpenPoint) + 16 * 256);
            largest = rep.scratch_bytes > largest ? rep.scratch_bytes : largest;
            l0 = hip_stub_launches();
            CHECK(hsw_gadget_shplonk_open(g, &oa, &rep) == HSW_OK && hip_stub_launches() == l0 + 3 && rep.launches == 3 && rep.columns == 5);
            // one item, one folded set
            const uint64_t scratch2 = a256(1ull * n_tiles * 32) + a256(8750ull * 32) + a256(70000ull * 32);
            CHECK(rep.scratch_bytes >= scratch2 && rep.scratch_bytes < scratch2 + sizeof(hsw::OpenPoint) + 16 * 256);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);          // one scratch, replaced when it grows
        }
        {   // sets of one column keep no folded column
            Call call(70000);
            call.first = {0, 1, 2, 3};
            call.cols = {3, 1, 0};                                           // (column 2 is listed by no set: allowed)
            const hsw_shplonk qa = call.quotient();
            CHECK(hsw_gadget_shplonk_quotient(g, &qa, &rep) == HSW_OK && rep.columns == 3);
            const uint64_t scratch = a256(6ull * 35 * 32) + a256(6ull * 8750 * 32);
            CHECK(rep.scratch_bytes >= scratch && rep.scratch_bytes < scratch + 3 * sizeof(hsw::OpenPoint) + 16 * 256);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);
        }
        {   // a larger call grows the scratch; a smaller one of either kind reuses it
            Call big(1ull << 20);
            const hsw_shplonk qa = big.quotient();
            CHECK(hsw_gadget_shplonk_quotient(g, &qa, &rep) == HSW_OK && rep.scratch_bytes > largest && hip_stub_live_device_allocations() == live0 + 1);
            Call small(300);
            const hsw_shplonk qs = small.quotient(), os = small.open();
            CHECK(hsw_gadget_shplonk_quotient(g, &qs, &rep) == HSW_OK && hsw_gadget_shplonk_open(g, &os, &rep) == HSW_OK);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);
        }
        CHECK(hip_stub_live_events() > 0);                                   // (the engine's own)
        hsw_gadget_destroy(g);                                               // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live0 + 1);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("shplonk lifecycle ok\n");
    return 0;
}
