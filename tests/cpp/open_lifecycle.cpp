// hsw_gadget_evaluate and hsw_gadget_open on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the
// stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every
// refusal that is decided before a launch, with its status and its hsw_last_error (and that it launches nothing,
// allocates nothing and writes neither out_evals nor status); what the report says of the geometry per (rows,
// tile_rows); the launches -- two per batch of columns, three per batch of groups; the growth and the reuse of the
// scratch that both calls share; the batches of groups under 1 GiB of scratch, and the batches of both calls under what
// the engine option "round_scratch" lowers that to; no device allocation and no event left at the end.  The columns and the quotients are addresses only: no launch runs, so nothing reads or writes them, and
// the evaluations the host tail copies out of the unwritten scratch are not looked at.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_gadget.hpp"
#include "../../halo2-dynamic-sha256_amd/csrc/hsw_open_value.hpp"
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

// n columns of `rows` cells and their addresses; n_out quotients behind them
struct Call {
    uint64_t rows;
    std::vector<const void *> in;
    std::vector<void *> quot;
    std::vector<uint8_t> points, challenges, evals;
    std::vector<uint32_t> status, qc, qp, gcols;
    std::vector<uint64_t> gfirst;
    Call(size_t n, uint64_t rows_, size_t n_items, size_t m) : rows(rows_), points(32 * n_items, 0), challenges(32 * n_items, 0), evals(32 * n_items, 0xA5),
                                                               status(n > n_items ? n : n_items, 0xFFFFFFFFu) {
        for (size_t b = 0; b < n; b++) in.push_back(reinterpret_cast<const void *>((uintptr_t)0x100000000000ull + b * 32 * rows));
        for (size_t k = 0; k < n_items; k++) {
            quot.push_back(reinterpret_cast<void *>((uintptr_t)0x300000000000ull + k * 32 * rows));
            points[32 * k] = (uint8_t)(k + 2);
            challenges[32 * k] = (uint8_t)(k + 3);
            qc.push_back((uint32_t)(k % n));
            qp.push_back((uint32_t)k);
            gfirst.push_back(k * m);
            for (size_t i = 0; i < m; i++) gcols.push_back((uint32_t)((k + i) % n));
        }
        gfirst.push_back(n_items * m);
    }
    hsw_evaluate evaluate(uint32_t tile_rows = 0) {
        return hsw_evaluate{0, tile_rows, rows, in.size(), in.data(), nullptr, qp.size(), points.data(), qc.size(), qc.data(), qp.data(), evals.data(), status.data()};
    }
    hsw_open open(uint32_t tile_rows = 0) {
        return hsw_open{0, tile_rows, rows, in.size(), in.data(), nullptr, quot.size(), gfirst.data(), gcols.data(), points.data(), challenges.data(),
                        quot.data(), evals.data(), status.data()};
    }
    bool untouched() const {
        for (uint8_t x : evals) if (x != 0xA5) return false;
        for (uint32_t x : status) if (x != 0xFFFFFFFFu) return false;
        return true;
    }
};

static bool refused_evaluate(hsw_engine *e, hsw_gadget *g, const hsw_evaluate &a, const Call &call, int status, const char *text) {
    hsw_evaluate_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    const int rc = hsw_gadget_evaluate(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "evaluate: got %d (%s), expected %d (...%s...)\n", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.launches == 0 && rep.columns == 0 && call.untouched();
}
static bool refused_open(hsw_engine *e, hsw_gadget *g, const hsw_open &a, const Call &call, int status, const char *text) {
    hsw_open_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    const int rc = hsw_gadget_open(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "open: got %d (%s), expected %d (...%s...)\n", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.launches == 0 && rep.groups == 0 && call.untouched();
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_evaluate) == 96 && sizeof(hsw_evaluate_report) == 72 && sizeof(hsw_open) == 104 && sizeof(hsw_open_report) == 72);
    CHECK(HSW_OPEN_CELL_NOT_BELOW_P == hsw::OPEN_CELL_NOT_BELOW_P && HSW_OPEN_CELL_NOT_BELOW_P == HSW_NTT_CELL_NOT_BELOW_P);
    CHECK(HSW_OPEN_MIN_TILE_ROWS == hsw::OPEN_MIN_TILE_ROWS && HSW_OPEN_MIN_TILE_ROWS <= 256 && HSW_OPEN_THREAD_ROWS == hsw::OPEN_ROWS);
    hsw_evaluate_report erep;
    hsw_open_report orep;
    {   // ---- a linear block-stream gadget evaluates and opens too; in 8-byte cells: refused, nothing launched
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        Call call(2, 300, 2, 1);
        const hsw_evaluate ea = call.evaluate();
        const hsw_open oa = call.open();
        CHECK(hsw_gadget_evaluate(g, &ea, &erep) == HSW_OK && erep.columns == 2 && erep.queries == 2 && erep.launches == 2 && erep.tile_rows == 2048 && erep.tiles == 1);
        CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.groups == 2 && orep.launches == 3 && orep.batches == 1 && orep.written == 600 && orep.thread_rows == 8);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        Call fresh(2, 300, 2, 1);
        CHECK(refused_evaluate(e, g, fresh.evaluate(), fresh, HSW_ERR_UNSUPPORTED, "32-byte"));
        CHECK(refused_open(e, g, fresh.open(), fresh, HSW_ERR_UNSUPPORTED, "32-byte"));
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
        Call call(3, 300, 2, 2);
        const hsw_evaluate eok = call.evaluate(256);
        const hsw_open ook = call.open(256);
        hsw_evaluate eb = eok;
        hsw_open ob = ook;
        CHECK(hsw_gadget_evaluate(nullptr, &eok, &erep) == HSW_ERR_INVALID_ARG && hsw_gadget_evaluate(g, nullptr, &erep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_evaluate(g, &eok, nullptr) == HSW_ERR_INVALID_ARG && call.untouched());
        CHECK(hsw_gadget_open(nullptr, &ook, &orep) == HSW_ERR_INVALID_ARG && hsw_gadget_open(g, nullptr, &orep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_open(g, &ook, nullptr) == HSW_ERR_INVALID_ARG && call.untouched());
        // what both calls share
        for (uint64_t rows : {(uint64_t)0, ((uint64_t)1 << 28) + 1}) {
            eb = eok; eb.rows = rows; ob = ook; ob.rows = rows;
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "rows is 1 .. 2^28") && refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "rows is 1 .. 2^28"));
        }
        for (uint32_t t : {128u, 255u, 384u, 1u << 21}) {
            eb = eok; eb.tile_rows = t; ob = ook; ob.tile_rows = t;
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "tile_rows 0 or a power of two") && refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "tile_rows 0 or a power of two"));
        }
        eb = eok; eb.flags = 1; ob = ook; ob.flags = 1;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "unknown flag") && refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "unknown flag"));
        eb = eok; eb.n_columns = 0; ob = ook; ob.n_columns = 0;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "n_columns is at least 1") && refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "n_columns is at least 1"));
        eb = eok; eb.d_columns = nullptr; ob = ook; ob.d_columns = nullptr;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "pointer array is NULL") && refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        for (int how = 0; how < 2; how++) {
            std::vector<const void *> ip(call.in);
            ip[1] = how ? static_cast<const uint8_t *>(ip[1]) + 8 : nullptr;
            eb = eok; eb.d_columns = ip.data(); ob = ook; ob.d_columns = ip.data();
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "column 1: a pointer that is NULL or not 16-byte aligned"));
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "column 1: a pointer that is NULL or not 16-byte aligned"));
        }
        {
            const uint64_t rows[3] = {300, 0, 301};
            eb = eok; eb.input_rows = rows; ob = ook; ob.input_rows = rows;
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "column 2: input_rows above rows") && refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "column 2: input_rows above rows"));
        }
        // evaluate's own
        eb = eok; eb.n_points = 0;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "n_points is at least 1"));
        eb = eok; eb.n_queries = 0;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "n_queries is at least 1"));
        eb = eok; eb.points = nullptr;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "points is NULL"));
        eb = eok; eb.query_column = nullptr;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "query index array is NULL"));
        eb = eok; eb.query_point = nullptr;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "query index array is NULL"));
        eb = eok; eb.out_evals = nullptr;
        CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "out_evals is NULL"));
        {
            const uint32_t qc[2] = {0, 3}, qp[2] = {2, 1};
            eb = eok; eb.query_column = qc;
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "query 1: its column index is out of range"));
            eb = eok; eb.query_point = qp;
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "query 0: its point index is out of range"));
            std::vector<uint8_t> pts(call.points);
            std::memcpy(pts.data() + 32, P_BYTES, 32);
            eb = eok; eb.points = pts.data();
            CHECK(refused_evaluate(e, g, eb, call, HSW_ERR_INVALID_ARG, "point 1: its stored limbs are not below p"));
        }
        // open's own
        ob = ook; ob.n_groups = 0;
        CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "n_groups is at least 1"));
        ob = ook; ob.group_first = nullptr;
        CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group index array is NULL"));
        ob = ook; ob.group_columns = nullptr;
        CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group index array is NULL"));
        ob = ook; ob.points = nullptr;
        CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "points or challenges is NULL"));
        ob = ook; ob.challenges = nullptr;
        CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "points or challenges is NULL"));
        ob = ook; ob.d_quotients = nullptr;
        CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "quotient pointer array is NULL"));
        {
            const uint64_t empty[3] = {0, 2, 2}, shifted[3] = {1, 2, 4};
            ob = ook; ob.group_first = empty;
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 1: an empty group"));
            ob = ook; ob.group_first = shifted;
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group_first[0] is 0"));
            const uint32_t cols[4] = {0, 1, 1, 3};
            ob = ook; ob.group_columns = cols;
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 1: a column index out of range"));
            std::vector<uint8_t> bad(call.points);
            std::memcpy(bad.data(), P_BYTES, 32);
            ob = ook; ob.points = bad.data();
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 0: a point whose stored limbs are not below p"));
            bad = call.challenges;
            std::memcpy(bad.data() + 32, P_BYTES, 32);
            ob = ook; ob.challenges = bad.data();
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 1: a challenge whose stored limbs are not below p"));
        }
        for (int how = 0; how < 2; how++) {
            std::vector<void *> qp(call.quot);
            qp[1] = how ? static_cast<void *>(static_cast<uint8_t *>(qp[1]) + 8) : nullptr;
            ob = ook; ob.d_quotients = qp.data();
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 1: a quotient pointer that is NULL or not 16-byte aligned"));
        }
        {   // overlaps: with the last row of a column, with another quotient; a column counts with all its rows, read or not
            std::vector<void *> qp(call.quot);
            qp[0] = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.in[2]) + 32 * 299);
            ob = ook; ob.d_quotients = qp.data();
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 0: its quotient overlaps a column or another quotient"));
            qp = call.quot;
            qp[1] = static_cast<uint8_t *>(qp[0]) + 32 * 299;
            ob = ook; ob.d_quotients = qp.data();
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 1: its quotient overlaps a column or another quotient"));
            qp = call.quot;
            qp[0] = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.in[2]) + 32 * 299);
            const uint64_t rows[3] = {300, 300, 0};
            ob = ook; ob.d_quotients = qp.data(); ob.input_rows = rows;
            CHECK(refused_open(e, g, ob, call, HSW_ERR_INVALID_ARG, "group 0: its quotient overlaps a column or another quotient"));
            qp[0] = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.in[2]) + 32 * 300);   // right behind the last column: allowed
            ob.d_quotients = qp.data();
            Call fresh(3, 300, 2, 2);
            ob.out_evals = fresh.evals.data(); ob.status = nullptr;          // (no status array: allowed)
            CHECK(hsw_gadget_open(g, &ob, &orep) == HSW_OK && orep.launches == 3);
        }
        CHECK(hip_stub_live_device_allocations() > 0);                       // (the gadget's own)
        hsw_gadget_destroy(g);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- the geometry in the report; launches; the scratch grows once and is reused by both calls; batches
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        const uint32_t tiles[] = {0, 256, 512, 4096, 1u << 20};
        for (uint32_t t : tiles) {
            Call call(3, 70000, 4, 2);
            const hsw_evaluate ea = call.evaluate(t);
            const hsw_open oa = call.open(t);
            const uint32_t used = t ? t : 2048, n_tiles = (70000 + used - 1) / used;
            int l0 = hip_stub_launches();
            CHECK(hsw_gadget_evaluate(g, &ea, &erep) == HSW_OK && hip_stub_launches() == l0 + 2 && erep.launches == 2);
            CHECK(erep.tile_rows == used && erep.tiles == n_tiles && erep.thread_rows == 8 && erep.columns == 3 && erep.queries == 4);
            CHECK(erep.scratch_bytes == 4ull * n_tiles * 32 && erep.first_refused == ~0ull && erep.refused_columns == 0 && erep.refused_queries == 0);
            l0 = hip_stub_launches();
            CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && hip_stub_launches() == l0 + 3 && orep.launches == 3 && orep.batches == 1);
            CHECK(orep.tile_rows == used && orep.tiles == n_tiles && orep.groups == 4 && orep.written == 4 * 70000ull && orep.first_refused == ~0ull);
            const uint64_t per_group = 32ull * n_tiles + ((32ull * 8750 + 255) & ~255ull) + ((32ull * 70000 + 255) & ~255ull);
            CHECK(orep.scratch_bytes == ((4 * per_group + 255) & ~255ull));
            CHECK(hip_stub_live_device_allocations() == live0 + 1);          // one scratch, replaced when it grows
            for (uint32_t s : call.status) CHECK(s == 0);
        }
        {   // a group of one column keeps no folded column; duplicate queries share an item
            Call call(3, 70000, 4, 1);
            const hsw_open oa = call.open();
            CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.scratch_bytes == ((4 * (32ull * 35 + ((32ull * 8750 + 255) & ~255ull)) + 255) & ~255ull));
            call.qc = {1, 1, 1, 1};
            call.qp = {2, 0, 2, 2};
            const hsw_evaluate ea = call.evaluate();
            CHECK(hsw_gadget_evaluate(g, &ea, &erep) == HSW_OK && erep.scratch_bytes == 2ull * 35 * 32 && erep.queries == 4);
        }
        {   // 2^20 rows: a folded group holds 36 MiB and 16 KiB of scratch -- thirty groups go in batches of 28 and 2
            Call call(2, 1ull << 20, 30, 2);
            const hsw_open oa = call.open();
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.batches == 2 && orep.launches == 6 && hip_stub_launches() == l0 + 6);
            const uint64_t per_group = 32ull * 512 + 32ull * (1u << 17) + 32ull * (1u << 20);
            CHECK(orep.scratch_bytes == 28 * per_group && orep.scratch_bytes <= 1ull << 30 && 29 * per_group > 1ull << 30 && orep.groups == 30);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);
            const size_t live1 = hip_stub_live_device_allocations();
            Call small(2, 300, 2, 1);                                        // a smaller call of either kind: the scratch is large enough
            const hsw_open ob = small.open();
            const hsw_evaluate eb = small.evaluate();
            CHECK(hsw_gadget_open(g, &ob, &orep) == HSW_OK && hsw_gadget_evaluate(g, &eb, &erep) == HSW_OK && hip_stub_live_device_allocations() == live1);
        }
        {   // one group larger than 1 GiB is a batch of its own
            Call call(2, 1ull << 25, 2, 2);
            const hsw_open oa = call.open();
            CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.batches == 2 && orep.launches == 6 && orep.scratch_bytes > 1ull << 30);
        }
        CHECK(hip_stub_live_events() > 0);                                   // (the engine's own)
        hsw_gadget_destroy(g);                                               // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live0 + 1);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- "round_scratch": 773 rows in tiles of 256 -- 4 tiles, 128 bytes an item -- on a gadget of their own
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        CHECK(hsw_engine_set_option(e, "round_scratch", 0) == HSW_ERR_INVALID_ARG && std::strstr(hsw_last_error(e), "round_scratch must be 1 .. 2^30 bytes"));
        CHECK(hsw_engine_set_option(e, "round_scratch", ((int64_t)1 << 30) + 1) == HSW_ERR_INVALID_ARG);
        // evaluate: five columns of 1, 3, 0, 2 and 1 queries, listed in an order that interleaves the columns
        Call call(5, 773, 8, 1);
        call.qc = {1, 0, 3, 1, 4, 3, 1, 1};                                  // (the last one a duplicate: seven items)
        call.qp = {0, 1, 2, 3, 4, 5, 6, 6};
        const hsw_evaluate ea = call.evaluate(256);
        CHECK(hsw_engine_set_option(e, "round_scratch", 4 * 128) == HSW_OK); // four items: columns {0, 1} and {3, 4}
        int l0 = hip_stub_launches();
        CHECK(hsw_gadget_evaluate(g, &ea, &erep) == HSW_OK && erep.launches == 4 && hip_stub_launches() == l0 + 4 && erep.scratch_bytes == 512 && erep.tiles == 4);
        CHECK(erep.columns == 5 && erep.queries == 8);
        const size_t cap4 = g->scratch.cap;
        const void *d4 = g->scratch.d;
        CHECK(hsw_engine_set_option(e, "round_scratch", 1) == HSW_OK);       // below one item: a column with all its points, alone
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_evaluate(g, &ea, &erep) == HSW_OK && erep.launches == 8 && hip_stub_launches() == l0 + 8 && erep.scratch_bytes == 3 * 128);
        CHECK(g->scratch.cap == cap4 && g->scratch.d == d4);                 // (a smaller need: the scratch as it was)
        CHECK(hsw_engine_set_option(e, "round_scratch", (int64_t)1 << 30) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_evaluate(g, &ea, &erep) == HSW_OK && erep.launches == 2 && hip_stub_launches() == l0 + 2 && erep.scratch_bytes == 7 * 128);
        CHECK(g->scratch.cap == cap4 + 3 * 128 && hip_stub_live_device_allocations() == live0 + 1);   // grown by three items: replaced, not added to
        // open: six groups, folded ones of 2, 3 and 2 columns and single columns in turn; a folded group holds 128 + 3,328 +
        // 24,832 = 28,288 bytes (tiles, a cell per thread, c), a single one 128 + 3,328 = 3,456
        call.gfirst = {0, 2, 3, 6, 7, 9, 10};
        call.gcols = {0, 1, 2, 3, 4, 0, 1, 2, 3, 4};
        call.quot.resize(6); call.points.resize(32 * 6); call.challenges.resize(32 * 6);
        const hsw_open oa = call.open(256);
        CHECK(hsw_engine_set_option(e, "round_scratch", 28288 + 3456) == HSW_OK);   // a folded group and the single one behind it
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.batches == 3 && orep.launches == 9 && hip_stub_launches() == l0 + 9 && orep.scratch_bytes == 31744);
        CHECK(orep.groups == 6 && orep.written == 6 * 773 && orep.tiles == 4);
        const size_t cap_pair = g->scratch.cap;
        const void *d_pair = g->scratch.d;
        CHECK(cap_pair > cap4 + 3 * 128);
        CHECK(hsw_engine_set_option(e, "round_scratch", 28288 + 3456 - 1) == HSW_OK);   // a byte short: every group alone
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.batches == 6 && orep.launches == 18 && hip_stub_launches() == l0 + 18 && orep.scratch_bytes == 28416);
        CHECK(hsw_engine_set_option(e, "round_scratch", 1) == HSW_OK);
        CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.batches == 6 && orep.launches == 18 && orep.scratch_bytes == 28416);
        CHECK(g->scratch.cap == cap_pair && g->scratch.d == d_pair);
        CHECK(hsw_engine_set_option(e, "round_scratch", (int64_t)1 << 30) == HSW_OK);
        l0 = hip_stub_launches();
        CHECK(hsw_gadget_open(g, &oa, &orep) == HSW_OK && orep.batches == 1 && orep.launches == 3 && hip_stub_launches() == l0 + 3);
        CHECK(orep.scratch_bytes == 3 * 28288 + 3 * 3456);                   // 95,232, a multiple of 256 as it is
        CHECK(g->scratch.cap == cap_pair + (95232 - 31744) && hip_stub_live_device_allocations() == live0 + 1);
        hsw_gadget_destroy(g);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("open lifecycle ok\n");
    return 0;
}
