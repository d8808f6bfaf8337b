// hsw_gadget_create_contexts (K Contexts of M digests each) on the host side under AddressSanitizer + UBSan +
// LeakSanitizer, against the stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do
// nothing): the creation rules, create / declare / reset / re-declare / destroy, a failing declaration that leaves
// the layout as it was, destroy with a pass half issued -- and every position a group reports against ONE
// HSW_GADGET_SHARED_CONTEXT gadget of the same M sizes: the same (column, row) in every Context, the same image
// offset plus c * S.  Built and run by tests/test_context_groups_host.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/hsw.h"

extern "C" {
size_t hip_stub_live_device_allocations();
size_t hip_stub_live_pinned_allocations();
size_t hip_stub_live_events();
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static const uint32_t WHOLE = HSW_GADGET_WHOLE_DIGEST;
static const uint64_t MAX_ROWS = (1u << 17) - 9;
static const uint64_t FILL = 0x5a5a5a5a5a5a5a5aull;

struct Decl { size_t h; uint64_t column, row, lookups; };

// One pass of `n` digests (all of them, as one batch) on a gadget laid out at (column 1, row 777) with 5 queued
// lookups and the declarations `decl`; returns the results
static std::vector<hsw_hash_result> pass(hsw_gadget *g, size_t n, const std::vector<Decl> &decl) {
    uint64_t columns = 0;
    CHECK(hsw_gadget_set_origin(g, 1, 777, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_OK);
    for (const Decl &d : decl) CHECK(hsw_gadget_set_digest_origin(g, d.h, d.column, d.row, d.lookups) == HSW_OK);
    std::vector<uint8_t> msg(150, 7);
    std::vector<const uint8_t *> in(n, msg.data());
    std::vector<size_t> len(n), pre(n, 0);
    for (size_t i = 0; i < n; i++) len[i] = (i * 37) % 120;
    std::vector<hsw_hash_result> r(n);
    CHECK(hsw_gadget_digest_batch(g, n, in.data(), len.data(), pre.data(), r.data()) == HSW_OK);
    return r;
}

// Contexts 0 and K - 1 of a group against the single shared-context gadget of the same sizes
static void compare_with_single(hsw_engine *e, const size_t *sizes, size_t M, size_t K, bool interlude) {
    hsw_gadget *one = nullptr, *grp = nullptr;
    CHECK(hsw_gadget_create_ex(e, sizes, M, 1, WHOLE | HSW_GADGET_SHARED_CONTEXT, &one) == HSW_OK);
    CHECK(hsw_gadget_create_contexts(e, sizes, M, K, 1, WHOLE, &grp) == HSW_OK);
    std::vector<Decl> decl;
    if (interlude) {
        // where digest 0 ends follows from the sizes alone: a probe pass of one digest
        hsw_gadget *probe = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, M, 1, WHOLE | HSW_GADGET_SHARED_CONTEXT, &probe) == HSW_OK);
        const std::vector<hsw_hash_result> p = pass(probe, 1, {});
        uint64_t c = 0, r = 0;
        CHECK(hsw_gadget_cell_position(probe, p[0].end_cell - 1, &c, &r) == HSW_OK);
        hsw_gadget_view pv;
        CHECK(hsw_gadget_streams(probe, &pv) == HSW_OK);
        decl.push_back(Decl{1, c + 2, 31, pv.lookup_cells + 13});          // crosses column breaks, 13 caller lookups
        hsw_gadget_destroy(probe);
    }
    const std::vector<hsw_hash_result> r1 = pass(one, M, decl), rg = pass(grp, M * K, decl);
    hsw_gadget_view v1, vg;
    CHECK(hsw_gadget_streams(one, &v1) == HSW_OK && hsw_gadget_streams(grp, &vg) == HSW_OK);
    CHECK(v1.columns == vg.columns && v1.max_rows == vg.max_rows);
    const uint64_t S = vg.columns * vg.max_rows;
    hsw_context_region reg0, regc;
    CHECK(hsw_gadget_context_region(grp, 0, &reg0) == HSW_OK);
    CHECK(hsw_gadget_context_region(grp, K, &regc) == HSW_ERR_INVALID_ARG);
    const uint64_t C = reg0.stream_cells, Lp = reg0.lookup_cells;
    CHECK(C == r1[M - 1].end_cell && Lp == v1.lookup_cells && reg0.columns == vg.columns && reg0.max_rows == MAX_ROWS);
    CHECK(vg.gate_cells == K * C && vg.lookup_capacity == K * Lp);
    const size_t ctxs[2] = {0, K - 1};
    for (size_t c : ctxs) {
        CHECK(hsw_gadget_context_region(grp, c, &regc) == HSW_OK);
        CHECK(regc.assigned == 1 && regc.first_stream_cell == c * C && regc.stream_cells == C && regc.lookup_cells == Lp);
        CHECK(regc.d_image == (uint8_t *)vg.d_gate + c * S * HSW_CELL_BYTES);
        CHECK(regc.d_lookup == (uint8_t *)vg.d_lookup + c * Lp * HSW_CELL_BYTES);
        CHECK(regc.origin_column == 1 && regc.origin_row == 777 && regc.origin_lookups == 5);
        CHECK(regc.d_chip_dense == (uint8_t *)vg.d_chip_dense + c * regc.chip_rows * HSW_CELL_BYTES);
        for (size_t j = 0; j < M; j++) {
            const hsw_hash_result &a = r1[j], &b = rg[c * M + j];
            CHECK(b.first_block == c * (vg.capacity_blocks / K) + a.first_block && b.n_blocks == a.n_blocks);
            CHECK(b.prologue_cell == c * C + a.prologue_cell && b.block_cell == c * C + a.block_cell);
            CHECK(b.epilogue_cell == c * C + a.epilogue_cell && b.end_cell == c * C + a.end_cell);
            CHECK(b.prologue_lookup == c * Lp + a.prologue_lookup && b.block_lookup == c * Lp + a.block_lookup);
            CHECK(b.epilogue_lookup == c * Lp + a.epilogue_lookup);
            const uint64_t cells[5] = {a.prologue_cell, a.block_cell, a.block_cell + 66307, a.epilogue_cell, a.end_cell - 1};
            for (uint64_t cell : cells) {
                uint64_t c1 = 0, w1 = 0, cg = 0, wg = 0;
                CHECK(hsw_gadget_cell_position(one, cell, &c1, &w1) == HSW_OK);
                CHECK(hsw_gadget_cell_position(grp, c * C + cell, &cg, &wg) == HSW_OK);
                CHECK(c1 == cg && w1 == wg);
            }
            hsw_result_cells q1, qg;
            CHECK(hsw_gadget_result_cells(one, j, &q1) == HSW_OK && hsw_gadget_result_cells(grp, c * M + j, &qg) == HSW_OK);
            CHECK(qg.input_len_cell == c * C + q1.input_len_cell && qg.input_bytes_cell0 == c * C + q1.input_bytes_cell0);
            CHECK(qg.n_input_bytes == q1.n_input_bytes);
            CHECK(std::memcmp(q1.input_len_pos, qg.input_len_pos, sizeof q1.input_len_pos) == 0);
            CHECK(std::memcmp(q1.input_bytes_pos0, qg.input_bytes_pos0, sizeof q1.input_bytes_pos0) == 0);
            CHECK(std::memcmp(q1.output_byte_pos, qg.output_byte_pos, sizeof q1.output_byte_pos) == 0);
            for (int k = 0; k < 32; k++) CHECK(qg.output_byte_cells[k] == c * C + q1.output_byte_cells[k]);
        }
    }
    // image offsets through the deliveries: every cell the single gadget's download touches at offset i is touched at
    // c * S + i in Context c of the group's, and no other; the same for the lookup column at c * Lp
    std::vector<uint64_t> g1(S * 4, FILL), l1(v1.lookup_capacity * 4, FILL), gg(K * S * 4, FILL), lg(K * Lp * 4, FILL);
    std::vector<uint64_t> cd(2 * vg.chip_col_stride * 4), cs(2 * vg.chip_col_stride * 4);
    hsw_region_host d1 = {g1.data(), l1.data(), cd.data(), cs.data()}, dg = {gg.data(), lg.data(), cd.data(), cs.data()};
    CHECK(hsw_gadget_download_region(one, &d1) == HSW_OK && hsw_gadget_download_region(grp, &dg) == HSW_OK);
    for (size_t c : ctxs) {
        for (uint64_t i = 0; i < S; i++) CHECK((g1[4 * i] == FILL) == (gg[4 * (c * S + i)] == FILL));
        for (uint64_t i = 0; i < Lp; i++) CHECK((l1[4 * i] == FILL) == (lg[4 * (c * Lp + i)] == FILL));
    }
    // the distinct delivery replayed into sentinel-filled buffers writes exactly the same cells
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(grp, &tape) == HSW_OK && tape.gate_cells == K * C);
    std::vector<uint64_t> distinct(tape.n_distinct * 4 + 4);
    size_t n = 0;
    CHECK(hsw_gadget_download_region_distinct(grp, distinct.data(), tape.n_distinct, &n) == HSW_OK && n == tape.n_distinct);
    std::vector<uint64_t> g2(K * S * 4, FILL), l2(K * Lp * 4, FILL);
    hsw_region_host d2 = {g2.data(), l2.data(), cd.data(), cs.data()};
    CHECK(hsw_gadget_replay_region(grp, distinct.data(), &d2, 3) == HSW_OK);
    for (uint64_t i = 0; i < K * S; i++) CHECK((g2[4 * i] == FILL) == (gg[4 * i] == FILL));
    for (uint64_t i = 0; i < K * Lp; i++) CHECK((l2[4 * i] == FILL) == (lg[4 * i] == FILL));
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(grp, &rep) == HSW_OK);
    hsw_gadget_destroy(one);
    hsw_gadget_destroy(grp);
}

int main() {
    hsw_engine *e = nullptr, *e16 = nullptr, *edef = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    CHECK(hsw_abi_version() == 3);
    size_t sizes[3] = {192, 64, 128};
    hsw_gadget *g = nullptr;
    // ---- the creation rules
    CHECK(hsw_gadget_create_contexts(e, sizes, 3, 4, 1, 0, &g) == HSW_ERR_INVALID_ARG && !g);               // no whole-digest
    CHECK(hsw_gadget_create_contexts(e, sizes, 3, 4, 1, WHOLE | HSW_GADGET_INDEPENDENT, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_contexts(e, sizes, 3, 4, 1, WHOLE | HSW_GADGET_CONTEXT_IMAGES, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_contexts(e, sizes, 3, 4, 1, WHOLE | 0x100u, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_contexts(e, sizes, 0, 4, 1, WHOLE, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_contexts(e, sizes, 3, 0, 1, WHOLE, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_contexts(e, nullptr, 3, 4, 1, WHOLE, &g) == HSW_ERR_INVALID_ARG && !g);
    CHECK(hsw_gadget_create_contexts(nullptr, sizes, 3, 4, 1, WHOLE, &g) == HSW_ERR_INVALID_ARG);
    size_t odd[2] = {64, 100};
    CHECK(hsw_gadget_create_contexts(e, odd, 2, 2, 1, WHOLE, &g) == HSW_ERR_SHAPE && !g);                  // lib.rs:57-59
    CHECK(hsw_engine_create_ex(0, nullptr, 16, 1, HSW_MODE_HALO2_INTERNALS, &e16) == HSW_OK);
    CHECK(hsw_gadget_create_contexts(e16, sizes, 3, 4, 1, WHOLE, &g) == HSW_ERR_UNSUPPORTED && !g);          // 8-bit table only
    hsw_engine_destroy(e16);
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_DEFAULT, &edef) == HSW_OK);
    CHECK(hsw_gadget_create_contexts(edef, sizes, 3, 4, 1, WHOLE, &g) == HSW_ERR_INVALID_ARG && !g);         // not internals mode
    hsw_engine_destroy(edef);
    {   // one Context's blocks x limb_calls_per_block must fill whole chip rows: 3 columns, 1 block of 4120 calls
        hsw_engine *e3 = nullptr;
        CHECK(hsw_engine_create_ex(0, nullptr, 8, 3, HSW_MODE_HALO2_INTERNALS, &e3) == HSW_OK);
        size_t one_block[1] = {64}, three[1] = {192};
        CHECK(hsw_gadget_create_contexts(e3, one_block, 1, 2, 1, WHOLE, &g) == HSW_ERR_UNSUPPORTED && !g);
        CHECK(hsw_gadget_create_contexts(e3, three, 1, 2, 1, WHOLE, &g) == HSW_OK && g);
        hsw_gadget_destroy(g);
        g = nullptr;
        hsw_engine_destroy(e3);
    }
    // the flag rules of hsw_gadget_create_ex stay: the two modes still do not combine there
    CHECK(hsw_gadget_create_ex(e, sizes, 3, 1, WHOLE | HSW_GADGET_SHARED_CONTEXT | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g) ==
          HSW_ERR_INVALID_ARG && !g);

    // ---- create / declare / reset / re-declare / destroy
    const size_t M = 3, K = 4;
    CHECK(hsw_gadget_create_contexts(e, sizes, M, K, 1, WHOLE | HSW_GADGET_SHARED_CONTEXT, &g) == HSW_OK && g);
    hsw_gadget_view v;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.capacity_blocks == K * 6);
    std::vector<uint8_t> msg(100, 3);
    const uint8_t *in[1] = {msg.data()};
    size_t len[1] = {msg.size()}, pre[1] = {0};
    hsw_hash_result r;
    CHECK(hsw_gadget_digest_batch(g, 1, in, len, pre, &r) == HSW_ERR_UNSUPPORTED);                          // no column image yet
    CHECK(hsw_gadget_set_digest_origin(g, 1, 0, 0, 0) == HSW_ERR_INVALID_ARG);                              // no column image yet
    uint64_t columns = 0;
    CHECK(hsw_gadget_set_origin(g, 1, 777, 0, 5) == HSW_OK);
    CHECK(hsw_gadget_set_columns(g, MAX_ROWS, &columns) == HSW_OK && columns == 4);
    hsw_context_region reg;
    CHECK(hsw_gadget_context_region(g, 0, &reg) == HSW_OK && reg.assigned == 0);
    const uint64_t C = reg.stream_cells, Lp0 = reg.lookup_cells;
    uint64_t c_end0 = 0, r_end0 = 0, c = 0, rw = 0;
    // digest 0 of a Context ends where the single gadget's does; a probe of the layout through Context 2's cells
    hsw_frame_shape fs0;
    hsw_shape sh;
    CHECK(hsw_engine_shape(e, &sh) == HSW_OK && hsw_frame_query(&sh, sizes[0], 1, &fs0) == HSW_OK);
    const uint64_t end0 = fs0.digest_cells + 1;                                                              // + the zero cell
    CHECK(hsw_gadget_cell_position(g, 2 * C + end0 - 1, &c_end0, &r_end0) == HSW_OK);
    CHECK(hsw_gadget_cell_position(g, end0, &c, &rw) == HSW_OK);
    const uint64_t c_e = c, r_e = rw;
    const uint64_t lk1 = 5 + fs0.digest_lookups;
    // refusals: each leaves layout and buffers as they were
    void *gate_before = nullptr;
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    gate_before = v.d_gate;
    const uint64_t cols_before = v.columns;
    CHECK(hsw_gadget_set_digest_origin(g, 0, c_end0 + 1, 0, lk1) == HSW_ERR_INVALID_ARG);                    // j = 0
    CHECK(hsw_gadget_set_digest_origin(g, M, c_end0 + 1, 0, lk1) == HSW_ERR_INVALID_ARG);                    // j >= M: ONE Context's digests
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0, r_end0, lk1) == HSW_ERR_INVALID_ARG);                   // before the free cell
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0 + 1, MAX_ROWS, lk1) == HSW_ERR_INVALID_ARG);             // row outside
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0 + 1, 0, lk1 - 1) == HSW_ERR_INVALID_ARG);                // lookups below
    CHECK(hsw_gadget_set_digest_origin(g, 1, 1 + HSW_GADGET_MAX_COLUMNS, 0, lk1) == HSW_ERR_TOO_LARGE);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.d_gate == gate_before && v.columns == cols_before);
    CHECK(hsw_gadget_cell_position(g, 3 * C + end0, &c, &rw) == HSW_OK && c == c_e && rw == r_e);
    CHECK(hsw_gadget_context_region(g, 3, &reg) == HSW_OK && reg.lookup_cells == Lp0 && reg.columns == cols_before);
    // declarations: an interlude before digest 1 into the next column, lookup entries only before digest 2
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0 + 1, 40, lk1 + 9) == HSW_OK);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.columns >= cols_before);
    for (size_t k = 0; k < K; k++) {
        CHECK(hsw_gadget_cell_position(g, k * C + end0, &c, &rw) == HSW_OK && c == c_end0 + 1 && rw == 40);
        CHECK(hsw_gadget_context_region(g, k, &reg) == HSW_OK && reg.lookup_cells == Lp0 + 9 && reg.columns == v.columns);
        CHECK(reg.d_image == (uint8_t *)v.d_gate + k * v.columns * v.max_rows * HSW_CELL_BYTES);
    }
    // a pass half issued (it ends in the middle of Context 1), then reset and the same declarations again: layout,
    // buffers and region tape are kept
    std::vector<const uint8_t *> ins(M * K, msg.data());
    std::vector<size_t> lens(M * K, 50), pres(M * K, 0);
    std::vector<hsw_hash_result> rr(M * K);
    CHECK(hsw_gadget_digest_batch(g, M + 1, ins.data(), lens.data(), pres.data(), rr.data()) == HSW_OK);
    CHECK(rr[M].prologue_cell == C && rr[M].first_block == 6 && rr[M].prologue_lookup == Lp0 + 9 + 5);
    CHECK(hsw_gadget_context_region(g, 0, &reg) == HSW_OK && reg.assigned == 1);
    CHECK(hsw_gadget_context_region(g, 1, &reg) == HSW_OK && reg.assigned == 0);
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0 + 1, 41, lk1 + 9) == HSW_ERR_INVALID_ARG);               // digest 1 is assigned
    hsw_region_tape tape;
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK && tape.gate_cells == rr[M].end_cell);
    const uint32_t *codes = tape.gate_code;
    {   // a delivery of the half-issued pass into exact-size buffers: Context 1 up to its cursor, nothing of Contexts 2, 3
        CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
        const uint64_t S = v.columns * v.max_rows, Lp = Lp0 + 9;
        std::vector<uint64_t> gate(K * S * 4, FILL), look(K * Lp * 4, FILL), cd(2 * v.chip_col_stride * 4), cs(2 * v.chip_col_stride * 4);
        hsw_region_host dst = {gate.data(), look.data(), cd.data(), cs.data()};
        CHECK(hsw_gadget_download_region(g, &dst) == HSW_OK);
        CHECK(gate[4 * 776] == FILL && gate[4 * 777] != FILL && gate[4 * (S + 777)] != FILL && gate[4 * (2 * S + 777)] == FILL);
        CHECK(look[4 * 4] == FILL && look[4 * 5] != FILL && look[4 * (Lp + 4)] == FILL && look[4 * (Lp + 5)] != FILL);
        for (uint64_t i = lk1; i < lk1 + 9; i++) CHECK(look[4 * i] == FILL);                               // the interlude's entries
        CHECK(look[4 * (lk1 + 9)] != FILL);
        uint64_t c1 = 0, w1 = 0;                                                                           // Context 1's digest 1: not issued
        CHECK(hsw_gadget_cell_position(g, C + end0, &c1, &w1) == HSW_OK);
        CHECK(gate[4 * (S + (c1 - 1) * MAX_ROWS + w1)] == FILL);
    }
    hsw_verify_report rep;
    CHECK(hsw_gadget_verify(g, &rep) == HSW_OK);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK);
    void *gate_kept = v.d_gate, *look_kept = v.d_lookup;
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0 + 1, 40, lk1 + 9) == HSW_OK);                           // the same again
    hsw_frame_shape fs1;
    CHECK(hsw_frame_query(&sh, sizes[1], 1, &fs1) == HSW_OK);
    uint64_t c2 = 0, r2 = 0;
    CHECK(hsw_gadget_cell_position(g, end0 + fs1.digest_cells - 1, &c2, &r2) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 2, c2, r2 + 1, lk1 + 9 + fs1.digest_lookups + 4) == HSW_OK);      // lookup entries only
    CHECK(hsw_gadget_digest_batch(g, M * K, ins.data(), lens.data(), pres.data(), rr.data()) == HSW_OK);
    CHECK(rr[2].prologue_cell == end0 + fs1.digest_cells && rr[2].prologue_lookup == lk1 + 9 + fs1.digest_lookups + 4);
    CHECK(hsw_gadget_context_region(g, K - 1, &reg) == HSW_OK && reg.assigned == 1 && reg.lookup_cells == Lp0 + 13);
    CHECK(hsw_gadget_region_tape(g, &tape) == HSW_OK && tape.gate_code == codes && tape.gate_cells == K * C);
    CHECK(hsw_gadget_reset(g) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 1, c_end0 + 1, 40, lk1 + 9) == HSW_OK);
    CHECK(hsw_gadget_set_digest_origin(g, 2, c2, r2 + 1, lk1 + 9 + fs1.digest_lookups + 4) == HSW_OK);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.d_gate != nullptr);
    void *gate_now = v.d_gate, *look_now = v.d_lookup;
    CHECK(hsw_gadget_set_digest_origin(g, 2, c2, r2 + 1, lk1 + 9 + fs1.digest_lookups + 4) == HSW_OK);
    CHECK(hsw_gadget_streams(g, &v) == HSW_OK && v.d_gate == gate_now && v.d_lookup == look_now);           // kept
    (void)gate_kept; (void)look_kept;
    // the calls that refuse in this mode
    hsw_region_compact cdst = {};
    CHECK(hsw_gadget_download_region_compact(g, &cdst) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_seek(g, 1) == HSW_ERR_UNSUPPORTED);
    CHECK(hsw_gadget_place(g, 2, nullptr, nullptr) == HSW_ERR_UNSUPPORTED);
    // destroy with a pass half issued: digest by digest into the middle of Context 2
    len[0] = 50;                                     // (fits every digest of the Context)
    for (size_t d = 0; d < 2 * M + 2; d++) CHECK(hsw_gadget_digest_batch(g, 1, in, len, pre, &r) == HSW_OK);
    CHECK(r.prologue_cell == 2 * C + end0 && r.first_block == 2 * 6 + 3);
    hsw_gadget_destroy(g);

    // ---- Contexts that come with their zero cell, input range checks off: the region tape (one reserved cell per
    //      Context stays unused), the distinct delivery and its replay, the verifier
    {
        hsw_gadget *z = nullptr;
        CHECK(hsw_gadget_create_contexts(e, sizes, M, K, 0, WHOLE, &z) == HSW_OK);
        CHECK(hsw_gadget_set_origin(z, 1, 40000, 1, 1234) == HSW_OK);
        CHECK(hsw_gadget_set_columns(z, MAX_ROWS, &columns) == HSW_OK);
        CHECK(hsw_gadget_digest_batch(z, M * K, ins.data(), lens.data(), pres.data(), rr.data()) == HSW_OK);
        hsw_context_region zr;
        CHECK(hsw_gadget_context_region(z, K - 1, &zr) == HSW_OK && zr.assigned == 1 && zr.origin_lookups == 1234);
        CHECK(hsw_gadget_streams(z, &v) == HSW_OK && v.gate_cells == K * zr.stream_cells && v.gate_capacity == K * (zr.stream_cells + 1));
        hsw_region_tape zt;
        CHECK(hsw_gadget_region_tape(z, &zt) == HSW_OK && zt.gate_cells == K * zr.stream_cells);
        std::vector<uint64_t> distinct(zt.n_distinct * 4 + 4);
        size_t n = 0;
        CHECK(hsw_gadget_download_region_distinct(z, distinct.data(), zt.n_distinct, &n) == HSW_OK && n == zt.n_distinct);
        const uint64_t S = v.columns * v.max_rows, Lp = zr.lookup_cells;
        std::vector<uint64_t> ga(K * S * 4, FILL), la(K * Lp * 4, FILL), gb(K * S * 4, FILL), lb(K * Lp * 4, FILL);
        std::vector<uint64_t> cd(2 * v.chip_col_stride * 4), cs(2 * v.chip_col_stride * 4);
        hsw_region_host da = {ga.data(), la.data(), cd.data(), cs.data()}, db = {gb.data(), lb.data(), cd.data(), cs.data()};
        CHECK(hsw_gadget_download_region(z, &da) == HSW_OK && hsw_gadget_replay_region(z, distinct.data(), &db, 2) == HSW_OK);
        for (uint64_t i = 0; i < K * S; i++) CHECK((ga[4 * i] == FILL) == (gb[4 * i] == FILL));
        for (uint64_t i = 0; i < K * Lp; i++) CHECK((la[4 * i] == FILL) == (lb[4 * i] == FILL));
        for (size_t k = 0; k < K; k++) {                                            // the caller's: rows above the origin, queued lookups
            CHECK(ga[4 * (k * S + 39999)] == FILL && ga[4 * (k * S + 40000)] != FILL);
            CHECK(la[4 * (k * Lp + 1233)] == FILL && la[4 * (k * Lp + 1234)] != FILL);
        }
        CHECK(hsw_gadget_verify(z, &rep) == HSW_OK);
        hsw_gadget_destroy(z);
    }

    // ---- positions against the single shared-context gadget
    compare_with_single(e, sizes, 3, 4, false);
    compare_with_single(e, sizes, 3, 4, true);
    size_t big[2] = {1024, 1024};                    // more than 17 columns per Context
    compare_with_single(e, big, 2, 2, false);
    compare_with_single(e, big, 2, 2, true);
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::puts("context groups lifecycle ok");
    return 0;
}
