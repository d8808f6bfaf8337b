// hsw_verify_block_body.inc -- the body of hsw_verify_kernel and of hsw_verify_table_kernel (hsw_verify.hip), included in both.  Expects in scope:
// MONT, TABLE (shared contexts: cells placed by the jump table), WIDE (columns by pointer table), p, tbl (PlaceTable *, null
// without TABLE).
// (A textual body rather than a __device__ function: through a function the existing kernels compiled to different code.)
    const u64 blk = blockIdx.x / p.slices;
    const u32 tid = (blockIdx.x % p.slices) * blockDim.x + threadIdx.x, nt = p.slices * blockDim.x;
    const uint4 *gate = reinterpret_cast<const uint4 *>(p.gate);
    const u64 dg = p.frame_every ? blk / p.frame_every : 0;
    u64 g0 = p.gate_cell0 + blk * (u64)p.gate_cells + dg * p.frame_cells;
    if (p.ctx_cells) {        // context images: the block's place in its own Context, whose image starts dg * ctx_cells further
        g0 = p.gate_cell0 + (blk - dg * p.frame_every) * (u64)p.gate_cells;
        gate += 2u * (size_t)(dg * p.ctx_cells);
    }
    // Context groups (TABLE, tbl->ctx_blocks): the launch is one digest index of several Contexts -- the block's
    // inputs, next state and chip cursor are those of the same block ctx_blocks further per Context
    u64 in_blk = blk;
    if constexpr (TABLE)
        if (tbl->ctx_blocks) in_blk = dg * tbl->ctx_blocks + (blk - dg * p.frame_every);
    const bool packed = p.n_breaks != 0;
    auto gcell = [&](u64 idx) -> Cell {
        if constexpr (TABLE) {
            const u64 k = tbl_count(*tbl, tbl->base + idx);
            return load_value<MONT>(gate, idx + (k ? tbl->cum[k - 1] : 0));
        } else {
            return load_value<MONT>(gate, packed ? place(p, idx) : idx);
        }
    };
    const uint8_t *bytes = p.blocks + 64 * in_blk;
    const u32 *pre = p.pre_states + 8 * in_blk;
    u32 bad = 0;
    u32 first = 0xffffffffu, first_class = 0;

    // a cell by structure id: stream cell or one of the cells outside the block's stream
    auto cell_of = [&](int64_t id, bool &known) -> Cell {
        known = true;
        if (id >= 0) return gcell(g0 + (u64)id);
        if (id >= -64) return small(bytes[-1 - id]);                        // input byte k = -1 - id
        if (id <= -100 && id >= -107) return small(pre[-100 - id]);          // pre-state word
        if (id == -1000) return small(0);                                    // the Context's zero cell
        known = false;                                                       // a halo2-base witness outside the stream
        return small(0);
    };
    auto fail = [&](u32 cls, u32 at) { bad++; if (at < first) { first = at; first_class = cls; } };

    // 1 + 2. gate rows x0 + x1*x2 = x3 (mod p), and -- on the same four loads -- what each of the row's cells
    //    must be: a fixed constant or a QuantumCell::Existing copy (every such cell sits in a gate row; the
    //    host checks that when it uploads the structure).  All-narrow rows are exact in 128 bits; the only
    //    rows with a full-width cell are the negations of ch: [a, p-a, 1, 0] and [M, p-a, 1, M-a]
    //    (compression.rs:320-335)
    //    Copies of stream cells are compared as stored (raw to raw: equal values have equal encodings, and a
    //    Montgomery stream needs no reduction for them).
    //    Work split: FOUR lanes per gate row, one per cell.  A quad then reads its row as 128 contiguous bytes
    //    and a wave instruction covers 16 rows in 16 lines -- with one lane per row every load instruction
    //    touched 64 different lines, 16 bytes of each, and the L1 had to keep them all until the row's eighth
    //    load (measured: 3.9 L2 requests per line of the stream, the kernel stalled on them 75 % of the time).
    //    Each lane checks its own cell (constant / copy: one source load per lane, all in flight together);
    //    the row equation gets the other three cells' low limbs by DPP quad broadcasts.
    auto raw_cell = [&](u64 idx) -> Cell {
        if constexpr (TABLE) {
            const u64 k = tbl_count(*tbl, tbl->base + idx);
            return load_cell(gate, idx + (k ? tbl->cum[k - 1] : 0));
        } else {
            return load_cell(gate, packed ? place(p, idx) : idx);
        }
    };
    auto quad64 = [](u64 v, int q) -> u64 {            // lane q of the quad's value, in every lane of the quad
        const int lo = (int)(u32)v, hi = (int)(u32)(v >> 32);
        int rl, rh;
        switch (q) {
            case 0: rl = __builtin_amdgcn_mov_dpp(lo, 0x00, 0xF, 0xF, true); rh = __builtin_amdgcn_mov_dpp(hi, 0x00, 0xF, 0xF, true); break;
            case 1: rl = __builtin_amdgcn_mov_dpp(lo, 0x55, 0xF, 0xF, true); rh = __builtin_amdgcn_mov_dpp(hi, 0x55, 0xF, 0xF, true); break;
            case 2: rl = __builtin_amdgcn_mov_dpp(lo, 0xAA, 0xF, 0xF, true); rh = __builtin_amdgcn_mov_dpp(hi, 0xAA, 0xF, 0xF, true); break;
            default: rl = __builtin_amdgcn_mov_dpp(lo, 0xFF, 0xF, 0xF, true); rh = __builtin_amdgcn_mov_dpp(hi, 0xFF, 0xF, 0xF, true); break;
        }
        return (u64)(u32)rl | ((u64)(u32)rh << 32);
    };
    const u32 j4 = threadIdx.x & 3u;                   // this lane's cell of the row
    const u32 slot = tid >> 2, nslots = nt >> 2;       // row slots of the launch slice (nt is a multiple of 4)
    for (u32 rb = 0; rb < p.n_rows; rb += nslots) {    // the same trip count in every lane: DPP needs whole quads
        const u32 r = rb + slot;
        const bool act = r < p.n_rows;
        const u32 c = p.gate_rows[act ? r : 0u];
        const u32 cell = c + j4;
        const Cell raw = raw_cell(g0 + cell);
        const uint8_t k = p.kind[cell];
        const int64_t rf = p.ref[cell];
        Cell w = raw;
        if (act && k == 2 && rf >= 0) w = raw_cell(g0 + (u64)rf);
        Cell x;
        if constexpr (MONT) x = from_mont(raw); else x = raw;
        // ---- the row: x0 + x1*x2 = x3
        const u64 l0 = quad64(x.l[0], 0), l1 = quad64(x.l[0], 1), l2 = quad64(x.l[0], 2), l3 = quad64(x.l[0], 3);
        const u64 up = x.l[1] | x.l[2] | x.l[3];        // 0 <=> this cell is narrow
        const u64 up0 = quad64(up, 0), up1 = quad64(up, 1), up2 = quad64(up, 2), up3 = quad64(up, 3);
        bool ok, general = false;
        if ((up0 | up1 | up2 | up3) == 0) {
            const unsigned __int128 s128 = (unsigned __int128)l1 * l2 + l0;
            ok = (u64)(s128 >> 64) == 0 && (u64)s128 == l3;
        } else {
            // the only rows with a full-width cell: [a, p-a, 1, 0] and [M, p-a, 1, M-a] (compression.rs:320-335)
            const u64 P0 = 0x43e1f593f0000001ull, P1 = 0x2833e84879b97091ull, P2 = 0xb85045b68181585dull, P3 = 0x30644e72e131a029ull;
            const u64 x11 = quad64(x.l[1], 1), x12 = quad64(x.l[2], 1), x13 = quad64(x.l[3], 1);
            const u64 a = P0 - l1;                                            // x1 = p - a
            ok = (up0 | up2 | up3) == 0 && l2 == 1 && x11 == P1 && x12 == P2 && x13 == P3 && a >= 1 && a <= 0x55555555ull &&
                 l0 >= a && l0 - a == l3;
            general = !ok;                                                    // (the same in all four lanes of the quad)
        }
        // ---- this lane's cell (reported below, after the row)
        bool enc_bad = false;
        u32 own = 0;
        if constexpr (MONT)            // a Montgomery cell is an encoding m < p: m + p reduces to the same value and would pass everything below
            enc_bad = act && geq_p(raw);
        if (act) {
            if (k == 1) { if (!same(x, small((u64)rf))) own = VERIFY_CONSTANT; }
            else if (k == 2) {
                if (rf >= 0) { if (!same(raw, w)) own = VERIFY_COPY; }
                else { bool known; const Cell e = cell_of(rf, known); if (known && !same(x, e)) own = VERIFY_COPY; }
            }
        }
        if (general) {
            // No honest row comes here.  A forged one may still hold mod p with full-width cells (a limb rewritten to p - 1
            // and its accumulators repaired): then the row is not what is wrong with it, and the report must name the bound
            // or the table that is.  The general evaluation of the frames, on the whole row in every lane of the quad --
            // after the cell's own checks, whose operands are dead by now.
            Cell q[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 4; i++) q[j].l[i] = quad64(x.l[i], j);
            ok = row_holds(q);
        }
        if (act && !ok && j4 == 0) fail(VERIFY_GATE_ROW, c);
        if (enc_bad) fail(VERIFY_RANGE, cell);
        if (own) fail(own, cell);
    }
    // 3. assert_equal / range_check accumulator copies
    for (u32 i = tid; i < p.n_assert_eq; i += nt) {
        bool ka, kb;
        const Cell a = cell_of(p.assert_eq[2 * i], ka), b = cell_of(p.assert_eq[2 * i + 1], kb);
        if (ka && kb && !same(a, b)) fail(VERIFY_ASSERT_EQ, (u32)(p.assert_eq[2 * i] >= 0 ? p.assert_eq[2 * i] : p.assert_eq[2 * i + 1]));
    }
    // 4. range_check bounds
    for (u32 i = tid; i < p.n_range; i += nt) {
        bool known;
        const Cell v = cell_of(p.range[2 * i], known);
        const int64_t bits = p.range[2 * i + 1];
        if (known && !(narrow(v) && (bits >= 64 || (v.l[0] >> bits) == 0))) fail(VERIFY_RANGE, (u32)p.range[2 * i]);
    }
    // 5. spread chip: limb call n of this block is absolute call N = cursor0 + blk*LC + n -> column N % ncols,
    //    row N / ncols (spread.rs:202-231); the cells are tied to gate cells and form a row of the spread table.
    //    Two lanes per limb call -- the dense pair and the spread pair -- each with one chip cell and one gate cell
    //    to load (compared as stored); the table relation takes the partner's low limb by a DPP swap.
    if (p.chip_dense) {
        const uint4 *cd = reinterpret_cast<const uint4 *>(p.chip_dense), *csp = reinterpret_cast<const uint4 *>(p.chip_spread);
        const u64 row0 = p.cursor0 / p.ncols - dg * p.chip_ctx_extra;       // (bound regions: the Context's own chip rows)
        const u32 half = threadIdx.x & 1u;                                    // 0: dense, 1: spread
        auto swap32 = [](u32 v) -> u32 { return (u32)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true); };   // quad_perm [1,0,3,2]
        for (u32 nb = 0; nb < p.limb_calls; nb += nt >> 1) {                  // the same trip count in every lane
            const u32 n = nb + (tid >> 1);
            const bool act = n < p.limb_calls;
            const u32 nn = act ? n : 0u;
            const u64 N = p.cursor0 + in_blk * (u64)p.limb_calls + nn;
            u64 at = (N % p.ncols) * (u64)p.chip_col_stride + (N / p.ncols - row0);
            if constexpr (WIDE)     // chip columns by pointer table: the column's own dense / spread offset (PlaceTable::chip_row)
                if (tbl->chip_row)
                    at = tbl->chip_row[((tbl->ctx0 + (tbl->ctx_blocks ? dg : 0)) * p.ncols + N % p.ncols) * 2u + half] + (N / p.ncols - p.cursor0 / p.ncols);
            const Cell rv = load_cell(half ? csp : cd, at);
            const int64_t id = p.chip[2 * nn + half];
            bool tied;
            Cell v;
            if constexpr (MONT) v = from_mont(rv); else v = rv;
            if (id >= 0) tied = same(rv, raw_cell(g0 + (u64)id));
            else { bool known; const Cell e = cell_of(id, known); tied = !known || same(v, e); }
            const u32 lo = (u32)v.l[0], hi = (u32)(v.l[0] >> 32);
            const u32 plo = swap32(lo), phi = swap32(hi);                     // the partner's low limb
            bool ok = tied && narrow(v);
            if constexpr (MONT) ok = ok && !geq_p(rv);                          // canonical encoding only
            if (half) ok = ok && phi == 0 && (u64)spread16(plo) == v.l[0];    // (dense, spread) is a row of the table
            else ok = ok && v.l[0] < (1ull << p.num_bits_lookup);
            const u32 both = (ok ? 1u : 0u) & swap32(ok ? 1u : 0u);
            if (act && half == 0 && !both) fail(VERIFY_CHIP, (u32)p.chip[2 * nn + 1]);
        }
    }
    // 6. lookup-advice column: entry j copies its source cell and is a 16-bit range-table entry
    if (p.lookup) {
        const uint4 *lk = reinterpret_cast<const uint4 *>(p.lookup);
        for (u32 j = tid; j < p.lookup_cells; j += nt) {
            bool known;
            const Cell src = cell_of(p.lookup_src[j], known);
            u64 at = p.lookup_cell0 + blk * (u64)p.lookup_cells + dg * p.frame_lookups + j;
            if constexpr (TABLE)
                if (!tbl->ctx_blocks) at += tbl->lk_shift[dg] - tbl->lk_shift[0];   // (a group's launch: one digest index, its shift is in p.lookup)
            if constexpr (WIDE)     // lookup columns by pointer table: the Context's own offset (PlaceTable::lk_row)
                if (tbl->lk_row && tbl->ctx_blocks) at += tbl->lk_row[tbl->ctx0 + dg] - tbl->lk_row[tbl->ctx0];
            const Cell rv = load_cell(lk, at);
            Cell v = rv;
            bool enc = true;
            if constexpr (MONT) { v = from_mont(rv); enc = !geq_p(rv); }
            if (!(enc && narrow(v) && v.l[0] < 65536 && (!known || same(v, src)))) fail(VERIFY_LOOKUP, j);
        }
    }
    // 7. next-state words
    if (p.next_states && tid < 8) {
        bool known;
        const Cell v = cell_of(p.next_state_cells[tid], known);
        if (!same(v, small(p.next_states[8 * in_blk + tid]))) fail(VERIFY_NEXT_STATE, (u32)p.next_state_cells[tid]);
    }
    if (bad) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&p.report->violations), (unsigned long long)bad);
        // first failing (block, cell, class): smallest packed key wins
        const unsigned long long key = ((unsigned long long)in_blk << 36) | ((unsigned long long)first << 4) | first_class;
        atomicMin(reinterpret_cast<unsigned long long *>(&p.report->first_key), key);
    }
