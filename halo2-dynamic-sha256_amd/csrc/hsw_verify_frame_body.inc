// hsw_verify_frame_body.inc -- the body of hsw_verify_frame_kernel and of hsw_verify_frame_table_kernel (hsw_verify.hip), included in both.  Expects in scope:
// MONT, TABLE (shared contexts: cells placed by the jump table), p, tbl (PlaceTable *, null without TABLE).
// (A textual body rather than a __device__ function: through a function the existing kernels compiled to different code.)
    const FrameDesc d = p.descs[blockIdx.x];
    const u32 tid = threadIdx.x, nt = blockDim.x;
    const uint4 *gate = reinterpret_cast<const uint4 *>(p.gate);
    const uint4 *lk = reinterpret_cast<const uint4 *>(p.lookup);
    const bool packed = p.n_breaks != 0;
    u64 at0 = 0;              // context images: the digest's Context starts at stream cell at0, its image ctx * ctx_image further
    if (p.ctx_stream) {
        const u64 ctx = d.prologue_cell / p.ctx_stream;
        at0 = ctx * p.ctx_stream;
        gate += 2u * (size_t)(ctx * p.ctx_image);
    }
    auto raw_gcell = [&](u64 idx) -> Cell {            // the cell as stored
        idx -= at0;           // (a Context group: the table is one Context's; at0 = 0 otherwise)
        if constexpr (TABLE) {
            const u64 k = tbl_count(*tbl, idx);
            return load_cell(gate, idx + (k ? tbl->cum[k - 1] : 0));
        } else {
            return load_cell(gate, packed ? place(p, idx) : idx);
        }
    };
    auto gcell = [&](u64 idx) -> Cell {
        const Cell c = raw_gcell(idx);
        if constexpr (MONT) return from_mont(c); else return c;
    };
    u32 bad = 0, first = 0xffffffffu, first_class = 0;
    auto fail = [&](u32 cls, u32 at) { bad++; if (at < first) { first = at; first_class = cls; } };
    const u32 N = d.n_blocks;
    const u32 target = d.num_round - d.precomputed_round;
    auto state_word = [&](u32 n, u32 i) -> u64 {
        return n == 0 ? p.pre_states[8 * d.first_block + i] : p.next_states[8 * (d.first_block + n - 1) + i];
    };

    for (int sec = 0; sec < 2; sec++) {
        const FrameVerifyParams::Section &S = sec ? p.epi : p.pro;
        const u64 base = sec ? d.epilogue_cell : d.prologue_cell;
        const u64 lbase = sec ? d.epilogue_lookup : d.prologue_lookup;
        const u32 tag = sec ? 0x40000000u : 0u;            // reported cell: section-relative, epilogue flagged
        // a cell by structure id (section-relative, or a cell of another section)
        auto cell_of = [&](int64_t id) -> Cell {
            if (id >= 0) return gcell(base + (u64)id);
            if (id == FS_ZERO) return small(0);
            if (id == FS_TARGET) return gcell(d.prologue_cell + frame::P_TGT);
            const u32 q = (u32)(FS_STATE0 - id);                       // 8 n + i
            return q < 8 ? gcell(d.prologue_cell + frame::P_STATE + q) : small(state_word(q / 8, q % 8));
        };
        for (u32 r = tid; r < S.n_rows; r += nt) {
            const u32 c = S.gate_rows[r];
            Cell x[4];
            for (int j = 0; j < 4; j++) x[j] = gcell(base + c + j);
            if (!row_holds(x)) fail(VERIFY_GATE_ROW, tag | c);
        }
        for (u32 c = tid; c < S.cells; c += nt) {
            const uint8_t k = S.kind[c];
            const Cell raw = raw_gcell(base + c);
            Cell v = raw;
            if constexpr (MONT) {      // a Montgomery cell is an encoding m < p: m + p reduces to the same value and would pass everything else
                if (geq_p(raw)) fail(VERIFY_RANGE, tag | c);
                if (k != 0) v = from_mont(raw);
            }
            if (k == 0) continue;
            if (k == 1) {
                const int64_t kv = S.ref[c];
                Cell want = small((u64)(kv >= 0 ? kv : -kv));
                if (kv < 0) {                                                       // p - |k|, |k| < 2^62: only limb 0 borrows
                    want.l[0] = 0x43e1f593f0000001ull - want.l[0];
                    want.l[1] = 0x2833e84879b97091ull; want.l[2] = 0xb85045b68181585dull; want.l[3] = 0x30644e72e131a029ull;
                }
                if (!same(v, want)) fail(VERIFY_CONSTANT, tag | c);
            } else if (!same(v, cell_of(S.ref[c]))) fail(VERIFY_COPY, tag | c);
        }
        for (u32 i = tid; i < S.n_assert_eq; i += nt)
            if (!same(cell_of(S.assert_eq[2 * i]), cell_of(S.assert_eq[2 * i + 1]))) fail(VERIFY_ASSERT_EQ, tag | (u32)S.assert_eq[2 * i + 1]);
        for (u32 i = tid; i < S.n_assert_const; i += nt)
            if (!same(cell_of(S.assert_const[2 * i]), small((u64)S.assert_const[2 * i + 1]))) fail(VERIFY_CONSTANT, tag | (u32)S.assert_const[2 * i]);
        for (u32 i = tid; i < S.n_range; i += nt) {
            const Cell v = cell_of(S.range[2 * i]);
            if (!(narrow(v) && (v.l[0] >> S.range[2 * i + 1]) == 0)) fail(VERIFY_RANGE, tag | (u32)S.range[2 * i]);
        }
        if (lk)
            for (u32 j = tid; j < S.n_lookup; j += nt) {
                const Cell rv = load_cell(lk, lbase + j);
                Cell v = rv;
                bool enc = true;
                if constexpr (MONT) { v = from_mont(rv); enc = !geq_p(rv); }      // canonical encoding only, as in the block body
                if (!(enc && narrow(v) && v.l[0] < 65536 && same(v, cell_of(S.lookup_src[j])))) fail(VERIFY_LOOKUP, tag | j);
            }
    }
    // ---- the facts of this digest and the links between the sections ----
    const u64 P0 = d.prologue_cell;
    if (tid == 0) {
        if (!same(gcell(P0 + frame::P_LEN), small(d.input_len))) fail(VERIFY_COPY, frame::P_LEN);           // AssignedHashResult.input_len
        if (!same(gcell(P0 + frame::P_PRE), small(d.precomputed_round))) fail(VERIFY_COPY, frame::P_PRE);
        if (d.zero_cell != ~0ull && !same(gcell(d.zero_cell), small(0))) fail(VERIFY_CONSTANT, frame::P_BYTES - 1);
        if constexpr (MONT)            // the zero cell stored as p reduces to 0
            if (d.zero_cell != ~0ull && geq_p(raw_gcell(d.zero_cell))) fail(VERIFY_RANGE, frame::P_BYTES - 1);
        (void)target;
    }
    if (tid < 8 && !same(gcell(P0 + frame::P_STATE + tid), small(state_word(0, tid)))) fail(VERIFY_COPY, frame::P_STATE + tid);
    for (u32 i = tid; i < 64u * N; i += nt)                                                                  // input bytes
        if (!same(gcell(P0 + frame::P_BYTES + i), small(p.blocks[64 * d.first_block + i]))) fail(VERIFY_COPY, frame::P_BYTES + i);
    for (u32 i = tid; i < 8u * (N - 1); i += nt)                                                             // the chain
        if (p.pre_states[8 * (d.first_block + 1) + i] != p.next_states[8 * d.first_block + i]) fail(VERIFY_NEXT_STATE, i);
    if (bad) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&p.report->violations), (unsigned long long)bad);
        const unsigned long long key = ((unsigned long long)d.first_block << 36) | ((unsigned long long)first << 4) | first_class;
        atomicMin(reinterpret_cast<unsigned long long *>(&p.report->first_key), key);
    }
