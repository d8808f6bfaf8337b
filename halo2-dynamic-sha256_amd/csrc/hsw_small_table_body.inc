// hsw_small_table_body.inc -- the body of hsw_small_table_kernel and of its wide overload (hsw_small.hpp), included in both.
// Expects in scope: L, REPR, WIDE (columns by pointer table: PlaceTable::cum_stride), p, fr, t.
// (A textual body rather than a __device__ function: through a function the existing kernels compiled to different code.)
    constexpr bool RC = true, TABLE = true;
    const PlaceTable *tbl = &t;
    using SP = SmallPlan<L, RC>;
    using EM = Em<SMALL_TILE, SMALL_ROWS, REPR, RC, true, true, WIDE>;
    __shared__ __attribute__((aligned(16))) u64 s_tile[(SMALL_ROWS + 1) * EM::STRIDE_W];   // +1 scratch row for lanes >= 16
    __shared__ u16 s_d16[SMALL_ROWS * SP::MAX_CALLS];
    __shared__ u16 s_lk16[SMALL_ROWS * SP::MAX_LK];
    __shared__ u32 s_states[8 * (SMALL_FRAME_MAX_BLOCKS + 2)];
    HSW_STAMP(0);
    const u32 lane = lane_id();
    const u32 n_expand = (u32)p.n_blocks * SMALL_ROLES;

    // ---- frame waves (whole-digest launches): hsw_frame_body.hpp ------------------------------------
    if constexpr (RC && REPR != 2) {
        if (blockIdx.x >= n_expand) {
            if (threadIdx.x >= 64u) return;                      // (frame workgroups use their first wave only)
            const u32 wpf = fr.state_waves + fr.byte_waves;
            const u32 fw = blockIdx.x - n_expand, fi = fw / wpf, slice = fw % wpf;
            const FrameDesc d = fi == 0u ? fr.d0 : fr.descs[fi];
            uint4 *gate = reinterpret_cast<uint4 *>(fr.gate0), *lookup = reinterpret_cast<uint4 *>(fr.lookup0);
            const u64 *inv = reinterpret_cast<const u64 *>(fr.inv_tbl);
            PlaceTable tc = t;                                   // columns by pointer table: the digest's Context's cum row
            if constexpr (WIDE) {
                if (fr.brk.ctx_stream) tc.cum += (d.prologue_cell / fr.brk.ctx_stream) * t.cum_stride;
                tbl = &tc;
            }
            if (slice >= fr.state_waves) {       // the input-byte cells: lib.rs:170-178
                framedev::frame_cells<REPR == 1, TABLE>(d, fr.blocks0, inv, gate, lookup, fr.brk, framedev::FRAME_BYTES,
                                                 (slice - fr.state_waves) * 64u + lane, fr.byte_waves * 64u,
                                                 [](u32, u32) -> u32 { return 0u; }, tbl);
                HSW_STAMP(4);
                return;
            }
            // candidate state n >= 1 = output of block n - 1 = pre-state of block n (the chain inputs); the
            // last block's output comes from the recurrence itself, computed here
            const u32 *ps0 = fr.pre0 + 8 * d.first_block, *ps_last = ps0 + 8 * (d.n_blocks - 1);
            // (the pre-states may sit in pinned host memory: fetch them now, they arrive while the chain runs)
            // (digests of at most SMALL_FRAME_MAX_BLOCKS blocks each -- enforced by launch_small_L; the launch itself
            // may hold up to 128 blocks, or any number with split = 2)
            static_assert(8 * SMALL_FRAME_MAX_BLOCKS <= 4 * 64, "four prefetch loads per lane cover the chain inputs");
            const u32 nw = 8u * d.n_blocks;
            u32 pre_w[4];
#pragma unroll
            for (u32 k = 0; k < 4; k++) pre_w[k] = lane + 64u * k < nw ? ps0[lane + 64u * k] : 0u;
            u32 lA, lE, lW;
            chain_latch<true>(reinterpret_cast<const u32 *>(fr.blocks0 + 64 * (d.first_block + d.n_blocks - 1)), ps_last,
                              64, 64 - (int)(lane & 3u), -1, lA, lE, lW);
#pragma unroll
            for (u32 k = 0; k < 4; k++) if (lane + 64u * k < nw) s_states[lane + 64u * k] = pre_w[k];
            if (lane < 8) s_states[nw + lane] = ps_last[lane] + (lane < 4 ? lA : lE);   // compression.rs:197-212
            __syncthreads();
            HSW_STAMP(1);
            framedev::frame_cells<REPR == 1, TABLE>(
                d, fr.blocks0, inv, gate, lookup, fr.brk, framedev::FRAME_STATES, slice * 64u + lane, fr.state_waves * 64u,
                [&](u32 n, u32 i) -> u32 { return s_states[8u * n + i]; }, tbl);
            HSW_STAMP(4);
            return;
        }
    }

    // Grid order.  Block-major, or (HSW_K_ROLE_MAJOR, launches of <= 16 blocks) role-major: the workgroups of one
    // role -- the same instructions -- then sit next to each other.  Same-box A/B through the C ABI: 16
    // Montgomery blocks 34.5 -> 32.6 us, canonical unchanged, 32 Montgomery blocks 47.1 -> 48.9 us (hence the
    // limit); a longest-roles-first permutation on top of it changed nothing (workgroups do not start in grid order).
    const bool role_major = (p.flags & HSW_K_ROLE_MAJOR) != 0u;
    const u32 role = role_major ? blockIdx.x / (u32)p.n_blocks : blockIdx.x % SMALL_ROLES;
    const size_t blk = role_major ? blockIdx.x - role * (u32)p.n_blocks : blockIdx.x / SMALL_ROLES;
    const u32 *bw = reinterpret_cast<const u32 *>(p.blocks + 64 * blk);
    u32 ps[8];                                   // this block's pre-state (wave-uniform)
    if (p.flags & HSW_K_CHAINED) {
        // ONE message: pre_states holds its initial state only; block b's pre-state is b compressions away
        // (the roles that never look at the state skip the walk)
#pragma unroll
        for (int i = 0; i < 8; i++) ps[i] = p.pre_states[i];
        const bool needs_state = role < SMALL_ROUND_ROLES || role == SMALL_ROLE_FEED || role == SMALL_ROLE_STATE;
        if (needs_state && blk != 0) {
            // the message schedules of the blocks before this one do not depend on the state: lane l expands
            // block l's (all at once), K + W goes through LDS (the tile is not in use yet; rows 65 words apart:
            // no bank conflicts), and only the 64-round recurrence of each block remains serial
            u32 *s_kw = reinterpret_cast<u32 *>(s_tile);
            static_assert(sizeof(s_tile) >= 32 * 65 * 4, "K + W of 31 blocks must fit the tile");
            // (helper waves never look at the state: they only keep the barriers company -- walking along would
            //  cost the emitters' SIMDs a third of their issue slots, 66 vs 47 us per 16 blocks)
            const bool emitter = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
            if (emitter && lane < (u32)blk) {
                const u32 *bl = reinterpret_cast<const u32 *>(p.blocks + 64 * (size_t)lane);
                u32 w[16];
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = __builtin_bswap32(bl[j]);
#pragma unroll
                for (int t = 0; t < 64; t++) {
                    if (t >= 16)
                        w[t & 15] = w[t & 15] + sha_s0(w[(t + 1) & 15]) + w[(t + 9) & 15] + sha_s1(w[(t + 14) & 15]);
                    s_kw[lane * 65u + (u32)t] = w[t & 15] + K256[t];
                }
            }
            __syncthreads();
            for (u32 b = 0; emitter && b < (u32)blk; b++) {
                u32 a = ps[0], bb = ps[1], c = ps[2], d = ps[3], e = ps[4], f = ps[5], g = ps[6], h = ps[7];
                const u32 *kw = s_kw + b * 65u;
#pragma unroll 16
                for (int t = 0; t < 64; t++) {
                    const u32 t1 = h + kw[t] + sha_S1(e) + sha_ch(e, f, g);
                    const u32 t2 = sha_S0(a) + sha_maj(a, bb, c);
                    h = g; g = f; f = e; e = d + t1; d = c; c = bb; bb = a; a = t1 + t2;
                }
                ps[0] += a; ps[1] += bb; ps[2] += c; ps[3] += d; ps[4] += e; ps[5] += f; ps[6] += g; ps[7] += h;
            }
            __syncthreads();                       // the tile takes the memory over
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) ps[i] = p.pre_states[8 * blk + i];
    }

    // wave 0 of the workgroup emits, the others (if any) only take their share of every flush: the same role
    // program instantiated without the staging stores (Em::HELPERS)
    using EMH = Em<SMALL_TILE, SMALL_ROWS, REPR, RC, true, false, WIDE>;
    if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0)
        small_role<L, REPR, RC, EMH, TABLE>(p, bw, ps, blk, role, s_tile, s_d16, s_lk16, tbl);
    else
        small_role<L, REPR, RC, EM, TABLE>(p, bw, ps, blk, role, s_tile, s_d16, s_lk16, tbl);
    HSW_STAMP(4);
