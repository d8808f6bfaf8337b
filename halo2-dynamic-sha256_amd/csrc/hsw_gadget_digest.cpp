// hsw_gadget_digest.cpp -- Sha256DynamicConfig::digest and its batched and device-fed forms (hsw_gadget.hpp): staging,
// the launches (hsw_gadget_launch.hpp), the results; and the ties a device-fed batch adds.
#include "hsw_gadget_launch.hpp"

#include <algorithm>
#include <cstring>
#include <iterator>

namespace hsw {

int Sha256DynamicConfig::digest(Context &ctx, const uint8_t *input, size_t input_len,
                                size_t precomputed_input_len, AssignedHashResult *result) {
    return digest_batch(ctx, 1, &input, &input_len, &precomputed_input_len, result);
}

// (c) The common tail of digest_batch and digest_batch_device, the plans made and nothing committed yet:
// stage(stream, zero_copy) issues what puts the batch's blocks at d_blocks + 64 * b0 and their pre-states at
// d_pre_states + 8 * b0 (zero_copy: the host-fed staging left them in the pinned buffers, read in place); then the
// expansion / frame launches, the next states, the results and the cursors.  Nothing after the staging knows where
// the bytes came from.  device_fed: the staged blocks and the states after the prefixes come back with the next states.
template <class Stage>
int Sha256DynamicConfig::digest_tail(Context &ctx, size_t n, const size_t *input_lens, std::vector<DigestPlan> &plans,
                                     size_t batch_blocks, bool host_chain, bool device_fed, Stage &&stage,
                                     AssignedHashResult *results) {
    const size_t b0 = ctx.blocks_done;
    for (size_t i = 0, off = 0; i < n; off += plans[i++].max_variable_round) {       // what the plans alone say
        AssignedHashResult &r = results[i];
        r.input_len = input_lens[i];
        r.first_block = b0 + off;
        r.n_blocks = plans[i].max_variable_round;
        r.spread_cursor0 = ctx.num_limb_sum + (uint64_t)off * ctx.shape.limb_calls_per_block;
        r.num_round = plans[i].num_round;
        r.target_round = plans[i].target_round;
        r.precomputed_round = plans[i].precomputed_round;
    }
    // ---- device: chain pre-pass + ONE expansion launch for the whole batch ----
    EngineScope es(ctx.engine);
    if (!es.ok) return HSW_ERR_NO_DEVICE;
    const hipStream_t stream = es.stream;
    // Small-batch launches (and any launch of up to 32 blocks) read their 96 input bytes per block straight from
    // the pinned staging (uncached PCIe reads: cheaper than two dependent copies while the waves are few).
    // Tiny batches (the reference's bench circuit is ONE 16-block digest) are latency-bound: they go to the
    // small-batch kernel, which for a whole-digest context also writes the frames -- ONE launch, inputs read
    // in place from the pinned staging, next states written straight into pinned memory, no copy launches.
    // (whole-digest contexts: one such launch per run of equally sized digests, each with its own frames)
    // (a Context group always takes the expansion + frame launches: its expansion launches are not contiguous runs)
    if (ctx.group_m && !ctx.layout.max_rows) return HSW_ERR_UNSUPPORTED;        // K images: hsw_gadget_set_columns first
    const bool small = !ctx.group_m && hsw_small_eligible(ctx.engine, batch_blocks);
    const bool zero_copy = host_chain && (ctx.whole ? small : (small || batch_blocks <= 32));
    uint32_t *d_next = ctx.d_next_states + 8 * b0;
    uint32_t *h_next = ctx.hp_next + 8 * b0;                                     // pinned: the D2H below is asynchronous
    // device-fed: the batch's staged blocks come back into its hp_blocks range (AssignedHashResult::input_bytes) and
    // the n states after the prefixes (the target_round == 0 selection) into its idle hp_pre range where they fit
    std::vector<uint32_t> init_pageable;
    uint32_t *h_init = nullptr;
    if (device_fed) {
        if (n > batch_blocks) init_pageable.resize(8 * n);
        h_init = n > batch_blocks ? init_pageable.data() : ctx.hp_pre + 8 * b0;
    }
    auto fetch_staged = [&]() -> hipError_t {
        if (!device_fed) return hipSuccess;
        hipError_t e = hipSuccess;
        if (batch_blocks) e = hipMemcpyAsync(ctx.hp_blocks + 64 * b0, ctx.d_blocks + 64 * b0, batch_blocks * 64, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_init, ctx.d_init_states, n * 32, hipMemcpyDeviceToHost, stream);
        return e;
    };
    hipError_t he = hipSuccess;
    int rc = HSW_OK;
    bool next_in_pinned = false;               // the kernel wrote the next states into hp_next itself
    std::vector<hsw_frame_desc> frames;
    uint64_t new_gate_cursor = ctx.gate_cursor, new_lookup_cursor = ctx.lookup_cursor;
    do {
        if (batch_blocks == 0 && !device_fed) break;
        if ((he = stage(stream, zero_copy)) != hipSuccess) break;
        if (batch_blocks == 0) { if ((he = fetch_staged()) == hipSuccess) he = hipStreamSynchronize(stream); break; }   // (device-fed: the prefix states)
        const size_t G = ctx.shape.gate_cells_per_block;
        // shared context: every launch placed by the jump table (uploaded when the layout changed)
        if (ctx.table_path() && (rc = ctx.upload_place()) != HSW_OK) break;
        Launch L(ctx, zero_copy, ctx.repr_flags);
        if (!ctx.whole) {
            // one call covers every block of the batch
            L.blocks(b0, batch_blocks);
            rc = hsw_witness_blocks_impl(ctx.engine, &L.a, nullptr, small ? ctx.dp_next + 8 * b0 : nullptr, nullptr);
            next_in_pinned = small && rc == HSW_OK;
        } else {
            // whole-digest stream: prologue | [zero cell] | blocks | epilogue per digest (hsw_frame.hpp).
            // Consecutive digests of equal size are ONE expansion launch (the kernel skips the frame
            // between their block streams); all frames of the batch are one hsw_frame_kernel launch.
            const size_t LK = ctx.shape.lookup_cells_per_block;
            uint64_t gc = ctx.gate_cursor, lc = ctx.lookup_cursor;
            bool zero_loaded = ctx.zero_loaded;
            // every digest a Context of its own: its own zero cell unless the Contexts come with one (context images)
            const bool own_zero = ctx.independent && !ctx.layout.origin_zero_loaded;
            const bool table = L.period.place != nullptr;
            frames.resize(n);
            std::vector<hsw_frame_shape> fss(n);
            for (size_t i = 0; i < n && rc == HSW_OK; i++) {
                rc = hsw_frame_query(&ctx.shape, max_variable_byte_sizes[cur_hash_idx + i], is_input_range_check ? 1 : 0, &fss[i]);
                if (rc != HSW_OK) break;
                AssignedHashResult &r = results[i];
                // context images: Context h's lookup column is cells [h*Lp, (h+1)*Lp), the caller's queued cells first
                // (lookup_pitch() apart: Lp, or what the caller bound)
                if (ctx.context_images) lc = (uint64_t)(cur_hash_idx + i) * ctx.lookup_pitch() + ctx.layout.origin_lookups;
                if (table && ctx.shared && !ctx.group_m) lc = ctx.layout.digest_lookup0[cur_hash_idx + i];   // after the caller's entries of the interlude
                if (ctx.group_m) {                           // digest j of Context cx: that Context's stream, image and lookup column
                    const size_t cx = (cur_hash_idx + i) / ctx.group_m, j = (cur_hash_idx + i) % ctx.group_m;
                    gc = cx * ctx.layout.period + ctx.layout.digest_cell0[j];
                    lc = cx * ctx.lookup_pitch() + ctx.layout.digest_lookup0[j];
                    zero_loaded = j != 0 || ctx.layout.origin_zero_loaded;
                }
                r.prologue_cell = gc;                        gc += fss[i].prologue_cells;
                r.prologue_lookup = lc;                      lc += fss[i].prologue_lookups;
                r.zero_cell = ~0ull;
                if (!zero_loaded || own_zero) { r.zero_cell = gc++; zero_loaded = true; }   // compression.rs:34 of the first block of a Context
                r.block_cell = gc;                           gc += (uint64_t)r.n_blocks * G;
                r.block_lookup = lc;                         lc += (uint64_t)r.n_blocks * LK;
                r.epilogue_cell = gc;                        gc += fss[i].epilogue_cells;
                r.epilogue_lookup = lc;                      lc += fss[i].epilogue_lookups;
                r.end_cell = gc;
                frames[i] = ctx.frame_desc(r, cur_hash_idx + i, is_input_range_check);
            }
            if (rc == HSW_OK && (gc > ctx.gate_capacity || lc > ctx.lookup_capacity)) rc = HSW_ERR_INVALID_ARG;
            size_t ob = 0;
            for (const Run &run : batch_runs(ctx, cur_hash_idx, n, [&](size_t k) { return frames[k].n_blocks; })) {
                if (rc != HSW_OK) break;
                const size_t i = run.first, j = i + run.count;   // (step 1: the run [i, j) of equally sized digests)
                L.run(cur_hash_idx + i, results[i], (size_t)frames[i].first_block, run.count, fss[i]);
                if (small) {
                    hsw_digests_args da{};
                    da.blocks = L.a;
                    da.descs = frames.data() + i; da.n_digests = j - i;      // this run's digests: frames in the same launch
                    da.d_blocks0 = L.in_blocks; da.d_pre_states0 = L.in_pre; da.d_next_states0 = ctx.d_next_states;
                    da.d_gate0 = ctx.gate_stream(); da.d_lookup0 = ctx.d_lookup;
                    da.frame_pack = L.frame_pack;
                    da.host_next_states = h_next + 8 * ob;
                    // (the device alias of the context's own pinned staging: no runtime lookup per call)
                    rc = hsw_witness_digests_impl(ctx.engine, &da, ctx.dp_next + 8 * (b0 + ob), L.per);
                    next_in_pinned = rc == HSW_OK;
                } else {
                    rc = hsw_witness_blocks_impl(ctx.engine, &L.a, nullptr, nullptr, L.per);
                }
                ob += L.a.n_blocks;
            }
            if (rc == HSW_OK && !small)
                rc = hsw_witness_frames_impl(ctx.engine, frames.data(), n, L.in_blocks, L.in_pre, ctx.d_next_states,
                                             ctx.gate_stream(), ctx.d_lookup, L.frame_pack, ctx.repr_flags, L.per);
            if (rc == HSW_OK) { new_gate_cursor = gc; new_lookup_cursor = lc; }
        }
        if (rc != HSW_OK) break;
        if (!next_in_pinned &&
            (he = hipMemcpyAsync(h_next, d_next, batch_blocks * 32, hipMemcpyDeviceToHost, stream)) != hipSuccess) break;
        if ((he = fetch_staged()) != hipSuccess) break;
        he = hipStreamSynchronize(stream);
    } while (0);
    if (rc != HSW_OK) return rc;
    if (he != hipSuccess) return hip_status(he);
    for (size_t i = 0, blk = b0; device_fed && i < n; blk += plans[i++].max_variable_round) {   // what the host-fed plans hold
        std::memcpy(plans[i].init_state, h_init + 8 * i, 32);
        plans[i].blocks.assign(ctx.hp_blocks + 64 * blk, ctx.hp_blocks + 64 * (blk + plans[i].max_variable_round));
    }

    // ---- results: the "select state #target_round" rule (lib.rs:294-310) ----
    size_t off = 0;
    for (size_t i = 0; i < n; i++) {
        AssignedHashResult &r = results[i];
        const DigestPlan &pl = plans[i];
        r.input_bytes = std::move(plans[i].blocks);          // the plan is done with them (copied to the staging above)
        uint32_t sel[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // output_h_out starts as zero cells (lib.rs:294-295)
        if (pl.target_round == 0) std::memcpy(sel, pl.init_state, 32);                 // candidate 0
        else if (pl.target_round <= pl.max_variable_round)
            std::memcpy(sel, &h_next[8 * (off + pl.target_round - 1)], 32);            // candidate target_round
        for (int w = 0; w < 8; w++) {                           // lib.rs:311-341 big-endian bytes
            r.output_bytes[4 * w] = (uint8_t)(sel[w] >> 24);
            r.output_bytes[4 * w + 1] = (uint8_t)(sel[w] >> 16);
            r.output_bytes[4 * w + 2] = (uint8_t)(sel[w] >> 8);
            r.output_bytes[4 * w + 3] = (uint8_t)sel[w];
        }
        off += pl.max_variable_round;
    }
    ctx.batches.push_back(Context::BatchRecord{cur_hash_idx, n, b0, batch_blocks, zero_copy, ctx.repr_flags});
    ctx.blocks_done += batch_blocks;
    if (ctx.whole) {
        ctx.gate_cursor = new_gate_cursor;
        ctx.lookup_cursor = new_lookup_cursor;
        ctx.zero_loaded = ctx.zero_loaded || batch_blocks != 0;
    }
    ctx.num_limb_sum += (uint64_t)batch_blocks * ctx.shape.limb_calls_per_block;   // spread.rs:228
    cur_hash_idx += n;                                                             // lib.rs:347
    return HSW_OK;
}

int Sha256DynamicConfig::digest_batch(Context &ctx, size_t n, const uint8_t *const *inputs,
                                      const size_t *input_lens, const size_t *precomputed_input_lens,
                                      AssignedHashResult *results) {
    if (!results || !inputs || !input_lens) return HSW_ERR_INVALID_ARG;
    if (n == 0) return HSW_OK;
    // max_variable_byte_sizes[cur_hash_idx] must exist for every hash (lib.rs:86 would panic)
    if (cur_hash_idx + n > max_variable_byte_sizes.size()) return HSW_ERR_INVALID_ARG;

    // ---- host: lib.rs:77-160 for every message; nothing is committed on error ----
    // (a) the plans, (b) host-fed staging: padded blocks, prefix pre-hash and -- usually -- the chain, (c) the tail
    std::vector<DigestPlan> plans(n);
    size_t batch_blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t max_sz = max_variable_byte_sizes[cur_hash_idx + i];
        const int rc = digest_prepare(inputs[i], input_lens[i],
                                      precomputed_input_lens ? precomputed_input_lens[i] : 0, max_sz, &plans[i]);
        if (rc != HSW_OK) return rc;
        batch_blocks += plans[i].max_variable_round;
    }
    if (ctx.blocks_done + batch_blocks > ctx.capacity_blocks || n > ctx.init_capacity) return HSW_ERR_INVALID_ARG;

    std::vector<uint8_t> h_blocks(batch_blocks * 64 ? batch_blocks * 64 : 1);
    std::vector<uint32_t> h_init(n * 8), h_offsets(n + 1);
    size_t off = 0;
    for (size_t i = 0; i < n; i++) {
        h_offsets[i] = (uint32_t)off;
        if (!plans[i].blocks.empty()) std::memcpy(h_blocks.data() + off * 64, plans[i].blocks.data(), plans[i].blocks.size());
        std::memcpy(&h_init[8 * i], plans[i].init_state, 32);
        off += plans[i].max_variable_round;
    }
    h_offsets[n] = (uint32_t)off;
    // The plain SHA chain (pre-state of every block, lib.rs:188,236) is the only serial part.  Chained
    // on the host it sits next to the prefix pre-hash the reference also does on the CPU (lib.rs:153-160)
    // and saves a dependent kernel launch; on the GPU (hsw_chain_var_kernel) every message has its own
    // lane.  Either way the witness cells -- and the next_states the digest is read from -- come from the
    // GPU.  Host-chained batches stage blocks and pre-states in pinned, device-mapped host memory.
    // Which side chains: the host walks all blocks at ~0.1 us each (x86 SHA extensions; 0.4 us scalar), the
    // GPU chains every message on its own wave (up to 2,048 messages: ~1.8 us per block) or lane (~3.6 us per
    // block) plus a dependent launch.  Many short messages -> GPU; few long ones -> host.
    size_t longest = 0;
    for (size_t i = 0; i < n; i++) longest = plans[i].max_variable_round > longest ? plans[i].max_variable_round : longest;
    const double t_host_us = (double)batch_blocks * (host_sha_is_fast() ? 0.1 : 0.4);
    const double t_gpu_us = 15.0 + (n <= (size_t)HSW_CHAIN_WAVE_MAX_MESSAGES ? 1.8 : 3.6) * (double)longest;   // a wave / a lane per message
    const bool host_chain = t_host_us <= t_gpu_us;
    const size_t b0 = ctx.blocks_done;
    if (host_chain && batch_blocks) {
        std::memcpy(ctx.hp_blocks + 64 * b0, h_blocks.data(), batch_blocks * 64);
        uint32_t *h_pre = ctx.hp_pre + 8 * b0;
        for (size_t i = 0; i < n; i++) {
            uint32_t st[8];
            std::memcpy(st, plans[i].init_state, 32);
            for (size_t j = 0; j < plans[i].max_variable_round; j++) {
                const size_t b = h_offsets[i] + j;
                std::memcpy(&h_pre[8 * b], st, 32);
                plain_compress(st, h_blocks.data() + 64 * b);
            }
        }
    }

    // what the tail issues once it knows whether the kernels read the pinned staging in place
    auto stage = [&](hipStream_t stream, bool zero_copy) -> hipError_t {
        hipError_t he = hipSuccess;
        uint32_t *d_off = ctx.d_offsets;
        if (host_chain && !zero_copy) {      // from pinned memory: both copies are asynchronous DMA
            if ((he = hipMemcpyAsync(ctx.d_blocks + 64 * b0, ctx.hp_blocks + 64 * b0, batch_blocks * 64, hipMemcpyHostToDevice, stream)) != hipSuccess) return he;
            if ((he = hipMemcpyAsync(ctx.d_pre_states + 8 * b0, ctx.hp_pre + 8 * b0, batch_blocks * 32, hipMemcpyHostToDevice, stream)) != hipSuccess) return he;
        }
        if (!host_chain) {
            if ((he = hipMemcpyAsync(ctx.d_blocks + 64 * b0, h_blocks.data(), batch_blocks * 64, hipMemcpyHostToDevice, stream)) != hipSuccess) return he;
            if ((he = hipMemcpyAsync(ctx.d_init_states, h_init.data(), n * 32, hipMemcpyHostToDevice, stream)) != hipSuccess) return he;
            if ((he = hipMemcpyAsync(d_off, h_offsets.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream)) != hipSuccess) return he;
            if ((he = launch_chain_var(ctx.d_blocks + 64 * b0, n, d_off, ctx.d_init_states, ctx.d_pre_states + 8 * b0, stream)) != hipSuccess) return he;
        }
        return he;
    };
    return digest_tail(ctx, n, input_lens, plans, batch_blocks, host_chain, /*device_fed=*/false, stage, results);
}

// The same batch with the message bytes in device memory (hsw_gadget_digest_levels_device; every level equal and no
// outputs: hsw_gadget_digest_batch_device): the plans follow from the lengths alone, and ONE hsw_ingest_kernel launch
// per dependency level does what the host-fed staging does with padding, prefix pre-hash, copies and chain -- and
// leaves each digest where a message of a later level reads it.  The launches follow each other on the engine's
// stream with nothing in between: the kernel boundary orders a level's stores before the next level's loads.  The
// host reads neither a message byte nor a digest from those addresses.
int Sha256DynamicConfig::digest_levels_device(Context &ctx, size_t n, const void *const *d_inputs, const size_t *input_lens,
                                              const size_t *precomputed_input_lens, const uint32_t *levels,
                                              void *const *d_outputs, AssignedHashResult *results) {
    if (!results || !d_inputs || !input_lens) return HSW_ERR_INVALID_ARG;
    if (n == 0) return HSW_OK;
    if (cur_hash_idx + n > max_variable_byte_sizes.size()) return HSW_ERR_INVALID_ARG;
    std::vector<DigestPlan> plans(n);
    std::vector<IngestDesc> by_msg(n);
    size_t batch_blocks = 0;
    for (size_t i = 0; i < n; i++) {
        if (!d_inputs[i] && input_lens[i]) return HSW_ERR_INVALID_ARG;
        int rc = digest_plan(input_lens[i], precomputed_input_lens ? precomputed_input_lens[i] : 0,
                             max_variable_byte_sizes[cur_hash_idx + i], &plans[i]);
        if (rc == HSW_OK && (uint64_t)input_lens[i] > 0xffffffffull) rc = HSW_ERR_TOO_LARGE;   // (the kernel's round counters are 32-bit)
        if (rc != HSW_OK) return rc;
        by_msg[i] = IngestDesc{static_cast<const uint8_t *>(d_inputs[i]), input_lens[i], (uint32_t)(ctx.blocks_done + batch_blocks),
                               (uint32_t)plans[i].max_variable_round, (uint32_t)plans[i].num_round, (uint32_t)plans[i].precomputed_round,
                               d_outputs ? static_cast<uint8_t *>(d_outputs[i]) : nullptr, (uint32_t)i, 0u};
        batch_blocks += plans[i].max_variable_round;
    }
    if (ctx.blocks_done + batch_blocks > ctx.capacity_blocks || n > ctx.init_capacity) return HSW_ERR_INVALID_ARG;

    // ---- who may read whom: byte ranges (a wave discards the bytes of a granule that are not its message's), sorted
    auto level = [&](size_t i) -> uint32_t { return levels ? levels[i] : 0u; };
    std::vector<std::pair<uintptr_t, size_t>> outs;              // (address, message) of every destination, by address
    for (size_t i = 0; d_outputs && i < n; i++)
        if (d_outputs[i]) outs.emplace_back(reinterpret_cast<uintptr_t>(d_outputs[i]), i);
    std::sort(outs.begin(), outs.end());
    char why[160];
    for (size_t k = 1; k < outs.size(); k++)
        if (outs[k].first - outs[k - 1].first < 32) {
            std::snprintf(why, sizeof why, "hsw_gadget_digest_levels_device: the outputs of messages %zu and %zu overlap",
                          outs[k - 1].second, outs[k].second);
            return hsw_engine_fail(ctx.engine, HSW_ERR_INVALID_ARG, why);
        }
    for (size_t i = 0; i < n && !outs.empty(); i++) {
        if (!input_lens[i]) continue;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(d_inputs[i]), hi = lo + input_lens[i];
        // the first destination that ends after lo (destinations are disjoint: at most one starts below lo and does)
        auto it = std::lower_bound(outs.begin(), outs.end(), std::make_pair(lo, (size_t)0));
        if (it != outs.begin() && lo - (it - 1)->first < 32) --it;
        for (; it != outs.end() && it->first < hi; ++it)
            if (level(it->second) >= level(i)) {
                std::snprintf(why, sizeof why, "hsw_gadget_digest_levels_device: message %zu (level %u) reads the output of message %zu "
                              "(level %u), which is not of a lower level", i, level(i), it->second, level(it->second));
                return hsw_engine_fail(ctx.engine, HSW_ERR_INVALID_ARG, why);
            }
    }

    // ---- the descriptor table, stably sorted by level: a level is a run of it, and a launch
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    if (levels) std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return levels[a] < levels[b]; });
    std::vector<IngestDesc> descs(n);
    for (size_t k = 0; k < n; k++) descs[k] = by_msg[order[k]];
    if (!ctx.d_ingest) {                                     // first device-fed batch: a descriptor per hash in flight
        EngineScope es(ctx.engine);
        if (!es.ok) return HSW_ERR_NO_DEVICE;
        const hipError_t he = hipMalloc(&ctx.d_ingest, (ctx.init_capacity ? ctx.init_capacity : 1) * sizeof(IngestDesc));
        if (he != hipSuccess) { ctx.d_ingest = nullptr; return hip_status(he); }
    }
    auto stage = [&](hipStream_t stream, bool) -> hipError_t {
        hipError_t he = hipMemcpyAsync(ctx.d_ingest, descs.data(), n * sizeof(IngestDesc), hipMemcpyHostToDevice, stream);
        for (size_t k0 = 0, k1; he == hipSuccess && k0 < n; k0 = k1) {
            for (k1 = k0 + 1; k1 < n && level(order[k1]) == level(order[k0]); k1++) {}
            he = launch_ingest(static_cast<const IngestDesc *>(ctx.d_ingest) + k0, k1 - k0, ctx.d_blocks, ctx.d_init_states,
                               ctx.d_pre_states, stream);
        }
        return he;
    };
    return digest_tail(ctx, n, input_lens, plans, batch_blocks, /*host_chain=*/false, /*device_fed=*/true, stage, results);
}

int Sha256DynamicConfig::digest_batch_device(Context &ctx, size_t n, const void *const *d_inputs, const size_t *input_lens,
                                             const size_t *precomputed_input_lens, AssignedHashResult *results) {
    return digest_levels_device(ctx, n, d_inputs, input_lens, precomputed_input_lens, nullptr, nullptr, results);
}

}  // namespace hsw

// The digest-to-digest copy constraints a device-fed batch adds (include/hsw.h, "ties").  The call has succeeded, so
// its destinations are disjoint and an input overlaps a destination of the same call only if that one's level is
// strictly lower: putting every destination of the call into the owner map first, then intersecting every message
// with the map, sees exactly "a lower level of this call, or an earlier call of the pass".  O((n + ties) log n).
void hsw_gadget::record_ties(size_t first, size_t n, const void *const *d_inputs, const size_t *input_lens,
                             const size_t *precomputed_input_lens, void *const *d_outputs) {
    for (size_t i = 0; d_outputs && i < n; i++) {
        if (!d_outputs[i]) continue;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(d_outputs[i]), hi = lo + 32;
        // what [lo, hi) covers of earlier runs goes: the run that begins below lo keeps its head, a run that ends
        // after hi keeps its tail (from the output byte that lies at hi)
        auto it = tie_owners.lower_bound(lo);
        if (it != tie_owners.begin()) {
            auto pv = std::prev(it);
            const uintptr_t ps = pv->first, pe = ps + pv->second.len;
            if (pe > lo) {
                const TieOwner o = pv->second;
                pv->second.len = lo - ps;
                if (pe > hi) tie_owners.emplace(hi, TieOwner{pe - hi, o.hash, o.byte0 + (uint32_t)(hi - ps)});
            }
        }
        while (it != tie_owners.end() && it->first < hi) {
            const uintptr_t s = it->first, e = s + it->second.len;
            const TieOwner o = it->second;
            it = tie_owners.erase(it);
            if (e > hi) { tie_owners.emplace(hi, TieOwner{e - hi, o.hash, o.byte0 + (uint32_t)(hi - s)}); break; }
        }
        tie_owners[lo] = TieOwner{32, (uint64_t)(first + i), 0};
    }
    if (tie_owners.empty()) return;
    for (size_t i = 0; i < n; i++) {
        if (!input_lens[i]) continue;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(d_inputs[i]), hi = lo + input_lens[i];
        const size_t pre = precomputed_input_lens ? precomputed_input_lens[i] : 0;
        auto it = tie_owners.upper_bound(lo);                // the first run that ends after lo
        if (it != tie_owners.begin() && std::prev(it)->first + std::prev(it)->second.len > lo) --it;
        for (; it != tie_owners.end() && it->first < hi; ++it) {
            const uintptr_t s = it->first > lo ? it->first : lo, e = it->first + it->second.len < hi ? it->first + it->second.len : hi;
            for (uintptr_t a = s; a < e; a++) {
                const size_t off = a - lo;                   // the byte's place in the message: input byte off - pre
                if (off < pre) tie_prefix_bytes++;           // hashed on the host side of the circuit: no cell
                else ties.push_back(Tie{it->second.hash, (uint64_t)(first + i), it->second.byte0 + (uint32_t)(a - it->first), (uint32_t)(off - pre)});
            }
        }
    }
}
