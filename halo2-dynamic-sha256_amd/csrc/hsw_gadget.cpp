// hsw_gadget.cpp -- Sha256DynamicConfig / Context mirror (see hsw_gadget.hpp)
// and its C ABI (include/hsw.h, "gadget front-end").
#include "hsw_gadget.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iterator>
#include <vector>
#include <cstring>
#include <new>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif

#include "hsw_nounwind.hpp"
#include "hsw_frame.hpp"
#include "hsw_kernels.h"

// library-internal entry points of hsw_api.cpp (hsw_engine.hpp)
bool hsw_small_eligible(const hsw_engine *e, size_t n_blocks);
int hsw_engine_fail(hsw_engine *e, int status, const char *what);
int hsw_witness_blocks_impl(hsw_engine *e, const hsw_witness_args *args, const hsw::SmallFrames *frames,
                            uint32_t *host_next_states, const hsw::ContextPeriod *period);
int hsw_witness_digests_impl(hsw_engine *e, const hsw_digests_args *args, uint32_t *dev_next_states,
                             const hsw::ContextPeriod *period);
int hsw_witness_frames_impl(hsw_engine *e, const hsw_frame_desc *descs, size_t n, const uint8_t *d_blocks,
                            const uint32_t *d_pre_states, const uint32_t *d_next_states, void *d_gate, void *d_lookup,
                            const hsw_pack_plan *pack, uint32_t flags, const hsw::ContextPeriod *period);
int hsw_verify_blocks_impl(hsw_engine *e, const hsw_witness_args *args, hsw_verify_report *report,
                           const hsw::ContextPeriod *period);
int hsw_verify_frames_impl(hsw_engine *e, const hsw_frame_desc *descs, size_t n, const uint8_t *d_blocks,
                           const uint32_t *d_pre_states, const uint32_t *d_next_states, const void *d_gate,
                           const void *d_lookup, const hsw_pack_plan *pack, uint32_t flags, hsw_verify_report *report,
                           const hsw::ContextPeriod *period);
int hsw_verify_pairs_impl(hsw_engine *e, const uint64_t *host_pairs, void *d_pairs, size_t n, hsw_tie_report *report);

namespace hsw {

namespace {

const uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
const uint32_t INIT_STATE[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,      // compression.rs:1003-1012
                                0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// What sha2::compress256 does for the precomputed prefix (lib.rs:160).  The
// prefix is by definition NOT part of the circuit, so the reference hashes it
// on the CPU too; this is not a fallback of the witness path.
void plain_compress_scalar(uint32_t st[8], const uint8_t *block) {
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
        w[i] = ((uint32_t)block[4 * i] << 24) | ((uint32_t)block[4 * i + 1] << 16) |
               ((uint32_t)block[4 * i + 2] << 8) | block[4 * i + 3];
    for (int i = 16; i < 64; i++) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int i = 0; i < 64; i++) {
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
// The same with the x86 SHA extensions (sha2 0.10.6 itself dispatches to them at run time): the plain
// chain of a long digest is the only serial part of the path, 0.4 us per block in scalar code.
// State lives as ABEF / CDGH, the operand order of sha256rnds2; a group of four rounds takes the four
// message words + K in one register, and sha256msg1 / sha256msg2 compute the next four schedule words.
__attribute__((target("sha,sse4.1,ssse3")))
void plain_compress_shani(uint32_t st[8], const uint8_t *block) {
    const __m128i bswap = _mm_set_epi64x(0x0c0d0e0f08090a0bULL, 0x0405060700010203ULL);
    __m128i tmp = _mm_loadu_si128(reinterpret_cast<const __m128i *>(&st[0]));        // d c b a (high .. low lane)
    __m128i s1 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(&st[4]));         // h g f e
    tmp = _mm_shuffle_epi32(tmp, 0xB1);                                              // c d a b
    s1 = _mm_shuffle_epi32(s1, 0x1B);                                                // e f g h
    __m128i s0 = _mm_alignr_epi8(tmp, s1, 8);                                        // a b e f
    s1 = _mm_blend_epi16(s1, tmp, 0xF0);                                             // c d g h
    const __m128i abef_save = s0, cdgh_save = s1;
    __m128i m[4];
    for (int i = 0; i < 16; i++) {
        if (i < 4) {
            m[i] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i *>(block + 16 * i)), bswap);
        } else {
            // W[4i..4i+3] from W[4i-16..], W[4i-12..], W[4i-8..], W[4i-4..]
            __m128i x = _mm_sha256msg1_epu32(m[i & 3], m[(i + 1) & 3]);              // W[t-16] + sigma0(W[t-15])
            x = _mm_add_epi32(x, _mm_alignr_epi8(m[(i + 3) & 3], m[(i + 2) & 3], 4));  // + W[t-7]
            m[i & 3] = _mm_sha256msg2_epu32(x, m[(i + 3) & 3]);                      // + sigma1(W[t-2])
        }
        __m128i wk = _mm_add_epi32(m[i & 3], _mm_loadu_si128(reinterpret_cast<const __m128i *>(&K[4 * i])));
        s1 = _mm_sha256rnds2_epu32(s1, s0, wk);
        wk = _mm_shuffle_epi32(wk, 0x0E);
        s0 = _mm_sha256rnds2_epu32(s0, s1, wk);
    }
    s0 = _mm_add_epi32(s0, abef_save);
    s1 = _mm_add_epi32(s1, cdgh_save);
    tmp = _mm_shuffle_epi32(s0, 0x1B);                                               // f e b a
    s1 = _mm_shuffle_epi32(s1, 0xB1);                                                // d c h g
    s0 = _mm_blend_epi16(tmp, s1, 0xF0);                                             // d c b a
    s1 = _mm_alignr_epi8(s1, tmp, 8);                                                // h g f e
    _mm_storeu_si128(reinterpret_cast<__m128i *>(&st[0]), s0);
    _mm_storeu_si128(reinterpret_cast<__m128i *>(&st[4]), s1);
}
bool have_shani() {
    static const bool ok = [] {
        if (std::getenv("HSW_NO_SHANI")) return false;      // tests: force the scalar code
        __builtin_cpu_init();
        return __builtin_cpu_supports("sha") != 0;
    }();
    return ok;
}
void plain_compress(uint32_t st[8], const uint8_t *block) {
    if (have_shani()) plain_compress_shani(st, block);
    else plain_compress_scalar(st, block);
}
bool host_sha_is_fast() { return have_shani(); }
#else
void plain_compress(uint32_t st[8], const uint8_t *block) { plain_compress_scalar(st, block); }
bool host_sha_is_fast() { return false; }
#endif

struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == dev) { ok = true; prev = -1; }          // already current: nothing to set, nothing to restore
        else ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int hip_status(hipError_t he) { return he == hipSuccess ? HSW_OK : he == hipErrorOutOfMemory ? HSW_ERR_NOMEM : HSW_ERR_HIP; }

// A zeroed device buffer of `bytes` (at least one cell; unassigned advice cells are 0) whose first `keep` bytes are
// those of `old`.  `old` itself is left alone: a caller can get several buffers and commit only when it has them all.
hipError_t fresh_zeroed(void **out, size_t bytes, const void *old = nullptr, size_t keep = 0) {
    if (!bytes) bytes = HSW_CELL_BYTES;
    void *p = nullptr;
    hipError_t he = hipMalloc(&p, bytes);
    if (he == hipSuccess) he = hipMemset(p, 0, bytes);
    if (he == hipSuccess && old && keep) he = hipMemcpy(p, old, keep, hipMemcpyDeviceToDevice);
    if (he != hipSuccess) { (void)hipFree(p); p = nullptr; }
    *out = p;
    return he;
}

}  // namespace

struct DeviceScopeG : DeviceScope { using DeviceScope::DeviceScope; };   // for the C ABI functions below

int digest_plan(size_t input_byte_size, size_t precomputed_input_len, size_t max_variable_byte_size, DigestPlan *plan) {
    if (!plan) return HSW_ERR_INVALID_ARG;
    const size_t one_round_size = 64;                                         // lib.rs:48
    if (max_variable_byte_size % one_round_size != 0) return HSW_ERR_SHAPE;   // lib.rs:57-59
    const size_t input_byte_size_with_9 = input_byte_size + 9;                // lib.rs:78
    const size_t num_round = (input_byte_size_with_9 + one_round_size - 1) / one_round_size;   // lib.rs:80-84
    const size_t padded_size = one_round_size * num_round;                    // lib.rs:85
    if (precomputed_input_len % one_round_size != 0) return HSW_ERR_SHAPE;    // lib.rs:89
    if (precomputed_input_len > padded_size ||
        padded_size - precomputed_input_len > max_variable_byte_size)
        return HSW_ERR_TOO_LARGE;                                             // lib.rs:90
    plan->num_round = num_round;
    plan->precomputed_round = precomputed_input_len / one_round_size;         // lib.rs:93
    plan->target_round = num_round - plan->precomputed_round;
    plan->max_variable_round = max_variable_byte_size / one_round_size;
    return HSW_OK;
}

int digest_prepare(const uint8_t *input, size_t input_byte_size, size_t precomputed_input_len,
                   size_t max_variable_byte_size, DigestPlan *plan) {
    if (!plan || (!input && input_byte_size)) return HSW_ERR_INVALID_ARG;
    DigestPlan lengths;
    const int rc = digest_plan(input_byte_size, precomputed_input_len, max_variable_byte_size, &lengths);
    if (rc != HSW_OK) return rc;
    const size_t one_round_size = 64;
    const size_t num_round = lengths.num_round, padded_size = one_round_size * num_round;
    const size_t zero_padding_byte_size = padded_size - (input_byte_size + 9);                // lib.rs:91
    const size_t remaining_byte_size = max_variable_byte_size + precomputed_input_len - padded_size;   // lib.rs:92
    const size_t precomputed_round = lengths.precomputed_round;
    const size_t total = max_variable_byte_size + precomputed_input_len;

    std::memcpy(plan->init_state, INIT_STATE, sizeof INIT_STATE);             // lib.rs:155
    const uint64_t bitlen = 8ull * (uint64_t)input_byte_size;                 // lib.rs:103-108 (big-endian)
    if (precomputed_input_len == 0) {
        // the common case: no prefix -- pad straight into the bytes fed to the circuit (lib.rs:98-117,170)
        plan->blocks.assign(max_variable_byte_size, 0);
        if (input_byte_size) std::memcpy(plan->blocks.data(), input, input_byte_size);
        size_t n = input_byte_size;
        plan->blocks[n++] = 0x80;                                             // lib.rs:99
        n += zero_padding_byte_size;                                          // lib.rs:100-102
        for (int i = 7; i >= 0; i--) plan->blocks[n++] = (uint8_t)(bitlen >> (8 * i));
        if (n != num_round * one_round_size) return HSW_ERR_INVALID_ARG;      // lib.rs:110
        if (n + remaining_byte_size != total) return HSW_ERR_INVALID_ARG;     // lib.rs:111-117
    } else {
        std::vector<uint8_t> padded(total, 0);                                // lib.rs:98-117
        if (input_byte_size) std::memcpy(padded.data(), input, input_byte_size);
        size_t n = input_byte_size;
        padded[n++] = 0x80;                                                   // lib.rs:99
        n += zero_padding_byte_size;                                          // lib.rs:100-102
        for (int i = 7; i >= 0; i--) padded[n++] = (uint8_t)(bitlen >> (8 * i));
        if (n != num_round * one_round_size) return HSW_ERR_INVALID_ARG;      // lib.rs:110
        if (n + remaining_byte_size != total) return HSW_ERR_INVALID_ARG;     // lib.rs:111-117
        for (size_t r = 0; r < precomputed_round; r++)                        // lib.rs:156-160
            plain_compress(plan->init_state, padded.data() + r * one_round_size);
        plan->blocks.assign(padded.begin() + (ptrdiff_t)precomputed_input_len, padded.end());   // lib.rs:170
    }
    plan->num_round = num_round;
    plan->precomputed_round = precomputed_round;
    plan->target_round = lengths.target_round;
    plan->max_variable_round = lengths.max_variable_round;
    return HSW_OK;
}

int Sha256DynamicConfig::configure(const std::vector<size_t> &sizes, uint32_t num_bits_lookup,
                                   uint32_t num_advice_columns, bool is_input_range_check,
                                   Sha256DynamicConfig *out) {
    if (!out) return HSW_ERR_INVALID_ARG;
    for (size_t b : sizes)
        if (b % 64 != 0) return HSW_ERR_SHAPE;                                // lib.rs:57-59
    hsw_shape s;
    const int rc = hsw_shape_query(num_bits_lookup, num_advice_columns, &s);  // SpreadConfig::configure, spread.rs:37
    if (rc != HSW_OK) return rc;
    out->max_variable_byte_sizes = sizes;
    out->cur_hash_idx = 0;                                                    // lib.rs:66
    out->num_bits_lookup = num_bits_lookup;
    out->num_advice_columns = num_advice_columns;
    out->is_input_range_check = is_input_range_check;
    return HSW_OK;
}

std::vector<std::pair<uint64_t, uint64_t>> Sha256DynamicConfig::load() const {
    std::vector<std::pair<uint64_t, uint64_t>> rows;                          // spread.rs:169-189
    for (uint64_t idx = 0; idx < (1ull << num_bits_lookup); idx++) {
        uint64_t sp = 0;
        for (int b = 0; b < 32; b++) sp |= ((idx >> b) & 1ull) << (2 * b);
        rows.emplace_back(idx, sp);
    }
    return rows;
}

Context::~Context() {
    if (!bound) { (void)hipFree(d_gate); (void)hipFree(d_chip_dense); (void)hipFree(d_chip_spread); (void)hipFree(d_lookup); }
    (void)hipFree(d_next_states); (void)hipFree(d_blocks); (void)hipFree(d_pre_states);
    (void)hipFree(d_init_states); (void)hipFree(d_offsets); (void)hipFree(d_place); (void)hipFree(d_ingest);
    if (hp_blocks) (void)hipHostFree(hp_blocks);
    free_compact_staging();
}

void Context::free_compact_staging() {
    (void)hipFree(d_c_gate); (void)hipFree(d_c_lookup); (void)hipFree(d_c_dense); (void)hipFree(d_c_spread);
    (void)hipFree(d_wide); (void)hipFree(d_wide_count);
    if (hp_wide_count) (void)hipHostFree(hp_wide_count);
    d_c_gate = d_c_lookup = d_c_dense = d_c_spread = d_wide = nullptr;
    d_wide_count = hp_wide_count = nullptr;
    wide_cap = 0;
}

int Sha256DynamicConfig::new_context(hsw_engine *engine, Context **out, bool whole_digest, bool independent,
                                     bool context_images, bool shared, size_t group_m) const {
    if (!engine || !out) return HSW_ERR_INVALID_ARG;
    *out = nullptr;
    hsw_shape s;
    int rc = hsw_engine_shape(engine, &s);
    if (rc != HSW_OK) return rc;
    if (s.num_bits_lookup != num_bits_lookup || s.num_advice_columns != num_advice_columns)
        return HSW_ERR_SHAPE;
    int device = 0;
    hsw_engine_stream(engine, nullptr, &device);
    DeviceScope ds(device);                                   // the context's buffers live on the engine's GPU
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
    Context *c = new (std::nothrow) Context();
    if (!c) return HSW_ERR_NOMEM;
    c->engine = engine;
    c->shape = s;
    size_t total = 0;
    for (size_t b : max_variable_byte_sizes) total += b / 64;
    c->capacity_blocks = total;
    c->chip_col_stride = (size_t)hsw_chip_rows(&s, 0, total);
    c->init_capacity = max_variable_byte_sizes.size();
    const size_t nb = total ? total : 1, nh = c->init_capacity ? c->init_capacity : 1;
    size_t gate_cells = nb * (size_t)s.gate_cells_per_block;
    if (whole_digest) {
        if (s.mode != HSW_MODE_HALO2_INTERNALS) { delete c; return HSW_ERR_INVALID_ARG; }
        c->whole = true;
        c->independent = independent;
        c->context_images = context_images;
        c->shared = shared;
        if (shared) c->declared.resize(group_m ? group_m : max_variable_byte_sizes.size());
        c->group_m = group_m;
        // the Context's zero cell: one, or one per digest when every digest is a Context of its own
        uint64_t cells = independent ? max_variable_byte_sizes.size() : 1, lookups = 0;
        for (size_t b : max_variable_byte_sizes) {
            if (independent && ((b / 64) * (uint64_t)s.limb_calls_per_block) % s.num_advice_columns != 0) {
                delete c;
                return HSW_ERR_UNSUPPORTED;                   // a context's chip rows must start on a row of their own
            }
            hsw_frame_shape fs;
            rc = hsw_frame_query(&s, b, is_input_range_check ? 1 : 0, &fs);
            if (rc == HSW_OK && fs.n_blocks == 0) rc = HSW_ERR_UNSUPPORTED;
            if (rc != HSW_OK) { delete c; return rc; }
            cells += fs.digest_cells;
            lookups += fs.digest_lookups;
            c->ctx_digest_cells = fs.digest_cells;            // (context images: every digest has this shape)
            c->ctx_own_lookups = fs.digest_lookups;
        }
        if (group_m) {                                        // K Contexts alike: a zero cell each, one Context's sums
            const uint64_t K = max_variable_byte_sizes.size() / group_m;
            c->ctx_digest_cells = (cells - 1) / K;
            c->ctx_own_lookups = lookups / K;
            c->ctx_blocks = total / (size_t)K;
            cells += K - 1;
            if (((uint64_t)c->ctx_blocks * s.limb_calls_per_block) % s.num_advice_columns != 0) {
                delete c;
                return HSW_ERR_UNSUPPORTED;                   // a Context's chip rows must start on a row of their own
            }
        }
        c->gate_capacity = cells;
        c->lookup_capacity = c->own_lookup_capacity = lookups;
        gate_cells = (size_t)cells;
    }
    hipError_t he = hipMalloc(&c->d_gate, gate_cells * HSW_CELL_BYTES);
    // touch the stream buffers once: the first write into fresh device memory is several times slower
    // (measured: 16-block digests 266 us instead of 54 us while a context's buffer was still untouched)
    if (he == hipSuccess) he = hipMemset(c->d_gate, 0, gate_cells * HSW_CELL_BYTES);
    if (he == hipSuccess && whole_digest) {
        const size_t lbytes = (size_t)(c->lookup_capacity ? c->lookup_capacity : 1) * HSW_CELL_BYTES;
        he = hipMalloc(&c->d_lookup, lbytes);
        if (he == hipSuccess) he = hipMemset(c->d_lookup, 0, lbytes);
    }
    const size_t col_bytes = (size_t)s.num_advice_columns * (c->chip_col_stride ? c->chip_col_stride : 1) * HSW_CELL_BYTES;
    if (he == hipSuccess) he = hipMalloc(&c->d_chip_dense, col_bytes);
    if (he == hipSuccess) he = hipMalloc(&c->d_chip_spread, col_bytes);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_next_states, nb * 32);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_blocks, nb * 64);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_pre_states, nb * 32);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_init_states, nh * 32);
    if (he == hipSuccess) he = hipMalloc((void **)&c->d_offsets, (nh + 1) * sizeof(uint32_t));
    if (he == hipSuccess) {
        void *pin = nullptr, *dpin = nullptr;
        he = hipHostMalloc(&pin, nb * 128, hipHostMallocMapped);
        if (he == hipSuccess) {
            c->hp_blocks = static_cast<uint8_t *>(pin);
            he = hipHostGetDevicePointer(&dpin, pin, 0);
        }
        if (he == hipSuccess) {
            c->hp_pre = reinterpret_cast<uint32_t *>(c->hp_blocks + nb * 64);
            c->hp_next = reinterpret_cast<uint32_t *>(c->hp_blocks + nb * 96);
            c->dp_blocks = static_cast<uint8_t *>(dpin);
            c->dp_pre = reinterpret_cast<uint32_t *>(c->dp_blocks + nb * 64);
            c->dp_next = reinterpret_cast<uint32_t *>(c->dp_blocks + nb * 96);
        }
    }
    if (he == hipSuccess) he = hipMemset(c->d_chip_dense, 0, col_bytes);
    if (he == hipSuccess) he = hipMemset(c->d_chip_spread, 0, col_bytes);
    if (he != hipSuccess) {
        delete c;
        return hip_status(he);
    }
    *out = c;
    return HSW_OK;
}

int Context::plan_layout(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t rows, const std::vector<DigestOrigin> &decl,
                         Layout *out) const {
    if (!rows) return HSW_OK;                             // no image: the stream as it is, from the origin
    // context images: ONE Context's walk (every Context is laid out alike), K images of it
    // (a Context group: ONE Context's group_m digests, with the declarations)
    const size_t n = context_images && !sizes.empty() ? 1 : group_m ? group_m : sizes.size();
    const int rc = layout_walk(shape, sizes.data(), n, rc_inputs, rows, shared ? &decl : nullptr, out);
    if (rc != HSW_OK) return rc;
    if (group_m) out->period = ctx_digest_cells + (out->origin_zero_loaded ? 0u : 1u);
    if (shared) return out->columns > HSW_GADGET_MAX_COLUMNS ? HSW_ERR_TOO_LARGE : HSW_OK;
    out->digest_cell0.clear(); out->digest_entry0.clear(); out->digest_lookup0.clear();   // (one lookup run, no table)
    if (context_images) out->period = ctx_digest_cells + (out->origin_zero_loaded ? 0u : 1u);
    return out->break_cell.size() > HSW_MAX_BREAKS ? HSW_ERR_TOO_LARGE : HSW_OK;
}

int Context::adopt(Layout &nl, bool fresh_image, bool fresh_lookup, uint64_t clear_from) {
    const size_t K = contexts(), none = ~(size_t)0;
    const bool table = (shared || by_pointer) && nl.max_rows, changed = !nl.same_map(layout);
    if (bound) {                                          // the caller's memory: it fits what was declared, or it does not
        if (nl.columns > binding.columns_capacity || lookups_needed(nl) > binding.lookup_capacity) return HSW_ERR_TOO_LARGE;
        layout = std::move(nl);
        lookup_capacity = (uint64_t)(K - 1) * lookup_pitch() + binding.lookup_capacity;
        place_dirty = place_dirty || changed || lookup_by_table();      // (the table's lookup rows count from Lp, the layout's)
        return HSW_OK;
    }
    size_t img_cells = none, img_keep = 0, lk_cells = none, lk_keep = 0;
    if (table && group_m) {
        // a Context group: K images and K lookup columns whose places follow from one Context's size -- a layout
        // that differs gets fresh, zeroed ones (the same layout again, pass after pass, keeps them)
        if (fresh_image || changed || nl.max_rows != layout.max_rows) img_cells = K * (size_t)nl.image_cells();
        if (fresh_lookup || nl.lookups_end != layout.lookups_end || K * (size_t)nl.lookups_end != lookup_capacity) lk_cells = K * (size_t)nl.lookups_end;
        fresh_lookup = false;
    } else if (table) {                                   // the image grows: the columns so far are copied over
        const uint64_t have = nl.max_rows == layout.max_rows ? image_columns : 0;   // (another column height: a fresh image)
        if (nl.columns > have) { img_cells = (size_t)nl.image_cells(); img_keep = (size_t)(have * nl.max_rows); }
    } else if (fresh_image) {
        img_cells = K * (size_t)nl.image_cells();
    }
    // the lookup-advice stream is indexed from the Context's first queued cell: [0, origin_lookups) are the caller's
    if (fresh_lookup) lk_cells = (size_t)own_lookup_capacity + K * (size_t)nl.origin_lookups;
    else if (table && !group_m && nl.lookups_end > lookup_capacity) { lk_cells = (size_t)nl.lookups_end; lk_keep = (size_t)lookup_capacity; }   // the interludes' entries
    const bool clear = table && changed && !group_m;
    if (img_cells != none || lk_cells != none || clear) {
        int device = 0;
        hsw_engine_stream(engine, nullptr, &device);
        DeviceScope ds(device);
        if (!ds.ok) return HSW_ERR_NO_DEVICE;
        // (the callers run on a drained engine: nothing still writes the buffers replaced here)
        void *img = nullptr, *lk = nullptr;
        hipError_t he = hipSuccess;
        if (img_cells != none) he = fresh_zeroed(&img, img_cells * HSW_CELL_BYTES, d_gate, img_keep * HSW_CELL_BYTES);
        if (he == hipSuccess && lk_cells != none) he = fresh_zeroed(&lk, lk_cells * HSW_CELL_BYTES, d_lookup, lk_keep * HSW_CELL_BYTES);
        if (he != hipSuccess) { (void)hipFree(img); return hip_status(he); }
        if (img) { (void)hipFree(d_gate); d_gate = img; image_columns = nl.columns; }
        if (lk) { (void)hipFree(d_lookup); d_lookup = lk; lookup_capacity = lk_cells; }
        if (img || lk) free_compact_staging();            // sized for the old geometry
        const uint64_t end = image_columns * nl.max_rows;
        if (clear && clear_from < end)                    // cells an earlier layout wrote past the unchanged part
            (void)hipMemset(static_cast<uint8_t *>(d_gate) + (size_t)clear_from * HSW_CELL_BYTES, 0, (size_t)(end - clear_from) * HSW_CELL_BYTES);
    }
    layout = std::move(nl);
    place_dirty = place_dirty || changed;
    return HSW_OK;
}

int Context::set_columns(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t rows) {
    if (!whole || blocks_done != 0 || gate_cursor != 0) return HSW_ERR_INVALID_ARG;
    if (independent && !context_images) return HSW_ERR_UNSUPPORTED;   // K regions in one stream: linear only
    const uint64_t G = shape.gate_cells_per_block;
    if (rows < G + 16) return HSW_ERR_INVALID_ARG;        // keeps a block inside <= 2 columns (kernel: <= 2 breaks per block)
    if (layout.origin_row >= rows) return HSW_ERR_INVALID_ARG;   // the Context's next free row lies inside its column
    if (bound && rows > layout.pitch) return HSW_ERR_TOO_LARGE;  // a bound column holds column_pitch cells at most
    Layout nl = layout.origin();
    // (shared context -- a new layout: the declarations made for the old one are dropped)
    const std::vector<DigestOrigin> none(declared.size());
    int rc = plan_layout(sizes, rc_inputs, rows, none, &nl);
    if (rc == HSW_OK) rc = adopt(nl, true, false, 0);
    if (rc == HSW_OK) declared = none;
    return rc;
}

int Context::upload_place() {
    if (!place_dirty && d_place) return HSW_OK;
    // [jump cells n][cumulative gaps n][per digest: the caller's lookup entries before it, cumulative]
    const Layout &l = layout;
    const size_t nb = l.break_cell.size(), H = shared ? l.digest_lookup0.size() : by_pointer ? init_capacity : 0;
    std::vector<uint64_t> h;
    if (by_pointer) {
        // columns by pointer table: [jump cells n = breaks + 1][K cum rows of n][per digest], jump 0 at stream cell 0.
        // A jump into image column k of Context c lands break_cum (columns one pitch apart) + what column k really
        // lies from there: col_off - k * pitch, modulo 2^64 (PlaceTable::cum_stride)
        // then, by pointer table too (PlaceTable::lk_row / chip_row): [K lookup rows][K * ncols * 2 chip rows]
        const size_t n = nb + 1, K = contexts(), ncols = shape.num_advice_columns;
        const size_t rows0 = n + K * n + (H ? H : 1);
        h.assign(rows0 + (lookup_by_table() ? K : 0) + (chips_by_table() ? K * ncols * 2 : 0), 0);
        size_t at = rows0;
        for (size_t c = 0; c < K && lookup_by_table(); c++) h[at++] = lookup_extra(c);
        for (size_t c = 0; c < K && chips_by_table(); c++)
            for (size_t k = 0; k < ncols; k++) {
                h[at++] = chip_column_cell(c, k, false) - c * ctx_chip_rows();
                h[at++] = chip_column_cell(c, k, true) - c * ctx_chip_rows();
            }
        std::vector<uint64_t> col(n, 0);
        for (size_t k = 0; k < nb; k++) {
            h[1 + k] = l.break_cell[k];
            uint64_t c = 0;
            l.position(l.break_cell[k], &c, nullptr);
            col[1 + k] = c - l.origin_column;
        }
        for (size_t c = 0; c < K; c++)
            for (size_t k = 0; k < n; k++)
                h[n + c * n + k] = (k ? l.break_cum[k - 1] : 0) + column_cell(c, col[k]) - col[k] * l.column_pitch();
        for (size_t d = 0; d < H && shared; d++) h[n + K * n + d] = l.digest_lookup0[d] - l.origin_lookups - l.digest_entry0[d];
    } else {
        h.assign(2 * nb + (H ? H : 1), 0);
        for (size_t k = 0; k < nb; k++) { h[k] = l.break_cell[k]; h[nb + k] = l.break_cum[k]; }
        for (size_t d = 0; d < H; d++) h[2 * nb + d] = l.digest_lookup0[d] - l.origin_lookups - l.digest_entry0[d];
    }
    if (d_place && h == place_host) { place_dirty = false; return HSW_OK; }   // the device already holds this table
    int device = 0;
    hsw_engine_stream(engine, nullptr, &device);
    DeviceScope ds(device);
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
    hipError_t he = hipSuccess;
    if (h.size() > place_cap) {
        void *p = nullptr;
        he = hipMalloc(&p, h.size() * sizeof(uint64_t));
        if (he != hipSuccess) return hip_status(he);
        (void)hipFree(d_place);
        d_place = p;
        place_cap = h.size();
    }
    he = hipMemcpy(d_place, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) return HSW_ERR_HIP;
    place_host.swap(h);
    place_dirty = false;
    return HSW_OK;
}

int Context::set_origin(const std::vector<size_t> &sizes, bool rc_inputs, uint64_t column, uint64_t row, bool zero_cell_loaded,
                        uint64_t lookups_queued) {
    if (!whole || blocks_done != 0 || gate_cursor != 0 || lookup_cursor != layout.origin_lookups) return HSW_ERR_INVALID_ARG;
    if (independent && !context_images) return HSW_ERR_UNSUPPORTED;
    if (layout.max_rows && row >= layout.max_rows) return HSW_ERR_INVALID_ARG;
    // the new layout, checked in full: nothing is touched if it cannot be had.  The column breaks follow from where
    // the stream starts: a new row, or a zero cell that comes or goes, lays the image out again (a fresh image); a
    // shared context drops its declarations and has every cell of an earlier layout zeroed
    Layout nl = layout.origin();                          // (in the same memory: a bound region's pitches stay)
    nl.origin_column = column; nl.origin_row = row; nl.origin_lookups = lookups_queued; nl.origin_zero_loaded = zero_cell_loaded;
    const std::vector<DigestOrigin> none(declared.size());
    const int rc = plan_layout(sizes, rc_inputs, layout.max_rows, none, &nl);
    if (rc != HSW_OK) return rc;
    const bool fresh_image = layout.max_rows && (row != layout.origin_row || zero_cell_loaded != layout.origin_zero_loaded);
    const int rc2 = adopt(nl, fresh_image, lookups_queued != layout.origin_lookups, 0);
    if (rc2 != HSW_OK) return rc2;
    declared = none;
    lookup_cursor = lookups_queued;
    zero_loaded = zero_cell_loaded;                       // (without the zero cell the stream is one cell shorter)
    return HSW_OK;
}

int Context::bind(const std::vector<size_t> &sizes, bool rc_inputs, const hsw_region_binding &b_in, const hsw_column_tables *t) {
    const uint64_t K = contexts();
    const size_t ncols = shape.num_advice_columns;
    hsw_region_binding b = b_in;
    void *const *col_ptrs = t ? t->d_column_ptrs : nullptr;
    const size_t n_ptrs = t ? t->n_column_ptrs : 0;
    const bool lk_tab = t && t->d_lookup_ptrs, chip_tab = t && (t->d_chip_dense_ptrs || t->d_chip_spread_ptrs);
    auto entries_ok = [](void *const *p, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (!p[i] || ((uintptr_t)p[i] & 127u)) return false;
        return true;
    };
    if (t && !col_ptrs) return HSW_ERR_INVALID_ARG;       // (without an image table: hsw_gadget_bind_region)
    if (col_ptrs) {                                       // columns by pointer table: one pointer per column per proof
        if (b.columns_capacity == 0 || b.columns_capacity > ~(size_t)0 / (size_t)K || n_ptrs != (size_t)K * (size_t)b.columns_capacity) return HSW_ERR_INVALID_ARG;
        if (!entries_ok(col_ptrs, n_ptrs)) return HSW_ERR_INVALID_ARG;
        b.d_columns = col_ptrs[0];
        b.context_pitch = 0;
    }
    if (t && t->n_lookup_ptrs != (lk_tab ? (size_t)K : 0)) return HSW_ERR_INVALID_ARG;
    if (lk_tab) {                                         // ... and one per lookup-advice column
        if (!entries_ok(t->d_lookup_ptrs, (size_t)K)) return HSW_ERR_INVALID_ARG;
        b.d_lookup = t->d_lookup_ptrs[0];
        b.lookup_pitch = 0;
    }
    if (chip_tab && (!t->d_chip_dense_ptrs || !t->d_chip_spread_ptrs)) return HSW_ERR_INVALID_ARG;   // both families or neither
    if (t && t->n_chip_ptrs != (chip_tab ? (size_t)K * ncols : 0)) return HSW_ERR_INVALID_ARG;
    if (chip_tab) {                                       // ... and two per chip column
        if (!entries_ok(t->d_chip_dense_ptrs, (size_t)K * ncols) || !entries_ok(t->d_chip_spread_ptrs, (size_t)K * ncols)) return HSW_ERR_INVALID_ARG;
        b.d_chip_dense = t->d_chip_dense_ptrs[0]; b.d_chip_spread = t->d_chip_spread_ptrs[0];
        b.chip_col_stride = b.chip_context_pitch = 0;
    }
    const void *ptrs[4] = {b.d_columns, b.d_lookup, b.d_chip_dense, b.d_chip_spread};
    // (128 bytes: a column that starts on a line boundary keeps the realigned write-out on whole lines)
    for (const void *p : ptrs)
        if (!p || ((uintptr_t)p & 127u)) return HSW_ERR_INVALID_ARG;
    // (a block's cells are addressed by 32-bit byte offsets from its first, the gaps of <= 2 column breaks included)
    if (b.column_pitch < layout.max_rows || b.column_pitch > (1ull << 24)) return HSW_ERR_INVALID_ARG;
    if (!chip_tab && b.chip_col_stride < b.chip_rows_capacity) return HSW_ERR_INVALID_ARG;
    if (K > 1) {
        if (!col_ptrs && (b.columns_capacity > ~0ull / b.column_pitch || b.context_pitch < b.columns_capacity * b.column_pitch)) return HSW_ERR_INVALID_ARG;
        if (!lk_tab && b.lookup_pitch < b.lookup_capacity) return HSW_ERR_INVALID_ARG;
        if (b.context_pitch > ~0ull / (K * HSW_CELL_BYTES) || b.lookup_pitch > ~0ull / (K * HSW_CELL_BYTES) ||
            b.chip_context_pitch > ~0ull / (K * HSW_CELL_BYTES))
            return HSW_ERR_INVALID_ARG;
    }
    Layout nl = layout.origin();
    nl.pitch = b.column_pitch;
    nl.image_pitch = K > 1 ? b.context_pitch : 0;
    const int rc = plan_layout(sizes, rc_inputs, layout.max_rows, declared, &nl);
    if (rc != HSW_OK) return rc;
    // (cells from entry 0, modulo 2^64: an entry below entry 0 wraps, and wraps back when the kernels scale by the cell size)
    auto offsets = [](void *const *p, size_t n) {
        std::vector<uint64_t> o(n);
        for (size_t i = 0; i < n; i++) o[i] = (uint64_t)((uintptr_t)p[i] - (uintptr_t)p[0]) / HSW_CELL_BYTES;
        return o;
    };
    std::vector<uint64_t> off, lko, cdo, cso;
    if (col_ptrs) off = offsets(col_ptrs, n_ptrs);
    if (lk_tab) lko = offsets(t->d_lookup_ptrs, (size_t)K);
    if (chip_tab) { cdo = offsets(t->d_chip_dense_ptrs, (size_t)K * ncols); cso = offsets(t->d_chip_spread_ptrs, (size_t)K * ncols); }
    if (nl.columns > b.columns_capacity || lookups_needed(nl) > b.lookup_capacity || ctx_chip_rows() > b.chip_rows_capacity) return HSW_ERR_TOO_LARGE;
    // (the caller ran on a drained engine: nothing still writes the buffers given up here)
    if (!bound) {
        int device = 0;
        hsw_engine_stream(engine, nullptr, &device);
        DeviceScope ds(device);
        if (!ds.ok) return HSW_ERR_NO_DEVICE;
        (void)hipFree(d_gate); (void)hipFree(d_lookup); (void)hipFree(d_chip_dense); (void)hipFree(d_chip_spread);
    }
    free_compact_staging();
    bound = true;
    binding = b;
    by_pointer = col_ptrs != nullptr;
    col_off.swap(off);
    lk_off.swap(lko); chip_dense_off.swap(cdo); chip_spread_off.swap(cso);
    d_gate = b.d_columns; d_lookup = b.d_lookup; d_chip_dense = b.d_chip_dense; d_chip_spread = b.d_chip_spread;
    chip_col_stride = (size_t)b.chip_col_stride;
    image_columns = b.columns_capacity;
    layout = std::move(nl);
    lookup_capacity = (K - 1) * lookup_pitch() + b.lookup_capacity;
    place_dirty = true;
    return HSW_OK;
}

int Context::unbind(const std::vector<size_t> &sizes, bool rc_inputs) {
    if (!bound) return HSW_OK;
    const size_t K = contexts();
    Layout nl = layout.origin();
    nl.pitch = nl.image_pitch = 0;
    const int rc = plan_layout(sizes, rc_inputs, layout.max_rows, declared, &nl);
    if (rc != HSW_OK) return rc;
    int device = 0;
    hsw_engine_stream(engine, nullptr, &device);
    DeviceScope ds(device);
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
    // what a fresh gadget with this layout owns (new_context, adopt)
    const size_t stride = (size_t)hsw_chip_rows(&shape, 0, capacity_blocks);
    const size_t col_bytes = (size_t)shape.num_advice_columns * (stride ? stride : 1) * HSW_CELL_BYTES;
    const size_t lk_cells = shared && group_m ? K * (size_t)nl.lookups_end : shared ? (size_t)std::max(nl.lookups_end, own_lookup_capacity)
                                                                                   : (size_t)own_lookup_capacity + K * (size_t)nl.origin_lookups;
    void *img = nullptr, *lk = nullptr, *cd = nullptr, *cs = nullptr;
    hipError_t he = fresh_zeroed(&img, K * (size_t)nl.image_cells() * HSW_CELL_BYTES);
    if (he == hipSuccess) he = fresh_zeroed(&lk, lk_cells * HSW_CELL_BYTES);
    if (he == hipSuccess) he = fresh_zeroed(&cd, col_bytes);
    if (he == hipSuccess) he = fresh_zeroed(&cs, col_bytes);
    if (he != hipSuccess) { (void)hipFree(img); (void)hipFree(lk); (void)hipFree(cd); (void)hipFree(cs); return hip_status(he); }
    bound = false;
    by_pointer = false;
    col_off.clear();
    lk_off.clear(); chip_dense_off.clear(); chip_spread_off.clear();
    binding = hsw_region_binding{};
    d_gate = img; d_lookup = lk; d_chip_dense = cd; d_chip_spread = cs;
    chip_col_stride = stride;
    image_columns = nl.columns;
    lookup_capacity = lk_cells;
    layout = std::move(nl);
    place_dirty = true;
    return HSW_OK;
}

// Where the launches of a batch write -- or, for hsw_gadget_verify, read: the generator and the verifier build
// their arguments here and nowhere else, so they agree in every kind of layout.  Made once per batch (what the
// frame launches need too), then filled in per launch.  `a`, `tbl` and `period` point at each other: not copyable.
struct Launch {
    const Context &c;
    const uint8_t *in_blocks;                 // the staging the batch's inputs are in, indexed by absolute block
    const uint32_t *in_pre;
    uint32_t flags;
    hsw_witness_args a{};
    hsw_pack_plan rel{};                      // plain image, context images: the breaks relative to the launch's first cell
    hsw_pack_plan abs{};                      // ... and as they are, for the frames (cell indices from stream cell 0)
    const hsw_pack_plan *frame_pack = nullptr;
    PlaceTable tbl{};                         // shared context: the jump table on the device (upload_place)
    ContextPeriod period{0, 0};
    const ContextPeriod *per = nullptr;       // context images: one Context's period; shared context: the table; else NULL

    Launch(const Context &ctx, bool inputs_in_pinned, uint32_t repr_flags)
        : c(ctx), in_blocks(inputs_in_pinned ? ctx.dp_blocks : ctx.d_blocks), in_pre(inputs_in_pinned ? ctx.dp_pre : ctx.d_pre_states),
          flags(repr_flags) {
        const Layout &l = c.layout;
        if (c.table_path()) {
            const uint64_t *d_place = static_cast<const uint64_t *>(c.d_place);
            size_t n = l.break_cell.size();
            tbl = PlaceTable{d_place, d_place + n, d_place + 2 * n, n, 0};
            if (c.by_pointer) {                          // jump 0 at cell 0, a cum row per Context (upload_place)
                n += 1;
                tbl = PlaceTable{d_place, d_place + n, d_place + n + c.contexts() * n, n, 0};
                tbl.cum_stride = n;
                // the lookup and chip rows after the per-digest shifts (upload_place)
                const uint64_t *rows = tbl.lk_shift + (c.shared ? l.digest_lookup0.size() ? l.digest_lookup0.size() : 1 : c.init_capacity ? c.init_capacity : 1);
                if (c.lookup_by_table()) { tbl.lk_row = rows; rows += c.contexts(); }
                if (c.chips_by_table()) tbl.chip_row = rows;
            }
            period.place = &tbl;
            per = &period;
            if (l.period) {                              // the periodic table: one Context's, every l.period stream cells
                const uint64_t image = c.by_pointer ? 0 : l.image_cells();      // (by pointer: the Context's cum row says where)
                tbl.ctx_blocks = c.blocks_per_context(); tbl.ctx_stream = l.period; tbl.ctx_image = image;
                period.stream_cells = l.period; period.image_cells = image;
            }
            period.chip_ctx_extra = c.chip_ctx_extra(); period.chip_rows_checked = c.bound;
        } else if (l.max_rows) {
            abs.n_breaks = (uint32_t)l.break_cell.size();
            for (size_t k = 0; k < abs.n_breaks; k++) { abs.break_cell[k] = l.break_cell[k]; abs.break_gap[k] = l.break_gap[k]; }
            frame_pack = &abs;
            if (l.period) { period = ContextPeriod{l.period, l.image_cells()}; per = &period; }
            period.chip_ctx_extra = c.chip_ctx_extra(); period.chip_rows_checked = c.bound;
        }
    }
    Launch(const Launch &) = delete;

    // n_blocks blocks from absolute block first_block on.  The chip cursor is the running num_limb_sum; column buffers
    // are addressed from absolute row 0 (cursor origin of the context).  Block-stream contexts: that is all
    void blocks(size_t first_block, size_t n_blocks) {
        const size_t cb = hsw_cell_bytes(flags);
        a = hsw_witness_args{};
        a.d_blocks = in_blocks + 64 * first_block; a.d_pre_states = in_pre + 8 * first_block; a.n_blocks = n_blocks;
        a.spread_cursor0 = (uint64_t)first_block * c.shape.limb_calls_per_block;
        // (a bound region: the chip rows of the launch's first Context, where the caller keeps that Context's)
        const size_t row_shift = (size_t)c.chip_launch_cell(a.spread_cursor0 - a.spread_cursor0 % c.shape.num_advice_columns);
        a.d_gate = static_cast<uint8_t *>(c.d_gate) + first_block * (size_t)c.shape.gate_cells_per_block * cb;
        a.d_chip_dense = static_cast<uint8_t *>(c.d_chip_dense) + row_shift * cb;
        a.d_chip_spread = static_cast<uint8_t *>(c.d_chip_spread) + row_shift * cb;
        a.chip_col_stride = c.chip_col_stride;
        a.d_next_states = c.d_next_states + 8 * first_block;
        a.flags = flags;
    }

    // Whole-digest contexts: the block streams of n_digests equally sized digests (shape fs) as ONE launch -- the
    // kernel skips the frame between two of them.  digest0: the first one's index in the pass, r0: its cells
    void run(size_t digest0, const AssignedHashResult &r0, size_t first_block, size_t n_digests, const hsw_frame_shape &fs) {
        blocks(first_block, (size_t)fs.n_blocks * n_digests);
        const size_t cb = hsw_cell_bytes(flags);
        const Layout &l = c.layout;
        // (context images: the run's first block in ITS Context's image; the breaks are that Context's)
        const uint64_t ctx0 = l.period ? r0.block_cell / l.period : 0, local = r0.block_cell - ctx0 * l.period;
        a.d_gate = static_cast<uint8_t *>(c.gate_stream()) + (size_t)((c.by_pointer ? 0 : ctx0 * l.image_cells()) + local) * cb;
        a.d_lookup = static_cast<uint8_t *>(c.d_lookup) + (size_t)(r0.block_lookup + c.lookup_extra(ctx0)) * cb;   // (by table: the Context's own column)
        a.frame_every = fs.n_blocks;
        // between the block streams of two digests: one epilogue, the next prologue -- and the next Context's zero cell
        // when every digest is a Context of its own, and (context images) its caller-owned lookup cells
        a.frame_cells = fs.epilogue_cells + fs.prologue_cells + (c.independent && !l.origin_zero_loaded ? 1u : 0u);
        a.frame_lookups = fs.epilogue_lookups + fs.prologue_lookups + (c.context_images ? l.origin_lookups + (c.lookup_pitch() - c.ctx_lookups()) : 0u);
        // (a Context group: the "digests" of the run are the SAME digest index of consecutive Contexts, whose lookup
        //  columns lie ctx_lookups() apart and whose blocks ctx_blocks apart -- PlaceTable::ctx_blocks)
        if (c.group_m) a.frame_lookups = c.lookup_pitch() - (uint64_t)fs.n_blocks * c.shape.lookup_cells_per_block;
        if (period.place) {                              // the run's first block cell, its digests' lookup shifts
            tbl.base = local;
            const uint64_t *shifts = c.by_pointer ? tbl.cum + c.contexts() * tbl.n : tbl.cell + 2 * tbl.n;
            tbl.lk_shift = shifts + (c.group_m ? digest0 % c.group_m : c.context_images ? 0 : digest0);
            if (c.by_pointer && l.period) {
                // a pointer table's Contexts: block b of the launch is block b % frame_every of Context ctx0 + b / frame_every,
                // whose cells go through ITS cum row from the Context's own stream cell on -- no image offset (ctx_cells = 0),
                // and stepping a Context steps the stream back by the Context's blocks: frame_cells = -(frame_every * G), mod 2^64
                tbl.ctx0 = ctx0;
                a.frame_cells = 0 - (uint64_t)fs.n_blocks * c.shape.gate_cells_per_block;
            }
        } else if (frame_pack) {                         // breaks before the launch's first cell are pure offsets
            rel.n_breaks = abs.n_breaks;
            for (uint32_t k = 0; k < rel.n_breaks; k++) {
                rel.break_cell[k] = abs.break_cell[k] > local ? abs.break_cell[k] - local : 0;
                rel.break_gap[k] = abs.break_gap[k];
            }
            a.pack = &rel;
        }
    }
};

// The expansion (and verify) launches of a batch of n digests from digest d0 of the pass on, as runs of `count` digests
// `step` apart from batch index `first`: neighbours of equal size (blocks_of(i): digest i of the batch) -- or, in a
// Context group, digest index j of every Context the batch holds it of: M launches, not K * M
struct Run { size_t first, count, step; };
template <class BlocksOf>
std::vector<Run> batch_runs(const Context &c, size_t d0, size_t n, BlocksOf blocks_of) {
    std::vector<Run> runs;
    if (c.group_m) {
        const size_t M = c.group_m;
        for (size_t j = 0; j < M; j++) {
            const size_t c_lo = d0 > j ? (d0 - j + M - 1) / M : 0;      // the first Context whose digest j the batch holds
            const size_t first = c_lo * M + j;
            if (first >= d0 + n) continue;
            runs.push_back(Run{first - d0, (d0 + n - first + M - 1) / M, M});
        }
        return runs;
    }
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        while (j < n && blocks_of(j) == blocks_of(i)) j++;
        runs.push_back(Run{i, j - i, 1});
        i = j;
    }
    return runs;
}

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
    // ---- device: chain pre-pass + ONE expansion launch for the whole batch ----
    hipStream_t stream = nullptr;
    int device = 0;
    hsw_engine_stream(ctx.engine, reinterpret_cast<void **>(&stream), &device);
    DeviceScope ds(device);
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
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
            size_t ob = 0;
            for (size_t i = 0; i < n && rc == HSW_OK; i++) {
                rc = hsw_frame_query(&ctx.shape, max_variable_byte_sizes[cur_hash_idx + i], is_input_range_check ? 1 : 0, &fss[i]);
                if (rc != HSW_OK) break;
                hsw_frame_desc &d = frames[i];
                AssignedHashResult &r = results[i];
                d.input_len = input_lens[i];
                d.first_block = b0 + ob;
                d.n_blocks = (uint32_t)plans[i].max_variable_round;
                d.num_round = (uint32_t)plans[i].num_round;
                d.precomputed_round = (uint32_t)plans[i].precomputed_round;
                d.is_input_range_check = is_input_range_check ? 1u : 0u;
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
                // (lookup columns by pointer table: the frame kernels address through the Context's offset, positions stay)
                const uint64_t lx = ctx.lookup_extra(ctx.context_images ? cur_hash_idx + i : ctx.group_m ? (cur_hash_idx + i) / ctx.group_m : 0);
                r.prologue_cell = d.prologue_cell = gc;      gc += fss[i].prologue_cells;
                r.prologue_lookup = lc; d.prologue_lookup = lc + lx;  lc += fss[i].prologue_lookups;
                d.zero_cell = ~0ull;
                if (!zero_loaded || own_zero) { d.zero_cell = gc++; zero_loaded = true; }   // compression.rs:34 of the first block of a Context
                r.block_cell = gc;                           gc += (uint64_t)d.n_blocks * G;
                r.block_lookup = lc;                         lc += (uint64_t)d.n_blocks * LK;
                r.epilogue_cell = d.epilogue_cell = gc;      gc += fss[i].epilogue_cells;
                r.epilogue_lookup = lc; d.epilogue_lookup = lc + lx;  lc += fss[i].epilogue_lookups;
                r.end_cell = gc;
                ob += d.n_blocks;
            }
            if (rc == HSW_OK && (gc > ctx.gate_capacity || lc > ctx.lookup_capacity)) rc = HSW_ERR_INVALID_ARG;
            ob = 0;
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
        r.input_len = input_lens[i];
        r.input_bytes = std::move(plans[i].blocks);          // the plan is done with them (copied to the staging above)
        r.first_block = b0 + off;
        r.n_blocks = pl.max_variable_round;
        r.spread_cursor0 = ctx.num_limb_sum + (uint64_t)off * ctx.shape.limb_calls_per_block;
        r.num_round = pl.num_round;
        r.target_round = pl.target_round;
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
        int device = 0;
        hsw_engine_stream(ctx.engine, nullptr, &device);
        DeviceScope ds(device);
        if (!ds.ok) return HSW_ERR_NO_DEVICE;
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

// ------------------------------------------------------------------- C ABI

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

extern "C" {

int hsw_digest_prepare(const uint8_t *input, size_t input_len, size_t precomputed_input_len,
                       size_t max_variable_byte_size, uint8_t *blocks_out, uint32_t init_state_out[8],
                       hsw_digest_info *info) try {
    hsw::DigestPlan plan;
    const int rc = hsw::digest_prepare(input, input_len, precomputed_input_len, max_variable_byte_size, &plan);
    if (rc != HSW_OK) return rc;
    if (blocks_out && !plan.blocks.empty()) std::memcpy(blocks_out, plan.blocks.data(), plan.blocks.size());
    if (init_state_out) std::memcpy(init_state_out, plan.init_state, 32);
    if (info) {
        info->num_round = plan.num_round;
        info->precomputed_round = plan.precomputed_round;
        info->target_round = plan.target_round;
        info->n_blocks = plan.max_variable_round;
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_create(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t n_hashes,
                      int is_input_range_check, hsw_gadget **out) try {
    return hsw_gadget_create_ex(e, max_variable_byte_sizes, n_hashes, is_input_range_check, 0, out);
} HSW_NO_UNWIND

int hsw_gadget_create_ex(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t n_hashes,
                         int is_input_range_check, uint32_t flags, hsw_gadget **out) try {
    if (!e || !out || (!max_variable_byte_sizes && n_hashes)) return HSW_ERR_INVALID_ARG;
    if (flags & ~(HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES | HSW_GADGET_SHARED_CONTEXT))
        return HSW_ERR_INVALID_ARG;
    const bool shared = (flags & HSW_GADGET_SHARED_CONTEXT) != 0;
    if (shared && (!(flags & HSW_GADGET_WHOLE_DIGEST) || (flags & (HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES))))
        return HSW_ERR_INVALID_ARG;
    if ((flags & HSW_GADGET_INDEPENDENT) && !(flags & HSW_GADGET_WHOLE_DIGEST)) return HSW_ERR_INVALID_ARG;
    const bool images = (flags & HSW_GADGET_CONTEXT_IMAGES) != 0;
    if (images && !(flags & HSW_GADGET_INDEPENDENT)) return HSW_ERR_INVALID_ARG;
    *out = nullptr;
    for (size_t i = 1; images && i < n_hashes; i++)        // K proofs of ONE circuit: every Context laid out alike
        if (max_variable_byte_sizes[i] != max_variable_byte_sizes[0]) return HSW_ERR_UNSUPPORTED;
    hsw_shape s;
    int rc = hsw_engine_shape(e, &s);
    if (rc != HSW_OK) return rc;
    if (shared && s.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;   // the table-path kernels: the 8-bit spread table
    hsw_gadget *g = new (std::nothrow) hsw_gadget();
    if (!g) return HSW_ERR_NOMEM;
    std::vector<size_t> sizes(max_variable_byte_sizes, max_variable_byte_sizes + n_hashes);
    rc = hsw::Sha256DynamicConfig::configure(sizes, s.num_bits_lookup, s.num_advice_columns,
                                             is_input_range_check != 0, &g->cfg);
    if (rc == HSW_OK) rc = g->cfg.new_context(e, &g->ctx, (flags & HSW_GADGET_WHOLE_DIGEST) != 0, (flags & HSW_GADGET_INDEPENDENT) != 0,
                                              images, shared);
    if (rc != HSW_OK) { delete g; return rc; }
    *out = g;
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_create_contexts(hsw_engine *e, const size_t *max_variable_byte_sizes, size_t digests_per_context,
                               size_t n_contexts, int is_input_range_check, uint32_t flags, hsw_gadget **out) try {
    if (!e || !out || !max_variable_byte_sizes || digests_per_context == 0 || n_contexts == 0) return HSW_ERR_INVALID_ARG;
    // (HSW_GADGET_SHARED_CONTEXT may be named: every Context of a group is one; the K-proof flags of create_ex are not this)
    if (!(flags & HSW_GADGET_WHOLE_DIGEST) || (flags & ~(HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_SHARED_CONTEXT))) return HSW_ERR_INVALID_ARG;
    *out = nullptr;
    hsw_shape s;
    int rc = hsw_engine_shape(e, &s);
    if (rc != HSW_OK) return rc;
    if (s.mode != HSW_MODE_HALO2_INTERNALS) return HSW_ERR_INVALID_ARG;
    if (s.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;              // the table-path kernels: the 8-bit spread table
    if (n_contexts > (~(size_t)0 >> 8) / digests_per_context) return HSW_ERR_TOO_LARGE;
    hsw_gadget *g = new (std::nothrow) hsw_gadget();
    if (!g) return HSW_ERR_NOMEM;
    std::vector<size_t> sizes;                               // digest d of the pass: digest d % M of Context d / M
    sizes.reserve(digests_per_context * n_contexts);
    for (size_t c = 0; c < n_contexts; c++) sizes.insert(sizes.end(), max_variable_byte_sizes, max_variable_byte_sizes + digests_per_context);
    rc = hsw::Sha256DynamicConfig::configure(sizes, s.num_bits_lookup, s.num_advice_columns, is_input_range_check != 0, &g->cfg);
    if (rc == HSW_OK) rc = g->cfg.new_context(e, &g->ctx, true, false, false, true, digests_per_context);
    if (rc != HSW_OK) { delete g; return rc; }
    *out = g;
    return HSW_OK;
} HSW_NO_UNWIND

void hsw_gadget_destroy(hsw_gadget *g) {
    if (!g) return;
    if (g->d_pairs) {                                        // (every check that used it was synchronous)
        int device = 0;
        hsw_engine_stream(g->ctx->engine, nullptr, &device);
        hsw::DeviceScopeG ds(device);
        (void)hipFree(g->d_pairs);
    }
    delete g->ctx;
    delete g;
}

static void fill_result(const hsw::AssignedHashResult &r, hsw_hash_result *o) {
    o->input_len = r.input_len;
    o->first_block = r.first_block;
    o->n_blocks = r.n_blocks;
    o->spread_cursor0 = r.spread_cursor0;
    o->num_round = r.num_round;
    o->target_round = r.target_round;
    std::memcpy(o->output_bytes, r.output_bytes, 32);
    o->prologue_cell = r.prologue_cell; o->block_cell = r.block_cell;
    o->epilogue_cell = r.epilogue_cell; o->end_cell = r.end_cell;
    o->prologue_lookup = r.prologue_lookup; o->block_lookup = r.block_lookup;
    o->epilogue_lookup = r.epilogue_lookup;
}

int hsw_gadget_digest_batch(hsw_gadget *g, size_t n, const uint8_t *const *inputs, const size_t *input_lens,
                            const size_t *precomputed_input_lens, hsw_hash_result *results) try {
    if (!g || !results) return HSW_ERR_INVALID_ARG;
    std::vector<hsw::AssignedHashResult> rs(n);
    const int rc = g->cfg.digest_batch(*g->ctx, n, inputs, input_lens, precomputed_input_lens, rs.data());
    if (rc != HSW_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        fill_result(rs[i], &results[i]);
        g->results.push_back(std::move(rs[i]));
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_digest_batch_device(hsw_gadget *g, size_t n, const void *const *d_inputs, const size_t *input_lens,
                                   const size_t *precomputed_input_lens, hsw_hash_result *results) try {
    if (!g || !results) return HSW_ERR_INVALID_ARG;
    std::vector<hsw::AssignedHashResult> rs(n);
    const int rc = g->cfg.digest_batch_device(*g->ctx, n, d_inputs, input_lens, precomputed_input_lens, rs.data());
    if (rc != HSW_OK) return rc;
    // (nothing to intersect without an earlier destination in the pass: no bookkeeping)
    if (g->ctx->whole && !g->tie_owners.empty()) g->record_ties(g->results.size(), n, d_inputs, input_lens, precomputed_input_lens, nullptr);
    for (size_t i = 0; i < n; i++) {
        fill_result(rs[i], &results[i]);
        g->results.push_back(std::move(rs[i]));
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_digest_levels_device(hsw_gadget *g, size_t n, const void *const *d_inputs, const size_t *input_lens,
                                    const size_t *precomputed_input_lens, const uint32_t *levels, void *const *d_outputs,
                                    hsw_hash_result *results) try {
    if (!g || !results) return HSW_ERR_INVALID_ARG;
    std::vector<hsw::AssignedHashResult> rs(n);
    const int rc = g->cfg.digest_levels_device(*g->ctx, n, d_inputs, input_lens, precomputed_input_lens, levels, d_outputs, rs.data());
    if (rc != HSW_OK) return rc;
    if (g->ctx->whole && (d_outputs || !g->tie_owners.empty())) g->record_ties(g->results.size(), n, d_inputs, input_lens, precomputed_input_lens, d_outputs);
    for (size_t i = 0; i < n; i++) {
        fill_result(rs[i], &results[i]);
        g->results.push_back(std::move(rs[i]));
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_digest(hsw_gadget *g, const uint8_t *input, size_t input_len, size_t precomputed_input_len,
                      hsw_hash_result *result) try {
    return hsw_gadget_digest_batch(g, 1, &input, &input_len, &precomputed_input_len, result);
} HSW_NO_UNWIND

int hsw_gadget_streams(hsw_gadget *g, hsw_gadget_view *view) try {
    if (!g || !view) return HSW_ERR_INVALID_ARG;
    view->d_gate = g->ctx->d_gate;
    view->d_chip_dense = g->ctx->d_chip_dense;
    view->d_chip_spread = g->ctx->d_chip_spread;
    view->d_next_states = g->ctx->d_next_states;
    view->chip_col_stride = g->ctx->chip_col_stride;
    view->blocks_done = g->ctx->blocks_done;
    view->capacity_blocks = g->ctx->capacity_blocks;
    view->num_limb_sum = g->ctx->num_limb_sum;
    view->cur_hash_idx = g->cfg.cur_hash_idx;
    view->gate_cells = g->ctx->gate_cursor;
    view->gate_capacity = g->ctx->gate_capacity;
    view->d_lookup = g->ctx->d_lookup;
    view->lookup_cells = g->ctx->lookup_cursor;
    view->lookup_capacity = g->ctx->lookup_capacity;
    view->max_rows = g->ctx->layout.max_rows;
    view->columns = g->ctx->layout.columns;
    view->origin_column = g->ctx->layout.origin_column;
    view->origin_row = g->ctx->layout.origin_row;
    view->origin_lookups = g->ctx->layout.origin_lookups;
    view->origin_zero_loaded = g->ctx->layout.origin_zero_loaded ? 1u : 0u;
    view->reserved_ = 0;
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_input_bytes(hsw_gadget *g, size_t hash_idx, uint8_t *out, size_t cap, size_t *len) try {
    if (!g || hash_idx >= g->results.size()) return HSW_ERR_INVALID_ARG;
    const std::vector<uint8_t> &b = g->results[hash_idx].input_bytes;
    if (len) *len = b.size();
    if (out) {
        if (cap < b.size()) return HSW_ERR_INVALID_ARG;
        if (!b.empty()) std::memcpy(out, b.data(), b.size());
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_result_cells(const hsw_gadget *g, size_t hash_idx, hsw_result_cells *out) try {
    if (!g || !out || hash_idx >= g->results.size()) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_INVALID_ARG;                  // block-stream contexts hold no frame cells
    const hsw::AssignedHashResult &r = g->results[hash_idx];
    std::memset(out, 0, sizeof *out);
    out->input_len_cell = r.prologue_cell + hsw::frame::P_LEN;
    out->input_bytes_cell0 = r.prologue_cell + hsw::frame::P_BYTES;
    out->n_input_bytes = (uint64_t)r.n_blocks * 64;
    g->ctx->layout.position(out->input_len_cell, &out->input_len_pos[0], &out->input_len_pos[1]);
    g->ctx->layout.position(out->input_bytes_cell0, &out->input_bytes_pos0[0], &out->input_bytes_pos0[1]);
    for (uint32_t w = 0; w < 8; w++)
        for (uint32_t i = 0; i < 4; i++) {
            const uint64_t cell = r.epilogue_cell + (uint64_t)hsw::frame::E_STATE * (r.n_blocks + 1) +
                                  (uint64_t)hsw::frame::E_WORD * w + 5u * i;
            out->output_byte_cells[4 * w + i] = cell;
            g->ctx->layout.position(cell, &out->output_byte_pos[4 * w + i][0], &out->output_byte_pos[4 * w + i][1]);
        }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_set_columns(hsw_gadget *g, uint64_t max_rows, uint64_t *n_columns) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    int rc = hsw_engine_synchronize(g->ctx->engine);          // the image is reallocated: nothing may still write the old one
    if (rc == HSW_OK) rc = g->ctx->set_columns(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, max_rows);
    if (rc == HSW_OK && n_columns) *n_columns = g->ctx->layout.columns;
    if (rc == HSW_OK) hsw::drop_region_tape_positions(g->tape);     // the codes are per stream cell; image positions follow the layout
    return rc;
} HSW_NO_UNWIND

int hsw_gadget_set_origin(hsw_gadget *g, uint64_t column, uint64_t row, int zero_cell_loaded,
                          uint64_t lookups_already_queued) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (!c.whole || g->cfg.cur_hash_idx != 0) return HSW_ERR_INVALID_ARG;   // before the first digest of a synthesis pass
    int rc = hsw_engine_synchronize(c.engine);
    if (rc != HSW_OK) return rc;
    const uint64_t old_row = c.layout.origin_row;
    const bool old_zero = c.layout.origin_zero_loaded;
    rc = c.set_origin(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, column, row, zero_cell_loaded != 0,
                      lookups_already_queued);
    if (rc != HSW_OK) return rc;                                  // (nothing was touched: origin, layout and tape as before)
    // the region tape (hsw_replay.cpp) numbers stream cells: only a zero cell that comes or goes changes it; a new
    // origin row moves the witnesses' image positions; column and queued lookups are offsets applied at delivery.
    // A prover that synthesizes the same circuit pass after pass keeps its tape.
    if (old_zero != (zero_cell_loaded != 0)) { hsw::free_region_tape(g->tape); g->tape = nullptr; }
    else if (old_row != row) hsw::drop_region_tape_positions(g->tape);
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_set_digest_origin(hsw_gadget *g, size_t h, uint64_t column, uint64_t row, uint64_t lookups_queued) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    const size_t n = c.group_m ? c.group_m : g->cfg.max_variable_byte_sizes.size();   // (a group: digest h of every Context alike)
    if (!c.shared || !c.layout.max_rows || h < 1 || h >= n || h < g->cfg.cur_hash_idx || row >= c.layout.max_rows)
        return HSW_ERR_INVALID_ARG;
    const hsw::DigestOrigin &was = c.declared[h];
    // the same declaration again (the next pass declaring what the last one did) changes nothing: the later digests'
    // layout depends on it only, so their declarations stay too
    if (was.set && was.column == column && was.row == row && was.lookups == lookups_queued) return HSW_OK;
    // digest h's declaration replaces the old one and drops the later ones (their layout follows from it)
    std::vector<hsw::DigestOrigin> decl(c.declared.begin(), c.declared.begin() + (ptrdiff_t)h);
    decl.resize(n);
    decl[h].set = true; decl[h].column = column; decl[h].row = row; decl[h].lookups = lookups_queued;
    int rc = hsw_engine_synchronize(c.engine);           // the image may grow: nothing may still write the old one
    if (rc != HSW_OK) return rc;
    // (cells past digest h-1's end: the same in both layouts up to there, stale beyond it if the layout changes)
    const uint64_t clear_from = c.layout.image_cell(c.layout.digest_cell0[h] - 1) + 1;
    hsw::Layout nl = c.layout.origin();
    rc = c.plan_layout(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, c.layout.max_rows, decl, &nl);
    if (rc == HSW_OK) rc = c.adopt(nl, false, false, clear_from);
    if (rc != HSW_OK) return rc;
    c.declared.swap(decl);
    hsw::drop_region_tape_positions(g->tape);           // the witnesses' image positions follow the layout
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_bind_region(hsw_gadget *g, const hsw_region_binding *b) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    // a whole-digest gadget with a column image (K linear regions in one stream, block streams: nothing to bind)
    if (!c.whole || !c.layout.max_rows) return HSW_ERR_UNSUPPORTED;
    if (g->cfg.cur_hash_idx != 0 || c.blocks_done != 0 || c.gate_cursor != 0) return HSW_ERR_INVALID_ARG;   // a fresh or reset gadget
    int rc = hsw_engine_synchronize(c.engine);           // buffers change hands: nothing may still write the old ones
    if (rc != HSW_OK) return rc;
    rc = b ? c.bind(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, *b)
           : c.unbind(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check);
    if (rc == HSW_OK) hsw::drop_region_tape_positions(g->tape);     // image positions follow the pitches
    return rc;
} HSW_NO_UNWIND

int hsw_gadget_bind_columns(hsw_gadget *g, const hsw_region_binding *b, void *const *d_column_ptrs, size_t n_ptrs) try {
    if (!g || !b || !d_column_ptrs) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (!c.whole || !c.layout.max_rows) return HSW_ERR_UNSUPPORTED;
    if (g->cfg.cur_hash_idx != 0 || c.blocks_done != 0 || c.gate_cursor != 0) return HSW_ERR_INVALID_ARG;   // a fresh or reset gadget
    // (the table-path kernels: the 8-bit spread table, as for shared contexts)
    if (c.shape.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;
    int rc = hsw_engine_synchronize(c.engine);
    if (rc != HSW_OK) return rc;
    hsw_column_tables t{};
    t.d_column_ptrs = d_column_ptrs; t.n_column_ptrs = n_ptrs;
    rc = c.bind(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, *b, &t);
    if (rc == HSW_OK) hsw::drop_region_tape_positions(g->tape);
    return rc;
} HSW_NO_UNWIND

int hsw_gadget_bind_column_tables(hsw_gadget *g, const hsw_region_binding *b, const hsw_column_tables *t) try {
    if (!g || !b || !t || !t->d_column_ptrs) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (!c.whole || !c.layout.max_rows) return HSW_ERR_UNSUPPORTED;
    if (g->cfg.cur_hash_idx != 0 || c.blocks_done != 0 || c.gate_cursor != 0) return HSW_ERR_INVALID_ARG;   // a fresh or reset gadget
    if (c.shape.num_bits_lookup != 8) return HSW_ERR_UNSUPPORTED;        // (the table-path kernels, as hsw_gadget_bind_columns)
    int rc = hsw_engine_synchronize(c.engine);
    if (rc != HSW_OK) return rc;
    rc = c.bind(g->cfg.max_variable_byte_sizes, g->cfg.is_input_range_check, *b, t);
    if (rc == HSW_OK) hsw::drop_region_tape_positions(g->tape);
    return rc;
} HSW_NO_UNWIND

int hsw_gadget_region_binding(const hsw_gadget *g, hsw_region_binding *out) try {
    if (!g || !out) return HSW_ERR_INVALID_ARG;
    const hsw::Context &c = *g->ctx;
    if (c.bound) { *out = c.binding; return HSW_OK; }
    const bool many = c.contexts() > 1;
    std::memset(out, 0, sizeof *out);
    out->d_columns = c.d_gate;
    out->column_pitch = c.layout.column_pitch();
    out->columns_capacity = c.shared && !c.group_m && c.image_columns ? c.image_columns : c.layout.columns;
    out->context_pitch = c.layout.image_cells();
    out->d_lookup = c.d_lookup;
    out->lookup_capacity = many ? c.ctx_lookups() : c.lookup_capacity;
    out->lookup_pitch = c.lookup_pitch();
    out->d_chip_dense = c.d_chip_dense; out->d_chip_spread = c.d_chip_spread;
    out->chip_col_stride = c.chip_col_stride;
    out->chip_rows_capacity = many ? c.ctx_chip_rows() : c.chip_col_stride;
    out->chip_context_pitch = c.ctx_chip_rows();         // consecutive rows of the same columns
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_reset(hsw_gadget *g) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    const int rc = hsw_engine_synchronize(g->ctx->engine);
    if (rc != HSW_OK) return rc;
    hsw::Context &c = *g->ctx;
    c.blocks_done = 0;
    c.num_limb_sum = 0;                 // spread.rs:70-71
    c.gate_cursor = 0;
    c.lookup_cursor = c.layout.origin_lookups; // the Context as the caller hands it over (hsw_gadget_set_origin)
    c.zero_loaded = c.layout.origin_zero_loaded;
    c.batches.clear();
    g->cfg.cur_hash_idx = 0;            // lib.rs:66
    g->results.clear();
    g->tie_owners.clear(); g->ties.clear(); g->tie_prefix_bytes = 0;   // the ties are the pass's
    return HSW_OK;
} HSW_NO_UNWIND

// Which allocations the chip columns live in, relative to the gate stream, is worth up to 8 % of an HBM-bound
// batch on MI355X and nothing in user space predicts it: try `candidates` allocations, timing the
// gadget's own batch (every digest an empty message) on each, and keep the fastest.
int hsw_gadget_place(hsw_gadget *g, unsigned candidates, float *ms_each, unsigned *kept) try {
    if (!g || candidates == 0 || candidates > 16) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (c.shared) return HSW_ERR_UNSUPPORTED;                     // (its trial batch would run over the declared interludes)
    if (c.bound) return HSW_ERR_UNSUPPORTED;                      // (the chip columns are the caller's: nothing to place)
    if (g->cfg.cur_hash_idx != 0 || c.blocks_done != 0) return HSW_ERR_INVALID_ARG;      // a fresh or reset gadget
    const size_t n = g->cfg.max_variable_byte_sizes.size();
    if (n == 0) return HSW_ERR_INVALID_ARG;
    hipStream_t stream = nullptr;
    int device = 0;
    hsw_engine_stream(c.engine, reinterpret_cast<void **>(&stream), &device);
    hsw::DeviceScopeG ds(device);
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
    hsw_shape s;
    int rc = hsw_engine_shape(c.engine, &s);
    if (rc != HSW_OK) return rc;
    const size_t col_bytes = (size_t)s.num_advice_columns * (c.chip_col_stride ? c.chip_col_stride : 1) * HSW_CELL_BYTES;
    const uint8_t nothing = 0;
    std::vector<const uint8_t *> in(n, &nothing);
    std::vector<size_t> lens(n, 0), pres(n, 0);
    std::vector<hsw_hash_result> res(n);
    struct Cand { void *dense, *spread; float ms; };
    std::vector<Cand> cands;
    auto restore = [&](size_t keep) {                        // install candidate `keep`, free the others
        for (size_t k = 0; k < cands.size(); k++)
            if (k != keep) { (void)hipFree(cands[k].dense); (void)hipFree(cands[k].spread); }
        c.d_chip_dense = cands[keep].dense;
        c.d_chip_spread = cands[keep].spread;
    };
    for (unsigned k = 0; k < candidates; k++) {
        Cand cd{c.d_chip_dense, c.d_chip_spread, 0.f};
        if (k > 0) {
            cd.dense = cd.spread = nullptr;
            hipError_t he = hipMalloc(&cd.dense, col_bytes);
            if (he == hipSuccess) he = hipMalloc(&cd.spread, col_bytes);
            if (he == hipSuccess) he = hipMemset(cd.dense, 0, col_bytes);
            if (he == hipSuccess) he = hipMemset(cd.spread, 0, col_bytes);
            if (he != hipSuccess) {                               // out of memory: judge the candidates there are
                (void)hipFree(cd.dense); (void)hipFree(cd.spread);
                (void)hipGetLastError();
                break;
            }
        }
        cands.push_back(cd);
        c.d_chip_dense = cd.dense;
        c.d_chip_spread = cd.spread;
        float best = 0.f;
        for (int rep = 0; rep < 3 && rc == HSW_OK; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            rc = hsw_gadget_digest_batch(g, n, in.data(), lens.data(), pres.data(), res.data());
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc == HSW_OK && (rep == 1 || (rep > 1 && ms < best))) best = ms;
            const int rr = hsw_gadget_reset(g);
            if (rc == HSW_OK) rc = rr;
        }
        if (rc != HSW_OK) { restore(0); return rc; }
        cands.back().ms = best;
    }
    size_t keep = 0;
    for (size_t k = 1; k < cands.size(); k++)
        if (cands[k].ms < cands[keep].ms) keep = k;
    for (size_t k = 0; k < cands.size() && ms_each; k++) ms_each[k] = cands[k].ms;
    for (size_t k = cands.size(); k < candidates && ms_each; k++) ms_each[k] = 0.f;
    if (kept) *kept = (unsigned)keep;
    restore(keep);
    hipError_t he = hipMemsetAsync(c.d_chip_dense, 0, col_bytes, stream);       // as a fresh gadget has them
    if (he == hipSuccess) he = hipMemsetAsync(c.d_chip_spread, 0, col_bytes, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    return he == hipSuccess ? HSW_OK : HSW_ERR_HIP;
} HSW_NO_UNWIND

int hsw_gadget_download_region(hsw_gadget *g, const hsw_region_host *dst) try {
    if (!g || !dst) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    hipStream_t stream = nullptr;
    int device = 0;
    hsw_engine_stream(c.engine, reinterpret_cast<void **>(&stream), &device);
    hsw::DeviceScopeG ds(device);
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
    const size_t cb = hsw_cell_bytes(c.repr_flags);
    hipError_t he = hipSuccess;
    auto copy = [&](void *h, const void *d, size_t cell0, size_t cells) {
        if (he == hipSuccess && cells)
            he = hipMemcpyAsync(static_cast<uint8_t *>(h) + cell0 * cb, static_cast<const uint8_t *>(d) + cell0 * cb,
                                cells * cb, hipMemcpyDeviceToHost, stream);
    };
    if (dst->gate && c.by_pointer) {
        // columns by pointer table: the host buffer is an UNBOUND gadget's (K images of columns x max_rows cells back to
        // back); every run of the stream between two jumps lies in one column and is one copy from that column's allocation
        const hsw::Layout &l = c.layout;
        const uint64_t K = l.period ? (c.gate_cursor + l.period - 1) / l.period : 1, R = l.max_rows, P = l.column_pitch();
        for (uint64_t h = 0; h < K; h++) {
            const uint64_t end = !l.period ? c.gate_cursor : c.gate_cursor < (h + 1) * l.period ? c.gate_cursor - h * l.period : l.period;
            uint64_t lo = 0;
            for (size_t k = 0; k <= l.break_cell.size() && lo < end; k++) {
                const uint64_t hi = k < l.break_cell.size() && l.break_cell[k] < end ? l.break_cell[k] : end;
                if (hi > lo && he == hipSuccess) {
                    const uint64_t at = lo + l.origin_row + l.gap_at(lo), col = at / P, row = at % P;   // (the run's first cell)
                    he = hipMemcpyAsync(static_cast<uint8_t *>(dst->gate) + (size_t)((h * l.columns + col) * R + row) * cb,
                                        static_cast<const uint8_t *>(c.d_gate) + (size_t)(c.column_cell(h, col) + row) * cb,
                                        (size_t)(hi - lo) * cb, hipMemcpyDeviceToHost, stream);
                }
                lo = hi > lo ? hi : lo;
            }
        }
    } else if (dst->gate && c.whole && c.layout.max_rows) {
        // the runs of the stream between two jumps up to the cursor, for every assigned Context (one, unless context
        // images: K images back to back, host layout = device layout).  Rows above the origin, the gaps at column ends
        // and the interludes' cells are the caller's or nobody's: never touched
        const hsw::Layout &l = c.layout;
        // (a Context group: the Contexts begun so far, the last one up to the cursor)
        const uint64_t K = c.group_m ? (c.gate_cursor + l.period - 1) / l.period : l.period ? g->cfg.cur_hash_idx : 1;
        for (uint64_t h = 0; h < K; h++) {
            const uint64_t end = !l.period ? c.gate_cursor : c.group_m && c.gate_cursor < (h + 1) * l.period ? c.gate_cursor - h * l.period : l.period;
            uint64_t lo = 0;
            for (size_t k = 0; k <= l.break_cell.size() && lo < end; k++) {
                const uint64_t hi = k < l.break_cell.size() && l.break_cell[k] < end ? l.break_cell[k] : end;
                if (hi > lo) copy(dst->gate, c.d_gate, (size_t)l.image_cell(h * l.period + lo), (size_t)(hi - lo));
                lo = hi > lo ? hi : lo;
            }
        }
    } else if (dst->gate) {
        const size_t cells = c.whole ? (size_t)c.gate_cursor : c.blocks_done * (size_t)c.shape.gate_cells_per_block;
        copy(dst->gate, c.d_gate, 0, cells);
    }
    // (lookup columns by pointer table: the host buffer is an unbound gadget's, Context cx's device cells lookup_extra(cx) further)
    auto copy_lookup = [&](uint64_t cx, uint64_t cell0, uint64_t cells) {
        if (he == hipSuccess && cells)
            he = hipMemcpyAsync(static_cast<uint8_t *>(dst->lookup) + (size_t)cell0 * cb,
                                static_cast<const uint8_t *>(c.d_lookup) + (size_t)(cell0 + c.lookup_extra(cx)) * cb,
                                (size_t)cells * cb, hipMemcpyDeviceToHost, stream);
    };
    if (dst->lookup && c.d_lookup && c.context_images) {
        const uint64_t Lp = c.lookup_pitch();              // Context h: its own entries after the caller's queued cells
        for (uint64_t h = 0; h < g->cfg.cur_hash_idx; h++)
            copy_lookup(h, h * Lp + c.layout.origin_lookups, c.ctx_own_lookups);
    } else if (dst->lookup && c.d_lookup && c.shared && !c.layout.digest_lookup0.empty()) {
        const size_t M = c.group_m ? c.group_m : c.layout.digest_entry0.size();
        const uint64_t own = c.group_m ? c.ctx_own_lookups : c.own_lookup_capacity, Lp = c.group_m ? c.lookup_pitch() : 0;
        for (size_t d = 0; d < g->cfg.cur_hash_idx; d++) {     // every digest's own entries; the interludes' are the caller's
            const size_t h = d % M, cx = d / M;                 // (a Context group: digest h of Context cx, in its own lookup column)
            const uint64_t end = h + 1 < c.layout.digest_entry0.size() ? c.layout.digest_entry0[h + 1] : own;
            copy_lookup(cx, cx * Lp + c.layout.digest_lookup0[h], end - c.layout.digest_entry0[h]);
        }
    } else if (dst->lookup && c.d_lookup) {
        copy(dst->lookup, c.d_lookup, (size_t)c.layout.origin_lookups, (size_t)(c.lookup_cursor - c.layout.origin_lookups));
    }
    const uint32_t ncols = c.shape.num_advice_columns;
    // the used rows of every chip column -- of every Context begun, where each has chip rows of its own (a bound region)
    // (chip columns by pointer table: the host buffers are an unbound gadget's -- ncols columns of all Contexts' rows,
    //  Context cx's after Context cx-1's -- and every column of every Context is one copy from its own allocation)
    const uint64_t per = c.chip_rows_per_context() ? c.ctx_limb_calls() : c.num_limb_sum ? c.num_limb_sum : 1;
    const size_t host_stride = c.chips_by_table() ? (size_t)hsw_chip_rows(&c.shape, 0, c.capacity_blocks) : c.chip_col_stride;
    auto copy_chip = [&](void *h, const void *d, size_t hcell, size_t dcell, size_t cells) {
        if (h && he == hipSuccess && cells)
            he = hipMemcpyAsync(static_cast<uint8_t *>(h) + hcell * cb, static_cast<const uint8_t *>(d) + dcell * cb, cells * cb,
                                hipMemcpyDeviceToHost, stream);
    };
    for (uint64_t n0 = 0; n0 < c.num_limb_sum; n0 += per) {
        const uint64_t n1 = n0 + per < c.num_limb_sum ? n0 + per : c.num_limb_sum, cx = n0 / per;
        const size_t rows = (size_t)((n1 - n0 + ncols - 1) / ncols);
        for (uint32_t k = 0; k < ncols; k++) {
            const size_t hcell = c.chips_by_table() ? k * host_stride + (size_t)(n0 / ncols) : (size_t)c.chip_column_cell(cx, k, false);
            copy_chip(dst->chip_dense, c.d_chip_dense, hcell, (size_t)c.chip_column_cell(cx, k, false), rows);
            copy_chip(dst->chip_spread, c.d_chip_spread, hcell, (size_t)c.chip_column_cell(cx, k, true), rows);
        }
    }
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    return he == hipSuccess ? HSW_OK : HSW_ERR_HIP;
} HSW_NO_UNWIND

int hsw_gadget_download_region_compact(hsw_gadget *g, hsw_region_compact *dst) try {
    if (!g || !dst) return HSW_ERR_INVALID_ARG;
    hsw::Context &c = *g->ctx;
    if (c.repr_flags != HSW_REPR_CANONICAL) return HSW_ERR_UNSUPPORTED;      // packs canonical 32-byte cells
    if (c.context_images) return HSW_ERR_UNSUPPORTED;                         // one image per Context: not packed here
    if ((c.shared && c.layout.max_rows) || c.group_m) return HSW_ERR_UNSUPPORTED;    // shared context: interludes are the caller's
    if (c.bound) return HSW_ERR_UNSUPPORTED;                                  // a bound region: the cells between columns are the caller's
    if (!dst->wide && dst->wide_cap) return HSW_ERR_INVALID_ARG;
    hipStream_t stream = nullptr;
    int device = 0;
    hsw_engine_stream(c.engine, reinterpret_cast<void **>(&stream), &device);
    hsw::DeviceScopeG ds(device);
    if (!ds.ok) return HSW_ERR_NO_DEVICE;
    const uint32_t ncols = c.shape.num_advice_columns;
    const size_t chip_cells = (size_t)ncols * (c.chip_col_stride ? c.chip_col_stride : 1);
    const size_t gate_cells = c.whole ? (c.layout.max_rows ? (size_t)(c.layout.max_rows * (c.layout.break_cell.size() + 1)) : (size_t)c.gate_capacity)
                                      : c.capacity_blocks * (size_t)c.shape.gate_cells_per_block;
    hipError_t he = hipSuccess;
    if (!c.d_wide) {        // first use (or the geometry changed: set_columns / set_origin drop the staging):
                            // the 8-byte staging of every stream, the side list and its counter
        // wide cells: 4 ch negations per round (256 per block) + a few dozen per digest frame
        c.wide_cap = c.capacity_blocks * 256 + 128 * (c.init_capacity + 1) + 4 * c.capacity_blocks + 64;
        he = hipMalloc(&c.d_c_gate, (gate_cells ? gate_cells : 1) * 8);
        if (he == hipSuccess && c.d_lookup) he = hipMalloc(&c.d_c_lookup, (size_t)(c.lookup_capacity ? c.lookup_capacity : 1) * 8);
        if (he == hipSuccess) he = hipMalloc(&c.d_c_dense, chip_cells * 8);
        if (he == hipSuccess) he = hipMalloc(&c.d_c_spread, chip_cells * 8);
        if (he == hipSuccess) he = hipMalloc((void **)&c.d_wide_count, sizeof(uint32_t));
        if (he == hipSuccess) he = hipHostMalloc((void **)&c.hp_wide_count, sizeof(uint32_t), hipHostMallocDefault);
        if (he == hipSuccess) he = hipMalloc(&c.d_wide, c.wide_cap * 48);
        if (he != hipSuccess) { c.free_compact_staging(); return hsw::hip_status(he); }
    }
    he = hipMemsetAsync(c.d_wide_count, 0, sizeof(uint32_t), stream);
    auto pack = [&](uint64_t *h, void *d8, const void *d32, uint64_t sid, size_t cell0, size_t cells) {
        if (he != hipSuccess || !cells || !h) return;
        he = hsw::launch_pack64(static_cast<const uint8_t *>(d32) + cell0 * 32, static_cast<uint8_t *>(d8) + cell0 * 8, cells, sid,
                                cell0, c.d_wide, (uint32_t)c.wide_cap, c.d_wide_count, stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(h + cell0, static_cast<uint8_t *>(d8) + cell0 * 8, cells * 8, hipMemcpyDeviceToHost, stream);
    };
    if (c.whole && c.layout.max_rows) {
        // ONE pass over the image from (column 0, row 0) to the last assigned cell: the few unassigned rows at
        // the end of every column are zero on the device and travel as zeros (a launch and a copy per column
        // would cost more than the bytes they save)
        uint64_t last_col = 0, last_row = 0;
        if (c.gate_cursor) { c.layout.position(c.gate_cursor - 1, &last_col, &last_row); last_row += 1; last_col -= c.layout.origin_column; }
        // (from the origin row on: the rows above it in image column 0 are the caller's cells)
        pack(dst->gate, c.d_c_gate, c.d_gate, HSW_STREAM_GATE, (size_t)c.layout.origin_row,
             c.gate_cursor ? (size_t)(last_col * c.layout.max_rows + last_row - c.layout.origin_row) : 0);
    } else {
        pack(dst->gate, c.d_c_gate, c.d_gate, HSW_STREAM_GATE, 0,
             c.whole ? (size_t)c.gate_cursor : c.blocks_done * (size_t)c.shape.gate_cells_per_block);
    }
    if (c.d_lookup)
        pack(dst->lookup, c.d_c_lookup, c.d_lookup, HSW_STREAM_LOOKUP, (size_t)c.layout.origin_lookups, (size_t)(c.lookup_cursor - c.layout.origin_lookups));
    const size_t rows = (size_t)((c.num_limb_sum + ncols - 1) / ncols);
    if (rows == c.chip_col_stride) {         // every column full: one pass per family
        pack(dst->chip_dense, c.d_c_dense, c.d_chip_dense, HSW_STREAM_CHIP_DENSE, 0, rows * ncols);
        pack(dst->chip_spread, c.d_c_spread, c.d_chip_spread, HSW_STREAM_CHIP_SPREAD, 0, rows * ncols);
    } else {
        for (uint32_t k = 0; k < ncols; k++) {
            pack(dst->chip_dense, c.d_c_dense, c.d_chip_dense, HSW_STREAM_CHIP_DENSE, k * c.chip_col_stride, rows);
            pack(dst->chip_spread, c.d_c_spread, c.d_chip_spread, HSW_STREAM_CHIP_SPREAD, k * c.chip_col_stride, rows);
        }
    }
    // the side list: the counter and as many entries as the caller has room for, in one pass of copies
    const size_t take = dst->wide_cap < c.wide_cap ? dst->wide_cap : c.wide_cap;
    if (he == hipSuccess) he = hipMemcpyAsync(c.hp_wide_count, c.d_wide_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess && take) he = hipMemcpyAsync(dst->wide, c.d_wide, take * 48, hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return HSW_ERR_HIP;
    dst->n_wide = *c.hp_wide_count;
    if (dst->n_wide > take) return HSW_ERR_TOO_LARGE;         // n_wide says how many entries the region has
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_region_widen(const uint64_t *compact, size_t n_cells, uint64_t stream_id, const hsw_wide_cell *wide, size_t n_wide,
                     void *cells32) try {
    if ((!compact || !cells32) && n_cells) return HSW_ERR_INVALID_ARG;
    if (!wide && n_wide) return HSW_ERR_INVALID_ARG;
    uint64_t *out = static_cast<uint64_t *>(cells32);
    for (size_t i = 0; i < n_cells; i++) { out[4 * i] = compact[i]; out[4 * i + 1] = 0; out[4 * i + 2] = 0; out[4 * i + 3] = 0; }
    for (size_t k = 0; k < n_wide; k++) {
        if (wide[k].stream != stream_id) continue;
        if (wide[k].index >= n_cells) return HSW_ERR_INVALID_ARG;
        std::memcpy(out + 4 * wide[k].index, wide[k].value, 32);
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_seek(hsw_gadget *g, size_t hash_idx) try {
    if (!g || hash_idx > g->cfg.max_variable_byte_sizes.size()) return HSW_ERR_INVALID_ARG;
    if (g->ctx->context_images) return HSW_ERR_UNSUPPORTED;       // K proofs of one circuit: nothing to deal out
    if (g->ctx->shared) return HSW_ERR_UNSUPPORTED;               // shared context: the layout follows the declared origins
    if (g->ctx->bound) return HSW_ERR_UNSUPPORTED;                // a bound region is one prover's own slabs
    int rc = hsw_engine_synchronize(g->ctx->engine);
    if (rc != HSW_OK) return rc;
    hsw::Context &c = *g->ctx;
    size_t blocks = 0;
    uint64_t gate = 0, lookup = c.layout.origin_lookups;
    for (size_t h = 0; h < hash_idx; h++) {
        const size_t b = g->cfg.max_variable_byte_sizes[h];
        blocks += b / 64;
        if (c.whole) {
            hsw_frame_shape fs;
            rc = hsw_frame_query(&c.shape, b, g->cfg.is_input_range_check ? 1 : 0, &fs);
            if (rc != HSW_OK) return rc;
            gate += fs.digest_cells + (c.independent || (h == 0 && !c.layout.origin_zero_loaded) ? 1 : 0);   // + the Context's zero cell, loaded by digest #0
            lookup += fs.digest_lookups;
        }
    }
    c.blocks_done = blocks;
    c.num_limb_sum = (uint64_t)blocks * c.shape.limb_calls_per_block;       // spread.rs:228-231
    c.gate_cursor = gate;
    c.lookup_cursor = lookup;
    c.zero_loaded = c.layout.origin_zero_loaded || hash_idx > 0;
    g->cfg.cur_hash_idx = hash_idx;
    c.batches.clear();
    g->results.clear();
    g->tie_owners.clear(); g->ties.clear(); g->tie_prefix_bytes = 0;   // (digests assigned elsewhere: nothing to tie to)
    g->results.resize(hash_idx);        // keeps hash_idx -> result indexing of hsw_gadget_input_bytes
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_verify(hsw_gadget *g, hsw_verify_report *report) try {
    if (!g || !report) return HSW_ERR_INVALID_ARG;
    std::memset(report, 0, sizeof *report);
    hsw::Context &c = *g->ctx;
    if (c.repr_flags & HSW_REPR_COMPACT64) return HSW_ERR_UNSUPPORTED;         // 32-byte cells only
    // shared context: every launch checks through the jump table (the layout of the digests so far is final)
    if (c.table_path()) {
        const int rc0 = c.upload_place();
        if (rc0 != HSW_OK) return rc0;
    }
    // block0: a block launch reports blocks counted from its own first one (the frames report the pass's), the
    // gadget's report names blocks of the pass
    auto merge = [&](const hsw_verify_report &r, uint64_t block0) {
        if (r.violations && !report->violations) {
            report->first_block = r.first_block + block0; report->first_cell = r.first_cell; report->first_class = r.first_class;
        }
        report->violations += r.violations; report->checks += r.checks; report->kernel_ms += r.kernel_ms;
    };
    for (const hsw::Context::BatchRecord &b : c.batches) {
        hsw::Launch L(c, b.inputs_in_pinned, b.repr_flags);
        hsw_verify_report r;
        if (!c.whole) {
            L.blocks(b.first_block, b.n_blocks);
            const int rc = hsw_verify_blocks(c.engine, &L.a, &r);
            if (rc != HSW_OK) return rc;
            merge(r, b.first_block);
            continue;
        }
        // the launches of the batch as it was generated: runs of equally sized digests, or a group's digest indices
        for (const hsw::Run &run : hsw::batch_runs(c, b.first_digest, b.n_digests, [&](size_t k) { return g->results[b.first_digest + k].n_blocks; })) {
            const hsw::AssignedHashResult &r0 = g->results[b.first_digest + run.first];
            hsw_frame_shape fs;
            int rc = hsw_frame_query(&c.shape, r0.n_blocks * 64, g->cfg.is_input_range_check ? 1 : 0, &fs);
            if (rc != HSW_OK) return rc;
            L.run(b.first_digest + run.first, r0, r0.first_block, run.count, fs);
            rc = hsw_verify_blocks_impl(c.engine, &L.a, &r, L.per);
            if (rc != HSW_OK) return rc;
            merge(r, r0.first_block);
            std::vector<hsw_frame_desc> descs(run.count);
            for (size_t k = 0; k < run.count; k++) {
                const hsw::AssignedHashResult &rk = g->results[b.first_digest + run.first + k * run.step];
                hsw_frame_desc &d = descs[k];
                d.input_len = rk.input_len; d.first_block = rk.first_block; d.n_blocks = (uint32_t)rk.n_blocks;
                d.num_round = (uint32_t)rk.num_round; d.precomputed_round = (uint32_t)(rk.num_round - rk.target_round);
                d.is_input_range_check = g->cfg.is_input_range_check ? 1u : 0u;
                d.prologue_cell = rk.prologue_cell; d.epilogue_cell = rk.epilogue_cell;
                const size_t dk = b.first_digest + run.first + k * run.step;
                const uint64_t lx = c.lookup_extra(c.context_images ? dk : c.group_m ? dk / c.group_m : 0);
                d.prologue_lookup = rk.prologue_lookup + lx; d.epilogue_lookup = rk.epilogue_lookup + lx;
                d.zero_cell = rk.block_cell == rk.prologue_cell + fs.prologue_cells + 1 ? rk.block_cell - 1 : ~0ull;
            }
            rc = hsw_verify_frames_impl(c.engine, descs.data(), descs.size(), L.in_blocks, L.in_pre, c.d_next_states, c.gate_stream(),
                                        c.d_lookup, L.frame_pack, b.repr_flags, &r, L.per);
            if (rc != HSW_OK) return rc;
            merge(r, 0);
        }
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_context_region(const hsw_gadget *g, size_t h, hsw_context_region *out) try {
    if (!g || !out) return HSW_ERR_INVALID_ARG;
    const hsw::Context &c = *g->ctx;
    if (!(c.context_images || c.group_m) || h >= c.contexts()) return HSW_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    const size_t cb = HSW_CELL_BYTES;                       // whole-digest contexts: 32-byte cells
    const uint32_t ncols = c.shape.num_advice_columns;
    // (a Context group: Context h holds group_m digests, ctx_blocks blocks)
    const uint64_t nb = c.group_m ? c.ctx_blocks : g->cfg.max_variable_byte_sizes[h] / 64, C = c.ctx_stream();
    out->stream_cells = C;
    out->first_stream_cell = h * C;
    out->columns = c.layout.columns;
    out->max_rows = c.layout.max_rows;
    if (c.layout.max_rows) {
        uint64_t col = 0, row = 0;
        c.layout.position(C - 1, &col, &row);
        out->last_column_rows = row + 1;
        out->d_image = static_cast<uint8_t *>(c.d_gate) + (size_t)c.column_cell(h, 0) * cb;   // (by pointer table: proof h's column 0)
    } else {
        out->d_image = static_cast<uint8_t *>(c.d_gate) + (size_t)(h * C) * cb;   // linear: the Context's stream
    }
    out->lookup_cells = c.ctx_lookups();
    out->d_lookup = static_cast<uint8_t *>(c.d_lookup) + (size_t)c.lookup_cell(h) * cb;   // (by pointer table: proof h's own column)
    out->chip_rows = nb * c.shape.limb_calls_per_block / ncols;
    out->chip_col_stride = c.chip_col_stride;
    // (a whole number of rows per Context; by pointer table: proof h's chip column 0 of each family)
    out->d_chip_dense = static_cast<uint8_t *>(c.d_chip_dense) + (size_t)c.chip_column_cell(h, 0, false) * cb;
    out->d_chip_spread = static_cast<uint8_t *>(c.d_chip_spread) + (size_t)c.chip_column_cell(h, 0, true) * cb;
    out->origin_column = c.layout.origin_column;
    out->origin_row = c.layout.origin_row;
    out->origin_lookups = c.layout.origin_lookups;
    out->assigned = (h + 1) * (c.group_m ? c.group_m : 1) <= g->cfg.cur_hash_idx ? 1u : 0u;   // every digest of the Context
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_cell_position(const hsw_gadget *g, uint64_t cell, uint64_t *column, uint64_t *row) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    g->ctx->layout.position(cell, column, row);
    return HSW_OK;
} HSW_NO_UNWIND

// ---- digest-to-digest copy constraints (include/hsw.h, "ties")

// gate-stream cells of one recorded tie: the child's output-byte cell (hsw_gadget_result_cells), the parent's input-byte cell
static void tie_cells(const hsw_gadget *g, const hsw_gadget::Tie &t, uint64_t *src_cell, uint64_t *dst_cell) {
    const hsw::AssignedHashResult &s = g->results[(size_t)t.src_hash], &d = g->results[(size_t)t.dst_hash];
    *src_cell = s.epilogue_cell + (uint64_t)hsw::frame::E_STATE * (s.n_blocks + 1) + (uint64_t)hsw::frame::E_WORD * (t.src_byte / 4) +
                5u * (t.src_byte % 4);
    *dst_cell = d.prologue_cell + hsw::frame::P_BYTES + t.dst_byte;
}

// a gate-stream cell some digest of this pass has been assigned (the pass order is the stream order)
static bool cell_assigned(const hsw_gadget *g, uint64_t cell) {
    const hsw::Context &c = *g->ctx;
    if (!c.whole || c.batches.empty() || c.batches[0].first_digest >= g->results.size()) return false;
    return cell >= g->results[c.batches[0].first_digest].prologue_cell && cell < c.gate_cursor;
}

static uint64_t cell_device_address(const hsw::Context &c, uint64_t cell) {
    return (uint64_t)reinterpret_cast<uintptr_t>(c.d_gate) + c.cell_offset(cell) * HSW_CELL_BYTES;   // (pointer tables: modulo 2^64)
}

int hsw_gadget_ties(const hsw_gadget *g, hsw_cell_tie *out, size_t cap, size_t *n, uint64_t *prefix_bytes_untied) try {
    if (!g) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;                  // block-stream contexts have no byte cells
    if (n) *n = g->ties.size();
    if (prefix_bytes_untied) *prefix_bytes_untied = g->tie_prefix_bytes;
    if (!out) return HSW_OK;
    if (cap < g->ties.size()) return HSW_ERR_TOO_LARGE;
    for (size_t i = 0; i < g->ties.size(); i++) {
        const hsw_gadget::Tie &t = g->ties[i];
        hsw_cell_tie &o = out[i];
        o.src_hash = t.src_hash; o.dst_hash = t.dst_hash; o.src_byte = t.src_byte; o.dst_byte = t.dst_byte;
        tie_cells(g, t, &o.src_cell, &o.dst_cell);
    }
    return HSW_OK;
} HSW_NO_UNWIND

int hsw_gadget_cell_address(const hsw_gadget *g, uint64_t cell, void **d_cell) try {
    if (!g || !d_cell) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;
    if (!cell_assigned(g, cell)) return HSW_ERR_INVALID_ARG;
    *d_cell = reinterpret_cast<void *>((uintptr_t)cell_device_address(*g->ctx, cell));
    return HSW_OK;
} HSW_NO_UNWIND

// n pairs (cells[2 i], cells[2 i + 1]): every cell validated and resolved before anything is launched
static int verify_pairs(hsw_gadget *g, size_t n, const std::vector<uint64_t> &cells, hsw_tie_report *report) {
    hsw::Context &c = *g->ctx;
    std::memset(report, 0, sizeof *report);
    if (n == 0) return HSW_OK;
    std::vector<uint64_t> addr(2 * n);
    for (size_t i = 0; i < 2 * n; i++) {
        const uint64_t cell = cells[i];
        if (!cell_assigned(g, cell)) return hsw_engine_fail(c.engine, HSW_ERR_INVALID_ARG, "a cell out of range or not assigned in this pass");
        addr[i] = cell_device_address(c, cell);
    }
    if (n > g->pairs_cap) {                                  // (every earlier check has been waited for: nothing reads the old one)
        int device = 0;
        hsw_engine_stream(c.engine, nullptr, &device);
        hsw::DeviceScopeG ds(device);
        if (!ds.ok) return HSW_ERR_NO_DEVICE;
        void *p = nullptr;
        const size_t cap = n > 2 * g->pairs_cap ? n : 2 * g->pairs_cap;
        const hipError_t he = hipMalloc(&p, cap * 16);
        if (he != hipSuccess) return hsw::hip_status(he);
        (void)hipFree(g->d_pairs);
        g->d_pairs = p; g->pairs_cap = cap;
    }
    return hsw_verify_pairs_impl(c.engine, addr.data(), g->d_pairs, n, report);
}

int hsw_gadget_verify_ties(hsw_gadget *g, hsw_tie_report *report) try {
    if (!g || !report) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;
    std::vector<uint64_t> cells(2 * g->ties.size());
    for (size_t i = 0; i < g->ties.size(); i++) tie_cells(g, g->ties[i], &cells[2 * i], &cells[2 * i + 1]);
    return verify_pairs(g, g->ties.size(), cells, report);
} HSW_NO_UNWIND

int hsw_gadget_verify_equal(hsw_gadget *g, const uint64_t *cells_a, const uint64_t *cells_b, size_t n, hsw_tie_report *report) try {
    if (!g || !report || ((!cells_a || !cells_b) && n)) return HSW_ERR_INVALID_ARG;
    if (!g->ctx->whole) return HSW_ERR_UNSUPPORTED;
    std::vector<uint64_t> cells(2 * n);
    for (size_t i = 0; i < n; i++) { cells[2 * i] = cells_a[i]; cells[2 * i + 1] = cells_b[i]; }
    return verify_pairs(g, n, cells, report);
} HSW_NO_UNWIND

int hsw_gadget_set_repr(hsw_gadget *g, uint32_t repr) try {
    if (!g || (repr & ~HSW_REPR_MASK) || repr == HSW_REPR_MASK) return HSW_ERR_INVALID_ARG;
    if (g->ctx->whole && (repr & HSW_REPR_COMPACT64)) return HSW_ERR_UNSUPPORTED;   // frames hold full-width cells
    if (g->ctx->blocks_done != 0 && hsw_cell_bytes(repr) != hsw_cell_bytes(g->ctx->repr_flags))
        return HSW_ERR_INVALID_ARG;               // the cell size of a context's streams cannot change midway
    g->ctx->repr_flags = repr;
    return HSW_OK;
} HSW_NO_UNWIND

}  // extern "C"
