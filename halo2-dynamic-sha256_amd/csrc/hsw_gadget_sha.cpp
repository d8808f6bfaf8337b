// hsw_gadget_sha.cpp -- the host half of lib.rs:77-160: padding, the plain SHA-256 of the precomputed prefix (and of
// a host-chained batch), the round counts.  No HIP call (see hsw_gadget.hpp).
#include "hsw_gadget.hpp"

#include <cstdlib>
#include <cstring>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif

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
#endif

}  // namespace

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
void plain_compress(uint32_t st[8], const uint8_t *block) {
    if (have_shani()) plain_compress_shani(st, block);
    else plain_compress_scalar(st, block);
}
bool host_sha_is_fast() { return have_shani(); }
#else
void plain_compress(uint32_t st[8], const uint8_t *block) { plain_compress_scalar(st, block); }
bool host_sha_is_fast() { return false; }
#endif

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
    // the common case, no prefix: pad straight into the bytes fed to the circuit (lib.rs:98-117,170)
    std::vector<uint8_t> with_prefix(precomputed_input_len ? total : 0, 0);
    if (!precomputed_input_len) plan->blocks.assign(max_variable_byte_size, 0);
    uint8_t *padded = precomputed_input_len ? with_prefix.data() : plan->blocks.data();
    if (input_byte_size) std::memcpy(padded, input, input_byte_size);
    size_t n = input_byte_size;
    padded[n++] = 0x80;                                                       // lib.rs:99
    n += zero_padding_byte_size;                                              // lib.rs:100-102
    const uint64_t bitlen = 8ull * (uint64_t)input_byte_size;                 // lib.rs:103-108 (big-endian)
    for (int i = 7; i >= 0; i--) padded[n++] = (uint8_t)(bitlen >> (8 * i));
    if (n != num_round * one_round_size) return HSW_ERR_INVALID_ARG;          // lib.rs:110
    if (n + remaining_byte_size != total) return HSW_ERR_INVALID_ARG;         // lib.rs:111-117
    if (precomputed_input_len) {
        for (size_t r = 0; r < precomputed_round; r++)                        // lib.rs:156-160
            plain_compress(plan->init_state, padded + r * one_round_size);
        plan->blocks.assign(with_prefix.begin() + (ptrdiff_t)precomputed_input_len, with_prefix.end());   // lib.rs:170
    }
    plan->num_round = num_round;
    plan->precomputed_round = precomputed_round;
    plan->target_round = lengths.target_round;
    plan->max_variable_round = lengths.max_variable_round;
    return HSW_OK;
}

}  // namespace hsw
