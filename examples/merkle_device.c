/* Plain C99: an 8-leaf Merkle tree hashed in circuit with ONE call (hsw_gadget_digest_levels_device) on a
 * whole-digest gadget with a column image.  The leaves already live in device memory (here: slices of a buffer the
 * device filled itself; the host only looks at a copy to check the result); the 15 digests go to a `nodes` array in
 * device memory -- leaves' digests first, then each level after the one below it -- and every inner message is the
 * 64 bytes of its two children where they lie.  No digest crosses to the host between the levels.  The root is
 * compared against a host SHA-256 the example carries itself.  Build like examples/digest_abc.c. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

#define LEAVES 8
#define NODES (2 * LEAVES - 1)
#define ARENA 1024u                 /* bytes the leaves are cut from */

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

/* ---- SHA-256 on the host (FIPS 180-4), for the comparison only ---- */
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void sha256(const uint8_t *msg, size_t len, uint8_t out[32]) {
    static const uint32_t k[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    const size_t rounds = (len + 9 + 63) / 64;
    for (size_t r = 0; r < rounds; r++) {
        uint8_t b[64];
        for (size_t i = 0; i < 64; i++) {
            const size_t p = 64 * r + i;
            b[i] = p < len ? msg[p] : p == len ? 0x80 : 0;
        }
        if (r + 1 == rounds)
            for (int i = 0; i < 8; i++) b[56 + i] = (uint8_t)(((uint64_t)len * 8) >> (56 - 8 * i));
        uint32_t w[64], s[8];
        for (int i = 0; i < 16; i++)
            w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
        for (int i = 16; i < 64; i++)
            w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
                   (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        memcpy(s, h, sizeof s);
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + k[i] + w[i];
            const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
            s[7] = s[6]; s[6] = s[5]; s[5] = s[4]; s[4] = s[3] + t1; s[3] = s[2]; s[2] = s[1]; s[1] = s[0]; s[0] = t1 + t2;
        }
        for (int i = 0; i < 8; i++) h[i] += s[i];
    }
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[NODES];
    for (int h = 0; h < NODES; h++) sizes[h] = 128;                    /* a leaf of up to 119 bytes, or two digests */
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_ex(eng, sizes, NODES, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, (1u << 17) - 9, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);

    /* device memory of the caller's: [ leaf bytes | nodes ].  The leaf bytes are produced on the device (a fill
       pattern here -- a previous kernel's output in a prover) and complete before the call below. */
    void *mem = NULL;
    if ((rc = hsw_device_alloc(0, ARENA + 32 * NODES, 0, &mem)) != HSW_OK) die("hsw_device_alloc", rc, eng);
    float ms = 0.f;
    if ((rc = hsw_fill_calibrate(eng, mem, ARENA, &ms)) != HSW_OK) die("hsw_fill_calibrate", rc, eng);
    uint8_t *d_leaves = (uint8_t *)mem, *d_nodes = d_leaves + ARENA;

    /* leaf i: lens[i] bytes at a byte offset of its own; then the inner messages, read in place from d_nodes */
    static const size_t leaf_len[LEAVES] = {0, 1, 55, 56, 63, 64, 100, 119};
    const void *inputs[NODES];
    void *outputs[NODES];
    size_t lens[NODES], leaf_at[LEAVES];
    uint32_t levels[NODES];
    for (int i = 0; i < LEAVES; i++) {
        leaf_at[i] = 120 * (size_t)i + (size_t)(2 * i + 1);            /* misaligned, each differently */
        inputs[i] = d_leaves + leaf_at[i]; lens[i] = leaf_len[i]; levels[i] = 0;
    }
    int n = LEAVES, below = 0, width = LEAVES;
    for (uint32_t level = 1; width > 1; level++, below += width, width /= 2)
        for (int j = 0; j < width / 2; j++, n++) {
            inputs[n] = d_nodes + 32 * (below + 2 * j); lens[n] = 64; levels[n] = level;
        }
    for (int k = 0; k < NODES; k++) outputs[k] = d_nodes + 32 * k;

    hsw_hash_result r[NODES];
    if ((rc = hsw_gadget_digest_levels_device(g, NODES, inputs, lens, NULL, levels, outputs, r)) != HSW_OK)
        die("hsw_gadget_digest_levels_device", rc, eng);

    /* the check: the same tree on the host, from a copy of the leaf bytes */
    uint8_t h_leaves[ARENA], want[NODES][32], got[NODES][32], pair[64];
    if ((rc = hsw_download(eng, h_leaves, d_leaves, ARENA)) != HSW_OK) die("hsw_download", rc, eng);
    if ((rc = hsw_download(eng, got, d_nodes, sizeof got)) != HSW_OK) die("hsw_download", rc, eng);
    for (int i = 0; i < LEAVES; i++) sha256(h_leaves + leaf_at[i], leaf_len[i], want[i]);
    n = LEAVES; below = 0; width = LEAVES;
    for (; width > 1; below += width, width /= 2)
        for (int j = 0; j < width / 2; j++, n++) {
            memcpy(pair, want[below + 2 * j], 32);
            memcpy(pair + 32, want[below + 2 * j + 1], 32);
            sha256(pair, 64, want[n]);
        }
    for (int k = 0; k < NODES; k++)
        if (memcmp(got[k], want[k], 32) != 0 || memcmp(r[k].output_bytes, want[k], 32) != 0) {
            fprintf(stderr, "node %d differs from the host's SHA-256\n", k);
            return 1;
        }
    char hex[65];
    for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", (unsigned)got[NODES - 1][k]);
    printf("%d leaves, %d digests in %llu advice columns, root %s\n", LEAVES, NODES, (unsigned long long)columns, hex);

    hsw_verify_report rep;
    if ((rc = hsw_gadget_verify(g, &rep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)rep.checks,
           (unsigned long long)rep.violations);
    if (rep.violations != 0) return 1;
    hsw_gadget_destroy(g);
    if ((rc = hsw_device_free(mem)) != HSW_OK) die("hsw_device_free", rc, eng);
    hsw_engine_destroy(eng);
    puts("merkle device ok");
    return 0;
}
