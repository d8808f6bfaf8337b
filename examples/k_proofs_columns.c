/* Plain C99: K = 8 proofs of the reference's BENCH circuit (benches/digest.rs:93-129 -- one digest of at most
 * 1024 bytes per proof, input range checks, k = 17, 9 advice columns) synthesized by ONE launch, every proof a
 * FlexGate column image of its own (HSW_GADGET_CONTEXT_IMAGES).  Pass 1 starts every proof at Context origin
 * (0, 0); pass 2, after a reset, at (column 2, row 131000), as a circuit that has used its chips first would.
 * Each proof's digest is read back from its own image through hsw_gadget_context_region.  Build like
 * examples/digest_abc.c. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

#define K 8

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[K];
    for (int h = 0; h < K; h++) sizes[h] = 1024;                                     /* MAX_BYTE_SIZE1 */
    hsw_gadget *g = NULL;
    rc = hsw_gadget_create_ex(eng, sizes, K, 1,
                              HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g);
    if (rc != HSW_OK) die("hsw_gadget_create_ex", rc, eng);
    const uint64_t max_rows = (1u << 17) - 9;                                        /* usable rows at k = 17 */
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, max_rows, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);

    /* proof h proves message h: 56 bytes of value h + 1 (proof 0 is the bench's own message) */
    uint8_t msg[K][56];
    const uint8_t *inputs[K];
    size_t lens[K], pre[K];
    for (int h = 0; h < K; h++) {
        memset(msg[h], h + 1, sizeof msg[h]);
        inputs[h] = msg[h]; lens[h] = sizeof msg[h]; pre[h] = 0;
    }
    const uint64_t origin[2][2] = {{0, 0}, {2, 131000}};
    for (int pass = 0; pass < 2; pass++) {
        if ((rc = hsw_gadget_reset(g)) != HSW_OK) die("hsw_gadget_reset", rc, eng);
        if ((rc = hsw_gadget_set_origin(g, origin[pass][0], origin[pass][1], 0, 0)) != HSW_OK) die("hsw_gadget_set_origin", rc, eng);
        hsw_hash_result r[K];
        if ((rc = hsw_gadget_digest_batch(g, K, inputs, lens, pre, r)) != HSW_OK) die("hsw_gadget_digest_batch", rc, eng);
        printf("pass %d: origin (column %llu, row %llu)\n", pass + 1, (unsigned long long)origin[pass][0],
               (unsigned long long)origin[pass][1]);
        for (int h = 0; h < K; h++) {
            hsw_context_region reg;
            if ((rc = hsw_gadget_context_region(g, (size_t)h, &reg)) != HSW_OK) die("hsw_gadget_context_region", rc, eng);
            /* AssignedHashResult.output_bytes: the 32 load_witness cells of the epilogue (lib.rs:317-324), read from
               proof h's own image at the (FlexGate column, row) the gadget reports */
            char hex[65];
            for (int b = 0; b < 32; b++) {
                const uint64_t cell = r[h].epilogue_cell + 76 * (r[h].n_blocks + 1) + 36 * (uint64_t)(b / 4) + 5 * (uint64_t)(b % 4);
                uint64_t col, row, val[4];
                hsw_gadget_cell_position(g, cell, &col, &row);
                const uint8_t *at = (const uint8_t *)reg.d_image + ((col - reg.origin_column) * reg.max_rows + row) * HSW_CELL_BYTES;
                if ((rc = hsw_download(eng, val, at, sizeof val)) != HSW_OK) die("hsw_download", rc, eng);
                if (val[0] != r[h].output_bytes[b] || val[1] || val[2] || val[3]) return 1;
                sprintf(hex + 2 * b, "%02x", (unsigned)val[0]);
            }
            printf("proof %d: %llu x %llu, digest %s\n", h, (unsigned long long)reg.columns, (unsigned long long)reg.max_rows, hex);
        }
        hsw_verify_report rep;
        if ((rc = hsw_gadget_verify(g, &rep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
        printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)rep.checks,
               (unsigned long long)rep.violations);
        if (rep.violations != 0) return 1;
    }
    /* what one single-proof gadget lays out at the second origin: every proof above has that many columns */
    hsw_gadget *one = NULL;
    uint64_t one_columns = 0;
    if ((rc = hsw_gadget_create_ex(eng, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &one)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);
    if ((rc = hsw_gadget_set_origin(one, origin[1][0], origin[1][1], 0, 0)) != HSW_OK) die("hsw_gadget_set_origin", rc, eng);
    if ((rc = hsw_gadget_set_columns(one, max_rows, &one_columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);
    printf("single-proof gadget at (2, 131000): %llu columns\n", (unsigned long long)one_columns);
    hsw_gadget_destroy(one);
    hsw_gadget_destroy(g);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
