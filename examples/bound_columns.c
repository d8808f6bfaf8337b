/* Plain C99: K = 8 proofs of the reference's BENCH circuit (benches/digest.rs:93-129 -- one digest of at most
 * 1024 bytes per proof, input range checks, k = 17) written STRAIGHT into a prover's own device memory
 * (hsw_gadget_bind_region): one slab per proof of 14 advice polynomials of n = 2^17 cells --
 * [9 FlexGate | 1 lookup | 2 dense | 2 spread] -- filled once by the caller.  The gadget's image columns are
 * max_rows = 2^17 - 9 cells high; the rows from max_rows up in every polynomial are the prover's blinding rows and
 * are never written.  Every AssignedHashResult output cell of every proof is read back from the proof's own slab
 * at column * 2^17 + row.  Build like examples/digest_abc.c (plus the HIP runtime for hipMalloc). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

#define K 8
#define N_ROWS (1u << 17)          /* cells per polynomial */
#define POLYS 14u                  /* polynomials per proof's slab */

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
    const uint64_t max_rows = N_ROWS - 9;                                            /* usable rows at k = 17 */
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, max_rows, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);

    /* the prover's memory: K slabs in one allocation of the library's allocator, filled once with a pattern of the
       caller's (a prover would zero its polynomials): cells the layout does not assign keep it */
    const uint64_t slab = (uint64_t)POLYS * N_ROWS;                                  /* cells */
    void *mem = NULL;
    if ((rc = hsw_device_alloc(0, (size_t)(K * slab) * HSW_CELL_BYTES, 0, &mem)) != HSW_OK) die("hsw_device_alloc", rc, eng);
    float ms = 0.f;
    if ((rc = hsw_fill_calibrate(eng, mem, (size_t)(K * slab) * HSW_CELL_BYTES, &ms)) != HSW_OK) die("hsw_fill_calibrate", rc, eng);
    uint8_t *base = (uint8_t *)mem;
    hsw_region_binding b;
    memset(&b, 0, sizeof b);
    b.d_columns = base;                                   b.column_pitch = N_ROWS; b.columns_capacity = 9; b.context_pitch = slab;
    b.d_lookup = base + 9ull * N_ROWS * HSW_CELL_BYTES;   b.lookup_capacity = N_ROWS; b.lookup_pitch = slab;
    b.d_chip_dense = base + 10ull * N_ROWS * HSW_CELL_BYTES;
    b.d_chip_spread = base + 12ull * N_ROWS * HSW_CELL_BYTES;
    b.chip_col_stride = N_ROWS; b.chip_rows_capacity = N_ROWS; b.chip_context_pitch = slab;
    if ((rc = hsw_gadget_bind_region(g, &b)) != HSW_OK) die("hsw_gadget_bind_region", rc, eng);

    /* proof h proves message h: 56 bytes of value h + 1 (proof 0 is the bench's own message) */
    uint8_t msg[K][56];
    const uint8_t *inputs[K];
    size_t lens[K], pre[K];
    for (int h = 0; h < K; h++) {
        memset(msg[h], h + 1, sizeof msg[h]);
        inputs[h] = msg[h]; lens[h] = sizeof msg[h]; pre[h] = 0;
    }
    hsw_hash_result r[K];
    if ((rc = hsw_gadget_digest_batch(g, K, inputs, lens, pre, r)) != HSW_OK) die("hsw_gadget_digest_batch", rc, eng);
    for (int h = 0; h < K; h++) {
        hsw_context_region reg;
        if ((rc = hsw_gadget_context_region(g, (size_t)h, &reg)) != HSW_OK) die("hsw_gadget_context_region", rc, eng);
        if (reg.d_image != base + (uint64_t)h * slab * HSW_CELL_BYTES) return 1;     /* the proof's own slab */
        /* AssignedHashResult.output_bytes: the 32 load_witness cells of the epilogue (lib.rs:317-324), read from
           proof h's own polynomials at the (FlexGate column, row) the gadget reports */
        char hex[65];
        for (int k = 0; k < 32; k++) {
            const uint64_t cell = r[h].epilogue_cell + 76 * (r[h].n_blocks + 1) + 36 * (uint64_t)(k / 4) + 5 * (uint64_t)(k % 4);
            uint64_t col, row, val[4];
            hsw_gadget_cell_position(g, cell, &col, &row);
            const uint8_t *at = base + ((uint64_t)h * slab + col * N_ROWS + row) * HSW_CELL_BYTES;
            if ((rc = hsw_download(eng, val, at, sizeof val)) != HSW_OK) die("hsw_download", rc, eng);
            if (val[0] != r[h].output_bytes[k] || val[1] || val[2] || val[3]) return 1;
            sprintf(hex + 2 * k, "%02x", (unsigned)val[0]);
        }
        /* a blinding row of the proof's last image column: still what the prover put there */
        uint64_t blind[4];
        const uint8_t *at = base + ((uint64_t)h * slab + (reg.columns - 1) * N_ROWS + max_rows) * HSW_CELL_BYTES;
        if ((rc = hsw_download(eng, blind, at, sizeof blind)) != HSW_OK) die("hsw_download", rc, eng);
        if (blind[0] != 0x01010101u || blind[1] || blind[2] != 0x01010101u || blind[3]) return 1;   /* hsw_fill_calibrate's pattern */
        printf("proof %d: %llu columns of %u cells, digest %s\n", h, (unsigned long long)reg.columns, N_ROWS, hex);
    }
    hsw_verify_report rep;
    if ((rc = hsw_gadget_verify(g, &rep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)rep.checks,
           (unsigned long long)rep.violations);
    if (rep.violations != 0) return 1;
    hsw_gadget_destroy(g);                                /* the slabs stay the caller's */
    if ((rc = hsw_device_free(mem)) != HSW_OK) die("hsw_device_free", rc, eng);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
