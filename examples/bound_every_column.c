/* Plain C99: K = 2 proofs of the reference's BENCH circuit (benches/digest.rs:93-129) written STRAIGHT into a prover
 * that keeps ALL its advice the way halo2_proofs does -- one allocation per column per proof (Vec<Polynomial<F>>),
 * wherever the allocator puts them (hsw_gadget_bind_column_tables): per proof 9 FlexGate columns, 1 lookup-advice
 * column and 2 dense + 2 spread chip columns, each a hipMalloc of n = 2^17 cells of its own -- 18 + 2 + 8 allocations.
 * Every AssignedHashResult output cell is read back through the column's own pointer, the first lookup entry and chip
 * row of every proof through theirs, then the region is verified on the device.  Build like examples/digest_abc.c,
 * plus -lamdhip64 for hipMalloc. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

/* the two HIP runtime calls this program makes itself (hip_runtime_api.h, which plain C99 -pedantic cannot include) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);

#define K 2
#define COLS 9
#define NCOLS 2                    /* num_advice_columns: chip columns per family */
#define N_ROWS (1u << 17)          /* cells per polynomial */

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[K];
    for (int h = 0; h < K; h++) sizes[h] = 1024;
    hsw_gadget *g = NULL;
    rc = hsw_gadget_create_ex(eng, sizes, K, 1,
                              HSW_GADGET_WHOLE_DIGEST | HSW_GADGET_INDEPENDENT | HSW_GADGET_CONTEXT_IMAGES, &g);
    if (rc != HSW_OK) die("hsw_gadget_create_ex", rc, eng);
    const uint64_t max_rows = N_ROWS - 9;
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, max_rows, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);
    if (columns != COLS) return 1;

    /* the prover's polynomials: one allocation per column per proof, the last column first */
    void *col[K * COLS], *lookup[K], *dense[K * NCOLS], *spread[K * NCOLS];
    void **all[4] = {col, lookup, dense, spread};
    const int count[4] = {K * COLS, K, K * NCOLS, K * NCOLS};
    for (int t = 3; t >= 0; t--)
        for (int i = count[t] - 1; i >= 0; i--)
            if (hipMalloc(&all[t][i], (size_t)N_ROWS * HSW_CELL_BYTES) != 0) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    hsw_region_binding b;                                  /* capacities only: no pitch describes these columns */
    memset(&b, 0, sizeof b);
    b.column_pitch = N_ROWS; b.columns_capacity = COLS;
    b.lookup_capacity = N_ROWS; b.chip_rows_capacity = N_ROWS;
    hsw_column_tables t;
    memset(&t, 0, sizeof t);
    t.d_column_ptrs = col;          t.n_column_ptrs = K * COLS;
    t.d_lookup_ptrs = lookup;       t.n_lookup_ptrs = K;
    t.d_chip_dense_ptrs = dense;    t.d_chip_spread_ptrs = spread; t.n_chip_ptrs = K * NCOLS;
    if ((rc = hsw_gadget_bind_column_tables(g, &b, &t)) != HSW_OK) die("hsw_gadget_bind_column_tables", rc, eng);

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
        if (reg.d_image != col[h * COLS] || reg.d_lookup != lookup[h] || reg.d_chip_dense != dense[h * NCOLS] ||
            reg.d_chip_spread != spread[h * NCOLS]) return 1;   /* proof h's own column-0 pointers */
        /* the proof's first limb call: dense < 2^8 in chip column 0, row 0, and its spread next to it; its first lookup
         * entry a 16-bit value */
        uint64_t d0[4], s0[4], l0[4];
        if ((rc = hsw_download(eng, d0, dense[h * NCOLS], sizeof d0)) != HSW_OK || (rc = hsw_download(eng, s0, spread[h * NCOLS], sizeof s0)) != HSW_OK ||
            (rc = hsw_download(eng, l0, lookup[h], sizeof l0)) != HSW_OK) die("hsw_download", rc, eng);
        uint64_t sp = 0;
        for (int bit = 0; bit < 8; bit++) sp |= ((d0[0] >> bit) & 1u) << (2 * bit);
        if (d0[0] >= 256 || d0[1] || s0[0] != sp || s0[1] || l0[0] >= 65536 || l0[1]) return 1;
        char hex[65];
        for (int k = 0; k < 32; k++) {
            const uint64_t cell = r[h].epilogue_cell + 76 * (r[h].n_blocks + 1) + 36 * (uint64_t)(k / 4) + 5 * (uint64_t)(k % 4);
            uint64_t c, row, val[4];
            hsw_gadget_cell_position(g, cell, &c, &row);
            const uint8_t *at = (const uint8_t *)col[h * COLS + c] + row * HSW_CELL_BYTES;   /* the column's own allocation */
            if ((rc = hsw_download(eng, val, at, sizeof val)) != HSW_OK) die("hsw_download", rc, eng);
            if (val[0] != r[h].output_bytes[k] || val[1] || val[2] || val[3]) return 1;
            sprintf(hex + 2 * k, "%02x", (unsigned)val[0]);
        }
        printf("proof %d: %llu + 1 + %d columns by pointer, digest %s\n", h, (unsigned long long)reg.columns, 2 * NCOLS, hex);
    }
    hsw_verify_report rep;
    if ((rc = hsw_gadget_verify(g, &rep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)rep.checks,
           (unsigned long long)rep.violations);
    if (rep.violations != 0) return 1;
    hsw_gadget_destroy(g);                                /* the columns stay the caller's */
    for (int t2 = 0; t2 < 4; t2++)
        for (int i = 0; i < count[t2]; i++) hipFree(all[t2][i]);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
