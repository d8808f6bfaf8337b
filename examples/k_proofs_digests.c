/* Plain C99: K = 4 proofs of a circuit that hashes TWO buffers per proof (the reference's Sha256DynamicConfig with
 * max_variable_byte_sizes = [128, 64], as its own TestCircuit makes two digests in one Context, lib.rs:455-466) and
 * assigns cells of its own between the two digests -- an interlude.  All 8 digests are synthesized by one
 * hsw_gadget_digest_batch call (two expansion launches: one per digest index, not one per digest), every proof a
 * FlexGate column image of its own (hsw_gadget_create_contexts).  The pass is verified on the device; then each
 * proof's two digests are read back from its own image through hsw_gadget_context_region.  Build like
 * examples/digest_abc.c. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

#define K 4
#define M 2

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    const size_t sizes[M] = {128, 64};                                               /* ONE proof's digests */
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_contexts(eng, sizes, M, K, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK)
        die("hsw_gadget_create_contexts", rc, eng);
    const uint64_t max_rows = (1u << 17) - 9;                                        /* usable rows at k = 17 */
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, max_rows, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);

    /* The interlude: after digest 0 the circuit assigns 1000 cells of its own and queues 12 lookups.  Where digest 0
       ends follows from the sizes alone (hsw_frame_query): its cells + the Context's zero cell, its lookup entries. */
    hsw_shape shape;
    hsw_frame_shape fs0;
    if ((rc = hsw_engine_shape(eng, &shape)) != HSW_OK) die("hsw_engine_shape", rc, eng);
    if ((rc = hsw_frame_query(&shape, sizes[0], 1, &fs0)) != HSW_OK) die("hsw_frame_query", rc, eng);
    uint64_t col = 0, row = 0;
    hsw_gadget_cell_position(g, fs0.digest_cells, &col, &row);                       /* digest 0's last cell (cells 0 .. digest_cells) */
    const uint64_t own_cells = 1000, own_lookups = 12;
    if ((rc = hsw_gadget_set_digest_origin(g, 1, col, row + 1 + own_cells, fs0.digest_lookups + own_lookups)) != HSW_OK)
        die("hsw_gadget_set_digest_origin", rc, eng);

    /* proof c hashes 100 bytes of value c + 1 and 55 bytes of value 0x80 + c */
    uint8_t msg[K * M][100];
    const uint8_t *inputs[K * M];
    size_t lens[K * M], pre[K * M];
    for (int c = 0; c < K; c++) {
        memset(msg[c * M], c + 1, 100);
        memset(msg[c * M + 1], 0x80 + c, 55);
        lens[c * M] = 100; lens[c * M + 1] = 55;
    }
    for (int d = 0; d < K * M; d++) { inputs[d] = msg[d]; pre[d] = 0; }
    hsw_hash_result r[K * M];
    hsw_launch_info before, after;
    memset(&before, 0, sizeof before);
    (void)hsw_last_launch(eng, &before);                                             /* (nothing launched yet: stays zero) */
    if ((rc = hsw_gadget_digest_batch(g, K * M, inputs, lens, pre, r)) != HSW_OK) die("hsw_gadget_digest_batch", rc, eng);
    if ((rc = hsw_last_launch(eng, &after)) != HSW_OK) die("hsw_last_launch", rc, eng);
    printf("%d digests, %u expansion launches\n", K * M, (unsigned)(after.seq - before.seq));

    hsw_verify_report rep;
    if ((rc = hsw_gadget_verify(g, &rep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)rep.checks,
           (unsigned long long)rep.violations);
    if (rep.violations != 0) return 1;

    for (int c = 0; c < K; c++) {
        hsw_context_region reg;
        if ((rc = hsw_gadget_context_region(g, (size_t)c, &reg)) != HSW_OK) die("hsw_gadget_context_region", rc, eng);
        if (!reg.assigned) return 1;
        for (int j = 0; j < M; j++) {
            const hsw_hash_result *d = &r[c * M + j];
            /* AssignedHashResult.output_bytes: the 32 load_witness cells of the epilogue (lib.rs:317-324), read from
               proof c's own image at the (FlexGate column, row) the gadget reports */
            char hex[65];
            for (int b = 0; b < 32; b++) {
                const uint64_t cell = d->epilogue_cell + 76 * (d->n_blocks + 1) + 36 * (uint64_t)(b / 4) + 5 * (uint64_t)(b % 4);
                uint64_t val[4];
                hsw_gadget_cell_position(g, cell, &col, &row);
                const uint8_t *at = (const uint8_t *)reg.d_image + ((col - reg.origin_column) * reg.max_rows + row) * HSW_CELL_BYTES;
                if ((rc = hsw_download(eng, val, at, sizeof val)) != HSW_OK) die("hsw_download", rc, eng);
                if (val[0] != d->output_bytes[b] || val[1] || val[2] || val[3]) return 1;
                sprintf(hex + 2 * b, "%02x", (unsigned)val[0]);
            }
            hsw_gadget_cell_position(g, d->prologue_cell, &col, &row);
            printf("proof %d digest %d: starts at (%llu, %llu) of %llu x %llu, digest %s\n", c, j, (unsigned long long)col,
                   (unsigned long long)row, (unsigned long long)reg.columns, (unsigned long long)reg.max_rows, hex);
        }
    }
    hsw_gadget_destroy(g);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
