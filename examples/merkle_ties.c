/* Plain C99: the 8-leaf Merkle tree of examples/merkle_device.c, and what makes its 15 digests a TREE for the circuit:
 * the copy constraints between them.  hsw_gadget_ties lists, for every inner node, "input-byte cell k of the parent
 * equals output-byte cell j of the child" -- 64 per inner node, 7 x 64 = 448 in all -- as the constrain_equal calls
 * the circuit makes; hsw_gadget_cell_position says where the two cells of one sit in the FlexGate image;
 * hsw_gadget_verify_ties checks all of them on the device, cell against cell (hsw_gadget_verify checks each digest
 * against its own inputs and would not notice a parent that hashed other bytes).  Build like examples/digest_abc.c. */
#include <stdio.h>
#include <stdlib.h>

#include "hsw.h"

#define LEAVES 8
#define NODES (2 * LEAVES - 1)
#define ARENA 1024u                 /* bytes the leaves are cut from */

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
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

    /* device memory of the caller's: [ leaf bytes | nodes ], the leaf bytes produced on the device */
    void *mem = NULL;
    if ((rc = hsw_device_alloc(0, ARENA + 32 * NODES, 0, &mem)) != HSW_OK) die("hsw_device_alloc", rc, eng);
    float ms = 0.f;
    if ((rc = hsw_fill_calibrate(eng, mem, ARENA, &ms)) != HSW_OK) die("hsw_fill_calibrate", rc, eng);
    uint8_t *d_leaves = (uint8_t *)mem, *d_nodes = d_leaves + ARENA;

    static const size_t leaf_len[LEAVES] = {0, 1, 55, 56, 63, 64, 100, 119};
    const void *inputs[NODES];
    void *outputs[NODES];
    size_t lens[NODES];
    uint32_t levels[NODES];
    for (int i = 0; i < LEAVES; i++) {
        inputs[i] = d_leaves + 120 * (size_t)i + (size_t)(2 * i + 1); lens[i] = leaf_len[i]; levels[i] = 0;
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

    /* the copy constraints between the digests: first the count, then the list */
    size_t n_ties = 0;
    uint64_t untied = 0;
    if ((rc = hsw_gadget_ties(g, NULL, 0, &n_ties, &untied)) != HSW_OK) die("hsw_gadget_ties", rc, eng);
    printf("%zu ties, %llu prefix bytes untied\n", n_ties, (unsigned long long)untied);
    if (n_ties != 7 * 64 || untied != 0) {
        fprintf(stderr, "this is not a tree of %d leaves\n", LEAVES);
        return 1;
    }
    hsw_cell_tie *ties = (hsw_cell_tie *)malloc(n_ties * sizeof *ties);
    if (!ties) return 1;
    if ((rc = hsw_gadget_ties(g, ties, n_ties, NULL, NULL)) != HSW_OK) die("hsw_gadget_ties", rc, eng);

    /* one of them, as the circuit sees it: constrain_equal(advice[sc][sr], advice[dc][dr]) */
    const hsw_cell_tie *t = &ties[n_ties - 1];
    uint64_t sc, sr, dc, dr;
    if ((rc = hsw_gadget_cell_position(g, t->src_cell, &sc, &sr)) != HSW_OK) die("hsw_gadget_cell_position", rc, eng);
    if ((rc = hsw_gadget_cell_position(g, t->dst_cell, &dc, &dr)) != HSW_OK) die("hsw_gadget_cell_position", rc, eng);
    printf("tie %zu: output byte %u of digest %llu at (column %llu, row %llu) = input byte %u of digest %llu at (column %llu, row %llu)\n",
           n_ties - 1, t->src_byte, (unsigned long long)t->src_hash, (unsigned long long)sc, (unsigned long long)sr, t->dst_byte,
           (unsigned long long)t->dst_hash, (unsigned long long)dc, (unsigned long long)dr);
    free(ties);

    hsw_tie_report rep;
    if ((rc = hsw_gadget_verify_ties(g, &rep)) != HSW_OK) die("hsw_gadget_verify_ties", rc, eng);
    printf("ties checked on the device: %llu pairs, %llu violations\n", (unsigned long long)rep.checks,
           (unsigned long long)rep.violations);
    if (rep.violations != 0 || rep.checks != n_ties) return 1;
    hsw_gadget_destroy(g);
    if ((rc = hsw_device_free(mem)) != HSW_OK) die("hsw_device_free", rc, eng);
    hsw_engine_destroy(eng);
    puts("merkle ties ok");
    return 0;
}
