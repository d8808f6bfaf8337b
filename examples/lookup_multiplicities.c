/* Plain C99: the lookup-table multiplicities of K = 2 proofs of the reference's BENCH circuit (benches/digest.rs:93-129),
 * counted on the device from the columns the prover owns (hsw_gadget_bind_column_tables: one hipMalloc per column per
 * proof, as examples/bound_every_column.c).  hsw_gadget_lookup_runs lists where the entries lie -- per proof one run of
 * the lookup-advice column and one per chip column --, hsw_gadget_lookup_multiplicities counts them into two tables per
 * proof: 2^16 counters of the range table, 2^8 of the spread table.  The totals are checked against the closed forms:
 * 3 + 2 * max + n_blocks * 3184 + 64 range entries per digest (is_input_range_check on), 4,120 limb calls per block.
 * With m in hand a prover writes halo2's permuted input column as "row t, m[t] times" (after adding the unassigned rows
 * to m[0]) or uses m as the logUp numerators; it never sorts.  Build like examples/digest_abc.c, plus -lamdhip64. */
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
#define RANGE_ROWS 65536u
#define SPREAD_ROWS 256u

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

static uint32_t range_host[K * RANGE_ROWS], spread_host[K * SPREAD_ROWS];

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
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, N_ROWS - 9, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);
    if (columns != COLS) return 1;

    /* the prover's polynomials: one allocation per column per proof, the last column first */
    void *col[K * COLS], *lookup[K], *dense[K * NCOLS], *spread[K * NCOLS];
    void **all[4] = {col, lookup, dense, spread};
    const int count[4] = {K * COLS, K, K * NCOLS, K * NCOLS};
    for (int t = 3; t >= 0; t--)
        for (int i = count[t] - 1; i >= 0; i--)
            if (hipMalloc(&all[t][i], (size_t)N_ROWS * HSW_CELL_BYTES) != 0) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    hsw_region_binding b;
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

    /* where the lookup entries lie: per proof 1 range run in its own lookup column, 1 run per chip column */
    const uint64_t range_per_proof = 3 + 2 * 1024 + 16 * 3184 + 64, chip_per_proof = 16 * 4120;
    hsw_lookup_run runs[K * (1 + NCOLS)];
    size_t n_runs = 0;
    if ((rc = hsw_gadget_lookup_runs(g, runs, K * (1 + NCOLS), &n_runs)) != HSW_OK) die("hsw_gadget_lookup_runs", rc, eng);
    if (n_runs != K * (1 + NCOLS)) return 1;
    for (size_t i = 0; i < n_runs; i++) {
        const hsw_lookup_run *x = &runs[i];
        if (x->table == HSW_LOOKUP_RANGE) {
            if (x->d_cells != lookup[x->context] || x->n != range_per_proof || x->d_spread) return 1;
        } else if (x->d_cells != dense[x->context * NCOLS + x->column] || x->d_spread != spread[x->context * NCOLS + x->column] ||
                   x->n != chip_per_proof / NCOLS) return 1;
    }

    /* count: the tables are the prover's own device memory */
    void *d_range = NULL, *d_spread = NULL;
    if (hipMalloc(&d_range, sizeof range_host) != 0 || hipMalloc(&d_spread, sizeof spread_host) != 0) return 1;
    hsw_lookup_counts out;
    memset(&out, 0, sizeof out);
    out.d_range = (uint32_t *)d_range; out.d_spread = (uint32_t *)d_spread;      /* pitches 0: the table sizes */
    hsw_lookup_report rep;
    if ((rc = hsw_gadget_lookup_multiplicities(g, &out, &rep)) != HSW_OK) die("hsw_gadget_lookup_multiplicities", rc, eng);
    printf("range entries %llu, spread entries %llu, not in table %llu\n", (unsigned long long)rep.range_entries,
           (unsigned long long)rep.spread_entries, (unsigned long long)rep.not_in_table);
    if (rep.range_entries != K * range_per_proof || rep.spread_entries != K * chip_per_proof || rep.not_in_table != 0) return 1;
    if ((rc = hsw_download(eng, range_host, d_range, sizeof range_host)) != HSW_OK ||
        (rc = hsw_download(eng, spread_host, d_spread, sizeof spread_host)) != HSW_OK) die("hsw_download", rc, eng);
    for (int h = 0; h < K; h++) {
        uint64_t sr = 0, ss = 0, used_r = 0, used_s = 0;
        for (uint32_t i = 0; i < RANGE_ROWS; i++) { sr += range_host[h * RANGE_ROWS + i]; used_r += range_host[h * RANGE_ROWS + i] != 0; }
        for (uint32_t i = 0; i < SPREAD_ROWS; i++) { ss += spread_host[h * SPREAD_ROWS + i]; used_s += spread_host[h * SPREAD_ROWS + i] != 0; }
        printf("proof %d: range %llu entries over %llu rows, spread %llu entries over %llu rows\n", h, (unsigned long long)sr,
               (unsigned long long)used_r, (unsigned long long)ss, (unsigned long long)used_s);
        if (sr != range_per_proof || ss != chip_per_proof) return 1;
    }
    /* counting again on top doubles every counter */
    out.flags = HSW_LOOKUP_ACCUMULATE;
    if ((rc = hsw_gadget_lookup_multiplicities(g, &out, &rep)) != HSW_OK) die("hsw_gadget_lookup_multiplicities", rc, eng);
    uint32_t twice[SPREAD_ROWS];
    if ((rc = hsw_download(eng, twice, d_spread, sizeof twice)) != HSW_OK) die("hsw_download", rc, eng);
    for (uint32_t i = 0; i < SPREAD_ROWS; i++)
        if (twice[i] != 2 * spread_host[i]) return 1;

    hsw_verify_report vrep;
    if ((rc = hsw_gadget_verify(g, &vrep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)vrep.checks,
           (unsigned long long)vrep.violations);
    if (vrep.violations != 0) return 1;
    hsw_gadget_destroy(g);                                /* the columns and the tables stay the caller's */
    hipFree(d_range); hipFree(d_spread);
    for (int t2 = 0; t2 < 4; t2++)
        for (int i = 0; i < count[t2]; i++) hipFree(all[t2][i]);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
