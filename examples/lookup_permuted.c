/* Plain C99: halo2's permuted lookup columns of K = 2 proofs of the reference's BENCH circuit (benches/digest.rs:93-129),
 * written on the device from the columns the prover owns (hsw_gadget_bind_column_tables: one hipMalloc per column per
 * proof, as examples/lookup_multiplicities.c).  Per proof there are three lookup arguments -- the range lookup of the
 * lookup-advice column and one spread lookup per chip column -- and each gets an A' and an S' column of USABLE rows:
 * hsw_gadget_lookup_permuted counts the argument's multiplicities, adds the unassigned rows to row 0 and writes
 * "row t, m'[t] times" into A' and the matching arrangement of the table into S'.  Nothing is sorted.  The program
 * downloads the columns and checks the two constraints halo2 puts on a permuted pair:
 *   A'[0] == S'[0],  and for i > 0:  A'[i] == S'[i]  or  A'[i] == A'[i-1].
 * Build like examples/digest_abc.c, plus -lamdhip64. */
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
#define USABLE (N_ROWS - 9)        /* the rest are blinding rows: the prover's */
#define ARGS (K * (1 + NCOLS))     /* K range arguments, then K * NCOLS spread arguments */

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

static uint64_t a_host[USABLE][4], s_host[USABLE][4];

/* the two permuted-pair constraints on one pair of downloaded columns; returns the number of distinct runs, 0 = violated */
static uint64_t check_pair(void) {
    uint64_t runs = 1;
    if (memcmp(a_host[0], s_host[0], 32) != 0) return 0;
    for (uint32_t i = 1; i < USABLE; i++) {
        const int same = memcmp(a_host[i], a_host[i - 1], 32) == 0;
        if (!same && memcmp(a_host[i], s_host[i], 32) != 0) return 0;
        runs += !same;
    }
    return runs;
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
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, USABLE, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);
    if (columns != COLS) return 1;

    /* the prover's polynomials: one allocation per column per proof, the last column first; the permuted columns too */
    void *col[K * COLS], *lookup[K], *dense[K * NCOLS], *spread[K * NCOLS], *perm_in[ARGS], *perm_tab[ARGS];
    void **all[6] = {col, lookup, dense, spread, perm_in, perm_tab};
    const int count[6] = {K * COLS, K, K * NCOLS, K * NCOLS, ARGS, ARGS};
    for (int t = 5; t >= 0; t--)
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

    /* the challenge of each proof, as the cells are stored (canonical here): any field element below p */
    uint64_t theta[K][4];
    for (int h = 0; h < K; h++) {
        theta[h][0] = 0x9e3779b97f4a7c15ull * (uint64_t)(h + 1); theta[h][1] = 0xc2b2ae3d27d4eb4full + (uint64_t)h;
        theta[h][2] = 0x165667b19e3779f9ull; theta[h][3] = 0x1000000000000000ull + (uint64_t)h;
    }
    const uint64_t range_per_proof = 3 + 2 * 1024 + 16 * 3184 + 64, chip_per_proof = 16 * 4120;
    hsw_lookup_permuted p;
    hsw_permuted_report rep;
    /* the K range arguments: columns perm_*[0 .. K) */
    memset(&p, 0, sizeof p);
    p.table = HSW_LOOKUP_RANGE; p.usable_rows = USABLE; p.n_arguments = K;
    p.d_input_columns = perm_in; p.d_table_columns = perm_tab;
    if ((rc = hsw_gadget_lookup_permuted(g, &p, &rep)) != HSW_OK) die("hsw_gadget_lookup_permuted", rc, eng);
    printf("range: %llu arguments, %llu entries, %llu cells written, not in table %llu\n", (unsigned long long)rep.arguments,
           (unsigned long long)rep.entries, (unsigned long long)rep.written, (unsigned long long)rep.not_in_table);
    if (rep.entries != K * range_per_proof || rep.written != 2ull * USABLE * K || rep.not_in_table != 0) return 1;
    /* the K * NCOLS spread arguments: columns perm_*[K .. ARGS), argument c * NCOLS + k */
    p.table = HSW_LOOKUP_SPREAD; p.n_arguments = K * NCOLS; p.thetas = theta;
    p.d_input_columns = perm_in + K; p.d_table_columns = perm_tab + K;
    if ((rc = hsw_gadget_lookup_permuted(g, &p, &rep)) != HSW_OK) die("hsw_gadget_lookup_permuted", rc, eng);
    printf("spread: %llu arguments, %llu entries, %llu cells written, not in table %llu\n", (unsigned long long)rep.arguments,
           (unsigned long long)rep.entries, (unsigned long long)rep.written, (unsigned long long)rep.not_in_table);
    if (rep.entries != K * chip_per_proof || rep.written != 2ull * USABLE * K * NCOLS || rep.not_in_table != 0) return 1;

    /* what halo2 asks of a permuted pair, on the host */
    for (int a = 0; a < ARGS; a++) {
        if ((rc = hsw_download(eng, a_host, perm_in[a], sizeof a_host)) != HSW_OK ||
            (rc = hsw_download(eng, s_host, perm_tab[a], sizeof s_host)) != HSW_OK) die("hsw_download", rc, eng);
        const uint64_t runs = check_pair();
        printf("argument %d (%s): %llu distinct rows in A', constraints hold: %s\n", a, a < K ? "range" : "spread",
               (unsigned long long)runs, runs ? "yes" : "NO");
        if (!runs || runs > (a < K ? 65536u : 256u)) return 1;
    }

    hsw_verify_report vrep;
    if ((rc = hsw_gadget_verify(g, &vrep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)vrep.checks,
           (unsigned long long)vrep.violations);
    if (vrep.violations != 0) return 1;
    hsw_gadget_destroy(g);                                /* the columns stay the caller's */
    for (int t2 = 0; t2 < 6; t2++)
        for (int i = 0; i < count[t2]; i++) hipFree(all[t2][i]);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
