/* Plain C99: the lookup argument's grand-product column Z of K = 2 proofs of the reference's BENCH circuit
 * (benches/digest.rs:93-129), written on the device.  examples/lookup_permuted.c continued: the prover owns every column
 * (hsw_gadget_bind_column_tables: one hipMalloc per column per proof), hsw_gadget_lookup_permuted writes the permuted
 * pair A' / S' of each of the three lookup arguments per proof, and hsw_gadget_lookup_product reads the unpermuted inputs
 * where the digests wrote them (hsw_gadget_lookup_runs: the lookup-advice column, the chip columns), the pair, and writes
 *   Z[0] = 1,  Z[i+1] = Z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma))
 * into a column of USABLE + 1 cells per argument.  The program downloads everything and checks the argument's own
 * constraint, row by row, with a small Montgomery multiply of its own:
 *   Z[0] == 1,  Z[i+1] (A'[i] + beta)(S'[i] + gamma) == Z[i] (A[i] + beta)(S[i] + gamma),  Z[USABLE] == 1.
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

/* ---- BN254 Fr on the host, eight 32-bit limbs: just enough to check the recurrence ---- */
typedef struct { uint32_t l[8]; } fe;
static const fe P = {{0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
static const fe R2 = {{0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u}};

static fe reduce_once(fe a) {                       /* a - p if a >= p (a < 2p) */
    fe d;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] - P.l[j] - br;
        d.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    return br ? a : d;
}
static fe add(fe a, fe b) {
    uint64_t cy = 0;
    for (int j = 0; j < 8; j++) { cy += (uint64_t)a.l[j] + b.l[j]; a.l[j] = (uint32_t)cy; cy >>= 32; }
    return reduce_once(a);
}
static fe mul(fe a, fe b) {                         /* a b 2^-256 mod p */
    uint32_t t[10];
    memset(t, 0, sizeof t);
    for (int i = 0; i < 8; i++) {
        uint64_t acc = 0;
        for (int j = 0; j < 8; j++) { acc = (uint64_t)a.l[j] * b.l[i] + t[j] + (acc >> 32); t[j] = (uint32_t)acc; }
        acc = (uint64_t)t[8] + (acc >> 32); t[8] = (uint32_t)acc; t[9] = (uint32_t)(acc >> 32);
        const uint32_t m = t[0] * 0xefffffffu;
        acc = (uint64_t)m * P.l[0] + t[0];
        for (int j = 1; j < 8; j++) { acc = (uint64_t)m * P.l[j] + t[j] + (acc >> 32); t[j - 1] = (uint32_t)acc; }
        acc = (uint64_t)t[8] + (acc >> 32); t[7] = (uint32_t)acc; t[8] = t[9] + (uint32_t)(acc >> 32);
    }
    fe r;
    memcpy(r.l, t, 32);
    return reduce_once(r);
}
static fe small(uint32_t x) { fe r; memset(&r, 0, sizeof r); r.l[0] = x; return r; }
static uint32_t spread_of(uint32_t t) { uint32_t s = 0; for (int b = 0; b < 16; b++) s |= ((t >> b) & 1u) << (2 * b); return s; }

static fe in_host[USABLE], sp_host[USABLE], a_host[USABLE], s_host[USABLE], z_host[USABLE + 1];

/* the recurrence over one argument's downloaded columns; theta_r = theta * 2^256 so that mul(x, theta_r) = x theta.
 * Both sides of a row carry the same power of 2^-256, so the canonical cells are compared as they are. */
static int check_product(int spread, uint64_t rows, fe theta_r, fe beta, fe gamma) {
    const uint32_t T = spread ? 256u : 65536u;
    const fe one = small(1);
    if (memcmp(&z_host[0], &one, 32) != 0 || memcmp(&z_host[USABLE], &one, 32) != 0) return 0;
    for (uint32_t i = 0; i < USABLE; i++) {
        fe a = small(0);
        if (i < rows) a = spread ? add(mul(in_host[i], theta_r), sp_host[i]) : in_host[i];
        const uint32_t t = i < T ? i : 0;
        const fe s = spread ? add(mul(small(t), theta_r), small(spread_of(t))) : small(t);
        const fe num = mul(add(a, beta), add(s, gamma)), den = mul(add(a_host[i], beta), add(s_host[i], gamma));
        const fe lhs = mul(z_host[i + 1], den), rhs = mul(z_host[i], num);
        if (memcmp(&lhs, &rhs, 32) != 0) return 0;
    }
    return 1;
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

    /* the prover's polynomials: one allocation per column per proof; the permuted columns and Z too */
    void *col[K * COLS], *lookup[K], *dense[K * NCOLS], *spread[K * NCOLS], *perm_in[ARGS], *perm_tab[ARGS], *z[ARGS];
    void **all[7] = {col, lookup, dense, spread, perm_in, perm_tab, z};
    const int count[7] = {K * COLS, K, K * NCOLS, K * NCOLS, ARGS, ARGS, ARGS};
    for (int t = 6; t >= 0; t--)
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

    /* the challenges of each proof, as the cells are stored (canonical here): any field elements below p */
    uint64_t theta[K][4], beta[K][4], gamma[K][4];
    for (int h = 0; h < K; h++) {
        theta[h][0] = 0x9e3779b97f4a7c15ull * (uint64_t)(h + 1); theta[h][1] = 0xc2b2ae3d27d4eb4full + (uint64_t)h;
        theta[h][2] = 0x165667b19e3779f9ull; theta[h][3] = 0x1000000000000000ull + (uint64_t)h;
        for (int j = 0; j < 4; j++) { beta[h][j] = theta[h][j] ^ 0x0123456789abcdefull; gamma[h][j] = theta[h][j] + 0x1111111111111111ull * (uint64_t)(j + 1); }
        beta[h][3] &= 0x1fffffffffffffffull; gamma[h][3] &= 0x1fffffffffffffffull;
    }

    /* where the unpermuted inputs are: the runs of the pass, one per argument for this circuit */
    hsw_lookup_run runs[ARGS];
    size_t n_runs = 0;
    if ((rc = hsw_gadget_lookup_runs(g, runs, ARGS, &n_runs)) != HSW_OK) die("hsw_gadget_lookup_runs", rc, eng);
    if (n_runs != ARGS) return 1;
    const void *in[ARGS], *in_spread[ARGS];
    uint64_t in_rows[ARGS];
    for (size_t i = 0; i < n_runs; i++) {          /* argument a: ranges first, as the columns above are numbered */
        const size_t a = runs[i].table == HSW_LOOKUP_RANGE ? runs[i].context : K + runs[i].context * NCOLS + runs[i].column;
        in[a] = runs[i].d_cells; in_spread[a] = runs[i].d_spread; in_rows[a] = runs[i].n;
    }

    hsw_lookup_permuted p;
    hsw_permuted_report prep;
    hsw_lookup_product q;
    hsw_product_report rep;
    uint32_t status[ARGS];
    for (int spread_arg = 0; spread_arg < 2; spread_arg++) {
        const int a0 = spread_arg ? K : 0, n = spread_arg ? K * NCOLS : K;
        memset(&p, 0, sizeof p);
        p.table = spread_arg ? HSW_LOOKUP_SPREAD : HSW_LOOKUP_RANGE; p.usable_rows = USABLE; p.n_arguments = (size_t)n;
        p.d_input_columns = perm_in + a0; p.d_table_columns = perm_tab + a0; p.thetas = spread_arg ? theta : NULL;
        if ((rc = hsw_gadget_lookup_permuted(g, &p, &prep)) != HSW_OK) die("hsw_gadget_lookup_permuted", rc, eng);
        if (prep.written != 2ull * USABLE * (uint64_t)n) return 1;
        memset(&q, 0, sizeof q);
        q.table = p.table; q.usable_rows = USABLE; q.n_arguments = (size_t)n;
        q.d_inputs = in + a0; q.d_inputs_spread = spread_arg ? in_spread + a0 : NULL; q.input_rows = in_rows + a0;
        q.d_permuted_inputs = (const void *const *)(perm_in + a0); q.d_permuted_tables = (const void *const *)(perm_tab + a0);
        q.d_products = z + a0;
        q.thetas = spread_arg ? theta : NULL; q.betas = beta; q.gammas = gamma; q.status = status + a0;
        if ((rc = hsw_gadget_lookup_product(g, &q, &rep)) != HSW_OK) die("hsw_gadget_lookup_product", rc, eng);
        printf("%s: %llu arguments, %llu cells written, open %llu, refused %llu, tiles of %u rows\n", spread_arg ? "spread" : "range",
               (unsigned long long)rep.arguments, (unsigned long long)rep.written, (unsigned long long)rep.open_arguments,
               (unsigned long long)rep.refused_arguments, rep.tile_rows);
        if (rep.written != (USABLE + 1ull) * (uint64_t)n || rep.open_arguments || rep.refused_arguments) return 1;
    }

    /* the argument's own constraint, on the host */
    for (int a = 0; a < ARGS; a++) {
        const int spread_arg = a >= K, c = spread_arg ? (a - K) / NCOLS : a;
        memset(in_host, 0, sizeof in_host); memset(sp_host, 0, sizeof sp_host);
        if ((rc = hsw_download(eng, in_host, in[a], (size_t)in_rows[a] * 32)) != HSW_OK ||
            (spread_arg && (rc = hsw_download(eng, sp_host, in_spread[a], (size_t)in_rows[a] * 32)) != HSW_OK) ||
            (rc = hsw_download(eng, a_host, perm_in[a], sizeof a_host)) != HSW_OK ||
            (rc = hsw_download(eng, s_host, perm_tab[a], sizeof s_host)) != HSW_OK ||
            (rc = hsw_download(eng, z_host, z[a], sizeof z_host)) != HSW_OK) die("hsw_download", rc, eng);
        fe th, be, ga;
        memcpy(&th, theta[c], 32); memcpy(&be, beta[c], 32); memcpy(&ga, gamma[c], 32);
        const int ok = status[a] == 0 && check_product(spread_arg, in_rows[a], mul(th, R2), be, ga);
        printf("argument %d (%s): %llu assigned rows, Z closes and satisfies the recurrence: %s\n", a, spread_arg ? "spread" : "range",
               (unsigned long long)in_rows[a], ok ? "yes" : "NO");
        if (!ok) return 1;
    }

    hsw_verify_report vrep;
    if ((rc = hsw_gadget_verify(g, &vrep)) != HSW_OK) die("hsw_gadget_verify", rc, eng);
    printf("verified on the device: %llu constraints, %llu violations\n", (unsigned long long)vrep.checks,
           (unsigned long long)vrep.violations);
    if (vrep.violations != 0) return 1;
    hsw_gadget_destroy(g);                                /* the columns stay the caller's */
    for (int t2 = 0; t2 < 7; t2++)
        for (int i = 0; i < count[t2]; i++) hipFree(all[t2][i]);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
