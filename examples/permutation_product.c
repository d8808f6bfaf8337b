/* Plain C99: the permutation argument's grand products of a two-leaf Merkle tree hashed in circuit -- what ENFORCES the
 * copy constraints that examples/merkle_ties.c lists.  Two leaves and their parent go through
 * hsw_gadget_digest_levels_device; hsw_gadget_ties names the 64 constrain_equal pairs (input byte k of the parent =
 * output byte j of a leaf) and hsw_gadget_cell_position places them in the FlexGate image.  The program then plays
 * keygen on the host: sigma is the identity delta^j omega^i except that the cells of every tie form a cycle; uploads
 * the sigma columns; and hsw_gadget_permutation_product reads the advice columns where the digests wrote them and writes
 *   Z_s[i+1] = Z_s[i] prod_j (v_j[i] + beta delta^j omega^i + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma)
 * for the S = ceil(columns / CHUNK) chunks, Z_0[0] = 1, Z_s[0] = Z_{s-1}[USABLE].  Everything is downloaded and the
 * argument's own constraint checked row by row with a small Montgomery multiply of the program's own; the last value is 1:
 * the tree satisfies its copy constraints.  omega and delta are this program's (any two elements with distinct labels
 * serve it; a prover passes its domain's).  Build like examples/digest_abc.c, plus -lamdhip64. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

/* the HIP runtime calls this program makes itself (hip_runtime_api.h, which plain C99 -pedantic cannot include) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);      /* kind 1: host to device */

#define NODES 3
#define N_ROWS (1u << 17)          /* cells per polynomial */
#define USABLE (N_ROWS - 9)        /* the rest are blinding rows: the prover's */
#define CHUNK 2                    /* halo2's cs_degree - 2 */
#define MAX_COLS 8

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

/* ---- BN254 Fr on the host, eight 32-bit limbs: just enough to build sigma and check the recurrence ---- */
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
static fe times(fe a, fe b) { return mul(mul(a, b), R2); }      /* a b, canonical in and out */

static fe label[MAX_COLS][USABLE], sigma[MAX_COLS][USABLE], v[MAX_COLS][USABLE], z[USABLE + 1];

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[NODES] = {128, 128, 128};
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_ex(eng, sizes, NODES, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);
    uint64_t columns = 0;
    if ((rc = hsw_gadget_set_columns(g, USABLE, &columns)) != HSW_OK) die("hsw_gadget_set_columns", rc, eng);
    if (columns > MAX_COLS) return 1;
    const size_t m = (size_t)columns, S = (m + CHUNK - 1) / CHUNK;

    /* two leaves cut from device memory of the caller's, the parent reads their digests where the leaves' launches wrote them */
    void *mem = NULL;
    if ((rc = hsw_device_alloc(0, 256 + 32 * NODES, 0, &mem)) != HSW_OK) die("hsw_device_alloc", rc, eng);
    float ms = 0.f;
    if ((rc = hsw_fill_calibrate(eng, mem, 256, &ms)) != HSW_OK) die("hsw_fill_calibrate", rc, eng);
    uint8_t *d_leaves = (uint8_t *)mem, *d_nodes = d_leaves + 256;
    const void *inputs[NODES] = {d_leaves + 1, d_leaves + 130, d_nodes};
    void *outputs[NODES] = {d_nodes, d_nodes + 32, d_nodes + 64};
    const size_t lens[NODES] = {10, 119, 64};
    const uint32_t levels[NODES] = {0, 0, 1};
    hsw_hash_result r[NODES];
    if ((rc = hsw_gadget_digest_levels_device(g, NODES, inputs, lens, NULL, levels, outputs, r)) != HSW_OK)
        die("hsw_gadget_digest_levels_device", rc, eng);
    hsw_cell_tie ties[64];
    size_t n_ties = 0;
    if ((rc = hsw_gadget_ties(g, NULL, 0, &n_ties, NULL)) != HSW_OK) die("hsw_gadget_ties", rc, eng);
    if (n_ties != 64) return 1;
    if ((rc = hsw_gadget_ties(g, ties, n_ties, NULL, NULL)) != HSW_OK) die("hsw_gadget_ties", rc, eng);

    /* keygen on the host: labels delta^j omega^i, sigma = the labels with every tie's two cells exchanged */
    const fe omega = small(5), delta = small(7);
    fe dj = small(1);
    for (size_t j = 0; j < m; j++) {
        fe w = dj;
        for (uint32_t i = 0; i < USABLE; i++) { label[j][i] = w; w = times(w, omega); }
        dj = times(dj, delta);
    }
    memcpy(sigma, label, sizeof label);
    for (size_t k = 0; k < n_ties; k++) {           /* (every source byte of this tree is tied once: cycles of two) */
        uint64_t sc, sr, dc, dr;
        if ((rc = hsw_gadget_cell_position(g, ties[k].src_cell, &sc, &sr)) != HSW_OK ||
            (rc = hsw_gadget_cell_position(g, ties[k].dst_cell, &dc, &dr)) != HSW_OK) die("hsw_gadget_cell_position", rc, eng);
        sigma[sc][sr] = label[dc][dr];
        sigma[dc][dr] = label[sc][sr];
    }

    /* the advice columns where the library keeps them, the sigma and Z columns the caller's */
    hsw_region_binding b;
    if ((rc = hsw_gadget_region_binding(g, &b)) != HSW_OK) die("hsw_gadget_region_binding", rc, eng);
    const void *d_cols[MAX_COLS], *d_sigma[MAX_COLS];
    void *d_z[MAX_COLS], *mine[2 * MAX_COLS];
    uint64_t rows[MAX_COLS];
    for (size_t j = 0; j < m; j++) {
        d_cols[j] = (const uint8_t *)b.d_columns + j * b.column_pitch * HSW_CELL_BYTES;
        rows[j] = USABLE;
        if (hipMalloc(&mine[j], sizeof sigma[j]) != 0 || hipMemcpy(mine[j], sigma[j], sizeof sigma[j], 1) != 0) return 1;
        d_sigma[j] = mine[j];
    }
    for (size_t s = 0; s < S; s++) {
        if (hipMalloc(&mine[m + s], (size_t)N_ROWS * HSW_CELL_BYTES) != 0) return 1;
        d_z[s] = mine[m + s];
    }
    const uint64_t beta[4] = {0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull, 0x1000000000000000ull};
    const uint64_t gamma[4] = {0x0123456789abcdefull, 0x1111111111111111ull, 0x2222222222222222ull, 0x0fffffffffffffffull};
    uint32_t status = 0;
    hsw_permutation_product q;
    hsw_permutation_report rep;
    memset(&q, 0, sizeof q);
    q.chunk_columns = CHUNK; q.usable_rows = USABLE; q.n_columns = m;
    q.d_columns = d_cols; q.column_rows = rows; q.d_sigmas = d_sigma; q.d_products = d_z;
    q.betas = beta; q.gammas = gamma; q.omega = &omega; q.delta = &delta; q.status = &status;
    if ((rc = hsw_gadget_permutation_product(g, &q, &rep)) != HSW_OK) die("hsw_gadget_permutation_product", rc, eng);
    printf("%llu proof, %llu products over %zu columns, %llu cells written, open %llu, refused %llu, tiles of %u rows\n",
           (unsigned long long)rep.proofs, (unsigned long long)rep.products, m, (unsigned long long)rep.written,
           (unsigned long long)rep.open_proofs, (unsigned long long)rep.refused_proofs, rep.tile_rows);
    if (rep.written != (USABLE + 1ull) * S || rep.open_proofs || rep.refused_proofs || status != 0) return 1;

    /* the argument's own constraint, on the host.  Both sides of a row carry the same power of 2^-256, so the
     * canonical cells are compared as they are */
    fe be, ga, last = small(1);
    memcpy(&be, beta, 32); memcpy(&ga, gamma, 32);
    for (size_t j = 0; j < m; j++)
        if ((rc = hsw_download(eng, v[j], d_cols[j], sizeof v[j])) != HSW_OK) die("hsw_download", rc, eng);
    for (size_t s = 0; s < S; s++) {
        if ((rc = hsw_download(eng, z, d_z[s], sizeof z)) != HSW_OK) die("hsw_download", rc, eng);
        int ok = memcmp(&z[0], &last, 32) == 0;
        for (uint32_t i = 0; ok && i < USABLE; i++) {
            fe lhs = z[i + 1], rhs = z[i];
            for (size_t j = s * CHUNK; j < m && j < (s + 1) * CHUNK; j++) {
                lhs = mul(lhs, add(add(v[j][i], times(be, sigma[j][i])), ga));
                rhs = mul(rhs, add(add(v[j][i], times(be, label[j][i])), ga));
            }
            ok = memcmp(&lhs, &rhs, 32) == 0;
        }
        printf("chunk %zu: starts where the last one ended and satisfies the recurrence: %s\n", s, ok ? "yes" : "NO");
        if (!ok) return 1;
        last = z[USABLE];
    }
    const fe one = small(1);
    printf("the last value is 1: %s\n", memcmp(&last, &one, 32) == 0 ? "yes" : "NO");
    if (memcmp(&last, &one, 32) != 0) return 1;

    hsw_tie_report trep;
    if ((rc = hsw_gadget_verify_ties(g, &trep)) != HSW_OK) die("hsw_gadget_verify_ties", rc, eng);
    printf("ties checked on the device: %llu pairs, %llu violations\n", (unsigned long long)trep.checks, (unsigned long long)trep.violations);
    if (trep.violations != 0) return 1;
    hsw_gadget_destroy(g);
    for (size_t k = 0; k < m + S; k++) hipFree(mine[k]);
    if ((rc = hsw_device_free(mem)) != HSW_OK) die("hsw_device_free", rc, eng);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
