/* Plain C99: a grand-product column Z taken through the three transforms halo2 applies to every column it commits and
 * opens -- lagrange_to_coeff, coeff_to_extended (2 extension bits) and extended_to_coeff -- without leaving the device.
 * The program makes Z with hsw_gadget_permutation_product over one value column of its own on the domain of 2^12 rows:
 * rows 2i and 2i+1 hold the same value and sigma exchanges their labels, so Z closes and is not constant.  Then
 *   coeff    = hsw_gadget_ntt(Z;      omega^-1,     scale 1/n)                        rows beyond USABLE count as 0
 *   extended = hsw_gadget_ntt(coeff;  omega_ext,    shift zeta, input_rows n)         the coset zeta * <omega_ext>
 *   back     = hsw_gadget_ntt(extended; omega_ext^-1, scale 1/4n, shift 1/zeta, HSW_NTT_SHIFT_AFTER)
 * and the host checks, with a small Montgomery multiply of the program's own: the coefficients evaluate to Z at a few
 * points of the domain and to the extended column at a few points of the coset (Horner), and `back` is the coefficients
 * cell for cell with zeros above them.  omega = 7^((p-1)/2^12), omega_ext = 7^((p-1)/2^14) and zeta = 7 are this
 * program's: the library pins no constant (a prover passes its domain's).  Build like examples/digest_abc.c, plus
 * -lamdhip64. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

/* the HIP runtime calls this program makes itself (hip_runtime_api.h, which plain C99 -pedantic cannot include) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);      /* kind 1: host to device */

#define K 12
#define EXT 2
#define N_ROWS (1u << K)           /* cells per polynomial */
#define N_EXT (1u << (K + EXT))
#define USABLE (N_ROWS - 6)        /* the rest are blinding rows: the prover's */

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

/* ---- BN254 Fr on the host, eight 32-bit limbs: just enough to build sigma and to evaluate a polynomial ---- */
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
static fe power(fe a, fe e) {                                   /* a^e, canonical in and out */
    fe r = small(1);
    for (int bit = 255; bit >= 0; bit--) {
        r = times(r, r);
        if ((e.l[bit >> 5] >> (bit & 31)) & 1u) r = times(r, a);
    }
    return r;
}
static fe inverse(fe a) { fe e = P; e.l[0] -= 2; return power(a, e); }
static fe root_of_unity(unsigned log_n) {                       /* 7^((p - 1) >> log_n) */
    fe e = P;
    e.l[0] -= 1;
    for (int j = 0; j < 8; j++) e.l[j] = (e.l[j] >> log_n) | (j < 7 ? e.l[j + 1] << (32 - log_n) : 0);
    return power(small(7), e);
}
static fe horner(const fe *c, size_t n, fe x) {
    fe acc = small(0);
    for (size_t j = n; j-- > 0;) acc = add(times(acc, x), c[j]);
    return acc;
}

static fe label[USABLE], sigma[USABLE], v[USABLE], z[N_ROWS], coeff[N_ROWS], extended[N_EXT], back[N_EXT];

static void transform(hsw_engine *eng, hsw_gadget *g, const char *what, uint32_t log_n, uint32_t flags, const void *in, uint64_t rows, void *out,
                      const fe *omega, const fe *shift, const fe *scale) {
    uint32_t status = 0;
    hsw_ntt q;
    hsw_ntt_report rep;
    memset(&q, 0, sizeof q);
    q.flags = flags; q.log_n = log_n; q.n_columns = 1;
    q.d_inputs = &in; q.input_rows = &rows; q.d_outputs = &out;
    q.omega = omega; q.shift = shift; q.scale = scale; q.status = &status;
    const int rc = hsw_gadget_ntt(g, &q, &rep);
    if (rc != HSW_OK) die("hsw_gadget_ntt", rc, eng);
    printf("%s: 2^%u points, %u launch(es), %llu cells written, refused %llu\n", what, log_n, rep.launches,
           (unsigned long long)rep.written, (unsigned long long)rep.refused_columns);
    if (rep.written != 1ull << log_n || rep.refused_columns || status != 0) exit(1);
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[1] = {64};
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_ex(eng, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);

    /* the domain, one value column with equal neighbours, and the sigma that exchanges them */
    const fe omega = root_of_unity(K), omega_ext = root_of_unity(K + EXT), zeta = small(7), delta = small(7);
    fe w = small(1);
    for (uint32_t i = 0; i < USABLE; i++) { label[i] = w; w = times(w, omega); }
    for (uint32_t i = 0; i < USABLE; i += 2) {
        v[i] = v[i + 1] = times(small(i + 3), small(0x9e3779b9u));
        sigma[i] = label[i + 1];
        sigma[i + 1] = label[i];
    }
    void *d_v = NULL, *d_sigma = NULL, *d_z = NULL, *d_coeff = NULL, *d_ext = NULL, *d_back = NULL;
    if (hipMalloc(&d_v, sizeof v) != 0 || hipMalloc(&d_sigma, sizeof sigma) != 0 || hipMalloc(&d_z, sizeof z) != 0 ||
        hipMalloc(&d_coeff, sizeof coeff) != 0 || hipMalloc(&d_ext, sizeof extended) != 0 || hipMalloc(&d_back, sizeof back) != 0) return 1;
    if (hipMemcpy(d_v, v, sizeof v, 1) != 0 || hipMemcpy(d_sigma, sigma, sizeof sigma, 1) != 0) return 1;

    /* Z on the device */
    const uint64_t beta[4] = {0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull, 0x1000000000000000ull};
    const uint64_t gamma[4] = {0x0123456789abcdefull, 0x1111111111111111ull, 0x2222222222222222ull, 0x0fffffffffffffffull};
    const void *cols[1], *sigmas[1];
    void *products[1];
    uint32_t status = 0;
    hsw_permutation_product q;
    hsw_permutation_report prep;
    memset(&q, 0, sizeof q);
    cols[0] = d_v; sigmas[0] = d_sigma; products[0] = d_z;
    q.chunk_columns = 1; q.usable_rows = USABLE; q.n_columns = 1;
    q.d_columns = cols; q.d_sigmas = sigmas; q.d_products = products;
    q.betas = beta; q.gammas = gamma; q.omega = &omega; q.delta = &delta; q.status = &status;
    if ((rc = hsw_gadget_permutation_product(g, &q, &prep)) != HSW_OK) die("hsw_gadget_permutation_product", rc, eng);
    if (prep.open_proofs || prep.refused_proofs || status != 0) return 1;
    memset(z, 0, sizeof z);
    if ((rc = hsw_download(eng, z, d_z, (USABLE + 1) * sizeof(fe))) != HSW_OK) die("hsw_download", rc, eng);
    const fe one = small(1);
    printf("Z: %u rows, closes: %s, constant: %s\n", USABLE + 1, memcmp(&z[USABLE], &one, 32) == 0 ? "yes" : "NO",
           memcmp(&z[1], &one, 32) == 0 ? "YES" : "no");
    if (memcmp(&z[USABLE], &one, 32) != 0 || memcmp(&z[1], &one, 32) == 0) return 1;

    /* the three transforms, on the device */
    const fe omega_inv = inverse(omega), omega_ext_inv = inverse(omega_ext), zeta_inv = inverse(zeta);
    const fe n_inv = inverse(small(N_ROWS)), n_ext_inv = inverse(small(N_EXT));
    transform(eng, g, "lagrange_to_coeff", K, 0, d_z, USABLE + 1, d_coeff, &omega_inv, NULL, &n_inv);
    transform(eng, g, "coeff_to_extended", K + EXT, 0, d_coeff, N_ROWS, d_ext, &omega_ext, &zeta, NULL);
    transform(eng, g, "extended_to_coeff", K + EXT, HSW_NTT_SHIFT_AFTER, d_ext, N_EXT, d_back, &omega_ext_inv, &zeta_inv, &n_ext_inv);
    if ((rc = hsw_download(eng, coeff, d_coeff, sizeof coeff)) != HSW_OK || (rc = hsw_download(eng, extended, d_ext, sizeof extended)) != HSW_OK ||
        (rc = hsw_download(eng, back, d_back, sizeof back)) != HSW_OK) die("hsw_download", rc, eng);

    /* on the host: the coefficients at points of the domain and of the coset, and the round trip */
    const uint32_t rows[6] = {0, 1, 2, USABLE - 1, USABLE, N_ROWS - 1}, ext_rows[5] = {0, 1, 5, N_EXT / 2 + 3, N_EXT - 1};
    int ok = 1;
    for (int k = 0; k < 6; k++) {
        fe e = small(rows[k]);
        const fe at = horner(coeff, N_ROWS, power(omega, e));
        ok = ok && memcmp(&at, &z[rows[k]], 32) == 0;
    }
    printf("the coefficients evaluate to Z on the domain (0 on the blinding rows): %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;
    for (int k = 0; k < 5; k++) {
        fe e = small(ext_rows[k]);
        const fe at = horner(coeff, N_ROWS, times(zeta, power(omega_ext, e)));
        ok = ok && memcmp(&at, &extended[ext_rows[k]], 32) == 0;
    }
    printf("the extended column is the polynomial on the coset: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;
    ok = memcmp(back, coeff, sizeof coeff) == 0;
    for (uint32_t i = N_ROWS; ok && i < N_EXT; i++)
        for (int j = 0; j < 8; j++) ok = ok && back[i].l[j] == 0;
    printf("extended_to_coeff returns the coefficients cell for cell, zeros above them: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;

    hsw_gadget_destroy(g);
    hipFree(d_v); hipFree(d_sigma); hipFree(d_z); hipFree(d_coeff); hipFree(d_ext); hipFree(d_back);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
