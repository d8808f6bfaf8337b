/* Plain C99: a grand-product column Z committed in Lagrange form without leaving the device -- halo2's commit_lagrange.
 * The program makes Z with hsw_gadget_permutation_product as examples/ntt_columns.c does (one value column on a domain of
 * 2^10 rows, equal neighbours, a sigma that exchanges their labels), uploads a vector of bases once -- G[j] = (j + 1) * s
 * * (1, 2) for a scalar s of its own, affine, Montgomery form mod q, as halo2curves stores a G1Affine -- and calls
 *   C = hsw_gadget_msm(Z; G)        sum_j Z[j] * G[j] over the USABLE + 1 rows of Z
 * The host then downloads Z and forms the same sum by double-and-add with a small Fq and the complete projective
 * formulas of its own, and compares the 64 bytes.  A real prover passes params.g_lagrange and adds blind * W itself.
 * Build like examples/digest_abc.c, plus -lamdhip64. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

/* the HIP runtime calls this program makes itself (hip_runtime_api.h, which plain C99 -pedantic cannot include) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);      /* kind 1: host to device */

#define K 10
#define N_ROWS (1u << K)
#define USABLE (N_ROWS - 6)        /* the rest are blinding rows: the prover's */

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

/* ---- a prime field on the host, eight 32-bit limbs, Montgomery multiply: Fr to build sigma, Fq for the curve ---- */
typedef struct { uint32_t l[8]; } fe;
typedef struct { fe p, r2; uint32_t np0; } field;
static const field FR = {{{0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
                         {{0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u}}, 0xefffffffu};
static const field FQ = {{{0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
                         {{0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u}}, 0xe4866389u};

static fe reduce_once(const field *f, fe a) {       /* a - p if a >= p (a < 2p) */
    fe d;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)a.l[j] - f->p.l[j] - br;
        d.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    return br ? a : d;
}
static fe add(const field *f, fe a, fe b) {
    uint64_t cy = 0;
    for (int j = 0; j < 8; j++) { cy += (uint64_t)a.l[j] + b.l[j]; a.l[j] = (uint32_t)cy; cy >>= 32; }
    return reduce_once(f, a);
}
static fe sub(const field *f, fe a, fe b) {         /* a + (p - b) */
    fe n;
    uint64_t br = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t x = (uint64_t)f->p.l[j] - b.l[j] - br;
        n.l[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    return add(f, a, reduce_once(f, n));
}
static fe mul(const field *f, fe a, fe b) {         /* a b 2^-256 mod p */
    uint32_t t[10];
    memset(t, 0, sizeof t);
    for (int i = 0; i < 8; i++) {
        uint64_t acc = 0;
        for (int j = 0; j < 8; j++) { acc = (uint64_t)a.l[j] * b.l[i] + t[j] + (acc >> 32); t[j] = (uint32_t)acc; }
        acc = (uint64_t)t[8] + (acc >> 32); t[8] = (uint32_t)acc; t[9] = (uint32_t)(acc >> 32);
        const uint32_t m = t[0] * f->np0;
        acc = (uint64_t)m * f->p.l[0] + t[0];
        for (int j = 1; j < 8; j++) { acc = (uint64_t)m * f->p.l[j] + t[j] + (acc >> 32); t[j - 1] = (uint32_t)acc; }
        acc = (uint64_t)t[8] + (acc >> 32); t[7] = (uint32_t)acc; t[8] = t[9] + (uint32_t)(acc >> 32);
    }
    fe r;
    memcpy(r.l, t, 32);
    return reduce_once(f, r);
}
static fe small(uint32_t x) { fe r; memset(&r, 0, sizeof r); r.l[0] = x; return r; }
static fe times(const field *f, fe a, fe b) { return mul(f, mul(f, a, b), f->r2); }      /* a b, canonical in and out */
static fe power(const field *f, fe a, fe e) {                                             /* a^e, canonical in and out */
    fe r = small(1);
    for (int bit = 255; bit >= 0; bit--) {
        r = times(f, r, r);
        if ((e.l[bit >> 5] >> (bit & 31)) & 1u) r = times(f, r, a);
    }
    return r;
}
static fe root_of_unity(unsigned log_n) {                       /* 7^((p - 1) >> log_n) in Fr */
    fe e = FR.p;
    e.l[0] -= 1;
    for (int j = 0; j < 8; j++) e.l[j] = (e.l[j] >> log_n) | (j < 7 ? e.l[j + 1] << (32 - log_n) : 0);
    return power(&FR, small(7), e);
}

/* ---- G1 on the host: (X : Y : Z) over Fq in Montgomery form, the complete formulas for a = 0, 3 b = 9 ---- */
typedef struct { fe x, y, z; } point;
static fe qa(fe a, fe b) { return add(&FQ, a, b); }
static fe qs(fe a, fe b) { return sub(&FQ, a, b); }
static fe qm(fe a, fe b) { return mul(&FQ, a, b); }
static fe q9(fe a) { fe t = qa(a, a); t = qa(t, t); t = qa(t, t); return qa(t, a); }
static point p_add(point p, point q) {
    fe t0 = qm(p.x, q.x), t1 = qm(p.y, q.y), t2 = qm(p.z, q.z), t3 = qm(qa(p.x, p.y), qa(q.x, q.y)), t4, x3, y3, z3;
    t3 = qs(t3, qa(t0, t1));
    t4 = qs(qm(qa(p.y, p.z), qa(q.y, q.z)), qa(t1, t2));
    y3 = qs(qm(qa(p.x, p.z), qa(q.x, q.z)), qa(t0, t2));
    t0 = qa(qa(t0, t0), t0); t2 = q9(t2);
    z3 = qa(t1, t2); t1 = qs(t1, t2); y3 = q9(y3);
    x3 = qs(qm(t3, t1), qm(t4, y3));
    y3 = qa(qm(t1, z3), qm(y3, t0));
    z3 = qa(qm(z3, t4), qm(t0, t3));
    point r;
    r.x = x3; r.y = y3; r.z = z3;
    return r;
}
static point p_double(point p) { return p_add(p, p); }         /* (complete: the same formula doubles) */
static point p_mul(fe k, point p) {                             /* double-and-add, k canonical */
    point acc;
    acc.x = small(0); acc.y = mul(&FQ, small(1), FQ.r2); acc.z = small(0);
    for (int bit = 255; bit >= 0; bit--) {
        acc = p_double(acc);
        if ((k.l[bit >> 5] >> (bit & 31)) & 1u) acc = p_add(acc, p);
    }
    return acc;
}
static void p_affine(point p, fe out[2]) {                      /* (X / Z, Y / Z) as stored; (0, 0) for the identity */
    fe e = FQ.p, zero = small(0);
    out[0] = out[1] = zero;
    if (memcmp(&p.z, &zero, 32) == 0) return;
    e.l[0] -= 2;
    const fe zi = mul(&FQ, power(&FQ, mul(&FQ, p.z, small(1)), e), FQ.r2);   /* out of Montgomery form, inverted, back in */
    out[0] = qm(p.x, zi);
    out[1] = qm(p.y, zi);
}

static fe label[USABLE], sigma[USABLE], v[USABLE], z[N_ROWS], bases[N_ROWS][2];

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[1] = {64};
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_ex(eng, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);

    /* the domain, one value column with equal neighbours, and the sigma that exchanges them */
    const fe omega = root_of_unity(K), delta = small(7);
    fe w = small(1);
    for (uint32_t i = 0; i < USABLE; i++) { label[i] = w; w = times(&FR, w, omega); }
    for (uint32_t i = 0; i < USABLE; i += 2) {
        v[i] = v[i + 1] = times(&FR, small(i + 3), small(0x9e3779b9u));
        sigma[i] = label[i + 1];
        sigma[i + 1] = label[i];
    }
    /* the bases: G[j] = (j + 1) * s * (1, 2) */
    point gen, step, at;
    gen.x = mul(&FQ, small(1), FQ.r2); gen.y = mul(&FQ, small(2), FQ.r2); gen.z = gen.x;
    step = p_mul(times(&FR, small(0x51ed270bu), small(0x9e3779b9u)), gen);
    at = step;
    for (uint32_t j = 0; j < N_ROWS; j++) { p_affine(at, bases[j]); at = p_add(at, step); }

    void *d_v = NULL, *d_sigma = NULL, *d_z = NULL, *d_bases = NULL;
    if (hipMalloc(&d_v, sizeof v) != 0 || hipMalloc(&d_sigma, sizeof sigma) != 0 || hipMalloc(&d_z, sizeof z) != 0 ||
        hipMalloc(&d_bases, sizeof bases) != 0) return 1;
    if (hipMemcpy(d_v, v, sizeof v, 1) != 0 || hipMemcpy(d_sigma, sigma, sizeof sigma, 1) != 0 || hipMemcpy(d_bases, bases, sizeof bases, 1) != 0) return 1;

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

    /* its commitment, on the device: the USABLE + 1 rows of Z against the first bases */
    const void *scalars[1];
    const uint64_t rows[1] = {USABLE + 1};
    fe commitment[2];
    hsw_msm m;
    hsw_msm_report mrep;
    memset(&m, 0, sizeof m);
    memset(commitment, 0xA5, sizeof commitment);
    scalars[0] = d_z;
    m.n_columns = 1; m.n_bases = N_ROWS; m.d_bases = d_bases; m.d_scalars = scalars; m.input_rows = rows;
    m.out_points = commitment; m.status = &status;
    if ((rc = hsw_gadget_msm(g, &m, &mrep)) != HSW_OK) die("hsw_gadget_msm", rc, eng);
    printf("commit_lagrange(Z): %llu rows, windows of %u bits x %u, %u slice(s) of %u rows, %u launches, refused %llu, bad bases %llu\n",
           (unsigned long long)rows[0], mrep.window_bits, mrep.windows, mrep.slices, mrep.slice_rows, mrep.launches,
           (unsigned long long)mrep.refused_columns, (unsigned long long)mrep.bad_bases);
    if (mrep.refused_columns || mrep.bad_bases || status != 0) return 1;

    /* on the host: Z closes, and the same sum by double-and-add */
    memset(z, 0, sizeof z);
    if ((rc = hsw_download(eng, z, d_z, (USABLE + 1) * sizeof(fe))) != HSW_OK) die("hsw_download", rc, eng);
    const fe one = small(1);
    printf("Z: %u rows, closes: %s, constant: %s\n", USABLE + 1, memcmp(&z[USABLE], &one, 32) == 0 ? "yes" : "NO",
           memcmp(&z[1], &one, 32) == 0 ? "YES" : "no");
    if (memcmp(&z[USABLE], &one, 32) != 0 || memcmp(&z[1], &one, 32) == 0) return 1;
    point sum;
    sum.x = small(0); sum.y = gen.x; sum.z = small(0);
    for (uint32_t j = 0; j <= USABLE; j++) {
        point b;
        b.x = bases[j][0]; b.y = bases[j][1]; b.z = gen.x;
        sum = p_add(sum, p_mul(z[j], b));
    }
    fe want[2];
    p_affine(sum, want);
    const int ok = memcmp(want, commitment, sizeof want) == 0;
    printf("the commitment is sum_j Z[j] * G[j], byte for byte: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;

    hsw_gadget_destroy(g);
    hipFree(d_v); hipFree(d_sigma); hipFree(d_z); hipFree(d_bases);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
