/* Plain C99: four committed columns opened with SHPLONK without leaving the device -- what halo2's create_proof does
 * after the evaluations, with ProverSHPLONK as the multi-opening.  Four columns in Lagrange form on a domain of 2^10 rows
 * (values of this program's own) are uploaded once; then, on the device,
 *   coeff = hsw_gadget_ntt(columns; omega^-1, scale 1/n)                        lagrange_to_coeff
 *   h     = hsw_gadget_shplonk_quotient(coeff; three rotation sets; y, v)       sum_i v^i floor(c_i / Z_i)
 *   H     = hsw_gadget_msm(h; G)                                                its commitment, n_bases = rows
 *   w     = hsw_gadget_shplonk_open(coeff, h; the same sets; y, v, u)           (L(X) - L(u)) / ((X - u) zd_0)
 *   W     = hsw_gadget_msm(w; G)
 * over the super point set T = {x, x omega, x omega^-1}: columns {0, 1} are queried at {x}, column 2 at {x, x omega} and
 * column 3 at all three.  The host downloads the coefficients, h and w and checks every cell with a small Montgomery
 * multiply of its own, by the definition: the fold with y, SUCCESSIVE Kate division root after root, the fold with v;
 * then L and the division by (X - u).  omega = 7^((p-1)/2^10), x, y, v, u and the bases G[j] = (j + 1) * s * (1, 2) are
 * this program's: the library pins no constant.  A real prover passes params.g, draws the challenges from its
 * transcript (u after it has written H) and adds the blinding terms itself.  Build like examples/digest_abc.c, plus
 * -lamdhip64. */
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
#define COLS 4

static void die(const char *what, int rc, const hsw_engine *e) {
    fprintf(stderr, "%s: %s (%s)\n", what, hsw_strerror(rc), e ? hsw_last_error(e) : "");
    exit(1);
}

/* ---- a prime field on the host, eight 32-bit limbs, Montgomery multiply: Fr for the columns, Fq for the curve ---- */
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
static fe inverse(fe a) { fe e = FR.p; e.l[0] -= 2; return power(&FR, a, e); }
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
static point p_mul(fe k, point p) {                             /* double-and-add, k canonical */
    point acc;
    acc.x = small(0); acc.y = mul(&FQ, small(1), FQ.r2); acc.z = small(0);
    for (int bit = 255; bit >= 0; bit--) {
        acc = p_add(acc, acc);                                  /* (complete: the same formula doubles) */
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
static void print_point(const char *name, const fe pt[2]) {
    printf("%s = (0x", name);
    for (int j = 7; j >= 0; j--) printf("%08x", pt[0].l[j]);
    printf(", 0x");
    for (int j = 7; j >= 0; j--) printf("%08x", pt[1].l[j]);
    printf(")  [Montgomery form mod q]\n");
}

static fe lagrange[COLS][N_ROWS], coeff[COLS][N_ROWS], h_cells[N_ROWS], w_cells[N_ROWS], bases[N_ROWS][2];
static fe fold[3][N_ROWS], want_h[N_ROWS], lin[N_ROWS];

/* q[j-1] = c[j] + z q[j], q[n-1] = 0, in place: floor(c(X) / (X - z)) */
static void kate(fe *c, size_t n, fe z) {
    fe s = small(0);
    for (size_t j = n; j-- > 0;) {
        const fe cj = c[j];
        c[j] = s;
        s = add(&FR, cj, times(&FR, z, s));
    }
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[1] = {64};
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_ex(eng, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);

    /* four columns in Lagrange form (zero on the blinding rows) and the bases G[j] = (j + 1) * s * (1, 2) */
    memset(lagrange, 0, sizeof lagrange);
    for (uint32_t b = 0; b < COLS; b++)
        for (uint32_t i = 0; i < USABLE; i++) lagrange[b][i] = times(&FR, small(i * COLS + b + 3), small(0x9e3779b9u + b));
    point gen, step, at;
    gen.x = mul(&FQ, small(1), FQ.r2); gen.y = mul(&FQ, small(2), FQ.r2); gen.z = gen.x;
    step = p_mul(times(&FR, small(0x51ed270bu), small(0x9e3779b9u)), gen);
    at = step;
    for (uint32_t j = 0; j < N_ROWS; j++) { p_affine(at, bases[j]); at = p_add(at, step); }
    void *d_lagrange = NULL, *d_coeff = NULL, *d_h = NULL, *d_w = NULL, *d_bases = NULL;
    if (hipMalloc(&d_lagrange, sizeof lagrange) != 0 || hipMalloc(&d_coeff, sizeof coeff) != 0 || hipMalloc(&d_h, sizeof h_cells) != 0 ||
        hipMalloc(&d_w, sizeof w_cells) != 0 || hipMalloc(&d_bases, sizeof bases) != 0) return 1;
    if (hipMemcpy(d_lagrange, lagrange, sizeof lagrange, 1) != 0 || hipMemcpy(d_bases, bases, sizeof bases, 1) != 0) return 1;
    const void *d_in[COLS], *d_co[COLS];
    void *d_out[COLS];
    for (uint32_t b = 0; b < COLS; b++) {
        d_in[b] = (const uint8_t *)d_lagrange + b * sizeof lagrange[0];
        d_co[b] = d_out[b] = (uint8_t *)d_coeff + b * sizeof coeff[0];
    }

    /* lagrange_to_coeff, on the device */
    const fe omega = root_of_unity(K), omega_inv = inverse(omega), n_inv = inverse(small(N_ROWS));
    uint32_t status[COLS] = {0, 0, 0, 0};
    hsw_ntt t;
    hsw_ntt_report trep;
    memset(&t, 0, sizeof t);
    t.log_n = K; t.n_columns = COLS; t.d_inputs = d_in; t.d_outputs = d_out; t.omega = &omega_inv; t.scale = &n_inv; t.status = status;
    if ((rc = hsw_gadget_ntt(g, &t, &trep)) != HSW_OK) die("hsw_gadget_ntt", rc, eng);
    printf("lagrange_to_coeff: %llu columns of 2^%u points, refused %llu\n", (unsigned long long)trep.columns, K, (unsigned long long)trep.refused_columns);
    if (trep.refused_columns) return 1;

    /* the rotation sets over T = {x, x omega, x omega^-1} */
    const fe x = times(&FR, small(0x6b8b4567u), small(0x327b23c6u)), y = times(&FR, small(0x643c9869u), small(0x66334873u));
    const fe v = times(&FR, small(0x74b0dc51u), small(0x19495cffu)), u = times(&FR, small(0x2ae8944au), small(0x625558ecu));
    fe T[3];
    T[0] = x; T[1] = times(&FR, x, omega); T[2] = times(&FR, x, omega_inv);
    const uint64_t set_first[4] = {0, 2, 3, 4}, set_point_first[4] = {0, 1, 3, 6};
    const uint32_t set_columns[4] = {0, 1, 2, 3}, set_points[6] = {0, 0, 1, 0, 1, 2};
    uint32_t word = 0;
    hsw_shplonk sp;
    hsw_shplonk_report srep;
    memset(&sp, 0, sizeof sp);
    sp.rows = N_ROWS; sp.n_columns = COLS; sp.d_columns = d_co; sp.n_points = 3; sp.points = T; sp.n_sets = 3;
    sp.set_first = set_first; sp.set_columns = set_columns; sp.set_point_first = set_point_first; sp.set_points = set_points;
    sp.y = &y; sp.v = &v; sp.d_out = d_h; sp.status = &word;
    if ((rc = hsw_gadget_shplonk_quotient(g, &sp, &srep)) != HSW_OK) die("hsw_gadget_shplonk_quotient", rc, eng);
    printf("shplonk quotient: %llu sets, %llu (set, point) items, %llu cells written, %u launches, refused %llu\n", (unsigned long long)srep.sets,
           (unsigned long long)srep.items, (unsigned long long)srep.written, srep.launches, (unsigned long long)srep.refused);
    if (srep.refused) return 1;

    /* H = commit(h), on the device; a prover writes it to the transcript and squeezes u */
    const void *scalars[1];
    fe commitment[2][2];
    hsw_msm m;
    hsw_msm_report mrep;
    memset(&m, 0, sizeof m);
    scalars[0] = d_h;
    m.n_columns = 1; m.n_bases = N_ROWS; m.d_bases = d_bases; m.d_scalars = scalars; m.out_points = commitment[0]; m.status = status;
    if ((rc = hsw_gadget_msm(g, &m, &mrep)) != HSW_OK) die("hsw_gadget_msm", rc, eng);
    if (mrep.refused_columns || mrep.bad_bases) return 1;
    print_point("H", commitment[0]);

    sp.u = &u; sp.d_h = d_h; sp.d_out = d_w;
    if ((rc = hsw_gadget_shplonk_open(g, &sp, &srep)) != HSW_OK) die("hsw_gadget_shplonk_open", rc, eng);
    printf("shplonk open: %llu columns with h, %llu cells written, %u launches, refused %llu\n", (unsigned long long)srep.columns,
           (unsigned long long)srep.written, srep.launches, (unsigned long long)srep.refused);
    if (srep.refused) return 1;
    scalars[0] = d_w;
    m.out_points = commitment[1];
    if ((rc = hsw_gadget_msm(g, &m, &mrep)) != HSW_OK) die("hsw_gadget_msm", rc, eng);
    if (mrep.refused_columns || mrep.bad_bases) return 1;
    print_point("W", commitment[1]);

    /* on the host: every cell, by the definition */
    if ((rc = hsw_download(eng, coeff, d_coeff, sizeof coeff)) != HSW_OK || (rc = hsw_download(eng, h_cells, d_h, sizeof h_cells)) != HSW_OK ||
        (rc = hsw_download(eng, w_cells, d_w, sizeof w_cells)) != HSW_OK)
        die("hsw_download", rc, eng);
    fe vi = small(1), zd[3], zt = small(1);
    memset(want_h, 0, sizeof want_h);
    memset(lin, 0, sizeof lin);
    for (int i = 0; i < 3; i++) {
        fe yk = small(1);
        memset(fold[i], 0, sizeof fold[i]);
        for (uint64_t k = set_first[i]; k < set_first[i + 1]; k++) {          /* c_i = sum_k y^k a_k: the first column gets y^0 */
            for (uint32_t j = 0; j < N_ROWS; j++) fold[i][j] = add(&FR, fold[i][j], times(&FR, yk, coeff[set_columns[k]][j]));
            yk = times(&FR, yk, y);
        }
        memcpy(lin, fold[i], sizeof lin);                                     /* (scratch: the quotient of this set) */
        zd[i] = small(1);
        for (uint32_t p = 0; p < 3; p++) {                                    /* zd_i: the points of T that are not in the set */
            int in_set = 0;
            for (uint64_t k = set_point_first[i]; k < set_point_first[i + 1]; k++) in_set = in_set || set_points[k] == p;
            if (!in_set) zd[i] = times(&FR, zd[i], sub(&FR, u, T[p]));
        }
        for (uint64_t k = set_point_first[i]; k < set_point_first[i + 1]; k++) kate(lin, N_ROWS, T[set_points[k]]);   /* root after root */
        for (uint32_t j = 0; j < N_ROWS; j++) want_h[j] = add(&FR, want_h[j], times(&FR, vi, lin[j]));
        vi = times(&FR, vi, v);
    }
    int ok = memcmp(want_h, h_cells, sizeof want_h) == 0;
    printf("h is sum_i v^i floor(c_i / Z_i) by successive division, cell for cell: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;
    for (uint32_t p = 0; p < 3; p++) zt = times(&FR, zt, sub(&FR, u, T[p]));
    vi = small(1);
    for (uint32_t j = 0; j < N_ROWS; j++) lin[j] = sub(&FR, small(0), times(&FR, zt, h_cells[j]));
    for (int i = 0; i < 3; i++) {
        const fe wgt = times(&FR, vi, zd[i]);
        for (uint32_t j = 0; j < N_ROWS; j++) lin[j] = add(&FR, lin[j], times(&FR, wgt, fold[i][j]));
        vi = times(&FR, vi, v);
    }
    kate(lin, N_ROWS, u);
    const fe zd0_inv = inverse(zd[0]);
    for (uint32_t j = 0; j < N_ROWS; j++) lin[j] = times(&FR, lin[j], zd0_inv);
    const fe zero = small(0);
    ok = memcmp(lin, w_cells, sizeof lin) == 0 && memcmp(&w_cells[N_ROWS - 1], &zero, 32) == 0 && memcmp(&h_cells[N_ROWS - 1], &zero, 32) == 0;
    printf("w is (L(X) - L(u)) / ((X - u) zd_0), cell for cell, and the top cells are zero: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;

    hsw_gadget_destroy(g);
    hipFree(d_lagrange); hipFree(d_coeff); hipFree(d_h); hipFree(d_w); hipFree(d_bases);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
