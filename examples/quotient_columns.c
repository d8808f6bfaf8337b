/* Plain C99: the quotient polynomial h(X) of a small circuit without leaving the device -- what halo2's create_proof
 * does between its last grand product and the commitments of h.  A satisfied toy circuit of 2^4 rows (10 usable) is built
 * on the host in Lagrange form: two advice columns that carry the FlexGate gate q (a + b c - d) under a selector each, a
 * third advice column, a permutation over the three (sets of 2 columns: S = 2) with a few copy constraints, a lookup
 * of one input in one table column and one of two in two, the grand products Z and the permuted pairs A', S' by their
 * recurrences, random cells in the blinding rows.  All 24 columns are uploaded once; then, on the device,
 *   coeff = hsw_gadget_ntt(columns; omega^-1, scale 1/n)                       lagrange_to_coeff
 *   ext   = hsw_gadget_ntt(coeff; omega_ext, shift zeta, input_rows n)         coeff_to_extended, N = 2^6
 *   h_ext = hsw_gadget_quotient(ext; the gates, the permutation, the lookups)  evaluate_h and the division by X^n - 1
 *   h     = hsw_gadget_ntt(h_ext; omega_ext^-1, shift 1/zeta after, scale 1/N) extended_to_coeff, in place
 *   C_k   = hsw_gadget_msm(h[k n .. (k + 1) n); G)                             the commitments of the three pieces of h
 * The host downloads the coefficients and checks, with a small Montgomery multiply of its own: every coefficient of h
 * at and beyond 3 n is zero (the circuit is satisfied), the folded expressions at a point x equal h(x) (x^n - 1), and
 * C_0 is sum_j h[j] * G[j] by double-and-add.  omega, zeta, delta = 7, the challenges and the bases are this program's:
 * the library pins no constant; a real prover draws theta, beta, gamma, y and x from its transcript.  Build like
 * examples/digest_abc.c, plus -lamdhip64. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsw.h"

/* the HIP runtime calls this program makes itself (hip_runtime_api.h, which plain C99 -pedantic cannot include) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);      /* kind 1: host to device */

#define K 4
#define N_ROWS (1u << K)           /* n: the rows of the circuit */
#define USABLE 10u                 /* u: the rest are blinding rows */
#define EXT 2                      /* e: the extended coset has N = 2^(K + e) rows, enough for degree 4 */
#define N_EXT (N_ROWS << EXT)
#define COLS 24
#define PIECES 3                   /* h has degree below (4 - 1) n */

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
static fe horner(const fe *c, size_t n, fe x) {
    fe acc = small(0);
    for (size_t j = n; j-- > 0;) acc = add(&FR, times(&FR, acc, x), c[j]);
    return acc;
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


enum { A0, A1, A2, Q0, Q1, T1, T2A, T2B, LKA, LKB, SG0, SG1, SG2, PZ0, PZ1, L1A, L1S, L1Z, L2A, L2S, L2Z, L0, LLAST, LACTIVE };
static fe lagrange[COLS][N_ROWS], coeff[COLS][N_ROWS], h_coeff[N_EXT], bases[N_ROWS][2];

static uint32_t lcg_state = 0x2545f491u;
static uint32_t lcg(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 4; }
static fe rnd(void) { return times(&FR, times(&FR, small(lcg()), small(lcg())), times(&FR, small(lcg()), small(lcg()))); }
static fe mul_add(fe a, fe b, fe c) { return add(&FR, times(&FR, a, b), c); }                /* a b + c */
static int less(fe a, fe b) {
    for (int j = 7; j >= 0; j--) if (a.l[j] != b.l[j]) return a.l[j] < b.l[j];
    return 0;
}
static int same(fe a, fe b) { return memcmp(&a, &b, 32) == 0; }

/* one lookup argument of the toy circuit: A and T compressed on the usable rows; A' sorted, S' a permutation of T with
 * S'[i] = A'[i] wherever A' changes, Z by its recurrence; random cells in the blinding rows */
static void lookup_columns(const fe *A, const fe *T, fe beta, fe gamma, fe *Ap, fe *Sp, fe *Z) {
    int used[USABLE], filled[USABLE];
    memset(used, 0, sizeof used); memset(filled, 0, sizeof filled);
    for (uint32_t i = 0; i < USABLE; i++) {                     /* insertion sort */
        uint32_t k = i;
        while (k > 0 && less(A[i], Ap[k - 1])) { Ap[k] = Ap[k - 1]; k--; }
        Ap[k] = A[i];
    }
    for (uint32_t i = 0; i < USABLE; i++) {
        if (i && same(Ap[i], Ap[i - 1])) continue;
        for (uint32_t k = 0; k < USABLE; k++)
            if (!used[k] && same(T[k], Ap[i])) { used[k] = 1; Sp[i] = Ap[i]; filled[i] = 1; break; }
        if (!filled[i]) { fprintf(stderr, "the toy circuit's lookup input is not in its table\n"); exit(1); }
    }
    for (uint32_t i = 0, k = 0; i < USABLE; i++) {
        if (filled[i]) continue;
        while (used[k]) k++;
        Sp[i] = T[k]; used[k] = 1;
    }
    Z[0] = small(1);
    for (uint32_t i = 0; i < USABLE; i++) {
        const fe num = times(&FR, add(&FR, A[i], beta), add(&FR, T[i], gamma)), den = times(&FR, add(&FR, Ap[i], beta), add(&FR, Sp[i], gamma));
        Z[i + 1] = times(&FR, Z[i], times(&FR, num, inverse(den)));
    }
    for (uint32_t i = USABLE; i < N_ROWS; i++) { Ap[i] = rnd(); Sp[i] = rnd(); if (i > USABLE) Z[i] = rnd(); }
}

int main(void) {
    hsw_engine *eng = NULL;
    int rc = hsw_engine_create_ex(0, NULL, 8, 2, HSW_MODE_HALO2_INTERNALS, &eng);
    if (rc != HSW_OK) die("hsw_engine_create_ex", rc, NULL);
    size_t sizes[1] = {64};
    hsw_gadget *g = NULL;
    if ((rc = hsw_gadget_create_ex(eng, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g)) != HSW_OK) die("hsw_gadget_create_ex", rc, eng);

    /* ---- the circuit, in Lagrange form ---- */
    const fe omega = root_of_unity(K), w = root_of_unity(K + EXT), delta = small(7), zeta = small(5);
    const fe theta = rnd(), beta = rnd(), gamma = rnd(), y = rnd();
    memset(lagrange, 0, sizeof lagrange);
    for (int k = 0; k < 2; k++)
        for (uint32_t r = 0; r + 3 < USABLE; r += 4) {
            fe *a = lagrange[A0 + k] + r;
            a[0] = rnd(); a[1] = rnd(); a[2] = rnd(); a[3] = mul_add(a[1], a[2], a[0]);
            lagrange[Q0 + k][r] = small(1);
        }
    for (uint32_t i = 0; i < N_ROWS; i++) {
        const uint32_t j = lcg() % 5;
        lagrange[T1][i] = small(i % 6); lagrange[T2A][i] = small(i % 5 + 100); lagrange[T2B][i] = small((i % 5) * (i % 5) + 7);
        lagrange[A2][i] = small(lcg() % 6);
        lagrange[LKA][i] = small(j + 100); lagrange[LKB][i] = small(j * j + 7);
    }
    /* copy constraints: cells joined in cycles; the gates of the rows they touch are made to hold again */
    {
        fe (*a)[N_ROWS] = lagrange;
        a[A1][0] = a[A0][3]; a[A1][3] = mul_add(a[A1][1], a[A1][2], a[A1][0]);
        a[A2][1] = a[A2][5] = a[A2][7];
        a[A0][4] = a[A0][0]; a[A0][7] = mul_add(a[A0][5], a[A0][6], a[A0][4]);
    }
    fe label[3][N_ROWS];
    for (int j = 0; j < 3; j++) {
        fe l = j == 0 ? small(1) : j == 1 ? delta : times(&FR, delta, delta);
        for (uint32_t i = 0; i < N_ROWS; i++) { label[j][i] = lagrange[SG0 + j][i] = l; l = times(&FR, l, omega); }
    }
    {
        const int cycles[3][3][2] = {{{0, 3}, {1, 0}, {-1, 0}}, {{2, 1}, {2, 5}, {2, 7}}, {{0, 0}, {0, 4}, {-1, 0}}};
        for (int c = 0; c < 3; c++) {
            const int len = cycles[c][2][0] < 0 ? 2 : 3;
            for (int k = 0; k < len; k++) {
                const int *from = cycles[c][k], *to = cycles[c][(k + 1) % len];
                lagrange[SG0 + from[0]][from[1]] = label[to[0]][to[1]];
            }
        }
    }
    for (int j = 0; j < 3; j++)
        for (uint32_t i = USABLE; i < N_ROWS; i++) lagrange[A0 + j][i] = rnd();
    {   /* the permutation's grand products over sets of 2 columns */
        fe last = small(1);
        for (int s = 0; s < 2; s++) {
            fe *Z = lagrange[PZ0 + s];
            Z[0] = last;
            for (uint32_t i = 0; i < USABLE; i++) {
                fe num = small(1), den = small(1);
                for (int j = 2 * s; j < 3 && j < 2 * s + 2; j++) {
                    const fe v = lagrange[A0 + j][i];
                    num = times(&FR, num, add(&FR, mul_add(beta, label[j][i], v), gamma));
                    den = times(&FR, den, add(&FR, mul_add(beta, lagrange[SG0 + j][i], v), gamma));
                }
                Z[i + 1] = times(&FR, Z[i], times(&FR, num, inverse(den)));
            }
            last = Z[USABLE];
            for (uint32_t i = USABLE + 1; i < N_ROWS; i++) Z[i] = rnd();
        }
        if (!same(last, small(1))) { fprintf(stderr, "the toy circuit's permutation does not close\n"); return 1; }
    }
    {   /* the lookups */
        fe A[N_ROWS], T[N_ROWS];
        lookup_columns(lagrange[A2], lagrange[T1], beta, gamma, lagrange[L1A], lagrange[L1S], lagrange[L1Z]);
        for (uint32_t i = 0; i < N_ROWS; i++) { A[i] = mul_add(lagrange[LKA][i], theta, lagrange[LKB][i]); T[i] = mul_add(lagrange[T2A][i], theta, lagrange[T2B][i]); }
        lookup_columns(A, T, beta, gamma, lagrange[L2A], lagrange[L2S], lagrange[L2Z]);
        if (!same(lagrange[L1Z][USABLE], small(1)) || !same(lagrange[L2Z][USABLE], small(1))) { fprintf(stderr, "a lookup's Z does not close\n"); return 1; }
    }
    lagrange[L0][0] = small(1); lagrange[LLAST][USABLE] = small(1);
    for (uint32_t i = 0; i < USABLE; i++) lagrange[LACTIVE][i] = small(1);
    /* the bases G[j] = (j + 1) * s * (1, 2) */
    point gen, step, at;
    gen.x = mul(&FQ, small(1), FQ.r2); gen.y = mul(&FQ, small(2), FQ.r2); gen.z = gen.x;
    step = p_mul(times(&FR, small(0x51ed270bu), small(0x9e3779b9u)), gen);
    at = step;
    for (uint32_t j = 0; j < N_ROWS; j++) { p_affine(at, bases[j]); at = p_add(at, step); }

    /* ---- on the device ---- */
    void *d_lagrange = NULL, *d_coeff = NULL, *d_ext = NULL, *d_h = NULL, *d_bases = NULL;
    const size_t ext_bytes = (size_t)N_EXT * 32;
    if (hipMalloc(&d_lagrange, sizeof lagrange) != 0 || hipMalloc(&d_coeff, sizeof coeff) != 0 || hipMalloc(&d_ext, COLS * ext_bytes) != 0 ||
        hipMalloc(&d_h, ext_bytes) != 0 || hipMalloc(&d_bases, sizeof bases) != 0) return 1;
    if (hipMemcpy(d_lagrange, lagrange, sizeof lagrange, 1) != 0 || hipMemcpy(d_bases, bases, sizeof bases, 1) != 0) return 1;
    const void *d_in[COLS], *d_co[COLS], *d_x[COLS];
    void *d_out[COLS], *d_xo[COLS];
    uint64_t base_rows[COLS];
    uint32_t status[COLS];
    for (uint32_t b = 0; b < COLS; b++) {
        d_in[b] = (const uint8_t *)d_lagrange + b * sizeof lagrange[0];
        d_co[b] = d_out[b] = (uint8_t *)d_coeff + b * sizeof coeff[0];
        d_x[b] = d_xo[b] = (uint8_t *)d_ext + b * ext_bytes;
        base_rows[b] = N_ROWS;
    }
    const fe omega_inv = inverse(omega), n_inv = inverse(small(N_ROWS)), w_inv = inverse(w), zeta_inv = inverse(zeta), n_ext_inv = inverse(small(N_EXT));
    hsw_ntt t;
    hsw_ntt_report trep;
    memset(&t, 0, sizeof t);
    t.log_n = K; t.n_columns = COLS; t.d_inputs = d_in; t.d_outputs = d_out; t.omega = &omega_inv; t.scale = &n_inv; t.status = status;
    if ((rc = hsw_gadget_ntt(g, &t, &trep)) != HSW_OK) die("hsw_gadget_ntt", rc, eng);
    printf("lagrange_to_coeff: %llu columns of 2^%u points, refused %llu\n", (unsigned long long)trep.columns, K, (unsigned long long)trep.refused_columns);
    if (trep.refused_columns) return 1;
    memset(&t, 0, sizeof t);
    t.log_n = K + EXT; t.n_columns = COLS; t.d_inputs = d_co; t.input_rows = base_rows; t.d_outputs = d_xo; t.omega = &w; t.shift = &zeta; t.status = status;
    if ((rc = hsw_gadget_ntt(g, &t, &trep)) != HSW_OK) die("hsw_gadget_ntt", rc, eng);
    printf("coeff_to_extended: %llu columns of 2^%u points, refused %llu\n", (unsigned long long)trep.columns, K + EXT, (unsigned long long)trep.refused_columns);
    if (trep.refused_columns) return 1;

    /* the quotient: the two gates as monomials +1 q a(0), +1 q b(1) c(2), (p - 1) q d(3); columns 0 .. 2 the proof's own,
     * 3 .. 9 the shared ones */
    fe minus_one = FR.p;
    minus_one.l[0] -= 1;
    fe coeffs[6];
    const uint32_t gate_first_term[3] = {0, 3, 6}, term_first_factor[7] = {0, 2, 5, 7, 9, 12, 14};
    const uint32_t factor_column[14] = {Q0, A0, Q0, A0, A0, Q0, A0, Q1, A1, Q1, A1, A1, Q1, A1};
    const int32_t factor_rotation[14] = {0, 0, 0, 1, 2, 0, 3, 0, 0, 0, 1, 2, 0, 3};
    for (int k = 0; k < 2; k++) { coeffs[3 * k] = coeffs[3 * k + 1] = small(1); coeffs[3 * k + 2] = minus_one; }
    const uint32_t perm_columns[3] = {A0, A1, A2}, first_input[3] = {0, 1, 3}, inputs[3] = {A2, LKA, LKB}, first_table[3] = {0, 1, 3}, tables[3] = {T1, T2A, T2B};
    const void *fixed[7], *sigmas[3], *pz[2], *lk_a[2], *lk_s[2], *lk_z[2];
    for (int j = 0; j < 7; j++) fixed[j] = d_x[Q0 + j];
    for (int j = 0; j < 3; j++) sigmas[j] = d_x[SG0 + j];
    pz[0] = d_x[PZ0]; pz[1] = d_x[PZ1];
    lk_a[0] = d_x[L1A]; lk_s[0] = d_x[L1S]; lk_z[0] = d_x[L1Z]; lk_a[1] = d_x[L2A]; lk_s[1] = d_x[L2S]; lk_z[1] = d_x[L2Z];
    void *h_out[1];
    uint32_t qstatus[1] = {0};
    h_out[0] = d_h;
    hsw_quotient q;
    hsw_quotient_report qrep;
    memset(&q, 0, sizeof q);
    q.log_rows = K; q.log_n = K + EXT; q.chunk_columns = 2; q.usable_rows = USABLE;
    q.n_proofs = 1; q.n_columns = 3; q.n_fixed = 7; q.d_columns = d_x; q.d_fixed = fixed;
    q.d_l0 = d_x[L0]; q.d_l_last = d_x[LLAST]; q.d_l_active = d_x[LACTIVE];
    q.gates.n_gates = 2; q.gates.n_terms = 6; q.gates.n_factors = 14; q.gates.gate_first_term = gate_first_term; q.gates.term_coeffs = coeffs;
    q.gates.term_first_factor = term_first_factor; q.gates.factor_column = factor_column; q.gates.factor_rotation = factor_rotation;
    q.n_perm_columns = 3; q.perm_columns = perm_columns; q.d_sigmas = sigmas; q.d_perm_products = pz;
    q.lookups.n_lookups = 2; q.lookups.first_input = first_input; q.lookups.inputs = inputs; q.lookups.first_table = first_table; q.lookups.tables = tables;
    q.lookups.d_permuted_inputs = lk_a; q.lookups.d_permuted_tables = lk_s; q.lookups.d_products = lk_z; q.lookups.thetas = &theta;
    q.betas = &beta; q.gammas = &gamma; q.ys = &y; q.omega_ext = &w; q.zeta = &zeta; q.delta = &delta;
    q.d_h = h_out; q.status = qstatus;
    if ((rc = hsw_gadget_quotient(g, &q, &qrep)) != HSW_OK) die("hsw_gadget_quotient", rc, eng);
    printf("quotient: %llu proof, %llu expressions, %llu cells written, %u launches, refused %llu\n", (unsigned long long)qrep.proofs,
           (unsigned long long)qrep.expressions, (unsigned long long)qrep.written, qrep.launches, (unsigned long long)qrep.refused_proofs);
    if (qrep.refused_proofs) return 1;

    /* extended_to_coeff, in place */
    const void *h_in[1];
    h_in[0] = d_h;
    memset(&t, 0, sizeof t);
    t.flags = HSW_NTT_SHIFT_AFTER; t.log_n = K + EXT; t.n_columns = 1; t.d_inputs = h_in; t.d_outputs = h_out; t.omega = &w_inv; t.shift = &zeta_inv;
    t.scale = &n_ext_inv; t.status = status;
    if ((rc = hsw_gadget_ntt(g, &t, &trep)) != HSW_OK) die("hsw_gadget_ntt", rc, eng);
    printf("extended_to_coeff: %llu column of 2^%u points, refused %llu\n", (unsigned long long)trep.columns, K + EXT, (unsigned long long)trep.refused_columns);
    if (trep.refused_columns) return 1;

    /* the commitments of the pieces of h */
    const void *scalars[PIECES];
    fe commitment[PIECES][2];
    uint32_t mstatus[PIECES];
    hsw_msm m;
    hsw_msm_report mrep;
    memset(&m, 0, sizeof m);
    for (int k = 0; k < PIECES; k++) scalars[k] = (const uint8_t *)d_h + (size_t)k * N_ROWS * 32;
    m.n_columns = PIECES; m.n_bases = N_ROWS; m.d_bases = d_bases; m.d_scalars = scalars; m.out_points = commitment; m.status = mstatus;
    if ((rc = hsw_gadget_msm(g, &m, &mrep)) != HSW_OK) die("hsw_gadget_msm", rc, eng);
    printf("commit(h): %llu pieces of %u rows, refused %llu, bad bases %llu\n", (unsigned long long)mrep.columns, N_ROWS,
           (unsigned long long)mrep.refused_columns, (unsigned long long)mrep.bad_bases);
    if (mrep.refused_columns || mrep.bad_bases) return 1;
    print_point("H_0", commitment[0]);

    /* ---- on the host ---- */
    if ((rc = hsw_download(eng, coeff, d_coeff, sizeof coeff)) != HSW_OK || (rc = hsw_download(eng, h_coeff, d_h, sizeof h_coeff)) != HSW_OK)
        die("hsw_download", rc, eng);
    const fe zero = small(0);
    int ok = 1, some = 0;
    for (uint32_t j = 0; j < N_EXT; j++) {
        if (j >= PIECES * N_ROWS) ok = ok && same(h_coeff[j], zero);
        else some = some || !same(h_coeff[j], zero);
    }
    ok = ok && some;
    printf("h has degree below 3 n: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;
    /* every polynomial at x omega^r for the rotations 0, 1, 2, 3, -1 and u; then the expressions, folded with y */
    const fe x = times(&FR, small(0x6b8b4567u), small(0x327b23c6u)), one = small(1);
    const uint32_t rots[6] = {0, 1, 2, 3, N_ROWS - 1, USABLE};
    fe ev[COLS][6], V = zero;
    for (int r = 0; r < 6; r++) {
        fe e = zero, z;
        e.l[0] = rots[r];
        z = times(&FR, x, power(&FR, omega, e));
        for (int b = 0; b < COLS; b++) ev[b][r] = horner(coeff[b], N_ROWS, z);
    }
#define FOLD(expr) V = mul_add(V, y, (expr))
    for (int k = 0; k < 2; k++) {
        const fe *a = ev[A0 + k];
        FOLD(times(&FR, ev[Q0 + k][0], sub(&FR, mul_add(a[1], a[2], a[0]), a[3])));
    }
    FOLD(times(&FR, ev[L0][0], sub(&FR, one, ev[PZ0][0])));
    FOLD(times(&FR, ev[LLAST][0], sub(&FR, times(&FR, ev[PZ1][0], ev[PZ1][0]), ev[PZ1][0])));
    FOLD(times(&FR, ev[L0][0], sub(&FR, ev[PZ1][0], ev[PZ0][5])));
    {
        fe dj = one;
        for (int s = 0; s < 2; s++) {
            fe left = ev[PZ0 + s][1], right = ev[PZ0 + s][0];
            for (int j = 2 * s; j < 3 && j < 2 * s + 2; j++, dj = times(&FR, dj, delta)) {
                const fe v = ev[A0 + j][0];
                left = times(&FR, left, add(&FR, mul_add(beta, ev[SG0 + j][0], v), gamma));
                right = times(&FR, right, add(&FR, mul_add(beta, times(&FR, dj, x), v), gamma));
            }
            FOLD(times(&FR, ev[LACTIVE][0], sub(&FR, left, right)));
        }
    }
    for (int l = 0; l < 2; l++) {
        const fe A = l ? mul_add(ev[LKA][0], theta, ev[LKB][0]) : ev[A2][0], S = l ? mul_add(ev[T2A][0], theta, ev[T2B][0]) : ev[T1][0];
        const fe *Ap = ev[L1A + 3 * l], *Sp = ev[L1S + 3 * l], *Z = ev[L1Z + 3 * l];
        const fe d = sub(&FR, Ap[0], Sp[0]);
        FOLD(times(&FR, ev[L0][0], sub(&FR, one, Z[0])));
        FOLD(times(&FR, ev[LLAST][0], sub(&FR, times(&FR, Z[0], Z[0]), Z[0])));
        FOLD(times(&FR, ev[LACTIVE][0], sub(&FR, times(&FR, Z[1], times(&FR, add(&FR, Ap[0], beta), add(&FR, Sp[0], gamma))),
                                            times(&FR, Z[0], times(&FR, add(&FR, A, beta), add(&FR, S, gamma))))));
        FOLD(times(&FR, ev[L0][0], d));
        FOLD(times(&FR, ev[LACTIVE][0], times(&FR, d, sub(&FR, Ap[0], Ap[4]))));
    }
    {
        fe e = zero;
        e.l[0] = N_ROWS;
        ok = same(V, times(&FR, horner(h_coeff, PIECES * N_ROWS, x), sub(&FR, power(&FR, x, e), one)));
    }
    printf("the folded expressions at x are h(x) (x^n - 1): %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;
    point sum;
    sum.x = small(0); sum.y = gen.x; sum.z = small(0);
    for (uint32_t j = 0; j < N_ROWS; j++) {
        point b;
        b.x = bases[j][0]; b.y = bases[j][1]; b.z = gen.x;
        sum = p_add(sum, p_mul(h_coeff[j], b));
    }
    fe want[2];
    p_affine(sum, want);
    ok = memcmp(want, commitment[0], sizeof want) == 0;
    printf("H_0 is sum_j h[j] * G[j], byte for byte: %s\n", ok ? "yes" : "NO");
    if (!ok) return 1;

    hsw_gadget_destroy(g);
    hipFree(d_lagrange); hipFree(d_coeff); hipFree(d_ext); hipFree(d_h); hipFree(d_bases);
    hsw_engine_destroy(eng);
    puts("ok");
    return 0;
}
