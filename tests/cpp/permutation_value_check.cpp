// The row rules of the permutation argument's grand products (csrc/hsw_permutation_value.hpp) against a model written
// here, on the CPU.  A stand-alone program: compile with -fsanitize=address,undefined and run it
// (tests/test_permutation_product_host.py does).
//
// The model knows nothing of Montgomery's method: numbers of nine 32-bit limbs, a * b mod p by shift-and-add, x / 2 mod p
// by (x or x + p) >> 1, 1 / x by the binary extended Euclid (not the Fermat power of fr_inv).  Checked: the staged route
// to omega^i (binary powers of omega^1024, the per-thread table, omega per row) against omega^i by square-and-multiply,
// at rows 0, 1023, 1024, 2^31 - 1 and around every table boundary; beta delta^j and the seeds; and the Z columns of small
// permutations, computed the way hsw_permutation_product.hip computes them (per thread its first row's omega power, a
// loop over the chunk's columns, the identity term times omega from row to row, then prefix of the numerators, suffix
// of the denominators over the proof's concatenated chunks and ONE inversion), against the recurrence
// Z_s[i+1] = Z_s[i] num_s[i] / den_s[i], Z_s[0] = Z_{s-1}[u], with an inversion per row -- in both cell forms, for m in
// {1, 3, 5}, L in {1, 2, 4}, u in {1, 5, 1030}, random columns of differing heights and columns that must close.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_permutation_value.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using hsw::PFe;

// ---- the model ---------------------------------------------------------------------------------------------------
struct Big { uint32_t l[9]; };
static const Big MP = {{0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u, 0}};

static Big big(const PFe &a) { Big b{}; std::memcpy(b.l, a.l, 32); return b; }
static PFe fe(const Big &b) { CHECK(b.l[8] == 0); PFe a; std::memcpy(a.l, b.l, 32); return a; }
static int cmp(const Big &a, const Big &b) {
    for (int j = 8; j >= 0; j--) if (a.l[j] != b.l[j]) return a.l[j] < b.l[j] ? -1 : 1;
    return 0;
}
static Big plus(const Big &a, const Big &b) {
    Big s; uint64_t cy = 0;
    for (int j = 0; j < 9; j++) { cy += (uint64_t)a.l[j] + b.l[j]; s.l[j] = (uint32_t)cy; cy >>= 32; }
    CHECK(cy == 0);
    return s;
}
static Big minus(const Big &a, const Big &b) {
    CHECK(cmp(a, b) >= 0);
    Big d; int64_t br = 0;
    for (int j = 0; j < 9; j++) { const int64_t x = (int64_t)a.l[j] - b.l[j] - br; d.l[j] = (uint32_t)x; br = x < 0; }
    return d;
}
static Big small(uint32_t x) { Big b{}; b.l[0] = x; return b; }
static bool is_even(const Big &a) { return (a.l[0] & 1u) == 0; }
static Big shr1(Big x) { for (int j = 0; j < 9; j++) x.l[j] = (x.l[j] >> 1) | (j < 8 ? x.l[j + 1] << 31 : 0); return x; }
static Big mod_p(Big a) { while (cmp(a, MP) >= 0) a = minus(a, MP); return a; }        // (a few steps at the most here)
static Big addmod(const Big &a, const Big &b) { return mod_p(plus(a, b)); }
static Big submod(const Big &a, const Big &b) { return cmp(a, b) >= 0 ? minus(a, b) : minus(plus(a, MP), b); }
static Big mulmod(const Big &a, const Big &b) {
    Big r{};
    for (int bit = 255; bit >= 0; bit--) {
        r = addmod(r, r);
        if ((b.l[bit >> 5] >> (bit & 31)) & 1u) r = addmod(r, a);
    }
    return r;
}
static Big half(const Big &a) { return shr1(is_even(a) ? a : plus(a, MP)); }
static Big model_from_mont(Big a) { for (int k = 0; k < 256; k++) a = half(a); return a; }
static Big model_times_R(Big a) { for (int k = 0; k < 256; k++) a = addmod(a, a); return a; }
static Big model_pow(const Big &a, uint64_t e) {
    Big r = small(1);
    for (int bit = 63; bit >= 0; bit--) { r = mulmod(r, r); if ((e >> bit) & 1u) r = mulmod(r, a); }
    return r;
}
// 1 / a mod p for 0 < a < p: binary extended Euclid (u x1 = a x2 = ... invariants u = x1 a, v = x2 a mod p)
static Big model_inv(const Big &a) {
    CHECK(cmp(a, small(0)) != 0);
    Big u = a, v = MP, x1 = small(1), x2 = small(0);
    while (cmp(u, small(1)) != 0 && cmp(v, small(1)) != 0) {
        while (is_even(u)) { u = shr1(u); x1 = half(x1); }
        while (is_even(v)) { v = shr1(v); x2 = half(x2); }
        if (cmp(u, v) >= 0) { u = minus(u, v); x1 = submod(x1, x2); }
        else { v = minus(v, u); x2 = submod(x2, x1); }
    }
    return cmp(u, small(1)) == 0 ? x1 : x2;
}

static Big value_of(const PFe &cell, bool mont) { return mont ? model_from_mont(big(cell)) : big(cell); }
static PFe cell_of(const Big &v, bool mont) { return fe(mont ? model_times_R(v) : v); }
static Big random_big(std::mt19937_64 &rng) {
    Big b{};
    for (int j = 0; j < 8; j++) b.l[j] = (uint32_t)rng();
    b.l[7] &= 0x3fffffffu;                                        // below 2^254 < 4p: mod_p takes at most 3 steps
    return mod_p(b);
}

static const uint32_t ROWS = 4, TILE = ROWS * hsw::PERMUTATION_TABLE;     // the kernels' geometry: 4 rows per thread, 1,024 per tile
static unsigned long long g_rows = 0, g_permutations = 0;

// omega^row in Montgomery form, the kernels' way
static PFe staged_omega(const hsw::PermutationPowers &pw, uint64_t row) {
    const PFe tile = hsw::permutation_omega_tile(pw, (uint32_t)(row / TILE));
    PFe w = hsw::permutation_omega_thread(pw, tile, (uint32_t)(row % TILE / ROWS));
    for (uint32_t r = 0; r < row % ROWS; r++) w = hsw::fr_mont_mul(w, pw.omega);
    return w;
}

static void check_powers(std::mt19937_64 &rng) {
    for (int mont = 0; mont < 2; mont++) {
        const Big omega = random_big(rng);
        hsw::PermutationPowers pw;
        hsw::permutation_stage_powers(hsw::permutation_to_mont(cell_of(omega, mont != 0), mont != 0), ROWS, pw);
        for (uint64_t row : {0ull, 1ull, 3ull, 4ull, 1019ull, 1023ull, 1024ull, 1025ull, 2047ull, 2048ull, 1024ull * 1023 + 1023, 1ull << 20,
                             (1ull << 30) + 5, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1023}) {
            const PFe w = staged_omega(pw, row);
            CHECK(hsw::pfe_below_p(w) && cmp(value_of(w, true), model_pow(omega, row)) == 0);
            g_rows++;
        }
    }
    // seeds: R^(n+1) as an element for canonical factors, R for Montgomery ones
    Big r = model_times_R(small(1));
    const Big R = r;
    for (uint32_t n = 1; n <= 6; n++) {
        r = mulmod(r, R);
        CHECK(cmp(big(hsw::permutation_seed(n, false)), r) == 0 && cmp(big(hsw::permutation_seed(n, true)), R) == 0);
    }
}

static void check_permutation(uint32_t m, uint32_t L, uint32_t u, bool mont, bool closes, std::mt19937_64 &rng) {
    const uint32_t S = (m + L - 1) / L;
    const Big beta = random_big(rng), gamma = random_big(rng), omega = random_big(rng), delta = random_big(rng);
    // the model's cells
    std::vector<Big> label((size_t)m * u);                        // delta^j omega^i
    Big dj = small(1);
    for (uint32_t j = 0; j < m; j++) {
        Big w = small(1);
        for (uint32_t i = 0; i < u; i++) { label[(size_t)j * u + i] = mulmod(dj, w); w = mulmod(w, omega); }
        dj = mulmod(dj, delta);
    }
    std::vector<Big> V((size_t)m * u), Sg((size_t)m * u);
    std::vector<uint32_t> rows(m, u);
    const Big constant = random_big(rng);
    for (uint32_t j = 0; j < m; j++) {
        if (!closes) rows[j] = (uint32_t)(rng() % (u + 1));
        for (uint32_t i = 0; i < u; i++) {
            // closes: every cell holds one value and sigma is the labels turned round, a permutation of all m u cells
            V[(size_t)j * u + i] = closes ? constant : i < rows[j] ? random_big(rng) : small(0);
            Sg[(size_t)j * u + i] = closes ? label[(size_t)(m - 1 - j) * u + (u - 1 - i)] : random_big(rng);
        }
    }
    // the recurrence, an inversion per row
    std::vector<Big> Z((size_t)S * (u + 1));
    Big z = small(1);
    for (uint32_t s = 0; s < S; s++) {
        Z[(size_t)s * (u + 1)] = z;
        for (uint32_t i = 0; i < u; i++) {
            Big num = small(1), den = small(1);
            for (uint32_t j = s * L; j < m && j < (s + 1) * L; j++) {
                const Big v = V[(size_t)j * u + i];
                num = mulmod(num, addmod(addmod(v, mulmod(beta, label[(size_t)j * u + i])), gamma));
                den = mulmod(den, addmod(addmod(v, mulmod(beta, Sg[(size_t)j * u + i])), gamma));
            }
            z = mulmod(mulmod(z, num), model_inv(den));
            Z[(size_t)s * (u + 1) + i + 1] = z;
        }
    }
    if (closes) CHECK(cmp(z, small(1)) == 0);
    // the kernels' way, on cells as stored
    std::vector<PFe> cv((size_t)m * u), cs((size_t)m * u);
    for (size_t k = 0; k < cv.size(); k++) { cv[k] = cell_of(V[k], mont); cs[k] = cell_of(Sg[k], mont); }
    const PFe beta_stored = cell_of(beta, mont);
    hsw::PermutationChallenges ch{hsw::product_theta_mul(beta_stored, mont), cell_of(gamma, mont)};
    hsw::PermutationPowers pw;
    hsw::permutation_stage_powers(hsw::permutation_to_mont(cell_of(omega, mont), mont), ROWS, pw);
    const PFe delta_mont = hsw::permutation_to_mont(cell_of(delta, mont), mont);
    std::vector<PFe> bd(m);
    Big bdj = beta;
    for (uint32_t j = 0; j < m; j++) {
        bd[j] = j ? hsw::permutation_next_beta_delta(bd[j - 1], delta_mont) : beta_stored;
        CHECK(cmp(value_of(bd[j], mont), bdj) == 0);
        bdj = mulmod(bdj, delta);
    }
    const uint32_t n_tiles = (u + 1 + TILE - 1) / TILE, span = n_tiles * TILE;      // rows at and beyond u: the factor 1
    std::vector<PFe> num((size_t)S * span, hsw::fr_one_mont()), den(num);
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t j0 = s * L, j1 = m - j0 < L ? m : j0 + L;
        const PFe seed = hsw::permutation_seed(j1 - j0, mont);
        for (uint32_t row0 = 0; row0 < span; row0 += ROWS) {
            const PFe w0 = staged_omega(pw, row0);
            for (uint32_t r = 0; r < ROWS && row0 + r < u; r++) num[(size_t)s * span + row0 + r] = den[(size_t)s * span + row0 + r] = seed;
            for (uint32_t j = j0; j < j1; j++) {
                PFe id = hsw::permutation_identity_term(bd[j], w0);
                for (uint32_t r = 0; r < ROWS; r++) {
                    const uint32_t i = row0 + r;
                    if (r) id = hsw::fr_mont_mul(id, pw.omega);
                    if (i >= u) continue;
                    const PFe v = i < rows[j] ? cv[(size_t)j * u + i] : hsw::fr_zero();
                    PFe &n = num[(size_t)s * span + i], &d = den[(size_t)s * span + i];
                    n = hsw::permutation_accumulate(n, hsw::permutation_factor(v, id, ch.gamma), j == j0, mont);
                    d = hsw::permutation_accumulate(d, hsw::permutation_factor(v, hsw::permutation_sigma_term(cs[(size_t)j * u + i], ch.beta_mul), ch.gamma), j == j0, mont);
                }
            }
        }
    }
    PFe D = hsw::fr_one_mont();
    for (const PFe &d : den) D = hsw::fr_mont_mul(D, d);
    std::vector<PFe> suffix(num.size());
    PFe run = hsw::fr_one_mont();
    for (size_t k = num.size(); k > 0; k--) { run = hsw::fr_mont_mul(run, den[k - 1]); suffix[k - 1] = run; }
    run = hsw::fr_inv(D);
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t i = 0; i < span; i++) {
            const size_t k = (size_t)s * span + i;
            if (i <= u) {
                const PFe cell = hsw::product_cell(hsw::fr_mont_mul(run, suffix[k]), mont);
                CHECK(hsw::pfe_below_p(cell));
                CHECK(cmp(value_of(cell, mont), Z[(size_t)s * (u + 1) + i]) == 0);
                g_rows++;
            }
            run = hsw::fr_mont_mul(run, num[k]);
        }
    g_permutations++;
}

int main() {
    std::mt19937_64 rng(20261020);
    check_powers(rng);
    for (uint32_t m : {1u, 3u, 5u})
        for (uint32_t L : {1u, 2u, 4u})
            for (uint32_t u : {1u, 5u, 1030u})
                for (int mont = 0; mont < 2; mont++) {
                    check_permutation(m, L, u, mont != 0, false, rng);
                    if (u != 1030 || (m == 5 && L == 2)) check_permutation(m, L, u, mont != 0, true, rng);
                }
    std::printf("permutation value check ok: %llu rows, %llu permutations\n", g_rows, g_permutations);
    return 0;
}
