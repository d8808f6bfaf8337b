// The device's Fr arithmetic (csrc/hsw_fr_mul.hpp) and the row rules of the lookup argument's grand product
// (csrc/hsw_product_value.hpp) against a model written here, on the CPU.  A stand-alone program: compile with
// -fsanitize=address,undefined and run it (tests/test_lookup_product_host.py does).
//
// The model knows nothing of Montgomery's method: numbers of nine 32-bit limbs, a * b mod p by shift-and-add (double,
// add, subtract p), x / 2 mod p by (x or x + p) >> 1, so a b 2^-256 is a product halved 256 times, and 1 / x is x^(p-2)
// by the same shift-and-add multiply.  Checked: fr_mont_mul, fr_add, fr_sub, fr_to_mont, fr_from_mont on all pairs of
// the corner operands and on random ones; fr_inv(x) x = 1 and fr_inv of the corners; and Z of small columns, computed
// the way hsw_lookup_product.hip computes it (tile products, prefix and suffix over the tiles, one inversion, prefix
// and suffix inside a tile), against the recurrence Z[i+1] = Z[i] num[i] / den[i] with an inversion per row.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_product_value.hpp"

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
static Big half(const Big &a) {
    Big x = (a.l[0] & 1u) ? plus(a, MP) : a;
    for (int j = 0; j < 9; j++) x.l[j] = (x.l[j] >> 1) | (j < 8 ? x.l[j + 1] << 31 : 0);
    return x;
}
static Big model_mont(const Big &a, const Big &b) { Big r = mulmod(a, b); for (int k = 0; k < 256; k++) r = half(r); return r; }
static Big model_times_R(Big a) { for (int k = 0; k < 256; k++) a = addmod(a, a); return a; }
static Big model_inv(const Big &a) {
    Big e = MP; e.l[0] -= 2;                      // p - 2 (the low limb is 0xf0000001)
    Big r{}; r.l[0] = 1;
    for (int bit = 255; bit >= 0; bit--) {
        r = mulmod(r, r);
        if ((e.l[bit >> 5] >> (bit & 31)) & 1u) r = mulmod(r, a);
    }
    return r;
}
static Big small(uint32_t x) { Big b{}; b.l[0] = x; return b; }

static bool same(const PFe &a, const Big &b) { return b.l[8] == 0 && std::memcmp(a.l, b.l, 32) == 0; }

static unsigned long long g_pairs = 0, g_columns = 0;

static void check_pair(const PFe &a, const PFe &b) {
    CHECK(hsw::pfe_below_p(a) && hsw::pfe_below_p(b));
    const Big A = big(a), B = big(b);
    CHECK(same(hsw::fr_mont_mul(a, b), model_mont(A, B)));
    CHECK(same(hsw::fr_add(a, b), addmod(A, B)));
    CHECK(same(hsw::fr_sub(a, b), submod(A, B)));
    g_pairs++;
}
static void check_single(const PFe &a) {
    const Big A = big(a);
    CHECK(same(hsw::fr_to_mont(a), model_times_R(A)));
    CHECK(same(hsw::fr_from_mont(hsw::fr_to_mont(a)), A));
    CHECK(same(hsw::fr_from_mont(a), model_mont(A, small(1))));
    const PFe inv = hsw::fr_inv(a);                               // a = x R: inv = x^-1 R, so inv * a * R^-1 = R (or 0 for a = 0)
    CHECK(hsw::pfe_below_p(inv));
    if (hsw::fr_is_zero(a)) CHECK(hsw::fr_is_zero(inv));
    else {
        CHECK(hsw::fr_equal(hsw::fr_mont_mul(inv, a), hsw::fr_one_mont()));
        CHECK(same(hsw::fr_from_mont(inv), model_inv(big(hsw::fr_from_mont(a)))));
    }
}

static PFe random_fe(std::mt19937_64 &rng) {
    Big b{};
    for (int j = 0; j < 8; j++) b.l[j] = (uint32_t)rng();
    b.l[7] &= 0x3fffffffu;                                        // below 2^254 < 4p: mod_p takes at most 3 steps
    return fe(mod_p(b));
}

// ---- Z of one column, the kernels' way -----------------------------------------------------------------------------
struct Column { std::vector<PFe> dense, spread, pin, ptab; uint32_t input_rows; };

static void kernel_rows(uint32_t kind, uint32_t T, uint32_t u, const Column &c, const hsw::ProductChallenges &ch, bool mont,
                        std::vector<PFe> &num, std::vector<PFe> &den) {
    for (uint32_t i = 0; i < u; i++) {
        PFe a = hsw::fr_zero();
        if (i < c.input_rows) a = hsw::product_input(kind, c.dense[i], c.spread[i], ch.theta_mul);
        num.push_back(hsw::product_term(a, hsw::product_table(kind, i, T, ch.theta, mont), ch, mont));
        den.push_back(hsw::product_term(c.pin[i], c.ptab[i], ch, mont));
    }
}

static std::vector<PFe> kernel_way(uint32_t kind, uint32_t T, uint32_t u, uint32_t tile, const Column &c, const hsw::ProductChallenges &ch, bool mont) {
    std::vector<PFe> num, den;
    kernel_rows(kind, T, u, c, ch, mont, num, den);
    const uint32_t n_tiles = (u + 1 + tile - 1) / tile;
    while (num.size() < (size_t)n_tiles * tile) { num.push_back(hsw::fr_one_mont()); den.push_back(hsw::fr_one_mont()); }   // rows at and beyond u
    std::vector<PFe> tn(n_tiles, hsw::fr_one_mont()), td(n_tiles, hsw::fr_one_mont());
    for (uint32_t k = 0; k < n_tiles; k++)
        for (uint32_t r = 0; r < tile; r++) { tn[k] = hsw::fr_mont_mul(tn[k], num[k * tile + r]); td[k] = hsw::fr_mont_mul(td[k], den[k * tile + r]); }
    PFe D = hsw::fr_one_mont();
    for (uint32_t k = 0; k < n_tiles; k++) D = hsw::fr_mont_mul(D, td[k]);
    PFe run_n = hsw::fr_inv(D), run_d = hsw::fr_one_mont();
    std::vector<PFe> factor(n_tiles);
    for (uint32_t k = n_tiles; k > 0; k--) { factor[k - 1] = run_d; run_d = hsw::fr_mont_mul(run_d, td[k - 1]); }
    for (uint32_t k = 0; k < n_tiles; k++) { factor[k] = hsw::fr_mont_mul(run_n, factor[k]); run_n = hsw::fr_mont_mul(run_n, tn[k]); }
    std::vector<PFe> z(u + 1);
    for (uint32_t k = 0; k < n_tiles; k++)
        for (uint32_t r = 0; r < tile && k * tile + r <= u; r++) {
            PFe v = factor[k];
            for (uint32_t q = 0; q < r; q++) v = hsw::fr_mont_mul(v, num[k * tile + q]);
            for (uint32_t q = r; q < tile; q++) v = hsw::fr_mont_mul(v, den[k * tile + q]);
            z[k * tile + r] = hsw::product_cell(v, mont);
        }
    return z;
}

// the value a cell stands for
static Big value_of(const PFe &cell, bool mont) { return mont ? model_mont(big(cell), small(1)) : big(cell); }
static PFe cell_of(const Big &v, bool mont) { return fe(mont ? model_times_R(v) : v); }
static uint32_t spread_of(uint32_t t) { uint32_t s = 0; for (int b = 0; b < 16; b++) s |= ((t >> b) & 1u) << (2 * b); return s; }

static void check_column(uint32_t kind, uint32_t T, uint32_t u, bool mont, bool permutation, std::mt19937_64 &rng) {
    const Big theta = big(random_fe(rng)), beta = big(random_fe(rng)), gamma = big(random_fe(rng));
    hsw::ProductChallenges ch;
    ch.theta = cell_of(theta, mont); ch.beta = cell_of(beta, mont); ch.gamma = cell_of(gamma, mont);
    ch.theta_mul = hsw::product_theta_mul(ch.theta, mont);
    auto val = [&](uint32_t t) {
        if (kind == 0) return small(t);
        if (kind == 1) return addmod(mulmod(small(t), theta), small(spread_of(t)));
        return addmod(small(t), mulmod(small(spread_of(t)), theta));
    };
    Column c;
    c.input_rows = permutation ? u : (uint32_t)(rng() % (u + 1));
    std::vector<Big> A(u), S(u), PA(u), PS(u);
    std::vector<uint32_t> rows(u);
    for (uint32_t i = 0; i < u; i++) {
        rows[i] = permutation ? (uint32_t)(rng() % T) : 0;
        const Big d = permutation ? small(rows[i]) : big(random_fe(rng)), s = permutation ? small(spread_of(rows[i])) : big(random_fe(rng));
        c.dense.push_back(cell_of(d, mont)); c.spread.push_back(cell_of(kind ? s : small(0), mont));
        if (i >= c.input_rows) A[i] = small(0);
        else A[i] = kind == 0 ? d : kind == 1 ? addmod(mulmod(d, theta), s) : addmod(d, mulmod(s, theta));
        S[i] = val(i < T ? i : 0);
    }
    for (uint32_t i = 0; i < u; i++) {
        // a permutation of the two columns (reversed: any one closes the product), or anything at all
        PA[i] = permutation ? A[u - 1 - i] : big(random_fe(rng));
        PS[i] = permutation ? S[u - 1 - i] : big(random_fe(rng));
        c.pin.push_back(cell_of(PA[i], mont)); c.ptab.push_back(cell_of(PS[i], mont));
    }
    std::vector<Big> Z(u + 1);
    Z[0] = small(1);
    for (uint32_t i = 0; i < u; i++) {
        const Big num = mulmod(addmod(A[i], beta), addmod(S[i], gamma)), den = mulmod(addmod(PA[i], beta), addmod(PS[i], gamma));
        CHECK(cmp(den, small(0)) != 0);
        Z[i + 1] = mulmod(mulmod(Z[i], num), model_inv(den));
    }
    if (permutation) CHECK(cmp(Z[u], small(1)) == 0);
    for (uint32_t tile : {1u, 2u, 3u, 4u, 64u}) {
        const std::vector<PFe> z = kernel_way(kind, T, u, tile, c, ch, mont);
        for (uint32_t i = 0; i <= u; i++) {
            CHECK(hsw::pfe_below_p(z[i]));
            CHECK(cmp(value_of(z[i], mont), Z[i]) == 0);
        }
    }
    g_columns++;
}

int main() {
    const Big R = model_times_R(small(1));
    const Big two254m1 = [] { Big b{}; for (int j = 0; j < 8; j++) b.l[j] = 0xffffffffu; b.l[7] = 0x3fffffffu; return mod_p(b); }();
    const std::vector<PFe> corners = {fe(small(0)), fe(small(1)), fe(minus(MP, small(1))), fe(R), fe(mulmod(R, R)), fe(two254m1)};
    CHECK(same(hsw::fr_one_mont(), R) && same(PFe{HSW_FR_R2}, mulmod(R, R)) && same(PFe{HSW_FR_R3}, mulmod(mulmod(R, R), R)));
    for (const PFe &a : corners) {
        check_single(a);
        for (const PFe &b : corners) check_pair(a, b);
    }
    std::mt19937_64 rng(20261020);
    for (int k = 0; k < 300; k++) {
        const PFe a = random_fe(rng), b = random_fe(rng);
        check_pair(a, b);
        if (k < 40) check_single(a);
        if (k < 12) for (const PFe &c : corners) { check_pair(a, c); check_pair(c, a); }
    }
    for (uint32_t u : {1u, 2u, 5u, 64u})
        for (uint32_t kind = 0; kind < 3; kind++) {
            if (u == 64 && kind != 1) continue;                   // (an inversion per row in the model: the long column once)
            for (int mont = 0; mont < 2; mont++)
                for (int perm = 0; perm < 2; perm++) check_column(kind, u < 4 ? 1 : 4, u, mont != 0, perm != 0, rng);
        }
    std::printf("fr mul check ok: %llu operand pairs, %llu columns\n", g_pairs, g_columns);
    return 0;
}
