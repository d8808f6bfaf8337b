// csrc/hsw_fq.hpp and csrc/hsw_g1.hpp on the CPU, under ASan + UBSan: Fq multiply, add, sub, negate and inverse against
// shift-and-add arithmetic on 4 x 64-bit words that shares no line with them, and the three complete formulas
// (mixed addition, addition, doubling) and the normalisation against affine chord-and-tangent arithmetic -- random
// points, P + P, P + (-P), the identity on either side.  Stand-alone: its own main, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_g1.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using hsw::Fq;
using hsw::G1;
using hsw::G1Affine;

// ---- the reference: integers below q as four 64-bit words, every product by shift-and-add
struct U { uint64_t w[4]; };
static const U Q = {{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
static bool u_eq(const U &a, const U &b) { return !std::memcmp(a.w, b.w, 32); }
static bool u_zero(const U &a) { return !(a.w[0] | a.w[1] | a.w[2] | a.w[3]); }
static bool u_ge(const U &a, const U &b) {
    for (int i = 3; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
    return true;
}
static U u_sub_raw(const U &a, const U &b) {
    U r;
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 x = (unsigned __int128)a.w[i] - b.w[i] - br;
        r.w[i] = (uint64_t)x;
        br = (x >> 64) & 1;
    }
    return r;
}
static U u_addmod(const U &a, const U &b) {                                 // a, b < q < 2^254: no carry out
    U r;
    unsigned __int128 cy = 0;
    for (int i = 0; i < 4; i++) {
        cy += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)cy;
        cy >>= 64;
    }
    return u_ge(r, Q) ? u_sub_raw(r, Q) : r;
}
static U u_submod(const U &a, const U &b) { return u_ge(a, b) ? u_sub_raw(a, b) : u_sub_raw(u_addmod(a, u_sub_raw(Q, b)), U{{0, 0, 0, 0}}); }
static U u_mulmod(const U &a, const U &b) {
    U r = {{0, 0, 0, 0}};
    for (int bit = 255; bit >= 0; bit--) {
        r = u_addmod(r, r);
        if ((b.w[bit >> 6] >> (bit & 63)) & 1) r = u_addmod(r, a);
    }
    return r;
}
static U u_powmod(const U &a, const U &e) {
    U r = {{1, 0, 0, 0}};
    for (int bit = 255; bit >= 0; bit--) {
        r = u_mulmod(r, r);
        if ((e.w[bit >> 6] >> (bit & 63)) & 1) r = u_mulmod(r, a);
    }
    return r;
}
static U u_inv(const U &a) { return u_powmod(a, u_sub_raw(Q, U{{2, 0, 0, 0}})); }
static U u_small(uint64_t x) { return U{{x, 0, 0, 0}}; }

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {                                                     // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static U u_random() {
    U r = {{rnd(), rnd(), rnd(), rnd() >> 3}};
    while (u_ge(r, Q)) r = u_sub_raw(r, Q);
    return r;
}

static U R1;                                                                // 2^256 mod q
static Fq to_fq(const U &a) {                                               // the same limbs, no change of form
    Fq f;
    for (int i = 0; i < 4; i++) { f.l[2 * i] = (uint32_t)a.w[i]; f.l[2 * i + 1] = (uint32_t)(a.w[i] >> 32); }
    return f;
}
static U to_u(const Fq &f) {
    U a;
    for (int i = 0; i < 4; i++) a.w[i] = f.l[2 * i] | (uint64_t)f.l[2 * i + 1] << 32;
    return a;
}
static Fq mont_of(const U &a) { return to_fq(u_mulmod(a, R1)); }           // by the reference, not by fq_to_mont

// ---- affine chord-and-tangent points over the reference; inf for the identity
struct P { U x, y; bool inf; };
static P p_neg(const P &a) { return a.inf ? a : P{a.x, u_zero(a.y) ? a.y : u_sub_raw(Q, a.y), false}; }
static P p_add(const P &a, const P &b) {
    if (a.inf) return b;
    if (b.inf) return a;
    U lam;
    if (u_eq(a.x, b.x)) {
        if (u_zero(u_addmod(a.y, b.y))) return P{{}, {}, true};
        lam = u_mulmod(u_mulmod(u_small(3), u_mulmod(a.x, a.x)), u_inv(u_addmod(a.y, a.y)));
    } else {
        lam = u_mulmod(u_submod(b.y, a.y), u_inv(u_submod(b.x, a.x)));
    }
    const U x3 = u_submod(u_submod(u_mulmod(lam, lam), a.x), b.x);
    return P{x3, u_submod(u_mulmod(lam, u_submod(a.x, x3)), a.y), false};
}
static P p_mul(uint64_t k, P a) {
    P acc{{}, {}, true};
    for (; k; k >>= 1) {
        if (k & 1) acc = p_add(acc, a);
        a = p_add(a, a);
    }
    return acc;
}
static G1Affine stored(const P &a) { return a.inf ? G1Affine{hsw::fq_zero(), hsw::fq_zero()} : G1Affine{mont_of(a.x), mont_of(a.y)}; }
static bool same(const G1 &got, const P &want) {
    const G1Affine g = hsw::g1_to_affine(got), w = stored(want);
    if (hsw::g1_is_identity(got) != want.inf) return false;
    return hsw::fq_equal(g.x, w.x) && hsw::fq_equal(g.y, w.y);
}

int main() {
    R1 = u_small(1);
    for (int i = 0; i < 256; i++) R1 = u_addmod(R1, R1);
    {   // ---- the constants
        const Fq q = HSW_FQ_Q, r = HSW_FQ_R, r2 = HSW_FQ_R2;
        CHECK(u_eq(to_u(q), Q) && u_eq(to_u(r), R1) && u_eq(to_u(r2), u_mulmod(R1, R1)));
        CHECK(!hsw::fq_below_q(q) && hsw::fq_below_q(to_fq(u_sub_raw(Q, u_small(1)))) && hsw::fq_below_q(hsw::fq_zero()));
        Fq top = hsw::fq_zero();
        top.l[7] = 0x80000000u;
        CHECK(!hsw::fq_below_q(top));
    }
    // ---- the field
    unsigned n_field = 0;
    const U edge[5] = {u_small(0), u_small(1), u_small(2), u_sub_raw(Q, u_small(1)), u_sub_raw(Q, u_small(2))};
    for (int k = 0; k < 200; k++) {
        const U a = k < 25 ? edge[k / 5] : u_random(), b = k < 25 ? edge[k % 5] : u_random();
        const Fq fa = to_fq(a), fb = to_fq(b);
        CHECK(u_eq(to_u(hsw::fq_add(fa, fb)), u_addmod(a, b)));
        CHECK(u_eq(to_u(hsw::fq_sub(fa, fb)), u_submod(a, b)));
        CHECK(u_eq(to_u(hsw::fq_neg(fa)), u_submod(u_small(0), a)));
        const Fq m = hsw::fq_mont_mul(fa, fb);                              // a b / R: times R it is a b
        CHECK(hsw::fq_below_q(m) && u_eq(u_mulmod(to_u(m), R1), u_mulmod(a, b)));
        CHECK(u_eq(to_u(hsw::fq_to_mont(fa)), u_mulmod(a, R1)) && u_eq(to_u(hsw::fq_from_mont(hsw::fq_to_mont(fa))), a));
        CHECK(u_eq(to_u(hsw::fq_mul_b3(fa)), u_mulmod(a, u_small(9))));
        n_field += 7;
    }
    for (int k = 0; k < 12; k++) {
        const U a = k < 3 ? edge[k + 1] : u_random();
        const Fq inv = hsw::fq_inv(mont_of(a));                              // x R -> x^-1 R
        CHECK(u_eq(to_u(inv), u_mulmod(u_inv(a), R1)));
        n_field++;
    }
    CHECK(hsw::fq_is_zero(hsw::fq_inv(hsw::fq_zero())));
    // ---- the curve
    const P G{u_small(1), u_small(2), false}, INF{{}, {}, true};
    unsigned n_curve = 0;
    CHECK(same(hsw::g1_identity(), INF) && same(hsw::g1_from_affine(stored(INF)), INF) && same(hsw::g1_from_affine(stored(G)), G));
    CHECK(hsw::g1_affine_is_identity(stored(INF)) && !hsw::g1_affine_is_identity(stored(G)));
    {
        const G1Affine z = hsw::g1_to_affine(hsw::g1_identity());            // the identity normalises to 64 zero bytes
        const uint8_t zero[64] = {0};
        CHECK(!std::memcmp(&z, zero, 64));
    }
    for (int k = 0; k < 12; k++) {
        const P a = p_mul((rnd() & 0xfffff) | 1, G), b = p_mul((rnd() & 0xfffff) | 1, G);
        // a projective reading of a with Z != 1: (x z, y z, z)
        const Fq z = mont_of(u_random());
        const G1Affine sa = stored(a), sb = stored(b);
        const G1 pa{hsw::fq_mont_mul(sa.x, z), hsw::fq_mont_mul(sa.y, z), z}, pb = hsw::g1_from_affine(sb), id = hsw::g1_identity();
        CHECK(same(pa, a));
        CHECK(same(hsw::g1_add_mixed(pa, sb), p_add(a, b)) && same(hsw::g1_add(pa, pb), p_add(a, b)) && same(hsw::g1_add(pb, pa), p_add(a, b)));
        CHECK(same(hsw::g1_add_mixed(pa, sa), p_add(a, a)) && same(hsw::g1_add(pa, hsw::g1_from_affine(sa)), p_add(a, a)) && same(hsw::g1_add(pa, pa), p_add(a, a)));
        CHECK(same(hsw::g1_double(pa), p_add(a, a)) && same(hsw::g1_double(id), INF));
        const G1Affine na = stored(p_neg(a));
        CHECK(same(hsw::g1_add_mixed(pa, na), INF) && same(hsw::g1_add(pa, hsw::g1_from_affine(na)), INF));
        CHECK(same(hsw::g1_add_mixed(id, sb), b) && same(hsw::g1_add(id, pb), b) && same(hsw::g1_add(pb, id), b) && same(hsw::g1_add(id, id), INF));
        // an identity that is not (0 : 1 : 0) but (0 : y : 0), as a sum P + (-P) leaves it
        const G1 id2 = hsw::g1_add_mixed(pa, na);
        CHECK(hsw::g1_is_identity(id2) && same(hsw::g1_add_mixed(id2, sb), b) && same(hsw::g1_add(id2, pa), a) && same(hsw::g1_double(id2), INF));
        n_curve += 19;
    }
    std::printf("g1 check ok: %u field checks, %u curve checks\n", n_field, n_curve);
    return 0;
}
