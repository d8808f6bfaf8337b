// The index rules of the permuted lookup pair (csrc/hsw_permuted_index.hpp) and the value of a table row
// (csrc/hsw_permuted_value.hpp) against brute-force models, on the CPU.  A stand-alone program: compile with
// -fsanitize=address,undefined and run it (tests/test_lookup_permuted_host.py does).
//
// The header's functions are called the way hsw_lookup_permuted.hip calls them: the arrays are built chunk by chunk
// with the chunk bases from a scan (for several chunk counts), and the output is resolved tile by tile through a
// window of the offsets (for several tile sizes).  The model sorts: A' = the sorted multiset of the entries plus u - E
// zeros; S' = the first position of every run gets the run's row, the other positions take what is left of the
// table plus u - T zeros, ascending.  Checked per case: the multisets, the two permuted-pair constraints, and
// that the output equals the model exactly.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_permuted_index.hpp"
#include "../../halo2-dynamic-sha256_amd/csrc/hsw_permuted_value.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

typedef std::vector<uint32_t> Vec;
static unsigned long long g_cases = 0;

// the contract of include/hsw.h, by sorting
static void model(const Vec &m, uint32_t u, Vec &A, Vec &S) {
    const uint32_t T = (uint32_t)m.size();
    A.clear();
    uint64_t E = 0;
    for (uint32_t t = 0; t < T; t++) { E += m[t]; A.insert(A.end(), m[t], t); }
    CHECK(E <= u);
    A.insert(A.end(), u - E, 0u);
    std::sort(A.begin(), A.end());
    Vec left;                                  // the table column: T rows and u - T padding rows that repeat row 0
    for (uint32_t t = 0; t < T; t++) left.push_back(t);
    left.insert(left.end(), u - T, 0u);
    S.assign(u, 0xffffffffu);
    for (uint32_t i = 0; i < u; i++)
        if (i == 0 || A[i] != A[i - 1]) {
            S[i] = A[i];
            left.erase(std::find(left.begin(), left.end(), A[i]));
        }
    std::sort(left.begin(), left.end());
    size_t q = 0;
    for (uint32_t i = 0; i < u; i++) if (S[i] == 0xffffffffu) S[i] = left[q++];
    CHECK(q == left.size());
}

// the header, the way the kernels use it
static void device_way(const Vec &m, uint32_t u, uint32_t chunks, uint32_t tile, Vec &A, Vec &S) {
    const uint32_t T = (uint32_t)m.size();
    uint64_t E = 0;
    for (uint32_t t = 0; t < T; t++) E += m[t];
    const uint32_t pad0 = u - (uint32_t)E;
    // exact-size arrays: a write past them is the sanitizer's to report
    Vec index(hsw::permuted_index_words(T), 0xeeeeeeeeu);
    uint32_t *used_off = index.data(), *used_row = used_off + T + 1, *spare_row = used_row + T;
    const uint32_t chunk = (T + chunks - 1) / chunks;
    std::vector<hsw::PermutedSums> base(chunks + 1);
    base[0] = hsw::PermutedSums{0, 0, 0};
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t lo = std::min(c * chunk, T), hi = std::min(lo + chunk, T);
        const hsw::PermutedSums s = hsw::permuted_chunk_sums(m.data(), lo, hi, pad0);
        base[c + 1] = hsw::PermutedSums{base[c].rows + s.rows, base[c].used + s.used, base[c].spare + s.spare};
    }
    const hsw::PermutedHead head = hsw::permuted_head(m.data(), T, u, pad0, base[chunks]);
    CHECK(base[chunks].rows == u && head.used >= 1 && head.used <= T && head.ok == 1);
    CHECK(head.zeros + base[chunks].spare == u - head.used);                   // both sides: the repeated positions
    used_off[head.used] = u;
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t lo = std::min(c * chunk, T), hi = std::min(lo + chunk, T);
        hsw::permuted_chunk_write(m.data(), lo, hi, pad0, base[c], used_off, used_row, spare_row);
    }
    A.assign(u, 0xffffffffu); S.assign(u, 0xffffffffu);
    for (uint32_t i0 = 0; i0 < u; i0 += tile) {
        const uint32_t i1 = std::min(u, i0 + tile);
        const uint32_t j0 = hsw::permuted_find(used_off, 0, head.used, i0);
        const uint32_t n = std::min(tile, head.used - j0);
        Vec win(used_off + j0, used_off + j0 + n + 1);                         // the LDS window, exact size
        const bool one_run = win[1] >= i1;
        for (uint32_t i = i0; i < i1; i++)
            hsw::permuted_rows(win.data(), one_run ? 1u : n, j0, i, used_row, spare_row, head.zeros, &A[i], &S[i]);
    }
}

static void check(const Vec &m, uint32_t u) {
    const uint32_t T = (uint32_t)m.size();
    Vec A, S, A2, S2;
    model(m, u, A, S);
    // the model itself has the properties the issue names
    uint64_t E = 0;
    for (uint32_t x : m) E += x;
    Vec ca(T, 0), cs(T, 0);
    for (uint32_t i = 0; i < u; i++) { CHECK(A[i] < T && S[i] < T); ca[A[i]]++; cs[S[i]]++; }
    for (uint32_t t = 0; t < T; t++) {
        CHECK(ca[t] == m[t] + (t == 0 ? u - (uint32_t)E : 0u));                // the entries plus u - E zeros
        CHECK(cs[t] == 1u + (t == 0 ? u - T : 0u));                            // the table plus u - T copies of row 0
    }
    CHECK(A[0] == S[0]);
    for (uint32_t i = 1; i < u; i++) CHECK(A[i] == S[i] || A[i] == A[i - 1]);
    const uint32_t chunk_counts[4] = {1, 3, (T + 3) / 4, 1024}, tiles[3] = {1, 7, 1024};      // (T + 3) / 4: four rows a chunk, the kernel's
    for (uint32_t chunks : chunk_counts)
        for (uint32_t tile : tiles) {
            device_way(m, u, chunks, tile, A2, S2);
            CHECK(A2 == A && S2 == S);
        }
    g_cases++;
}

// every m of T rows with sum m = E
static void exhaustive(Vec &head, uint32_t t, uint32_t left, uint32_t u) {
    if (t == head.size()) { Vec m(head); m.push_back(left); check(m, u); return; }
    for (uint32_t k = 0; k <= left; k++) { head[t] = k; exhaustive(head, t + 1, left - k, u); }
}

static void corners(uint32_t T, uint32_t u, std::mt19937 &rng) {
    Vec m(T, 0);
    check(m, u);                                                              // E = 0
    m.assign(T, 0); m[T - 1] = u; check(m, u);                                 // all of u on row T - 1 (E = u, m'[0] = 0)
    m.assign(T, 1); m[0] = 0; m[1] = u - (T - 2); check(m, u);                 // E = u with m'[0] = 0
    if (u == T) { m.assign(T, 1); check(m, u); }                               // no repeated position
    m.assign(T, 1); check(m, u);                                               // every row used, the rest on row 0
    m.assign(T, 0); m[0] = u; check(m, u);                                     // E = u on row 0
    for (int rep = 0; rep < 6; rep++) {                                        // seeded random, sparse and dense
        m.assign(T, 0);
        const uint32_t E = rep == 0 ? u : rng() % (u + 1);
        for (uint32_t e = 0; e < E; e++) m[rep % 2 ? rng() % T : (rng() % 16) * (T / 16) + rng() % 3]++;
        check(m, u);
    }
}

// s * a mod p by shift-and-add on the header's own add (itself checked on p - 1 below)
static hsw::PFe slow_mul(uint32_t s, const hsw::PFe &a) {
    hsw::PFe r{{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int b = 31; b >= 0; b--) {
        r = hsw::pfe_add(r, r);
        if ((s >> b) & 1u) r = hsw::pfe_add(r, a);
    }
    return r;
}
static void values(std::mt19937 &rng) {
    const uint32_t P[8] = HSW_PV_P;
    hsw::PFe pm1, one{{1, 0, 0, 0, 0, 0, 0, 0}}, zero{{0, 0, 0, 0, 0, 0, 0, 0}};
    std::memcpy(pm1.l, P, sizeof P);
    CHECK(!hsw::pfe_below_p(pm1));
    pm1.l[0] -= 1;                                                             // p - 1
    CHECK(hsw::pfe_below_p(pm1) && hsw::pfe_below_p(zero));
    const hsw::PFe w = hsw::pfe_add(pm1, one);                                 // (p - 1) + 1 = 0
    CHECK(std::memcmp(w.l, zero.l, 32) == 0);
    const hsw::PFe x = hsw::pfe_add(pm1, pm1);                                 // = p - 2
    CHECK(x.l[0] == P[0] - 2 && x.l[7] == P[7]);
    const uint32_t scalars[6] = {0, 1, 0xffffu, 0x55555555u, 0xffffffffu, 0x80000000u};
    for (int rep = 0; rep < 2000; rep++) {
        hsw::PFe a;
        do { for (int j = 0; j < 8; j++) a.l[j] = rng(); a.l[7] &= 0x3fffffffu; } while (!hsw::pfe_below_p(a));
        if (rep == 0) a = pm1;
        if (rep == 1) a = zero;
        const uint32_t s = rep < 12 ? scalars[rep % 6] : rng();
        const hsw::PFe got = hsw::pfe_mul_small(s, a), want = slow_mul(s, a);
        CHECK(std::memcmp(got.l, want.l, 32) == 0 && hsw::pfe_below_p(got));
        // the value of a row in both orders of the fold and both representations, against the same slow multiply
        const uint32_t t = s & 0xffffu, sp = hsw::pfe_spread_of(t);
        const hsw::PFe R = hsw::pfe_repr(1, true);
        for (int mont = 0; mont < 2; mont++) {
            const hsw::PFe rt = mont ? slow_mul(t, R) : hsw::PFe{{t, 0, 0, 0, 0, 0, 0, 0}};
            const hsw::PFe rs = mont ? slow_mul(sp, R) : hsw::PFe{{sp, 0, 0, 0, 0, 0, 0, 0}};
            const hsw::PFe v0 = hsw::permuted_value(0, t, a, mont != 0), v1 = hsw::permuted_value(1, t, a, mont != 0), v2 = hsw::permuted_value(2, t, a, mont != 0);
            const hsw::PFe w1 = hsw::pfe_add(slow_mul(t, a), rs), w2 = hsw::pfe_add(slow_mul(sp, a), rt);
            CHECK(std::memcmp(v0.l, rt.l, 32) == 0 && std::memcmp(v1.l, w1.l, 32) == 0 && std::memcmp(v2.l, w2.l, 32) == 0);
        }
    }
    CHECK(hsw::pfe_spread_of(0xffffu) == 0x55555555u && hsw::pfe_spread_of(0x5u) == 0x11u);
    const hsw::PFe R = hsw::pfe_repr(1, true);
    CHECK(R.l[0] == 0x4ffffffbu && R.l[7] == 0x0e0a77c1u);
}

int main() {
    for (uint32_t T : {2u, 4u})
        for (uint32_t u : {T, T + 1, T + 5})
            for (uint32_t E = 0; E <= u; E++) {                               // every m with sum m <= u
                Vec head(T - 1, 0);
                exhaustive(head, 0, E, u);
            }
    const unsigned long long small = g_cases;
    std::mt19937 rng(20260101u);
    for (uint32_t u : {256u, 257u, 2060u, 4099u}) corners(256, u, rng);
    values(rng);
    std::printf("permuted index check ok: %llu exhaustive cases, %llu corner and random cases\n", small, g_cases - small);
    return 0;
}
