// The launches of csrc/hsw_msm_value.hpp run on the CPU, under ASan + UBSan, against double-and-add: for every
// window_bits from 1 to the maximum, slice_rows 64, rows {0, 1, 63, 64, 65, 300}, canonical and Montgomery cells, the
// accumulate launch (a workgroup per (slice, window): chunks, digits, counting sort, buckets by the mixed formula), the
// reduce launch (the slices summed, then the weighted bucket sum BOTH ways: msm_weighted_sum and the kernel's suffix scan
// and tree over 256 places) and the finish (Horner, normalisation) give sum_j a[j] * G[j], computed term by term with
// g1_double and g1_add (tests/cpp/g1_check.cpp checks those against affine arithmetic).  The scalars hold 0, 1, r - 1,
// powers of two and equal-digit values, the bases identities, duplicates and a negated pair; the vectors are exactly
// input_rows long, so a read beyond is a sanitizer report.  Also: the library's own plan, a larger chunk than a slice
// never, a refused cell.  Stand-alone: its own main, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_msm_value.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using namespace hsw;

static uint64_t rng_state = 12345;
static uint64_t rnd() {                                                     // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static PFe random_scalar() {
    PFe a;
    do {
        for (int j = 0; j < 8; j++) a.l[j] = (uint32_t)rnd();
        a.l[7] &= 0x3fffffffu;
    } while (!pfe_below_p(a));
    return a;
}
static G1 scalar_mul(const PFe &k, const G1 &p) {                          // double-and-add, the top bit first
    G1 acc = g1_identity();
    for (int bit = 255; bit >= 0; bit--) {
        acc = g1_double(acc);
        if ((k.l[bit >> 5] >> (bit & 31)) & 1u) acc = g1_add(acc, p);
    }
    return acc;
}
static bool same_point(const G1Affine &a, const G1Affine &b) { return !std::memcmp(&a, &b, sizeof a); }

// ---- the launches, a loop per workgroup and per thread
static uint32_t accumulate(const MsmPlan &g, const std::vector<PFe> &cells, bool mont, const std::vector<G1Affine> &bases, std::vector<G1> &partial) {
    const uint32_t rows = (uint32_t)cells.size();
    uint32_t status = 0;
    for (uint32_t slice = 0; slice < g.slices; slice++)
        for (uint32_t w = 0; w < g.windows; w++) {
            const uint32_t row0 = slice * g.slice_rows;
            if (row0 >= rows) continue;
            const uint32_t row_end = rows - row0 < g.slice_rows ? rows : row0 + g.slice_rows;
            std::vector<G1> bucket(g.buckets, g1_identity());
            for (uint32_t chunk0 = row0; chunk0 < row_end; chunk0 += g.chunk_rows) {
                const uint32_t n = row_end - chunk0 < g.chunk_rows ? row_end - chunk0 : g.chunk_rows;
                uint32_t hist[MSM_THREADS] = {0}, start[MSM_THREADS];
                std::vector<uint32_t> digit_rank(n);
                std::vector<uint16_t> sorted(n, 0xffff);
                for (uint32_t l = 0; l < n; l++) {
                    PFe a;
                    uint32_t d = 0;
                    if (msm_canonical(cells[chunk0 + l], mont, a)) d = msm_digit(a, w, g.window_bits);
                    else status |= MSM_CELL_NOT_BELOW_P;
                    CHECK(d <= g.buckets);
                    digit_rank[l] = d << 16 | (d ? hist[d]++ : 0u);
                }
                for (uint32_t t = 0; t < MSM_THREADS; t++) start[t] = t ? msm_bucket_start(hist, t) : 0u;
                for (uint32_t l = 0; l < n; l++)
                    if (digit_rank[l] >> 16) sorted.at(start[digit_rank[l] >> 16] + (digit_rank[l] & 0xffffu)) = (uint16_t)l;
                for (uint32_t t = 0; t < g.buckets; t++)
                    for (uint32_t j = 0; j < hist[t + 1]; j++) {
                        const G1Affine b = bases.at(chunk0 + sorted.at(start[t + 1] + j));
                        if (!g1_affine_is_identity(b)) bucket[t] = g1_add_mixed(bucket[t], b);
                    }
            }
            for (uint32_t t = 0; t < g.buckets; t++) partial.at(msm_partial_index(g, 0, w, slice, t + 1)) = bucket[t];
        }
    return status;
}
// the kernel's way to sum_d d * B_d: suffix sums over 256 places by doubling offsets, then a tree sum
static G1 scan_and_tree(std::vector<G1> place) {
    CHECK(place.size() == MSM_THREADS);
    for (uint32_t off = 1; off < MSM_THREADS; off <<= 1) {
        std::vector<G1> next(place);
        for (uint32_t t = 0; t < MSM_THREADS; t++) next[t] = g1_add(place[t], t + off < MSM_THREADS ? place[t + off] : g1_identity());
        place.swap(next);
    }
    for (uint32_t off = MSM_THREADS / 2; off >= 1; off >>= 1)
        for (uint32_t t = 0; t < off; t++) place[t] = g1_add(place[t], place[t + off]);
    return place[0];
}
static void reduce(const MsmPlan &g, uint32_t rows, const std::vector<G1> &partial, std::vector<G1> &windows, bool both) {
    const uint32_t n_slices = msm_slices(rows, g.slice_rows);
    for (uint32_t w = 0; w < g.windows; w++) {
        std::vector<G1> place(MSM_THREADS, g1_identity());
        for (uint32_t t = 0; t < g.buckets; t++)
            for (uint32_t s = 0; s < n_slices; s++) place[t] = g1_add(place[t], partial.at(msm_partial_index(g, 0, w, s, t + 1)));
        windows[w] = msm_weighted_sum(place.data(), g.buckets);
        if (both) {
            const G1Affine a = msm_normalise(windows[w]), b = msm_normalise(scan_and_tree(place));
            CHECK(same_point(a, b));
        }
    }
}
static G1Affine run(uint32_t window_bits, uint32_t slice_rows, const std::vector<PFe> &cells, bool mont, const std::vector<G1Affine> &bases, uint32_t *status,
                    bool both) {
    MsmPlan g;
    CHECK(msm_plan((uint32_t)cells.size(), window_bits, slice_rows, g));
    CHECK(g.windows * g.window_bits >= MSM_SCALAR_BITS && (g.windows - 1) * g.window_bits < MSM_SCALAR_BITS && g.chunk_rows <= g.slice_rows);
    std::vector<G1> partial(msm_partial_points(g), G1{fq_zero(), fq_zero(), fq_zero()}), windows(g.windows);
    *status = accumulate(g, cells, mont, bases, partial);
    reduce(g, (uint32_t)cells.size(), partial, windows, both);
    return msm_normalise(msm_horner(windows.data(), g.windows, g.window_bits));
}

int main() {
    {   // ---- the plan and the digits
        MsmPlan g;
        CHECK(!msm_plan(100, 9, 0, g) && !msm_plan(100, 0, 32, g) && !msm_plan(100, 0, 96, g) && !msm_plan(100, 0, 1u << 29, g));
        CHECK(msm_plan(1u << 20, 0, 0, g) && g.window_bits == 8 && g.windows == 32 && g.buckets == 255 && g.slice_rows == 4096 && g.slices == 256 && g.chunk_rows == 4096);
        CHECK(msm_plan(1u << 28, 0, 0, g) && g.slice_rows == 1u << 18 && g.slices == 1024 && g.chunk_rows == 4096);
        CHECK(msm_plan(0, 5, 64, g) && g.windows == 51 && g.slices == 1 && g.buckets == 31 && g.chunk_rows == 64);
        CHECK(msm_plan(300, 1, 64, g) && g.windows == 254 && g.slices == 5 && g.buckets == 1);
        const PFe a = random_scalar();
        for (uint32_t c = 1; c <= MSM_MAX_WINDOW_BITS; c++) {                // the digits put together again are the scalar
            PFe back = fr_zero();
            const uint32_t W = (MSM_SCALAR_BITS + c - 1) / c;
            for (uint32_t w = 0; w < W; w++) {
                const uint32_t d = msm_digit(a, w, c);
                for (uint32_t k = 0; k < c; k++)
                    if (((d >> k) & 1u) && w * c + k < 256) back.l[(w * c + k) >> 5] |= 1u << ((w * c + k) & 31u);
            }
            CHECK(fr_equal(a, back));
        }
    }
    // ---- bases: a chain k G with G = (1, 2), then identities, duplicates and a negated pair put in
    const uint32_t N = 300;
    std::vector<G1Affine> bases(N);
    {
        const G1Affine gen{fq_to_mont(Fq{{1, 0, 0, 0, 0, 0, 0, 0}}), fq_to_mont(Fq{{2, 0, 0, 0, 0, 0, 0, 0}})};
        G1 p = scalar_mul(random_scalar(), g1_from_affine(gen));
        const G1 step = scalar_mul(random_scalar(), g1_from_affine(gen));
        for (uint32_t j = 0; j < N; j++) { bases[j] = g1_to_affine(p); p = g1_add(p, step); }
        bases[5] = G1Affine{fq_zero(), fq_zero()};
        bases[64] = G1Affine{fq_zero(), fq_zero()};
        bases[9] = bases[8];
        bases[70] = bases[8];
        bases[11] = G1Affine{bases[10].x, fq_neg(bases[10].y)};
        bases[0] = gen;
    }
    const uint32_t P_[8] = HSW_PV_P;
    unsigned runs = 0;
    const uint32_t heights[6] = {0, 1, 63, 64, 65, 300};
    for (uint32_t rows : heights) {
        std::vector<PFe> scalars(rows);                                    // canonical values
        for (uint32_t j = 0; j < rows; j++) scalars[j] = random_scalar();
        if (rows > 12) {
            scalars[1] = fr_zero();
            scalars[2] = PFe{{1, 0, 0, 0, 0, 0, 0, 0}};
            std::memcpy(&scalars[3], P_, 32); scalars[3].l[0] -= 1;          // r - 1
            scalars[4] = fr_zero(); scalars[4].l[7] = 1u << 29;              // 2^253
            for (int j = 0; j < 8; j++) scalars[6].l[j] = 0x11111111u;       // equal digits at c = 1, 2, 4, 8
            scalars[10] = scalars[11];                                       // the negated pair under one scalar
            scalars[8] = scalars[2];
        }
        G1 want = g1_identity();
        for (uint32_t j = 0; j < rows; j++) want = g1_add(want, scalar_mul(scalars[j], g1_from_affine(bases[j])));
        const G1Affine expected = msm_normalise(want);
        for (int mont = 0; mont < 2; mont++) {
            std::vector<PFe> cells(scalars);
            if (mont) for (PFe &x : cells) x = fr_to_mont(x);
            const std::vector<G1Affine> seen(bases.begin(), bases.begin() + rows);   // exactly the rows that may be read
            for (uint32_t c = 1; c <= MSM_MAX_WINDOW_BITS; c++) {
                uint32_t status = ~0u;
                const G1Affine got = run(c, 64, cells, mont != 0, seen, &status, c == 3 || c == 8);
                CHECK(status == 0 && same_point(got, expected));
                runs++;
            }
            uint32_t status = ~0u;
            CHECK(same_point(run(0, 0, cells, mont != 0, seen, &status, false), expected) && status == 0);   // the library's plan: one slice
            runs++;
            if (rows == 300) {                                               // a cell equal to r, and one with a high limb set
                for (int how = 0; how < 2; how++) {
                    std::vector<PFe> bad(cells);
                    if (how) bad[299].l[7] |= 0x80000000u; else std::memcpy(&bad[17], P_, 32);
                    (void)run(8, 64, bad, mont != 0, seen, &status, false);
                    CHECK(status == MSM_CELL_NOT_BELOW_P);
                }
            }
        }
    }
    {   // the negated pair alone under one scalar: the identity, 64 zero bytes
        std::vector<PFe> cells(12, fr_zero());
        cells[10] = cells[11] = random_scalar();
        const std::vector<G1Affine> seen(bases.begin(), bases.begin() + 12);
        uint32_t status = ~0u;
        const G1Affine got = run(8, 64, cells, false, seen, &status, true);
        const uint8_t zero[64] = {0};
        CHECK(status == 0 && !std::memcmp(&got, zero, 64));
        runs++;
    }
    std::printf("msm value check ok: %u runs\n", runs);
    return 0;
}
