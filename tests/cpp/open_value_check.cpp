// The rules of evaluating and opening device columns (csrc/hsw_open_value.hpp) on the CPU: the launches of hsw_open.hip
// run thread for thread -- tiles (the load rule: rows at and beyond a column's height are 0 and are not read; the fold;
// Horner over a thread's rows; the workgroup scan step by step; the seeds, the sweeps' chain and the tile's sum), scan
// (chunks of tiles, the workgroup scan, every tile's carry-in in place of its sum) and write (the seed, q[j] = s[j+1]
// down a thread's rows, the chain through thread 0) -- and compared with the plain recurrence
//   c[j] = fold over the group's columns,   s[j] = c[j] + z s[j+1],   q[j] = s[j+1],   c(z) = s[0]
// in hsw_fr_mul.hpp arithmetic.  Both cell forms; tile_rows 0 (2048), 256, 512 and 4096 (two sweeps per tile); rows
// around a thread's 8 rows, around every tile size, 2 T + 3, and sizes with more tiles than the scan has threads (chunks
// of 2 and 3 tiles, the last chunk short); groups of 1 and 3 columns with heights 0, 1, rows - 1 and rows, the tallest
// first and last; z and v among 0, 1, p - 1 and random.  A stand-alone program: compile with
// -fsanitize=address,undefined and run it (tests/test_open_host.py does).  Every column is a vector of exactly the rows
// that may be read, every scratch array of its exact size: a rule that leaves its range is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_open_value.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using namespace hsw;

static unsigned long long g_runs = 0, g_rows = 0;

struct Column { std::vector<PFe> cells; };                      // exactly the rows that may be read

static void load_rows(const Column &col, uint32_t row0, PFe *a) {
    for (uint32_t k = 0; k < OPEN_ROWS; k++) a[k] = row0 + k < col.cells.size() ? col.cells.at(row0 + k) : fr_zero();
}

// suffix_scan of hsw_open.hip: every step reads what the step before left
static void suffix_scan(std::vector<PFe> &sh, const PFe *pow, bool log, uint32_t active) {
    uint32_t k = 0;
    for (uint32_t s = 1; s < active; s <<= 1, k++) {
        const std::vector<PFe> old(sh);
        for (uint32_t t = 0; t + s < active; t++) sh[t] = open_step(old[t], pow[log ? k : s], old.at(t + s));
    }
}

// the scan launch for one item: tiles holds the sums, and the carry-ins afterwards; returns s[0]
static PFe scan_launch(const OpenGeometry &geo, const OpenPoint &pt, std::vector<PFe> &tiles) {
    CHECK(tiles.size() == geo.n_tiles);
    std::vector<PFe> sh(OPEN_THREADS, fr_zero());
    uint32_t covered = 0;
    for (uint32_t t = 0; t < OPEN_THREADS; t++) {
        uint32_t lo, hi;
        open_chunk(geo, t, lo, hi);
        CHECK(lo <= hi && hi <= geo.n_tiles && lo == covered);
        covered = hi;
        PFe L = fr_zero();
        for (uint32_t k = hi; k-- > lo;) L = open_step(tiles.at(k), pt.zt, L);
        sh[t] = L;
    }
    CHECK(covered == geo.n_tiles);
    suffix_scan(sh, pt.zc, true, OPEN_THREADS);
    PFe eval = fr_zero();
    for (uint32_t t = 0; t < OPEN_THREADS; t++) {
        uint32_t lo, hi;
        open_chunk(geo, t, lo, hi);
        PFe run = t + 1 < OPEN_THREADS ? sh[t + 1] : fr_zero();
        for (uint32_t k = hi; k-- > lo;) {
            const PFe own = tiles.at(k);
            tiles.at(k) = run;
            run = open_step(own, pt.zt, run);
        }
        if (t == 0) eval = run;
    }
    return eval;
}

struct Opened { std::vector<PFe> q; PFe eval; };

// what hsw_gadget_open stages and what the three launches do with it, for one group
static Opened open_launches(uint32_t rows, uint32_t tile_rows, bool mont, const std::vector<const Column *> &cols, const PFe &z_stored, const PFe &v_stored) {
    OpenGeometry geo;
    CHECK(open_geometry(rows, tile_rows, geo));
    CHECK(geo.active * OPEN_ROWS * geo.sweeps == geo.tile_rows && geo.active <= OPEN_THREADS && (uint64_t)geo.n_tiles * geo.tile_rows >= rows);
    CHECK((uint64_t)(geo.n_tiles - 1) * geo.tile_rows < rows && (uint64_t)geo.chunk * OPEN_THREADS >= geo.n_tiles);
    OpenPoint pt;
    open_stage_point(open_to_mont(z_stored, mont), geo, pt);
    const PFe v = open_to_mont(v_stored, mont);
    const uint32_t m = (uint32_t)cols.size();
    std::vector<PFe> c_scratch(m > 1 ? rows : 0), seeds(geo.seeds), tiles(geo.n_tiles);
    std::vector<char> seeded(geo.seeds, 0);
    std::vector<PFe> sh(OPEN_THREADS);
    for (uint32_t tile = 0; tile < geo.n_tiles; tile++) {                 // ---- tiles
        PFe carry = fr_zero();
        for (uint32_t sweep = geo.sweeps; sweep-- > 0;) {
            for (uint32_t t = 0; t < OPEN_THREADS; t++) {
                const uint32_t row0 = open_row0(geo, tile, sweep, t);
                sh[t] = fr_zero();
                if (!(t < geo.active && row0 < rows)) continue;
                PFe c[OPEN_ROWS];
                for (uint32_t i = 0; i < m; i++) {
                    PFe a[OPEN_ROWS];
                    load_rows(*cols[i], row0, a);
                    for (uint32_t k = 0; k < OPEN_ROWS; k++) c[k] = i ? open_fold(c[k], v, a[k]) : a[k];
                }
                if (m > 1)
                    for (uint32_t k = 0; k < OPEN_ROWS; k++)
                        if (row0 + k < rows) c_scratch.at(row0 + k) = c[k];
                sh[t] = open_horner(c, pt.z);
            }
            suffix_scan(sh, pt.zr, false, geo.active);
            for (uint32_t t = 0; t < geo.active; t++) {
                const uint32_t row0 = open_row0(geo, tile, sweep, t);
                if (row0 >= rows) continue;
                CHECK(!seeded.at(row0 / OPEN_ROWS));
                seeded[row0 / OPEN_ROWS] = 1;
                seeds[row0 / OPEN_ROWS] = t + 1 < geo.active ? sh[t + 1] : fr_zero();
            }
            carry = sweep + 1 == geo.sweeps ? sh[0] : open_step(sh[0], pt.zr[geo.active], carry);
        }
        tiles[tile] = carry;
    }
    for (char s : seeded) CHECK(s);
    Opened out;
    out.eval = scan_launch(geo, pt, tiles);                               // ---- scan
    out.q.assign(rows, fr_zero());
    std::vector<char> written(rows, 0);
    Column folded;
    folded.cells = c_scratch;
    const Column &src = m > 1 ? folded : *cols[0];
    for (uint32_t tile = 0; tile < geo.n_tiles; tile++) {                 // ---- write
        PFe carry = tiles[tile];
        for (uint32_t sweep = geo.sweeps; sweep-- > 0;) {
            PFe next = fr_zero();
            for (uint32_t t = 0; t < geo.active; t++) {
                const uint32_t row0 = open_row0(geo, tile, sweep, t);
                PFe s = fr_zero();
                if (row0 < rows) {
                    PFe c[OPEN_ROWS];
                    load_rows(src, row0, c);
                    s = open_step(seeds.at(row0 / OPEN_ROWS), pt.zr[geo.active - 1 - t], carry);
                    for (int k = (int)OPEN_ROWS - 1; k >= 0; k--)
                        if (row0 + (uint32_t)k < rows) {
                            CHECK(!written[row0 + (uint32_t)k]);
                            written[row0 + (uint32_t)k] = 1;
                            out.q[row0 + (uint32_t)k] = s;
                            s = open_step(c[k], pt.z, s);
                        }
                }
                if (t == 0) next = s;
            }
            carry = next;
        }
    }
    for (char w : written) CHECK(w);
    g_runs++;
    g_rows += rows;
    return out;
}

// the two launches of hsw_gadget_evaluate for one column and its points
static std::vector<PFe> evaluate_launches(uint32_t rows, uint32_t tile_rows, bool mont, const Column &col, const std::vector<PFe> &z_stored) {
    OpenGeometry geo;
    CHECK(open_geometry(rows, tile_rows, geo));
    std::vector<OpenPoint> pts(z_stored.size());
    for (size_t i = 0; i < pts.size(); i++) open_stage_point(open_to_mont(z_stored[i], mont), geo, pts[i]);
    std::vector<std::vector<PFe>> tiles(pts.size(), std::vector<PFe>(geo.n_tiles));
    std::vector<PFe> sh(OPEN_THREADS);
    for (uint32_t tile = 0; tile < geo.n_tiles; tile++)
        for (uint32_t sweep = geo.sweeps; sweep-- > 0;)
            for (size_t i = 0; i < pts.size(); i++) {
                for (uint32_t t = 0; t < OPEN_THREADS; t++) {
                    const uint32_t row0 = open_row0(geo, tile, sweep, t);
                    sh[t] = fr_zero();
                    if (!(t < geo.active && row0 < rows)) continue;
                    PFe a[OPEN_ROWS];
                    load_rows(col, row0, a);
                    sh[t] = open_horner(a, pts[i].z);
                }
                suffix_scan(sh, pts[i].zr, false, geo.active);
                tiles[i][tile] = sweep + 1 == geo.sweeps ? sh[0] : open_step(sh[0], pts[i].zr[geo.active], tiles[i][tile]);
            }
    std::vector<PFe> out;
    for (size_t i = 0; i < pts.size(); i++) out.push_back(scan_launch(geo, pts[i], tiles[i]));
    g_runs++;
    g_rows += rows;
    return out;
}

// the plain recurrence
static Opened plain(uint32_t rows, bool mont, const std::vector<const Column *> &cols, const PFe &z_stored, const PFe &v_stored) {
    const PFe z = open_to_mont(z_stored, mont), v = open_to_mont(v_stored, mont);
    std::vector<PFe> c(rows, fr_zero());
    for (uint32_t j = 0; j < rows; j++)
        for (size_t i = 0; i < cols.size(); i++) {
            const PFe a = j < cols[i]->cells.size() ? cols[i]->cells[j] : fr_zero();
            c[j] = i ? fr_add(fr_mont_mul(c[j], v), a) : a;
        }
    Opened out;
    out.q.assign(rows, fr_zero());
    PFe s = fr_zero();                                                     // s[rows]
    for (uint32_t j = rows; j-- > 0;) {
        out.q[j] = s;
        s = fr_add(c[j], fr_mont_mul(z, s));
    }
    out.eval = s;
    return out;
}

int main() {
    std::mt19937_64 rng(20261021);
    const auto random_below_p = [&]() {
        PFe x;
        do {
            for (int j = 0; j < 8; j++) x.l[j] = (uint32_t)rng();
            x.l[7] &= 0x3fffffffu;
        } while (!pfe_below_p(x));
        return x;
    };
    {   // the geometry and the staged powers
        OpenGeometry geo;
        CHECK(!open_geometry(0, 0, geo) && !open_geometry((1ull << 28) + 1, 0, geo) && open_geometry(1ull << 28, 0, geo) && geo.n_tiles == 1u << 17 && geo.chunk == 512);
        CHECK(!open_geometry(100, 128, geo) && !open_geometry(100, 384, geo) && !open_geometry(100, 1u << 21, geo) && open_geometry(100, 1u << 20, geo) && geo.sweeps == 512);
        CHECK(open_geometry(100, 0, geo) && geo.tile_rows == 2048 && geo.active == 256 && geo.sweeps == 1 && geo.n_tiles == 1 && geo.seeds == 13);
        CHECK(open_geometry(100, 256, geo) && geo.active == 32 && geo.sweeps == 1);
        CHECK(open_geometry(257 * 256 + 5, 256, geo) && geo.n_tiles == 258 && geo.chunk == 2);
        const PFe z = random_below_p();
        OpenPoint pt;
        open_stage_point(z, geo, pt);
        PFe x = fr_one_mont();
        for (uint32_t k = 0; k < 8; k++) x = fr_mont_mul(x, z);
        CHECK(fr_equal(pt.zr[0], fr_one_mont()) && fr_equal(pt.zr[1], x) && fr_equal(pt.zr[256], open_power(z, 2048)));
        CHECK(fr_equal(pt.zt, open_power(z, 256)) && fr_equal(pt.zc[0], open_power(z, 512)) && fr_equal(pt.zc[7], open_power(z, 512 * 128)));
    }
    const PFe zero = fr_zero(), one_c = PFe{{1, 0, 0, 0, 0, 0, 0, 0}};
    const uint32_t T = OPEN_MIN_TILE_ROWS, R = OPEN_ROWS;
    const uint32_t heights[] = {1, 2, 3, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 3, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 257 * T + 5, 513 * T + 1};
    const uint32_t tile_choices[] = {0, T, 2 * T, 4096};
    for (uint32_t rows : heights)
        for (int mont = 0; mont < 2; mont++) {
            const PFe one = mont ? fr_one_mont() : one_c, pm1 = fr_sub(zero, one);
            // columns of heights rows, rows - 1, 1 and 0, with 0, 1 and p - 1 among the cells
            Column full, shorter, single, empty;
            for (uint32_t j = 0; j < rows; j++) full.cells.push_back(random_below_p());
            for (uint32_t j = 0; j + 1 < rows; j++) shorter.cells.push_back(random_below_p());
            single.cells.push_back(random_below_p());
            full.cells[0] = pm1;
            if (rows > 2) { full.cells[1] = zero; full.cells[rows - 1] = one; }
            const PFe zr = random_below_p(), vr = random_below_p();
            const PFe zs[4] = {zr, zero, one, pm1}, vs[3] = {vr, zero, one};
            const std::vector<const Column *> groups[5] = {{&full}, {&shorter}, {&full, &single, &shorter}, {&empty, &shorter, &full}, {&empty}};
            const bool large = rows > 5000;
            for (int gi = 0; gi < 5; gi++)
                for (int zi = 0; zi < (large ? 1 : 4); zi++)
                    for (int vi = 0; vi < (large || groups[gi].size() == 1 ? 1 : 3); vi++) {
                        if (large && gi != 0 && gi != 2) continue;
                        const Opened want = plain(rows, mont != 0, groups[gi], zs[zi], vs[vi]);
                        CHECK(fr_is_zero(want.q[rows - 1]));
                        for (uint32_t tr : tile_choices) {
                            if (large && tr != T && tr != 0) continue;
                            const Opened got = open_launches(rows, tr, mont != 0, groups[gi], zs[zi], vs[vi]);
                            if (!fr_equal(got.eval, want.eval)) {
                                std::fprintf(stderr, "rows %u tile_rows %u mont %d group %d z %d v %d: c(z) differs\n", rows, tr, mont, gi, zi, vi);
                                return 1;
                            }
                            for (uint32_t j = 0; j < rows; j++)
                                if (!fr_equal(got.q[j], want.q[j])) {
                                    std::fprintf(stderr, "rows %u tile_rows %u mont %d group %d z %d v %d: q[%u] differs\n", rows, tr, mont, gi, zi, vi, j);
                                    return 1;
                                }
                        }
                    }
            // evaluate: one pass over a column for four points
            const std::vector<PFe> points = {zr, zero, one, pm1};
            for (const Column *col : {&full, &shorter, &empty}) {
                if (large && col != &full) continue;
                for (uint32_t tr : tile_choices) {
                    if (large && tr != T && tr != 0) continue;
                    const std::vector<PFe> got = evaluate_launches(rows, tr, mont != 0, *col, points);
                    for (size_t i = 0; i < points.size(); i++) CHECK(fr_equal(got[i], plain(rows, mont != 0, {col}, points[i], zero).eval));
                }
            }
        }
    std::printf("open value check ok: %llu runs, %llu rows\n", g_runs, g_rows);
    return 0;
}
