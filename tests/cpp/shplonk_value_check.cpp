// The rules of SHPLONK's multi-point opening of device columns (csrc/hsw_shplonk_value.hpp over hsw_open_value.hpp) on
// the CPU: the launches of hsw_shplonk.hip and the scan of hsw_open.hip run thread for thread -- tiles (the load rule,
// the fold with one staged weight per column, per item Horner over a thread's rows, the workgroup scan step by step, the
// seeds and the chain of the sweeps through the item's tile cell), scan (chunks of tiles, every tile's carry-in in place
// of its sum) and write (per item the seed and the recurrence down a thread's rows, the weighted sum, ONE store per
// output cell, the chain through the item's tile cell) -- and compared with the plain definition in hsw_fr_mul.hpp
// arithmetic: the y-fold, SUCCESSIVE Kate division root after root, the v-fold; then L and the division by (X - u).
// Both cell forms; tile_rows 0 (2048), 256, 512 and 4096 (two sweeps per tile); rows around a thread's 8 rows and every
// tile size, below the number of a set's points, and with more tiles than the scan has threads; sets of (m, t) = (1, 1),
// (1, 3), (3, 2), (5, 4) and (2, 16), together and alone; columns of heights rows, rows - 1, 1 and 0; y, v among 0, 1 and
// random; a point equal to 0.  A stand-alone program: compile with -fsanitize=address,undefined and run it
// (tests/test_shplonk_host.py does).  Every column is a vector of exactly the rows that may be read, every scratch
// array of its exact size: a rule that leaves its range is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_shplonk_value.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using namespace hsw;

static unsigned long long g_runs = 0, g_rows = 0;

typedef std::vector<PFe> Column;                                // exactly the rows that may be read
struct Set { std::vector<uint32_t> cols, points; };             // indices into the columns and into T

static void load_rows(const Column &col, uint32_t row0, PFe *a) {
    for (uint32_t k = 0; k < OPEN_ROWS; k++) a[k] = row0 + k < col.size() ? col.at(row0 + k) : fr_zero();
}

// suffix_scan of the kernels: every step reads what the step before left
static void suffix_scan(std::vector<PFe> &sh, const PFe *pow, bool log, uint32_t active) {
    uint32_t k = 0;
    for (uint32_t s = 1; s < active; s <<= 1, k++) {
        const std::vector<PFe> old(sh);
        for (uint32_t t = 0; t + s < active; t++) sh[t] = open_step(old[t], pow[log ? k : s], old.at(t + s));
    }
}

// hsw_open_scan_kernel for one item: tiles[0 .. n_tiles) holds the sums, and the carry-ins afterwards
static void scan_launch(const OpenGeometry &geo, const OpenPoint &pt, PFe *tiles) {
    std::vector<PFe> sh(OPEN_THREADS, fr_zero());
    for (uint32_t t = 0; t < OPEN_THREADS; t++) {
        uint32_t lo, hi;
        open_chunk(geo, t, lo, hi);
        PFe L = fr_zero();
        for (uint32_t k = hi; k-- > lo;) L = open_step(tiles[k], pt.zt, L);
        sh[t] = L;
    }
    suffix_scan(sh, pt.zc, true, OPEN_THREADS);
    for (uint32_t t = 0; t < OPEN_THREADS; t++) {
        uint32_t lo, hi;
        open_chunk(geo, t, lo, hi);
        PFe run = t + 1 < OPEN_THREADS ? sh[t + 1] : fr_zero();
        for (uint32_t k = hi; k-- > lo;) {
            const PFe own = tiles[k];
            tiles[k] = run;
            run = open_step(own, pt.zt, run);
        }
    }
}

// what the launches are given: the staging of hsw_gadget_shplonk.cpp
struct Staged {
    std::vector<const Column *> cols;
    std::vector<uint32_t> refs;                                 // a set's columns
    std::vector<PFe> col_weights;
    struct S { uint32_t first, m, item_first, n_items; };
    std::vector<S> sets;
    std::vector<uint32_t> item_point;
    std::vector<PFe> item_weights;
    std::vector<PFe> points;                                    // Montgomery form
    bool unit;
};

// the three launches, thread for thread
static std::vector<PFe> launches(uint32_t rows, uint32_t tile_rows, const Staged &st) {
    OpenGeometry geo;
    CHECK(open_geometry(rows, tile_rows, geo));
    std::vector<OpenPoint> pts(st.points.size());
    for (size_t i = 0; i < pts.size(); i++) open_stage_point(st.points[i], geo, pts[i]);
    const size_t n_items = st.item_point.size();
    std::vector<PFe> tiles(n_items * geo.n_tiles), seeds(n_items * geo.seeds);
    std::vector<char> seeded(seeds.size(), 0);
    std::vector<Column> c_scratch(st.sets.size());
    std::vector<PFe> sh(OPEN_THREADS);
    for (size_t si = 0; si < st.sets.size(); si++) {                      // ---- tiles: a workgroup per (set, tile)
        const Staged::S &set = st.sets[si];
        if (set.m > 1) c_scratch[si].assign(rows, fr_zero());
        for (uint32_t tile = 0; tile < geo.n_tiles; tile++)
            for (uint32_t sweep = geo.sweeps; sweep-- > 0;) {
                std::vector<PFe> c((size_t)OPEN_THREADS * OPEN_ROWS, fr_zero());
                for (uint32_t t = 0; t < geo.active; t++) {
                    const uint32_t row0 = open_row0(geo, tile, sweep, t);
                    if (row0 >= rows) continue;
                    PFe *ct = &c[(size_t)t * OPEN_ROWS];
                    load_rows(*st.cols.at(st.refs.at(set.first)), row0, ct);
                    for (uint32_t i = 1; i < set.m; i++) {
                        PFe a[OPEN_ROWS];
                        load_rows(*st.cols.at(st.refs.at(set.first + i)), row0, a);
                        for (uint32_t k = 0; k < OPEN_ROWS; k++) ct[k] = shplonk_fold(ct[k], st.col_weights.at(set.first + i), a[k]);
                    }
                    if (set.m > 1)
                        for (uint32_t k = 0; k < OPEN_ROWS; k++)
                            if (row0 + k < rows) c_scratch[si].at(row0 + k) = ct[k];
                }
                for (uint32_t i = 0; i < set.n_items; i++) {
                    const uint32_t item = set.item_first + i;
                    const OpenPoint &pt = pts.at(st.item_point.at(item));
                    for (uint32_t t = 0; t < OPEN_THREADS; t++) {
                        const uint32_t row0 = open_row0(geo, tile, sweep, t);
                        sh[t] = t < geo.active && row0 < rows ? open_horner(&c[(size_t)t * OPEN_ROWS], pt.z) : fr_zero();
                    }
                    suffix_scan(sh, pt.zr, false, geo.active);
                    for (uint32_t t = 0; t < geo.active; t++) {
                        const uint32_t row0 = open_row0(geo, tile, sweep, t);
                        if (row0 >= rows) continue;
                        const size_t at = (size_t)item * geo.seeds + row0 / OPEN_ROWS;
                        CHECK(!seeded.at(at));
                        seeded[at] = 1;
                        seeds[at] = t + 1 < geo.active ? sh[t + 1] : fr_zero();
                    }
                    PFe &cell = tiles.at((size_t)item * geo.n_tiles + tile);
                    cell = sweep + 1 == geo.sweeps ? sh[0] : open_step(sh[0], pt.zr[geo.active], cell);
                }
            }
    }
    for (char s : seeded) CHECK(s);
    for (size_t item = 0; item < n_items; item++) scan_launch(geo, pts.at(st.item_point[item]), &tiles[item * geo.n_tiles]);   // ---- scan
    std::vector<PFe> out(rows, fr_zero());
    std::vector<char> written(rows, 0);
    for (uint32_t tile = 0; tile < geo.n_tiles; tile++)                   // ---- write: a workgroup per tile
        for (uint32_t sweep = geo.sweeps; sweep-- > 0;) {
            std::vector<PFe> acc((size_t)OPEN_THREADS * OPEN_ROWS, fr_zero());
            for (size_t si = 0; si < st.sets.size(); si++) {
                const Staged::S &set = st.sets[si];
                const Column &src = set.m > 1 ? c_scratch[si] : *st.cols.at(st.refs.at(set.first));
                for (uint32_t i = 0; i < set.n_items; i++) {
                    const uint32_t item = set.item_first + i;
                    const OpenPoint &pt = pts.at(st.item_point.at(item));
                    PFe &cell = tiles.at((size_t)item * geo.n_tiles + tile);
                    const PFe carry = cell;
                    PFe next = fr_zero();
                    for (uint32_t t = 0; t < OPEN_THREADS; t++) {
                        const uint32_t row0 = open_row0(geo, tile, sweep, t);
                        PFe s = fr_zero();
                        if (t < geo.active && row0 < rows) {
                            PFe c[OPEN_ROWS];
                            load_rows(src, row0, c);
                            s = open_step(seeds.at((size_t)item * geo.seeds + row0 / OPEN_ROWS), pt.zr[geo.active - 1 - t], carry);
                            for (int k = (int)OPEN_ROWS - 1; k >= 0; k--)
                                if (row0 + (uint32_t)k < rows) {
                                    PFe &a = acc[(size_t)t * OPEN_ROWS + (uint32_t)k];
                                    a = st.unit ? fr_add(a, s) : shplonk_gather(a, st.item_weights.at(item), s);
                                    s = open_step(c[k], pt.z, s);
                                }
                        }
                        if (t == 0) next = s;
                    }
                    if (geo.sweeps > 1) cell = next;
                }
            }
            for (uint32_t t = 0; t < geo.active; t++) {
                const uint32_t row0 = open_row0(geo, tile, sweep, t);
                for (uint32_t k = 0; k < OPEN_ROWS; k++)
                    if (row0 + k < rows) {
                        CHECK(!written.at(row0 + k));
                        written[row0 + k] = 1;
                        out[row0 + k] = acc[(size_t)t * OPEN_ROWS + k];
                    }
            }
        }
    for (char w : written) CHECK(w);
    g_runs++;
    g_rows += rows;
    return out;
}

static Staged stage_quotient(const std::vector<const Column *> &cols, const std::vector<Set> &sets, const std::vector<PFe> &T, const PFe &y, const PFe &v) {
    Staged st;
    st.cols = cols; st.points = T; st.unit = false;
    PFe vi = fr_one_mont();
    for (const Set &s : sets) {
        const uint32_t first = (uint32_t)st.refs.size(), item_first = (uint32_t)st.item_point.size();
        st.refs.insert(st.refs.end(), s.cols.begin(), s.cols.end());
        st.col_weights.resize(st.refs.size());
        shplonk_column_weights(fr_one_mont(), y, (uint32_t)s.cols.size(), &st.col_weights[first]);
        CHECK(s.points.size() <= SHPLONK_MAX_SET_POINTS);
        PFe zs[SHPLONK_MAX_SET_POINTS];
        for (size_t k = 0; k < s.points.size(); k++) zs[k] = T.at(s.points[k]);
        for (size_t k = 0; k < s.points.size(); k++) {
            st.item_point.push_back(s.points[k]);
            st.item_weights.push_back(fr_mont_mul(vi, shplonk_lambda(zs, (uint32_t)s.points.size(), (uint32_t)k)));
        }
        st.sets.push_back(Staged::S{first, (uint32_t)s.cols.size(), item_first, (uint32_t)s.points.size()});
        vi = fr_mont_mul(vi, v);
    }
    return st;
}

static std::vector<PFe> zd_of(const std::vector<Set> &sets, const std::vector<PFe> &T, const PFe &u) {
    std::vector<PFe> zd;
    for (const Set &s : sets) {
        std::vector<uint8_t> in_set(T.size(), 0);
        for (uint32_t t : s.points) in_set.at(t) = 1;
        zd.push_back(shplonk_vanish(u, T.data(), (uint32_t)T.size(), in_set.data()));
    }
    return zd;
}

static Staged stage_open(std::vector<const Column *> cols, const Column *h, const std::vector<Set> &sets, const std::vector<PFe> &T, const PFe &y, const PFe &v, const PFe &u) {
    Staged st;
    st.points = {u}; st.unit = true;
    const std::vector<PFe> zd = zd_of(sets, T, u);
    CHECK(!fr_is_zero(zd[0]));
    const PFe inv = fr_inv(zd[0]);
    PFe vi = fr_one_mont();
    for (size_t i = 0; i < sets.size(); i++) {
        const uint32_t first = (uint32_t)st.refs.size();
        st.refs.insert(st.refs.end(), sets[i].cols.begin(), sets[i].cols.end());
        st.col_weights.resize(st.refs.size());
        shplonk_column_weights(i ? fr_mont_mul(vi, fr_mont_mul(zd[i], inv)) : fr_one_mont(), y, (uint32_t)sets[i].cols.size(), &st.col_weights[first]);
        vi = fr_mont_mul(vi, v);
    }
    st.refs.push_back((uint32_t)cols.size());
    cols.push_back(h);
    st.cols = cols;
    st.col_weights.push_back(fr_sub(fr_zero(), fr_mont_mul(shplonk_vanish(u, T.data(), (uint32_t)T.size(), nullptr), inv)));
    st.item_point = {0};
    st.item_weights = {fr_one_mont()};
    st.sets.push_back(Staged::S{0, (uint32_t)st.refs.size(), 0, 1});
    return st;
}

// ---- the plain definition
static Column kate(const Column &c, const PFe &z) {
    Column q(c.size(), fr_zero());
    PFe s = fr_zero();
    for (size_t j = c.size(); j-- > 0;) {
        q[j] = s;
        s = fr_add(c[j], fr_mont_mul(z, s));
    }
    return q;
}
static Column fold(const std::vector<const Column *> &cols, const Set &s, const PFe &y, uint32_t rows) {
    Column c(rows, fr_zero());
    PFe w = fr_one_mont();
    for (uint32_t b : s.cols) {
        for (size_t j = 0; j < cols[b]->size(); j++) c[j] = fr_add(c[j], fr_mont_mul((*cols[b])[j], w));
        w = fr_mont_mul(w, y);
    }
    return c;
}
static Column plain_quotient(uint32_t rows, const std::vector<const Column *> &cols, const std::vector<Set> &sets, const std::vector<PFe> &T, const PFe &y, const PFe &v) {
    Column h(rows, fr_zero());
    PFe vi = fr_one_mont();
    for (const Set &s : sets) {
        Column q = fold(cols, s, y, rows);
        for (uint32_t t : s.points) q = kate(q, T[t]);                    // successive division, root after root
        for (uint32_t j = 0; j < rows; j++) h[j] = fr_add(h[j], fr_mont_mul(q[j], vi));
        vi = fr_mont_mul(vi, v);
    }
    return h;
}
static Column plain_open(uint32_t rows, const std::vector<const Column *> &cols, const Column &h, const std::vector<Set> &sets, const std::vector<PFe> &T, const PFe &y,
                         const PFe &v, const PFe &u) {
    const std::vector<PFe> zd = zd_of(sets, T, u);
    const PFe zt = shplonk_vanish(u, T.data(), (uint32_t)T.size(), nullptr), inv = fr_inv(zd[0]);
    Column L(rows, fr_zero());
    for (uint32_t j = 0; j < rows; j++) L[j] = fr_sub(fr_zero(), fr_mont_mul(h[j], zt));
    PFe vi = fr_one_mont();
    for (size_t i = 0; i < sets.size(); i++) {
        const Column c = fold(cols, sets[i], y, rows);
        const PFe w = fr_mont_mul(vi, zd[i]);
        for (uint32_t j = 0; j < rows; j++) L[j] = fr_add(L[j], fr_mont_mul(c[j], w));
        vi = fr_mont_mul(vi, v);
    }
    Column w = kate(L, u);
    for (PFe &x : w) x = fr_mont_mul(x, inv);
    return w;
}

static bool same(const Column &a, const Column &b, const char *what, uint32_t rows, uint32_t tr, int mont, int shape) {
    CHECK(a.size() == b.size());
    for (size_t j = 0; j < a.size(); j++)
        if (!fr_equal(a[j], b[j])) {
            std::fprintf(stderr, "rows %u tile_rows %u mont %d shape %d: %s[%zu] differs\n", rows, tr, mont, shape, what, j);
            return false;
        }
    return true;
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
    {   // lambda: 1 for one point; the sum over a set of two or more is 0; the definition for two points
        PFe z[4] = {random_below_p(), random_below_p(), fr_zero(), random_below_p()};
        CHECK(fr_equal(shplonk_lambda(z, 1, 0), fr_one_mont()));
        for (uint32_t t = 2; t <= 4; t++) {
            PFe sum = fr_zero();
            for (uint32_t k = 0; k < t; k++) sum = fr_add(sum, shplonk_lambda(z, t, k));
            CHECK(fr_is_zero(sum));
        }
        CHECK(fr_equal(fr_mont_mul(shplonk_lambda(z, 2, 0), fr_sub(z[0], z[1])), fr_one_mont()));
        CHECK(fr_equal(shplonk_vanish(z[0], z, 4, nullptr), fr_zero()));
        const uint8_t skip[4] = {1, 0, 1, 1};
        CHECK(fr_equal(shplonk_vanish(z[0], z, 4, skip), fr_sub(z[0], z[1])));
    }
    const PFe zero = fr_zero();
    const uint32_t T_ = OPEN_MIN_TILE_ROWS;
    const uint32_t heights[] = {1, 2, 3, 7, 8, 9, 17, 255, 256, 257, 2 * T_ + 3, 2047, 2048, 2053, 4096 + 9, 257 * T_ + 3};
    const uint32_t tile_choices[] = {0, T_, 2 * T_, 4096};
    // the shapes (m, t): five sets together, and each alone
    const uint32_t shape_m[5] = {1, 1, 3, 5, 2}, shape_t[5] = {1, 3, 2, 4, 16};
    for (uint32_t rows : heights)
        for (int mont = 0; mont < 2; mont++) {
            const bool large = rows > 5000;
            // 12 columns: heights rows, rows - 1, 1, 0 and rows again
            std::vector<Column> store(12);
            for (size_t b = 0; b < store.size(); b++) {
                const uint32_t hgt = b % 5 == 1 ? rows - 1 : b % 5 == 2 ? 1 : b % 5 == 3 ? 0 : rows;
                for (uint32_t j = 0; j < hgt; j++) store[b].push_back(random_below_p());
            }
            std::vector<const Column *> cols;
            for (const Column &col : store) cols.push_back(&col);
            std::vector<PFe> T(16);                                       // (every constant goes through open_to_mont as the host's do)
            for (PFe &z : T) z = open_to_mont(random_below_p(), mont != 0);
            T[1] = zero;                                                  // a point equal to 0
            for (int shape = 0; shape < 6; shape++) {
                if (large && shape != 0 && shape != 2) continue;
                std::vector<Set> sets;
                uint32_t next_col = 0;
                for (uint32_t i = 0; i < 5; i++) {
                    if (shape && shape - 1 != (int)i) continue;
                    Set s;
                    for (uint32_t k = 0; k < shape_m[i]; k++) s.cols.push_back(next_col++);
                    for (uint32_t k = 0; k < shape_t[i]; k++) s.points.push_back((k + i) % 16);
                    sets.push_back(s);
                }
                // T of the call: the points some set uses
                std::vector<int> remap(16, -1);
                std::vector<PFe> Tc;
                for (Set &s : sets)
                    for (uint32_t &t : s.points) {
                        if (remap[t] < 0) { remap[t] = (int)Tc.size(); Tc.push_back(T[t]); }
                        t = (uint32_t)remap[t];
                    }
                const PFe one = fr_one_mont();
                const PFe ys[3] = {open_to_mont(random_below_p(), mont != 0), zero, one}, vs[3] = {open_to_mont(random_below_p(), mont != 0), zero, one};
                for (int ci = 0; ci < (large ? 1 : 3); ci++) {
                    const PFe y = ys[ci], v = vs[(ci + (shape & 1)) % 3], u = open_to_mont(random_below_p(), mont != 0);
                    const Column h = plain_quotient(rows, cols, sets, Tc, y, v);
                    const Column w = plain_open(rows, cols, h, sets, Tc, y, v, u);
                    CHECK(fr_is_zero(w[rows - 1]) && fr_is_zero(h[rows - 1]));
                    const Staged sq = stage_quotient(cols, sets, Tc, y, v), so = stage_open(cols, &h, sets, Tc, y, v, u);
                    for (uint32_t tr : tile_choices) {
                        if (large && tr != T_) continue;
                        if (!same(launches(rows, tr, sq), h, "h", rows, tr, mont, shape)) return 1;
                        if (!same(launches(rows, tr, so), w, "w", rows, tr, mont, shape)) return 1;
                    }
                }
            }
        }
    std::printf("shplonk value check ok: %llu runs, %llu rows\n", g_runs, g_rows);
    return 0;
}
