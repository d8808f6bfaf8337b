// The index rules of the Fr NTT (csrc/hsw_ntt_value.hpp) on the CPU: the launches of hsw_ntt.hip run point for point --
// per launch and workgroup a tile of 1024 places, the load rule (rows beyond the height are 0, the shift from the
// windows and the tile table, the inter-launch twiddle from the table of w's powers), the steps thread by thread, the
// store rule (reversed field, digit-reversed address, scale or tile table) -- and compared with the direct sum
//   out[i] = c sum_j a[j] g^j w^(i j)     or     c g^i sum_j a[j] w^(i j)
// in hsw_fr_mul.hpp arithmetic.  Every log_n from 1 to 12, every pass_log from 1 to 10 and the default, both flags,
// input_rows in {0, 1, N - 5 where positive, N}, both cell forms; then the default plan at log_n 15 and 16, where digits
// of 8 bits (tiles of 2^8 strided x 4 adjacent cells) first appear, on sampled rows.  A stand-alone program: compile with
// -fsanitize=address,undefined and run it (tests/test_ntt_host.py does).  Every table is a vector of its exact size,
// so an index rule that leaves its range is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_ntt_value.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using namespace hsw;

static const uint32_t TILE = 1u << NTT_TILE_LOG;
static unsigned long long g_points = 0, g_transforms = 0;

static PFe pow_mont(PFe base, const uint32_t *e, int limbs) {           // base^e by square and multiply, Montgomery form
    PFe r = fr_one_mont();
    for (int bit = 32 * limbs - 1; bit >= 0; bit--) {
        r = fr_mont_mul(r, r);
        if ((e[bit >> 5] >> (bit & 31)) & 1u) r = fr_mont_mul(r, base);
    }
    return r;
}
static PFe small_mont(uint32_t x) { return fr_to_mont(PFe{{x, 0, 0, 0, 0, 0, 0, 0}}); }

// 7^((p - 1) / 2^log_n), Montgomery form
static PFe root_of_unity(uint32_t log_n) {
    const uint32_t pm1[8] = {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    uint32_t e[8];
    for (int j = 0; j < 8; j++) {
        const uint64_t two = ((uint64_t)(j < 7 ? pm1[j + 1] : 0) << 32) | pm1[j];
        e[j] = (uint32_t)(two >> log_n);
    }
    return pow_mont(small_mont(7), e, 8);
}

struct Call {
    uint32_t log_n, pass_log, flags;
    uint32_t rows;
    bool mont, has_shift, has_scale;
    PFe omega, shift, scale;                // as stored in the representation
};

// what hsw_gadget_ntt stages and what hsw_ntt_kernel does with it
static std::vector<PFe> run_launches(const Call &call, const std::vector<PFe> &in, uint32_t *launches) {
    NttPlan plan;
    CHECK(ntt_plan(call.log_n, call.pass_log, plan));
    const uint32_t L = call.log_n, N = 1u << L;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < plan.n_pass; k++) {
        CHECK(plan.bits[k] >= 1 && plan.bits[k] <= (call.pass_log ? call.pass_log : (uint32_t)NTT_TILE_LOG));
        sum += plan.bits[k];
    }
    CHECK(sum == L);
    *launches = plan.n_pass;
    const PFe omega = ntt_to_mont(call.omega, call.mont);
    CHECK(ntt_root_is_primitive(omega, L));
    const PFe shift = call.has_shift ? ntt_to_mont(call.shift, call.mont) : fr_zero();
    const PFe scale = call.has_scale ? ntt_to_mont(call.scale, call.mont) : fr_zero();
    const bool shift_in = call.has_shift && !(call.flags & NTT_SHIFT_AFTER);
    const int out_mode = call.has_shift && (call.flags & NTT_SHIFT_AFTER) ? 2 : call.has_scale ? 1 : 0;
    NttWindows wwin, gwin;
    ntt_stage_windows(omega, wwin);
    std::vector<PFe> table(N / 2 ? N / 2 : 1);
    for (uint32_t e = 0; e < table.size(); e++) table[e] = ntt_power(wwin, e);
    const NttPass pass0 = ntt_pass(plan, 0), pass_last = ntt_pass(plan, plan.n_pass - 1);
    std::vector<PFe> tile_tab(TILE);
    if (call.has_shift) {
        ntt_stage_windows(shift, gwin);
        for (uint32_t l = 0; l < TILE; l++) {
            if (shift_in) tile_tab[l] = ntt_power(gwin, ntt_offset(pass0, l));
            else {
                tile_tab[l] = ntt_power(gwin, ntt_out_index(plan, ntt_offset(pass_last, ntt_store_local(pass_last, l))) & (N - 1));
                if (call.has_scale) tile_tab[l] = fr_mont_mul(tile_tab[l], scale);
            }
        }
    }
    std::vector<PFe> scratch(plan.n_pass > 1 ? N : 0), out(N);
    std::vector<char> written(N, 0);
    std::vector<PFe> sh(TILE);
    for (uint32_t k = 0; k < plan.n_pass; k++) {
        const NttPass g = ntt_pass(plan, k);
        const bool first = k == 0, last = k + 1 == plan.n_pass;
        const uint32_t points = 1u << ntt_tile_log(g);
        CHECK(ntt_tile_log(g) <= NTT_TILE_LOG && g.field_bits >= 1 && g.field_shift + g.field_bits <= ntt_tile_log(g));
        std::vector<char> seen(N, 0);
        for (uint32_t wg = 0; wg < ntt_workgroups(g); wg++) {
            const uint32_t base = ntt_base(g, wg);
            const uint32_t done = first ? 0u : ntt_done_index(plan, k, base);
            const PFe g_base = first && shift_in ? ntt_power(gwin, base) : fr_zero();
            for (uint32_t l = 0; l < TILE; l++) {                         // load
                PFe v = fr_zero();
                if (l < points) {
                    const uint32_t addr = base + ntt_offset(g, l);
                    CHECK(addr < N && !seen[addr]);
                    seen[addr] = 1;
                    if (first) {
                        if (addr < call.rows) {
                            v = in.at(addr);
                            if (shift_in) v = fr_mont_mul(v, fr_mont_mul(g_base, tile_tab[l]));
                        }
                    } else {
                        const uint32_t I = !last ? done : ntt_done_index(plan, k, addr);
                        if (!last) CHECK(ntt_done_index(plan, k, addr) == done);
                        const uint32_t e = ntt_twiddle_exponent(g, ntt_field(g, l), I);
                        CHECK(e < N);
                        v = fr_mont_mul(scratch.at(addr), ntt_twiddle(table.data(), L, e));
                    }
                }
                sh[l] = v;
            }
            const auto step = [&](uint32_t ql, bool do_a, uint32_t fb_a, bool do_b, uint32_t fb_b) {
                std::vector<char> touched(TILE, 0);
                for (uint32_t t = 0; t < NTT_THREADS; t++) {
                    const uint32_t l0 = ntt_step_local(t, ql), q = 1u << ql;
                    CHECK(l0 + 3 * q < TILE);
                    for (uint32_t m = 0; m < 4; m++) { CHECK(!touched[l0 + m * q]); touched[l0 + m * q] = 1; }
                    PFe &x0 = sh[l0], &x1 = sh[l0 + q], &x2 = sh[l0 + 2 * q], &x3 = sh[l0 + 3 * q];
                    const uint32_t ea0 = ntt_stage_exponent(g, l0, fb_a), ea1 = ntt_stage_exponent(g, l0 + q, fb_a);
                    const uint32_t eb0 = ntt_stage_exponent(g, l0, fb_b), eb1 = ntt_stage_exponent(g, l0 + 2 * q, fb_b);
                    if (do_a) {
                        CHECK(ea0 < table.size() && ea1 < table.size());
                        ntt_butterfly(x0, x2, table.data(), ea0, fb_a != 0);
                        ntt_butterfly(x1, x3, table.data(), ea1, fb_a != 0);
                    }
                    if (do_b) {
                        CHECK(eb0 < table.size() && eb1 < table.size());
                        ntt_butterfly(x0, x1, table.data(), eb0, fb_b != 0);
                        ntt_butterfly(x2, x3, table.data(), eb1, fb_b != 0);
                    }
                }
            };
            int fb = (int)g.field_bits - 1;
            if (g.field_bits & 1u) {
                const uint32_t qh = g.field_shift + (uint32_t)fb;
                if (qh >= 1) step(qh - 1, true, (uint32_t)fb, false, 0);
                else step(0, false, 0, true, 0);
                fb--;
            }
            for (; fb >= 1; fb -= 2) step(g.field_shift + (uint32_t)fb - 1, true, (uint32_t)fb, true, (uint32_t)fb - 1);
            const PFe g_out = last && out_mode == 2 ? ntt_power(gwin, ntt_out_index(plan, base)) : fr_zero();
            for (uint32_t lam = 0; lam < points; lam++) {                 // store
                const uint32_t o = ntt_store_local(g, lam), addr = base + ntt_offset(g, o);
                CHECK(o < points && addr < N);
                PFe v = sh.at(ntt_reverse_field(g, o));
                if (!last) { scratch.at(addr) = v; continue; }
                if (out_mode == 1) v = fr_mont_mul(v, scale);
                else if (out_mode == 2) v = fr_mont_mul(v, fr_mont_mul(g_out, tile_tab[lam]));
                const uint32_t i = ntt_out_index(plan, addr);
                CHECK(i < N && !written[i]);
                written[i] = 1;
                out[i] = v;
                g_points++;
            }
        }
    }
    for (uint32_t i = 0; i < N; i++) CHECK(written[i]);
    g_transforms++;
    return out;
}

// sum_{j < rows} b[j] w^(i j) for every i, the powers of w from a table made by repeated multiplication
static std::vector<PFe> direct_sum(const std::vector<PFe> &b, uint32_t rows, const std::vector<PFe> &wpow, uint32_t N) {
    std::vector<PFe> out(N);
    for (uint32_t i = 0; i < N; i++) {
        PFe s = fr_zero();
        for (uint32_t j = 0; j < rows; j++) s = fr_add(s, fr_mont_mul(b[j], wpow[(uint32_t)(((uint64_t)i * j) & (N - 1))]));
        out[i] = s;
    }
    return out;
}

int main() {
    std::mt19937_64 rng(20261020);
    const auto random_below_p = [&]() {
        PFe x;
        do {
            for (int j = 0; j < 8; j++) x.l[j] = (uint32_t)rng();
            x.l[7] &= 0x3fffffffu;
        } while (!pfe_below_p(x));
        return x;
    };
    {   // the plans: one launch up to pass_log, the launch counts of the default, and roots that are not primitive
        NttPlan plan;
        CHECK(!ntt_plan(0, 0, plan) && !ntt_plan(29, 0, plan) && !ntt_plan(5, 11, plan));
        const uint32_t expect[29] = {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4};
        for (uint32_t L = 1; L <= 28; L++) {
            CHECK(ntt_plan(L, 0, plan) && plan.n_pass == expect[L]);
            for (uint32_t k = 0; k < plan.n_pass; k++) {
                const NttPass g = ntt_pass(plan, k);
                if (plan.n_pass > 1) CHECK(k + 1 < plan.n_pass ? g.lo_bits >= 2 : g.hi_bits >= 2 && g.lo_bits >= 2);   // runs of four cells
            }
        }
        CHECK(ntt_root_is_primitive(root_of_unity(8), 8) && !ntt_root_is_primitive(root_of_unity(7), 8) && !ntt_root_is_primitive(root_of_unity(9), 8));
        CHECK(!ntt_root_is_primitive(fr_one_mont(), 1) && ntt_root_is_primitive(root_of_unity(1), 1));
    }
    const PFe g_mont = small_mont(5), c_mont = fr_inv(small_mont(12345));
    for (uint32_t L = 1; L <= 12; L++) {
        const uint32_t N = 1u << L;
        const PFe w = root_of_unity(L);
        std::vector<PFe> wpow(N), gpow(N), in(N);
        wpow[0] = gpow[0] = fr_one_mont();
        for (uint32_t j = 1; j < N; j++) { wpow[j] = fr_mont_mul(wpow[j - 1], w); gpow[j] = fr_mont_mul(gpow[j - 1], g_mont); }
        for (uint32_t j = 0; j < N; j++) in[j] = random_below_p();
        std::vector<PFe> shifted(N);
        for (uint32_t j = 0; j < N; j++) shifted[j] = fr_mont_mul(in[j], gpow[j]);
        std::vector<uint32_t> heights = {0, 1};
        if (N > 5) heights.push_back(N - 5);
        if (N > 1) heights.push_back(N);
        for (uint32_t rows : heights) {
            // [0]: no shift, no scale; [1]: flags 0 with shift and scale; [2]: shift after, with scale
            std::vector<PFe> want[3];
            want[0] = direct_sum(in, rows, wpow, N);
            want[1] = direct_sum(shifted, rows, wpow, N);
            want[2] = want[0];
            for (uint32_t i = 0; i < N; i++) {
                want[1][i] = fr_mont_mul(want[1][i], c_mont);
                want[2][i] = fr_mont_mul(fr_mont_mul(want[2][i], gpow[i]), c_mont);
            }
            for (uint32_t pass_log = 0; pass_log <= 10; pass_log++)
                for (int mont = 0; mont < 2; mont++)
                    for (int kind = 0; kind < 4; kind++) {                // 3: shift after without a scale
                        Call call{};
                        call.log_n = L; call.pass_log = pass_log; call.rows = rows; call.mont = mont != 0;
                        call.flags = kind >= 2 ? (uint32_t)NTT_SHIFT_AFTER : 0u;
                        call.has_shift = kind != 0; call.has_scale = kind == 1 || kind == 2;
                        call.omega = mont ? w : fr_from_mont(w);
                        call.shift = mont ? g_mont : fr_from_mont(g_mont);
                        call.scale = mont ? c_mont : fr_from_mont(c_mont);
                        uint32_t launches = 0;
                        const std::vector<PFe> got = run_launches(call, in, &launches);
                        const uint32_t p = pass_log ? pass_log : 10u, s = p > 3 ? p - 2 : 1u;
                        CHECK(launches == (L <= p ? 1u : (L + s - 1) / s));
                        for (uint32_t i = 0; i < N; i++) {
                            const PFe expect = kind == 3 ? fr_mont_mul(want[0][i], gpow[i]) : want[kind][i];
                            if (!fr_equal(got[i], expect)) {
                                std::fprintf(stderr, "log_n %u pass_log %u rows %u mont %d kind %d: row %u differs\n", L, pass_log, rows, mont, kind, i);
                                return 1;
                            }
                        }
                    }
        }
    }
    // Digits of 8 bits -- a tile of 2^8 strided x 4 adjacent cells, runs of exactly four -- first appear at log_n 15
    // (digits 8, 7) and 16 (8, 8) of the default plan: every launch as above, 64 sampled rows against the direct sum
    for (uint32_t L = 15; L <= 16; L++) {
        const uint32_t N = 1u << L, rows = N - 5;
        const PFe w = root_of_unity(L);
        NttPlan plan;
        CHECK(ntt_plan(L, 0, plan) && plan.n_pass == 2 && plan.bits[0] == 8 && ntt_pass(plan, 0).lo_bits == 2 && ntt_pass(plan, 1).hi_bits == 10u - plan.bits[1]);
        std::vector<PFe> wpow(N), gpow(N), in(N);
        wpow[0] = gpow[0] = fr_one_mont();
        for (uint32_t j = 1; j < N; j++) { wpow[j] = fr_mont_mul(wpow[j - 1], w); gpow[j] = fr_mont_mul(gpow[j - 1], g_mont); }
        for (uint32_t j = 0; j < N; j++) in[j] = random_below_p();
        std::vector<uint32_t> sample = {0, 1, N / 2, N - 1};
        while (sample.size() < 64) sample.push_back((uint32_t)rng() & (N - 1));
        for (int mont = 0; mont < 2; mont++)
            for (int kind = 1; kind <= 2; kind++) {                       // flags 0 and shift after, both with shift and scale
                Call call{};
                call.log_n = L; call.pass_log = 0; call.rows = rows; call.mont = mont != 0;
                call.flags = kind == 2 ? (uint32_t)NTT_SHIFT_AFTER : 0u;
                call.has_shift = call.has_scale = true;
                call.omega = mont ? w : fr_from_mont(w);
                call.shift = mont ? g_mont : fr_from_mont(g_mont);
                call.scale = mont ? c_mont : fr_from_mont(c_mont);
                uint32_t launches = 0;
                const std::vector<PFe> got = run_launches(call, in, &launches);
                CHECK(launches == 2);
                for (uint32_t i : sample) {
                    PFe s = fr_zero();
                    for (uint32_t j = 0; j < rows; j++) {
                        const PFe term = fr_mont_mul(in[j], wpow[(uint32_t)(((uint64_t)i * j) & (N - 1))]);
                        s = fr_add(s, kind == 1 ? fr_mont_mul(term, gpow[j]) : term);
                    }
                    if (kind == 2) s = fr_mont_mul(s, gpow[i]);
                    CHECK(fr_equal(got[i], fr_mont_mul(s, c_mont)));
                }
            }
    }
    std::printf("ntt value check ok: %llu points, %llu transforms\n", g_points, g_transforms);
    return 0;
}
