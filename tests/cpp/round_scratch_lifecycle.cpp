// The calls of the proving round on ONE gadget, one after the other, under AddressSanitizer + UBSan + LeakSanitizer
// against the stand-in HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing): they share one
// scratch (hsw_gadget::scratch), so an upload or a read-back longer than what the call reserved is an ordinary ASan
// report.  The sequence starts and ends with the same small call and mixes small and large needs so that the scratch
// is replaced several times.  Checked here: one device allocation for the scratch whatever ran (and one per twiddle
// table of the NTT); a call that needs no more than the scratch holds allocates nothing; a refused call of every family
// allocates nothing and launches nothing; the launches per call are those of the family's own lifecycle program;
// nothing is left at the end.  The columns are addresses only: no launch runs, so nothing reads them.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_gadget.hpp"
#include "../../halo2-dynamic-sha256_amd/csrc/hsw_ntt_value.hpp"
#include "../../include/hsw.h"

extern "C" {
size_t hip_stub_live_device_allocations();
size_t hip_stub_live_pinned_allocations();
size_t hip_stub_live_events();
int hip_stub_launches();
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using hsw::PFe;

// 7^((p - 1) / 2^log_n) as a canonical cell: a primitive 2^log_n-th root of unity
static PFe root(uint32_t log_n) {
    uint32_t e[8] = {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};   // p - 1
    for (uint32_t k = 0; k < log_n; k++)
        for (int j = 0; j < 8; j++) e[j] = (e[j] >> 1) | (j < 7 ? e[j + 1] << 31 : 0);
    const PFe seven = hsw::fr_to_mont(PFe{{7, 0, 0, 0, 0, 0, 0, 0}});
    PFe r = hsw::fr_one_mont();
    for (int bit = 255; bit >= 0; bit--) {
        r = hsw::fr_mont_mul(r, r);
        if ((e[bit >> 5] >> (bit & 31)) & 1u) r = hsw::fr_mont_mul(r, seven);
    }
    return hsw::fr_from_mont(r);
}

// device addresses that overlap nothing: `cells` cells each, one after the other
static uintptr_t g_at = 0x100000000000ull;
static void *column(uint64_t cells) {
    void *p = reinterpret_cast<void *>(g_at);
    g_at += 32 * cells + 4096;
    return p;
}
static std::vector<const void *> columns(size_t n, uint64_t cells) {
    std::vector<const void *> v;
    for (size_t i = 0; i < n; i++) v.push_back(column(cells));
    return v;
}
static std::vector<void *> outputs(size_t n, uint64_t cells) {
    std::vector<void *> v;
    for (size_t i = 0; i < n; i++) v.push_back(column(cells));
    return v;
}

static hsw_gadget *g = nullptr;
static size_t live0 = 0, tables = 0, growths = 0;

// what a call may do to the scratch: replace it by a larger one (GROWS), or leave it as it is (STAYS, REFUSED: and launch nothing)
enum Want { GROWS, STAYS, REFUSED };
struct Watch {
    Want want;
    int launches, l0;
    void *d;
    size_t cap, live;
    Watch(Want w, int n) : want(w), launches(n), l0(hip_stub_launches()), d(g->scratch.d), cap(g->scratch.cap), live(hip_stub_live_device_allocations()) {}
    bool ok(int rc) const {
        if (check(rc)) return true;
        std::fprintf(stderr, "status %d (%s), %d launches, scratch %zu -> %zu bytes, %zu device allocations\n", rc, rc == HSW_OK ? "" : hsw_last_error(g->ctx->engine),
                     hip_stub_launches() - l0, cap, g->scratch.cap, hip_stub_live_device_allocations());
        return false;
    }
    bool check(int rc) const {
        const hsw::DeviceScratch &s = g->scratch;
        if (want == REFUSED) return rc != HSW_OK && hip_stub_launches() == l0 && s.d == d && s.cap == cap && hip_stub_live_device_allocations() == live;
        if (rc != HSW_OK || hip_stub_launches() != l0 + launches || !s.d) return false;
        if (hip_stub_live_device_allocations() != live0 + 1 + tables) return false;       // the scratch, and the twiddle tables so far
        if (want == STAYS) return s.d == d && s.cap == cap;
        growths++;
        return s.cap > cap;
    }
};

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    const size_t sizes[1] = {128};
    CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);      // one Context, two chip columns: two spread arguments
    live0 = hip_stub_live_device_allocations();
    CHECK(!g->scratch.d && g->scratch.cap == 0);
    uint64_t ch[2][4] = {{5, 0, 0, 0}, {9, 9, 0, 0}};
    const uint64_t omega3[4] = {3, 0, 0, 0};
    uint32_t status[8];

    // ---- the lookup argument's grand product, the small call the sequence starts and ends with: it makes the scratch
    const std::vector<const void *> p_in = columns(2, 1000), p_spread = columns(2, 1000), p_pin = columns(2, 1000), p_ptab = columns(2, 1000);
    const std::vector<void *> p_z = outputs(2, 1001);
    const hsw_lookup_product pa{HSW_LOOKUP_SPREAD, 0, 1000, 2, p_in.data(), p_spread.data(), nullptr, p_pin.data(), p_ptab.data(), p_z.data(), ch, ch, ch, status};
    hsw_product_report prep;
    {
        const Watch w(GROWS, 3);
        CHECK(w.ok(hsw_gadget_lookup_product(g, &pa, &prep)) && prep.arguments == 2 && prep.written == 2 * 1001 && prep.first_open == ~0ull && prep.first_refused == ~0ull);
    }
    const size_t small_cap = g->scratch.cap;
    {
        hsw_lookup_product bad = pa; bad.n_arguments = 1;
        hsw_product_report rep;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_lookup_product(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "n_arguments"));
    }

    // ---- evaluate and open: 2 columns of 300 rows; 2 queries, 2 groups of one column
    const std::vector<const void *> o_in = columns(2, 300);
    const std::vector<void *> o_quot = outputs(2, 300);
    std::vector<uint8_t> o_points(64, 0), o_chal(64, 0), o_evals(64, 0);
    o_points[0] = 2; o_points[32] = 3; o_chal[0] = 4; o_chal[32] = 5;
    const uint32_t o_qc[2] = {0, 1}, o_qp[2] = {0, 1}, o_gcols[2] = {0, 1};
    const uint64_t o_gfirst[3] = {0, 1, 2};
    const hsw_evaluate ev{0, 0, 300, 2, o_in.data(), nullptr, 2, o_points.data(), 2, o_qc, o_qp, o_evals.data(), status};
    const hsw_open op{0, 0, 300, 2, o_in.data(), nullptr, 2, o_gfirst, o_gcols, o_points.data(), o_chal.data(), o_quot.data(), o_evals.data(), status};
    hsw_evaluate_report erep;
    hsw_open_report orep;
    {
        const Watch w(GROWS, 2);
        CHECK(w.ok(hsw_gadget_evaluate(g, &ev, &erep)) && erep.launches == 2 && erep.queries == 2);
    }
    {
        hsw_evaluate bad = ev; bad.flags = 1;
        hsw_evaluate_report rep;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_evaluate(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "unknown flag"));
        hsw_open bad_open = op; bad_open.d_quotients = nullptr;
        CHECK(w.ok(hsw_gadget_open(g, &bad_open, &orep)) && std::strstr(hsw_last_error(e), "quotient pointer array"));
    }

    // ---- the permuted lookup columns: the spread arguments of a pass with nothing digested (zero, prepare, values, write)
    {
        const std::vector<void *> in = outputs(2, 1000), tab = outputs(2, 1000);
        const hsw_lookup_permuted a{HSW_LOOKUP_SPREAD, 0, 1000, 2, in.data(), tab.data(), ch, nullptr, 0};
        hsw_permuted_report rep;
        {
            const Watch w(STAYS, 4);
            CHECK(w.ok(hsw_gadget_lookup_permuted(g, &a, &rep)) && rep.arguments == 2 && rep.entries == 0 && rep.written == 2 * 1000 * 2);
        }
        hsw_lookup_permuted bad = a; bad.usable_rows = 255;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_lookup_permuted(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "below the table size"));
    }

    // ---- the permutation argument's grand products: 5 columns in sets of 2, 3000 rows
    {
        const std::vector<const void *> v = columns(5, 3000), sigma = columns(5, 3000);
        const std::vector<void *> z = outputs(3, 3001);
        const hsw_permutation_product a{0, 2, 3000, 5, v.data(), nullptr, sigma.data(), z.data(), ch, ch, omega3, ch[1], status};
        hsw_permutation_report rep;
        {
            const Watch w(STAYS, 3);
            CHECK(w.ok(hsw_gadget_permutation_product(g, &a, &rep)) && rep.proofs == 1 && rep.products == 3 && rep.written == 3 * 3001);
        }
        hsw_permutation_product bad = a; bad.chunk_columns = 0;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_permutation_product(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "at least 1"));
    }

    // ---- the NTT: two launches at log_n = 11, so the points of both columns lie in the scratch; the first twiddle table
    hsw_ntt_report nrep;
    {
        const std::vector<const void *> in = columns(2, 1 << 11);
        const std::vector<void *> out = outputs(2, 1 << 11);
        const PFe w11 = root(11);
        const hsw_ntt a{0, 11, 0, 0, 2, in.data(), nullptr, out.data(), &w11, nullptr, nullptr, status};
        {
            tables = 1;
            const Watch w(GROWS, 1 + 2);
            CHECK(w.ok(hsw_gadget_ntt(g, &a, &nrep)) && nrep.launches == 2 && nrep.scratch_bytes == 2 * (32ull << 11));
            CHECK(hip_stub_live_device_allocations() == live0 + 2);
        }
        hsw_ntt bad = a; bad.log_n = 29;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_ntt(g, &bad, &nrep)) && std::strstr(hsw_last_error(e), "log_n is 1 .. 28"));
    }

    // ---- the commitments: 3 columns over 300 bases (check, accumulate, reduce): the partial buckets need more
    {
        const std::vector<const void *> in = columns(3, 300);
        const void *bases = column(2 * 300);
        std::vector<uint8_t> out(64 * 3, 0);
        const hsw_msm a{0, 0, 0, 0, 3, 300, bases, in.data(), nullptr, out.data(), status};
        hsw_msm_report rep;
        {
            const Watch w(GROWS, 3);
            CHECK(w.ok(hsw_gadget_msm(g, &a, &rep)) && rep.columns == 3 && rep.launches == 3 && rep.scratch_bytes > 2 * (32ull << 11));
        }
        hsw_msm bad = a; bad.n_bases = 0;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_msm(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "n_bases is 1 .. 2^28"));
    }

    // ---- open (tiles, scan, write), after something larger
    {
        const Watch w(STAYS, 3);
        CHECK(w.ok(hsw_gadget_open(g, &op, &orep)) && orep.groups == 2 && orep.launches == 3 && orep.batches == 1 && orep.written == 600);
    }

    // ---- SHPLONK, both calls: the sets ({0, 1} at {z0}), ({2} at {z0, z1}), ({3} at {z0, z1, z2})
    {
        const std::vector<const void *> in = columns(4, 300);
        std::vector<uint8_t> points(96, 0), y(32, 0), v(32, 0), u(32, 0);
        points[0] = 2; points[32] = 3; points[64] = 4; y[0] = 7; v[0] = 9; u[0] = 11;
        const uint64_t first[4] = {0, 2, 3, 4}, pfirst[4] = {0, 1, 3, 6};
        const uint32_t cols[4] = {0, 1, 2, 3}, pts[6] = {0, 0, 1, 0, 1, 2};
        const hsw_shplonk q{0, 0, 300, 4, in.data(), nullptr, 3, points.data(), 3, first, cols, pfirst, pts, y.data(), v.data(), nullptr, nullptr, column(300), status};
        hsw_shplonk o = q;
        o.u = u.data(); o.d_h = column(300);
        hsw_shplonk_report rep;
        {
            const Watch w(STAYS, 3);
            CHECK(w.ok(hsw_gadget_shplonk_quotient(g, &q, &rep)) && rep.sets == 3 && rep.items == 6 && rep.columns == 4 && rep.launches == 3 && rep.written == 300);
        }
        {
            const Watch w(STAYS, 3);
            CHECK(w.ok(hsw_gadget_shplonk_open(g, &o, &rep)) && rep.sets == 3 && rep.columns == 5 && rep.launches == 3 && rep.written == 300);
        }
        hsw_shplonk bad = q; bad.n_sets = 0;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_shplonk_quotient(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "n_sets is at least 1"));
        bad = o; bad.u = nullptr;
        CHECK(w.ok(hsw_gadget_shplonk_open(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "u is NULL"));
    }

    // ---- the quotient: 2 proofs of 3 own and 2 shared columns on a coset of 2^6 rows -- two gates, a permutation of 3
    //      columns in sets of 2, two lookups (gates, permutation, lookups, finish)
    {
        const size_t K = 2;
        const uint64_t N = 64;
        const std::vector<const void *> cols = columns(K * 3, N), fixed = columns(2, N), sigmas = columns(3, N), pz = columns(K * 2, N), la = columns(K * 2, N),
                                        ls = columns(K * 2, N), lz = columns(K * 2, N);
        const std::vector<void *> h = outputs(K, N);
        const uint32_t gft[3] = {0, 3, 4}, tff[5] = {0, 2, 4, 6, 6}, fcol[6] = {3, 0, 3, 0, 3, 0}, perm[3] = {0, 4, 2}, fi[3] = {0, 1, 3}, fin[3] = {2, 0, 4}, ft[3] = {0, 1, 3},
                       ftab[3] = {3, 4, 1};
        const int32_t frot[6] = {0, 0, 0, 1, 0, 3};
        std::vector<uint8_t> coeffs(32 * 4, 0), ys(32 * K, 0), betas(32 * K, 0), gammas(32 * K, 0), thetas(32 * K, 0), zeta(32, 0), delta(32, 0);
        for (size_t t = 0; t < 4; t++) coeffs[32 * t] = (uint8_t)(t + 1);
        for (size_t k = 0; k < K; k++) { ys[32 * k] = 2; betas[32 * k] = 3; gammas[32 * k] = 4; thetas[32 * k] = 5; }
        zeta[0] = 5; delta[0] = 7;
        const PFe w6 = root(6);
        hsw_quotient a{};
        a.log_rows = 4; a.log_n = 6; a.chunk_columns = 2; a.usable_rows = 10;
        a.n_proofs = K; a.n_columns = 3; a.n_fixed = 2;
        a.d_columns = cols.data(); a.d_fixed = fixed.data(); a.d_l0 = column(N); a.d_l_last = column(N); a.d_l_active = column(N);
        a.gates = hsw_quotient_gates{2, 4, 6, gft, coeffs.data(), tff, fcol, frot};
        a.n_perm_columns = 3; a.perm_columns = perm; a.d_sigmas = sigmas.data(); a.d_perm_products = pz.data();
        a.lookups = hsw_quotient_lookups{2, fi, fin, ft, ftab, la.data(), ls.data(), lz.data(), thetas.data()};
        a.betas = betas.data(); a.gammas = gammas.data(); a.ys = ys.data();
        a.omega_ext = &w6; a.zeta = zeta.data(); a.delta = delta.data();
        a.d_h = h.data(); a.status = status;
        hsw_quotient_report rep;
        {
            const Watch w(STAYS, 4);
            CHECK(w.ok(hsw_gadget_quotient(g, &a, &rep)) && rep.proofs == 2 && rep.launches == 4 && rep.written == 128 && rep.expressions == 2 + 5 + 10);
            CHECK(rep.scratch_bytes == 2 * 64 * 32);
        }
        hsw_quotient bad = a; bad.n_proofs = 0;
        const Watch w(REFUSED, 0);
        CHECK(w.ok(hsw_gadget_quotient(g, &bad, &rep)) && std::strstr(hsw_last_error(e), "n_proofs is at least 1"));
    }

    // ---- the largest need of the sequence: the NTT at log_n = 16, and a second twiddle table
    {
        const std::vector<const void *> in = columns(2, 1 << 16);
        const std::vector<void *> out = outputs(2, 1 << 16);
        const PFe w16 = root(16);
        const hsw_ntt a{0, 16, 0, 0, 2, in.data(), nullptr, out.data(), &w16, nullptr, nullptr, status};
        tables = 2;
        {
            const Watch w(GROWS, 1 + 2);
            CHECK(w.ok(hsw_gadget_ntt(g, &a, &nrep)) && nrep.launches == 2 && nrep.scratch_bytes == 2 * (32ull << 16));
        }
        const Watch w(STAYS, 2);                                             // the same root again: no table kernel
        CHECK(w.ok(hsw_gadget_ntt(g, &a, &nrep)) && nrep.twiddle_ms == 0);
    }

    // ---- evaluate after everything larger, then the small call of the start again: nothing is allocated for either,
    //      and each reports what it reported
    {
        const hsw_evaluate_report first = erep;
        const Watch w(STAYS, 2);
        CHECK(w.ok(hsw_gadget_evaluate(g, &ev, &erep)) && erep.launches == first.launches && erep.queries == first.queries && erep.scratch_bytes == first.scratch_bytes);
    }
    {
        const hsw_product_report first = prep;
        const Watch w(STAYS, 3);
        CHECK(w.ok(hsw_gadget_lookup_product(g, &pa, &prep)) && prep.arguments == first.arguments && prep.written == first.written && prep.tile_rows == first.tile_rows);
        CHECK(g->scratch.cap > small_cap);
    }
    CHECK(growths == 5);
    hsw_gadget_destroy(g);
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("round scratch lifecycle ok\n");
    return 0;
}
