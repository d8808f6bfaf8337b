// The thread bodies of the quotient kernels (csrc/hsw_quotient_value.hpp) against the plain definition, on the CPU.  A
// stand-alone program: compile with -fsanitize=address,undefined and run it (tests/test_quotient_host.py does).
//
// The model knows nothing of Montgomery's method: numbers of nine 32-bit limbs, a * b mod p by shift-and-add, 1 / x by
// the binary extended Euclid.  It computes h row by row as include/hsw.h defines it -- every gate, the permutation's
// expressions and the lookups' folded as V = V y + expr, then V / (X_i^n - 1) with an inversion per row.  The bodies run
// the way hsw_quotient.hip runs them: tile by tile and thread by thread, gates, permutation, lookups, finish, with V in
// a scratch array between the "launches", w^row0 from the staged tile and thread powers, and everything staged as
// hsw_gadget_quotient.cpp stages it.  Both cell forms; (log_rows, e) = (3,1), (4,2), (6,3); rotations -(n-1), -1, 0, +3,
// +(n-1), so that rows wrap at both ends; monomials of 0, 1 and HSW_QUOTIENT_MAX_FACTORS factors; permutations of
// (columns, L) = (2,4), (4,2), (5,2): S = 1, 2, and 3 with a short last set; lookups of 1 + 1 and 2 + 2 columns; two
// proofs with their own challenges; a cell not below p is reported by the body that reads it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_quotient_value.hpp"

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


static Big model_pow_big(const Big &a, const Big &e) {
    Big r = small(1);
    for (int bit = 255; bit >= 0; bit--) { r = mulmod(r, r); if ((e.l[bit >> 5] >> (bit & 31)) & 1u) r = mulmod(r, a); }
    return r;
}
// 7^((p-1) / 2^log_n): a primitive 2^log_n-th root of unity
static Big model_root(uint32_t log_n) {
    Big e = minus(MP, small(1));
    for (uint32_t k = 0; k < log_n; k++) e = shr1(e);
    return model_pow_big(small(7), e);
}

using hsw::QUOTIENT_ROWS;
using hsw::QUOTIENT_TILE;
static unsigned long long g_rows = 0, g_runs = 0;

typedef std::vector<Big> Col;                       // N values
struct Term { Big coeff; std::vector<uint32_t> col; std::vector<int32_t> rot; };
typedef std::vector<Term> Gate;

struct Circuit {
    uint32_t log_rows, e, u, m, F, K, L;
    std::vector<Gate> gates;
    std::vector<uint32_t> perm;                     // column indices
    std::vector<std::vector<uint32_t>> lk_in, lk_tab;
    // values
    std::vector<Col> cols;                          // K x m
    std::vector<Col> fixed, sigmas;                 // F, n_perm
    std::vector<Col> perm_z;                        // K x S
    std::vector<Col> lk_a, lk_s, lk_z;              // K x n_lookups
    Col l0, l_last, l_active;
    std::vector<Big> y, theta, beta, gamma;         // K
    Big w, zeta, delta;
};

static Col random_col(std::mt19937_64 &rng, size_t N) {
    Col c(N);
    for (Big &x : c) x = random_big(rng);
    c[0] = small(0); c[1 % N] = minus(MP, small(1)); c[2 % N] = small(1);
    return c;
}

// h of proof c by the definition
static Col model_h(const Circuit &q, uint32_t c) {
    const uint32_t N = 1u << (q.log_rows + q.e), ext = 1u << q.e, n = 1u << q.log_rows;
    const size_t S = q.perm.empty() ? 0 : (q.perm.size() + q.L - 1) / q.L, nl = q.lk_in.size();
    auto column = [&](uint32_t j) -> const Col & { return j < q.m ? q.cols[(size_t)c * q.m + j] : q.fixed[j - q.m]; };
    auto rot = [&](uint32_t i, int64_t r) { return (uint32_t)(((int64_t)i + r * (int64_t)ext + (int64_t)N * 4) % N); };
    Col h(N);
    Big x = q.zeta;
    for (uint32_t i = 0; i < N; i++, x = mulmod(x, q.w)) {
        Big V = small(0);
        auto fold = [&](const Big &expr) { V = addmod(mulmod(V, q.y[c]), expr); };
        for (const Gate &g : q.gates) {
            Big s = small(0);
            for (const Term &t : g) {
                Big a = t.coeff;
                for (size_t f = 0; f < t.col.size(); f++) a = mulmod(a, column(t.col[f])[rot(i, t.rot[f])]);
                s = addmod(s, a);
            }
            fold(s);
        }
        if (S) {
            const Col *Z = &q.perm_z[(size_t)c * S];
            fold(mulmod(q.l0[i], submod(small(1), Z[0][i])));
            fold(mulmod(q.l_last[i], submod(mulmod(Z[S - 1][i], Z[S - 1][i]), Z[S - 1][i])));
            for (size_t s = 1; s < S; s++) fold(mulmod(q.l0[i], submod(Z[s][i], Z[s - 1][rot(i, q.u)])));
            Big dj = small(1);
            for (size_t s = 0; s < S; s++) {
                Big left = Z[s][rot(i, 1)], right = Z[s][i];
                for (size_t j = s * q.L; j < q.perm.size() && j < (s + 1) * q.L; j++, dj = mulmod(dj, q.delta)) {
                    const Big v = column(q.perm[j])[i];
                    left = mulmod(left, addmod(addmod(v, mulmod(q.beta[c], q.sigmas[j][i])), q.gamma[c]));
                    right = mulmod(right, addmod(addmod(v, mulmod(mulmod(q.beta[c], dj), x)), q.gamma[c]));
                }
                fold(mulmod(q.l_active[i], submod(left, right)));
            }
        }
        for (size_t l = 0; l < nl; l++) {
            Big A = small(0), Sv = small(0);
            for (uint32_t j : q.lk_in[l]) A = addmod(mulmod(A, q.theta[c]), column(j)[i]);
            for (uint32_t j : q.lk_tab[l]) Sv = addmod(mulmod(Sv, q.theta[c]), column(j)[i]);
            const Col &Ap = q.lk_a[c * nl + l], &Sp = q.lk_s[c * nl + l], &Z = q.lk_z[c * nl + l];
            fold(mulmod(q.l0[i], submod(small(1), Z[i])));
            fold(mulmod(q.l_last[i], submod(mulmod(Z[i], Z[i]), Z[i])));
            const Big left = mulmod(mulmod(Z[rot(i, 1)], addmod(Ap[i], q.beta[c])), addmod(Sp[i], q.gamma[c]));
            const Big right = mulmod(mulmod(Z[i], addmod(A, q.beta[c])), addmod(Sv, q.gamma[c]));
            fold(mulmod(q.l_active[i], submod(left, right)));
            fold(mulmod(q.l0[i], submod(Ap[i], Sp[i])));
            fold(mulmod(q.l_active[i], mulmod(submod(Ap[i], Sp[i]), submod(Ap[i], Ap[rot(i, -1)]))));
        }
        const Big t = submod(model_pow(x, n), small(1));
        h[i] = mulmod(V, model_inv(t));
    }
    return h;
}

typedef std::vector<PFe> Cells;
static Cells cells_of(const Col &c, bool mont) { Cells r(c.size()); for (size_t i = 0; i < c.size(); i++) r[i] = cell_of(c[i], mont); return r; }
static std::vector<Cells> cells_of(const std::vector<Col> &v, bool mont) { std::vector<Cells> r; for (const Col &c : v) r.push_back(cells_of(c, mont)); return r; }
static std::vector<const PFe *> pointers(const std::vector<Cells> &v) { std::vector<const PFe *> r; for (const Cells &c : v) r.push_back(c.data()); return r; }

// The bodies, staged and run as the entry point and the kernels do.  bad: (proof, column) whose cell 3 is replaced by p
static void run(const Circuit &q, bool mont, int bad_proof) {
    const uint32_t log_n = q.log_rows + q.e, N = 1u << log_n, n = 1u << q.log_rows;
    const size_t n_perm = q.perm.size(), S = n_perm ? (n_perm + q.L - 1) / q.L : 0, nl = q.lk_in.size();
    std::vector<Cells> cols = cells_of(q.cols, mont), fixed = cells_of(q.fixed, mont), sigmas = cells_of(q.sigmas, mont), pz = cells_of(q.perm_z, mont);
    std::vector<Cells> la = cells_of(q.lk_a, mont), ls = cells_of(q.lk_s, mont), lz = cells_of(q.lk_z, mont);
    const Cells l0 = cells_of(q.l0, mont), l_last = cells_of(q.l_last, mont), l_active = cells_of(q.l_active, mont);
    if (bad_proof >= 0) std::memcpy(cols[(size_t)bad_proof * q.m].data() + 3, MP.l, 32);       // p itself: not below p
    const std::vector<const PFe *> p_cols = pointers(cols), p_fixed = pointers(fixed), p_sig = pointers(sigmas), p_pz = pointers(pz);
    const std::vector<const PFe *> p_la = pointers(la), p_ls = pointers(ls), p_lz = pointers(lz);
    // the descriptor tables
    std::vector<uint32_t> gft{0}, tff{0}, fcol, foff, fi{0}, fin, ft{0}, ftab;
    std::vector<PFe> coeff;
    for (const Gate &g : q.gates) {
        for (const Term &t : g) {
            coeff.push_back(hsw::quotient_coeff(cell_of(t.coeff, mont), (uint32_t)t.col.size(), mont));
            for (size_t f = 0; f < t.col.size(); f++) {
                fcol.push_back(t.col[f]);
                foff.push_back((uint32_t)(((uint64_t)(t.rot[f] + (int64_t)n) << q.e) & (N - 1)));
            }
            tff.push_back((uint32_t)fcol.size());
        }
        gft.push_back((uint32_t)coeff.size());
    }
    fcol.push_back(0); foff.push_back(0); coeff.push_back(hsw::fr_zero());               // (never empty: data() is a pointer)
    for (size_t l = 0; l < nl; l++) {
        for (uint32_t j : q.lk_in[l]) fin.push_back(j);
        for (uint32_t j : q.lk_tab[l]) ftab.push_back(j);
        fi.push_back((uint32_t)fin.size()); ft.push_back((uint32_t)ftab.size());
    }
    const PFe w = cell_of(q.w, true), zeta = cell_of(q.zeta, true), delta = cell_of(q.delta, true);
    std::vector<hsw::QuotientProof> proofs(q.K);
    std::vector<PFe> beta_delta(q.K * n_perm + 1);
    for (uint32_t c = 0; c < q.K; c++) {
        proofs[c].y = cell_of(q.y[c], true); proofs[c].theta = cell_of(q.theta[c], true);
        proofs[c].beta = cell_of(q.beta[c], mont); proofs[c].gamma = cell_of(q.gamma[c], mont);
        proofs[c].beta_mul = hsw::product_theta_mul(proofs[c].beta, mont);
        PFe bd = hsw::fr_mont_mul(proofs[c].beta, zeta);
        for (size_t j = 0; j < n_perm; j++) { beta_delta[c * n_perm + j] = bd; bd = hsw::permutation_next_beta_delta(bd, delta); }
    }
    hsw::QuotientConstants kc;
    kc.one = hsw::pfe_repr(1u, mont);
    kc.r2 = hsw::quotient_r_power(2); kc.r3 = hsw::quotient_r_power(3); kc.r4 = hsw::quotient_r_power(4);
    const uint32_t L = n_perm ? (q.L < n_perm ? q.L : (uint32_t)n_perm) : 1u;
    kc.seed_full = hsw::quotient_r_power(L + 2);
    kc.seed_last = hsw::quotient_r_power((uint32_t)(n_perm ? n_perm - (S - 1) * L : 0) + 2);
    CHECK(cmp(value_of(kc.r2, true), model_times_R(small(1))) == 0);     // R^2 is R in Montgomery form
    std::vector<hsw::PermutationPowers> powers(1);
    hsw::permutation_stage_powers(w, QUOTIENT_ROWS, powers[0]);
    std::vector<PFe> t_inv((size_t)1 << q.e);
    CHECK(hsw::quotient_stage_t_inv(zeta, w, q.log_rows, q.e, t_inv.data()));
    std::vector<Cells> V(q.K, Cells(N)), h(q.K, Cells(N));
    std::vector<PFe *> p_h;
    for (Cells &c : h) p_h.push_back(c.data());
    std::vector<uint32_t> status(q.K, 0);
    hsw::QuotientParams p{};
    p.N = N; p.mask = N - 1; p.ext = 1u << q.e; p.u_off = (q.u << q.e) & (N - 1);
    p.m = q.m; p.F = q.F;
    p.cols = p_cols.data(); p.fixed = p_fixed.data();
    p.l0 = l0.data(); p.l_last = l_last.data(); p.l_active = l_active.data();
    p.n_gates = (uint32_t)q.gates.size(); p.n_perm = (uint32_t)n_perm; p.L = L; p.S = (uint32_t)S;
    p.gate_first_term = gft.data(); p.term_first_factor = tff.data(); p.factor_column = fcol.data(); p.factor_offset = foff.data(); p.term_coeff = coeff.data();
    p.perm_columns = q.perm.data(); p.sigmas = p_sig.data(); p.perm_z = p_pz.data(); p.beta_delta = beta_delta.data(); p.powers = powers.data();
    p.n_lookups = (uint32_t)nl; p.first_input = fi.data(); p.inputs = fin.data(); p.first_table = ft.data(); p.tables = ftab.data();
    p.lk_a = p_la.data(); p.lk_s = p_ls.data(); p.lk_z = p_lz.data();
    p.proofs = proofs.data(); p.t_inv = t_inv.data(); p.h = p_h.data(); p.status = status.data(); p.k = &kc;
    const uint32_t tiles = (N + QUOTIENT_TILE - 1) / QUOTIENT_TILE;
    for (uint32_t c = 0; c < q.K; c++) {
        p.first = 1;
        for (int family = 0; family < 4; family++) {                  // the launches
            if ((family == 0 && q.gates.empty()) || (family == 1 && !n_perm) || (family == 2 && !nl)) continue;
            for (uint32_t tile = 0; tile < tiles; tile++) {
                const PFe wt = hsw::permutation_omega_tile(powers[0], tile);
                for (uint32_t t = 0; t < hsw::QUOTIENT_THREADS; t++) {
                    const uint32_t row0 = (tile * hsw::QUOTIENT_THREADS + t) * QUOTIENT_ROWS;
                    if (row0 >= N) continue;
                    if (family == 3) {
                        if (!(status[c] & hsw::QUOTIENT_CELL_NOT_BELOW_P)) hsw::quotient_finish_rows(p, V[c].data(), p.h[c], row0);
                        continue;
                    }
                    PFe v[QUOTIENT_ROWS];
                    hsw::quotient_begin(p, V[c].data(), row0, v);
                    bool ok = true;
                    if (family == 0) ok = hsw::quotient_gates_rows(p, c, row0, v);
                    else if (family == 1) {
                        const PFe x0 = hsw::permutation_omega_thread(powers[0], wt, t);
                        ok = mont ? hsw::quotient_permutation_rows<true>(p, c, row0, x0, v) : hsw::quotient_permutation_rows<false>(p, c, row0, x0, v);
                    } else ok = mont ? hsw::quotient_lookups_rows<true>(p, c, row0, v) : hsw::quotient_lookups_rows<false>(p, c, row0, v);
                    if (!ok) status[c] |= hsw::QUOTIENT_CELL_NOT_BELOW_P;
                    hsw::quotient_end(V[c].data(), row0, v);
                }
            }
            p.first = 0;
        }
        if ((int)c == bad_proof) {
            CHECK(status[c] == hsw::QUOTIENT_CELL_NOT_BELOW_P);
            for (const PFe &x : h[c]) CHECK(hsw::fr_is_zero(x));                          // nothing was written
            continue;
        }
        CHECK(status[c] == 0);
        const Col want = model_h(q, c);
        for (uint32_t i = 0; i < N; i++) CHECK(hsw::fr_equal(h[c][i], cell_of(want[i], mont)));
        g_rows += N;
    }
    g_runs++;
}

static Circuit make(std::mt19937_64 &rng, uint32_t log_rows, uint32_t e, uint32_t n_perm, uint32_t L, bool gates, bool lookups) {
    Circuit q{};
    q.log_rows = log_rows; q.e = e; q.m = 3; q.F = 2; q.K = 2; q.L = L;
    const uint32_t n = 1u << log_rows, N = n << e;
    q.u = n - 3;
    const int32_t far = (int32_t)n - 1, near3 = n > 3 ? 3 : 1;
    if (gates) {
        q.gates.push_back(Gate{Term{random_big(rng), {}, {}}});                                        // a bare constant
        q.gates.push_back(Gate{Term{small(1), {0}, {-far}}, Term{minus(MP, small(1)), {4}, {far}}});   // single factors, both ends
        q.gates.push_back(Gate{Term{random_big(rng), {0, 1, 2, 3, 4, 0, 1, 2}, {-far, -1, 0, near3, far, 0, 1, -1}},   // MAX_FACTORS
                               Term{small(1), {3, 0}, {0, 0}}, Term{small(1), {3, 0, 0}, {0, 1, 2}}, Term{minus(MP, small(1)), {3, 0}, {0, near3}}});
    }
    for (uint32_t j = 0; j < n_perm; j++) q.perm.push_back((j * 2 + 1) % (q.m + q.F));                 // proof and fixed columns mixed
    if (lookups) { q.lk_in = {{2}, {0, 4}}; q.lk_tab = {{3}, {4, 1}}; }
    const size_t S = n_perm ? (n_perm + (L < n_perm ? L : n_perm) - 1) / (L < n_perm ? L : n_perm) : 0;
    for (uint32_t i = 0; i < q.K * q.m; i++) q.cols.push_back(random_col(rng, N));
    for (uint32_t i = 0; i < q.F; i++) q.fixed.push_back(random_col(rng, N));
    for (uint32_t i = 0; i < n_perm; i++) q.sigmas.push_back(random_col(rng, N));
    for (size_t i = 0; i < q.K * S; i++) q.perm_z.push_back(random_col(rng, N));
    for (size_t i = 0; i < q.K * q.lk_in.size(); i++) { q.lk_a.push_back(random_col(rng, N)); q.lk_s.push_back(random_col(rng, N)); q.lk_z.push_back(random_col(rng, N)); }
    q.l0 = random_col(rng, N); q.l_last = random_col(rng, N); q.l_active = random_col(rng, N);
    for (uint32_t c = 0; c < q.K; c++) { q.y.push_back(random_big(rng)); q.theta.push_back(random_big(rng)); q.beta.push_back(random_big(rng)); q.gamma.push_back(random_big(rng)); }
    q.w = model_root(log_rows + e); q.zeta = random_big(rng); q.delta = small(7);
    if (n_perm && L > n_perm) q.L = n_perm;                           // (the model's sets are the staged ones)
    return q;
}

int main() {
    std::mt19937_64 rng(20261021);
    const uint32_t shapes[3][2] = {{3, 1}, {4, 2}, {6, 3}};
    const uint32_t perms[3][2] = {{2, 4}, {4, 2}, {5, 2}};
    for (int mont = 0; mont < 2; mont++) {
        for (int s = 0; s < 3; s++) {
            const uint32_t lr = shapes[s][0], e = shapes[s][1];
            run(make(rng, lr, e, 0, 1, true, false), mont, -1);                       // gates alone
            for (int k = 0; k < 3 && s < 2; k++) run(make(rng, lr, e, perms[k][0], perms[k][1], false, false), mont, -1);   // S = 1, 2, 3
            if (s < 2) run(make(rng, lr, e, 0, 1, false, true), mont, -1);            // lookups alone
            run(make(rng, lr, e, perms[s][0], perms[s][1], true, true), mont, -1);    // everything
        }
        run(make(rng, 4, 2, 4, 2, true, true), mont, 1);                              // proof 1 reads a cell that is p
        run(make(rng, 4, 2, 0, 1, true, false), mont, 0);
    }
    // zeta on the coset's own vanishing set has no t_inv
    PFe t_inv[4];
    CHECK(!hsw::quotient_stage_t_inv(hsw::fr_one_mont(), cell_of(model_root(6), true), 4, 2, t_inv));
    std::printf("quotient value check ok: %llu runs, %llu rows\n", g_runs, g_rows);
    return 0;
}
