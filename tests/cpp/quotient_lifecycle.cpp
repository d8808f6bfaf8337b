// hsw_gadget_quotient on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in HIP runtime
// of hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every refusal that is decided
// before a launch, with its status and its hsw_last_error naming the item (and that it launches nothing, allocates
// nothing and writes no status); the launches -- one per family that is present and the finish, per batch; what the
// report says; the growth and the reuse of the scratch across calls; the batches of proofs under the "quotient_scratch"
// option, a batch being at least one proof; no device allocation and no event left at the end.  The columns and the h
// are addresses only: no launch runs, so nothing reads or writes them.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../halo2-dynamic-sha256_amd/csrc/hsw_quotient_value.hpp"
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

static const uint8_t P_BYTES[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                    0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};   // p itself: not below p

// 7^((p-1) / 2^log_n) as a canonical cell: a primitive 2^log_n-th root of unity
static hsw::PFe root(uint32_t log_n) {
    uint32_t e[8] = {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};   // p - 1
    for (uint32_t k = 0; k < log_n; k++)
        for (int j = 0; j < 8; j++) e[j] = (e[j] >> 1) | (j < 7 ? e[j + 1] << 31 : 0);
    const hsw::PFe seven = hsw::fr_to_mont(hsw::PFe{{7, 0, 0, 0, 0, 0, 0, 0}});
    hsw::PFe r = hsw::fr_one_mont();
    for (int bit = 255; bit >= 0; bit--) {
        r = hsw::fr_mont_mul(r, r);
        if ((e[bit >> 5] >> (bit & 31)) & 1u) r = hsw::fr_mont_mul(r, seven);
    }
    return hsw::fr_from_mont(r);
}

// K proofs of 3 own and 2 shared columns: two gates, a permutation of 3 columns in sets of 2, two lookups
struct Call {
    uint32_t log_rows, log_n;
    size_t K;
    uint64_t N;
    std::vector<const void *> cols, fixed, sigmas, pz, la, ls, lz;
    std::vector<void *> h;
    const void *l0, *l_last, *l_active;
    std::vector<uint32_t> gft{0, 3, 4}, tff{0, 2, 4, 6, 6}, fcol{3, 0, 3, 0, 3, 0}, perm{0, 4, 2}, fi{0, 1, 3}, fin{2, 0, 4}, ft{0, 1, 3}, ftab{3, 4, 1}, status;
    std::vector<int32_t> frot{0, 0, 0, 1, 0, 3};
    std::vector<uint8_t> coeffs, ys, betas, gammas, thetas, omega, zeta, delta;
    Call(size_t K_, uint32_t log_rows_ = 4, uint32_t e = 2) : log_rows(log_rows_), log_n(log_rows_ + e), K(K_), N(1ull << (log_rows_ + e)), status(K_, 0xFFFFFFFFu),
                                                            coeffs(32 * 4, 0), ys(32 * K_, 0), betas(32 * K_, 0), gammas(32 * K_, 0), thetas(32 * K_, 0),
                                                            omega(32, 0), zeta(32, 0), delta(32, 0) {
        uintptr_t at = 0x100000000000ull;
        auto next = [&]() { const uintptr_t x = at; at += 32 * N; return reinterpret_cast<const void *>(x); };
        for (size_t i = 0; i < K * 3; i++) cols.push_back(next());
        for (size_t i = 0; i < 2; i++) fixed.push_back(next());
        for (size_t i = 0; i < 3; i++) sigmas.push_back(next());
        for (size_t i = 0; i < K * 2; i++) { pz.push_back(next()); la.push_back(next()); ls.push_back(next()); lz.push_back(next()); }
        l0 = next(); l_last = next(); l_active = next();
        for (size_t i = 0; i < K; i++) h.push_back(const_cast<void *>(next()));
        for (size_t t = 0; t < 4; t++) coeffs[32 * t] = (uint8_t)(t + 1);
        for (size_t k = 0; k < K; k++) { ys[32 * k] = 2; betas[32 * k] = 3; gammas[32 * k] = 4; thetas[32 * k] = 5; }
        const hsw::PFe w = root(log_n);
        std::memcpy(omega.data(), w.l, 32);
        zeta[0] = 5; delta[0] = 7;
    }
    hsw_quotient args() {
        hsw_quotient a{};
        a.log_rows = log_rows; a.log_n = log_n; a.chunk_columns = 2; a.usable_rows = (1ull << log_rows) - 6;
        a.n_proofs = K; a.n_columns = 3; a.n_fixed = 2;
        a.d_columns = cols.data(); a.d_fixed = fixed.data(); a.d_l0 = l0; a.d_l_last = l_last; a.d_l_active = l_active;
        a.gates = hsw_quotient_gates{2, 4, 6, gft.data(), coeffs.data(), tff.data(), fcol.data(), frot.data()};
        a.n_perm_columns = 3; a.perm_columns = perm.data(); a.d_sigmas = sigmas.data(); a.d_perm_products = pz.data();
        a.lookups = hsw_quotient_lookups{2, fi.data(), fin.data(), ft.data(), ftab.data(), la.data(), ls.data(), lz.data(), thetas.data()};
        a.betas = betas.data(); a.gammas = gammas.data(); a.ys = ys.data();
        a.omega_ext = omega.data(); a.zeta = zeta.data(); a.delta = delta.data();
        a.d_h = h.data(); a.status = status.data();
        return a;
    }
    bool untouched() const {
        for (uint32_t x : status) if (x != 0xFFFFFFFFu) return false;
        return true;
    }
};

static bool refused(hsw_engine *e, hsw_gadget *g, const hsw_quotient &a, const Call &call, int status, const char *text) {
    hsw_quotient_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    const int rc = hsw_gadget_quotient(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "quotient: got %d (%s), expected %d (...%s...)\n", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.launches == 0 && rep.proofs == 0 && call.untouched();
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_quotient_gates) == 64 && sizeof(hsw_quotient_lookups) == 72 && sizeof(hsw_quotient) == 320 && sizeof(hsw_quotient_report) == 80);
    CHECK(HSW_QUOTIENT_CELL_NOT_BELOW_P == hsw::QUOTIENT_CELL_NOT_BELOW_P && HSW_QUOTIENT_CELL_NOT_BELOW_P == HSW_NTT_CELL_NOT_BELOW_P);
    CHECK(HSW_QUOTIENT_MAX_FACTORS == hsw::QUOTIENT_MAX_FACTORS && HSW_QUOTIENT_MAX_EXTENSION == hsw::QUOTIENT_MAX_EXTENSION);
    hsw_quotient_report rep;
    {   // ---- a linear block-stream gadget takes the call too; in 8-byte cells: refused, nothing launched
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        Call call(2);
        const hsw_quotient a = call.args();
        CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && rep.proofs == 2 && rep.launches == 4 && rep.written == 128 && rep.expressions == 2 + 5 + 10);
        CHECK(rep.rows_per_thread == hsw::QUOTIENT_ROWS && rep.scratch_bytes == 2 * 64 * 32 && rep.first_refused == ~0ull && rep.refused_proofs == 0);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        Call fresh(2);
        CHECK(refused(e, g, fresh.args(), fresh, HSW_ERR_UNSUPPORTED, "32-byte"));
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- every refusal
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        Call call(2);
        const hsw_quotient ok = call.args();
        hsw_quotient b = ok;
        CHECK(hsw_gadget_quotient(nullptr, &ok, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_quotient(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_quotient(g, &ok, nullptr) == HSW_ERR_INVALID_ARG && call.untouched());
        const int INV = HSW_ERR_INVALID_ARG;
        b = ok; b.n_proofs = 0; CHECK(refused(e, g, b, call, INV, "n_proofs is at least 1"));
        b = ok; b.gates.n_gates = 0; b.gates.n_terms = 0; b.gates.n_factors = 0; b.n_perm_columns = 0; b.lookups.n_lookups = 0;
        CHECK(refused(e, g, b, call, INV, "nothing to fold"));
        b = ok; b.log_n = 29; CHECK(refused(e, g, b, call, INV, "log_n is at most 28"));
        b = ok; b.log_n = b.log_rows; CHECK(refused(e, g, b, call, INV, "the extension log_n - log_rows is 1 .. 8"));
        b = ok; b.log_rows = 2; b.log_n = 11; CHECK(refused(e, g, b, call, INV, "the extension log_n - log_rows is 1 .. 8"));
        b = ok; b.usable_rows = 0; CHECK(refused(e, g, b, call, INV, "usable_rows is 1 .. 2^log_rows - 1"));
        b = ok; b.usable_rows = 16; CHECK(refused(e, g, b, call, INV, "usable_rows is 1 .. 2^log_rows - 1"));
        b = ok; b.flags = 1; CHECK(refused(e, g, b, call, INV, "unknown flag"));
        b = ok; b.gates.n_gates = (size_t)1 << 32; CHECK(refused(e, g, b, call, HSW_ERR_TOO_LARGE, "does not fit 32 bits"));
        b = ok; b.n_proofs = (size_t)1 << 32; CHECK(refused(e, g, b, call, HSW_ERR_TOO_LARGE, "does not fit 32 bits"));
        {   // the offset arrays
            const uint32_t down[3] = {0, 4, 3}, short_[3] = {0, 2, 3}, late[3] = {1, 3, 4};
            b = ok; b.gates.gate_first_term = down; CHECK(refused(e, g, b, call, INV, "gate_first_term is not ascending from 0 to n_terms"));
            b = ok; b.gates.gate_first_term = short_; CHECK(refused(e, g, b, call, INV, "gate_first_term is not ascending from 0 to n_terms"));
            b = ok; b.gates.gate_first_term = late; CHECK(refused(e, g, b, call, INV, "gate_first_term is not ascending from 0 to n_terms"));
            const uint32_t tdown[5] = {0, 2, 1, 6, 6}, tend[5] = {0, 2, 4, 5, 5};
            b = ok; b.gates.term_first_factor = tdown; CHECK(refused(e, g, b, call, INV, "term_first_factor is not ascending from 0 to n_factors"));
            b = ok; b.gates.term_first_factor = tend; CHECK(refused(e, g, b, call, INV, "term_first_factor is not ascending from 0 to n_factors"));
            const uint32_t one_gate[2] = {0, 1}, nine[2] = {0, 9}, cols9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            const int32_t rot9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            b = ok; b.gates = hsw_quotient_gates{1, 1, 9, one_gate, call.coeffs.data(), nine, cols9, rot9};
            CHECK(refused(e, g, b, call, INV, "term 0: more than HSW_QUOTIENT_MAX_FACTORS factors"));
            const uint32_t fcol[6] = {3, 5, 3, 0, 3, 0};
            b = ok; b.gates.factor_column = fcol; CHECK(refused(e, g, b, call, INV, "factor 1: its column index is out of range"));
            for (int32_t r : {16, -16}) {
                const int32_t frot[6] = {0, 0, r, 1, 0, 3};
                b = ok; b.gates.factor_rotation = frot; CHECK(refused(e, g, b, call, INV, "factor 2: a rotation of 2^log_rows rows or more"));
            }
            std::vector<uint8_t> bad(call.coeffs);
            std::memcpy(bad.data() + 32, P_BYTES, 32);
            b = ok; b.gates.term_coeffs = bad.data(); CHECK(refused(e, g, b, call, INV, "term 1: a coefficient whose stored limbs are not below p"));
            b = ok; b.gates.term_coeffs = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the gates is NULL"));
            b = ok; b.gates.gate_first_term = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the gates is NULL"));
            b = ok; b.gates.factor_rotation = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the gates is NULL"));
            b = ok; b.gates.n_gates = 0; CHECK(refused(e, g, b, call, INV, "terms or factors without a gate"));
        }
        {   // the permutation
            const uint32_t perm[3] = {0, 5, 2};
            b = ok; b.perm_columns = perm; CHECK(refused(e, g, b, call, INV, "permutation column 1: its column index is out of range"));
            b = ok; b.chunk_columns = 0; CHECK(refused(e, g, b, call, INV, "chunk_columns is at least 1"));
            b = ok; b.d_sigmas = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the permutation is NULL"));
            b = ok; b.d_perm_products = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the permutation is NULL"));
            b = ok; b.delta = nullptr; CHECK(refused(e, g, b, call, INV, "delta is NULL"));
            b = ok; b.delta = P_BYTES; CHECK(refused(e, g, b, call, INV, "omega_ext, zeta or delta whose stored limbs are not below p"));
        }
        {   // the lookups
            const uint32_t none[3] = {0, 1, 1}, idx[3] = {2, 0, 5};
            b = ok; b.lookups.first_input = none; CHECK(refused(e, g, b, call, INV, "lookup 1: no input column"));
            const uint32_t none0[3] = {0, 0, 3};
            b = ok; b.lookups.first_table = none0; CHECK(refused(e, g, b, call, INV, "lookup 0: no table column"));
            b = ok; b.lookups.inputs = idx; CHECK(refused(e, g, b, call, INV, "lookup 1: an input column index out of range"));
            b = ok; b.lookups.tables = idx; CHECK(refused(e, g, b, call, INV, "lookup 1: a table column index out of range"));
            b = ok; b.lookups.thetas = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the lookups is NULL"));
            b = ok; b.lookups.d_products = nullptr; CHECK(refused(e, g, b, call, INV, "an array of the lookups is NULL"));
            std::vector<uint8_t> bad(call.thetas);
            std::memcpy(bad.data() + 32, P_BYTES, 32);
            b = ok; b.lookups.thetas = bad.data(); CHECK(refused(e, g, b, call, INV, "proof 1: a theta whose stored limbs are not below p"));
        }
        {   // arrays, challenges and constants
            b = ok; b.d_columns = nullptr; CHECK(refused(e, g, b, call, INV, "d_columns is NULL"));
            b = ok; b.d_fixed = nullptr; CHECK(refused(e, g, b, call, INV, "d_fixed is NULL"));
            b = ok; b.d_h = nullptr; CHECK(refused(e, g, b, call, INV, "d_h is NULL"));
            b = ok; b.ys = nullptr; CHECK(refused(e, g, b, call, INV, "ys is NULL"));
            b = ok; b.zeta = nullptr; CHECK(refused(e, g, b, call, INV, "omega_ext or zeta is NULL"));
            b = ok; b.betas = nullptr; CHECK(refused(e, g, b, call, INV, "betas or gammas is NULL"));
            b = ok; b.d_l_last = nullptr; CHECK(refused(e, g, b, call, INV, "d_l0, d_l_last or d_l_active is NULL"));
            std::vector<uint8_t> bad(call.ys);
            std::memcpy(bad.data() + 32, P_BYTES, 32);
            b = ok; b.ys = bad.data(); CHECK(refused(e, g, b, call, INV, "proof 1: a y whose stored limbs are not below p"));
            b = ok; b.betas = bad.data(); CHECK(refused(e, g, b, call, INV, "proof 1: a beta whose stored limbs are not below p"));
            b = ok; b.gammas = bad.data(); CHECK(refused(e, g, b, call, INV, "proof 1: a gamma whose stored limbs are not below p"));
            b = ok; b.zeta = P_BYTES; CHECK(refused(e, g, b, call, INV, "omega_ext, zeta or delta whose stored limbs are not below p"));
            const hsw::PFe w5 = root(5), w7 = root(7);                      // a root of another order
            b = ok; b.omega_ext = w5.l; CHECK(refused(e, g, b, call, INV, "omega_ext is not a primitive 2^log_n-th root of unity"));
            b = ok; b.omega_ext = w7.l; CHECK(refused(e, g, b, call, INV, "omega_ext is not a primitive 2^log_n-th root of unity"));
            uint8_t one[32] = {1};
            b = ok; b.zeta = one; CHECK(refused(e, g, b, call, INV, "the vanishing polynomial is 0 on its coset"));
            b = ok; b.zeta = call.omega.data(); CHECK(refused(e, g, b, call, INV, "the vanishing polynomial is 0 on its coset"));   // w^n (w^n)^3 = 1
        }
        for (int how = 0; how < 2; how++) {   // pointers
            std::vector<const void *> p(call.cols);
            p[4] = how ? static_cast<const uint8_t *>(p[4]) + 8 : nullptr;
            b = ok; b.d_columns = p.data(); CHECK(refused(e, g, b, call, INV, "column 4: a pointer that is NULL or not 16-byte aligned"));
            p = call.lz;
            p[3] = how ? static_cast<const uint8_t *>(p[3]) + 4 : nullptr;
            b = ok; b.lookups.d_products = p.data(); CHECK(refused(e, g, b, call, INV, "lookup product 3: a pointer that is NULL or not 16-byte aligned"));
            std::vector<void *> hp(call.h);
            hp[1] = how ? static_cast<void *>(static_cast<uint8_t *>(hp[1]) + 8) : nullptr;
            b = ok; b.d_h = hp.data(); CHECK(refused(e, g, b, call, INV, "proof 1: a d_h pointer that is NULL or not 16-byte aligned"));
        }
        b = ok; b.d_l0 = static_cast<const uint8_t *>(call.l0) + 8; CHECK(refused(e, g, b, call, INV, "l0 0: a pointer that is NULL or not 16-byte aligned"));
        {   // overlaps: with the last row of a column, with another d_h, with a shared column
            std::vector<void *> hp(call.h);
            hp[0] = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.cols[2]) + 32 * 63);
            b = ok; b.d_h = hp.data(); CHECK(refused(e, g, b, call, INV, "proof 0: its d_h overlaps column 2"));
            hp = call.h;
            hp[1] = static_cast<uint8_t *>(hp[0]) + 32 * 63;
            b = ok; b.d_h = hp.data(); CHECK(refused(e, g, b, call, INV, "proof 1: its d_h overlaps the d_h of proof 0"));
            hp = call.h;
            hp[1] = const_cast<void *>(call.sigmas[1]);
            b = ok; b.d_h = hp.data(); CHECK(refused(e, g, b, call, INV, "proof 1: its d_h overlaps sigma 1"));
            hp[1] = const_cast<uint8_t *>(static_cast<const uint8_t *>(call.l_active) - 32 * 63);
            b = ok; b.d_h = hp.data(); CHECK(refused(e, g, b, call, INV, "proof 1: its d_h overlaps l_last 0"));
            hp = call.h;
            hp[0] = static_cast<uint8_t *>(hp[1]) + 32 * 64;               // right behind the last h: allowed; and no status array
            b = ok; b.d_h = hp.data(); b.status = nullptr;
            CHECK(hsw_gadget_quotient(g, &b, &rep) == HSW_OK && rep.launches == 4);
        }
        CHECK(hip_stub_live_device_allocations() > 0);                       // (the gadget's own)
        hsw_gadget_destroy(g);
    }
    CHECK(hip_stub_live_device_allocations() == 0);
    {   // ---- launches per family; the scratch grows once and is reused; batches
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, HSW_GADGET_WHOLE_DIGEST, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        {
            Call call(3);
            hsw_quotient a = call.args();
            int l0 = hip_stub_launches();
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 4 && rep.launches == 4 && rep.expressions == 17);
            CHECK(rep.proofs == 3 && rep.written == 3 * 64 && rep.scratch_bytes == 3 * 64 * 32 && hip_stub_live_device_allocations() == live0 + 1);
            for (uint32_t s : call.status) CHECK(s == 0);
            a.gates.n_gates = 0; a.gates.n_terms = 0; a.gates.n_factors = 0;             // no gate: betas and the fixed family still needed
            l0 = hip_stub_launches();
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3 && rep.expressions == 15);
            a = call.args(); a.n_perm_columns = 0; a.lookups.n_lookups = 0;             // gates alone need no l0, beta, gamma, delta
            a.d_l0 = a.d_l_last = a.d_l_active = nullptr; a.betas = a.gammas = a.delta = nullptr;
            l0 = hip_stub_launches();
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 2 && rep.expressions == 2);
            a = call.args(); a.chunk_columns = 100;                                      // a set wider than the permutation: one set
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && rep.expressions == 2 + 3 + 10);
        }
        {   // a larger call replaces the scratch, a smaller one reuses it
            Call large(2, 10, 3);
            const hsw_quotient a = large.args();
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && rep.scratch_bytes == 2ull * 8192 * 32 && hip_stub_live_device_allocations() == live0 + 1);
            Call small(1);
            const hsw_quotient s = small.args();
            CHECK(hsw_gadget_quotient(g, &s, &rep) == HSW_OK && rep.scratch_bytes == 64 * 32 && hip_stub_live_device_allocations() == live0 + 1);
        }
        {   // batches: five proofs, two at a time; then one at a time under a bound below one proof
            CHECK(hsw_engine_set_option(e, "quotient_scratch", 0) == HSW_ERR_INVALID_ARG);
            CHECK(hsw_engine_set_option(e, "quotient_scratch", ((int64_t)1 << 30) + 1) == HSW_ERR_INVALID_ARG);
            CHECK(hsw_engine_set_option(e, "quotient_scratch", 2 * 64 * 32 + 31) == HSW_OK);
            Call call(5);
            const hsw_quotient a = call.args();
            int l0 = hip_stub_launches();
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && rep.launches == 12 && hip_stub_launches() == l0 + 12 && rep.scratch_bytes == 2 * 64 * 32);
            CHECK(rep.proofs == 5 && rep.written == 5 * 64);
            CHECK(hsw_engine_set_option(e, "quotient_scratch", 1) == HSW_OK);
            l0 = hip_stub_launches();
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && rep.launches == 20 && hip_stub_launches() == l0 + 20 && rep.scratch_bytes == 64 * 32);
            CHECK(hsw_engine_set_option(e, "quotient_scratch", (int64_t)1 << 30) == HSW_OK);
            CHECK(hsw_gadget_quotient(g, &a, &rep) == HSW_OK && rep.launches == 4 && rep.scratch_bytes == 5 * 64 * 32);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);
        }
        CHECK(hip_stub_live_events() > 0);                                   // (the engine's own)
        hsw_gadget_destroy(g);                                               // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live0 + 1);
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("quotient lifecycle ok\n");
    return 0;
}
