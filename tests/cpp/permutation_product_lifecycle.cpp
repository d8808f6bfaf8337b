// hsw_gadget_permutation_product on the host side under AddressSanitizer + UBSan + LeakSanitizer, against the stand-in
// HIP runtime of hip_stub.cpp ("device" memory = heap memory, launches do nothing).  Checked here: every refusal that is
// decided before a launch, with its status and its hsw_last_error (and that it launches nothing and allocates nothing);
// the products, cells and launches of a call for (K, m, L, u) in {(1,1,1,1), (3,5,2,1024), (2,4,4,2500)}; the limit on
// the tiles of one launch; the overlap sweep (Z over a value column, over a sigma column, over another Z); the growth
// of the gadget's scratch and its release (no device allocation and no event left at the end).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

static const uint32_t WHOLE = HSW_GADGET_WHOLE_DIGEST;
static const uint64_t P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

// the caller's columns: per proof m value columns (u cells), S Z columns (u + 1 cells), and m sigma columns, exact size
struct Columns {
    size_t K, m, L, S;
    uint64_t u;
    std::vector<const void *> v, sigma;
    std::vector<void *> z, mine;
    void *cells(uint64_t n) {
        void *p = std::aligned_alloc(32, (size_t)n * 32);
        CHECK(p);
        std::memset(p, 0, (size_t)n * 32);
        mine.push_back(p);
        return p;
    }
    Columns(size_t K_, size_t m_, size_t L_, uint64_t u_) : K(K_), m(m_), L(L_), S((m_ + L_ - 1) / L_), u(u_) {
        for (size_t j = 0; j < m; j++) sigma.push_back(cells(u));
        for (size_t c = 0; c < K; c++) {
            for (size_t j = 0; j < m; j++) v.push_back(cells(u));
            for (size_t s = 0; s < S; s++) z.push_back(cells(u + 1));
        }
    }
    ~Columns() { for (void *p : mine) std::free(p); }
    hsw_permutation_product args(const void *betas, const void *gammas, const void *omega, const void *delta, uint32_t *status) const {
        return hsw_permutation_product{0, (uint32_t)L, u, m, v.data(), nullptr, sigma.data(), z.data(), betas, gammas, omega, delta, status};
    }
};

static bool refused(hsw_engine *e, hsw_gadget *g, const hsw_permutation_product &a, int status, const char *text) {
    hsw_permutation_report rep;
    const int l0 = hip_stub_launches();
    const size_t live = hip_stub_live_device_allocations();
    const int rc = hsw_gadget_permutation_product(g, &a, &rep);
    if (rc != status || !std::strstr(hsw_last_error(e), text)) {
        std::fprintf(stderr, "got %d (%s), expected %d (...%s...)\n", rc, hsw_last_error(e), status, text);
        return false;
    }
    return hip_stub_launches() == l0 && hip_stub_live_device_allocations() == live && rep.written == 0;
}

int main() {
    CHECK(hsw_abi_version() == 3 && HSW_ABI_MINOR == 1);
    CHECK(sizeof(hsw_permutation_product) == 96 && sizeof(hsw_permutation_report) == 80);
    hsw_permutation_report rep;
    uint64_t ch[3][4] = {{5, 0, 0, 0}, {P[0] - 1, P[1], P[2], P[3]}, {7, 7, 7, 1}};            // (p - 1 is a field element)
    const uint64_t above[3][4] = {{5, 0, 0, 0}, {1, 0, 0, 0}, {7, 7, 7, ~0ull}};               // the third is above p
    const uint64_t omega[4] = {3, 0, 0, 0}, delta[4] = {9, 9, 0, 0};
    uint32_t status[8];
    {   // ---- a linear block-stream gadget is one proof; in 8-byte cells: refused, nothing launched
        hsw_engine *e = nullptr;
        CHECK(hsw_engine_create(0, nullptr, 8, 3, &e) == HSW_OK);
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create(e, sizes, 1, 0, &g) == HSW_OK);
        const Columns col(1, 2, 1, 70);
        const hsw_permutation_product a = col.args(ch, ch, omega, delta, status);
        CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK && rep.proofs == 1 && rep.products == 2 && rep.written == 2 * 71);
        CHECK(hsw_gadget_reset(g) == HSW_OK && hsw_gadget_set_repr(g, HSW_REPR_COMPACT64) == HSW_OK);
        CHECK(refused(e, g, a, HSW_ERR_UNSUPPORTED, "32-byte"));
        hsw_gadget_destroy(g);
        hsw_engine_destroy(e);
    }
    hsw_engine *e = nullptr;
    CHECK(hsw_engine_create_ex(0, nullptr, 8, 2, HSW_MODE_HALO2_INTERNALS, &e) == HSW_OK);
    {   // ---- a single Context, K = 1: (m, L, u) = (1, 1, 1); every refusal; scratch growth
        const size_t sizes[1] = {128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 1, 1, WHOLE, &g) == HSW_OK);
        const size_t live0 = hip_stub_live_device_allocations();
        const Columns col(1, 5, 2, 3000);
        const hsw_permutation_product ok = col.args(ch, ch, omega, delta, status);
        hsw_permutation_product bad = ok;
        CHECK(hsw_gadget_permutation_product(nullptr, &ok, &rep) == HSW_ERR_INVALID_ARG && hsw_gadget_permutation_product(g, nullptr, &rep) == HSW_ERR_INVALID_ARG);
        CHECK(hsw_gadget_permutation_product(g, &ok, nullptr) == HSW_ERR_INVALID_ARG);
        bad.usable_rows = 0;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "at least 1"));
        bad = ok; bad.n_columns = 0;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "at least 1"));
        bad = ok; bad.chunk_columns = 0;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "at least 1"));
        bad = ok; bad.flags = 1;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "unknown flag"));
        bad = ok; bad.usable_rows = (1ull << 31) + 1;
        CHECK(refused(e, g, bad, HSW_ERR_TOO_LARGE, "above 2^31"));
        // a NULL pointer array, one by one
        bad = ok; bad.d_columns = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        bad = ok; bad.d_sigmas = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        bad = ok; bad.d_products = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "pointer array is NULL"));
        // a NULL or misaligned column, in every family
        for (int family = 0; family < 3; family++)
            for (int how = 0; how < 2; how++) {
                std::vector<const void *> cp(family == 0 ? col.v : col.sigma);
                std::vector<void *> zp(col.z);
                if (family < 2) cp[1] = how ? static_cast<const uint8_t *>(cp[1]) + 8 : nullptr;
                else zp[1] = how ? static_cast<uint8_t *>(zp[1]) + 8 : nullptr;
                bad = ok;
                if (family == 0) bad.d_columns = cp.data();
                if (family == 1) bad.d_sigmas = cp.data();
                if (family == 2) bad.d_products = zp.data();
                CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, family == 1 ? "sigma column pointer" : "proof 0: a"));
                CHECK(std::strstr(hsw_last_error(e), "NULL or not 16-byte aligned"));
            }
        {
            uint64_t rows[5] = {3000, 0, 17, 3001, 5};
            bad = ok; bad.column_rows = rows;
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "proof 0: column_rows above usable_rows"));
        }
        // challenges, omega, delta: missing, equal to p, above p
        bad = ok; bad.betas = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "is NULL"));
        bad = ok; bad.gammas = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "is NULL"));
        bad = ok; bad.omega = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "is NULL"));
        bad = ok; bad.delta = nullptr;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "is NULL"));
        bad = ok; bad.betas = P;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "a challenge whose stored limbs are not below p"));
        bad = ok; bad.gammas = above[2];
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "a challenge whose stored limbs are not below p"));
        bad = ok; bad.omega = P;
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "omega or delta"));
        bad = ok; bad.delta = above[2];
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "omega or delta"));
        // more tiles than one launch takes: u = 2^31 is 2^21 + 1 tiles per chunk; 1,024 chunks of them.  (The pointers
        // are never followed: nothing is launched.)
        {
            const size_t m = 1024;
            std::vector<const void *> v(m), sg(m);
            std::vector<void *> z(m);
            for (size_t j = 0; j < m; j++) {
                v[j] = reinterpret_cast<const void *>((uintptr_t)((3 * j + 1) << 37));
                sg[j] = reinterpret_cast<const void *>((uintptr_t)((3 * j + 2) << 37));
                z[j] = reinterpret_cast<void *>((uintptr_t)((3 * j + 3) << 37));
            }
            const hsw_permutation_product huge{0, 1, 1ull << 31, m, v.data(), nullptr, sg.data(), z.data(), ch, ch, omega, delta, nullptr};
            CHECK(refused(e, g, huge, HSW_ERR_TOO_LARGE, "too many tiles"));
        }
        // the overlap sweep: Z over a value column, Z over a sigma column, Z over Z; the text names the proof
        {
            std::vector<void *> zp(col.z);
            zp[1] = const_cast<void *>(col.v[3]);
            bad = ok; bad.d_products = zp.data();
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "proof 0: a Z column of its overlaps"));
            zp = col.z; zp[2] = static_cast<uint8_t *>(const_cast<void *>(col.sigma[4])) + 32 * 2999;      // row 0 of Z on the last cell of sigma
            bad.d_products = zp.data();
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "overlaps"));
            zp = col.z; zp[2] = static_cast<uint8_t *>(zp[0]) + 32 * 3000;                                // row 0 of Z_2 is row u of Z_0
            bad.d_products = zp.data();
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "overlaps"));
            std::vector<const void *> sp(col.sigma);
            sp[0] = static_cast<const uint8_t *>(col.z[1]) + 32 * 3000;                                   // a sigma column starts in row u of a Z
            bad = ok; bad.d_sigmas = sp.data();
            CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, "overlaps"));
            // ... while columns that are only read may be one and the same, and a value column with no assigned row lies anywhere
            std::vector<const void *> vp(col.v);
            vp[1] = col.v[0]; vp[2] = col.sigma[0]; vp[3] = col.z[0];
            const uint64_t rows[5] = {3000, 3000, 17, 0, 1};
            bad = ok; bad.d_columns = vp.data(); bad.column_rows = rows;
            CHECK(hip_stub_live_device_allocations() == live0);                   // nothing so far needed the scratch
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_permutation_product(g, &bad, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
        }
        CHECK(hip_stub_live_device_allocations() == live0 + 1);                   // the scratch
        {   // (K, m, L, u) = (1, 1, 1, 1)
            const Columns one(1, 1, 1, 1);
            const hsw_permutation_product a = one.args(ch, ch, omega, delta, status);
            const int l0 = hip_stub_launches();
            CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);   // tiles, scan, write
            CHECK(rep.proofs == 1 && rep.products == 1 && rep.written == 2 && rep.open_proofs == 0 && rep.refused_proofs == 0);
            CHECK(rep.first_open == ~0ull && rep.first_refused == ~0ull && rep.tile_rows == 1024 && status[0] == 0);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);               // the scratch was large enough
        }
        {   // twenty times the tiles: the scratch grows, once (replaced, not added)
            const Columns wide(1, 40, 1, 3000);
            const hsw_permutation_product a = wide.args(ch, ch, omega, delta, nullptr);                   // (no status array: allowed)
            CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK && rep.products == 40 && rep.written == 40 * 3001);
            CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK && hsw_gadget_permutation_product(g, &ok, &rep) == HSW_OK);
            CHECK(hip_stub_live_device_allocations() == live0 + 1);
        }
        CHECK(hip_stub_live_events() > 0);                                        // (the engine's own)
        hsw_gadget_destroy(g);                                                    // frees the scratch: the leak check at the end
        CHECK(hip_stub_live_device_allocations() < live0 + 1);
    }
    {   // ---- a pass whose batches differ in representation: refused, nothing launched; a reset clears it
        const size_t sizes[2] = {64, 64};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_ex(e, sizes, 2, 1, WHOLE, &g) == HSW_OK);
        const Columns col(1, 3, 2, 100);
        const hsw_permutation_product a = col.args(ch, ch, omega, delta, status);
        std::vector<uint8_t> msg(40, 7);
        const uint8_t *in[1] = {msg.data()};
        const size_t len[1] = {40}, pre[1] = {0};
        hsw_hash_result r[1];
        CHECK(hsw_gadget_digest_batch(g, 1, in, len, pre, r) == HSW_OK);
        CHECK(hsw_gadget_set_repr(g, HSW_REPR_MONTGOMERY) == HSW_OK);
        CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK);             // one batch so far: canonical
        CHECK(hsw_gadget_digest_batch(g, 1, in, len, pre, r) == HSW_OK);
        CHECK(refused(e, g, a, HSW_ERR_UNSUPPORTED, "differ in representation"));
        CHECK(hsw_gadget_reset(g) == HSW_OK);
        CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK && rep.products == 2 && rep.written == 2 * 101);
        hsw_gadget_destroy(g);
    }
    for (int which = 0; which < 2; which++) {   // ---- Context groups: (K, m, L, u) = (3, 5, 2, 1024) and (2, 4, 4, 2500)
        const size_t K = which ? 2 : 3, m = which ? 4 : 5, L = which ? 4 : 2, S = which ? 1 : 3;
        const uint64_t u = which ? 2500 : 1024;
        const size_t sizes[2] = {64, 128};
        hsw_gadget *g = nullptr;
        CHECK(hsw_gadget_create_contexts(e, sizes, 2, K, 1, WHOLE, &g) == HSW_OK);
        const Columns col(K, m, L, u);
        CHECK(col.S == S);
        hsw_permutation_product a = col.args(ch, ch, omega, delta, status);
        const size_t events = hip_stub_live_events(), live = hip_stub_live_device_allocations();
        const int l0 = hip_stub_launches();
        if (K == 3) {
            a.gammas = above;
            CHECK(refused(e, g, a, HSW_ERR_INVALID_ARG, "not below p"));          // the third Context's is above p
            a.gammas = ch;
        }
        // a proof's Z over another proof's value column: the Z's proof is named
        std::vector<void *> zp(col.z);
        zp[(K - 1) * S] = const_cast<void *>(col.v[0]);
        hsw_permutation_product bad = a;
        bad.d_products = zp.data();
        CHECK(refused(e, g, bad, HSW_ERR_INVALID_ARG, K == 3 ? "proof 2: a Z column of its overlaps" : "proof 1: a Z column of its overlaps"));
        std::memset(status, 0xff, sizeof status);
        CHECK(hsw_gadget_permutation_product(g, &a, &rep) == HSW_OK && hip_stub_launches() == l0 + 3);
        CHECK(rep.proofs == K && rep.products == K * S && rep.written == K * S * (u + 1) && rep.tile_rows == 1024);
        CHECK(rep.open_proofs == 0 && rep.refused_proofs == 0 && rep.first_open == ~0ull && rep.first_refused == ~0ull);
        for (size_t c = 0; c < K; c++) CHECK(status[c] == 0);
        CHECK(status[K] == 0xffffffffu);                                          // one word per proof
        CHECK(hip_stub_live_device_allocations() == live + 1 && hip_stub_live_events() == events);   // the calls' own events are gone
        hsw_gadget_destroy(g);
        CHECK(hip_stub_live_device_allocations() <= live);                        // the scratch went with the gadget's own buffers
    }
    hsw_engine_destroy(e);
    CHECK(hip_stub_live_device_allocations() == 0 && hip_stub_live_pinned_allocations() == 0 && hip_stub_live_events() == 0);
    std::printf("permutation product lifecycle ok\n");
    return 0;
}
