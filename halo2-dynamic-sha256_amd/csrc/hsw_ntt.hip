// hsw_ntt.hip -- the Fr NTT of device columns, natural order in and out.
//
// hsw_gadget_ntt (hsw_gadget_ntt.cpp).  The rules -- digits, tiles, twiddle exponents -- are hsw_ntt_value.hpp's; ONE
// kernel runs every launch of a transform, with fewer stages where a digit is short:
//   load    a workgroup per (tile, column), NTT_POINTS points per thread, consecutive lanes on consecutive cells, into
//           LDS limb-major (sh[limb][l]: every access 4 bytes at lane stride one).  Launch 0 reads the caller's column:
//           rows at and beyond its height are 0 and are not read, every cell read is checked against p, and with a
//           shift before the transform a cell is multiplied by g^(tile's base) g^(offset), the first from g's windows
//           (uniform over the workgroup), the second from a table of the tile.  A later launch reads the scratch and
//           multiplies by the inter-launch twiddle from the table of w's powers.
//   steps   two radix-2 stages per LDS round trip: a thread takes the four points that differ in two bits of the
//           field, runs the stage of the upper bit on (0,2) (1,3) and of the lower on (0,1) (2,3), and puts them back.
//           A field of odd width does its top bit alone first.  Field bit 0 multiplies by 1 and multiplies nothing.
//   store   consecutive lanes on consecutive cells of the destination, each read from LDS where the bit-reversed field
//           left it.  The last launch writes the caller's output at the digit-reversed address, times c or c g^i.
// A refused column: launch 0 sets the bit (a vector atomic), the last launch reads it before its first barrier and
// returns, workgroup-uniform; a transform of one launch decides in LDS between load and store.  Every thread reaches
// every barrier.  Cell indices are below 2^28 and stay 32-bit; the byte offset is formed in load_cell / store_cell from
// 2 * (size_t)i, and a twiddle's from the pointer arithmetic on const PFe *, both 64-bit.
// The LDS helpers are the product kernels', repeated here so that their translation units stay as they are.  Vector
// loads, vector stores and vector atomics only.
#include "hsw_ntt.h"

namespace hsw {

typedef unsigned int u32;

namespace {

enum : u32 { TILE = 1u << NTT_TILE_LOG };

__device__ __forceinline__ PFe load_cell(const uint4 *col, u32 i) {
    const uint4 a = col[2 * (size_t)i], b = col[2 * (size_t)i + 1];
    return PFe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void store_cell(uint4 *col, u32 i, const PFe &v) {
    col[2 * (size_t)i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    col[2 * (size_t)i + 1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ void lds_put(u32 *sh, u32 l, const PFe &v) {
    for (int j = 0; j < 8; j++) sh[j * TILE + l] = v.l[j];
}
__device__ __forceinline__ PFe lds_get(const u32 *sh, u32 l) {
    PFe v;
    for (int j = 0; j < 8; j++) v.l[j] = sh[j * TILE + l];
    return v;
}

// point l of the tile into LDS; false if a stored cell that was read is not below p
__device__ __forceinline__ bool ntt_load(const NttParams &p, const NttColumn &c, u32 base, u32 done, const PFe &g_base, u32 l, u32 *sh) {
    const NttPass &g = p.pass;
    PFe v = fr_zero();
    bool ok = true;
    if (l < (1u << ntt_tile_log(g))) {
        const u32 addr = base + ntt_offset(g, l);
        if (g.k == 0) {
            if (addr < c.rows) {
                v = load_cell(c.in, addr);
                ok = pfe_below_p(v);
                if (p.shift_in) v = fr_mont_mul(v, fr_mont_mul(g_base, p.tile_in[l]));
            }
        } else {
            const u32 I = g.k + 1 < g.n_pass ? done : ntt_done_index(p.plan, g.k, addr);
            v = fr_mont_mul(load_cell(c.scratch, addr), ntt_twiddle(p.twiddle, g.log_n, ntt_twiddle_exponent(g, ntt_field(g, l), I)));
        }
    }
    lds_put(sh, l, v);
    return ok;
}

// One LDS round trip: the stage of field bit fb_a over the pairs that differ in bit ql + 1 of l, then the stage of
// field bit fb_b over those that differ in bit ql.  Ends synchronised
__device__ __forceinline__ void ntt_step(const NttParams &p, u32 *sh, u32 ql, bool do_a, u32 fb_a, bool do_b, u32 fb_b) {
    const NttPass &g = p.pass;
    const u32 l0 = ntt_step_local(threadIdx.x, ql), q = 1u << ql;
    PFe x0 = lds_get(sh, l0), x1 = lds_get(sh, l0 + q), x2 = lds_get(sh, l0 + 2 * q), x3 = lds_get(sh, l0 + 3 * q);
    if (do_a) {
        ntt_butterfly(x0, x2, p.twiddle, ntt_stage_exponent(g, l0, fb_a), fb_a != 0);
        ntt_butterfly(x1, x3, p.twiddle, ntt_stage_exponent(g, l0 + q, fb_a), fb_a != 0);
    }
    if (do_b) {
        ntt_butterfly(x0, x1, p.twiddle, ntt_stage_exponent(g, l0, fb_b), fb_b != 0);
        ntt_butterfly(x2, x3, p.twiddle, ntt_stage_exponent(g, l0 + 2 * q, fb_b), fb_b != 0);
    }
    lds_put(sh, l0, x0); lds_put(sh, l0 + q, x1); lds_put(sh, l0 + 2 * q, x2); lds_put(sh, l0 + 3 * q, x3);
    __syncthreads();
}

// the lam-th store of the workgroup
__device__ __forceinline__ void ntt_store(const NttParams &p, const NttColumn &c, u32 base, const PFe &g_base, u32 lam, const u32 *sh) {
    const NttPass &g = p.pass;
    if (lam >= (1u << ntt_tile_log(g))) return;
    const u32 o = ntt_store_local(g, lam), addr = base + ntt_offset(g, o);
    PFe v = lds_get(sh, ntt_reverse_field(g, o));
    if (g.k + 1 < g.n_pass) { store_cell(c.scratch, addr, v); return; }
    if (p.out_mode == NTT_OUT_SCALE) v = fr_mont_mul(v, p.scale);
    else if (p.out_mode == NTT_OUT_TABLE) v = fr_mont_mul(v, fr_mont_mul(g_base, p.tile_out[lam]));
    store_cell(c.out, ntt_out_index(p.plan, addr), v);
}

}  // namespace

__global__ __launch_bounds__(NTT_THREADS) void hsw_ntt_kernel(NttParams p) {
    __shared__ u32 sh[8 * TILE];
    __shared__ u32 shBad;
    const NttPass &g = p.pass;
    const u32 t = threadIdx.x, col = blockIdx.y;
    const bool first = g.k == 0, last = g.k + 1 == g.n_pass;
    if (last && !first && (p.status[col] & NTT_CELL_NOT_BELOW_P)) return;   // (workgroup-uniform: decided by launch 0)
    const NttColumn c = p.cols[col];
    const u32 base = ntt_base(g, blockIdx.x);
    const u32 done = first ? 0u : ntt_done_index(p.plan, g.k, base);
    PFe g_base = fr_zero();
    if (first && p.shift_in) g_base = ntt_power(*p.shift, base);
    if (t == 0) shBad = 0;
    __syncthreads();
    bool ok = ntt_load(p, c, base, done, g_base, t, sh);
    ok = ntt_load(p, c, base, done, g_base, NTT_THREADS + t, sh) && ok;
    ok = ntt_load(p, c, base, done, g_base, 2 * NTT_THREADS + t, sh) && ok;
    ok = ntt_load(p, c, base, done, g_base, 3 * NTT_THREADS + t, sh) && ok;
    if (!ok) {
        if (last) atomicOr(&shBad, 1u);
        else atomicOr(&p.status[col], NTT_CELL_NOT_BELOW_P);
    }
    __syncthreads();
    int fb = (int)g.field_bits - 1;
    if (g.field_bits & 1u) {                                               // the top bit alone
        const u32 qh = g.field_shift + (u32)fb;
        if (qh >= 1) ntt_step(p, sh, qh - 1, true, (u32)fb, false, 0);
        else ntt_step(p, sh, 0, false, 0, true, 0);
        fb--;
    }
    for (; fb >= 1; fb -= 2) ntt_step(p, sh, g.field_shift + (u32)fb - 1, true, (u32)fb, true, (u32)fb - 1);
    if (last && first && shBad) {                                          // (workgroup-uniform; no barrier follows)
        if (t == 0) atomicOr(&p.status[col], NTT_CELL_NOT_BELOW_P);
        return;
    }
    if (last && p.out_mode == NTT_OUT_TABLE) g_base = ntt_power(*p.shift, ntt_out_index(p.plan, base));
    ntt_store(p, c, base, g_base, t, sh);
    ntt_store(p, c, base, g_base, NTT_THREADS + t, sh);
    ntt_store(p, c, base, g_base, 2 * NTT_THREADS + t, sh);
    ntt_store(p, c, base, g_base, 3 * NTT_THREADS + t, sh);
}

__global__ __launch_bounds__(NTT_THREADS) void hsw_ntt_twiddle_kernel(PFe *table, const NttWindows *windows, u32 count) {
    const u32 e = blockIdx.x * NTT_THREADS + threadIdx.x;
    if (e >= count) return;
    store_cell(reinterpret_cast<uint4 *>(table), e, ntt_power(*windows, e));
}

hipError_t launch_ntt_twiddles(PFe *table, const NttWindows *windows, uint32_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_ntt_twiddle_kernel, dim3((count + NTT_THREADS - 1) / NTT_THREADS), dim3(NTT_THREADS), 0, stream, table, windows, count);
    return hipGetLastError();
}

hipError_t launch_ntt_pass(const NttParams &p, uint32_t n_columns, hipStream_t stream) {
    if (n_columns == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_ntt_kernel, dim3(ntt_workgroups(p.pass), n_columns), dim3(NTT_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
