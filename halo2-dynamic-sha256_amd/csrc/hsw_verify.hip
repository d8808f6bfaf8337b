// hsw_verify.hip -- on-device check of a block witness against the gadget's constraint system.
//
// What MockProver::verify checks for the path (reference lib.rs:525-526), evaluated in HBM right where the
// witness was written: every gate row x0 + x1*x2 = x3, every copy constraint (QuantumCell::Existing and
// assert_equal), every fixed constant, every range_check bound, the spread-chip cells (tied to their gate
// cells, and (dense, spread) a row of the spread table), the lookup-column copies, the next-state words --
// with the block bytes and the pre-state entering only through the external cells they are
// copy-constrained to.  The structure is the product's own (csrc/hsw_structure.hpp); no value is
// recomputed from the inputs, so a stream that passes is the witness of its inputs by the uniqueness
// argument of SURVEY 8c.  One pass over the gate rows (four lanes per row, one cell each) checks the row
// equation and, on the same loads, the constants and copies among the row's cells; then the assert_equal
// pairs, range bounds, chip ties and lookup copies.  ~3.0 ms for 4,096 blocks (1.8x the time it took to
// write them).  `slices` workgroups may share a block: small batches are sliced to fill the chip.
#include "hsw_expand.hpp"
#include "hsw_frame.hpp"
#include "hsw_verify.h"

namespace hsw {

namespace {

struct Cell { u64 l[4]; };

DEV Cell load_cell(const uint4 *gate, u64 idx) {
    const uint4 a = gate[2 * idx], b = gate[2 * idx + 1];
    Cell c;
    c.l[0] = (u64)a.x | ((u64)a.y << 32); c.l[1] = (u64)a.z | ((u64)a.w << 32);
    c.l[2] = (u64)b.x | ((u64)b.y << 32); c.l[3] = (u64)b.z | ((u64)b.w << 32);
    return c;
}
// HSW_REPR_MONTGOMERY streams are checked in the canonical domain: every loaded cell m = x * 2^256 mod p is
// reduced to x on the fly (one Montgomery reduction) wherever its VALUE is needed -- gate equation, constants, ranges;
// copies of stream cells are compared as stored.  3.1-3.3 ms per 4,096 blocks against 3.0 ms canonical.
DEV Cell from_mont(const Cell &a) {
    const u64 P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    const u64 INV = 0xc2e1f593efffffffull;                       // -p^-1 mod 2^64
    u64 t[5] = {a.l[0], a.l[1], a.l[2], a.l[3], 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 m = t[0] * INV;
        unsigned __int128 s = (unsigned __int128)m * P[0] + t[0];
        u64 carry = (u64)(s >> 64);
#pragma unroll
        for (int j = 1; j < 4; j++) {
            s = (unsigned __int128)m * P[j] + t[j] + carry;
            t[j - 1] = (u64)s;
            carry = (u64)(s >> 64);
        }
        s = (unsigned __int128)t[4] + carry;
        t[3] = (u64)s;
        t[4] = (u64)(s >> 64);
    }
    Cell r;
    r.l[0] = t[0]; r.l[1] = t[1]; r.l[2] = t[2]; r.l[3] = t[3];
    // r < 2p: one conditional subtraction
    bool ge = t[4] != 0;
    if (!ge) { ge = true; for (int i = 3; i >= 0; i--) { if (r.l[i] > P[i]) break; if (r.l[i] < P[i]) { ge = false; break; } } }
    if (ge) { u64 br = 0; for (int i = 0; i < 4; i++) { const unsigned __int128 d = (unsigned __int128)r.l[i] - P[i] - br; r.l[i] = (u64)d; br = (u64)(d >> 64) & 1; } }
    return r;
}
template <bool MONT>
DEV Cell load_value(const uint4 *base, u64 idx) {
    const Cell c = load_cell(base, idx);
    if constexpr (MONT) return from_mont(c); else return c;
}
DEV bool narrow(const Cell &c) { return (c.l[1] | c.l[2] | c.l[3]) == 0; }
DEV bool same(const Cell &a, const Cell &b) { return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3]; }
DEV Cell small(u64 v) { Cell c; c.l[0] = v; c.l[1] = c.l[2] = c.l[3] = 0; return c; }

// FlexGate column packing: where stream cell i sits
template <class P>
DEV u64 place(const P &p, u64 i) {
    u64 gap = 0;
    for (u32 k = 0; k < p.n_breaks; k++) gap += p.break_cell[k] <= i ? p.break_gap[k] : 0;
    return i + gap;
}

// ---- generic field arithmetic for the few full-width rows of a digest frame (is_zero's z + a*inv = 1, the
// differences of is_equal / select): canonical 4 x u64 limbs, double-and-add -- slow and simple; a frame has
// a few hundred such rows, a block none beyond the negation pattern handled inline.
DEV bool geq_p(const Cell &a) {
    const u64 P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    for (int i = 3; i >= 0; i--) { if (a.l[i] > P[i]) return true; if (a.l[i] < P[i]) return false; }
    return true;
}
DEV Cell sub_p(const Cell &a) {
    const u64 P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    Cell r; u64 br = 0;
    for (int i = 0; i < 4; i++) { const unsigned __int128 d = (unsigned __int128)a.l[i] - P[i] - br; r.l[i] = (u64)d; br = (u64)(d >> 64) & 1; }
    return r;
}
DEV Cell add_mod(const Cell &a, const Cell &b) {          // a, b < p < 2^254: no carry out of 256 bits
    Cell r; u64 cy = 0;
    for (int i = 0; i < 4; i++) { const unsigned __int128 s = (unsigned __int128)a.l[i] + b.l[i] + cy; r.l[i] = (u64)s; cy = (u64)(s >> 64); }
    return geq_p(r) ? sub_p(r) : r;
}
DEV Cell neg_mod(const Cell &a) {                           // p - a (0 stays 0)
    if ((a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0) return a;
    const u64 P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    Cell r; u64 br = 0;
    for (int i = 0; i < 4; i++) { const unsigned __int128 d = (unsigned __int128)P[i] - a.l[i] - br; r.l[i] = (u64)d; br = (u64)(d >> 64) & 1; }
    return r;
}
// a * k for a 64-bit k: double-and-add from k's top bit
DEV Cell mul_small(const Cell &a, u64 k) {
    Cell r = small(0);
    if (k == 0) return r;
    for (int bit = 63 - __builtin_clzll(k); bit >= 0; bit--) {
        r = add_mod(r, r);
        if ((k >> bit) & 1) r = add_mod(r, a);
    }
    return r;
}
// a * b: through the operand that is small, or the negation of something small (the differences n - target,
// state_n - state_target, -2^16 of a frame are); both full width only for corrupted cells
DEV Cell mul_mod(const Cell &a, const Cell &b) {
    if (narrow(b)) return mul_small(a, b.l[0]);
    if (narrow(a)) return mul_small(b, a.l[0]);
    const Cell nb = neg_mod(b);
    if (narrow(nb)) return neg_mod(mul_small(a, nb.l[0]));
    const Cell na = neg_mod(a);
    if (narrow(na)) return neg_mod(mul_small(b, na.l[0]));
    Cell r = small(0);
    for (int bit = 255; bit >= 0; bit--) {
        r = add_mod(r, r);
        if ((b.l[bit >> 6] >> (bit & 63)) & 1) r = add_mod(r, a);
    }
    return r;
}
// x0 + x1*x2 == x3 (mod p) for canonical cells
DEV bool row_holds(const Cell x[4]) {
    if (narrow(x[0]) && narrow(x[1]) && narrow(x[2]) && narrow(x[3])) {
        const unsigned __int128 s = (unsigned __int128)x[1].l[0] * x[2].l[0] + x[0].l[0];
        return (u64)(s >> 64) == 0 && (u64)s == x[3].l[0];
    }
    if (geq_p(x[0]) || geq_p(x[1]) || geq_p(x[2]) || geq_p(x[3])) return false;     // not canonical
    return same(add_mod(x[0], mul_mod(x[1], x[2])), x[3]);
}

}  // namespace

// TABLE (shared contexts, hsw_kernels.h PlaceTable): stream cells placed by the jump table -- launch-relative cell i
// sits at i + the gaps of the jumps at or before tbl->base + i -- and the block's lookup entries shifted past the
// caller's entries queued before its digest.
template <bool MONT>
__global__ __launch_bounds__(256) void hsw_verify_kernel(VerifyParams p) {
    constexpr bool TABLE = false, WIDE = false;
    const PlaceTable *tbl = nullptr;
    (void)tbl;
#include "hsw_verify_block_body.inc"
}
// shared contexts (HSW_GADGET_SHARED_CONTEXT): the same checks, placed by a jump table
template <bool MONT>
__global__ __launch_bounds__(256) void hsw_verify_table_kernel(VerifyParams p, PlaceTable t) {
    constexpr bool TABLE = true, WIDE = false;
    const PlaceTable *tbl = &t;
#include "hsw_verify_block_body.inc"
}

// ---------------------------------------------------------------- digest frames
// One workgroup per digest: prologue and epilogue cells against their structure, plus the links a
// replayer would make by copy constraints and this check makes through the arrays both sides were checked
// against: input length / rounds, the initial state, the input bytes, pre-state of block b = next state of
// block b - 1, the candidate states of the epilogue.
// TABLE: frame cells placed by the jump table (absolute stream cells); the lookup indices are absolute already.
template <bool MONT>
__global__ __launch_bounds__(256) void hsw_verify_frame_kernel(FrameVerifyParams p) {
    constexpr bool TABLE = false;
    const PlaceTable *tbl = nullptr;
    (void)tbl;
#include "hsw_verify_frame_body.inc"
}
// shared contexts (HSW_GADGET_SHARED_CONTEXT): the same checks, placed by a jump table
template <bool MONT>
__global__ __launch_bounds__(256) void hsw_verify_frame_table_kernel(FrameVerifyParams p, PlaceTable t) {
    constexpr bool TABLE = true;
    const PlaceTable *tbl = &t;
#include "hsw_verify_frame_body.inc"
}

// Columns by pointer table (PlaceTable::cum_stride != 0): every Context is checked through its own cum row (overloads,
// so that the kernels above keep their names and code).
template <bool MONT, bool WIDE>
__global__ __launch_bounds__(256) void hsw_verify_table_kernel(VerifyParams p, PlaceTable t) {
    static_assert(WIDE, "the wide instantiation only");
    constexpr bool TABLE = true;
    // the block's Context (a launch over several Contexts: one per frame_every blocks), workgroup-uniform
    if (t.ctx_blocks) t.cum += (t.ctx0 + (blockIdx.x / p.slices) / p.frame_every) * t.cum_stride;
    const PlaceTable *tbl = &t;
#include "hsw_verify_block_body.inc"
}
template <bool MONT, bool WIDE>
__global__ __launch_bounds__(256) void hsw_verify_frame_table_kernel(FrameVerifyParams p, PlaceTable t) {
    static_assert(WIDE, "the wide instantiation only");
    constexpr bool TABLE = true;
    if (p.ctx_stream) t.cum += (p.descs[blockIdx.x].prologue_cell / p.ctx_stream) * t.cum_stride;
    const PlaceTable *tbl = &t;
#include "hsw_verify_frame_body.inc"
}

// ---------------------------------------------------------------- copy constraints between any two cells
// hsw_gadget_verify_ties / hsw_gadget_verify_equal: the host has resolved both cells of every pair to device addresses
// (Context::cell_offset: layout, jumps, Context images, pitches and pointer tables are all in the address), so the
// kernel knows no layout.  One lane per pair, each cell two 16-byte loads, compared as stored; a failing lane counts
// itself and offers its index as the first.
__global__ __launch_bounds__(256) void hsw_verify_pairs_kernel(const CellPair *pairs, u64 n, VerifyReport *report) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const CellPair pr = pairs[i];
    const Cell a = load_cell(static_cast<const uint4 *>(pr.a), 0), b = load_cell(static_cast<const uint4 *>(pr.b), 0);
    if (!same(a, b)) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&report->violations), 1ull);
        atomicMin(reinterpret_cast<unsigned long long *>(&report->first_key), (unsigned long long)i);
    }
}

hipError_t launch_verify_pairs(const CellPair *d_pairs, size_t n, VerifyReport *report, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_verify_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_pairs, (u64)n, report);
    return hipGetLastError();
}

hipError_t launch_verify_frames_table(const FrameVerifyParams &p, const PlaceTable &t, size_t n_digests, hipStream_t stream) {
    if (n_digests == 0) return hipSuccess;
    if (t.cum_stride) {
        if (p.montgomery) hipLaunchKernelGGL((hsw_verify_frame_table_kernel<true, true>), dim3((unsigned)n_digests), dim3(256), 0, stream, p, t);
        else hipLaunchKernelGGL((hsw_verify_frame_table_kernel<false, true>), dim3((unsigned)n_digests), dim3(256), 0, stream, p, t);
        return hipGetLastError();
    }
    if (p.montgomery) hipLaunchKernelGGL(hsw_verify_frame_table_kernel<true>, dim3((unsigned)n_digests), dim3(256), 0, stream, p, t);
    else hipLaunchKernelGGL(hsw_verify_frame_table_kernel<false>, dim3((unsigned)n_digests), dim3(256), 0, stream, p, t);
    return hipGetLastError();
}

hipError_t launch_verify_table(const VerifyParams &p, const PlaceTable &t, size_t n_blocks, hipStream_t stream) {
    if (n_blocks == 0) return hipSuccess;
    if (t.cum_stride) {
        if (p.montgomery) hipLaunchKernelGGL((hsw_verify_table_kernel<true, true>), dim3((unsigned)(n_blocks * p.slices)), dim3(256), 0, stream, p, t);
        else hipLaunchKernelGGL((hsw_verify_table_kernel<false, true>), dim3((unsigned)(n_blocks * p.slices)), dim3(256), 0, stream, p, t);
        return hipGetLastError();
    }
    if (p.montgomery) hipLaunchKernelGGL(hsw_verify_table_kernel<true>, dim3((unsigned)(n_blocks * p.slices)), dim3(256), 0, stream, p, t);
    else hipLaunchKernelGGL(hsw_verify_table_kernel<false>, dim3((unsigned)(n_blocks * p.slices)), dim3(256), 0, stream, p, t);
    return hipGetLastError();
}

hipError_t launch_verify_frames(const FrameVerifyParams &p, size_t n_digests, hipStream_t stream) {
    if (n_digests == 0) return hipSuccess;
    if (p.montgomery) hipLaunchKernelGGL(hsw_verify_frame_kernel<true>, dim3((unsigned)n_digests), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(hsw_verify_frame_kernel<false>, dim3((unsigned)n_digests), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_verify(const VerifyParams &p, size_t n_blocks, hipStream_t stream) {
    if (n_blocks == 0) return hipSuccess;
    if (p.montgomery) hipLaunchKernelGGL(hsw_verify_kernel<true>, dim3((unsigned)(n_blocks * p.slices)), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(hsw_verify_kernel<false>, dim3((unsigned)(n_blocks * p.slices)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hsw
