// hsw_quotient.hip -- the quotient h(X) of device columns on the extended coset, written on the device.
//
// hsw_gadget_quotient (hsw_gadget_quotient.cpp).  The row rules are hsw_quotient_value.hpp's; a kernel per family, all
// on the stream and nothing read by the host in between:
//   gates        a thread owns QUOTIENT_ROWS consecutive extended rows of one proof (blockIdx.y), a workgroup a tile of
//                512.  A loop over the gates, their monomials and factors, whose descriptors (offsets, column indices,
//                rotations as row offsets, coefficients) are read from device memory with indices that do not depend on
//                the thread; one running product and one sum per row in registers, V folded per gate.
//   permutation  the same rows: l0 (1 - Z_0), l_last (Z^2 - Z), the S - 1 links, then per set the two products over the
//                set's columns.  w^row comes from the staged powers: lane 0 multiplies up the tile's, shared through
//                LDS, a thread goes on from its table entry and by w per row.
//   lookups      per lookup the theta folds of its input and table columns and the five expressions.
//   finish       h = V t_inv[row mod 2^e], stored only if the proof's status word is clear.
// V lives in the gadget's scratch between launches, N cells per proof of the batch; the first launch of a batch starts
// from 0 and reads none of it.  Every stored cell that is read is checked against p; a cell that is not below p sets the
// proof's status word and the arithmetic goes on with garbage, never out of range: every row index is taken mod N.
// Vector loads, vector stores and vector atomics only.
#include "hsw_quotient.h"

namespace hsw {

typedef unsigned int u32;

namespace {

// w^(the thread's first row), in Montgomery form.  Ends synchronised
__device__ __forceinline__ PFe quotient_row0_power(const QuotientParams &p, u32 tile, u32 *shW) {
    const u32 t = threadIdx.x;
    if (t == 0) {
        const PFe w = permutation_omega_tile(*p.powers, tile);
        for (int j = 0; j < 8; j++) shW[j] = w.l[j];
    }
    __syncthreads();
    PFe w;
    for (int j = 0; j < 8; j++) w.l[j] = shW[j];
    return permutation_omega_thread(*p.powers, w, t);
}

}  // namespace

__global__ __launch_bounds__(QUOTIENT_THREADS) void hsw_quotient_gates_kernel(QuotientParams p, u32 base) {
    const u32 c = base + blockIdx.y, row0 = (blockIdx.x * QUOTIENT_THREADS + threadIdx.x) * QUOTIENT_ROWS;
    if (row0 >= p.N) return;
    PFe *Vb = p.V + (size_t)blockIdx.y * p.N;
    PFe V[QUOTIENT_ROWS];
    quotient_begin(p, Vb, row0, V);
    if (!quotient_gates_rows(p, c, row0, V)) atomicOr(&p.status[c], QUOTIENT_CELL_NOT_BELOW_P);
    quotient_end(Vb, row0, V);
}

template <bool MONT>
__global__ __launch_bounds__(QUOTIENT_THREADS) void hsw_quotient_permutation_kernel(QuotientParams p, u32 base) {
    __shared__ u32 shW[8];
    const u32 c = base + blockIdx.y, row0 = (blockIdx.x * QUOTIENT_THREADS + threadIdx.x) * QUOTIENT_ROWS;
    const PFe x0 = quotient_row0_power(p, blockIdx.x, shW);
    if (row0 >= p.N) return;
    PFe *Vb = p.V + (size_t)blockIdx.y * p.N;
    PFe V[QUOTIENT_ROWS];
    quotient_begin(p, Vb, row0, V);
    if (!quotient_permutation_rows<MONT>(p, c, row0, x0, V)) atomicOr(&p.status[c], QUOTIENT_CELL_NOT_BELOW_P);
    quotient_end(Vb, row0, V);
}

template <bool MONT>
__global__ __launch_bounds__(QUOTIENT_THREADS) void hsw_quotient_lookups_kernel(QuotientParams p, u32 base) {
    const u32 c = base + blockIdx.y, row0 = (blockIdx.x * QUOTIENT_THREADS + threadIdx.x) * QUOTIENT_ROWS;
    if (row0 >= p.N) return;
    PFe *Vb = p.V + (size_t)blockIdx.y * p.N;
    PFe V[QUOTIENT_ROWS];
    quotient_begin(p, Vb, row0, V);
    if (!quotient_lookups_rows<MONT>(p, c, row0, V)) atomicOr(&p.status[c], QUOTIENT_CELL_NOT_BELOW_P);
    quotient_end(Vb, row0, V);
}

__global__ __launch_bounds__(QUOTIENT_THREADS) void hsw_quotient_finish_kernel(QuotientParams p, u32 base) {
    const u32 c = base + blockIdx.y, row0 = (blockIdx.x * QUOTIENT_THREADS + threadIdx.x) * QUOTIENT_ROWS;
    if (row0 >= p.N) return;
    if (p.status[c] & QUOTIENT_CELL_NOT_BELOW_P) return;          // (decided before this launch)
    quotient_finish_rows(p, p.V + (size_t)blockIdx.y * p.N, p.h[c], row0);
}

namespace {
dim3 quotient_grid(const QuotientParams &p, uint32_t n) { return dim3((p.N + QUOTIENT_TILE - 1) / QUOTIENT_TILE, n); }
}  // namespace

hipError_t launch_quotient_gates(const QuotientParams &p, uint32_t base, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_quotient_gates_kernel, quotient_grid(p, n), dim3(QUOTIENT_THREADS), 0, stream, p, base);
    return hipGetLastError();
}

hipError_t launch_quotient_permutation(const QuotientParams &p, uint32_t base, uint32_t n, bool montgomery, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (montgomery) hipLaunchKernelGGL(hsw_quotient_permutation_kernel<true>, quotient_grid(p, n), dim3(QUOTIENT_THREADS), 0, stream, p, base);
    else hipLaunchKernelGGL(hsw_quotient_permutation_kernel<false>, quotient_grid(p, n), dim3(QUOTIENT_THREADS), 0, stream, p, base);
    return hipGetLastError();
}

hipError_t launch_quotient_lookups(const QuotientParams &p, uint32_t base, uint32_t n, bool montgomery, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (montgomery) hipLaunchKernelGGL(hsw_quotient_lookups_kernel<true>, quotient_grid(p, n), dim3(QUOTIENT_THREADS), 0, stream, p, base);
    else hipLaunchKernelGGL(hsw_quotient_lookups_kernel<false>, quotient_grid(p, n), dim3(QUOTIENT_THREADS), 0, stream, p, base);
    return hipGetLastError();
}

hipError_t launch_quotient_finish(const QuotientParams &p, uint32_t base, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hsw_quotient_finish_kernel, quotient_grid(p, n), dim3(QUOTIENT_THREADS), 0, stream, p, base);
    return hipGetLastError();
}

}  // namespace hsw
