// hsw_quotient.h -- launch interface of the quotient h(X) of device columns (hsw_quotient.hip; hsw_gadget_quotient in
// hsw_gadget_quotient.cpp is its only caller).
#ifndef HSW_QUOTIENT_H
#define HSW_QUOTIENT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_quotient_value.hpp"

namespace hsw {

// Every launch: n proofs from proof `base` on, whose V is p.V + (proof - base) N.  gates, permutation and lookups fold
// their family into V (p.first: V starts at 0); finish writes h of the proofs whose status word is clear
hipError_t launch_quotient_gates(const QuotientParams &p, uint32_t base, uint32_t n, hipStream_t stream);
hipError_t launch_quotient_permutation(const QuotientParams &p, uint32_t base, uint32_t n, bool montgomery, hipStream_t stream);
hipError_t launch_quotient_lookups(const QuotientParams &p, uint32_t base, uint32_t n, bool montgomery, hipStream_t stream);
hipError_t launch_quotient_finish(const QuotientParams &p, uint32_t base, uint32_t n, hipStream_t stream);

}  // namespace hsw
#endif
