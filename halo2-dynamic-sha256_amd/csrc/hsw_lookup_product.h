// hsw_lookup_product.h -- launch interface of the lookup argument's grand product (hsw_lookup_product.hip;
// hsw_gadget_lookup_product in hsw_gadget_product.cpp is its only caller).
#ifndef HSW_LOOKUP_PRODUCT_H
#define HSW_LOOKUP_PRODUCT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_product_value.hpp"

namespace hsw {

enum : uint32_t { PRODUCT_TILE = 1024, PRODUCT_THREADS = 256, PRODUCT_ROWS = PRODUCT_TILE / PRODUCT_THREADS };   // rows of Z per workgroup / per thread

// status bits of an argument on the device: HSW_PRODUCT_* of include/hsw.h
enum : uint32_t { PRODUCT_OPEN = 1, PRODUCT_ZERO_DENOM = 2, PRODUCT_CELL_NOT_BELOW_P = 4, PRODUCT_REFUSED = 6 };

// One argument, as the three stages take it (cells of two uint4 each, 16-byte aligned)
struct ProductArg {
    const uint4 *in, *in_spread;   // RANGE: the lookup-advice column, NULL; SPREAD: the dense and the spread column
    const uint4 *pin, *ptab;       // A' and S': u cells
    uint4 *z;                      // Z: u + 1 cells
    uint32_t input_rows;           // rows of in / in_spread that are read; the rest count as 0
    uint32_t context;              // whose challenges
};

struct ProductParams {
    const ProductArg *args;
    const ProductChallenges *ch;   // per context
    uint32_t n_args, n_tiles;      // n_tiles = ceil((u + 1) / PRODUCT_TILE) per argument
    uint32_t T, u, kind;           // kind: PERMUTED_VALUE_* of hsw_lookup_permuted.h
    PFe *tiles;                    // n_args x n_tiles x 2: a tile's two products, then its factor of the write stage
    uint32_t *status;              // n_args, zeroed by the caller
};

// every tile's product of num and of den into tiles[][0 / 1]; a stored cell that is not below p sets the argument's bit
hipError_t launch_product_tiles(const ProductParams &p, bool montgomery, hipStream_t stream);
// per argument: tiles[t][0] = (numerators of the tiles before t) x (denominators of the tiles after t) / D; D = 0 sets
// PRODUCT_ZERO_DENOM
hipError_t launch_product_scan(const ProductParams &p, hipStream_t stream);
// Z of every argument that is not refused; Z[u] != 1 sets PRODUCT_OPEN
hipError_t launch_product_write(const ProductParams &p, bool montgomery, hipStream_t stream);

}  // namespace hsw
#endif
