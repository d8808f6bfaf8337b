// hsw_permutation_product.h -- launch interface of the permutation argument's grand products (hsw_permutation_product.hip;
// hsw_gadget_permutation_product in hsw_gadget_permutation.cpp is its only caller).
#ifndef HSW_PERMUTATION_PRODUCT_H
#define HSW_PERMUTATION_PRODUCT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hsw_lookup_product.h"
#include "hsw_permutation_value.hpp"

namespace hsw {

static_assert(PRODUCT_THREADS == PERMUTATION_TABLE, "one entry of PermutationPowers::thread per thread of a workgroup");
static_assert((1ull << 31) / PRODUCT_TILE < (1ull << PERMUTATION_TILE_BITS) - 1, "a tile index of u = 2^31 has its binary powers");

// One value column of one proof (cells of two uint4 each, 16-byte aligned)
struct PermutationColumn {
    const uint4 *v;
    uint32_t rows, reserved_;      // rows of v that are read; the rest count as 0
};

// Tiles, status bits and thread geometry are the lookup product's (PRODUCT_* of hsw_lookup_product.h).  The tiles of a
// proof are those of its chunks one after the other, (s, tile) at s * n_tiles + tile: the prefix over them IS the chain
// Z_s[0] = Z_{s-1}[u].
struct PermutationParams {
    const PermutationColumn *cols;     // n_proofs x m
    const PFe *beta_delta;             // n_proofs x m: beta_c delta^j in cell form
    const uint4 *const *sigmas;        // m columns of u cells, shared by the proofs
    uint4 *const *z;                   // n_proofs x S columns of u + 1 cells
    const PermutationChallenges *ch;   // per proof
    const PermutationPowers *powers;
    PFe seed_full, seed_last;          // permutation_seed of a chunk of L columns and of the last chunk
    uint32_t n_proofs, m, L, S;
    uint32_t n_tiles, u;               // n_tiles = ceil((u + 1) / PRODUCT_TILE) per chunk
    PFe *tiles;                        // n_proofs x S x n_tiles x 2: a tile's two products, then its factor of the write stage
    uint32_t *status;                  // n_proofs, zeroed by the caller
};

// every tile's product of num and of den into tiles[][0 / 1]; a stored cell that is not below p sets the proof's bit
hipError_t launch_permutation_tiles(const PermutationParams &p, bool montgomery, hipStream_t stream);
// per proof: tiles[t][0] = (numerators of the tiles before t) x (denominators of the tiles after t) / D; D = 0 sets
// PRODUCT_ZERO_DENOM
hipError_t launch_permutation_scan(const PermutationParams &p, hipStream_t stream);
// the S columns of every proof that is not refused; Z_{S-1}[u] != 1 sets PRODUCT_OPEN
hipError_t launch_permutation_write(const PermutationParams &p, bool montgomery, hipStream_t stream);

}  // namespace hsw
#endif
