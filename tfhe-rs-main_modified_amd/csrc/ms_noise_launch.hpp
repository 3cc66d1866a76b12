// ms_noise_launch.hpp — host entry points of ms_noise_reduction.hip (the drift-technique modulus switch noise
// reduction, core_crypto/algorithms/modulus_switch_noise_reduction.rs).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ms_noise_measure.hpp"

namespace mi {

// The prepared key: tiles of 64 candidates, word-major inside a tile, tile[c / 64][j][c % 64] with j over the lwe_dim
// mask words and then the body; the lanes of the last tile beyond zeros_count hold 0 and are never read as candidates.
struct MsNoiseGeometry {
  size_t lwe_dim = 0, zeros_count = 0;
};
inline size_t ms_noise_tiles(const MsNoiseGeometry& g) { return (g.zeros_count + 63) / 64; }
inline size_t ms_noise_key_bytes(const MsNoiseGeometry& g) { return ms_noise_tiles(g) * (g.lwe_dim + 1) * 64 * 8; }
// zeros: zeros_count rows of lwe_dim + 1 u64 (the LweCiphertextList layout)
hipError_t launch_ms_noise_prepare(uint64_t* tiles, const uint64_t* zeros, const MsNoiseGeometry& g, hipStream_t s);

// What one launch writes; a NULL pointer is an output not asked for.
struct MsNoiseOut {
  double* measures = nullptr;    // [b * stride]: the measure of lwe_in[b]; all_candidates: [b * stride + 1 + c] too
  int all_candidates = 0;        // run every tile to the end (stride 1 + zeros_count) instead of choosing
  int64_t* candidate = nullptr;  // -1 (NoAddition) or the index of the added encryption of zero
  int32_t* satisfied = nullptr;  // 1 (SatisfyingBound) or 0 (BestNotSatisfyingBound)
  uint64_t* lwe = nullptr;       // lwe_in[b] + the chosen zero (may be lwe_in), or that through the standard switch
  int switched = 0;
};
hipError_t launch_ms_noise(const MsNoiseOut& out, const uint64_t* tiles, const MsNoiseGeometry& g,
                           const msn::Params& p, const uint64_t* lwe_in, size_t batch, int log_modulus, hipStream_t s);

}  // namespace mi
