// lwe_linear_algebra_launch.hpp — host entry points of lwe_linear_algebra.hip: the gathered linear combination of LWE
// rows (core_crypto/algorithms/lwe_linear_algebra.rs, the CUDA backend's lwe_indexes_in / lwe_indexes_out) and the
// index patterns of the radix drivers (c_api_shortint.cpp), which are written on the device so that no driver copies
// from the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mi {

// out[i] = sum_t coeff[i * terms + t] * in[index[i * terms + t]] + (0, ..., 0, plaintext[i]) over rows of `words` u64,
// wrapping; a term whose index is >= n_in contributes nothing; coeff nullptr: every coefficient 1; plaintext nullptr:
// nothing added
hipError_t launch_lwe_linear_combination(uint64_t* out, const uint64_t* in, size_t words, size_t n_in, size_t n_out,
                                         size_t terms, const uint32_t* index, const int64_t* coeff,
                                         const uint64_t* plaintext, hipStream_t s);

// The one rule every row index of the radix drivers is an instance of (c_api_shortint.cpp), for j < count:
//   v = j % period; q = v / block, r = v % block  (the integer and the block of item v)
//   idx[j] = r < r_min ? 0xFFFFFFFF : base + q * q_mul + (r - r_sub)
struct IndexRule {
  uint32_t period, block, r_min, base, q_mul, r_sub;
};
hipError_t launch_index_rule(uint32_t* idx, size_t count, IndexRule rule, hipStream_t s);
// idx[j] = j < split ? lo : ((j - split) % block == 0 ? first : rest): the LUT of each item of a round
hipError_t launch_lut_rule(uint32_t* idx, size_t count, size_t split, uint32_t lo, size_t block, uint32_t first,
                           uint32_t rest, hipStream_t s);
// idx[2 j] = a[j], idx[2 j + 1] = b[j]: two index arrays interleaved into the (n_out x 2) array of a two-term call;
// coeff (when not nullptr) gets (ca, cb) per row
hipError_t launch_index_pairs(uint32_t* idx, int64_t* coeff, const uint32_t* a, const uint32_t* b, size_t count,
                              int64_t ca, int64_t cb, hipStream_t s);
// lut_eff[j] = in_index[j] < n_in ? (lut_index ? lut_index[j] : j) : 0xFFFFFFFF: an item whose input is out of range
// keeps its output row (mi_shortint_apply_lut_batch)
hipError_t launch_mask_lut_index(uint32_t* lut_eff, const uint32_t* in_index, const uint32_t* lut_index, size_t n_in,
                                 size_t count, hipStream_t s);

}  // namespace mi
