// lwe_linear_algebra.hip — the linear algebra of LWE ciphertexts over batches, with gather.
//
// Reference: tfhe/src/core_crypto/algorithms/lwe_linear_algebra.rs — lwe_ciphertext_add_assign (:67) and _add (:190),
// lwe_ciphertext_plaintext_add_assign (:275) and _plaintext_sub_assign (:383), lwe_ciphertext_opposite_assign (:490),
// lwe_ciphertext_cleartext_mul_assign (:555) and _cleartext_mul (:624), lwe_ciphertext_sub_assign (:702) and _sub
// (:789), each in its native_mod_compatible form; and the
// input / output index arrays of the CUDA backend (lwe_indexes_in / lwe_indexes_out, backends/tfhe-cuda-backend/cuda/
// include/pbs/programmable_bootstrap.h), which are the gather of one term with coefficient 1.
//
// One kernel: output row i is the wrapping sum of up to `terms` input rows, each picked by an index and scaled by a
// signed cleartext, plus a plaintext on the body.  It is memory-bound: every thread moves one 8-byte word of a row per
// step, consecutive threads consecutive words, so a wave reads and writes 512 contiguous bytes.  Rows are lwe_dim + 1
// words, an odd count at every real shape: a row starts 8-byte aligned and not 16-byte aligned, so the words are not
// widened to 16 bytes.  The indices and coefficients of a row are the same for every thread of a tile (scalar loads).
// The grid is capped and strides over the tiles (row, chunk of 256 words).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lwe_linear_algebra_launch.hpp"

namespace mi {
namespace lin {

using u64 = uint64_t;

constexpr unsigned MAX_BLOCKS = 256u * 16u;  // 16 workgroups of 256 threads per CU

__device__ __forceinline__ uint64_t gs_start() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t gs_step() { return (uint64_t)gridDim.x * blockDim.x; }

static unsigned blocks_for(uint64_t count) {
  const uint64_t b = (count + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

__global__ __launch_bounds__(256) void linear_combination_kernel(u64* __restrict__ out, const u64* __restrict__ in,
                                                                 uint32_t words, uint32_t chunks, uint64_t n_in,
                                                                 uint64_t n_out, uint32_t terms,
                                                                 const uint32_t* __restrict__ index,
                                                                 const int64_t* __restrict__ coeff,
                                                                 const u64* __restrict__ plaintext) {
  const uint64_t tiles = n_out * chunks;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t row = tile / chunks;
    const uint32_t w = (uint32_t)(tile % chunks) * 256u + threadIdx.x;
    if (w >= words) continue;
    u64 acc = 0;
    for (uint32_t t = 0; t < terms; ++t) {
      const uint64_t src = index[row * terms + t];
      if (src >= n_in) continue;
      const u64 c = coeff ? (u64)coeff[row * terms + t] : (u64)1;
      acc += c * in[src * words + w];
    }
    if (plaintext && w == words - 1) acc += plaintext[row];
    out[row * words + w] = acc;
  }
}

__global__ __launch_bounds__(256) void index_rule_kernel(uint32_t* __restrict__ idx, uint64_t count, IndexRule rule) {
  for (uint64_t j = gs_start(); j < count; j += gs_step()) {
    const uint32_t v = (uint32_t)(j % rule.period), q = v / rule.block, r = v % rule.block;
    idx[j] = r < rule.r_min ? 0xFFFFFFFFu : rule.base + q * rule.q_mul + (r - rule.r_sub);
  }
}

__global__ __launch_bounds__(256) void lut_rule_kernel(uint32_t* __restrict__ idx, uint64_t count, uint64_t split,
                                                       uint32_t lo, uint64_t block, uint32_t first, uint32_t rest) {
  for (uint64_t j = gs_start(); j < count; j += gs_step())
    idx[j] = j < split ? lo : ((j - split) % block == 0 ? first : rest);
}

__global__ __launch_bounds__(256) void index_pairs_kernel(uint32_t* __restrict__ idx, int64_t* __restrict__ coeff,
                                                          const uint32_t* __restrict__ a,
                                                          const uint32_t* __restrict__ b, uint64_t count, int64_t ca,
                                                          int64_t cb) {
  for (uint64_t j = gs_start(); j < count; j += gs_step()) {
    idx[2 * j] = a[j];
    idx[2 * j + 1] = b[j];
    if (coeff) {
      coeff[2 * j] = ca;
      coeff[2 * j + 1] = cb;
    }
  }
}

__global__ __launch_bounds__(256) void mask_lut_index_kernel(uint32_t* __restrict__ lut_eff,
                                                             const uint32_t* __restrict__ in_index,
                                                             const uint32_t* __restrict__ lut_index, uint64_t n_in,
                                                             uint64_t count) {
  for (uint64_t j = gs_start(); j < count; j += gs_step())
    lut_eff[j] = in_index[j] < n_in ? (lut_index ? lut_index[j] : (uint32_t)j) : 0xFFFFFFFFu;
}

}  // namespace lin

hipError_t launch_lwe_linear_combination(uint64_t* out, const uint64_t* in, size_t words, size_t n_in, size_t n_out,
                                         size_t terms, const uint32_t* index, const int64_t* coeff,
                                         const uint64_t* plaintext, hipStream_t s) {
  if (n_out == 0) return hipSuccess;
  const uint64_t chunks = (words + 255) / 256, tiles = (uint64_t)n_out * chunks;
  const unsigned grid = (unsigned)(tiles < lin::MAX_BLOCKS ? tiles : lin::MAX_BLOCKS);
  hipLaunchKernelGGL(lin::linear_combination_kernel, dim3(grid), dim3(256), 0, s, out, in, (uint32_t)words,
                     (uint32_t)chunks, (uint64_t)n_in, (uint64_t)n_out, (uint32_t)terms, index, coeff, plaintext);
  return hipGetLastError();
}

hipError_t launch_index_rule(uint32_t* idx, size_t count, IndexRule rule, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(lin::index_rule_kernel, dim3(lin::blocks_for(count)), dim3(256), 0, s, idx, (uint64_t)count, rule);
  return hipGetLastError();
}

hipError_t launch_lut_rule(uint32_t* idx, size_t count, size_t split, uint32_t lo, size_t block, uint32_t first,
                           uint32_t rest, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(lin::lut_rule_kernel, dim3(lin::blocks_for(count)), dim3(256), 0, s, idx, (uint64_t)count,
                     (uint64_t)split, lo, (uint64_t)block, first, rest);
  return hipGetLastError();
}

hipError_t launch_index_pairs(uint32_t* idx, int64_t* coeff, const uint32_t* a, const uint32_t* b, size_t count,
                              int64_t ca, int64_t cb, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(lin::index_pairs_kernel, dim3(lin::blocks_for(count)), dim3(256), 0, s, idx, coeff, a, b,
                     (uint64_t)count, ca, cb);
  return hipGetLastError();
}

hipError_t launch_mask_lut_index(uint32_t* lut_eff, const uint32_t* in_index, const uint32_t* lut_index, size_t n_in,
                                 size_t count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(lin::mask_lut_index_kernel, dim3(lin::blocks_for(count)), dim3(256), 0, s, lut_eff, in_index,
                     lut_index, (uint64_t)n_in, (uint64_t)count);
  return hipGetLastError();
}

}  // namespace mi
