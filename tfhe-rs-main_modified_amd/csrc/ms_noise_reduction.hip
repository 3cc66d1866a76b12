// ms_noise_reduction.hip — the drift-technique modulus switch noise reduction of the classic *_KS_PBS_TUNIFORM_2M128
// parameter sets (core_crypto/algorithms/modulus_switch_noise_reduction.rs, https://eprint.iacr.org/2024/1718):
//   measure_modulus_switch_noise_estimation_for_binary_key              :71-86
//   choose_candidate_to_improve_modulus_switch_noise_for_binary_key     :99-195
//   improve_lwe_ciphertext_modulus_switch_noise_for_binary_key          :202-242
//   ModulusSwitchNoiseReductionKey::improve_noise_and_modulus_switch    shortint/server_key/
//                                                                       modulus_switch_noise_reduction.rs
//
// One wave per input LWE, one lane per candidate of the current tile of 64 encryptions of zero.  The reference's two
// f64 sums run sequentially over the mask, and so does every lane here: the measures, and with them the chosen
// candidate, are the reference's bit for bit (no tree reduction of the sums anywhere).  Each step of the loop reads one
// wave-uniform input word and one 512-byte row of the prepared key.
//
// This file is compiled with -ffp-contract=off (see ms_noise_measure.hpp and the Makefile).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ks_device.hpp"
#include "ms_noise_launch.hpp"

namespace mi {
namespace msn {

using u64 = uint64_t;

// zeros (zeros_count rows of size words) -> tile[c / 64][j][c % 64]; the padding lanes of the last tile get 0
__global__ __launch_bounds__(256) void prepare_kernel(u64* __restrict__ tiles, const u64* __restrict__ zeros, u64 size,
                                                      u64 zeros_count, u64 total) {
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
    const u64 row = i >> 6, c = row / size * 64 + (i & 63);
    tiles[i] = c < zeros_count ? zeros[c * size + row % size] : 0;
  }
}

// The measure of x (ADD = false) or of x + this lane's candidate (col: the lane's column of one tile).  x is
// wave-uniform; the loop is the reference's, in its order.
template <bool ADD>
__device__ __forceinline__ double lane_measure(const u64* x, const u64* col, uint32_t dim, uint32_t log_mod,
                                               const Params& p) {
  Sums a;
#pragma unroll 8
  for (uint32_t j = 0; j < dim; ++j) add_mask_word(a, ADD ? x[j] + col[(u64)j * 64] : x[j], log_mod);
  return finish_measure(a, ADD ? x[dim] + col[(u64)dim * 64] : x[dim], log_mod, p);
}

// MEASURE: out.measures alone (the base measure, and every candidate's when out.all_candidates).  Otherwise the
// choice, and with out.lwe the addition of the chosen zero (and the standard switch when out.switched).  out.lwe may
// be lwe_in: a wave has read its whole input before the choice is known, and the tail reads and writes word by word.
template <bool MEASURE>
__global__ __launch_bounds__(256) void ms_noise_kernel(MsNoiseOut out, const u64* tiles, uint32_t dim, u64 zeros_count,
                                                       Params p, const u64* lwe_in, u64 batch, uint32_t log_mod) {
  const uint32_t lane = threadIdx.x & 63;
  const u64 item = (u64)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (item >= batch) return;
  const u64 size = (u64)dim + 1, n_tiles = (zeros_count + 63) / 64;
  const u64* x = lwe_in + item * size;
  const double base = lane_measure<false>(x, nullptr, dim, log_mod, p);

  if (MEASURE) {
    double* m = out.measures + item * (out.all_candidates ? 1 + zeros_count : 1);
    if (lane == 0) m[0] = base;
    if (!out.all_candidates) return;
    for (u64 t = 0; t < n_tiles; ++t) {
      const u64 c = t * 64 + lane;
      const double v = lane_measure<true>(x, tiles + t * size * 64 + lane, dim, log_mod, p);
      if (c < zeros_count) m[1 + c] = v;
    }
    return;
  }

  // choose_candidate (:146-194).  A tile's verdict is a ballot of measure <= bound: every earlier measure exceeded the
  // bound, so the lowest voting lane is both the first satisfying candidate and the best so far.  Without a vote each
  // lane keeps its own first minimum (strict <, starting from the base measure, so the unmodified input wins ties).
  int64_t chosen = -1;
  bool satisfied = base <= p.bound;
  if (!satisfied) {
    double best = base;
    int64_t best_idx = -1;
    for (u64 t = 0; t < n_tiles; ++t) {
      const u64 c = t * 64 + lane;
      const bool valid = c < zeros_count;  // the padding lanes never vote and never win
      const double v = lane_measure<true>(x, tiles + t * size * 64 + lane, dim, log_mod, p);
      const u64 votes = __ballot(valid && v <= p.bound);
      if (votes) {
        chosen = (int64_t)(t * 64 + (u64)__builtin_ctzll(votes));
        satisfied = true;
        break;
      }
      if (valid && v < best) {
        best = v;
        best_idx = (int64_t)c;
      }
    }
    if (!satisfied) {
      // the smallest measure and, among equals, the smallest index (-1, the base measure, before every candidate)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double om = __shfl_xor(best, off, 64);
        const int64_t oi = (int64_t)__shfl_xor((long long)best_idx, off, 64);
        if (om < best || (om == best && oi < best_idx)) {
          best = om;
          best_idx = oi;
        }
      }
      chosen = best_idx;
    }
  }
  if (lane == 0) {
    if (out.candidate) out.candidate[item] = chosen;
    if (out.satisfied) out.satisfied[item] = satisfied ? 1 : 0;
  }
  if (!out.lwe) return;
  // lwe_ciphertext_add_assign of the chosen zero (:234-241), then the standard switch of mi_lwe_modulus_switch_batch
  u64* y = out.lwe + item * size;
  const u64* col = chosen >= 0 ? tiles + ((u64)chosen >> 6) * size * 64 + ((u64)chosen & 63) : nullptr;
  for (u64 j = lane; j < size; j += 64) {
    u64 w = x[j];
    if (col) w += col[j * 64];
    y[j] = out.switched ? ks::ms_word<u64>(w, log_mod) : w;
  }
}

}  // namespace msn

hipError_t launch_ms_noise_prepare(uint64_t* tiles, const uint64_t* zeros, const MsNoiseGeometry& g, hipStream_t s) {
  const uint64_t total = (uint64_t)ms_noise_tiles(g) * (g.lwe_dim + 1) * 64;
  const uint64_t blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 65535 * 4 ? blocks : 65535 * 4);
  hipLaunchKernelGGL(msn::prepare_kernel, dim3(grid), dim3(256), 0, s, tiles, zeros, (uint64_t)g.lwe_dim + 1,
                     (uint64_t)g.zeros_count, total);
  return hipGetLastError();
}

hipError_t launch_ms_noise(const MsNoiseOut& out, const uint64_t* tiles, const MsNoiseGeometry& g, const msn::Params& p,
                           const uint64_t* lwe_in, size_t batch, int log_modulus, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  const unsigned grid = (unsigned)((batch + 3) / 4);
  const bool measure = !out.candidate && !out.satisfied && !out.lwe;
  if (measure)
    hipLaunchKernelGGL(msn::ms_noise_kernel<true>, dim3(grid), dim3(256), 0, s, out, tiles, (uint32_t)g.lwe_dim,
                       (uint64_t)g.zeros_count, p, lwe_in, (uint64_t)batch, (uint32_t)log_modulus);
  else
    hipLaunchKernelGGL(msn::ms_noise_kernel<false>, dim3(grid), dim3(256), 0, s, out, tiles, (uint32_t)g.lwe_dim,
                       (uint64_t)g.zeros_count, p, lwe_in, (uint64_t)batch, (uint32_t)log_modulus);
  return hipGetLastError();
}

}  // namespace mi
