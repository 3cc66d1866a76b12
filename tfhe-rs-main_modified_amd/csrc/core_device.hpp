// core_device.hpp — the device-side companions of core_scalar.hpp's rules: what needs LDS and barriers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "core_scalar.hpp"

namespace mi {
namespace core {

// algorithms/modulus_switch.rs:60-104 centered_binary_ms_body_correction_to_add, reduced over the TG threads of
// one ciphertext (gt = index within them; sh = 2 TG u64 of that ciphertext's LDS, free again on return).  Every
// thread of the workgroup calls it (barriers).
template <int TG>
__device__ uint64_t centered_body_correction(const uint64_t* __restrict__ lwe, uint32_t n_lwe, unsigned log_mod, int gt,
                                             uint64_t* sh) {
  // (the text the f64 engine had: with CenteredSums in its place pbs_kernel_k1l1 compiled to a slower schedule; the sums
  // and the closing formula are CenteredSums' add and correction, restated)
  uint64_t sum_half = 0;
  int64_t sum_hed = 0;
  for (uint32_t i = gt; i < n_lwe; i += TG) {
    const uint64_t a = lwe[i];
    const int64_t err = (int64_t)((modulus_switch(a, log_mod) << (64u - log_mod)) - a);
    const int64_t half = err / 2;
    sum_half += (uint64_t)half;
    sum_hed += 2 * half - err;
  }
  sh[gt] = sum_half;
  sh[TG + gt] = (uint64_t)sum_hed;
  __syncthreads();
  // TG = 64 (k + 1) is no power of two at k = 2 (192 -> ... -> 3 -> 2 -> 1): the upper part of the `live` entries
  // folds onto the lower one, and an odd count keeps its middle entry for the next round
  for (int live = TG; live > 1;) {
    const int s = (live + 1) / 2;
    if (gt + s < live) {
      sh[gt] += sh[gt + s];
      sh[TG + gt] = (uint64_t)((int64_t)sh[TG + gt] + (int64_t)sh[TG + gt + s]);
    }
    __syncthreads();
    live = s;
  }
  const uint64_t total_half = sh[0];
  const int64_t total_hed = (int64_t)sh[TG];
  __syncthreads();
  const uint64_t sum_halving = (uint64_t)(total_hed / 2);
  const uint64_t half_case = 1ull << (64u - log_mod - 1u);
  return total_half - sum_halving - half_case;
}

}  // namespace core
}  // namespace mi
