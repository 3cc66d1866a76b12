// ks_device.hpp — device helpers shared by keyswitch.hip and packing_keyswitch.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {
namespace ks {

// modulus_switch (fft_impl/common.rs:10-23) at Scalar = T: identity at log_mod == BITS
template <typename T>
__device__ __forceinline__ T ms_word(T x, uint32_t log_mod) {
  constexpr uint32_t BITS = 8 * sizeof(T);
  return log_mod >= BITS ? x : (T)(x + ((T)1 << (BITS - log_mod - 1u))) >> (BITS - log_mod);
}

}  // namespace ks
}  // namespace mi
