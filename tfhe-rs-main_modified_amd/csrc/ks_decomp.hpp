// ks_decomp.hpp — the signed-byte recoding of the keyswitches' digits (keyswitch.hip; the digits themselves are
// core_scalar.hpp's decomp_init / decomp_next, read as int64_t), callable from host code so that
// tests/cpp/ks_decomp_check.cpp can check both on the rounding corners without a GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "core_scalar.hpp"

namespace mi {
namespace ks {

// signed byte t of x: x = sum_t s_t 2^(8t) mod 2^64, s_t in [-128, 127]
__host__ __device__ __forceinline__ int8_t signed_byte(uint64_t x, int t) {
  unsigned carry = 0;
  int s = 0;
  for (int u = 0; u <= t; ++u) {
    const unsigned v = (unsigned)((x >> (8 * u)) & 255u) + carry;
    carry = v >= 128u;
    s = (int)v - (carry ? 256 : 0);
  }
  return (int8_t)s;
}

}  // namespace ks
}  // namespace mi
