// ks_decomp.hpp — the signed decomposition digits and the signed-byte recoding of the keyswitches (keyswitch.hip),
// callable from host code so that tests/cpp/ks_decomp_check.cpp can check them on the rounding corners without a GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {
namespace ks {

// decomposer.rs:64-71 + :156-185 init_decomposer_state (native u64, closest representable).  pre_rounded: the
// packing keyswitch decomposes closest_representable(input) (lwe_packing_keyswitch.rs:173-174), whose rounding bit
// is 0, so the tie state 2^(rep-1) is balanced only when the bit below it is set; the state is otherwise the same.
__host__ __device__ __forceinline__ uint64_t decomp_init(uint64_t input, int base_log, int level,
                                                         bool pre_rounded = false) {
  const unsigned rep = (unsigned)(base_log * level), non_rep = 64u - rep;
  uint64_t res = input >> (non_rep - 1);
  const uint64_t rounding_bit = pre_rounded ? 0u : res & 1u;
  res += 1;
  res >>= 1;
  res &= (~0ull) >> (64u - rep);
  const uint64_t need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
  return res - (need_balance << rep);
}

// iter.rs:131-151 decompose_one_level (arithmetic shift); the digit as a signed integer.  |digit| <= 2^(B-1) with
// base_log up to 63 at one level, so it needs all 64 bits: an int drops +2^31 at B = 32 and everything at B >= 33.
__host__ __device__ __forceinline__ int64_t decompose_one(int base_log, uint64_t& state) {
  const uint64_t mask = (1ull << base_log) - 1;
  const uint64_t res = state & mask;
  state = (uint64_t)((int64_t)state >> base_log);
  const uint64_t carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return (int64_t)(res - (carry << base_log));
}

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
