// ks128_decomp.hpp — the signed-byte recodings of the 128-bit packing keyswitch (packing_keyswitch128.hip; its digits
// are core_scalar.hpp's pre-rounded decomp_init / decomp_next at u128, read as int64_t: base_log <= 63, so |digit| <=
// 2^62), callable from host code so that tests/cpp/ks128_decomp_check.cpp can check both on the rounding corners
// without a GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ks_decomp.hpp"

namespace mi {
namespace ks128 {

typedef unsigned __int128 u128;
typedef __int128 i128;

// bytes per digit: d = sum_{s < nd} e_s 2^(8s), e_s in [-128, 127] (|d| <= 2^(base_log - 1) needs base_log + 1 bits)
__host__ __device__ __forceinline__ int digit_bytes(int base_log) { return (base_log + 1 + 7) / 8; }

// signed byte s of a digit (s < digit_bytes <= 8): the 64-bit recoding of ks_decomp.hpp
__host__ __device__ __forceinline__ int8_t digit_byte(int64_t d, int s) { return ks::signed_byte((uint64_t)d, s); }

// the 16 signed bytes of a key word: x = sum_t out[t] 2^(8t) mod 2^128, out[t] in [-128, 127]
__host__ __device__ __forceinline__ void signed_bytes16(u128 x, int8_t (&out)[16]) {
  unsigned carry = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const unsigned v = (unsigned)((uint64_t)(x >> (8 * t)) & 255u) + carry;
    carry = v >= 128u;
    out[t] = (int8_t)((int)v - (carry ? 256 : 0));
  }
}

}  // namespace ks128
}  // namespace mi
