// ks128_decomp.hpp — the pre-rounded signed decomposition of a u128 and the signed-byte recodings of the 128-bit
// packing keyswitch (packing_keyswitch128.hip), callable from host code so that tests/cpp/ks128_decomp_check.cpp can
// check them on the rounding corners without a GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ks_decomp.hpp"

namespace mi {
namespace ks128 {

typedef unsigned __int128 u128;
typedef __int128 i128;

// SignedDecomposer::<u128>::init_decomposer_state (decomposer.rs:156-185) of closest_representable(input)
// (decomposer.rs:25-49), which is what the packing keyswitch decomposes (lwe_packing_keyswitch.rs:173-174).  The
// rounded word has the same kept bits as the input's own rounding and a rounding bit of 0, so the tie state 2^(rep-1)
// is balanced only when the bit below it is set (ks_decomp.hpp's pre_rounded rule at 128 bits).  1 <= rep <= 127.
__host__ __device__ __forceinline__ u128 decomp_init_pre_rounded(u128 input, int base_log, int level) {
  const unsigned rep = (unsigned)(base_log * level), non_rep = 128u - rep;
  u128 res = input >> (non_rep - 1);
  res += 1;
  res >>= 1;
  res &= (~(u128)0) >> (128u - rep);
  const u128 need_balance = ((res - 1) & res) >> (rep - 1);
  return res - (need_balance << rep);
}

// iter.rs:131-151 decompose_one_level on a u128 state (arithmetic shift).  base_log <= 63, so |digit| <= 2^62 fits an
// int64.
__host__ __device__ __forceinline__ int64_t decompose_one(int base_log, u128& state) {
  const u128 mask = ((u128)1 << base_log) - 1;
  const u128 res = state & mask;
  state = (u128)((i128)state >> base_log);
  const u128 carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return (int64_t)(i128)(res - (carry << base_log));
}

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
