// shortint_internal.hpp — what the source files of the shortint / integer layer share (c_api_shortint.cpp,
// c_api_radix_mul.cpp): the key behind mi_shortint_key, the order of its lookup tables and the argument checks of the
// radix calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "c_api_internal.hpp"

// The key's lookup tables, in the order of d_luts.  MSG x mod m, CARRY x / m, STATE0 x >= m, STATE (x >= m) + 2 (x ==
// m - 1), SCAN (cur, prev) -> cur == 2 ? prev : cur; MUL_LSB (x, y) -> (x y) mod m and MUL_MSB (x, y) -> (x y) / m on
// the packed operand m x + y (integer/server_key/radix_parallel/mul.rs:339-345).
enum { LUT_MSG = 0, LUT_CARRY = 1, LUT_STATE0 = 2, LUT_STATE = 3, LUT_SCAN = 4, LUT_MUL_LSB = 5, LUT_MUL_MSB = 6,
       N_KEY_LUTS = 7 };

struct mi_shortint_key {
  const mi_lwe_ksk* ksk = nullptr;
  int engine = 0;
  const void* pbs = nullptr;
  const mi_ms_noise_key* ms_noise = nullptr;
  int ms_mode = 0;
  uint64_t m = 0, c = 0;
  size_t big = 0, small_ = 0, n = 0;  // k N, the small LWE dimension, N
  int k = 1, device = 0;
  uint64_t* d_luts = nullptr;  // N_KEY_LUTS GLWEs of the radix drivers
};

namespace mi {
namespace shortint {

constexpr size_t MAX_ITEMS = 0x3FFFFFull;

inline int hip_status(hipError_t e, const char* what) { return e == hipSuccess ? MI_OK : capi::hip_fail(e, what); }

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

inline int check_radix(const mi_shortint_key* key, const void* radix, size_t n_blocks, size_t n_integers) {
  if (!key) return capi::fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (n_blocks == 0) return capi::fail(MI_ERR_INVALID_ARG, "n_blocks is 0");
  if (n_blocks > MAX_ITEMS || (n_integers && n_blocks > MAX_ITEMS / 2 / n_integers))
    return capi::fail(MI_ERR_INVALID_ARG, "batch too large");
  if (n_integers && !radix) return capi::fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  return MI_OK;
}

}  // namespace shortint
}  // namespace mi
