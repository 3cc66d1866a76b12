// shortint_internal.hpp — what the source files of the shortint / integer layer share (c_api_shortint.cpp,
// c_api_radix_mul.cpp): the key behind mi_shortint_key, the order of its lookup tables, the argument checks of the
// radix calls and the stages the radix composites are written in (RadixStages).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "c_api_internal.hpp"
#include "carve.hpp"
#include "lwe_linear_algebra_launch.hpp"

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

inline int check_radix(const mi_shortint_key* key, const void* radix, size_t n_blocks, size_t n_integers) {
  if (!key) return capi::fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (n_blocks == 0) return capi::fail(MI_ERR_INVALID_ARG, "n_blocks is 0");
  if (n_blocks > MAX_ITEMS || (n_integers && n_blocks > MAX_ITEMS / 2 / n_integers))
    return capi::fail(MI_ERR_INVALID_ARG, "batch too large");
  if (n_integers && !radix) return capi::fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  return MI_OK;
}

// The stages the radix composites are written in (LC, APPLY as in c_api_shortint.cpp): each writes its index arrays on
// the device by rule into the carved arrays of ix (StageIndex, carve.hpp), then makes the one public call.  The
// contract of every stage: no more entries than the composite carved (count, items, coefficients: see StageIndex).
struct RadixStages {
  const mi_shortint_key* key;
  hipStream_t s;
  StageIndex ix;
  // LC  out[j] = in[a(j)], one term; the rule is always written to ia
  int gather(uint64_t* out, const uint64_t* in, size_t n_in, size_t count, IndexRule a) const {
    MI_TRY_HIP(launch_index_rule(ix.ia, count, a, s), "radix index launch");
    return mi_lwe_linear_combination_batch(out, in, key->big, n_in, count, 1, ix.ia, nullptr, nullptr, key->device, s);
  }
  // LC  out[j] = ca * in[a(j)] + cb * in[b(j)]; unit coefficients are passed as NULL
  int combine2(uint64_t* out, const uint64_t* in, size_t n_in, size_t count, IndexRule a, IndexRule b, int64_t ca = 1,
               int64_t cb = 1) const {
    int64_t* cf = ca == 1 && cb == 1 ? nullptr : ix.coeff;
    MI_TRY_HIP(launch_index_rule(ix.ia, count, a, s), "radix index launch");
    MI_TRY_HIP(launch_index_rule(ix.ib, count, b, s), "radix index launch");
    MI_TRY_HIP(launch_index_pairs(ix.pairs, cf, ix.ia, ix.ib, count, ca, cb, s), "radix index launch");
    return mi_lwe_linear_combination_batch(out, in, key->big, n_in, count, 2, ix.pairs, cf, nullptr, key->device, s);
  }
  // APPLY  out[items] <- in[n_in] through the key's tables, item j reading input in_rule(j), or j without a rule; its
  // table as launch_lut_rule takes it: lo below `split`, then `first` at the start of each `block` items, else `rest`
  int apply(uint64_t* out, const uint64_t* in, size_t n_in, size_t items, const IndexRule* in_rule, size_t split,
            uint32_t lo, size_t block, uint32_t first, uint32_t rest) const {
    if (in_rule) MI_TRY_HIP(launch_index_rule(ix.in_idx, items, *in_rule, s), "radix index launch");
    MI_TRY_HIP(launch_lut_rule(ix.lut_idx, items, split, lo, block, first, rest, s), "radix index launch");
    return mi_shortint_apply_lut_batch(key, out, in, n_in, in_rule ? ix.in_idx : nullptr, key->d_luts, ix.lut_idx,
                                       N_KEY_LUTS, items, s);
  }
};

// The fourth stage needs no index array: dst = lhs | rhs, `bytes` each, two device-to-device copies into one input list
inline int stage_pair(uint64_t* dst, const uint64_t* lhs, const uint64_t* rhs, size_t bytes, const char* what,
                      hipStream_t s) {
  MI_TRY_HIP(hipMemcpyAsync(dst, lhs, bytes, hipMemcpyDeviceToDevice, s), what);
  return capi::hip_status(hipMemcpyAsync(dst + bytes / sizeof(uint64_t), rhs, bytes, hipMemcpyDeviceToDevice, s), what);
}

}  // namespace shortint
}  // namespace mi
