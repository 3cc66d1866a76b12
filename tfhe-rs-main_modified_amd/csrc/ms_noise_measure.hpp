// ms_noise_measure.hpp — the one copy of the drift technique's arithmetic (core_crypto/algorithms/
// modulus_switch_noise_reduction.rs:14-86), shared by every entry of ms_noise_reduction.hip and by host code.
//
// The reference sums the rounding errors of the mask sequentially in f64 with a separate multiply and add, so this
// header is written with plain `*` and `+` only and its translation units are compiled with -ffp-contract=off: the
// compiler fuses `q += e * e` (and the __dadd_rn(__dmul_rn()) spelling too) into one FMA otherwise, which changes the
// sum of squares and with it the chosen candidate.  No intrinsic, no fma() in here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {
namespace msn {

// the three doubles of a ModulusSwitchNoiseReductionKey as the measure uses them; modular_variance is
// Variance::get_modular_variance at the native modulus: variance * 2^64 * 2^64 in that order (dispersion.rs:258-262)
struct Params {
  double bound, r_sigma, modular_variance;
};

// the two running sums of measure_modulus_switch_noise_expectancy_variance_for_binary_key (:49-57)
struct Sums {
  double s = 0.0, q = 0.0;
};

// round_error_float (:14-36): round(x) - x as a signed value, converted with one rounding (Rust's `as f64`).
// log_modulus in [1, 64]; the rounding is the identity at 64 (fft_impl/common.rs:15-17), which is drop = 0 and
// half = 0 here: no branch on the word's path, so the loops that call this keep their loads together
__host__ __device__ inline double round_error_float(uint64_t x, uint32_t log_modulus) {
  const uint32_t drop = 64u - log_modulus;  // the low bits the switch drops, 0 .. 63
  const uint64_t half = drop ? (uint64_t)1 << (drop - 1u) : 0;
  const uint64_t rounded = ((x + half) >> drop) << drop;
  return (double)(int64_t)(rounded - x);
}

// one mask word (:52-57)
__host__ __device__ inline void add_mask_word(Sums& a, uint64_t x, uint32_t log_modulus) {
  const double error = round_error_float(x, log_modulus);
  a.s = a.s + error;
  a.q = a.q + error * error;
}

// the body term and the final formula (:59-85)
__host__ __device__ inline double finish_measure(const Sums& a, uint64_t body, uint32_t log_modulus, const Params& p) {
  const double body_error = round_error_float(body, log_modulus);
  const double expectancy = body_error - a.s / 2.0;
  const double variance = a.q / 4.0;
  const double std_dev = __builtin_sqrt(variance + p.modular_variance);
  return __builtin_fabs(expectancy) + std_dev * p.r_sigma;
}

}  // namespace msn
}  // namespace mi
