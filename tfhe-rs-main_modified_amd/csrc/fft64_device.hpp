// fft64_device.hpp — device helpers shared by the f64-FFT engines: the N = 2048 one-wave engine (fft64_pbs.hip) and
// the shape-generic engine (fft64_generic.hip).  Complex f64 arithmetic (FMA-contracted as the reference's pulp
// kernels' mul_add) and the torus conversions of fft_impl/fft64/math/fft/mod.rs; the native decomposition, the modulus
// switch and the monomial rules of the blind rotation are core_scalar.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "core_device.hpp"

namespace mi {
namespace fft {

using u64 = uint64_t;

struct __align__(16) cplx {
  double re, im;
};

__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
  return {__fma_rn(a.re, b.re, -a.im * b.im), __fma_rn(a.re, b.im, a.im * b.re)};
}
// a * conj(b)
__device__ __forceinline__ cplx cmulc(cplx a, cplx b) {
  return {__fma_rn(a.re, b.re, a.im * b.im), __fma_rn(a.im, b.re, -a.re * b.im)};
}
// acc + a * b
__device__ __forceinline__ cplx cfma(cplx a, cplx b, cplx acc) {
  return {__fma_rn(a.re, b.re, __fma_rn(-a.im, b.im, acc.re)), __fma_rn(a.re, b.im, __fma_rn(a.im, b.re, acc.im))};
}
__device__ __forceinline__ cplx mul_neg_i(cplx a) { return {a.im, -a.re}; }  // -i a
__device__ __forceinline__ cplx mul_pos_i(cplx a) { return {-a.im, a.re}; }  // +i a

// ---- conversions (fft_impl/fft64/math/fft/mod.rs) -------------------------------------------------
// The contract of the three conversions below is pinned bit for bit, on every engine, by tests/torus_corners.py
// (the classes in numbers, host models of these functions) and tests/test_torus_corners_gpu.py.
//
// u64 -> i64 -> f64 (into_signed().cast_into()): the correctly rounded (nearest, ties to even) double of the signed
// word, as Rust's `as f64`; exact below 2^53 in magnitude
__device__ __forceinline__ double s64_to_f64(u64 x) { return (double)(int64_t)x; }

// Scalar::from_torus (commons/math/torus/mod.rs:72-78) of x = y / 2^64, taking y = x 2^64 (an exact power-of-two
// scaling by the caller): round(fract(x) 2^64) mod 2^64 = round(y) mod 2^64.  All steps
// exact: r = rint(y); z = r - rint(r 2^-64) 2^64 in [-2^63, 2^63]; z = hi 2^32 + lo with lo in [0, 2^32); the
// words are read from the mantissas of hi + 1.5 2^52 and lo + 2^52.  The result is round-half-even(y) mod 2^64: the
// reference's word except in two classes.  (1) y an exact half-integer (|x| < 2^-11): the nearest even word where the
// reference rounds half away from zero, one unit apart when floor(y) is even.  (2) the reference's fract = +1/2
// (x = -(n + 1/2)): 2^63 where the reference saturates to i64::MAX = 2^63 - 1.
__device__ __forceinline__ void torus_words(double y, uint32_t& h, uint32_t& l) {
  const double r = __builtin_rint(y);
  const double z = __fma_rn(-__builtin_rint(r * 0x1p-64), 0x1p64, r);
  const double hi = __builtin_floor(z * 0x1p-32);
  const double lo = __fma_rn(-hi, 0x1p32, z);
  h = (uint32_t)__double_as_longlong(hi + 0x1.8p52);
  l = (uint32_t)__double_as_longlong(lo + 0x1p52);
}
__device__ __forceinline__ u64 from_torus_scaled(double y) {
  uint32_t h, l;
  torus_words(y, h, l);
  return ((u64)h << 32) | l;
}
// acc += from_torus(t) (t in torus units) as one 32-bit add with carry per word: f = fract(t) = t - floor(t) in
// [0, 1); s = f 2^32 exact; the high word is trunc(s), the low word fract(s) 2^32 rounded (nearest, ties to even)
// through the mantissa of fract(s) 2^32 + 2^52.  The added word, against the exact from_torus(t):
//   * equal for t >= 2^-12, for 0 <= t < 2^-12 with t 2^64 an integer, for t <= -1/2, and for -1/2 < t < 0 with t a
//     multiple of 2^-53 (f is then exact: t's bits below 2^0) -- but t = -(n + 1/2) adds 2^63 where the reference
//     saturates to 2^63 - 1;
//   * 0 < t < 2^-12 with bits below 2^-64: the low word rounds half-even where the reference rounds half away (one
//     unit apart on an exact half with an even floor, equal otherwise), and where t 2^64 mod 2^32 >= 2^32 - 1/2 the
//     low word rounds up to 2^32, reads as 0 and its carry is dropped: exactly 2^32 below the reference;
//   * -1/2 < t < 0 otherwise: f = 1 + t is NOT exact, it needs one bit more than a double of [1/2, 1) has and is
//     rounded to a multiple of 2^-53 (-0.3 -> 0.7 rounded), so the word is off by up to 2^10; for -2^-54 <= t < 0 it
//     rounds to 1 and the instruction clamps it to 1 - 2^-53: the word 2^64 - 2^11, up to 2^11 from the reference.
// All far below the external product's own f64 error (2^24 and up: DESIGN.md §4, measured accuracy of the f64 path).
__device__ __forceinline__ void add_torus(u64& acc, double t) {
  const double f = __builtin_amdgcn_fract(t);
  const double s = f * 0x1p32;
  const uint32_t h = (uint32_t)s;
  const uint32_t l = (uint32_t)__double_as_longlong(__fma_rn(__builtin_amdgcn_fract(s), 0x1p32, 0x1p52));
  const uint32_t alo = (uint32_t)acc, ahi = (uint32_t)(acc >> 32);
  const uint32_t nlo = alo + l;
  const uint32_t nhi = ahi + h + (nlo < alo ? 1u : 0u);
  acc = ((u64)nhi << 32) | nlo;
}

// ---- the native decomposition, the modulus switch and the centered correction: core_scalar.hpp's ----
using core::decomp_init;
using core::decomp_next;
__device__ __forceinline__ u64 decomp_init_native(u64 x, int base_log, int level) {
  return core::decomp_init<u64>(x, base_log, level);
}
__device__ __forceinline__ u64 decompose_one_level(int base_log, u64& state) {
  return core::decomp_next<u64>(base_log, state);
}
using core::centered_body_correction;
using core::Monomial;
using core::modulus_switch;

}  // namespace fft
}  // namespace mi
