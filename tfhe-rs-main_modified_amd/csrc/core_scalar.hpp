// core_scalar.hpp — the one definition of each scalar rule of the reference that more than one engine runs: the signed
// decomposition, the NTT paths' digit stream, the modulus switches, the arithmetic modulo the Goldilocks prime, the
// partial sums of the centered modulus switch, and the index rules of the monomial rotations and of the sample
// extraction.  Everything is __host__ __device__ with no device-only construct, so a host program can include this
// header alone: tests/cpp/{ks_decomp,ks128_decomp,fft_decomp,ntt_digits}_check.cpp check on the host the very text the
// kernels compile.  Reference paths relative to tfhe/src/core_crypto.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {
namespace core {

static constexpr uint64_t P = 0xFFFFFFFF00000001ull;  // the Goldilocks prime 2^64 - 2^32 + 1 (mi_arith.hpp's GL_P)
static constexpr uint64_t EPS = 0xFFFFFFFFull;        // 2^64 - P

template <class W>
struct Word;
template <>
struct Word<uint64_t> {
  typedef int64_t S;
  static constexpr unsigned BITS = 64;
};
template <>
struct Word<uint32_t> {
  typedef int32_t S;
  static constexpr unsigned BITS = 32;
};
template <>
struct Word<unsigned __int128> {
  typedef __int128 S;
  static constexpr unsigned BITS = 128;
};

// ---- signed decomposition ----------------------------------------------------------------------------------------
// SignedDecomposer::init_decomposer_state (commons/math/decomposition/decomposer.rs:64-71, :156-185; native modulus,
// closest representable) at Scalar = W; 1 <= rep = base_log * level < BITS.  pre_rounded: the packing keyswitches
// decompose closest_representable(input) (lwe_packing_keyswitch.rs:173-174), whose kept bits are the input's own
// rounding and whose rounding bit is 0, so the tie state 2^(rep-1) is balanced only when the bit below it is set; the
// state is otherwise the same.
template <class W>
__host__ __device__ __forceinline__ W decomp_init(W input, int base_log, int level, bool pre_rounded = false) {
  constexpr unsigned BITS = Word<W>::BITS;
  const unsigned rep = (unsigned)(base_log * level), non_rep = BITS - rep;
  W res = input >> (non_rep - 1);
  const W rounding_bit = pre_rounded ? (W)0 : res & 1u;
  res += 1;
  res >>= 1;
  res &= (~(W)0) >> (BITS - rep);
  const W need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
  return res - (need_balance << rep);
}

// decompose_one_level (iter.rs:131-151; arithmetic shift): the next digit, least significant level first, as a two's
// complement word.  |digit| <= 2^(base_log - 1) with base_log up to 63, so a signed reading needs 64 bits.
template <class W>
__host__ __device__ __forceinline__ W decomp_next(int base_log, W& state) {
  typedef typename Word<W>::S S;
  const W mask = ((W)1 << base_log) - 1;
  const W res = state & mask;
  state = (W)((S)state >> base_log);
  const W carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return res - (carry << base_log);
}

// decomposer.rs:25-49 native_closest_representable, then decomposer.rs:521-548 (q = p, 64 bits)
__host__ __device__ __forceinline__ uint64_t closest_abs_nonnative(uint64_t abs_value, int base_log, int level) {
  const unsigned shift = 64u - (unsigned)(level * base_log) - 1u;
  uint64_t res = abs_value >> shift;
  res += 1;
  res &= ~1ull;
  return res << shift;
}

// The digit stream of the NTT paths: decomposer.rs:156-185 + iter.rs:131-151 on the native word (BNF) or the
// sign-magnitude form modulo p (Solinas, iter.rs:623-745), each digit mapped into [0, p) (ntt64.rs:231-238 /
// iter.rs:722-731).
template <bool BNF>
struct NttDigits {
  uint64_t state;
  bool sign;
  __host__ __device__ __forceinline__ void init(uint64_t x, int base_log, int level) {
    if (BNF) {
      state = decomp_init<uint64_t>(x, base_log, level);
      sign = false;
    } else {
      const unsigned shift = 64u - (unsigned)(base_log * level);
      sign = x >= P / 2 + 1;  // div_ceil(2)
      state = closest_abs_nonnative(sign ? P - x : x, base_log, level) >> shift;
    }
  }
  __host__ __device__ __forceinline__ uint64_t next(int base_log) {
    uint64_t term = decomp_next<uint64_t>(base_log, state);
    if (!BNF && sign) term = (uint64_t)0 - term;
    return ((int64_t)term < 0) ? term + P : term;
  }
};

// ---- modulus switches --------------------------------------------------------------------------------------------
// fft_impl/common.rs:10-23
__host__ __device__ __forceinline__ uint64_t modulus_switch(uint64_t input, unsigned log_modulus) {
  return (input + (1ull << (64u - log_modulus - 1u))) >> (64u - log_modulus);
}

// ntt64_pbs.rs:540-549 pbs_modulus_switch_non_native + algorithms/misc.rs:6-18 divide_round(input 2^log_mod, p).  The
// result may be 2^log_mod itself: X^(2N) = 1, so a caller that wants a value in [0, 2N) masks it.
__host__ __device__ __forceinline__ uint64_t ms_non_native(uint64_t input, unsigned log_mod) {
  const unsigned __int128 num = ((unsigned __int128)input) << log_mod;
  // num / p with the 2^64 = p + EPS split (num < 2^(64 + log_mod))
  const uint64_t nh = (uint64_t)(num >> 64), nl = (uint64_t)num;
  unsigned __int128 r = (unsigned __int128)nh * EPS + nl;  // num = nh*p + r
  uint64_t q = nh;
  while (r >= P) { r -= P; ++q; }
  return q + (r >= (P >> 1) ? 1 : 0);
}

// ---- arithmetic modulo p on canonical residues (ntt64.rs:110-137 / 244-266) ---------------------------------------
__host__ __device__ __forceinline__ uint64_t neg_custom(uint64_t a) { return a == 0 ? 0 : P - a; }
__host__ __device__ __forceinline__ uint64_t sub_custom(uint64_t a, uint64_t b) { return a >= b ? a - b : a - b + P; }
__host__ __device__ __forceinline__ uint64_t add_custom(uint64_t a, uint64_t b) { return sub_custom(a, neg_custom(b)); }

// negation modulo the ciphertext modulus: 2^64 (BNF) or p
template <bool BNF>
__host__ __device__ __forceinline__ uint64_t neg_q(uint64_t a) { return BNF ? (uint64_t)0 - a : neg_custom(a); }

// ---- centered modulus switch ---------------------------------------------------------------------------------------
// centered_binary_ms_body_correction_to_add (algorithms/modulus_switch.rs:60-104) at Scalar = T, split where a
// parallel reduction cuts it: the wrapping sum of the halved rounding errors and the exact sum of the halving errors
// (each in {-1, 0, 1}) are order-free, so partial sums merge in any order.  H holds the second sum: the word's signed
// type, or a narrower one where the caller bounds the element count.
template <class T, class H = typename Word<T>::S>
struct CenteredSums {
  typedef typename Word<T>::S S;
  static constexpr unsigned BITS = Word<T>::BITS;
  T half = 0;
  H hed = 0;
  // one mask element; log_mod = BITS: the switch is the identity and the error 0
  __host__ __device__ __forceinline__ void add(T a, unsigned log_mod) {
    const unsigned drop = BITS - log_mod;
    const T round = log_mod >= BITS ? a : (T)((T)((T)(a + ((T)1 << (drop - 1u))) >> drop) << drop);
    const S err = (S)(T)(round - a), h = err / 2;  // signed division truncates toward zero, as Rust's
    half += (T)h;
    hed += (H)(2 * h - err);
  }
  __host__ __device__ __forceinline__ void merge(const CenteredSums& o) {
    half += o.half;
    hed += o.hed;
  }
  // total_half - total_hed / 2 - half_case; log_mod < BITS (the reference's half_case shift underflows at BITS)
  __host__ __device__ __forceinline__ T correction(unsigned log_mod) const {
    const T half_case = (T)1 << (BITS - log_mod - 1u);
    return (T)(half - (T)(hed / 2)) - half_case;
  }
};

// ---- monomial rotations and sample extraction ------------------------------------------------------------------------
// X^a with a in [0, 2N): a = full N + rem, X^N = -1.  Division (polynomial_wrapping_monic_monomial_div_assign):
// new[m] = old[(m + rem) % N], negated for m >= N - rem; multiplication (.._mul_assign): new[e] = old[(e - rem) % N],
// negated for e < rem; both negated once more when full.  Sample extraction at nth = 0
// (glwe_sample_extraction.rs:89-160): out[0] = A[0], out[j] = -A[N - j].  n = N, a power of two, known at compile
// time or not.
struct Monomial {
  uint32_t full = 0, rem = 0;
  Monomial() = default;
  // switched: a modulus-switched value; its bits from log2(2N) up are ignored
  __host__ __device__ __forceinline__ Monomial(uint64_t switched, unsigned logn)
      : full((uint32_t)(switched >> logn) & 1u), rem((uint32_t)switched & ((1u << logn) - 1u)) {}
  // I: the caller's index type (int or uint32_t), so that its compares stay what they were
  template <class I>
  __host__ __device__ __forceinline__ I div_src(I m, I n) const { return (m + (I)rem) & (n - 1); }
  template <class I>
  __host__ __device__ __forceinline__ bool div_neg(I m, I n) const { return full ^ (uint32_t)(m >= n - (I)rem); }
  template <class I>
  __host__ __device__ __forceinline__ I mul_src(I e, I n) const { return (e - (I)rem) & (n - 1); }
  template <class I>
  __host__ __device__ __forceinline__ bool mul_neg(I e) const { return full ^ (uint32_t)(e < (I)rem); }
  template <class I>
  __host__ __device__ static __forceinline__ I extract_src(I j, I n) { return j == 0 ? 0 : n - j; }
  template <class I>
  __host__ __device__ static __forceinline__ bool extract_neg(I j) { return j != 0; }
};

}  // namespace core
}  // namespace mi
