// pbs128_device.hpp — what the two 128-bit bootstraps share (pbs128.hip: the classic one; pbs128_multi_bit.hip: the
// multi-bit one): the kernel-side shape, the u128 accesses, the digits of a u128 as residues, the sums of the mac, the routing of
// the plan's transform, the chunk plan, and the launchers of pbs128.hip's passes that the multi-bit step reuses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "mi_arith.hpp"
#include "ntt64_launch.hpp"
#include "pbs_device.hpp"
#include "pbs_passes.hpp"

namespace mi {
namespace pbs128 {

using pbs::Monomial;
using pbs::P;
typedef unsigned __int128 u128;
typedef __int128 i128;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

struct Shape {
  uint32_t logn, n, k, level, limb_bits, n_limbs;
  int base_log;
};

// u128 values are two little-endian u64 words (lo, hi), 16-byte aligned: element i at p + 2 i
__device__ __forceinline__ u128 ld128(const u64* p, uint64_t i) {
  const u64x2 v = *reinterpret_cast<const u64x2*>(p + 2 * i);
  return (u128)v.x | ((u128)v.y << 64);
}
__device__ __forceinline__ void st128(u64* p, uint64_t i, u128 v) {
  const u64x2 w = {(u64)v, (u64)(v >> 64)};
  *reinterpret_cast<u64x2*>(p + 2 * i) = w;
}

// the `level` digits of x as canonical residues, least significant level first: dst[li * level_stride]
__device__ __forceinline__ void decompose_store(u128 x, u64* __restrict__ dst, uint64_t level_stride, int base_log,
                                                int level) {
  // SignedDecomposer<u128> (what collect_next_term_split_scalar, ggsw.rs:517-567, computes on split words); rep =
  // base_log * level in [1, 127]; a digit lies in [-2^(B-1), 2^(B-1)] and B <= 58 wherever a limb plan exists, so it
  // fits an i64
  u128 state = core::decomp_init<u128>(x, base_log, level);
  for (int li = 0; li < level; ++li) {
    const int64_t d = (int64_t)(u64)core::decomp_next<u128>(base_log, state);
    dst[(uint64_t)li * level_stride] = d < 0 ? P + (u64)d : (u64)d;
  }
}

// the switched value in [0, 2N) of an input word: the u64 paths' modulus_switch (fft_impl/common.rs:10-23), or the word
// itself when the caller switched already (MI_MS_PRE_SWITCHED)
__device__ __forceinline__ uint32_t switched(u64 raw, unsigned log_mod, int pre) {
  return (uint32_t)(pre ? raw : pbs::modulus_switch(raw, log_mod)) & ((1u << log_mod) - 1u);
}

// One sum of the mac: Goldilocks::add of Goldilocks::mul per term, or (WIDE) the terms' 128-bit products summed in
// pbs_device.hpp's Acc128 and reduced once at the end — 9 registers per sum instead of 2, so only where the
// KP1 * NL sums of a thread still fit (the production shape's 18 do).  Both give the canonical residue of the sum.
template <bool WIDE>
struct MacSum;
template <>
struct MacSum<false> {
  u64 v = 0;
  __device__ __forceinline__ void mac(u64 x, u64 w) { v = Goldilocks::add(v, Goldilocks::mul(x, w)); }
  __device__ __forceinline__ u64 value() const { return v; }
};
template <>
struct MacSum<true> {
  pbs::Acc128 a;
  __device__ __forceinline__ void mac(u64 x, u64 w) { a.mac(x, w); }
  __device__ __forceinline__ u64 value() const { return a.value(0); }
};

inline Shape shape_of(const Pbs128Shape& p) {
  return Shape{(uint32_t)p.logn, 1u << p.logn, (uint32_t)p.k, (uint32_t)p.level, (uint32_t)p.limb_bits,
               (uint32_t)p.n_limbs, p.base_log};
}

// the plan's transform over `batch` contiguous polynomials (the routing of mi_ntt64_fwd_batch / mi_ntt64_inv_batch)
inline hipError_t ntt(bool fwd, const Ntt128Route& r, u64* d, size_t batch, hipStream_t s) {
  const size_t n = (size_t)1 << r.logn;
  if (r.twisted) return launch_ntt_tw(fwd, d, batch, n, fwd ? r.twist_f : r.twist_i, s);
  if (r.split) return launch_ntt_split(fwd, r.logn, d, batch, n, fwd ? r.tw : r.itw, r.st, s);
  return launch_ntt(fwd, r.logn, true, MontParams{}, d, batch, n, fwd ? r.tw : r.itw, s);
}

// u64 words of one chunk item: its digits and limb products (+ its accumulator and body correction when `rotation`)
inline size_t item_words(const Shape& sh, bool rotation) {
  const size_t per = (size_t)(sh.k + 1) * sh.n;
  return per * sh.level + per * sh.n_limbs + (rotation ? 2 * per + 1 : 0);
}

// ciphertexts per chunk: chunk_items of the item's scratch.  MI_PBS128_CHUNK, read on every call, lowers the bound (the
// tests force two chunks with it)
inline size_t chunk_size(const Shape& sh, size_t batch, bool rotation) {
  size_t chunk = chunk_items(item_words(sh, rotation) * sizeof(u64), batch);
  if (const char* v = std::getenv("MI_PBS128_CHUNK")) {
    const long long c = std::atoll(v);
    if (c >= 1) chunk = std::min<size_t>(chunk, (size_t)c);
  }
  return chunk;
}

// pbs128.hip's passes over `nb` items, as the multi-bit step issues them:
// digits[b][li (k + 1) + c][N] = the decomposition of glwe itself (glwe_decompose<false>)
hipError_t launch_decompose(u64* digits, const u64* glwe, uint32_t nb, const Shape& sh, hipStream_t s);
// acc[b] = src / X^ms(body of lwe_in[b]), the standard switch (init_acc); src_stride 0: one shared LUT
hipError_t launch_init_acc(u64* acc, const u64* src, uint64_t src_stride, const u64* lwe_in, uint32_t n_lwe,
                           uint32_t nb, const Shape& sh, hipStream_t s);
// out = sum_j centered(y_j) 2^(w j) mod 2^128: the recombination into a destination that starts from zero
hipError_t launch_recombine_assign(u64* out, const u64* y, uint32_t nb, const Shape& sh, hipStream_t s);
// sample extraction at degree 0 (extract)
hipError_t launch_extract(u64* lwe_out, const u64* acc, uint32_t nb, const Shape& sh, hipStream_t s);

}  // namespace pbs128
}  // namespace mi
