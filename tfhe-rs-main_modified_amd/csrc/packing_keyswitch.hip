// packing_keyswitch.hip — LWE packing keyswitch and GLWE modulus-switch compression.
//
// Reference: tfhe/src/core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187
// (keyswitch_lwe_ciphertext_into_glwe_ciphertext) and :296-379
// (keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext); entities/
// compressed_modulus_switched_glwe_ciphertext.rs:169-256 (compress / extract) over entities/packed_integers.rs:39-222.
//
// Over a batch the packing keyswitch of ciphertext d is row d of the same mod-2^64 GEMM keyswitch.hip runs on the
// int8 matrix cores: K = in_dim * level digit columns (of the pre-rounded mask, KsMode::Packing) against (k + 1) N
// key columns, the input body added at column k N (the constant coefficient of the body polynomial).  The GEMM
// writes one row T[d] per ciphertext into scratch; the list form multiplies row d by X^d and sums the rows of a GLWE
// (polynomial_wrapping_monic_monomial_mul_assign + slice_wrapping_add_assign, :369-378):
//   out[g][p][j] = sum_{d < cnt} +- T[g per + d][p N + ((j - d) mod N)], negated when j < d.
//   * pks_rotate_sum_kernel (pks_rotate.hpp, shared with packing_keyswitch128.hip): one thread per output word
//     (p, j), looping over a slice of d.  For fixed d consecutive j
//     read consecutive words (a rotation only moves where the 8 N-byte row wraps), so every wave load is one or two
//     contiguous runs and needs no LDS staging; the adds wrap, so any split of the d range gives the same bits.  With
//     few GLWEs (one GLWE at N = 256, k = 4 is 1,280 outputs = 5 workgroups) the d range is split over `part`
//     workgroups whose partial sums go to scratch and pks_reduce_kernel adds them: plain stores, no atomics.
//   * T is capped (PKS_ROW_CAP_BYTES): larger calls run chunk by chunk on the caller's stream, whole GLWEs per chunk;
//     a GLWE whose rows alone exceed the cap is summed piecewise into the output (degree offset d0, accumulate).
//   * glwe_compress_kernel: one thread per packed u64 word gathers the modulus-switched values overlapping it
//     (PackedIntegers::pack's own loop, packed_integers.rs:89-121), so no word is written twice;
//     glwe_extract_kernel: one thread per output word (unpack :150-219, the scaling shift and the zeroed tail of the
//     body polynomial, compressed_modulus_switched_glwe_ciphertext.rs:240-249).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keyswitch_launch.hpp"
#include "ks_device.hpp"
#include "pks_rotate.hpp"

namespace mi {
namespace ks {

using u64 = uint64_t;

// packed[b][i], i < words: bits [64 i, 64 i + 64) of the little-end-first concatenation of the `count` values
// modulus_switch(glwe[b][j], log_mod), log_mod bits each
__global__ __launch_bounds__(256) void glwe_compress_kernel(u64* __restrict__ packed, const u64* __restrict__ glwe,
                                                            uint64_t glwe_words, uint64_t count, uint64_t words,
                                                            uint32_t log_mod, uint64_t batch) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * words) return;
  const uint64_t b = idx / words, i = idx % words;
  const u64* x = glwe + b * glwe_words;
  uint64_t j = 64 * i / log_mod;
  u64 value = ms_word<u64>(x[j], log_mod) >> (64 * i - j * log_mod);
  for (++j; j * log_mod < 64 * (i + 1) && j < count; ++j) value |= ms_word<u64>(x[j], log_mod) << (j * log_mod - 64 * i);
  packed[idx] = value;
}

// glwe[b][w], w < glwe_words: value w of packed[b] scaled back by 2^(64 - log_mod) for w < count, else 0 (the tail of
// the body polynomial)
__global__ __launch_bounds__(256) void glwe_extract_kernel(u64* __restrict__ glwe, const u64* __restrict__ packed,
                                                           uint64_t glwe_words, uint64_t count, uint64_t words,
                                                           uint32_t log_mod, uint64_t batch) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * glwe_words) return;
  const uint64_t b = idx / glwe_words, w = idx % glwe_words;
  u64 v = 0;
  if (w < count) {
    const u64* p = packed + b * words;
    const uint64_t start = w * log_mod, blk = start / 64, end_blk = (start + log_mod - 1) / 64;
    const uint32_t rem = (uint32_t)(start % 64);
    v = p[blk] >> rem;
    if (end_blk != blk) v |= p[blk + 1] << (64u - rem);  // rem > 0 here
    v <<= 64u - log_mod;  // drops the bits above log_mod (the reference's mask), then scales
  }
  glwe[idx] = v;
}

}  // namespace ks

static constexpr size_t PKS_MAX_ROWS = (size_t)1 << 21;  // rows of one GEMM launch (its batch bound is 2^22 - 1)

PksPlan pks_plan_rows(size_t out_size, size_t word_bytes, size_t n_lwe, size_t lwe_per_glwe) {
  PksPlan p;
  if (n_lwe == 0) return p;
  const size_t row_bytes = out_size * word_bytes, n_glwe = (n_lwe + lwe_per_glwe - 1) / lwe_per_glwe;
  size_t n_g, per;  // GLWEs and rows per GLWE of the largest rotate-and-sum launch
  if (lwe_per_glwe * row_bytes <= PKS_ROW_CAP_BYTES) {
    n_g = PKS_ROW_CAP_BYTES / (lwe_per_glwe * row_bytes);
    if (n_g * lwe_per_glwe > PKS_MAX_ROWS) n_g = PKS_MAX_ROWS / lwe_per_glwe;  // >= 1: lwe_per_glwe^2 <= 2^22 here
    if (n_g > n_glwe) n_g = n_glwe;
    per = lwe_per_glwe;
    p.rows = n_g * per;
  } else {  // one GLWE piecewise
    p.piecewise = true;
    n_g = 1;
    per = PKS_ROW_CAP_BYTES / row_bytes;
    if (per == 0) per = 1;
    p.rows = per;
  }
  if (p.rows > n_lwe) p.rows = n_lwe;
  // split the d range until the launch has ~1024 workgroups, slices of at least 8 rows
  const size_t blocks = n_g * ((out_size + 255) / 256);
  size_t part = (1024 + blocks - 1) / blocks;
  if (part > (per + 7) / 8) part = (per + 7) / 8;
  const size_t dl = (per + part - 1) / part;
  p.part = (per + dl - 1) / dl;
  p.t_bytes = p.rows * row_bytes;
  p.partial_bytes = p.part > 1 ? n_g * p.part * row_bytes : 0;
  return p;
}

PksPlan pks_plan(const KsGeometry& g, size_t n_lwe, size_t lwe_per_glwe) {
  PksPlan p = pks_plan_rows(g.out_size, 8, n_lwe, lwe_per_glwe);
  if (n_lwe != 0) p.digit_bytes = ks_digit_bytes(g, p.rows);
  return p;
}

hipError_t launch_packing_keyswitch(uint64_t* glwe_out, const uint64_t* lwe_in, const void* frag, void* t, void* digits,
                                    void* partials, size_t n_lwe, size_t lwe_per_glwe, size_t polynomial_size,
                                    const KsGeometry& g, const PksPlan& plan, hipStream_t st) {
  const size_t lwe_size = g.in_dim + 1;
  return ks::pks_run<uint64_t>(glwe_out, (uint64_t*)t, (uint64_t*)partials, n_lwe, lwe_per_glwe, polynomial_size,
                               g.out_size, plan, st, [&](size_t first, size_t rows) {
                                 return launch_keyswitch(t, lwe_in + first * lwe_size, frag, digits, rows, g, st);
                               });
}

size_t glwe_compressed_words(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus) {
  return (((size_t)glwe_dim * polynomial_size + bodies_count) * (size_t)log_modulus + 63) / 64;
}

hipError_t launch_glwe_compress(uint64_t* packed, const uint64_t* glwe, size_t polynomial_size, int glwe_dim,
                                size_t bodies_count, int log_modulus, size_t batch, hipStream_t st) {
  const uint64_t words = glwe_compressed_words(polynomial_size, glwe_dim, bodies_count, log_modulus);
  if (batch == 0 || words == 0) return hipSuccess;
  const uint64_t total = (uint64_t)batch * words;
  hipLaunchKernelGGL(ks::glwe_compress_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, packed, glwe,
                     (uint64_t)(glwe_dim + 1) * polynomial_size, (uint64_t)glwe_dim * polynomial_size + bodies_count,
                     words, (uint32_t)log_modulus, (uint64_t)batch);
  return hipGetLastError();
}

hipError_t launch_glwe_extract(uint64_t* glwe, const uint64_t* packed, size_t polynomial_size, int glwe_dim,
                               size_t bodies_count, int log_modulus, size_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  const uint64_t glwe_words = (uint64_t)(glwe_dim + 1) * polynomial_size, total = (uint64_t)batch * glwe_words;
  hipLaunchKernelGGL(ks::glwe_extract_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, glwe, packed,
                     glwe_words, (uint64_t)glwe_dim * polynomial_size + bodies_count,
                     (uint64_t)glwe_compressed_words(polynomial_size, glwe_dim, bodies_count, log_modulus),
                     (uint32_t)log_modulus, (uint64_t)batch);
  return hipGetLastError();
}

}  // namespace mi
