// pks_rotate.hpp — the rotate-and-sum pass and the chunk loop of the packing keyswitches, shared by
// packing_keyswitch.hip (W = u64) and packing_keyswitch128.hip (W = unsigned __int128: the same adds and negations
// on two words, 16-byte accesses).  The GEMM of a chunk writes one row T[d] per ciphertext; the list form multiplies
// row d by X^d and sums the rows of a GLWE (polynomial_wrapping_monic_monomial_mul_assign +
// slice_wrapping_add_assign, lwe_packing_keyswitch.rs:369-378):
//   out[g][p][j] = sum_{d < cnt} +- T[g per + d][p N + ((j - d) mod N)], negated when j < d.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keyswitch_launch.hpp"

namespace mi {
namespace ks {

struct RotShape {
  uint32_t n_g;       // GLWEs of this launch
  uint32_t per;       // rows of T per GLWE
  uint32_t cnt_last;  // ciphertexts of the last GLWE (the others hold `per`)
  uint32_t d0;        // degree of a GLWE's first row (non-zero when one GLWE is summed piecewise)
  uint32_t log_n, out_size;  // N = 2^log_n, (k + 1) N words per row
  uint32_t wb;        // workgroups of 256 words per row
  uint32_t dl, part;  // rows per slice of the d range, slices per GLWE
  uint32_t accumulate;  // add to the output instead of overwriting it
};

// grid.x = n_g * wb, grid.y = part.  dst: the output GLWEs (part == 1) or the partial sums [g][slice][word].
template <typename W>
__global__ __launch_bounds__(256) void pks_rotate_sum_kernel(W* __restrict__ dst, const W* __restrict__ t,
                                                             RotShape s) {
  const uint32_t g = blockIdx.x / s.wb, w = (blockIdx.x % s.wb) * 256 + threadIdx.x, slice = blockIdx.y;
  if (w >= s.out_size) return;
  const uint32_t n_mask = (1u << s.log_n) - 1u, j = w & n_mask;
  const uint32_t cnt = g + 1 == s.n_g ? s.cnt_last : s.per;
  const uint32_t lo = slice * s.dl, hi = min(cnt, lo + s.dl);
  const W* row = t + ((uint64_t)g * s.per + lo) * s.out_size + (w - j);  // polynomial p of row lo
  W acc = 0;
#pragma unroll 4
  for (uint32_t d = lo; d < hi; ++d, row += s.out_size) {
    const uint32_t deg = s.d0 + d;  // < N: lwe_per_glwe <= N
    const W v = row[(j - deg) & n_mask];
    acc += j < deg ? (W)0 - v : v;
  }
  if (s.part == 1) {
    W* o = dst + (uint64_t)g * s.out_size + w;
    *o = s.accumulate ? *o + acc : acc;
  } else {
    dst[((uint64_t)g * s.part + slice) * s.out_size + w] = acc;
  }
}

// out[g][w] (+)= sum over the slices of partial[g][slice][w]; grid.x = n_g * wb
template <typename W>
__global__ __launch_bounds__(256) void pks_reduce_kernel(W* __restrict__ out, const W* __restrict__ partial,
                                                         RotShape s) {
  const uint32_t g = blockIdx.x / s.wb, w = (blockIdx.x % s.wb) * 256 + threadIdx.x;
  if (w >= s.out_size) return;
  const W* p = partial + (uint64_t)g * s.part * s.out_size + w;
  W* o = out + (uint64_t)g * s.out_size + w;
  W acc = s.accumulate ? *o : 0;
  for (uint32_t q = 0; q < s.part; ++q) acc += p[(uint64_t)q * s.out_size];
  *o = acc;
}

template <typename W>
hipError_t rotate_sum(W* out, const W* t, W* partials, RotShape s, hipStream_t st) {
  s.dl = (s.per + s.part - 1) / s.part;
  const dim3 grid1(s.n_g * s.wb, s.part);
  hipLaunchKernelGGL(pks_rotate_sum_kernel<W>, grid1, dim3(256), 0, st, s.part == 1 ? out : partials, t, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || s.part == 1) return e;
  hipLaunchKernelGGL(pks_reduce_kernel<W>, dim3(s.n_g * s.wb), dim3(256), 0, st, out, partials, s);
  return hipGetLastError();
}

// The chunks of one call (PksPlan): whole GLWEs per chunk, or pieces of plan.rows rows of one GLWE summed into the
// output.  gemm(first, rows) writes the keyswitched rows of ciphertexts [first, first + rows) to t.
template <typename W, typename Gemm>
hipError_t pks_run(W* glwe_out, W* t, W* partials, size_t n_lwe, size_t lwe_per_glwe, size_t polynomial_size,
                   size_t out_size, const PksPlan& plan, hipStream_t st, Gemm gemm) {
  if (n_lwe == 0) return hipSuccess;
  const size_t n_glwe = (n_lwe + lwe_per_glwe - 1) / lwe_per_glwe;
  RotShape s;
  s.log_n = (uint32_t)__builtin_ctzll(polynomial_size);
  s.out_size = (uint32_t)out_size;
  s.wb = (uint32_t)((out_size + 255) / 256);
  s.part = (uint32_t)plan.part;
  s.dl = 0;
  if (!plan.piecewise) {  // whole GLWEs per chunk
    const size_t gpc = (plan.rows + lwe_per_glwe - 1) / lwe_per_glwe;
    for (size_t g0 = 0; g0 < n_glwe; g0 += gpc) {
      const size_t first = g0 * lwe_per_glwe, rows = n_lwe - first < gpc * lwe_per_glwe ? n_lwe - first : gpc * lwe_per_glwe;
      hipError_t e = gemm(first, rows);
      if (e != hipSuccess) return e;
      s.n_g = (uint32_t)((rows + lwe_per_glwe - 1) / lwe_per_glwe);
      s.per = (uint32_t)lwe_per_glwe;
      s.cnt_last = (uint32_t)(rows - (size_t)(s.n_g - 1) * lwe_per_glwe);
      s.d0 = 0;
      s.accumulate = 0;
      e = rotate_sum<W>(glwe_out + g0 * out_size, t, partials, s, st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  for (size_t gi = 0; gi < n_glwe; ++gi) {  // one GLWE's rows exceed the cap: pieces of plan.rows rows
    const size_t first = gi * lwe_per_glwe, cnt = n_lwe - first < lwe_per_glwe ? n_lwe - first : lwe_per_glwe;
    for (size_t d0 = 0; d0 < cnt; d0 += plan.rows) {
      const size_t rows = cnt - d0 < plan.rows ? cnt - d0 : plan.rows;
      hipError_t e = gemm(first + d0, rows);
      if (e != hipSuccess) return e;
      s.n_g = 1;
      s.per = (uint32_t)plan.rows;  // the slices the partial sums were sized for
      s.cnt_last = (uint32_t)rows;
      s.d0 = (uint32_t)d0;
      s.accumulate = d0 != 0;
      e = rotate_sum<W>(glwe_out + gi * out_size, t, partials, s, st);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace ks
}  // namespace mi
