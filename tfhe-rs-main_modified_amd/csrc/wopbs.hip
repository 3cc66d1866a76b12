// wopbs.hip — the elementwise passes of the bootstrap without padding bit (WoP-PBS).
//
// Reference: tfhe/src/core_crypto/fft_impl/fft64/crypto/wop_pbs/mod.rs — extract_bits (:61-220),
// circuit_bootstrap_boolean + homomorphic_shift_boolean (:238-435), cmux_tree_memory_optimized (:459-583),
// vertical_packing (:771-825), blind_rotate_assign (:838-863).
//
// Every stage there is a loop over bootstraps, keyswitches and CMUXes with a few word-wise steps in between.  The heavy
// steps are the library's batched entry points (mi_fft64_pbs_batch*, mi_lwe_keyswitch_batch, mi_lwe_pfpks_batch,
// mi_fft64_cmux_batch_indexed, mi_bsk_to_fourier64, mi_sample_extract_batch), called by c_api_wopbs.cpp; this file
// holds the steps in between, each one memory-bound pass over its batch:
//   * the left shifts and body constants of extract_bits and homomorphic_shift_boolean, and their trivial accumulators;
//   * the CMUX tree's leaves.  The tree runs breadth-first and in place: the nodes of a layer are kept in bit-reversed
//     order, position p of tree t at GLWE p * trees + t, so node 2 m (position q) and node 2 m + 1 (position q + half)
//     of every tree are the items of one contiguous ct0 batch and one contiguous ct1 batch, and the layer's results,
//     left in ct0 by the CMUX, are the next layer's nodes in the same order: no data moves between layers;
//   * the monomial division of the rotation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "core_scalar.hpp"
#include "wopbs_launch.hpp"

namespace mi {
namespace wop {

using u64 = uint64_t;
using core::Monomial;

__device__ __forceinline__ uint64_t gs_start() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t gs_step() { return (uint64_t)gridDim.x * blockDim.x; }

static unsigned blocks_for(uint64_t count) {
  const uint64_t b = (count + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 65535u * 16u ? 65535u * 16u : b);
}

__global__ __launch_bounds__(256) void lwe_shift_kernel(u64* __restrict__ out, const u64* __restrict__ in,
                                                        uint64_t words, uint64_t n_in, uint64_t rep, int shift,
                                                        u64 body_add) {
  const uint64_t total = n_in * rep * words;
  for (uint64_t i = gs_start(); i < total; i += gs_step()) {
    const uint64_t w = i % words, b = i / words / rep;
    out[i] = (in[b * words + w] << shift) + (w == words - 1 ? body_add : 0);
  }
}

__global__ __launch_bounds__(256) void body_add_kernel(u64* __restrict__ lwe, uint64_t words, uint64_t n, uint64_t rep,
                                                       int exp0, int step) {
  for (uint64_t b = gs_start(); b < n; b += gs_step()) lwe[b * words + words - 1] += (u64)1 << (exp0 + step * (int)(b % rep));
}

__global__ __launch_bounds__(256) void fill_acc_kernel(u64* __restrict__ acc, uint64_t mask_words, uint64_t per,
                                                       uint64_t rep, int exp0, int step) {
  for (uint64_t i = gs_start(); i < per * rep; i += gs_step()) {
    const uint64_t l = i / per, w = i % per;
    acc[i] = w < mask_words ? 0 : (u64)0 - ((u64)1 << (exp0 + step * (int)l));
  }
}

__global__ __launch_bounds__(256) void iota_mod_kernel(uint32_t* __restrict__ idx, uint64_t count, uint64_t rep) {
  for (uint64_t i = gs_start(); i < count; i += gs_step()) idx[i] = (uint32_t)(i % rep);
}

__global__ __launch_bounds__(256) void sub_assign_kernel(u64* __restrict__ a, const u64* __restrict__ b,
                                                         uint64_t count) {
  for (uint64_t i = gs_start(); i < count; i += gs_step()) a[i] -= b[i];
}

__global__ __launch_bounds__(256) void copy_rows_kernel(u64* __restrict__ dst, uint64_t dst_stride,
                                                        const u64* __restrict__ src, uint64_t words, uint64_t n) {
  for (uint64_t i = gs_start(); i < words * n; i += gs_step()) dst[(i / words) * dst_stride + i % words] = src[i];
}

__global__ __launch_bounds__(256) void tree_leaves_kernel(u64* __restrict__ buf, const u64* __restrict__ lut,
                                                          uint32_t k, uint32_t logn, uint64_t n_polys, int r,
                                                          uint64_t trees, uint64_t t0, uint64_t n_outputs) {
  const uint64_t per = (uint64_t)(k + 1) << logn, total = (trees << r) * per;
  for (uint64_t i = gs_start(); i < total; i += gs_step()) {
    const uint64_t node = i / per, w = i % per;
    const uint64_t p = node / trees, t = node % trees;
    if (w < ((uint64_t)k << logn)) {
      buf[i] = 0;
      continue;
    }
    const uint64_t leaf = r ? (uint64_t)(__brev((uint32_t)p) >> (32 - r)) : 0;
    const uint64_t o = (t0 + t) % n_outputs;
    buf[i] = lut[((o * n_polys + leaf) << logn) + (w - ((uint64_t)k << logn))];
  }
}

__global__ __launch_bounds__(256) void ggsw_index_kernel(uint32_t* __restrict__ idx, uint64_t count, uint64_t trees,
                                                         uint64_t t0, uint64_t n_outputs, uint64_t ggsw_stride,
                                                         uint64_t g) {
  for (uint64_t i = gs_start(); i < count; i += gs_step())
    idx[i] = (uint32_t)(((t0 + i % trees) / n_outputs) * ggsw_stride + g);
}

__global__ __launch_bounds__(256) void monomial_div_kernel(u64* __restrict__ ct1, const u64* __restrict__ ct0,
                                                           uint64_t polys, uint32_t logn, u64 degree) {
  const uint32_t nn = 1u << logn;
  const Monomial x(degree, logn);
  for (uint64_t i = gs_start(); i < (polys << logn); i += gs_step()) {
    const uint32_t m = (uint32_t)i & (nn - 1);
    const u64 v = ct0[(i & ~(uint64_t)(nn - 1)) + x.div_src(m, nn)];
    ct1[i] = x.div_neg(m, nn) ? (u64)0 - v : v;
  }
}

}  // namespace wop

hipError_t launch_wop_lwe_shift(uint64_t* out, const uint64_t* in, size_t words, size_t n_in, size_t rep, int shift,
                                uint64_t body_add, hipStream_t s) {
  if (n_in * rep == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::lwe_shift_kernel, dim3(wop::blocks_for(n_in * rep * words)), dim3(256), 0, s, out, in,
                     (uint64_t)words, (uint64_t)n_in, (uint64_t)rep, shift, body_add);
  return hipGetLastError();
}

hipError_t launch_wop_body_add(uint64_t* lwe, size_t words, size_t n, size_t rep, int exp0, int step, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::body_add_kernel, dim3(wop::blocks_for(n)), dim3(256), 0, s, lwe, (uint64_t)words, (uint64_t)n,
                     (uint64_t)rep, exp0, step);
  return hipGetLastError();
}

hipError_t launch_wop_fill_acc(uint64_t* acc, size_t k, size_t n, size_t rep, int exp0, int step, hipStream_t s) {
  if (rep == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::fill_acc_kernel, dim3(wop::blocks_for((k + 1) * n * rep)), dim3(256), 0, s, acc,
                     (uint64_t)(k * n), (uint64_t)((k + 1) * n), (uint64_t)rep, exp0, step);
  return hipGetLastError();
}

hipError_t launch_wop_iota_mod(uint32_t* idx, size_t count, size_t rep, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::iota_mod_kernel, dim3(wop::blocks_for(count)), dim3(256), 0, s, idx, (uint64_t)count,
                     (uint64_t)rep);
  return hipGetLastError();
}

hipError_t launch_wop_sub_assign(uint64_t* a, const uint64_t* b, size_t count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::sub_assign_kernel, dim3(wop::blocks_for(count)), dim3(256), 0, s, a, b, (uint64_t)count);
  return hipGetLastError();
}

hipError_t launch_wop_copy_rows(uint64_t* dst, size_t dst_stride, const uint64_t* src, size_t words, size_t n,
                                hipStream_t s) {
  if (words * n == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::copy_rows_kernel, dim3(wop::blocks_for(words * n)), dim3(256), 0, s, dst,
                     (uint64_t)dst_stride, src, (uint64_t)words, (uint64_t)n);
  return hipGetLastError();
}

hipError_t launch_wop_tree_leaves(uint64_t* buf, const uint64_t* lut, size_t k, int logn, size_t n_polys, int r,
                                  size_t trees, size_t t0, size_t n_outputs, hipStream_t s) {
  if (trees == 0) return hipSuccess;
  const uint64_t total = ((uint64_t)trees << r) * ((uint64_t)(k + 1) << logn);
  hipLaunchKernelGGL(wop::tree_leaves_kernel, dim3(wop::blocks_for(total)), dim3(256), 0, s, buf, lut, (uint32_t)k,
                     (uint32_t)logn, (uint64_t)n_polys, r, (uint64_t)trees, (uint64_t)t0, (uint64_t)n_outputs);
  return hipGetLastError();
}

hipError_t launch_wop_ggsw_index(uint32_t* idx, size_t count, size_t trees, size_t t0, size_t n_outputs,
                                 size_t ggsw_stride, size_t g, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::ggsw_index_kernel, dim3(wop::blocks_for(count)), dim3(256), 0, s, idx, (uint64_t)count,
                     (uint64_t)trees, (uint64_t)t0, (uint64_t)n_outputs, (uint64_t)ggsw_stride, (uint64_t)g);
  return hipGetLastError();
}

hipError_t launch_wop_monomial_div(uint64_t* ct1, const uint64_t* ct0, size_t polys, int logn, uint64_t degree,
                                   hipStream_t s) {
  if (polys == 0) return hipSuccess;
  hipLaunchKernelGGL(wop::monomial_div_kernel, dim3(wop::blocks_for((uint64_t)polys << logn)), dim3(256), 0, s, ct1,
                     ct0, (uint64_t)polys, (uint32_t)logn, degree);
  return hipGetLastError();
}

}  // namespace mi
