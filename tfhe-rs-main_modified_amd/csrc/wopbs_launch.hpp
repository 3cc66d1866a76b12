// wopbs_launch.hpp — host entry points of wopbs.hip: the elementwise passes between the public stages of the
// bootstrap without padding bit (fft_impl/fft64/crypto/wop_pbs/mod.rs).  The transforms, the keyswitches and the
// bootstraps themselves are the existing entry points; c_api_wopbs.cpp strings them together.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mi {

// out[(b * rep + l)][i] = (in[b][i] << shift) + (i == words - 1 ? body_add : 0) for b < n_in, l < rep: the left shift of
// extract_bits (:156-162) and lwe_ciphertext_cleartext_mul by 2^shift with q/4 added (homomorphic_shift_boolean,
// :389-398), once per output level
hipError_t launch_wop_lwe_shift(uint64_t* out, const uint64_t* in, size_t words, size_t n_in, size_t rep, int shift,
                                uint64_t body_add, hipStream_t s);
// lwe[b][words - 1] += 2^(exp0 + step * (b % rep)) for b < n
hipError_t launch_wop_body_add(uint64_t* lwe, size_t words, size_t n, size_t rep, int exp0, int step, hipStream_t s);
// rep trivial accumulators of (k + 1) N words: zero mask, every body coefficient -2^(exp0 + step * l) (:193-200,
// :411-418)
hipError_t launch_wop_fill_acc(uint64_t* acc, size_t k, size_t n, size_t rep, int exp0, int step, hipStream_t s);
// idx[i] = i % rep
hipError_t launch_wop_iota_mod(uint32_t* idx, size_t count, size_t rep, hipStream_t s);
// a[i] -= b[i]
hipError_t launch_wop_sub_assign(uint64_t* a, const uint64_t* b, size_t count, hipStream_t s);
// dst[b * dst_stride + i] = src[b * words + i] for b < n, i < words
hipError_t launch_wop_copy_rows(uint64_t* dst, size_t dst_stride, const uint64_t* src, size_t words, size_t n,
                                hipStream_t s);

// The CMUX tree's working set: `trees` trees of 2^r nodes, node position p of tree t at GLWE p * trees + t, so that
// the first half of the positions is a contiguous ct0 batch and the second half the matching ct1 batch at every layer.
// Leaf position p holds LUT polynomial bitrev_r(p) of output (t0 + t) % n_outputs as a trivial GLWE.
hipError_t launch_wop_tree_leaves(uint64_t* buf, const uint64_t* lut, size_t k, int logn, size_t n_polys, int r,
                                  size_t trees, size_t t0, size_t n_outputs, hipStream_t s);
// idx[i] = ((t0 + i % trees) / n_outputs) * ggsw_stride + g: the GGSW of item i's evaluation
hipError_t launch_wop_ggsw_index(uint32_t* idx, size_t count, size_t trees, size_t t0, size_t n_outputs,
                                 size_t ggsw_stride, size_t g, hipStream_t s);
// ct1[i] = ct0[i] / X^degree for `polys` polynomials of 2^logn coefficients (polynomial_wrapping_monic_monomial_div_
// assign with its full-cycle rule: degree is taken mod 2N)
hipError_t launch_wop_monomial_div(uint64_t* ct1, const uint64_t* ct0, size_t polys, int logn, uint64_t degree,
                                   hipStream_t s);

}  // namespace mi
