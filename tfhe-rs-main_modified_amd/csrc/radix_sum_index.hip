// radix_sum_index.hip — the index arrays of the radix sum of ciphertexts and of the radix multiplication.
//
// Reference: tfhe/src/integer/server_key/radix_parallel/sum.rs:14-147 (unchecked_partial_sum_ciphertexts_vec_
// parallelized: columns, chunks of max_sum_size rows, messages and carries moved to their columns) and mul.rs:333-400
// (compute_terms_for_mul_low: the lsb and msb terms of every rhs block).  The arithmetic of both runs in the existing
// linear combination, keyswitch and bootstrap kernels; the kernels here only say which row goes where.
//
// They are index writers: one thread per entry, consecutive threads consecutive entries (coalesced 4-byte stores, 8-byte
// for the coefficients), a capped grid that strides over the entries as launch_index_rule's does.  What describes a
// round is a struct passed by value (radix_sum_index_launch.hpp): it is read through the kernel argument segment, a
// thread finds its column by a scan over at most RADIX_MAX_BLOCKS prefix sums that every lane of a wave mostly shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "radix_sum_index_launch.hpp"

namespace mi {
namespace rsum {

constexpr unsigned MAX_BLOCKS = 256u * 16u;
constexpr uint32_t NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint64_t gs_start() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t gs_step() { return (uint64_t)gridDim.x * blockDim.x; }

static unsigned blocks_for(uint64_t count) {
  const uint64_t b = (count + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

// the chunks of a column: none while it has fewer than s rows
__device__ __forceinline__ uint32_t chunks_of(uint32_t len, uint32_t s) { return len >= s ? len / s : 0u; }

// the slot at position pos of column c's list
__device__ __forceinline__ uint32_t slot_at(const uint32_t* __restrict__ prev, const SumColumn& c, uint32_t pos) {
  return prev ? prev[c.list_off + pos] : c.list_off + pos;
}

__global__ __launch_bounds__(256) void sum_round_kernel(uint32_t* __restrict__ sum_index, uint32_t* __restrict__ in_index,
                                                        uint32_t* __restrict__ lut_index, uint32_t* __restrict__ new_list,
                                                        const uint32_t* __restrict__ prev, const SumRound r,
                                                        uint32_t lut_msg, uint32_t lut_carry) {
  const uint64_t I = r.integers, s = r.s;
  const uint64_t n_sum = (r.final_round ? (uint64_t)r.n_cols : (uint64_t)r.n_chunks) * I * s;
  const uint64_t n_item = r.final_round ? 0 : (uint64_t)r.n_items * I;
  const uint64_t n_list = r.final_round ? 0 : (uint64_t)r.new_total;
  const uint64_t total = n_sum + n_item + n_list;
  for (uint64_t e = gs_start(); e < total; e += gs_step()) {
    if (e < n_sum) {
      const uint32_t p = (uint32_t)(e % s);
      const uint64_t row = e / s;
      if (r.final_round) {  // row = i * n_cols + b: the rows of column b, ragged
        const uint32_t b = (uint32_t)(row % r.n_cols), i = (uint32_t)(row / r.n_cols);
        sum_index[e] = p < r.col[b].len ? (uint32_t)(slot_at(prev, r.col[b], p) * I + i) : NONE;
      } else {  // row = chunk * I + i
        const uint32_t chunk = (uint32_t)(row / I), i = (uint32_t)(row % I);
        uint32_t b = 0;
        while (b + 1 < r.n_cols && r.col[b + 1].chunk_off <= chunk) ++b;
        const uint32_t pos = (chunk - r.col[b].chunk_off) * (uint32_t)s + p;
        sum_index[e] = (uint32_t)(slot_at(prev, r.col[b], pos) * I + i);
      }
    } else if (e < n_sum + n_item) {
      const uint64_t j = e - n_sum;
      const uint32_t item = (uint32_t)(j / I), i = (uint32_t)(j % I);
      uint32_t b = 0;
      while (b + 1 < r.n_cols && r.col[b + 1].item_off <= item) ++b;
      const uint32_t k = item - r.col[b].item_off;
      const uint32_t below = b ? chunks_of(r.col[b - 1].len, r.s) : 0u;  // the carries of column b - 1 come first
      const bool carry = k < below;
      const uint32_t chunk = carry ? r.col[b - 1].chunk_off + k : r.col[b].chunk_off + (k - below);
      in_index[j] = (uint32_t)(chunk * I + i);
      lut_index[j] = carry ? lut_carry : lut_msg;
    } else {
      const uint32_t j = (uint32_t)(e - n_sum - n_item);
      uint32_t b = 0;
      while (b + 1 < r.n_cols && r.col[b + 1].new_off <= j) ++b;
      const uint32_t pos = j - r.col[b].new_off, len = r.col[b].len;
      const uint32_t used = chunks_of(len, r.s) * r.s, rest = len - used;
      new_list[j] = pos < rest ? slot_at(prev, r.col[b], used + pos) : r.out_base + r.col[b].item_off + (pos - rest);
    }
  }
}

__global__ __launch_bounds__(256) void sum_gather_kernel(uint32_t* __restrict__ index, const SumGather g) {
  const uint64_t I = g.integers;
  const uint64_t total = (uint64_t)g.n_terms * g.n_cols * I;
  for (uint64_t e = gs_start(); e < total; e += gs_step()) {
    const uint32_t i = (uint32_t)(e % I);
    const uint32_t b = (uint32_t)((e / I) % g.n_cols), u = (uint32_t)(e / I / g.n_cols);
    if (b < g.first[u]) continue;  // the term is zero here: no slot, and its row is never read
    uint32_t rank = 0;
    for (uint32_t v = 0; v < u; ++v) rank += g.first[v] <= b ? 1u : 0u;
    const uint64_t slot = g.col_base[b] + rank;
    index[slot * I + i] = (uint32_t)((((uint64_t)(g.t0 + u) * g.n_integers + g.i0 + i) * g.n_cols) + b);
  }
}

// the largest d with d (d + 1) / 2 <= v, v < 2^15
__device__ __forceinline__ uint32_t tri_root(uint32_t v) {
  uint32_t d = (uint32_t)((__fsqrt_rn(8.0f * (float)v + 1.0f) - 1.0f) * 0.5f);
  while (d * (d + 1) / 2 > v) --d;
  while ((d + 1) * (d + 2) / 2 <= v) ++d;
  return d;
}

// the largest b with b b <= v, v < 2^15
__device__ __forceinline__ uint32_t sq_root(uint32_t v) {
  uint32_t b = (uint32_t)__fsqrt_rn((float)v);
  while (b * b > v) --b;
  while ((b + 1) * (b + 1) <= v) ++b;
  return b;
}

__global__ __launch_bounds__(256) void mul_pairs_kernel(uint32_t* __restrict__ pack_index, int64_t* __restrict__ pack_coeff,
                                                        uint32_t* __restrict__ in_index, uint32_t* __restrict__ lut_index,
                                                        const MulPairs a) {
  const uint64_t I = a.integers, B = a.n_blocks;
  const uint64_t n_pack = B * (B + 1) / 2 * I * 2;
  const uint64_t n_item = (a.with_msb ? B * B : B * (B + 1) / 2) * I;
  for (uint64_t e = gs_start(); e < n_pack + n_item; e += gs_step()) {
    if (e < n_pack) {
      const uint32_t side = (uint32_t)(e & 1), i = (uint32_t)((e >> 1) % I), p = (uint32_t)((e >> 1) / I);
      const uint32_t d = tri_root(p), j = p - d * (d + 1) / 2;
      pack_index[e] = (uint32_t)(side ? I * B + i * B + j : i * B + (d - j));
      pack_coeff[e] = side ? (int64_t)1 : a.m;
    } else {
      const uint64_t q = e - n_pack;
      const uint32_t i = (uint32_t)(q % I), v = (uint32_t)(q / I);
      // column b starts at slot b^2 with the msb terms (2 b + 1 rows), at b (b + 1) / 2 without (b + 1 rows)
      const uint32_t b = a.with_msb ? sq_root(v) : tri_root(v);
      const uint32_t k = v - (a.with_msb ? b * b : b * (b + 1) / 2);
      const bool msb = k > b;
      const uint32_t p = msb ? (b - 1) * b / 2 + (k - b - 1) : b * (b + 1) / 2 + k;
      in_index[q] = (uint32_t)(p * I + i);
      lut_index[q] = msb ? a.lut_msb : a.lut_lsb;
    }
  }
}

}  // namespace rsum

hipError_t launch_radix_sum_round(uint32_t* sum_index, uint32_t* in_index, uint32_t* lut_index, uint32_t* new_list,
                                  const uint32_t* prev_list, const SumRound& round, uint32_t lut_msg,
                                  uint32_t lut_carry, hipStream_t s) {
  const uint64_t I = round.integers;
  const uint64_t total = round.final_round
                             ? (uint64_t)round.n_cols * I * round.s
                             : (uint64_t)round.n_chunks * I * round.s + (uint64_t)round.n_items * I + round.new_total;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(rsum::sum_round_kernel, dim3(rsum::blocks_for(total)), dim3(256), 0, s, sum_index, in_index,
                     lut_index, new_list, prev_list, round, lut_msg, lut_carry);
  return hipGetLastError();
}

hipError_t launch_radix_sum_gather(uint32_t* index, const SumGather& g, hipStream_t s) {
  const uint64_t total = (uint64_t)g.n_terms * g.n_cols * g.integers;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(rsum::sum_gather_kernel, dim3(rsum::blocks_for(total)), dim3(256), 0, s, index, g);
  return hipGetLastError();
}

hipError_t launch_radix_mul_pairs(uint32_t* pack_index, int64_t* pack_coeff, uint32_t* in_index, uint32_t* lut_index,
                                  const MulPairs& p, hipStream_t s) {
  if (p.integers == 0 || p.n_blocks == 0) return hipSuccess;
  const uint64_t B = p.n_blocks, I = p.integers;
  const uint64_t total = B * (B + 1) * I + (p.with_msb ? B * B : B * (B + 1) / 2) * I;
  hipLaunchKernelGGL(rsum::mul_pairs_kernel, dim3(rsum::blocks_for(total)), dim3(256), 0, s, pack_index, pack_coeff,
                     in_index, lut_index, p);
  return hipGetLastError();
}

}  // namespace mi
