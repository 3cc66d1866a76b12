// radix_sum_index_launch.hpp — host entry points of radix_sum_index.hip: the index arrays of the radix sum and
// multiplication drivers (c_api_radix_mul.cpp) that are no instance of IndexRule.  Everything a kernel has to know about
// a round arrives in its arguments (a struct by value), so that no driver copies from the host.
//
// Rows of a pass over I integers are numbered slot-major: the row of slot v of integer i is v * I + i, in the pool of
// block rows, in the list of chunk sums (slot = chunk) and in the list of packed pairs (slot = pair) alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mi {

// the by-value descriptors hold one entry per block: 128 blocks keep every argument struct under 3 KiB (the kernel
// argument segment is 4 KiB)
constexpr uint32_t RADIX_MAX_BLOCKS = 128;
constexpr uint32_t RADIX_GATHER_TERMS = 256;  // terms per launch of the gather rule

// One column of one round of the sum schedule.  The column's list is entries [list_off, list_off + len) of the list of
// slots the previous round wrote (round 0: the slots themselves, the pool starts column-major).  With q = len >= s ?
// len / s : 0 its chunks are chunks [chunk_off, chunk_off + q) of the round; its next list starts at new_off: the
// len - q s rows left, then the slots out_base + item_off ... of the carries of column b - 1's chunks and of the
// messages of its own chunks, which are items [item_off, ...) of the round's lookup.
struct SumColumn {
  uint32_t list_off, len, chunk_off, new_off, item_off;
};
struct SumRound {
  uint32_t n_cols, s, integers;
  uint32_t n_chunks, n_items, new_total;  // per integer
  uint32_t out_base;                      // first slot of the round's outputs
  uint32_t final_round;                   // 1: the block sums, one ragged "chunk" per column, row i * n_cols + b
  SumColumn col[RADIX_MAX_BLOCKS];
};
// A round (final_round = 0): sum_index (integers * n_chunks x s) gets the pool rows of every chunk, in_index and
// lut_index (integers * n_items) the chunk sum and the table (lut_msg / lut_carry) of every item, new_list (new_total)
// the next lists.  The block sums (final_round = 1): sum_index (integers * n_cols x s), row i * n_cols + b holding the
// rows of column b, padded with 0xFFFFFFFF; the other arrays are not written.  prev_list nullptr: the identity.
hipError_t launch_radix_sum_round(uint32_t* sum_index, uint32_t* in_index, uint32_t* lut_index, uint32_t* new_list,
                                  const uint32_t* prev_list, const SumRound& round, uint32_t lut_msg,
                                  uint32_t lut_carry, hipStream_t s);

// The rows of up to RADIX_GATHER_TERMS terms of a sum in the column-major pool: term t0 + u (u < n_terms) lives from
// block first[u] up and its block b goes to slot col_base[b] + #{u' < u : first[u'] <= b}.  index[slot * integers + i] =
// ((t0 + u) * n_integers + i0 + i) * n_cols + b, the row of the caller's `terms`.
struct SumGather {
  uint32_t n_cols, n_terms, t0, integers, n_integers, i0;
  uint32_t first[RADIX_GATHER_TERMS];
  uint32_t col_base[RADIX_MAX_BLOCKS];
};
hipError_t launch_radix_sum_gather(uint32_t* index, const SumGather& g, hipStream_t s);

// The triangular pair rule of the multiplication of B-block integers at message modulus m, for `integers` integers.
// Pair p = d (d + 1) / 2 + j is (lhs block d - j, rhs block j), d < B.  With `staged` = lhs[I B] | rhs[I B]:
//   pack_index[(p I + i) 2 + {0, 1}] = i B + d - j, I B + i B + j;  pack_coeff = m, 1
// The products are the pool's first slots, column-major in the reference's chain order: column b holds the lsb of the
// pairs (b - j, j), j = 0 .. b, then (with_msb) the msb of the pairs (b - 1 - j, j), j = 0 .. b - 1.  For slot v:
//   in_index[v I + i] = p I + i;  lut_index[v I + i] = lut_lsb or lut_msb
struct MulPairs {
  uint32_t n_blocks, integers, with_msb, lut_lsb, lut_msb;
  int64_t m;
};
hipError_t launch_radix_mul_pairs(uint32_t* pack_index, int64_t* pack_coeff, uint32_t* in_index, uint32_t* lut_index,
                                  const MulPairs& p, hipStream_t s);

}  // namespace mi
