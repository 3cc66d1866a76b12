// packing_keyswitch128.hip — the LWE packing keyswitch and the GLWE modulus-switch compression at Scalar = u128:
// shortint's compression of noise-squashed ciphertexts (compress_noise_squashed_ciphertexts_into_list,
// shortint/list_compression/noise_squashing_compression.rs:23-118; V1_4_NOISE_SQUASHING_COMP_PARAM_MESSAGE_2_CARRY_2_
// KS_PBS_TUNIFORM_2M128, shortint/parameters/v1_4/noise_squashing/p_fail_2_minus_128/mod.rs:21-32: base 2^61, one
// level, k = 6, N = 1024, 128 LWEs per GLWE, native u128, input LWE dimension 4096).
//
// Reference (paths relative to tfhe/src/core_crypto): algorithms/lwe_packing_keyswitch.rs:102-187
// (keyswitch_lwe_ciphertext_into_glwe_ciphertext) and :296-379 (the list form), generic in Scalar; entities/
// compressed_modulus_switched_glwe_ciphertext.rs:169-256 over entities/packed_integers.rs:39-222 and modulus_switch
// (fft_impl/common.rs:10-23).  Every u128 is two little-endian u64 words, 16-byte aligned.
//
// For one ciphertext T = (0, .., body at word k N, .., 0) - sum_i sum_li d_{i,li} KEY[i][li] mod 2^128, d_{i,.} the
// digits of decompose(closest_representable(a_i)), least significant first, pairing with the key block's entries in
// stored order.  Over a batch this is a GEMM mod 2^128, rows x (in_dim level) x ((k + 1) N), on
// v_mfma_i32_16x16x64_i8:
//   * every key word is recoded once into 16 signed bytes, x = sum_t s_t 2^(8t) mod 2^128 (pksk128_prepare_kernel;
//     the prepared key has the size of the raw key);
//   * every digit into nd = ceil((base_log + 1) / 8) signed bytes, d = sum_s e_s 2^(8s) (pks128_digits_kernel, the
//     pre-rounded decomposition of ks128_decomp.hpp);
//   * acc[u] += e_s s_t for every pair with u = s + t < 16 (pairs with s + t >= 16 vanish mod 2^128): 16 i32
//     accumulators per output tile, sum_{s < nd} (16 - s) MFMAs per 16 x 16 x 64 step (100 at nd = 8) over a depth of
//     in_dim level.  |acc[u]| <= in_dim level min(nd, 16) 2^14 < 2^31 under the rule in_dim level nd < 2^17 that key
//     creation enforces;
//   * the fold T = base - sum_u acc[u] << 8u in two-word arithmetic.
// (The u64 engine's scheme, key rows pre-shifted once per digit byte, would need 16 x 8 = 128 MFMAs per step and an
// 8 times larger prepared key, 3.76 GB at the production shape.)
// Fragment maps as keyswitch.hip: lane l holds row / column (l & 15) of the tile and the 16 consecutive k of group
// l >> 4; C/D: col = l & 15, row = 4 (l >> 4) + reg.
//   afrag[((rt KB + kb) nd + s) 64 + lane]  byte s of the digits k = 64 kb + 16 (lane >> 4) + j of row 16 rt + (lane & 15)
//   bfrag[((ct KB + kb) 16 + t) 64 + lane]  byte t of key rows k (as above), column 16 ct + (lane & 15)
// pks128_gemm_kernel: a 4-wave workgroup owns 64 rows x 32 columns, each wave 2 row tiles x 1 column tile (32
// accumulators of 16 x 16 i32); a step's fragments are whole 1 KiB wave loads straight from global memory into
// registers, the next step's issued before this step's MFMAs.  No LDS staging: the two waves that share a fragment
// read it through the CU's vector cache.  Workgroups are mapped XCD-aware (gemm_block).
// The rotate-and-sum pass and the chunking (pks_plan_rows, PKS_ROW_CAP_BYTES, the piecewise case) are
// pks_rotate.hpp's at W = u128.  glwe_compress128_kernel / glwe_extract128_kernel: PackedIntegers<u128> packs into
// 128-bit words; as (lo, hi) u64 pairs that is the bit string the u64 packer writes, rounded up to an even word count.
//
// Out of scope here: sample extraction of u128 LWEs at a monomial degree (the list's unpack, a client-side step),
// non-native u128 moduli, the C++ mirror header, serialised formats, and fusing the
// digit pass into the GEMM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keyswitch_launch.hpp"
#include "ks128_decomp.hpp"
#include "pks_rotate.hpp"

namespace mi {
namespace ks128 {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

static constexpr int MT = 2;             // row tiles (of 16) per wave
static constexpr int WAVE_R = 2, WAVE_C = 2;  // waves of a workgroup: row groups x column tiles
static constexpr int ROW_TILES = MT * WAVE_R;  // row tiles per workgroup: rows are padded to whole workgroups
static constexpr int NPL = 16;           // signed-byte planes of a key word

struct Shape {
  uint32_t in_dim, out_size, level, base_log, nd;
  uint32_t K, KB;  // GEMM depth in_dim level, its blocks of 64
  uint32_t CT;     // column tiles, padded to whole workgroups (WAVE_C)
  uint32_t body_col;
};

__device__ __forceinline__ uint4 pack16(const int8_t (&b)[16]) {
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    w[q] = (uint32_t)(uint8_t)b[4 * q] | ((uint32_t)(uint8_t)b[4 * q + 1] << 8) |
           ((uint32_t)(uint8_t)b[4 * q + 2] << 16) | ((uint32_t)(uint8_t)b[4 * q + 3] << 24);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// once per key: one thread per (column tile, k block, lane) recodes its 16 key words and writes their 16 planes;
// columns >= out_size and rows >= K are zero
__global__ __launch_bounds__(256) void pksk128_prepare_kernel(uint4* __restrict__ frag, const u128* __restrict__ ksk,
                                                              Shape s) {
  const uint64_t total = (uint64_t)s.CT * s.KB * 64;
  for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t lane = idx & 63;
    const uint64_t piece = idx >> 6;  // ct * KB + kb
    const uint32_t kb = (uint32_t)(piece % s.KB), ct = (uint32_t)(piece / s.KB);
    const uint32_t col = ct * 16 + (lane & 15), k0 = kb * 64 + 16 * (lane >> 4);
    uint32_t w[NPL][4];
#pragma unroll
    for (int t = 0; t < NPL; ++t) w[t][0] = w[t][1] = w[t][2] = w[t][3] = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t k = k0 + j;
      const u128 x = (k < s.K && col < s.out_size) ? ksk[(uint64_t)k * s.out_size + col] : (u128)0;
      int8_t o[NPL];
      signed_bytes16(x, o);
#pragma unroll
      for (int t = 0; t < NPL; ++t) w[t][j >> 2] |= (uint32_t)(uint8_t)o[t] << (8 * (j & 3));
    }
#pragma unroll
    for (int t = 0; t < NPL; ++t) frag[(piece * NPL + t) * 64 + lane] = make_uint4(w[t][0], w[t][1], w[t][2], w[t][3]);
  }
}

// per batch: one thread per (row tile, k block, lane) decomposes its 16 digit columns k = i level + li (terms least
// significant first, iter.rs:103-119) and writes their nd byte planes; rows >= batch and k >= K are zero
__global__ __launch_bounds__(256) void pks128_digits_kernel(uint4* __restrict__ afrag, const u128* __restrict__ lwe_in,
                                                            uint32_t batch, uint32_t row_tiles, Shape s) {
  const uint64_t total = (uint64_t)row_tiles * s.KB * 64;
  const int bl = (int)s.base_log, lv = (int)s.level;
  for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t lane = idx & 63;
    const uint64_t piece = idx >> 6;  // rt * KB + kb
    const uint32_t kb = (uint32_t)(piece % s.KB), rt = (uint32_t)(piece / s.KB);
    const uint32_t row = rt * 16 + (lane & 15), k0 = kb * 64 + 16 * (lane >> 4);
    const bool live = row < batch;
    const u128* x = lwe_in + (uint64_t)row * (s.in_dim + 1);
    uint32_t i = k0 / s.level, li = k0 - i * s.level;
    u128 state = 0;
    if (live && k0 < s.K) {  // the state after terms 0 .. li - 1 of coefficient i
      state = core::decomp_init<u128>(x[i], bl, lv, true);
      for (uint32_t u = 0; u < li; ++u) (void)core::decomp_next<u128>(bl, state);
    }
    int64_t d[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t k = k0 + j;
      d[j] = 0;
      if (live && k < s.K) {
        d[j] = (int64_t)(i128)core::decomp_next<u128>(bl, state);
        if (++li == s.level) {  // next mask coefficient
          li = 0;
          ++i;
          if (k + 1 < s.K) state = core::decomp_init<u128>(x[i], bl, lv, true);
        }
      }
    }
    for (uint32_t sb = 0; sb < s.nd; ++sb) {
      int8_t b[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) b[j] = digit_byte(d[j], (int)sb);
      afrag[(piece * s.nd + sb) * 64 + lane] = pack16(b);
    }
  }
}

__device__ __forceinline__ i32x4 as_frag(const uint4 x) { return i32x4{(int)x.x, (int)x.y, (int)x.z, (int)x.w}; }

// Block bid of the launch order -> (row group, column group): workgroups x, x + 8, ... are dispatched to the same XCD,
// so XCD x takes the contiguous range [x * per, (x + 1) * per) of an order that walks the row groups inside each
// column group: the workgroups an XCD runs together share a few column groups' key fragments in its L2, and the key
// is read from memory once per launch rather than once per XCD (keyswitch.hip's ks_block).
__device__ __forceinline__ bool gemm_block(uint32_t bid, uint32_t n_rg, uint32_t n_cg, uint32_t& rg, uint32_t& cg) {
  const uint32_t tiles = n_rg * n_cg, per = (tiles + 7) / 8, t = (bid & 7) * per + (bid >> 3);
  if (t >= tiles) return false;
  rg = t % n_rg;
  cg = t / n_rg;
  return true;
}

// t[row][col] = base - sum_u acc[u] << 8u mod 2^128, base = the input body at col == body_col, else 0.
// grid.x = 8 * ceil(n_rg * n_cg / 8) (gemm_block).
template <int ND>
__global__ __launch_bounds__(64 * WAVE_R * WAVE_C) void pks128_gemm_kernel(u128* __restrict__ t,
                                                                           const u128* __restrict__ lwe_in,
                                                                           const uint4* __restrict__ afrag,
                                                                           const uint4* __restrict__ bfrag,
                                                                           uint32_t batch, uint32_t n_rg, Shape s) {
  uint32_t rg, cg;
  if (!gemm_block(blockIdx.x, n_rg, s.CT / WAVE_C, rg, cg)) return;  // whole workgroup; the kernel has no barrier
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w / WAVE_C, wc = w % WAVE_C;
  const uint32_t rt0 = (rg * WAVE_R + wr) * MT, ct = cg * WAVE_C + wc;
  const uint4* pa = afrag + (uint64_t)rt0 * s.KB * (ND * 64) + lane;  // row tile m adds m * KB * ND * 64
  const uint4* pb = bfrag + (uint64_t)ct * s.KB * (NPL * 64) + lane;
  const uint64_t a_tile = (uint64_t)s.KB * (ND * 64);
  i32x4 acc[MT][NPL];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int u = 0; u < NPL; ++u) acc[m][u] = i32x4{0, 0, 0, 0};
  uint4 A[MT][ND], B[NPL], NA[MT][ND], NB[NPL];
  auto load = [&](uint32_t kb, uint4(&a)[MT][ND], uint4(&b)[NPL]) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int sb = 0; sb < ND; ++sb) a[m][sb] = pa[m * a_tile + ((uint64_t)kb * ND + sb) * 64];
#pragma unroll
    for (int p = 0; p < NPL; ++p) b[p] = pb[((uint64_t)kb * NPL + p) * 64];
  };
  load(0, A, B);
  for (uint32_t kb = 0; kb < s.KB; ++kb) {
    load(kb + 1 < s.KB ? kb + 1 : kb, NA, NB);  // the last step reloads itself: unused
#pragma unroll
    for (int sb = 0; sb < ND; ++sb)
#pragma unroll
      for (int p = 0; p + sb < NPL; ++p)
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[m][sb + p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(as_frag(A[m][sb]), as_frag(B[p]), acc[m][sb + p], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int sb = 0; sb < ND; ++sb) A[m][sb] = NA[m][sb];
#pragma unroll
    for (int p = 0; p < NPL; ++p) B[p] = NB[p];
  }
  const uint32_t col = ct * 16 + (lane & 15);
  if (col >= s.out_size) return;
  const bool is_body = col == s.body_col;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t row = (rt0 + m) * 16 + 4 * (lane >> 4) + r;
      if (row >= batch) continue;
      u128 v = 0;
#pragma unroll
      for (int u = 0; u < NPL; ++u) v += (u128)(i128)acc[m][u][r] << (8 * u);
      const u128 base = is_body ? lwe_in[(uint64_t)row * (s.in_dim + 1) + s.in_dim] : (u128)0;
      t[(uint64_t)row * s.out_size + col] = base - v;
    }
  }
}

// modulus_switch (fft_impl/common.rs:10-23) at Scalar = u128: identity at log_mod == 128
__device__ __forceinline__ u128 ms_word128(u128 x, uint32_t log_mod) {
  return log_mod >= 128u ? x : (u128)(x + ((u128)1 << (128u - log_mod - 1u))) >> (128u - log_mod);
}

// packed[b][i], i < words: bits [128 i, 128 i + 128) of the little-end-first concatenation of the `count` values
// modulus_switch(glwe[b][j], log_mod), log_mod bits each (PackedIntegers::pack's own loop, packed_integers.rs:89-121,
// one thread per packed word)
__global__ __launch_bounds__(256) void glwe_compress128_kernel(u128* __restrict__ packed, const u128* __restrict__ glwe,
                                                               uint64_t glwe_words, uint64_t count, uint64_t words,
                                                               uint32_t log_mod, uint64_t batch) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * words) return;
  const uint64_t b = idx / words, i = idx % words;
  const u128* x = glwe + b * glwe_words;
  uint64_t j = 128 * i / log_mod;
  u128 value = ms_word128(x[j], log_mod) >> (128 * i - j * log_mod);
  for (++j; j * log_mod < 128 * (i + 1) && j < count; ++j) value |= ms_word128(x[j], log_mod) << (j * log_mod - 128 * i);
  packed[idx] = value;
}

// glwe[b][w], w < glwe_words: value w of packed[b] scaled back by 2^(128 - log_mod) for w < count, else 0 (the tail of
// the body polynomial; unpack packed_integers.rs:150-219, compressed_modulus_switched_glwe_ciphertext.rs:240-249)
__global__ __launch_bounds__(256) void glwe_extract128_kernel(u128* __restrict__ glwe, const u128* __restrict__ packed,
                                                              uint64_t glwe_words, uint64_t count, uint64_t words,
                                                              uint32_t log_mod, uint64_t batch) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * glwe_words) return;
  const uint64_t b = idx / glwe_words, w = idx % glwe_words;
  u128 v = 0;
  if (w < count) {
    const u128* p = packed + b * words;
    const uint64_t start = w * log_mod, blk = start / 128, end_blk = (start + log_mod - 1) / 128;
    const uint32_t rem = (uint32_t)(start % 128);
    v = p[blk] >> rem;
    if (end_blk != blk) v |= p[blk + 1] << (128u - rem);  // rem > 0 here
    v <<= 128u - log_mod;  // drops the bits above log_mod (the reference's mask), then scales
  }
  glwe[idx] = v;
}

static Shape make_shape(const Pks128Geometry& g) {
  Shape s;
  s.in_dim = (uint32_t)g.in_dim;
  s.out_size = (uint32_t)g.out_size;
  s.level = (uint32_t)g.level;
  s.base_log = (uint32_t)g.base_log;
  s.nd = (uint32_t)digit_bytes(g.base_log);
  s.K = (uint32_t)(g.in_dim * (size_t)g.level);
  s.KB = (s.K + 63) / 64;
  s.CT = (uint32_t)((g.out_size + 16 * WAVE_C - 1) / (16 * WAVE_C) * WAVE_C);
  s.body_col = (uint32_t)g.body_col;
  return s;
}

static uint32_t padded_row_tiles(size_t rows) { return (uint32_t)((rows + 16 * ROW_TILES - 1) / (16 * ROW_TILES) * ROW_TILES); }

static unsigned capped_grid(uint64_t threads) {
  const uint64_t blocks = (threads + 255) / 256;
  return (unsigned)(blocks < 65535 * 4 ? blocks : 65535 * 4);
}

// digits, then the GEMM, of `rows` ciphertexts into t
static hipError_t launch_gemm(u128* t, const u128* lwe_in, const void* frag, void* digits, size_t rows, const Shape& s,
                              hipStream_t st) {
  const uint32_t row_tiles = padded_row_tiles(rows);
  hipLaunchKernelGGL(pks128_digits_kernel, dim3(capped_grid((uint64_t)row_tiles * s.KB * 64)), dim3(256), 0, st,
                     (uint4*)digits, lwe_in, (uint32_t)rows, row_tiles, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t n_rg = row_tiles / ROW_TILES, n_cg = s.CT / WAVE_C;
  const dim3 grid(8 * ((n_rg * n_cg + 7) / 8)), block(64 * WAVE_R * WAVE_C);
#define MI_PKS128_GEMM(ND)                                                                                       \
  case ND:                                                                                                       \
    hipLaunchKernelGGL(pks128_gemm_kernel<ND>, grid, block, 0, st, t, lwe_in, (const uint4*)digits,              \
                       (const uint4*)frag, (uint32_t)rows, n_rg, s);                                             \
    break;
  switch (s.nd) {
    MI_PKS128_GEMM(1)
    MI_PKS128_GEMM(2)
    MI_PKS128_GEMM(3)
    MI_PKS128_GEMM(4)
    MI_PKS128_GEMM(5)
    MI_PKS128_GEMM(6)
    MI_PKS128_GEMM(7)
    MI_PKS128_GEMM(8)
    default:
      return hipErrorInvalidValue;  // base_log > 63: refused at key creation
  }
#undef MI_PKS128_GEMM
  return hipGetLastError();
}

}  // namespace ks128

size_t pks128_key_bytes(const Pks128Geometry& g) {
  const ks128::Shape s = ks128::make_shape(g);
  return (size_t)s.CT * s.KB * ks128::NPL * 64 * 16;
}

size_t pks128_digit_bytes(const Pks128Geometry& g, size_t rows) {
  const ks128::Shape s = ks128::make_shape(g);
  return (size_t)ks128::padded_row_tiles(rows) * s.KB * s.nd * 64 * 16;
}

hipError_t launch_pksk128_prepare(void* frag, const uint64_t* pksk, const Pks128Geometry& g, hipStream_t st) {
  const ks128::Shape s = ks128::make_shape(g);
  hipLaunchKernelGGL(ks128::pksk128_prepare_kernel, dim3(ks128::capped_grid((uint64_t)s.CT * s.KB * 64)), dim3(256), 0,
                     st, (uint4*)frag, (const ks128::u128*)pksk, s);
  return hipGetLastError();
}

hipError_t launch_packing_keyswitch128(uint64_t* glwe_out, const uint64_t* lwe_in, const void* frag, void* t,
                                       void* digits, void* partials, size_t n_lwe, size_t lwe_per_glwe,
                                       size_t polynomial_size, const Pks128Geometry& g, const PksPlan& plan,
                                       hipStream_t st) {
  using ks128::u128;
  const ks128::Shape s = ks128::make_shape(g);
  const u128* in = (const u128*)lwe_in;
  const size_t lwe_size = g.in_dim + 1;
  return ks::pks_run<u128>((u128*)glwe_out, (u128*)t, (u128*)partials, n_lwe, lwe_per_glwe, polynomial_size,
                           g.out_size, plan, st, [&](size_t first, size_t rows) {
                             return ks128::launch_gemm((u128*)t, in + first * lwe_size, frag, digits, rows, s, st);
                           });
}

size_t glwe_compressed_words128(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus) {
  return (((size_t)glwe_dim * polynomial_size + bodies_count) * (size_t)log_modulus + 127) / 128;
}

hipError_t launch_glwe_compress128(uint64_t* packed, const uint64_t* glwe, size_t polynomial_size, int glwe_dim,
                                   size_t bodies_count, int log_modulus, size_t batch, hipStream_t st) {
  using ks128::u128;
  const uint64_t words = glwe_compressed_words128(polynomial_size, glwe_dim, bodies_count, log_modulus);
  if (batch == 0 || words == 0) return hipSuccess;
  const uint64_t total = (uint64_t)batch * words;
  hipLaunchKernelGGL(ks128::glwe_compress128_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     (u128*)packed, (const u128*)glwe, (uint64_t)(glwe_dim + 1) * polynomial_size,
                     (uint64_t)glwe_dim * polynomial_size + bodies_count, words, (uint32_t)log_modulus,
                     (uint64_t)batch);
  return hipGetLastError();
}

hipError_t launch_glwe_extract128(uint64_t* glwe, const uint64_t* packed, size_t polynomial_size, int glwe_dim,
                                  size_t bodies_count, int log_modulus, size_t batch, hipStream_t st) {
  using ks128::u128;
  if (batch == 0) return hipSuccess;
  const uint64_t glwe_words = (uint64_t)(glwe_dim + 1) * polynomial_size, total = (uint64_t)batch * glwe_words;
  hipLaunchKernelGGL(ks128::glwe_extract128_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     (u128*)glwe, (const u128*)packed, glwe_words, (uint64_t)glwe_dim * polynomial_size + bodies_count,
                     (uint64_t)glwe_compressed_words128(polynomial_size, glwe_dim, bodies_count, log_modulus),
                     (uint32_t)log_modulus, (uint64_t)batch);
  return hipGetLastError();
}

}  // namespace mi
