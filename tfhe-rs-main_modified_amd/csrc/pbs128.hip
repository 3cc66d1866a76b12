// pbs128.hip — the exact 128-bit programmable bootstrap on the Goldilocks NTT: external product, CMUX, blind rotation
// and PBS over Z_{2^128}[X]/(X^N + 1) (shortint's noise squashing, V1_4_NOISE_SQUASHING_PARAM_MESSAGE_2_CARRY_2_KS_PBS_
// TUNIFORM_2M128: k = 2, N = 2048, base 2^24, 3 levels, native u128, u64 input LWE of dimension 918;
// shortint/parameters/v1_4/noise_squashing/p_fail_2_minus_128/mod.rs:8-19).  Reference paths relative to
// /root/reference/tfhe/src/core_crypto:
//   programmable_bootstrap_f128_lwe_ciphertext, fft_impl/fft128_u128/crypto/bootstrap.rs:60-247 (blind_rotate_assign_split,
//   blind_rotate_u128), fft_impl/fft128_u128/crypto/ggsw.rs (add_external_product_assign_split, cmux_split,
//   collect_next_term_split_scalar :517-567), commons/math/decomposition/decomposer.rs:156-185 + iter.rs:131-151.
//
// The reference multiplies with a double-double FFT.  Here every product is exact: the decomposed digits are small
// (|d| <= 2^(B-1)), so each 128-bit key coefficient g is split into limbs g = sum_j g_j 2^(w j), 0 <= g_j < 2^w, with w
// the largest width for which a whole column sum of limb products stays below p / 2 (p = 2^64 - 2^32 + 1):
//   R N 2^(B-1) (2^w - 1) <= (p - 1) / 2,  R = (k + 1) level            (mi_pbs128_limb_plan; w = 25, 6 limbs at the
// production shape).  A limb product read back from the Goldilocks transform is then the integer itself (centered
// lift), and sum_j y_j 2^(w j) mod 2^128 is the reference's product with its transform error removed.
//
// MI355X design: the structure of pbs_large.hip.  The accumulators of a chunk of ciphertexts live in HBM and one
// external product is five streaming passes over the whole chunk, the launch count per step independent of the batch:
//   decompose : k + 1 u128 polynomials -> R digit polynomials as canonical residues (negative d = p - |d|), least
//               significant level first, row r = level_index (k + 1) + polynomial  -> digits [b][R][N]
//               (blind rotation: ct1 = X^a acc - acc read straight from acc, as large_rotate_decompose)
//   forward   : the plan's transform over all chunk x R digit polynomials
//   mac       : y[b][c][j] = sum_r digits[b][r] . key[r][c][j] mod p; each digit is read once, the (k + 1) n_limbs sums
//               of a coefficient stay in registers, the step's GGSW is shared by the chunk
//   inverse   : the plan's transform over chunk x (k + 1) x n_limbs (N^-1 is folded into the prepared key)
//   recombine : out += sum_j centered(y_j) 2^(w j) mod 2^128, two-word wrapping arithmetic, 16-byte accesses
// A mask element that switches to 0 gives ct1 = 0 and an exactly zero contribution, so every item runs every step; the
// reference's skip (bootstrap.rs:100) changes no value.
//
// Out of scope here: non-native power-of-two moduli below 2^128 (the closest_representable step of blind_rotate_u128,
// bootstrap.rs:217-231), u32 / u128 input LWEs, a LUT index per item, the C++ mirror, the
// serialised Fourier128LweBootstrapKey format (transform output of the reference's own FFT: no meaning here), and fusing
// the passes (mac into the transforms is the follow-up).  The noise-squashing packing keyswitch (base_log 61 over u128)
// is packing_keyswitch128.hip; the multi-bit 128-bit bootstrap is pbs128_multi_bit.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "scratch.hpp"
#include "pbs128_device.hpp"

namespace mi {
namespace pbs128 {

// key preparation, first half: limb j of every coefficient of `n_polys` standard-domain u128 polynomials,
// dst[(poly n_limbs + j) N + e] = (g >> (w j)) mod 2^w
__global__ __launch_bounds__(256) void split_key(u64* __restrict__ dst, const u64* __restrict__ src, uint64_t count,
                                                 Shape sh) {
  const u64 mask = ((u64)1 << sh.limb_bits) - 1;
  for (uint64_t i = grid_stride_start(); i < count; i += grid_stride()) {
    const uint64_t poly = i >> sh.logn, e = i & (sh.n - 1);
    const u128 g = ld128(src, i);
    u64* o = dst + ((poly * sh.n_limbs) << sh.logn) + e;
    for (uint32_t j = 0; j < sh.n_limbs; ++j) o[(uint64_t)j << sh.logn] = (u64)(g >> (sh.limb_bits * j)) & mask;
  }
}

// external product / CMUX input: CMUX first writes glwe -= out back (ct1 = ct1 - ct0, cmux_split), then both
// decompose glwe into digits[b][li (k + 1) + c][N]
template <bool CMUX>
__global__ __launch_bounds__(256) void glwe_decompose(u64* __restrict__ digits, u64* __restrict__ glwe,
                                                      const u64* __restrict__ out, uint32_t batch, Shape sh) {
  const uint64_t per = (uint64_t)(sh.k + 1) * sh.n, total = per * batch;
  for (uint64_t i = grid_stride_start(); i < total; i += grid_stride()) {
    const uint64_t b = i / per, ce = i % per;
    u128 x = ld128(glwe, i);
    if (CMUX) {
      x -= ld128(out, i);
      st128(glwe, i, x);
    }
    decompose_store(x, digits + b * sh.level * per + ce, per, sh.base_log, (int)sh.level);
  }
}

// acc[b] = src / X^ms(body) (polynomial_wrapping_monic_monomial_div_assign_split, bootstrap.rs:82-91); src =
// the shared LUT (src_stride 0) or the item's own accumulator
__global__ __launch_bounds__(256) void init_acc(u64* __restrict__ acc, const u64* __restrict__ src, uint64_t src_stride,
                                                const u64* __restrict__ lwe_in, const u64* __restrict__ corr,
                                                uint32_t n_lwe, int pre, uint32_t batch, Shape sh) {
  const uint64_t per = (uint64_t)(sh.k + 1) * sh.n, total = per * batch;
  for (uint64_t i = grid_stride_start(); i < total; i += grid_stride()) {
    const uint64_t b = i / per, ce = i % per;
    const uint32_t c = (uint32_t)(ce >> sh.logn), m = (uint32_t)(ce & (sh.n - 1));
    const u64 raw = lwe_in[b * (n_lwe + 1) + n_lwe] + (corr ? corr[b] : 0);
    const Monomial xb(switched(raw, sh.logn + 1, pre), sh.logn);
    u128 v = ld128(src, b * src_stride + (uint64_t)c * sh.n + xb.div_src(m, sh.n));
    if (xb.div_neg(m, sh.n)) v = (u128)0 - v;
    st128(acc, i, v);
  }
}

// step `step` of the blind rotation: ct1 = X^a acc - acc (polynomial_wrapping_monic_monomial_mul_assign_split, then the
// CMUX difference), decomposed into digits[b][li (k + 1) + c][N]
__global__ __launch_bounds__(256) void rotate_decompose(u64* __restrict__ digits, const u64* __restrict__ acc,
                                                        const u64* __restrict__ lwe_in, uint32_t n_lwe, uint32_t step,
                                                        int pre, uint32_t batch, Shape sh) {
  const uint64_t per = (uint64_t)(sh.k + 1) * sh.n, total = per * batch;
  for (uint64_t i = grid_stride_start(); i < total; i += grid_stride()) {
    const uint64_t b = i / per, ce = i % per;
    const uint32_t e = (uint32_t)(ce & (sh.n - 1));
    const Monomial xa(switched(lwe_in[b * (n_lwe + 1) + step], sh.logn + 1, pre), sh.logn);
    const uint64_t base = i - e;  // the polynomial's first coefficient
    u128 v = ld128(acc, base + xa.mul_src(e, sh.n));  // X^a acc
    if (xa.mul_neg(e)) v = (u128)0 - v;
    decompose_store(v - ld128(acc, i), digits + b * sh.level * per + ce, per, sh.base_log, (int)sh.level);
  }
}

// y[b][c][j][e] = sum_r digits[b][r][e] . key[r][c][j][e] mod p over the R = level (k + 1) rows of the step's prepared
// GGSW (N^-1 folded in).  One thread per coefficient and item: each digit is read once and the KP1 * NL sums stay in
// registers.  Grid: x over the coefficients, y over the items.
// One sum of the mac: MacSum (pbs128_device.hpp), the wide form where the KP1 * NL sums of a thread fit.
template <int KP1, int NL>
__global__ __launch_bounds__(256) void mac(u64* __restrict__ y, const u64* __restrict__ digits,
                                           const u64* __restrict__ ggsw, uint32_t batch, Shape sh) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= sh.n) return;
  const uint64_t n = sh.n;
  const uint32_t rows = sh.level * KP1;
  for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {
    const u64* d = digits + (uint64_t)b * rows * n + e;
    MacSum<(KP1 * NL <= 18)> acc[KP1][NL];
    for (uint32_t r = 0; r < rows; ++r) {
      // the digits are read once: non-temporal, so the stream does not evict the GGSW every item re-reads
      const u64 x = __builtin_nontemporal_load(d + (uint64_t)r * n);
      const u64* g = ggsw + (uint64_t)r * KP1 * NL * n + e;
#pragma unroll
      for (int c = 0; c < KP1; ++c)
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[c][j].mac(x, g[(uint64_t)(c * NL + j) * n]);
    }
    u64* o = y + (uint64_t)b * KP1 * NL * n + e;
#pragma unroll
    for (int c = 0; c < KP1; ++c)
#pragma unroll
      for (int j = 0; j < NL; ++j) __builtin_nontemporal_store(acc[c][j].value(), o + (uint64_t)(c * NL + j) * n);
  }
}

// out[b][c][e] += sum_j v_j 2^(w j) mod 2^128, v_j = y[b][c][j][e] taken as v - p when v > (p - 1) / 2 (the exact
// integer limb sum): two-word wrapping arithmetic with explicit carries.  ADD false: out = that sum (the destination of
// the multi-bit step starts from zero)
template <bool ADD>
__global__ __launch_bounds__(256) void recombine(u64* __restrict__ out, const u64* __restrict__ y, uint32_t batch,
                                                 Shape sh) {
  const uint64_t total = (uint64_t)(sh.k + 1) * sh.n * batch;
  for (uint64_t i = grid_stride_start(); i < total; i += grid_stride()) {
    const uint64_t poly = i >> sh.logn, e = i & (sh.n - 1);
    const u64* v = y + ((poly * sh.n_limbs) << sh.logn) + e;
    u64x2 acc = {0, 0};
    if (ADD) acc = *reinterpret_cast<const u64x2*>(out + 2 * i);
    for (uint32_t j = 0; j < sh.n_limbs; ++j) {
      const u64 r = __builtin_nontemporal_load(v + ((uint64_t)j << sh.logn));
      const int64_t sv = (int64_t)(r > (P - 1) / 2 ? r - P : r);  // |sv| < 2^63
      const unsigned s = sh.limb_bits * j;                        // < 128
      u64 tlo, thi;  // the sign-extended sv shifted left by s, mod 2^128
      if (s == 0) {
        tlo = (u64)sv;
        thi = (u64)(sv >> 63);
      } else if (s < 64) {
        tlo = (u64)sv << s;
        thi = (u64)(sv >> (64 - s));
      } else {
        tlo = 0;
        thi = (u64)sv << (s - 64);
      }
      const u64 lo = acc.x + tlo;
      acc.y += thi + (lo < tlo ? 1u : 0u);
      acc.x = lo;
    }
    *reinterpret_cast<u64x2*>(out + 2 * i) = acc;
  }
}

// sample extraction of coefficient 0 (Monomial::extract_*) per mask polynomial, out[k N] = B[0]
__global__ __launch_bounds__(256) void extract(u64* __restrict__ lwe_out, const u64* __restrict__ acc, uint32_t batch,
                                               Shape sh) {
  const uint64_t per = (uint64_t)(sh.k + 1) * sh.n, per_out = (uint64_t)sh.k * sh.n + 1, total = per_out * batch;
  for (uint64_t i = grid_stride_start(); i < total; i += grid_stride()) {
    const uint64_t b = i / per_out, o = i % per_out;
    const uint32_t c = (uint32_t)(o >> sh.logn), j = (uint32_t)(o & (sh.n - 1));  // o = k N gives c = k, j = 0
    const u128 v = ld128(acc, b * per + (uint64_t)c * sh.n + Monomial::extract_src(j, sh.n));
    st128(lwe_out, i, Monomial::extract_neg(j) ? (u128)0 - v : v);
  }
}

template <int KP1>
static hipError_t launch_mac_k(u64* y, const u64* digits, const u64* ggsw, uint32_t nb, const Shape& sh,
                               hipStream_t s) {
  const dim3 grid((sh.n + 255) / 256, std::min<uint32_t>(nb, 65535));
#define MI_MAC128(NL) \
  case NL: hipLaunchKernelGGL((mac<KP1, NL>), grid, dim3(256), 0, s, y, digits, ggsw, nb, sh); break;
  switch (sh.n_limbs) {
    MI_MAC128(1) MI_MAC128(2) MI_MAC128(3) MI_MAC128(4) MI_MAC128(5) MI_MAC128(6) MI_MAC128(7) MI_MAC128(8)
    MI_MAC128(9) MI_MAC128(10) MI_MAC128(11) MI_MAC128(12) MI_MAC128(13) MI_MAC128(14) MI_MAC128(15) MI_MAC128(16)
    default: return hipErrorInvalidValue;
  }
#undef MI_MAC128
  return hipGetLastError();
}

static hipError_t launch_mac(u64* y, const u64* digits, const u64* ggsw, uint32_t nb, const Shape& sh, hipStream_t s) {
  switch (sh.k) {
    case 1: return launch_mac_k<2>(y, digits, ggsw, nb, sh, s);
    case 2: return launch_mac_k<3>(y, digits, ggsw, nb, sh, s);
    case 3: return launch_mac_k<4>(y, digits, ggsw, nb, sh, s);
    default: return hipErrorInvalidValue;
  }
}

// transform, mac, inverse, recombine of `nb` items whose digits are written: out += GGSW (.) (the decomposed input)
static hipError_t product_tail(u64* out, u64* digits, u64* y, const u64* ggsw, uint32_t nb, const Shape& sh,
                               const Ntt128Route& rt, hipStream_t s) {
  const size_t kp1 = sh.k + 1;
  hipError_t e = ntt(true, rt, digits, (size_t)nb * sh.level * kp1, s);
  if (e == hipSuccess) e = launch_mac(y, digits, ggsw, nb, sh, s);
  if (e == hipSuccess) e = ntt(false, rt, y, (size_t)nb * kp1 * sh.n_limbs, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(recombine<true>, dim3(blocks_for((uint64_t)nb * kp1 * sh.n)), dim3(256), 0, s, out, y, nb, sh);
  return hipGetLastError();
}

hipError_t launch_decompose(u64* digits, const u64* glwe, uint32_t nb, const Shape& sh, hipStream_t s) {
  hipLaunchKernelGGL(glwe_decompose<false>, dim3(blocks_for((uint64_t)nb * (sh.k + 1) * sh.n)), dim3(256), 0, s, digits,
                     const_cast<u64*>(glwe), (const u64*)nullptr, nb, sh);
  return hipGetLastError();
}

hipError_t launch_init_acc(u64* acc, const u64* src, uint64_t src_stride, const u64* lwe_in, uint32_t n_lwe,
                           uint32_t nb, const Shape& sh, hipStream_t s) {
  hipLaunchKernelGGL(init_acc, dim3(blocks_for((uint64_t)nb * (sh.k + 1) * sh.n)), dim3(256), 0, s, acc, src, src_stride,
                     lwe_in, (const u64*)nullptr, n_lwe, 0, nb, sh);
  return hipGetLastError();
}

hipError_t launch_recombine_assign(u64* out, const u64* y, uint32_t nb, const Shape& sh, hipStream_t s) {
  hipLaunchKernelGGL(recombine<false>, dim3(blocks_for((uint64_t)nb * (sh.k + 1) * sh.n)), dim3(256), 0, s, out, y, nb,
                     sh);
  return hipGetLastError();
}

hipError_t launch_extract(u64* lwe_out, const u64* acc, uint32_t nb, const Shape& sh, hipStream_t s) {
  hipLaunchKernelGGL(extract, dim3(blocks_for((uint64_t)nb * ((uint64_t)sh.k * sh.n + 1))), dim3(256), 0, s, lwe_out,
                     acc, nb, sh);
  return hipGetLastError();
}

}  // namespace pbs128

size_t pbs128_ggsw_words(const Pbs128Shape& p) {
  return (size_t)p.level * (p.k + 1) * (p.k + 1) * p.n_limbs << p.logn;
}

hipError_t launch_pbs128_key_prepare(uint64_t* dst, const uint64_t* src, size_t n_ggsw, const Pbs128Shape& p,
                                     const Ntt128Route& rt, hipStream_t s) {
  using namespace pbs128;
  const Shape sh = shape_of(p);
  const size_t polys = (size_t)p.level * (p.k + 1) * (p.k + 1), words = pbs128_ggsw_words(p);
  // GGSW by GGSW, straight into its place in the prepared key: limbs, the forward transform in place, N^-1
  for (size_t g = 0; g < n_ggsw; ++g) {
    u64* d = dst + g * words;
    const uint64_t count = (uint64_t)polys << p.logn;
    hipLaunchKernelGGL(split_key, dim3(blocks_for(count)), dim3(256), 0, s, d, src + 2 * g * count, count, sh);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = ntt(true, rt, d, polys * p.n_limbs, s);
    if (e == hipSuccess) e = launch_scale(d, d, words, rt.n_inv, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ext_product128(bool cmux, uint64_t* out, uint64_t* glwe, const uint64_t* ggsw, size_t batch,
                                 const Pbs128Shape& p, const Ntt128Route& rt, hipStream_t s) {
  using namespace pbs128;
  if (batch == 0) return hipSuccess;
  const Shape sh = shape_of(p);
  const size_t per = (size_t)(p.k + 1) * sh.n, chunk = chunk_size(sh, batch, false);
  u64* scratch = nullptr;
  hipError_t e = mi::scratch_alloc((void**)&scratch, chunk * item_words(sh, false) * sizeof(u64), s);
  if (e != hipSuccess) return e;
  u64* digits = scratch;
  u64* y = digits + chunk * sh.level * per;
  for (size_t b0 = 0; b0 < batch && e == hipSuccess; b0 += chunk) {
    const uint32_t nb = (uint32_t)std::min(chunk, batch - b0);
    u64* o = out + 2 * b0 * per;
    u64* g = glwe + 2 * b0 * per;
    const dim3 grid(blocks_for((uint64_t)nb * per));
    if (cmux) hipLaunchKernelGGL(glwe_decompose<true>, grid, dim3(256), 0, s, digits, g, o, nb, sh);
    else hipLaunchKernelGGL(glwe_decompose<false>, grid, dim3(256), 0, s, digits, g, o, nb, sh);
    e = hipGetLastError();
    if (e == hipSuccess) e = product_tail(o, digits, y, ggsw, nb, sh, rt, s);
  }
  const hipError_t ef = mi::scratch_free(scratch, s);
  return e != hipSuccess ? e : ef;
}

hipError_t launch_blind_rotate128(uint64_t* lwe_out, uint64_t* acc_glwe, const uint64_t* lut, const uint64_t* lwe_in,
                                  const uint64_t* key, size_t n_lwe, size_t batch, int centered, int pre,
                                  const Pbs128Shape& p, const Ntt128Route& rt, hipStream_t s) {
  using namespace pbs128;
  if (batch == 0) return hipSuccess;
  const Shape sh = shape_of(p);
  const size_t per = (size_t)(p.k + 1) * sh.n, chunk = chunk_size(sh, batch, true);
  const size_t ggsw_words = pbs128_ggsw_words(p), per_out = (size_t)p.k * sh.n + 1;
  u64* scratch = nullptr;
  hipError_t e = mi::scratch_alloc((void**)&scratch, chunk * item_words(sh, true) * sizeof(u64), s);
  if (e != hipSuccess) return e;
  u64* acc = scratch;  // u128 accumulators first (16-byte aligned, as the pool's blocks are)
  u64* digits = acc + chunk * 2 * per;
  u64* y = digits + chunk * sh.level * per;
  u64* corr = y + chunk * sh.n_limbs * per;
  // one lane (run_blind_rotation never forks): every L.off is 0 and L.st is s, so the chunk's buffers are the lane's
  auto init = [&](const Lane& L) -> hipError_t {
    const u64 *in = lwe_in + L.b0 * (n_lwe + 1), *src = lut ? lut : acc_glwe + 2 * L.b0 * per;
    const hipError_t e =
        centered ? launch_body_correction(corr, in, (uint32_t)n_lwe, p.logn + 1, L.nb, L.st) : hipSuccess;
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(init_acc, dim3(blocks_for((uint64_t)L.nb * per)), dim3(256), 0, L.st, acc, src,
                       (uint64_t)(lut ? 0 : per), in, centered ? corr : (const u64*)nullptr, (uint32_t)n_lwe, pre, L.nb,
                       sh);
    return hipGetLastError();
  };
  auto step = [&](const Lane& L, uint32_t i) -> hipError_t {
    hipLaunchKernelGGL(rotate_decompose, dim3(blocks_for((uint64_t)L.nb * per)), dim3(256), 0, L.st, digits, acc,
                       lwe_in + L.b0 * (n_lwe + 1), (uint32_t)n_lwe, i, pre, L.nb, sh);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : product_tail(acc, digits, y, key + (size_t)i * ggsw_words, L.nb, sh, rt, L.st);
  };
  auto finish = [&](const Lane& L) -> hipError_t {
    if (!lwe_out)
      return hipMemcpyAsync(acc_glwe + 2 * L.b0 * per, acc, (size_t)L.nb * per * 2 * sizeof(u64),
                            hipMemcpyDeviceToDevice, L.st);
    hipLaunchKernelGGL(extract, dim3(blocks_for((uint64_t)L.nb * per_out)), dim3(256), 0, L.st,
                       lwe_out + 2 * L.b0 * per_out, acc, L.nb, sh);
    return hipGetLastError();
  };
  e = run_blind_rotation(batch, chunk, (uint32_t)n_lwe, 1, s, init, step, finish);
  const hipError_t ef = mi::scratch_free(scratch, s);
  return e != hipSuccess ? e : ef;
}

}  // namespace mi
