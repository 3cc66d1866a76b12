// pbs128_multi_bit.hip — the exact multi-bit 128-bit programmable bootstrap on the Goldilocks NTT (shortint's noise
// squashing under a multi-bit key, V1_3_NOISE_SQUASHING_PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_
// 2M128: k = 2, N = 2048, base 2^23, 3 levels, grouping factor 4, native u128;
// shortint/parameters/v1_3/noise_squashing/p_fail_2_minus_128/mod.rs:65-77).  Reference: tfhe/src/core_crypto/
// algorithms/lwe_multi_bit_programmable_bootstrapping.rs:
//   multi_bit_programmable_bootstrap_f128_lwe_ciphertext, multi_bit_f128_deterministic_blind_rotate_assign,
//   prepare_multi_bit_fourier_128_ggsw_mem_optimized  :2257-2700 (the std_* forms, bundle in the standard domain,
//   :1849-2255); modulus_switch_multi_bit :30-51, selection_bit :55-65.
//
// The key is (n / g) groups of 2^g GGSWs over u128; GGSW idx of group i encrypts prod_m (s[i g + m] XOR NOT bit_m(idx)),
// bit_m(idx) = (idx >> (g - 1 - m)) & 1 (the layout of fft64_multi_bit.hip).  One step handles the g mask elements of a
// group:
//   d_idx  = modulus_switch(wrapping sum of the mask elements idx selects, log2(2N))      idx = 1 .. 2^g - 1
//   bundle = G_0 + sum_idx X^(d_idx) G_idx                                                 mod 2^128
//   acc    = 0 + bundle (.) acc                                                            (not a CMUX)
//
// Exactness.  The reference multiplies with a double-double FFT; here, as in pbs128.hip, the key coefficients are split
// into limbs and the products run on the Goldilocks transform.  X^d is a pointwise factor there: the plan's forward
// transform is y[j] = sum_i x_i psi^((2 bitrev(j) + 1) i), so slot j of X^d x is psi^((2 bitrev(j) + 1) d mod 2N) y[j].
// The bundle is never formed:
//   bundle (.) acc = sum_idx sum_r (digit_r X^(d_idx)) G_idx,r
// is the classic mac over 2^g R rows, R = (k + 1) level, whose digit stream is multiplied by the phase.  digit_r X^d
// has the digit's coefficients (|d| <= 2^(B-1)) at other places and signs, so a whole column sum of limb products stays
// inside (-p/2, p/2) as long as
//   2^g R N 2^(B-1) (2^w - 1) <= (p - 1) / 2          (mi_pbs128_multi_bit_limb_plan; w = 22, 6 limbs at the shape above)
// and is read back as the integer it is.  That width is up to 4 bits below the classic one, so where the classic key
// stops at 16 limbs (w >= 8) this one goes on to 32 (w >= 4): every shape that has a classic key has a multi-bit one.
//
// MI355X design: the passes of pbs128.hip over a chunk of accumulators held in HBM, per step
//   decompose : acc itself -> R digit polynomials per item (pbs128.hip glwe_decompose<false>)
//   forward   : the plan's transform over chunk x R
//   mac       : multi_bit_mac below: y[b][c][j] = sum_idx sum_r (digits[b][r] ph_idx) K_idx[r][c][j]
//   inverse   : the plan's transform over chunk x (k + 1) x n_limbs (N^-1 is folded into the prepared key)
//   recombine : acc = sum_j centered(y_j) 2^(w j) mod 2^128 (pbs128.hip recombine<false>: it overwrites)
// init_acc (the division by X^body) and extract are pbs128.hip's.
//
// Out of scope: non-native moduli, a LUT index per item, the C++ mirror, the serialised
// Fourier128LweMultiBitBootstrapKey format (transform output of the reference's own FFT: no meaning here).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "scratch.hpp"
#include "pbs128_device.hpp"

namespace mi {
namespace pbs128 {

// The mac of one multi-bit step.  One thread per coefficient (slot) e and item b; grid: x over the slots, y over the
// items.  The group's 2^G prepared GGSWs are contiguous at `grp` (ggsw_words apart) and shared by the whole chunk; only
// the degrees are the item's.  Per GGSW idx the degree d_idx is the standard switch of the wrapping sum of the mask
// elements idx selects (uniform per item: scalar), the phase of this slot is roots[(2 bitrev(e) + 1) d_idx mod 2N]
// (roots = the 2N powers of psi; ph_0 = 1), and the R digit rows times that phase run through the classic mac against
// K_idx.  The digits are re-read per GGSW (R words against the R (k + 1) n_limbs key words of that GGSW) so that neither
// the 2^G - 1 phases nor a phased digit stream are held: the KP1 * NL sums of a thread stay in registers throughout.
// NL = the limbs a thread sums.  PART false: all n_limbs = NL of them.  PART true (n_limbs above 16: the multi-bit
// width is up to 4 bits narrower than the classic one): grid z cuts the limbs into parts of NL, thread z sums limbs
// [z NL, min((z + 1) NL, n_limbs)), so that no thread holds more than 16 sums per polynomial.
template <int KP1, int NL, int G, bool PART>
__global__ __launch_bounds__(256) void multi_bit_mac(u64* __restrict__ y, const u64* __restrict__ digits,
                                                     const u64* __restrict__ grp, uint64_t ggsw_words,
                                                     const u64* __restrict__ roots, const u64* __restrict__ lwe_in,
                                                     uint32_t n_lwe, uint32_t group, uint32_t batch, Shape sh) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= sh.n) return;
  const uint64_t n = sh.n;
  const uint32_t rows = sh.level * KP1, mask2n = 2u * sh.n - 1u;
  const uint32_t nl = PART ? sh.n_limbs : NL, j0 = PART ? blockIdx.z * NL : 0;  // this thread's limbs: j0 + [0, NL)
  const uint32_t slot = 2u * (__brev(e) >> (32u - sh.logn)) + 1u;  // the exponent of psi this slot evaluates at
  for (uint32_t b = blockIdx.y; b < batch; b += gridDim.y) {
    const u64* d = digits + (uint64_t)b * rows * n + e;
    const u64* a = lwe_in + (uint64_t)b * (n_lwe + 1) + (uint64_t)group * G;
    MacSum<(KP1 * NL <= 18)> acc[KP1][NL];
#pragma unroll 1
    for (uint32_t idx = 0; idx < (1u << G); ++idx) {
      // modulus_switch_multi_bit: the switch of the sum, not the sum of switches; bit G - 1 - m of idx selects element m
      u64 sum = 0;
#pragma unroll
      for (int m = 0; m < G; ++m)
        if ((idx >> (G - 1 - m)) & 1u) sum += a[m];
      const uint32_t deg = switched(sum, sh.logn + 1, 0);
      const u64 ph = roots[(deg * slot) & mask2n];  // idx = 0: deg = 0, roots[0] = 1, and the multiply is skipped
      const u64* kg = grp + (uint64_t)idx * ggsw_words + (uint64_t)j0 * n + e;
#pragma unroll 1
      for (uint32_t r = 0; r < rows; ++r) {
        u64 x = d[(uint64_t)r * n];
        if (idx != 0) x = Goldilocks::mul(x, ph);
        const u64* g = kg + (uint64_t)r * KP1 * nl * n;
#pragma unroll
        for (int c = 0; c < KP1; ++c)
#pragma unroll
          for (int j = 0; j < NL; ++j)
            if (!PART || j0 + j < nl) acc[c][j].mac(x, g[((uint64_t)c * nl + j) * n]);
      }
    }
    u64* o = y + ((uint64_t)b * KP1 * nl + j0) * n + e;
#pragma unroll
    for (int c = 0; c < KP1; ++c)
#pragma unroll
      for (int j = 0; j < NL; ++j)
        if (!PART || j0 + j < nl) __builtin_nontemporal_store(acc[c][j].value(), o + ((uint64_t)c * nl + j) * n);
  }
}

struct MacArgs {
  u64* y;
  const u64 *digits, *grp, *roots, *lwe_in;
  uint64_t ggsw_words;
  uint32_t n_lwe, group, nb;
};

template <int KP1, int G>
static hipError_t launch_mac_kg(const MacArgs& a, const Shape& sh, hipStream_t s) {
  const uint32_t parts = (sh.n_limbs + 15) / 16, per_part = (sh.n_limbs + parts - 1) / parts;
  const dim3 grid((sh.n + 255) / 256, std::min<uint32_t>(a.nb, 65535), parts);
#define MI_MAC128MB(NL, PART)                                                                                      \
  hipLaunchKernelGGL((multi_bit_mac<KP1, NL, G, PART>), grid, dim3(256), 0, s, a.y, a.digits, a.grp, a.ggsw_words, \
                     a.roots, a.lwe_in, a.n_lwe, a.group, a.nb, sh);                                               \
  break;
  if (parts == 1) {
    switch (per_part) {
      case 1: MI_MAC128MB(1, false) case 2: MI_MAC128MB(2, false) case 3: MI_MAC128MB(3, false)
      case 4: MI_MAC128MB(4, false) case 5: MI_MAC128MB(5, false) case 6: MI_MAC128MB(6, false)
      case 7: MI_MAC128MB(7, false) case 8: MI_MAC128MB(8, false) case 9: MI_MAC128MB(9, false)
      case 10: MI_MAC128MB(10, false) case 11: MI_MAC128MB(11, false) case 12: MI_MAC128MB(12, false)
      case 13: MI_MAC128MB(13, false) case 14: MI_MAC128MB(14, false) case 15: MI_MAC128MB(15, false)
      case 16: MI_MAC128MB(16, false)
      default: return hipErrorInvalidValue;
    }
  } else if (parts == 2) {  // 17 ... 32 limbs: two parts of 9 ... 16
    switch (per_part) {
      case 9: MI_MAC128MB(9, true) case 10: MI_MAC128MB(10, true) case 11: MI_MAC128MB(11, true)
      case 12: MI_MAC128MB(12, true) case 13: MI_MAC128MB(13, true) case 14: MI_MAC128MB(14, true)
      case 15: MI_MAC128MB(15, true) case 16: MI_MAC128MB(16, true)
      default: return hipErrorInvalidValue;
    }
  } else {
    return hipErrorInvalidValue;
  }
#undef MI_MAC128MB
  return hipGetLastError();
}

template <int G>
static hipError_t launch_mac_g(const MacArgs& a, const Shape& sh, hipStream_t s) {
  switch (sh.k) {
    case 1: return launch_mac_kg<2, G>(a, sh, s);
    case 2: return launch_mac_kg<3, G>(a, sh, s);
    case 3: return launch_mac_kg<4, G>(a, sh, s);
    default: return hipErrorInvalidValue;
  }
}

static hipError_t launch_multi_bit_mac(int g, const MacArgs& a, const Shape& sh, hipStream_t s) {
  switch (g) {
    case 2: return launch_mac_g<2>(a, sh, s);
    case 3: return launch_mac_g<3>(a, sh, s);
    case 4: return launch_mac_g<4>(a, sh, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pbs128

hipError_t launch_multi_bit_blind_rotate128(uint64_t* lwe_out, uint64_t* acc_glwe, const uint64_t* lut,
                                            const uint64_t* lwe_in, const uint64_t* key, const uint64_t* roots,
                                            size_t n_lwe, int grouping_factor, size_t batch, const Pbs128Shape& p,
                                            const Ntt128Route& rt, hipStream_t s) {
  using namespace pbs128;
  if (batch == 0) return hipSuccess;
  if (grouping_factor < 2 || grouping_factor > 4 || n_lwe % (size_t)grouping_factor) return hipErrorInvalidValue;
  const Shape sh = shape_of(p);
  const size_t kp1 = (size_t)p.k + 1, per = kp1 * sh.n, chunk = chunk_size(sh, batch, true);
  const size_t ggsw_words = pbs128_ggsw_words(p), per_out = (size_t)p.k * sh.n + 1;
  const size_t group_words = ggsw_words << grouping_factor;
  u64* scratch = nullptr;
  hipError_t e = mi::scratch_alloc((void**)&scratch, chunk * item_words(sh, true) * sizeof(u64), s);
  if (e != hipSuccess) return e;
  u64* acc = scratch;  // u128 accumulators first (16-byte aligned, as the pool's blocks are)
  u64* digits = acc + chunk * 2 * per;
  u64* y = digits + chunk * sh.level * per;
  // one lane, as launch_blind_rotate128: every L.off is 0 and L.st is s, so the chunk's buffers are the lane's
  auto init = [&](const Lane& L) -> hipError_t {
    return launch_init_acc(acc, lut ? lut : acc_glwe + 2 * L.b0 * per, (uint64_t)(lut ? 0 : per),
                           lwe_in + L.b0 * (n_lwe + 1), (uint32_t)n_lwe, L.nb, sh, L.st);
  };
  auto step = [&](const Lane& L, uint32_t i) -> hipError_t {
    hipError_t e = launch_decompose(digits, acc, L.nb, sh, L.st);
    if (e == hipSuccess) e = ntt(true, rt, digits, (size_t)L.nb * sh.level * kp1, L.st);
    if (e == hipSuccess)
      e = launch_multi_bit_mac(grouping_factor,
                               MacArgs{y, digits, key + (size_t)i * group_words, roots, lwe_in + L.b0 * (n_lwe + 1),
                                       ggsw_words, (uint32_t)n_lwe, i, L.nb},
                               sh, L.st);
    if (e == hipSuccess) e = ntt(false, rt, y, (size_t)L.nb * kp1 * sh.n_limbs, L.st);
    if (e == hipSuccess) e = launch_recombine_assign(acc, y, L.nb, sh, L.st);
    return e;
  };
  auto finish = [&](const Lane& L) -> hipError_t {
    if (!lwe_out)
      return hipMemcpyAsync(acc_glwe + 2 * L.b0 * per, acc, (size_t)L.nb * per * 2 * sizeof(u64),
                            hipMemcpyDeviceToDevice, L.st);
    return launch_extract(lwe_out + 2 * L.b0 * per_out, acc, L.nb, sh, L.st);
  };
  e = run_blind_rotation(batch, chunk, (uint32_t)(n_lwe / (size_t)grouping_factor), 1, s, init, step, finish);
  const hipError_t ef = mi::scratch_free(scratch, s);
  return e != hipSuccess ? e : ef;
}

}  // namespace mi
