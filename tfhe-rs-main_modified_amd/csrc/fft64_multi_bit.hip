// fft64_multi_bit.hip — the multi-bit programmable bootstrap of tfhe core_crypto on the one-wave N = 2048 f64-FFT
// engine (fft64_engine.hpp).  Reference paths relative to /root/reference/tfhe/src/core_crypto:
//   selection_bit / modulus_switch_multi_bit   algorithms/lwe_multi_bit_programmable_bootstrapping.rs:30-65
//   prepare_multi_bit_ggsw_mem_optimized       algorithms/lwe_multi_bit_programmable_bootstrapping.rs:115-154
//   multi_bit_deterministic_blind_rotate_assign  algorithms/lwe_multi_bit_programmable_bootstrapping.rs:644-869
//   incomplete_monomial_forward_as_integer     fft_impl/fft64/math/fft/mod.rs:436-473
//   update_with_fmadd_factor                   fft_impl/fft64/crypto/ggsw.rs:700-755
//
// The key is (n / g) groups of 2^g Fourier GGSWs; GGSW idx of group i encrypts prod_m (s[i g + m] XOR NOT bit_m(idx)),
// bit_m(idx) = (idx >> (g - 1 - m)) & 1.  One blind-rotation step handles the g mask elements of a group:
//   d_idx  = modulus_switch(wrapping sum of the mask elements idx selects, log2(2N))      idx = 1 .. 2^g - 1
//   bundle = G_0 + sum_idx G_idx X^(d_idx)                                                (Fourier domain)
//   acc    = 0 + bundle (.) acc                                                            (not a CMUX)
// so a bootstrap runs n / g external products where the classic one runs n CMUXes.
//
// The step here: the accumulator is decomposed and transformed as in ext_product_add; the bundle is never stored: as
// each position's key elements arrive they are combined in registers, bundle[e] = G_0[e] + sum_idx G_idx[e] ph_idx,
// and fed to the multiply-accumulate.  The 2^g key GGSWs are the same for every item; only the phases ph_idx are per
// item.
//
// Phases.  X^d at frequency f is zeta^(d (1 - 4 f) mod 2N), zeta = exp(i pi / N).  Position (lane L, register R) holds
// f = f6(L) + 64 R (low6_frequency), so the exponent is d (1 - 4 f6(L)) - 256 d R: one lookup per (idx, lane) in the
// plan's table of the 2N roots zeta^j (64 KiB, `roots`), then across the 16 registers one complex multiply by
// zeta^(-256 d R) = W16^(d R mod 16), a wave-uniform 16th root read from constant memory.  The degrees are uniform per
// wave (one ciphertext per K + 1 waves) and computed once per step from the LWE mask.
//
// After the decomposition the old accumulator is dead (the destination starts at zero), so its registers hold the
// phases and the product during the step: the k = 1, level-1 kernel keeps the classic kernel's 2 waves per SIMD, four
// ciphertexts per workgroup (idle waves of a ragged last workgroup still take part in the barriers).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft64_decomp.hpp"
#include "fft64_device.hpp"
#include "fft64_engine.hpp"
#include "fft64_launch.hpp"

namespace mi {
namespace fft {

// W16^j = exp(-2 pi i j / 16)
__device__ __forceinline__ cplx w16(uint32_t j) {
  static constexpr double T[16][2] = {{1.0, 0.0},  {C8, -S8},  {R2, -R2},  {S8, -C8},  {0.0, -1.0}, {-S8, -C8},
                                      {-R2, -R2},  {-C8, -S8}, {-1.0, 0.0}, {-C8, S8},  {-R2, R2},   {-S8, C8},
                                      {0.0, 1.0},  {S8, C8},   {R2, R2},   {C8, S8}};
  return {T[j & 15u][0], T[j & 15u][1]};
}

// modulus_switch_multi_bit: d[idx - 1] for idx = 1 .. 2^G - 1 from the group's G mask elements (wave-uniform).  The
// switch is applied to the wrapping sum, not to each element.
template <int G>
__device__ __forceinline__ void group_degrees(uint32_t (&d)[(1 << G) - 1], const u64* __restrict__ mask) {
  constexpr unsigned LOG_MOD = 12;  // PolynomialSize(2048)::to_blind_rotation_input_modulus_log
  u64 a[G], sum[1 << G];
#pragma unroll
  for (int m = 0; m < G; ++m) a[m] = mask[m];
  sum[0] = 0;
#pragma unroll
  for (int idx = 1; idx < (1 << G); ++idx) {
    const int p = __builtin_ctz(idx);  // bit p of idx selects mask element G - 1 - p
    sum[idx] = sum[idx & (idx - 1)] + a[G - 1 - p];
    d[idx - 1] = __builtin_amdgcn_readfirstlane((uint32_t)modulus_switch(sum[idx], LOG_MOD) & (2u * N - 1u));
  }
}

// One multi-bit step on registers: acc <- from_torus(bundle (.) acc).  Wave w (< K + 1) owns GLWE polynomial w; `grp`
// = the group's 2^G GGSWs, each level x (K+1) x (K+1) x M complex in the Fourier layout, highest level first; `mask`
// the group's G LWE mask elements; `roots` the 2N roots zeta^j.  pair / t1 / t2 / ps as ext_product_add.
template <int K, bool L1, bool WGB, int G>
__device__ __forceinline__ void multi_bit_step(u64 (&acc)[NPL], const cplx* __restrict__ grp,
                                               const u64* __restrict__ mask, const cplx* __restrict__ roots,
                                               int base_log, int level, cplx* pair, const cplx* t1, const cplx* t2,
                                               const cplx* cm, const cplx* cmi, int w, int lane,
                                               PairSync<K, WGB>& ps) {
  constexpr int NI = (1 << G) - 1;
  uint32_t d[NI];
  group_degrees<G>(d, mask);
  const uint32_t c0 = (1u - 4u * (uint32_t)low6_frequency(lane)) & (2u * N - 1u);

  cplx* buf = pair + w * BUF;
  const size_t ggsw_len = (size_t)level * (K + 1) * (K + 1) * M;
  u64 st[L1 ? 1 : NPL];
  if (!L1) {
#pragma unroll
    for (int r = 0; r < NPL; ++r) st[r] = decomp_init_native(acc[r], base_log, level);
  }
  cplx y[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) y[r] = {0.0, 0.0};
#pragma unroll 1
  for (int li = 0; li < (L1 ? 1 : level); ++li) {
    cplx u[16];
    if (L1) {
      if (base_log <= 31) {  // uniform: digits from the high words, exact in int32
#pragma unroll
        for (int m = 0; m < 16; ++m)
          u[m] = {(double)decompose_l1_hi((uint32_t)(acc[m] >> 32), base_log),
                  (double)decompose_l1_hi((uint32_t)(acc[m + 16] >> 32), base_log)};
      } else {
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          u64 s0 = decomp_init_native(acc[m], base_log, 1), s1 = decomp_init_native(acc[m + 16], base_log, 1);
          const u64 d0 = decompose_one_level(base_log, s0), d1 = decompose_one_level(base_log, s1);
          u[m] = {s64_to_f64(d0), s64_to_f64(d1)};
        }
      }
    } else {
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const u64 d0 = decompose_one_level(base_log, st[m]), d1 = decompose_one_level(base_log, st[m + 16]);
        u[m] = {s64_to_f64(d0), s64_to_f64(d1)};
      }
    }
    fft_fwd(u, buf, t1, t2, cm, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) buf[r * 64 + lane] = u[r];
    // ph[i] = zeta^(d_i (1 - 4 f6(lane))): the phase of register 0 (looked up after the transform, whose registers
    // it would otherwise crowd)
    cplx ph[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) ph[i] = roots[(d[i] * c0) & (2u * N - 1u)];
    // The decomposition yields the least significant level first, which every GGSW stores first; this wave reads
    // column w of each.  The key is read in units of IC GGSWs x (K + 1) rows at one register position, each unit issued
    // DEPTH units ahead of its use (the first ones before the exchange barrier, so their latency overlaps the wait).
    // The scheduler, left alone, hoists every load and phase of the step and sinks every product, and spills; the
    // empty asm statements hold the order: a unit's load offset, its phases and the values it leaves (`tie`) each pass
    // through one at the place the unit belongs, and volatile statements keep their order.
    const char* mat = reinterpret_cast<const char*>(grp + (size_t)li * (K + 1) * (K + 1) * M);
    uint32_t voff = (uint32_t)(w * M + lane) * (uint32_t)sizeof(cplx);  // this lane's byte offset in a GGSW row
    constexpr int NG = 1 << G, IC = 4, CH = NG / IC, UNITS = 16 * CH;
    constexpr int DEPTH = G == 2 ? 2 : 1;  // deeper ones spill at the 256 VGPRs of the k = 1, level-1 kernel
    cplx kb[DEPTH + 1][IC][K + 1];
    auto load_unit = [&](int t, cplx(&dst)[IC][K + 1]) {
      const int r = t / CH, c = t % CH;
#pragma unroll
      for (int j = 0; j < IC; ++j)
#pragma unroll
        for (int rr = 0; rr <= K; ++rr)
          dst[j][rr] = *reinterpret_cast<const cplx*>(
              mat + ((size_t)(c * IC + j) * ggsw_len + (size_t)rr * (K + 1) * M + r * 64) * sizeof(cplx) + voff);
    };
    auto tie = [](cplx& z) { asm volatile("" : "+v"(z.re), "+v"(z.im)); };
#pragma unroll
    for (int t = 0; t < DEPTH; ++t) load_unit(t, kb[t]);
    ps.sync();
    cplx bun[K + 1];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int c = 0; c < CH; ++c) {  // unit t = (r, c); two short loops, so that both unroll before the arrays are split
      const int t = r * CH + c;
      asm volatile("" : "+v"(voff) : : "memory");
      if (t + DEPTH < UNITS) load_unit(t + DEPTH, kb[(t + DEPTH) % (DEPTH + 1)]);
      const cplx(&kt)[IC][K + 1] = kb[t % (DEPTH + 1)];
#pragma unroll
      for (int j = 0; j < IC; ++j) {
        const int idx = c * IC + j;
        if (idx == 0) {  // G_0 is not rotated
#pragma unroll
          for (int rr = 0; rr <= K; ++rr) bun[rr] = kt[0][rr];
          continue;
        }
        tie(ph[idx - 1]);
        const cplx p = r == 0 ? ph[idx - 1] : cmul(ph[idx - 1], w16(d[idx - 1] * (uint32_t)r));
#pragma unroll
        for (int rr = 0; rr <= K; ++rr) bun[rr] = cfma(kt[j][rr], p, bun[rr]);
      }
      if (c == CH - 1) {
        cplx a = y[r];
#pragma unroll
        for (int rr = 0; rr <= K; ++rr) a = cfma(pair[rr * BUF + r * 64 + lane], bun[rr], a);
        y[r] = a;
        tie(y[r]);
      } else {
#pragma unroll
        for (int rr = 0; rr <= K; ++rr) tie(bun[rr]);
      }
    }
    ps.sync();
  }
  fft_inv(y, buf, t1, t2, cmi, lane);
#pragma unroll
  for (int m = 0; m < 16; ++m) {  // the destination starts at zero: convert_add_backward_torus into 0
    acc[m] = 0;
    acc[m + 16] = 0;
    add_torus(acc[m], y[m].re);
    add_torus(acc[m + 16], y[m].im);
  }
}

// The two ends of a bootstrap, which do not depend on the rotation.  They restate pbs_body's (fft64_pbs.hip), which
// keeps its own text so that the classic kernels compile to the same code as before this file existed.
// acc = the polynomial `lp` / X^body (polynomial_wrapping_monic_monomial_div), coefficient lane + 64 r, body < 2N
__device__ __forceinline__ void lut_div_monomial(u64 (&acc)[NPL], const u64* __restrict__ lp, u64 body, int lane) {
  const int full = (int)(body / N) & 1, rem = (int)(body % N);
#pragma unroll
  for (int r = 0; r < NPL; ++r) {
    const int m = lane + 64 * r;  // div: new[m] = old[(m + rem) % N], negated for m >= N - rem
    u64 v = lp[(m + rem) & (N - 1)];
    if (full ^ (m >= N - rem)) v = (u64)0 - v;
    acc[r] = v;
  }
}

// The end of a bootstrap: wave w's polynomial `acc` of item b goes out as the rotated GLWE (io.glwe_out) or as its part
// of sample 0 (extract_lwe_sample_from_glwe_ciphertext, glwe_sample_extraction.rs:89-160, nth = 0) through `mine`, the
// wave's LDS buffer of N u64.
template <int K>
__device__ __forceinline__ void store_pbs_result(u64* __restrict__ lwe_out, const PbsIo& io, const u64 (&acc)[NPL],
                                                 u64* mine, uint32_t b, int w, int lane, bool valid) {
  if (io.glwe_out) {  // the rotated accumulator (the LUT was divided by X^body before the loop)
    if (valid) {
      u64* g = io.glwe_out + ((size_t)b * (K + 1) + w) * N;
#pragma unroll
      for (int r = 0; r < NPL; ++r) g[lane + 64 * r] = acc[r];
    }
    return;
  }
  u64* out = lwe_out + (size_t)b * (K * N + 1);
  if (w < K) {
#pragma unroll
    for (int r = 0; r < NPL; ++r) mine[lane + 64 * r] = acc[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (valid) {
#pragma unroll
      for (int r = 0; r < NPL; ++r) {
        const int j = lane + 64 * r;
        out[(size_t)w * N + j] = (j == 0) ? mine[0] : (u64)0 - mine[N - j];
      }
    }
  } else if (lane == 0 && valid) {
    out[(size_t)K * N] = acc[0];
  }
}

// lwe_in: batch x (n + 1), native, switched here with the standard switch; fbsk: (n / G) x 2^G x level x (K+1) x (K+1)
// x M complex; io and the outputs as pbs_body.  No group is skipped and nothing is subtracted.
template <int K, bool L1, int CT, int G>
__device__ __forceinline__ void multi_bit_body(u64* __restrict__ lwe_out, const u64* __restrict__ lwe_in,
                                               const PbsIo& io, const cplx* __restrict__ fbsk,
                                               const cplx* __restrict__ roots, uint32_t n_lwe, uint32_t batch,
                                               int base_log, int level, const Tables& tb, Wg<K, CT>& wg) {
  constexpr unsigned LOG_MOD = 12;
  load_tables(wg, tb);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ct = wave / (K + 1), w = wave % (K + 1);
  const uint32_t b0 = blockIdx.x * CT + ct;
  const uint32_t b = b0 < batch ? b0 : batch - 1;
  const u64* lut = io.lut_for(b, (uint64_t)(K + 1) * N);
  const bool valid = b0 < batch && lut;  // every wave takes part in the barriers
  if (!lut) lut = io.lut;
  const u64* lwe = lwe_in + (size_t)b * (n_lwe + 1);
  const size_t group_len = ((size_t)level * (K + 1) * (K + 1) * M) << G;
  cplx* pair = wg.bufs + ct * (K + 1) * BUF;
  u64* mine = reinterpret_cast<u64*>(pair + w * BUF);

  u64 acc[NPL];
  lut_div_monomial(acc, lut + (size_t)w * N, modulus_switch(lwe[n_lwe], LOG_MOD), lane);
  // Every workgroup form meets at the workgroup barrier: the ciphertexts of a workgroup then read the same key lines at
  // the same time and share them in the CU's L1 (a step reads 2^G GGSWs, not one; with PairSync's pairwise counters
  // each ciphertext drifts and streams the key from L2 on its own: 55.1 against 28.4 ms per batch of 4096 at g = 3).
  PairSync<K, true> ps{wg.flags + ct * (K + 1), w, 0u};
  const uint32_t groups = n_lwe / G;
  for (uint32_t i = 0; i < groups; ++i)
    multi_bit_step<K, L1, true, G>(acc, fbsk + (size_t)i * group_len, lwe + (size_t)i * G, roots, base_log, level,
                                      pair, wg.t1, wg.t2, wg.cm, wg.cmi, w, lane, ps);
  store_pbs_result<K>(lwe_out, io, acc, mine, b, w, lane, valid);
}

template <int K, bool L1, int G>
__global__ __launch_bounds__(64 * (K + 1)) void multi_bit_kernel(u64* __restrict__ lwe_out,
                                                                 const u64* __restrict__ lwe_in, PbsIo io,
                                                                 const cplx* __restrict__ fbsk,
                                                                 const cplx* __restrict__ roots, uint32_t n_lwe,
                                                                 uint32_t batch, int base_log, int level, Tables tb) {
  __shared__ Wg<K, 1> wg;
  multi_bit_body<K, L1, 1, G>(lwe_out, lwe_in, io, fbsk, roots, n_lwe, batch, base_log, level, tb, wg);
}
template <int G>
__global__ __launch_bounds__(128 * CT_FAST) __attribute__((amdgpu_waves_per_eu(2))) void multi_bit_kernel_k1l1(
    u64* __restrict__ lwe_out, const u64* __restrict__ lwe_in, PbsIo io, const cplx* __restrict__ fbsk,
    const cplx* __restrict__ roots, uint32_t n_lwe, uint32_t batch, int base_log, int level, Tables tb) {
  __shared__ Wg<1, CT_FAST> wg;
  multi_bit_body<1, true, CT_FAST, G>(lwe_out, lwe_in, io, fbsk, roots, n_lwe, batch, base_log, level, tb, wg);
}

}  // namespace fft

// ---- launcher -------------------------------------------------------------------------------------
template <int K, bool L1, int G>
static hipError_t multi_bit_one(uint64_t* out, const uint64_t* lwe_in, const PbsIo& io, const fft::cplx* g,
                                const fft::cplx* roots, size_t n_lwe, size_t batch, int base_log, int level,
                                const FftTables& t, hipStream_t s) {
  if (K == 1 && L1)
    hipLaunchKernelGGL(fft::multi_bit_kernel_k1l1<G>, dim3((unsigned)((batch + fft::CT_FAST - 1) / fft::CT_FAST)),
                       dim3(128 * fft::CT_FAST), 0, s, out, lwe_in, io, g, roots, (uint32_t)n_lwe, (uint32_t)batch,
                       base_log, level, fft::tables(t));
  else
    hipLaunchKernelGGL((fft::multi_bit_kernel<K, L1, G>), dim3((unsigned)batch), dim3(64 * (K + 1)), 0, s, out, lwe_in,
                       io, g, roots, (uint32_t)n_lwe, (uint32_t)batch, base_log, level, fft::tables(t));
  return hipGetLastError();
}

template <int G>
static hipError_t multi_bit_g(int k, uint64_t* out, const uint64_t* lwe_in, const PbsIo& io, const fft::cplx* g,
                              const fft::cplx* roots, size_t n_lwe, size_t batch, int base_log, int level,
                              const FftTables& t, hipStream_t s) {
  const bool l1 = level == 1;
  if (k == 1)
    return l1 ? multi_bit_one<1, true, G>(out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s)
              : multi_bit_one<1, false, G>(out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s);
  if (k == 2)
    return l1 ? multi_bit_one<2, true, G>(out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s)
              : multi_bit_one<2, false, G>(out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s);
  return hipErrorInvalidValue;
}

hipError_t launch_fft64_multi_bit_pbs(int k, int grouping_factor, uint64_t* out, const uint64_t* lwe_in,
                                      const PbsIo& io, const double* fbsk, size_t n_lwe, size_t batch, int base_log,
                                      int level, const FftTables& t, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (!t.roots || n_lwe % (size_t)grouping_factor) return hipErrorInvalidValue;
  const auto* g = reinterpret_cast<const fft::cplx*>(fbsk);
  const auto* roots = reinterpret_cast<const fft::cplx*>(t.roots);
  switch (grouping_factor) {
    case 2: return multi_bit_g<2>(k, out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s);
    case 3: return multi_bit_g<3>(k, out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s);
    case 4: return multi_bit_g<4>(k, out, lwe_in, io, g, roots, n_lwe, batch, base_log, level, t, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mi
