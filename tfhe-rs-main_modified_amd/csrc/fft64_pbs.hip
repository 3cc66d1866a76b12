// fft64_pbs.hip — the f64-FFT programmable bootstrap of tfhe core_crypto (the default shortint PBS path)
// on MI355X.  Reference paths relative to /root/reference/tfhe/src/core_crypto:
//   negacyclic FFT          fft_impl/fft64/math/fft/mod.rs:30-76 (Twisties), 227-356 (conversions),
//                           524-586 (forward_with_conv / backward_with_conv)
//   external product        fft_impl/fft64/crypto/ggsw.rs:483-603 (+ update_with_fmadd :617-698)
//   blind rotate / PBS      fft_impl/fft64/crypto/bootstrap.rs:294-381, 481-521
//   key conversion          fft_impl/fft64/crypto/bootstrap.rs:199-225 (forward_as_torus per polynomial)
//
// The transform: a real negacyclic polynomial of N = 2048 u64 coefficients is folded into M = 1024 complex
// values u[n] = x[n] + i x[n + M] (forward_with_conv's split), twisted by w^n = exp(i pi n / 2M)
// (Twisties::new(M)), and transformed with an M-point complex DFT (exp(-2 pi i / M) kernel).  The reference
// runs tfhe-fft's measured "unordered" plan, whose Fourier-domain order is implementation defined; here the
// order is this engine's own (documented below, exported by mi_fft64_fourier_order); the reference serialises the
// natural order, which fourier_reorder_kernel converts to and from.  Results are f64 computations, not bit-identical to the reference's
// (parity is decryption + an error bound against a numpy restatement).
//
// MI355X mapping: one wave per polynomial, 16 complex values per lane in VGPRs (lane j holds u[j + 64 m],
// m < 16), M = 16 x 64 split into three radix passes (fft_fwd below): an in-lane DFT16 over m; a DFT4 over the
// two top lane bits done in registers with gfx950's half-lane swaps (v_permlane32_swap / v_permlane16_swap);
// one LDS transpose (rows of 17, conflict-free) and an in-lane DFT16 over the low four lane bits.  The inverse
// runs the conjugate passes in reverse.  All f64 arithmetic is FMA-contracted by hand where the reference's pulp
// kernels use mul_add.  The transform, PairSync and the workgroup layout live in fft64_engine.hpp, shared with the
// multi-bit PBS (fft64_multi_bit.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft64_decomp.hpp"
#include "fft64_device.hpp"
#include "fft64_engine.hpp"
#include "fft64_launch.hpp"

namespace mi {
namespace fft {

// ---- forward_as_torus / backward_as_torus over a batch of polynomials (key conversion, tests) ------
// one wave per polynomial; `fourier`: batch x 1024 complex in the Fourier layout (position reg * 64 + lane)
__global__ __launch_bounds__(64) void fwd_torus_kernel(cplx* __restrict__ fourier, const u64* __restrict__ std_,
                                                       uint64_t batch, Tables tb) {
  __shared__ cplx buf[BUF];
  __shared__ cplx t2[TB];
  const int lane = threadIdx.x;
  if (lane < TB) t2[lane] = tb.t2[lane];
  __syncthreads();
  const uint64_t b = blockIdx.x;
  if (b >= batch) return;
  const u64* x = std_ + b * N;
  constexpr double NORM = 1.0 / 18446744073709551616.0;  // 2^-64 (convert_forward_torus)
  cplx u[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) u[m] = {s64_to_f64(x[lane + 64 * m]) * NORM, s64_to_f64(x[M + lane + 64 * m]) * NORM};
  fft_fwd(u, buf, tb.t1, t2, tb.cm, lane);
  cplx* out = fourier + b * M;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[r * 64 + lane] = u[r];
}

__global__ __launch_bounds__(64) void bwd_torus_kernel(u64* __restrict__ std_, const cplx* __restrict__ fourier,
                                                       uint64_t batch, int add, Tables tb) {
  __shared__ cplx buf[BUF];
  __shared__ cplx t2[TB];
  const int lane = threadIdx.x;
  if (lane < TB) t2[lane] = tb.t2[lane];
  __syncthreads();
  const uint64_t b = blockIdx.x;
  if (b >= batch) return;
  const cplx* in = fourier + b * M;
  cplx u[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) u[r] = in[r * 64 + lane];
  fft_inv(u, buf, tb.t1, t2, tb.cmi, lane);
  u64* x = std_ + b * N;
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const u64 re = from_torus_scaled(u[m].re * 0x1p64), im = from_torus_scaled(u[m].im * 0x1p64);
    x[lane + 64 * m] = add ? x[lane + 64 * m] + re : re;
    x[M + lane + 64 * m] = add ? x[M + lane + 64 * m] + im : im;
  }
}

// ---- Fourier order interchange (tfhe-fft/src/unordered.rs:943-1020, serialize / deserialize_fourier_buffer) ----
// The reference serialises a Fourier polynomial in the natural DFT order (element i = frequency i), whatever its
// plan's internal order.  Engine position p = 64 r + l holds frequency fft64_frequency(r, l) = 64 r + f(l), a
// permutation of the low six bits only.  One 256-lane workgroup per polynomial stages it in LDS (coalesced 16-B
// reads), then writes the other order coalesced; in place is safe (every read lands before the barrier).
template <bool TO_STD>
__global__ __launch_bounds__(256) void fourier_reorder_kernel(cplx* out, const cplx* in, uint64_t polys) {
  __shared__ cplx buf[M];
  const uint64_t b = blockIdx.x;
  if (b >= polys) return;
  const cplx* src = in + b * M;
#pragma unroll
  for (int i = 0; i < M / 256; ++i) buf[threadIdx.x + 256 * i] = src[threadIdx.x + 256 * i];
  __syncthreads();
  cplx* dst = out + b * M;
#pragma unroll
  for (int i = 0; i < M / 256; ++i) {
    const int j = threadIdx.x + 256 * i, hi = j & ~63, lo = j & 63;
    dst[j] = buf[hi | (TO_STD ? low6_position(lo) : low6_frequency(lo))];
  }
}

// ---- external product on registers ----------------------------------------------------------------
// Wave w (< K + 1, wave-uniform) owns GLWE polynomial w.  in: ct1[NPL] = this wave's polynomial of the GLWE
// to decompose (coefficient lane + 64 r); acc[r] += from_torus(the product's polynomial w).  `ggsw`: level x
// (K+1) rows x (K+1) cols x M complex (Fourier layout), highest level first, as the reference's
// FourierGgswCiphertext.  `pair` = this ciphertext's (K+1) per-wave LDS buffers; t1 / t2 the twiddle tables
// (LDS copies in the PBS / external-product kernels).
template <int K, bool L1, bool WGB>
__device__ __forceinline__ void ext_product_add(u64 (&acc)[NPL], const u64 (&ct1)[NPL], const cplx* __restrict__ ggsw,
                                                int base_log, int level, cplx* pair, const cplx* t1, const cplx* t2,
                                                const cplx* cm, const cplx* cmi, int w, int lane,
                                                PairSync<K, WGB>& ps) {
  cplx* buf = pair + w * BUF;
  cplx y[16];
  if (L1) {
    cplx u[16];
    if (base_log <= 31) {  // uniform: digits from the high words, exact in int32
#pragma unroll
      for (int m = 0; m < 16; ++m)
        u[m] = {(double)decompose_l1_hi((uint32_t)(ct1[m] >> 32), base_log),
                (double)decompose_l1_hi((uint32_t)(ct1[m + 16] >> 32), base_log)};
    } else {
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        u64 s0 = decomp_init_native(ct1[m], base_log, 1), s1 = decomp_init_native(ct1[m + 16], base_log, 1);
        const u64 d0 = decompose_one_level(base_log, s0), d1 = decompose_one_level(base_log, s1);
        u[m] = {s64_to_f64(d0), s64_to_f64(d1)};  // convert_forward_integer: into_signed as f64
      }
    }
    fft_fwd(u, buf, t1, t2, cm, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) buf[r * 64 + lane] = u[r];
    // update_with_fmadd: y_w = sum_rr X_rr * G[rr][w] (own transform from registers, the other K from LDS).
    // Branch-free (the other rows are rr = o + (o >= w), o < K); the key rows are loaded in batches of HB positions,
    // each issued one batch ahead (the first before the exchange barrier, so its latency overlaps the wait).  One-box
    // A/Bs: in the 4-ciphertext PBS workgroups HB = 4 is 0.9 % faster than 2 and HB = 8 1.9 % slower than 4
    // (profiles/r3/fft_hb*_ab); the one-ciphertext external-product workgroups (WGB) lost 10 % with 4, so they keep 2.
    const cplx* gw = ggsw + (size_t)(w * (K + 1) + w) * M + lane;
    const cplx* go[K];
    const cplx* xo[K];
#pragma unroll
    for (int o = 0; o < K; ++o) {
      const int rr = o + (o >= w ? 1 : 0);
      go[o] = ggsw + (size_t)(rr * (K + 1) + w) * M + lane;
      xo[o] = pair + rr * BUF + lane;
    }
    constexpr int HB = WGB ? 2 : 4;
    cplx kw[HB], ko[K][HB];
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      kw[j] = gw[j * 64];
#pragma unroll
      for (int o = 0; o < K; ++o) ko[o][j] = go[o][j * 64];
    }
    ps.sync();
#pragma unroll
    for (int h = 0; h < 16 / HB; ++h) {
#pragma unroll
      for (int j = 0; j < HB; ++j) {
        const int r = h * HB + j;
        cplx a = cmul(u[r], kw[j]);
#pragma unroll
        for (int o = 0; o < K; ++o) a = cfma(xo[o][r * 64], ko[o][j], a);
        y[r] = a;
      }
      if (h + 1 < 16 / HB) {
#pragma unroll
        for (int j = 0; j < HB; ++j) {
          const int r = (h + 1) * HB + j;
          kw[j] = gw[r * 64];
#pragma unroll
          for (int o = 0; o < K; ++o) ko[o][j] = go[o][r * 64];
        }
      }
    }
    ps.sync();
  } else {
    u64 st[NPL];
#pragma unroll
    for (int r = 0; r < NPL; ++r) st[r] = decomp_init_native(ct1[r], base_log, level);
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = {0.0, 0.0};
#pragma unroll 1
    for (int li = 0; li < level; ++li) {
      cplx u[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const u64 d0 = decompose_one_level(base_log, st[m]), d1 = decompose_one_level(base_log, st[m + 16]);
        u[m] = {s64_to_f64(d0), s64_to_f64(d1)};
      }
      fft_fwd(u, buf, t1, t2, cm, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) buf[r * 64 + lane] = u[r];
      ps.sync();
      // the decomposition iterator yields the least significant level first, which the GGSW stores first
      const cplx* mat = ggsw + (size_t)li * (K + 1) * (K + 1) * M;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        cplx a = y[r];
#pragma unroll
        for (int rr = 0; rr <= K; ++rr)
          a = cfma(pair[rr * BUF + r * 64 + lane], mat[(size_t)(rr * (K + 1) + w) * M + r * 64 + lane], a);
        y[r] = a;
      }
      ps.sync();
    }
  }
  fft_inv(y, buf, t1, t2, cmi, lane);
#pragma unroll
  for (int m = 0; m < 16; ++m) {  // convert_add_backward_torus
    add_torus(acc[m], y[m].re);
    add_torus(acc[m + 16], y[m].im);
  }
}

// EXT : out[b] += GGSW (.) glwe[b]                       (add_external_product_assign)
// CMUX: glwe[b] -= out[b]; out[b] += GGSW (.) glwe[b]    (cmux: ct1 -= ct0; ct0 += ext(ct1))
template <int K, bool CMUX, bool L1, int CT>
__device__ __forceinline__ void ext_product_body(u64* __restrict__ out, u64* __restrict__ glwe,
                                                 const cplx* __restrict__ ggsw, uint32_t batch, int base_log,
                                                 int level, const Tables& tb, Wg<K, CT>& wg) {
  load_tables(wg, tb);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ct = wave / (K + 1), w = wave % (K + 1);
  const uint32_t b0 = blockIdx.x * CT + ct;
  const bool valid = b0 < batch;  // every wave takes part in the barriers
  const uint32_t b = valid ? b0 : batch - 1;
  u64* in = glwe + ((size_t)b * (K + 1) + w) * N;
  u64* o = out + ((size_t)b * (K + 1) + w) * N;
  u64 ct1[NPL], acc[NPL];
#pragma unroll
  for (int r = 0; r < NPL; ++r) {
    ct1[r] = in[lane + 64 * r];
    acc[r] = o[lane + 64 * r];
    if (CMUX) {
      ct1[r] -= acc[r];
      if (valid) in[lane + 64 * r] = ct1[r];
    }
  }
  PairSync<K, CT == 1> ps{wg.flags + ct * (K + 1), w, 0u};
  ext_product_add<K, L1>(acc, ct1, ggsw, base_log, level, wg.bufs + ct * (K + 1) * BUF, wg.t1, wg.t2, wg.cm, wg.cmi, w,
                         lane, ps);
  if (valid) {
#pragma unroll
    for (int r = 0; r < NPL; ++r) o[lane + 64 * r] = acc[r];
  }
}

// One GLWE per workgroup (the external product / CMUX entry points; the PBS kernel below batches 4 ciphertexts
// per workgroup for the shortint shape).
template <int K, bool CMUX, bool L1>
__global__ __launch_bounds__(64 * (K + 1)) void ext_product_kernel(u64* __restrict__ out, u64* __restrict__ glwe,
                                                                   const cplx* __restrict__ ggsw, uint32_t batch,
                                                                   int base_log, int level, Tables tb) {
  __shared__ Wg<K, 1> wg;
  ext_product_body<K, CMUX, L1, 1>(out, glwe, ggsw, batch, base_log, level, tb, wg);
}
// One GGSW per item: workgroup b (one item) runs the same body with GGSW idx[b] of the
// list; an index >= n_ggsw ends the whole workgroup before it touches anything (uniform: before any barrier).
template <int K, bool CMUX, bool L1>
__global__ __launch_bounds__(64 * (K + 1)) void ext_product_indexed_kernel(u64* __restrict__ out,
                                                                           u64* __restrict__ glwe,
                                                                           const cplx* __restrict__ ggsw_list,
                                                                           const uint32_t* __restrict__ idx,
                                                                           uint32_t n_ggsw, int base_log, int level,
                                                                           Tables tb) {
  __shared__ Wg<K, 1> wg;
  const uint32_t g = idx[blockIdx.x];
  if (g >= n_ggsw) return;
  const size_t ggsw_len = (size_t)level * (K + 1) * (K + 1) * M;
  ext_product_body<K, CMUX, L1, 1>(out, glwe, ggsw_list + (size_t)g * ggsw_len, gridDim.x, base_log, level, tb, wg);
}
// ---- programmable bootstrap (bootstrap.rs:481-521 + blind_rotate_assign :294-381) -------------------
// lwe_in: batch x (n + 1); lut: (K+1) x N shared; fbsk: n x level x (K+1) x (K+1) x M complex;
// lwe_out: batch x (K N + 1).  ms_mode: 0 standard, 1 centered, 2 pre-switched (values in [0, 2N)).
// With several ciphertexts per workgroup a mask element that switches to 0 is not skipped (the reference
// skips it, bootstrap.rs:336): its CMUX difference is the zero polynomial, whose digits, transforms and
// products are exactly 0, so the accumulator is unchanged bit for bit either way.
// io (pbs_io.hpp): the item's LUT (shared, per item or indexed) and the output form (LWE of sample 0, or the rotated
// GLWE itself: blind_rotate_assign, fft64_pbs.rs:186-250).  An item whose LUT index is out of range runs on LUT 0 like a
// padding item and writes nothing.
template <int K, bool L1, int CT>
__device__ __forceinline__ void pbs_body(u64* __restrict__ lwe_out, const u64* __restrict__ lwe_in, const PbsIo& io,
                                         const cplx* __restrict__ fbsk, uint32_t n_lwe,
                                         uint32_t batch, int base_log, int level, int ms_mode, const Tables& tb,
                                         Wg<K, CT>& wg) {
  constexpr int TG = 64 * (K + 1);
  constexpr unsigned LOG_MOD = 12;  // PolynomialSize(2048)::to_blind_rotation_input_modulus_log
  load_tables(wg, tb);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ct = wave / (K + 1), w = wave % (K + 1);
  const uint32_t b0 = blockIdx.x * CT + ct;
  const uint32_t b = b0 < batch ? b0 : batch - 1;
  const u64* lut = io.lut_for(b, (uint64_t)(K + 1) * N);
  const bool valid = b0 < batch && lut;  // every wave takes part in the barriers
  if (!lut) lut = io.lut;
  const u64* lwe = lwe_in + (size_t)b * (n_lwe + 1);
  const size_t ggsw_len = (size_t)level * (K + 1) * (K + 1) * M;
  cplx* pair = wg.bufs + ct * (K + 1) * BUF;
  u64* mine = reinterpret_cast<u64*>(pair + w * BUF);  // this wave's rotation buffer (2048 u64 = 16 KiB)

  u64 body_corr = 0;
  if (ms_mode == 1)
    body_corr = centered_body_correction<TG>(lwe, n_lwe, LOG_MOD, w * 64 + lane, reinterpret_cast<u64*>(pair));
  const u64 body = (ms_mode == 2) ? (lwe[n_lwe] & (2 * N - 1)) : modulus_switch(lwe[n_lwe] + body_corr, LOG_MOD);

  // local accumulator = LUT / X^body (polynomial_wrapping_monic_monomial_div)
  u64 acc[NPL];
  {
    const u64* lp = lut + (size_t)w * N;
    const int full = (int)(body / N) & 1, rem = (int)(body % N);
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
      const int m = lane + 64 * r;  // div: new[m] = old[(m + rem) % N], negated for m >= N - rem
      u64 v = lp[(m + rem) & (N - 1)];
      if (full ^ (m >= N - rem)) v = (u64)0 - v;
      acc[r] = v;
    }
  }

  const uint32_t lane_bytes = (uint32_t)lane * 8u;
  PairSync<K, CT == 1> ps{wg.flags + ct * (K + 1), w, 0u};

  for (uint32_t i = 0; i < n_lwe; ++i) {
    const uint32_t a = (uint32_t)((ms_mode == 2) ? (lwe[i] & (2 * N - 1)) : modulus_switch(lwe[i], LOG_MOD));
    if (CT == 1 && a == 0) continue;  // bootstrap.rs:336 (uniform per workgroup)
    const bool full = (a >> 11) & 1u;
    const int rem = (int)(a & (N - 1));
#pragma unroll
    for (int r = 0; r < NPL; ++r) mine[lane + 64 * r] = acc[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // polynomial_wrapping_monic_monomial_mul_and_subtract: ct1[e] = s_e acc[(e - rem) mod N] - acc[e], s_e = -1 iff
    // Monomial::mul_neg(e) (core_scalar.hpp; the source is its mul_src, restated here on byte addresses).  With m = s_e < 0 ? ~0 : 0:  s_e v - acc = (v ^ m) - (acc + m).
    // Source of e = lane + 64 r: (e - rem) mod N at byte rot + 512 r (no wrap: e >= rem) or that minus 16 KiB.
    // Lanes >= rem never wrap; below rem, e < rem holds exactly for the wrapped sources, which are the
    // in-range ones — so one per-lane base (A or A - 16 KiB) selected by the same compare as the sign, and the
    // 512 r in the instruction's offset field.
    const uint32_t rot = (lane_bytes - (uint32_t)rem * 8u) & (8u * N - 1u);
    const char* base_a = reinterpret_cast<const char*>(mine) + rot;
    const char* base_b = lane >= rem ? base_a : base_a - 8 * N;
    u64 ct1[NPL];
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
      const bool wrapped = lane < rem - 64 * r;
      const u64 v = *reinterpret_cast<const u64*>((wrapped ? base_a : base_b) + 512 * r);
      const uint32_t m = (wrapped != full) ? ~0u : 0u;
      const u64 mm = ((u64)m << 32) | m;
      ct1[r] = (v ^ mm) - (acc[r] + mm);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    ext_product_add<K, L1>(acc, ct1, fbsk + (size_t)i * ggsw_len, base_log, level, pair, wg.t1, wg.t2, wg.cm, wg.cmi, w,
                           lane, ps);
  }

  if (io.glwe_out) {  // the rotated accumulator (the LUT was divided by X^body before the loop)
    if (valid) {
      u64* g = io.glwe_out + ((size_t)b * (K + 1) + w) * N;
#pragma unroll
      for (int r = 0; r < NPL; ++r) g[lane + 64 * r] = acc[r];
    }
    return;
  }
  // extract_lwe_sample_from_glwe_ciphertext (glwe_sample_extraction.rs:89-160), nth = 0
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

template <int K, bool L1>
__global__ __launch_bounds__(64 * (K + 1)) void pbs_kernel(u64* __restrict__ lwe_out, const u64* __restrict__ lwe_in,
                                                           PbsIo io, const cplx* __restrict__ fbsk,
                                                           uint32_t n_lwe, uint32_t batch, int base_log, int level,
                                                           int ms_mode, Tables tb) {
  __shared__ Wg<K, 1> wg;
  pbs_body<K, L1, 1>(lwe_out, lwe_in, io, fbsk, n_lwe, batch, base_log, level, ms_mode, tb, wg);
}
__global__ __launch_bounds__(128 * CT_FAST) __attribute__((amdgpu_waves_per_eu(2))) void pbs_kernel_k1l1(
    u64* __restrict__ lwe_out, const u64* __restrict__ lwe_in, PbsIo io,
    const cplx* __restrict__ fbsk, uint32_t n_lwe, uint32_t batch, int base_log, int level, int ms_mode, Tables tb) {
  __shared__ Wg<1, CT_FAST> wg;
  pbs_body<1, true, CT_FAST>(lwe_out, lwe_in, io, fbsk, n_lwe, batch, base_log, level, ms_mode, tb, wg);
}

}  // namespace fft

// ---- launchers ----------------------------------------------------------------------------------
using fft::tables;

hipError_t launch_fft64_fwd_torus(double* fourier, const uint64_t* std_, size_t batch, const FftTables& t,
                                  hipStream_t s) {
  if (batch == 0) return hipSuccess;
  hipLaunchKernelGGL(fft::fwd_torus_kernel, dim3((unsigned)batch), dim3(64), 0, s,
                     reinterpret_cast<fft::cplx*>(fourier), std_, (uint64_t)batch, tables(t));
  return hipGetLastError();
}

hipError_t launch_fft64_bwd_torus(uint64_t* std_, const double* fourier, size_t batch, bool add, const FftTables& t,
                                  hipStream_t s) {
  if (batch == 0) return hipSuccess;
  hipLaunchKernelGGL(fft::bwd_torus_kernel, dim3((unsigned)batch), dim3(64), 0, s, std_,
                     reinterpret_cast<const fft::cplx*>(fourier), (uint64_t)batch, add ? 1 : 0, tables(t));
  return hipGetLastError();
}

hipError_t launch_fft64_reorder(double* out, const double* in, size_t polys, bool to_standard, hipStream_t s) {
  if (polys == 0) return hipSuccess;
  auto* o = reinterpret_cast<fft::cplx*>(out);
  const auto* i = reinterpret_cast<const fft::cplx*>(in);
  if (to_standard)
    hipLaunchKernelGGL(fft::fourier_reorder_kernel<true>, dim3((unsigned)polys), dim3(256), 0, s, o, i, (uint64_t)polys);
  else
    hipLaunchKernelGGL(fft::fourier_reorder_kernel<false>, dim3((unsigned)polys), dim3(256), 0, s, o, i, (uint64_t)polys);
  return hipGetLastError();
}

template <int K, bool CMUX, bool L1>
static hipError_t ext_one(uint64_t* out, uint64_t* glwe, const fft::cplx* g, size_t batch, int base_log, int level,
                          const FftTables& t, hipStream_t s) {
  hipLaunchKernelGGL((fft::ext_product_kernel<K, CMUX, L1>), dim3((unsigned)batch), dim3(64 * (K + 1)), 0, s, out, glwe,
                     g, (uint32_t)batch, base_log, level, tables(t));
  return hipGetLastError();
}

template <int K, bool CMUX, bool L1>
static hipError_t ext_one_indexed(uint64_t* out, uint64_t* glwe, const fft::cplx* g, const uint32_t* idx,
                                  size_t n_ggsw, size_t batch, int base_log, int level, const FftTables& t,
                                  hipStream_t s) {
  hipLaunchKernelGGL((fft::ext_product_indexed_kernel<K, CMUX, L1>), dim3((unsigned)batch), dim3(64 * (K + 1)), 0, s,
                     out, glwe, g, idx, (uint32_t)n_ggsw, base_log, level, tables(t));
  return hipGetLastError();
}

template <int K>
static hipError_t ext_k_indexed(bool cmux, uint64_t* out, uint64_t* glwe, const double* ggsw, const uint32_t* idx,
                                size_t n_ggsw, size_t batch, int base_log, int level, const FftTables& t,
                                hipStream_t s) {
  const auto* g = reinterpret_cast<const fft::cplx*>(ggsw);
  if (level == 1)
    return cmux ? ext_one_indexed<K, true, true>(out, glwe, g, idx, n_ggsw, batch, base_log, level, t, s)
                : ext_one_indexed<K, false, true>(out, glwe, g, idx, n_ggsw, batch, base_log, level, t, s);
  return cmux ? ext_one_indexed<K, true, false>(out, glwe, g, idx, n_ggsw, batch, base_log, level, t, s)
              : ext_one_indexed<K, false, false>(out, glwe, g, idx, n_ggsw, batch, base_log, level, t, s);
}

template <int K>
static hipError_t ext_k(bool cmux, uint64_t* out, uint64_t* glwe, const double* ggsw, size_t batch, int base_log,
                        int level, const FftTables& t, hipStream_t s) {
  const auto* g = reinterpret_cast<const fft::cplx*>(ggsw);
  if (level == 1)
    return cmux ? ext_one<K, true, true>(out, glwe, g, batch, base_log, level, t, s)
                : ext_one<K, false, true>(out, glwe, g, batch, base_log, level, t, s);
  return cmux ? ext_one<K, true, false>(out, glwe, g, batch, base_log, level, t, s)
              : ext_one<K, false, false>(out, glwe, g, batch, base_log, level, t, s);
}

hipError_t launch_fft64_ext_product(int k, bool cmux, uint64_t* out, uint64_t* glwe, const double* ggsw, size_t batch,
                                    int base_log, int level, const FftTables& t, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (k == 1) return ext_k<1>(cmux, out, glwe, ggsw, batch, base_log, level, t, s);
  if (k == 2) return ext_k<2>(cmux, out, glwe, ggsw, batch, base_log, level, t, s);
  return hipErrorInvalidValue;
}

hipError_t launch_fft64_ext_product_indexed(int k, bool cmux, uint64_t* out, uint64_t* glwe, const double* ggsw_list,
                                            const uint32_t* idx, size_t n_ggsw, size_t batch, int base_log, int level,
                                            const FftTables& t, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (k == 1) return ext_k_indexed<1>(cmux, out, glwe, ggsw_list, idx, n_ggsw, batch, base_log, level, t, s);
  if (k == 2) return ext_k_indexed<2>(cmux, out, glwe, ggsw_list, idx, n_ggsw, batch, base_log, level, t, s);
  return hipErrorInvalidValue;
}

template <int K, bool L1>
static hipError_t pbs_one(uint64_t* out, const uint64_t* lwe_in, const PbsIo& lut, const fft::cplx* g, size_t n_lwe,
                          size_t batch, int base_log, int level, int ms_mode, const FftTables& t, hipStream_t s) {
  if (K == 1 && L1)
    hipLaunchKernelGGL(fft::pbs_kernel_k1l1, dim3((unsigned)((batch + fft::CT_FAST - 1) / fft::CT_FAST)),
                       dim3(128 * fft::CT_FAST), 0, s, out, lwe_in, lut, g, (uint32_t)n_lwe, (uint32_t)batch, base_log,
                       level, ms_mode, tables(t));
  else
    hipLaunchKernelGGL((fft::pbs_kernel<K, L1>), dim3((unsigned)batch), dim3(64 * (K + 1)), 0, s, out, lwe_in, lut, g,
                       (uint32_t)n_lwe, (uint32_t)batch, base_log, level, ms_mode, tables(t));
  return hipGetLastError();
}

hipError_t launch_fft64_pbs(int k, uint64_t* out, const uint64_t* lwe_in, const PbsIo& lut, const double* fbsk,
                            size_t n_lwe, size_t batch, int base_log, int level, int ms_mode, const FftTables& t,
                            hipStream_t s) {
  if (batch == 0) return hipSuccess;
  const auto* g = reinterpret_cast<const fft::cplx*>(fbsk);
  const bool l1 = level == 1;
  if (k == 1)
    return l1 ? pbs_one<1, true>(out, lwe_in, lut, g, n_lwe, batch, base_log, level, ms_mode, t, s)
              : pbs_one<1, false>(out, lwe_in, lut, g, n_lwe, batch, base_log, level, ms_mode, t, s);
  if (k == 2)
    return l1 ? pbs_one<2, true>(out, lwe_in, lut, g, n_lwe, batch, base_log, level, ms_mode, t, s)
              : pbs_one<2, false>(out, lwe_in, lut, g, n_lwe, batch, base_log, level, ms_mode, t, s);
  return hipErrorInvalidValue;
}

}  // namespace mi
