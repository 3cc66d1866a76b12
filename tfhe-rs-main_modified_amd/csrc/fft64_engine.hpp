// fft64_engine.hpp — the one-wave N = 2048 f64-FFT engine shared by the kernels that run on it: the classic PBS /
// external product (fft64_pbs.hip) and the multi-bit PBS (fft64_multi_bit.hip).  The transform (fft_fwd / fft_inv: see
// fft64_pbs.hip's header for the mapping), the synchronisation of a ciphertext's waves (PairSync) and the workgroup
// layout (Wg).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft64_device.hpp"
#include "fft64_launch.hpp"
#include "pbs_io.hpp"

namespace mi {
namespace fft {

constexpr double C8 = 0.92387953251128673848;   // cos(pi / 8)
constexpr double S8 = 0.38268343236508978178;   // sin(pi / 8)
constexpr double R2 = 0.70710678118654752440;   // sqrt(1/2)

// DFT4 in place on a[o], a[o + s], a[o + 2s], a[o + 3s]; INV: exp(+2 pi i / 4) kernel
template <bool INV>
__device__ __forceinline__ void dft4(cplx* a, int o, int s) {
  const cplx a0 = a[o], a1 = a[o + s], a2 = a[o + 2 * s], a3 = a[o + 3 * s];
  const cplx s02 = cadd(a0, a2), d02 = csub(a0, a2), s13 = cadd(a1, a3), d13 = csub(a1, a3);
  const cplx r = INV ? mul_pos_i(d13) : mul_neg_i(d13);
  a[o] = cadd(s02, s13);
  a[o + 2 * s] = csub(s02, s13);
  a[o + s] = cadd(d02, r);
  a[o + 3 * s] = csub(d02, r);
}

// x * W16^e (forward: exp(-2 pi i e / 16); INV: conjugate), e in 1..9
template <bool INV>
__device__ __forceinline__ cplx tw16(cplx x, int e) {
  double c, s;  // W = c - i s (forward)
  switch (e) {
    case 1: c = C8, s = S8; break;
    case 2: c = R2, s = R2; break;
    case 3: c = S8, s = C8; break;
    case 4: return INV ? mul_pos_i(x) : mul_neg_i(x);
    case 6: c = -R2, s = R2; break;
    case 9: c = -C8, s = -S8; break;  // exp(-2 pi i 9/16) = -cos(pi/8) + i sin(pi/8)
    default: return x;
  }
  if (e == 2 || e == 6) {  // (c - i s) with |c| = |s| = R2: 2 adds + 2 muls
    const double sgn_c = (e == 2) ? 1.0 : -1.0;
    if (!INV) {  // (re + i im)(sgn R2 - i R2)
      const double re = sgn_c * x.re + x.im, im = sgn_c * x.im - x.re;
      return {re * R2, im * R2};
    } else {  // (re + i im)(sgn R2 + i R2)
      const double re = sgn_c * x.re - x.im, im = sgn_c * x.im + x.re;
      return {re * R2, im * R2};
    }
  }
  const cplx w = {c, INV ? s : -s};
  return cmul(x, w);
}

// DFT16 of a[0..16) in place, natural order in and out: X[k1 + 4 k2] = sum_m a[m] W16^(m k)
template <bool INV>
__device__ __forceinline__ void dft16(cplx (&a)[16]) {
#pragma unroll
  for (int m1 = 0; m1 < 4; ++m1) dft4<INV>(a, m1, 4);  // over m2: a[m1 + 4 k1] = b[m1][k1]
#pragma unroll
  for (int m1 = 1; m1 < 4; ++m1)
#pragma unroll
    for (int k1 = 1; k1 < 4; ++k1) a[m1 + 4 * k1] = tw16<INV>(a[m1 + 4 * k1], m1 * k1);
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) dft4<INV>(a, 4 * k1, 1);  // over m1: a[4 k1 + k2] = X[k1 + 4 k2]
  cplx t[16];
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) t[k1 + 4 * k2] = a[4 * k1 + k2];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = t[i];
}

constexpr int ROW = 17;                // transpose row stride (complex): conflict-free both ways
constexpr int BUF = 64 * ROW;          // per-wave LDS buffer (complex): 17 KiB
constexpr int TB = 48;                 // pass-3 twiddle table: [q1 - 1][jl], q1 = 1..3

// In-register exchanges across the lane halves (gfx950 v_permlane32_swap / v_permlane16_swap): lanes 32..63
// of `a` trade places with lanes 0..31 of `b` (X = 32), or lanes 16..31 / 48..63 of `a` with lanes 0..15 /
// 32..47 of `b` (X = 16).  For a pair of registers holding elements (r, r') this turns the lane bit into the
// register bit: afterwards the low lanes hold (r: bit 0, r: bit 1) and the high lanes (r': bit 0, r': bit 1).
template <int X>
__device__ __forceinline__ void swap_dw(double& a, double& b) {
  const u64 x = __double_as_longlong(a), y = __double_as_longlong(b);
  uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32), yl = (uint32_t)y, yh = (uint32_t)(y >> 32);
  if constexpr (X == 32) {
    const auto l = __builtin_amdgcn_permlane32_swap(xl, yl, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(xh, yh, false, false);
    xl = l[0], yl = l[1], xh = h[0], yh = h[1];
  } else {
    const auto l = __builtin_amdgcn_permlane16_swap(xl, yl, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(xh, yh, false, false);
    xl = l[0], yl = l[1], xh = h[0], yh = h[1];
  }
  a = __longlong_as_double((long long)(((u64)xh << 32) | xl));
  b = __longlong_as_double((long long)(((u64)yh << 32) | yl));
}
template <int X>
__device__ __forceinline__ void swap_c(cplx& a, cplx& b) {
  swap_dw<X>(a.re, b.re);
  swap_dw<X>(a.im, b.im);
}

// The per-m twist factor exp(i pi m / 32) (the host table's cm, rounded the same way from long double): built in SGPRs
// right at its use by volatile scalar moves (volatile: not hoisted out of the blind-rotation loop, where 30 live
// constants would spill), so the pass-1 twist and the inverse's untwist read no table (16 serialised LDS loads per
// transform otherwise, each a full LDS latency in front of 4 FMAs)
__device__ __forceinline__ double sconst(u64 bits) {
  uint32_t lo, hi;
  asm volatile("s_mov_b32 %0, %1" : "=s"(lo) : "i"((uint32_t)bits));
  asm volatile("s_mov_b32 %0, %1" : "=s"(hi) : "i"((uint32_t)(bits >> 32)));
  return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
template <bool CONJ_SCALED>  // false: exp(i pi m / 32); true: exp(-i pi m / 32) / M (the host table's cmi)
__device__ __forceinline__ cplx cm_const(int m) {
  constexpr u64 T[16][2] = {
      {0x3ff0000000000000ull, 0x0000000000000000ull},
      {0x3fefd88da3d12526ull, 0x3fb917a6bc29b42cull},
      {0x3fef6297cff75cb0ull, 0x3fc8f8b83c69a60bull},
      {0x3fee9f4156c62ddaull, 0x3fd294062ed59f06ull},
      {0x3fed906bcf328d46ull, 0x3fd87de2a6aea963ull},
      {0x3fec38b2f180bdb1ull, 0x3fde2b5d3806f63bull},
      {0x3fea9b66290ea1a3ull, 0x3fe1c73b39ae68c8ull},
      {0x3fe8bc806b151741ull, 0x3fe44cf325091dd6ull},
      {0x3fe6a09e667f3bcdull, 0x3fe6a09e667f3bcdull},
      {0x3fe44cf325091dd6ull, 0x3fe8bc806b151741ull},
      {0x3fe1c73b39ae68c8ull, 0x3fea9b66290ea1a3ull},
      {0x3fde2b5d3806f63bull, 0x3fec38b2f180bdb1ull},
      {0x3fd87de2a6aea963ull, 0x3fed906bcf328d46ull},
      {0x3fd294062ed59f06ull, 0x3fee9f4156c62ddaull},
      {0x3fc8f8b83c69a60bull, 0x3fef6297cff75cb0ull},
      {0x3fb917a6bc29b42cull, 0x3fefd88da3d12526ull}};
  const cplx c = {sconst(T[m][0]), sconst(T[m][1])};
  if (CONJ_SCALED) return {c.re * (1.0 / 1024.0), -c.im * (1.0 / 1024.0)};  // 1 / M: a power of two, exact
  return c;
}

// Forward: u[m] = folded value at n = lane + 64 m (untwisted); out: the Fourier layout.  M = 16 x 64 with
// n = j + 64 m, j = jl + 16 jh (jl = lane & 15, jh = lane >> 4), frequency f = k1 + 16 q1 + 64 q2:
//   pass 1  in-lane DFT16 over m -> k1 (register), twiddle T1[k1][j] = w^j omega^(j k1) (`t1`, twist folded in;
//           the per-m twist factor `cm` = exp(i pi m / 32) goes before the DFT16)
//   pass 2  DFT4 over jh (lane bits 5, 4) in registers: two radix-2 stages, each one half-lane swap of the
//           register pairs (r, r + 8) / (r, r + 4) and a butterfly (the W4 twiddle -i is per register)
//           -> q1 = q10 + 2 q11 in register bits 3, 2; lane bits 5, 4 now hold k1 bits 3, 2
//   pass 3  twiddle W64^(jl q1) (`t2` = [q1 - 1][jl]), LDS transpose of lane bits 0..3 <-> register bits
//           (rows of 17: conflict-free), in-lane DFT16 over jl -> q2
// Position (lane L, register R) holds f = k1 + 16 q1 + 64 R with k1 = (L & 3) | ((L >> 4) & 3) << 2,
// q1 = ((L >> 3) & 1) | ((L >> 2) & 1) << 1.
__device__ __forceinline__ void fft_fwd(cplx (&u)[16], cplx* buf, const cplx* __restrict__ t1, const cplx* t2,
                                        const cplx* __restrict__ cm, int lane) {
  (void)cm;  // the table's values are cm_const<false>'s
#pragma unroll
  for (int m = 1; m < 16; ++m) u[m] = cmul(u[m], cm_const<false>(m));
  dft16<false>(u);
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) u[k1] = cmul(u[k1], t1[k1 * 64 + lane]);
  // radix 2 over jh1 (lane bit 5): (r, r + 8) = (jh1 = 0, jh1 = 1) -> (q10 = 0, q10 = 1)
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    swap_c<32>(u[r], u[r + 8]);
    const cplx a = u[r], b = u[r + 8];
    u[r] = cadd(a, b);
    u[r + 8] = csub(a, b);
  }
  // radix 2 over jh0 (lane bit 4) with W4^(jh0 q10): (r, r + 4) = (jh0 = 0, jh0 = 1) -> (q11 = 0, q11 = 1)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (r & 4) continue;
    swap_c<16>(u[r], u[r + 4]);
    const cplx a = u[r], b = (r & 8) ? mul_neg_i(u[r + 4]) : u[r + 4];
    u[r] = cadd(a, b);
    u[r + 4] = csub(a, b);
  }
  const int jl = lane & 15;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q1 = ((r >> 3) & 1) | (((r >> 2) & 1) << 1);
    if (q1) u[r] = cmul(u[r], t2[(q1 - 1) * 16 + jl]);
    buf[ROW * lane + r] = u[r];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int row = (lane & 48) * ROW + (lane & 15);  // element (lane' = 16 h + jl, r = lane & 15)
#pragma unroll
  for (int j = 0; j < 16; ++j) u[j] = buf[row + ROW * j];
  dft16<false>(u);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Inverse of fft_fwd (the conjugate transpose of every pass in reverse order), including the 1/M normalisation
// and the untwist (`cmi` = exp(-i pi m / 32) / M: the output is the torus value, ready for add_torus /
// from_torus).
__device__ __forceinline__ void fft_inv(cplx (&u)[16], cplx* buf, const cplx* __restrict__ t1, const cplx* t2,
                                        const cplx* __restrict__ cmi, int lane) {
  dft16<true>(u);
  const int row = (lane & 48) * ROW + (lane & 15);
#pragma unroll
  for (int j = 0; j < 16; ++j) buf[row + ROW * j] = u[j];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int jl = lane & 15;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    u[r] = buf[ROW * lane + r];
    const int q1 = ((r >> 3) & 1) | (((r >> 2) & 1) << 1);
    if (q1) u[r] = cmulc(u[r], t2[(q1 - 1) * 16 + jl]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (r & 4) continue;
    const cplx a = u[r], b = u[r + 4];
    u[r] = cadd(a, b);
    u[r + 4] = (r & 8) ? mul_pos_i(csub(a, b)) : csub(a, b);
    swap_c<16>(u[r], u[r + 4]);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const cplx a = u[r], b = u[r + 8];
    u[r] = cadd(a, b);
    u[r + 8] = csub(a, b);
    swap_c<32>(u[r], u[r + 8]);
  }
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) u[k1] = cmulc(u[k1], t1[k1 * 64 + lane]);
  dft16<true>(u);
  (void)cmi;  // the table's values are cm_const<true>'s
#pragma unroll
  for (int m = 0; m < 16; ++m) u[m] = cmul(u[m], cm_const<true>(m));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Tables {
  const cplx* t1;   // [16][64] forward pass-1 twiddles (twist folded in)
  const cplx* t2;   // [3][16] W64^(jl q1), q1 = 1..3
  const cplx* cm;   // [16] exp(i pi m / 32)
  const cplx* cmi;  // [16] exp(-i pi m / 32) / M
};

constexpr int N = 2048, M = 1024, NPL = N / 64;  // 32 coefficients per lane

// position <-> frequency of the low six bits: position 64 r + l holds frequency 64 r + f(l) (fft64_frequency)
__device__ __forceinline__ int low6_frequency(int l) {  // f(l): see fft64_frequency (fft64_launch.hpp)
  return (l & 3) | (((l >> 4) & 3) << 2) | (((l >> 3) & 1) << 4) | (((l >> 2) & 1) << 5);
}
__device__ __forceinline__ int low6_position(int k) {  // f^-1
  return (k & 3) | (((k >> 5) & 1) << 2) | (((k >> 4) & 1) << 3) | (((k >> 2) & 3) << 4);
}

// Synchronisation of the (K + 1) waves of one ciphertext.  A workgroup holding one ciphertext uses its barrier;
// with several ciphertexts per workgroup each wave publishes a step counter in LDS and waits for its partners'
// (s_sleep between polls), so the ciphertexts of a workgroup do not have to run in lockstep.
template <int K, bool WG_BARRIER>
struct PairSync {
  uint32_t* flags;  // this ciphertext's K + 1 counters (LDS)
  int w;
  uint32_t count;
  __device__ __forceinline__ void sync() {
    if (WG_BARRIER) {
      __syncthreads();
      return;
    }
    ++count;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    *reinterpret_cast<volatile uint32_t*>(flags + w) = count;
    // wait (in one asm block, so the register allocator sees straight-line code) until every partner's counter
    // has reached ours: poll with ds_read_b32, the decision on the first lane's value (all lanes read the same
    // address), s_sleep between polls
#pragma unroll
    for (int o = 0; o < K; ++o) {
      const int rr = o + (o >= w ? 1 : 0);
      const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(flags + rr);
      uint32_t v, sv;
      asm volatile(
          "s_waitcnt lgkmcnt(0)\n"
          "1:\n\t"
          "ds_read_b32 %0, %2\n\t"
          "s_waitcnt lgkmcnt(0)\n\t"
          "v_readfirstlane_b32 %1, %0\n\t"
          "s_cmp_ge_u32 %1, %3\n\t"
          "s_cbranch_scc1 2f\n\t"
          "s_sleep 1\n\t"
          "s_branch 1b\n"
          "2:"
          : "=&v"(v), "=&s"(sv)
          : "v"(lds), "s"(count)
          : "memory", "scc");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
};

// Workgroup layout of the batched kernels: CT ciphertexts x (K + 1) waves; LDS = CT (K + 1) transpose /
// exchange buffers + the two twiddle tables, copied once per workgroup.
template <int K, int CT>
struct Wg {
  static constexpr int WAVES = CT * (K + 1), THREADS = 64 * WAVES;
  cplx bufs[WAVES * BUF];
  cplx t1[16 * 64];
  cplx t2[TB];
  cplx cm[16], cmi[16];
  uint32_t flags[WAVES];
};

template <int K, int CT>
__device__ __forceinline__ void load_tables(Wg<K, CT>& wg, const Tables& tb) {
  for (int i = threadIdx.x; i < 16 * 64; i += Wg<K, CT>::THREADS) wg.t1[i] = tb.t1[i];
  if (threadIdx.x < TB) wg.t2[threadIdx.x] = tb.t2[threadIdx.x];
  if (threadIdx.x < 16) {
    wg.cm[threadIdx.x] = tb.cm[threadIdx.x];
    wg.cmi[threadIdx.x] = tb.cmi[threadIdx.x];
  }
  if (threadIdx.x < Wg<K, CT>::WAVES) wg.flags[threadIdx.x] = 0;
  __syncthreads();
}

constexpr int CT_FAST = 4;

inline Tables tables(const FftTables& t) {
  return {reinterpret_cast<const cplx*>(t.t1), reinterpret_cast<const cplx*>(t.t2),
          reinterpret_cast<const cplx*>(t.cm), reinterpret_cast<const cplx*>(t.cmi)};
}

}  // namespace fft
}  // namespace mi
