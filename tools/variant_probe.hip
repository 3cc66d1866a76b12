// variant_probe.hip — diagnostic build (not part of the library): times the forward and inverse bodies of the twisted
// N = 2048 transform that several trees generate (tools/gen_variants.py TOOLS_DIR... -> tools/_variant_bodies.hpp; the
// default is this tree twice, a body and its identical control) against each other on one stream, interleaved in
// rounds so a clock drift hits every variant alike, and reports per variant whether it writes the same bits as
// variant 0.  One more variant past the generated ones is body 0 in the library's launch form (forward: one wave per
// workgroup, inverse: four).
//
// The probe passes every body the library's per-lane addresses (the W1x lane map, lane = i + 32 par, as
// ntt64_tw_device.hpp).  A tree whose bodies need other per-lane addresses is out of its scope.
//
//   python tools/gen_variants.py [TOOLS_DIR ...] > tools/_variant_bodies.hpp
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/variant_probe.hip -o tools/variant_probe
//   ./tools/variant_probe [batch]          (one JSON line per variant)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "_variant_bodies.hpp"

using u64 = uint64_t;
static constexpr int WAVE_LDS2 = 1088;

#define FWD_ARGS                                                                                              \
  [g_lo] "s"(glo), [g_hi] "s"(ghi), [tw_lo] "s"(twlo), [tw_hi] "s"(twhi), [lw] "s"(lw), [l8] "v"(l8),          \
      [t1w] "v"(t1w), [t1r] "v"(t1r), [t2wl] "v"(t2wl), [t2wh] "v"(t2wh), [t2r] "v"(t2r), [lwo] "v"(lwo)
#define INV_ARGS                                                                                              \
  [g_lo] "s"(glo), [g_hi] "s"(ghi), [tw_lo] "s"(twlo), [tw_hi] "s"(twhi), [lw] "s"(lw), [l8] "v"(l8),          \
      [t1w] "v"(t1w), [t1r] "v"(t1r), [t4w] "v"(t4w), [t4r] "v"(t4r), [lwo] "v"(lwo), [t1x] "v"(t1x),        \
      [t1y] "v"(t1y)

template <int V, bool FWD, int W>
__global__ __launch_bounds__(64 * W) void probe_kernel(u64* __restrict__ data, uint32_t batch, const u64* __restrict__ twist) {
  __shared__ u64 lds[W * WAVE_LDS2];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t poly = blockIdx.x * W + wv;
  if (poly >= batch) return;
  u64* p = data + (uint64_t)poly * 2048;
  const uint32_t S = (uint32_t)(uintptr_t)(lds + wv * WAVE_LDS2);
  // the lane pair of block i: lanes i and i + 32
  const uint32_t par = lane >> 5, i = lane & 31;
  const uint32_t l8 = lane * 8;
  const uint32_t t1w = S + (lane & 31) * 8;
  const uint32_t t1r = S + (i * 33 + par) * 8;
  const uint32_t lwo = par * 128;
  const uint32_t glo = (uint32_t)(uintptr_t)p, ghi = (uint32_t)((uintptr_t)p >> 32);
  const uint32_t twlo = (uint32_t)(uintptr_t)twist, twhi = (uint32_t)((uintptr_t)twist >> 32);
  const u64* lw = twist + 2048;
  if constexpr (FWD) {
    const uint32_t t2wl = S + ((i & 15) * 65 + 33 * par) * 8;
    const uint32_t t2wh = S + ((i & 15) * 65 + 31 * par + 1) * 8;
    const uint32_t t2r = S + (lane ^ (lane >> 5)) * 8;
#define MI_RUN_FWD(n) \
  if constexpr (V == n) MI_TW_BODY_FWD_V##n(FWD_ARGS);
    MI_FOR_EACH_VARIANT(MI_RUN_FWD)
  } else {
    const uint32_t t4w = S + ((i & 15) * 65 + par) * 8;
    const uint32_t t4r = S + lane * 8;
    const uint32_t t1x = S + (lane + (lane >> 5)) * 8;
    const uint32_t t1y = S + ((i & 15) * 66 + 33 * par) * 8;
#define MI_RUN_INV(n) \
  if constexpr (V == n) MI_TW_BODY_INV_V##n(INV_ARGS);
    MI_FOR_EACH_VARIANT(MI_RUN_INV)
  }
}

__global__ void fill(u64* d, size_t n, u64 seed) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) {
    u64 x = (i + 1) * 0x9E3779B97F4A7C15ull ^ seed;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 32;
    d[i] = x % 0xFFFFFFFF00000001ull;
  }
}

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

template <int V>  // one wave per workgroup, as the library's ntt_tw_body_kernel
static void launch(bool fwd, u64* data, uint32_t batch, const u64* twist, hipStream_t s) {
  if (fwd)
    hipLaunchKernelGGL((probe_kernel<V, true, 1>), dim3(batch), dim3(64), 0, s, data, batch, twist);
  else
    hipLaunchKernelGGL((probe_kernel<V, false, 1>), dim3(batch), dim3(64), 0, s, data, batch, twist);
}

// variants past the generated ones: body 0 in the library's launch form (forward: one wave per workgroup, inverse: four)
static void launch_v(int v, bool fwd, u64* data, uint32_t batch, const u64* twist, hipStream_t s) {
  if (v == MI_N_VARIANTS) {
    if (fwd)
      hipLaunchKernelGGL((probe_kernel<0, true, 1>), dim3(batch), dim3(64), 0, s, data, batch, twist);
    else
      hipLaunchKernelGGL((probe_kernel<0, false, 4>), dim3((batch + 3) / 4), dim3(256), 0, s, data, batch, twist);
    return;
  }
#define MI_LAUNCH(n) \
  if (v == n) launch<n>(fwd, data, batch, twist, s);
  MI_FOR_EACH_VARIANT(MI_LAUNCH)
}

int main(int argc, char** argv) {
  const uint32_t batch = argc > 1 ? (uint32_t)atoi(argv[1]) : 8192;
  const int nv = MI_N_VARIANTS + 1;
  const size_t n = (size_t)batch * 2048;
  u64 *data, *twist, *ref;
  CK(hipMalloc(&data, n * 8));
  CK(hipMalloc(&ref, n * 8));
  // the real plan's twist tables are not needed for timing: any table gives the same instruction stream; for
  // the bit-identity check every variant runs on the same input and table
  CK(hipMalloc(&twist, 8192 * 8));
  hipStream_t s;
  CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipLaunchKernelGGL(fill, dim3(32), dim3(256), 0, s, twist, (size_t)8192, 11ull);
  // bit-identity vs variant 0 (fwd then inv)
  std::vector<u64> h0(n), h1(n);
  std::vector<int> same(nv, 1);
  for (int v = 0; v < nv; ++v) {
    hipLaunchKernelGGL(fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, data, n, 7ull);
    launch_v(v, true, data, batch, twist, s);
    launch_v(v, false, data, batch, twist, s);
    CK(hipStreamSynchronize(s));
    CK(hipMemcpy(v == 0 ? h0.data() : h1.data(), data, n * 8, hipMemcpyDeviceToHost));
    if (v) same[v] = memcmp(h0.data(), h1.data(), n * 8) == 0;
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int it = 0; it < 20000; ++it) launch_v(0, it & 1 ? false : true, data, batch, twist, s);  // clock settles
  // rounds visit the variants in a rotated order, so no variant always follows the same one (the power-capped
  // clock carries heat from one timed block into the next)
  // (at least 19 rounds, whatever the number of variants: the median of a variant is over its R timed blocks)
  const int K = 300, R = std::max(2 * nv + 1, 19);
  std::vector<std::vector<double>> fw(nv), iv(nv);
  for (int r = 0; r < R; ++r)
    for (int vi = 0; vi < nv; ++vi)
      for (int d = 0; d < 2; ++d) {
        const int v = (vi + r) % nv;
        CK(hipEventRecord(e0, s));
        for (int it = 0; it < K; ++it) launch_v(v, d == 0, data, batch, twist, s);
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        (d == 0 ? fw : iv)[v].push_back(ms * 1000.0 / K);
      }
  for (int v = 0; v < nv; ++v) {
    std::sort(fw[v].begin(), fw[v].end());
    std::sort(iv[v].begin(), iv[v].end());
    printf("{\"variant\": %d, \"batch\": %u, \"fwd_us_median\": %.2f, \"inv_us_median\": %.2f, \"fwd_us_min\": %.2f, "
           "\"inv_us_min\": %.2f, \"same_bits_as_v0\": %s}\n",
           v, batch, fw[v][R / 2], iv[v][R / 2], fw[v][0], iv[v][0], same[v] ? "true" : "false");
  }
  return 0;
}
