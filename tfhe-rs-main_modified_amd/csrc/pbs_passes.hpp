// pbs_passes.hpp — the host scaffolding of the engines that run a blind rotation as device-wide passes over
// accumulators held in HBM (pbs_large.hip, fft64_generic.hip, pbs128.hip): the chunk and lane plan, the driver that
// issues the passes over the caller's stream and pooled side streams, and the small launch helpers the three share.
// Scratch allocation and layout stay with each engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "scratch.hpp"

namespace mi {

// ---- the plan: pure host functions, no HIP call (tests/cpp/lane_plan_check.cpp runs them on a CPU) ----
// ciphertexts per chunk: one chunk's scratch (item_bytes each) stays below ~4 GiB (of 288 GB), one item at the least
inline size_t chunk_items(size_t item_bytes, size_t batch) {
  return std::max<size_t>(1, std::min(batch, ((size_t)4 << 30) / item_bytes));
}

// lanes for a chunk of nb ciphertexts: one below 64; else the engine's measured default for its shape (DESIGN.md
// section 4; no environment override) clamped to 1 ... 1 + StreamFork::MAX_SIDE, with >= 16 ciphertexts per lane
inline int lanes_wanted(uint32_t nb, int dflt) {
  const int lanes = std::max(1, std::min(dflt, 1 + StreamFork::MAX_SIDE));
  return nb >= 64 ? std::min(lanes, (int)(nb / 16)) : 1;
}

// lane j of `lanes`: ciphertexts [off, off + n) of the chunk; the first nb % lanes lanes take one more
struct LanePart { uint32_t off, n; };
inline LanePart lane_part(uint32_t nb, int lanes, int j) {
  const uint32_t q = nb / (uint32_t)lanes, r = nb % (uint32_t)lanes, i = (uint32_t)j;
  return LanePart{i * q + std::min(i, r), q + (i < r ? 1u : 0u)};
}

__device__ __forceinline__ uint64_t grid_stride_start() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t grid_stride() { return (uint64_t)gridDim.x * blockDim.x; }

// workgroups of 256 threads for a grid-stride pass over `total` elements
inline unsigned blocks_for(uint64_t total) { return (unsigned)std::min<uint64_t>((total + 255) / 256, 65536); }

// corr[b] = centered_binary_ms_body_correction_to_add of the nb ciphertexts at lwe (pbs_passes.hip)
hipError_t launch_body_correction(uint64_t* corr, const uint64_t* lwe, uint32_t n_lwe, unsigned log_mod, uint32_t nb,
                                  hipStream_t s);

// one lane's share of a chunk: ciphertexts [b0, b0 + nb) of the caller's batch, which are [off, off + nb) of the chunk
// (where the lane's scratch slices start), and the stream its launches go to
struct Lane { size_t b0; uint32_t off, nb; hipStream_t st; };

// The blind rotations of `batch` ciphertexts, `chunk` at a time.  A chunk runs as lanes_wanted(nb, dflt_lanes) lanes
// (fewer when a side stream cannot be had; none is forked for one lane), the first on the caller's stream `s`, the
// others on pooled side streams, their launches interleaved: init(L) for every lane, step(L, i) for every lane at each
// of the n_steps CMUX steps, finish(L) for every lane.  Each ciphertext's rotation is independent, so the lanes share
// nothing but the key, and one lane's memory-bound passes overlap another's transform bodies.  The first error ends the
// issue and is returned; `s` is ordered after the side streams also then (the caller frees the scratch on `s`).
template <class Init, class Step, class Finish>
hipError_t run_blind_rotation(size_t batch, size_t chunk, uint32_t n_steps, int dflt_lanes, hipStream_t s, Init init,
                              Step step, Finish finish) {
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < batch && e == hipSuccess; c0 += chunk) {
    const uint32_t nb = (uint32_t)std::min(chunk, batch - c0);
    StreamFork fork;
    const int want = lanes_wanted(nb, dflt_lanes);
    if (want > 1) (void)fork.fork(s, want - 1);
    const int lanes = 1 + fork.sides();
    Lane L[1 + StreamFork::MAX_SIDE];
    for (int j = 0; j < lanes; ++j) {
      const LanePart p = lane_part(nb, lanes, j);
      L[j] = Lane{c0 + p.off, p.off, p.n, j == 0 ? s : fork.side(j - 1)};
    }
    for (int j = 0; j < lanes && e == hipSuccess; ++j) e = init(L[j]);
    for (uint32_t i = 0; i < n_steps && e == hipSuccess; ++i)
      for (int j = 0; j < lanes && e == hipSuccess; ++j) e = step(L[j], i);
    for (int j = 0; j < lanes && e == hipSuccess; ++j) e = finish(L[j]);
    const hipError_t ej = fork.join();
    if (e == hipSuccess) e = ej;
  }
  return e;
}

}  // namespace mi
