// pbs_passes.hip — the one kernel of pbs_passes.hpp, shared by pbs_large.hip, fft64_generic.hip and pbs128.hip
#include "pbs_passes.hpp"

#include "pbs_device.hpp"

namespace mi {

// centered_binary_ms_body_correction_to_add (algorithms/modulus_switch.rs:60-104), one workgroup per ciphertext
__global__ __launch_bounds__(256) void body_correction_kernel(u64* __restrict__ corr, const u64* __restrict__ lwe,
                                                              uint32_t n_lwe, unsigned log_mod) {
  __shared__ u64 sh[512];
  const u64 v = pbs::centered_body_correction<256>(lwe + (uint64_t)blockIdx.x * (n_lwe + 1), n_lwe, log_mod,
                                                   (int)threadIdx.x, sh);
  if (threadIdx.x == 0) corr[blockIdx.x] = v;
}

hipError_t launch_body_correction(uint64_t* corr, const uint64_t* lwe, uint32_t n_lwe, unsigned log_mod, uint32_t nb,
                                  hipStream_t s) {
  hipLaunchKernelGGL(body_correction_kernel, dim3(nb), dim3(256), 0, s, corr, lwe, n_lwe, log_mod);
  return hipGetLastError();
}

}  // namespace mi
