// c_api_ms_noise.cpp — the modulus switch noise reduction family of the C ABI: the prepared key of encryptions of
// zero (mi_ms_noise_key) and the measure / choose / improve / improve-and-switch entries (kernels:
// ms_noise_reduction.hip).
#include <cmath>
#include <new>

#include "ms_noise_launch.hpp"
#include "c_api_internal.hpp"

using namespace mi::capi;

struct mi_ms_noise_key {
  int device = 0;
  mi::MsNoiseGeometry geo;
  double bound = 0.0, r_sigma = 0.0, input_variance = 0.0;  // as given (mi_ms_noise_key_info)
  mi::msn::Params params{};                                 // what the kernels are told
  uint64_t* tiles = nullptr;                                // the prepared copy (ms_noise_launch.hpp)
};

namespace {

// the checks every batch entry shares, in their order; MI_OK with *run = false means there is nothing to do
int check_batch_entry(const mi_ms_noise_key* key, const void* lwe_in, size_t batch, int log_modulus, bool* run) {
  *run = false;
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  // modulus_switch asserts log_modulus <= Scalar::BITS and is the identity there (fft_impl/common.rs:10-23)
  if (log_modulus < 1 || log_modulus > 64) return fail(MI_ERR_INVALID_ARG, "log_modulus must be in [1, 64]");
  if (batch == 0) return MI_OK;
  if (!lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  *run = true;
  return MI_OK;
}

int run(const mi_ms_noise_key* key, const mi::MsNoiseOut& out, const uint64_t* lwe_in, size_t batch, int log_modulus,
        void* stream) {
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e =
      mi::launch_ms_noise(out, key->tiles, key->geo, key->params, lwe_in, batch, log_modulus, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "modulus switch noise reduction launch");
}

}  // namespace

extern "C" {

int mi_ms_noise_key_create(const uint64_t* zeros, size_t lwe_dim, size_t zeros_count, double ms_bound,
                           double ms_r_sigma_factor, double ms_input_variance, int device, void* stream,
                           mi_ms_noise_key** out_key) {
  if (out_key) *out_key = nullptr;
  if (!zeros) return fail(MI_ERR_INVALID_ARG, "zeros is NULL");
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  if (lwe_dim == 0 || lwe_dim > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "lwe dimension out of range");
  // choose_candidate's assert_ne (modulus_switch_noise_reduction.rs:126-130)
  if (zeros_count == 0) return fail(MI_ERR_INVALID_ARG, "expected at least one encryption of zero");
  if (zeros_count > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "zeros_count out of range");
  if (std::isnan(ms_bound) || std::isnan(ms_r_sigma_factor) || std::isnan(ms_input_variance))
    return fail(MI_ERR_INVALID_ARG, "ms_bound, ms_r_sigma_factor and ms_input_variance must not be NaN");
  if (ms_r_sigma_factor < 0.0 || ms_input_variance < 0.0)
    return fail(MI_ERR_INVALID_ARG, "ms_r_sigma_factor and ms_input_variance must not be negative");

  mi_ms_noise_key* key = new (std::nothrow) mi_ms_noise_key;
  if (!key) return fail(MI_ERR_OOM, "host allocation failed");
  key->device = device;
  key->geo = mi::MsNoiseGeometry{lwe_dim, zeros_count};
  key->bound = ms_bound;
  key->r_sigma = ms_r_sigma_factor;
  key->input_variance = ms_input_variance;
  // Variance::get_modular_variance (dispersion.rs:258-262): variance * modulus * modulus, modulus = 2^64 as f64
  const double modulus = 18446744073709551616.0;
  key->params = mi::msn::Params{ms_bound, ms_r_sigma_factor, ms_input_variance * modulus * modulus};

  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(device);
  if (!g.ok) {
    delete key;
    return fail(MI_ERR_INVALID_ARG, "bad device");
  }
  if (hipMalloc(&key->tiles, mi::ms_noise_key_bytes(key->geo)) != hipSuccess) {
    delete key;
    return fail(MI_ERR_OOM, "modulus switch noise reduction key allocation failed");
  }
  hipError_t e = mi::launch_ms_noise_prepare(key->tiles, zeros, key->geo, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(key->tiles);
    delete key;
    return hip_fail(e, "modulus switch noise reduction key preparation");
  }
  *out_key = key;
  return MI_OK;
}

int mi_ms_noise_key_destroy(mi_ms_noise_key* key) {
  if (!key) return MI_OK;
  {
    DeviceGuard g(key->device);
    if (key->tiles) (void)hipFree(key->tiles);
  }
  delete key;
  return MI_OK;
}

int mi_ms_noise_key_info(const mi_ms_noise_key* key, size_t* lwe_dim, size_t* zeros_count, double* ms_bound,
                         double* ms_r_sigma_factor, double* ms_input_variance) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (lwe_dim) *lwe_dim = key->geo.lwe_dim;
  if (zeros_count) *zeros_count = key->geo.zeros_count;
  if (ms_bound) *ms_bound = key->bound;
  if (ms_r_sigma_factor) *ms_r_sigma_factor = key->r_sigma;
  if (ms_input_variance) *ms_input_variance = key->input_variance;
  return MI_OK;
}

int mi_lwe_ms_noise_measure_batch(const mi_ms_noise_key* key, double* measures, const uint64_t* lwe_in, size_t batch,
                                  int log_modulus, int all_candidates, void* stream) {
  bool go;
  const int st = check_batch_entry(key, lwe_in, batch, log_modulus, &go);
  if (st != MI_OK || !go) return st;
  if (!measures) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  mi::MsNoiseOut out;
  out.measures = measures;
  out.all_candidates = all_candidates != 0;
  return run(key, out, lwe_in, batch, log_modulus, stream);
}

int mi_lwe_ms_noise_choose_batch(const mi_ms_noise_key* key, int64_t* candidate, int32_t* satisfied,
                                 const uint64_t* lwe_in, size_t batch, int log_modulus, void* stream) {
  bool go;
  const int st = check_batch_entry(key, lwe_in, batch, log_modulus, &go);
  if (st != MI_OK || !go) return st;
  if (!candidate || !satisfied) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  mi::MsNoiseOut out;
  out.candidate = candidate;
  out.satisfied = satisfied;
  return run(key, out, lwe_in, batch, log_modulus, stream);
}

int mi_lwe_ms_noise_improve_batch(const mi_ms_noise_key* key, uint64_t* lwe_out, const uint64_t* lwe_in, size_t batch,
                                  int log_modulus, int64_t* candidate, int32_t* satisfied, void* stream) {
  bool go;
  const int st = check_batch_entry(key, lwe_in, batch, log_modulus, &go);
  if (st != MI_OK || !go) return st;
  if (!lwe_out) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  mi::MsNoiseOut out;
  out.lwe = lwe_out;
  out.candidate = candidate;
  out.satisfied = satisfied;
  return run(key, out, lwe_in, batch, log_modulus, stream);
}

int mi_lwe_ms_noise_improve_and_switch_batch(const mi_ms_noise_key* key, uint64_t* switched, const uint64_t* lwe_in,
                                             size_t batch, int log_modulus, void* stream) {
  bool go;
  const int st = check_batch_entry(key, lwe_in, batch, log_modulus, &go);
  if (st != MI_OK || !go) return st;
  if (!switched) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  mi::MsNoiseOut out;
  out.lwe = switched;
  out.switched = 1;
  return run(key, out, lwe_in, batch, log_modulus, stream);
}

}  // extern "C"
