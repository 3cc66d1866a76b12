// c_api_pbs.cpp — the NTT external product / PBS family of the C ABI: the key conversion, the external product, CMUX
// and prepared GGSW entries, the prepared bootstrap key, the bootstrap / blind rotation entries and sample extraction.
#include <memory>
#include <new>

#include "scratch.hpp"
#include "c_api_internal.hpp"

using namespace mi::capi;

// polynomial sizes from which the PBS / external product run as device-wide passes with the accumulators in HBM
// (pbs_large.hip) instead of one fused workgroup per ciphertext (pbs_kernels.hip): at N = 8192 the fused kernel (1024
// lanes, 128 VGPRs, spilling) takes 994.5 ms per 1024 PBS of the 3_3 shape, the passes 786.7 ms; below it the fused
// kernels win (profiles/r3/fused_vs_large_pbs.txt)
static constexpr int LARGE_PATH_MIN_LOGN = 13;

int mi::capi::check_pbs_shape(const mi_ntt64_plan* plan, int k, int base_log, int level, int variant) {
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (variant != MI_NTT64_SOLINAS && variant != MI_NTT64_BNF) return fail(MI_ERR_INVALID_ARG, "unknown variant");
  if (level < 1 || base_log < 1 || base_log * level > 63)
    return fail(MI_ERR_INVALID_ARG, "decomposition must satisfy level >= 1, base_log >= 1, base_log*level < 64");
  // the compiled shapes (pbs_kernels.hip): N in {1024, 2048, 4096} with k in {1, 2}, N = 512 with k in {1, 4}
  // (PARAM_MESSAGE_1_CARRY_1), N = 8192 with k = 1 (PARAM_MESSAGE_3_CARRY_3)
  const int ln = plan->logn;
  // (PARAM_MESSAGE_1_CARRY_1); and N = 2^13 ... 2^17 with k in {1, 2} on the multi-kernel path of pbs_large.hip
  // (PARAM_MESSAGE_3_CARRY_3: N = 8192, 4_4: N = 65536)
  const bool shape_ok = plan->goldilocks && ((ln >= 10 && ln <= 12 && (k == 1 || k == 2)) ||
                                             (ln == 9 && (k == 1 || k == 4)) ||
                                             (ln >= LARGE_PATH_MIN_LOGN && ln <= 17 && (k == 1 || k == 2)));
  if (!shape_ok)
    return fail(MI_ERR_UNSUPPORTED,
                "external product / PBS run for the Solinas plan at N in {1024, 2048, 4096} with k in {1, 2}, "
                "N = 512 with k in {1, 4}, N in {8192, ..., 131072} with k in {1, 2}");
  return MI_OK;
}

// the split-transform tables of a plan (launch_ntt_split), or NULL: the large-N passes then run the window kernels.
// The tables live in the plan, so the pointer is valid for the plan's lifetime.
static const mi::SplitTw* split_of(const mi_ntt64_plan* plan) { return plan->d_split ? &plan->split : nullptr; }

// the twisted-transform bodies (pbs_tw.hip) cover level 1, base_log <= 31 (BNF and Solinas) on the
// Solinas N = 2048 plan; every other shape runs the generic kernels (pbs_kernels.hip)
bool mi::capi::twisted_ext_applies(const mi_ntt64_plan* plan, int variant, int k, int base_log, int level) {
  (void)variant;
  return k == 1 && level == 1 && base_log <= 31 && plan->twisted;
}

extern "C" {

int mi_bsk_to_ntt64(const mi_ntt64_plan* plan, const uint64_t* bsk_std, uint64_t* bsk_ntt, size_t n_polys,
                    unsigned in_modulus_width, int normalize, void* stream) {
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (n_polys == 0) return MI_OK;
  if (!bsk_std || !bsk_ntt) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (in_modulus_width > 64) return fail(MI_ERR_INVALID_ARG, "in_modulus_width > 64");
  if (!plan->goldilocks || plan->logn < 9 || plan->logn > 17)
    return fail(MI_ERR_UNSUPPORTED, "key conversion runs for the Solinas plan at N in {512, ..., 131072}");
  if (n_polys > 0x7FFFFFFFull) return fail(MI_ERR_INVALID_ARG, "too many polynomials");
  DeviceGuard g(plan->device);
  if (plan->twisted && in_modulus_width == 64) {  // the fused twisted-body conversion (ntt64_tw.hip)
    hipError_t e = mi::launch_ntt_tw_ms64(bsk_ntt, bsk_std, n_polys, normalize ? plan->d_twist_fn : plan->d_twist_f,
                                          (hipStream_t)stream);
    return e == hipSuccess ? MI_OK : hip_fail(e, "bsk conversion launch");
  }
  hipError_t e = plan->logn > 13  // the fused conversion kernel covers N <= 8192
                     ? mi::launch_bsk_to_ntt_large(plan->logn, bsk_ntt, bsk_std, n_polys, in_modulus_width,
                                                   normalize ? 1 : 0, plan->n_inv, plan->d_twid, (hipStream_t)stream,
                                                   split_of(plan))
                     : mi::launch_bsk_to_ntt(plan->logn, bsk_ntt, bsk_std, n_polys, in_modulus_width, normalize ? 1 : 0,
                                             plan->n_inv, plan->d_twid, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "bsk conversion launch");
}

static int ext_common(const mi_ntt64_plan* plan, bool cmux, uint64_t* out, uint64_t* in, const uint64_t* ggsw,
                      const uint32_t* gidx, size_t n_ggsw, int k, int base_log, int level, size_t batch, int variant,
                      void* stream, bool prepared = false) {
  int st = check_pbs_shape(plan, k, base_log, level, variant);
  if (st != MI_OK) return st;
  if (batch == 0) return MI_OK;
  if (!out || !in || !ggsw) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0x7FFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  if (n_ggsw == 0 || n_ggsw > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "GGSW count out of range");
  DeviceGuard g(plan->device);
  hipError_t e;
  if (twisted_ext_applies(plan, variant, k, base_log, level))
    e = mi::launch_ext_tw(cmux, variant == MI_NTT64_SOLINAS, out, in, ggsw, batch, base_log, plan->d_twist_f,
                          (hipStream_t)stream, gidx, (uint32_t)n_ggsw, prepared);
  else if (plan->logn >= LARGE_PATH_MIN_LOGN)
    e = mi::launch_ext_product_large(plan->logn, k, variant == MI_NTT64_BNF, cmux, level, out, in, ggsw, batch,
                                     base_log, plan->d_twid, plan->d_inv_twid, plan->n_inv, (hipStream_t)stream, gidx,
                                     (uint32_t)n_ggsw, split_of(plan));
  else
    e = mi::launch_ext_product(plan->logn, k, variant == MI_NTT64_BNF, cmux, level, out, in, ggsw, batch, base_log,
                               plan->d_twid, plan->d_inv_twid, plan->n_inv, (hipStream_t)stream, gidx,
                               (uint32_t)n_ggsw);
  return e == hipSuccess ? MI_OK : hip_fail(e, cmux ? "cmux launch" : "external product launch");
}

int mi_ntt64_ggsw_create(const mi_ntt64_plan* plan, const uint64_t* ggsw_list, size_t n_ggsw, int k, int base_log,
                         int level, int variant, void* stream, mi_ntt64_ggsw** out) {
  if (!out) return fail(MI_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  int st = check_pbs_shape(plan, k, base_log, level, variant);
  if (st != MI_OK) return st;
  if (!ggsw_list) return fail(MI_ERR_INVALID_ARG, "ggsw_list is NULL");
  if (n_ggsw == 0 || n_ggsw > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "GGSW count out of range");
  std::unique_ptr<mi_ntt64_ggsw> g(new (std::nothrow) mi_ntt64_ggsw);
  if (!g) return fail(MI_ERR_OOM, "host allocation failed");
  g->plan = plan;
  g->n_ggsw = n_ggsw;
  g->k = k;
  g->base_log = base_log;
  g->level = level;
  g->variant = variant;
  g->ggsw = ggsw_list;
  if (twisted_ext_applies(plan, variant, k, base_log, level) && mi::ext_tw_reads_w1p()) {
    const size_t polys = n_ggsw * 4;  // k = 1, level 1: (k + 1)^2 polynomials per GGSW
    DeviceGuard dg(plan->device);
    if (hipMalloc(&g->owned, polys * plan->n * sizeof(u64)) != hipSuccess)
      return fail(MI_ERR_OOM, "GGSW copy allocation failed");
    hipError_t e = mi::launch_prepare_tw_key(g->owned, ggsw_list, polys, 0, 0, (hipStream_t)stream, true);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) {
      (void)hipFree(g->owned);
      return hip_fail(e, "GGSW preparation");
    }
    g->ggsw = g->owned;
  }
  *out = g.release();
  return MI_OK;
}

int mi_ntt64_ggsw_destroy(mi_ntt64_ggsw* g) {
  if (!g) return MI_OK;
  if (g->owned) {
    DeviceGuard dg(g->plan->device);
    (void)hipFree(g->owned);
  }
  delete g;
  return MI_OK;
}

int mi_ntt64_ggsw_info(const mi_ntt64_ggsw* g, size_t* n_ggsw, int* k, int* base_log, int* level, int* variant) {
  if (!g) return fail(MI_ERR_INVALID_ARG, "ggsw is NULL");
  if (n_ggsw) *n_ggsw = g->n_ggsw;
  if (k) *k = g->k;
  if (base_log) *base_log = g->base_log;
  if (level) *level = g->level;
  if (variant) *variant = g->variant;
  return MI_OK;
}

int mi_ext_product_ntt64_prepared_batch(const mi_ntt64_ggsw* g, uint64_t* out_glwe, const uint64_t* in_glwe,
                                        const uint32_t* ggsw_index, size_t batch, void* stream) {
  if (!g) return fail(MI_ERR_INVALID_ARG, "ggsw is NULL");
  return ext_common(g->plan, false, out_glwe, const_cast<uint64_t*>(in_glwe), g->ggsw, ggsw_index,
                    ggsw_index ? g->n_ggsw : 1, g->k, g->base_log, g->level, batch, g->variant, stream, g->owned != nullptr);
}

int mi_cmux_ntt64_prepared_batch(const mi_ntt64_ggsw* g, uint64_t* ct0, uint64_t* ct1, const uint32_t* ggsw_index,
                                 size_t batch, void* stream) {
  if (!g) return fail(MI_ERR_INVALID_ARG, "ggsw is NULL");
  return ext_common(g->plan, true, ct0, ct1, g->ggsw, ggsw_index, ggsw_index ? g->n_ggsw : 1, g->k, g->base_log,
                    g->level, batch, g->variant, stream, g->owned != nullptr);
}

int mi_ext_product_ntt64_batch(const mi_ntt64_plan* plan, uint64_t* out_glwe, const uint64_t* in_glwe,
                               const uint64_t* ggsw_ntt, int k, int base_log, int level, size_t batch, int variant,
                               void* stream) {
  return ext_common(plan, false, out_glwe, const_cast<uint64_t*>(in_glwe), ggsw_ntt, nullptr, 1, k, base_log, level,
                    batch, variant, stream);
}

int mi_cmux_ntt64_batch(const mi_ntt64_plan* plan, uint64_t* ct0, uint64_t* ct1, const uint64_t* ggsw_ntt, int k,
                        int base_log, int level, size_t batch, int variant, void* stream) {
  return ext_common(plan, true, ct0, ct1, ggsw_ntt, nullptr, 1, k, base_log, level, batch, variant, stream);
}

int mi_ext_product_ntt64_batch_indexed(const mi_ntt64_plan* plan, uint64_t* out_glwe, const uint64_t* in_glwe,
                                       const uint64_t* ggsw_list, const uint32_t* ggsw_index, size_t n_ggsw, int k,
                                       int base_log, int level, size_t batch, int variant, void* stream) {
  if (!ggsw_index && batch) return fail(MI_ERR_INVALID_ARG, "ggsw_index is NULL");
  return ext_common(plan, false, out_glwe, const_cast<uint64_t*>(in_glwe), ggsw_list, ggsw_index, n_ggsw, k, base_log,
                    level, batch, variant, stream);
}

int mi_cmux_ntt64_batch_indexed(const mi_ntt64_plan* plan, uint64_t* ct0, uint64_t* ct1, const uint64_t* ggsw_list,
                                const uint32_t* ggsw_index, size_t n_ggsw, int k, int base_log, int level,
                                size_t batch, int variant, void* stream) {
  if (!ggsw_index && batch) return fail(MI_ERR_INVALID_ARG, "ggsw_index is NULL");
  return ext_common(plan, true, ct0, ct1, ggsw_list, ggsw_index, n_ggsw, k, base_log, level, batch, variant, stream);
}

}  // extern "C"

bool mi::capi::pbs_key_needs_copy(const mi_ntt64_plan* plan, int variant, int k, int base_log, int level) {
  return variant == MI_NTT64_BNF || twisted_ext_applies(plan, variant, k, base_log, level);
}

int mi::capi::prepare_pbs_key(const mi_ntt64_plan* plan, int variant, int k, int base_log, int level, u64* dst,
                              const u64* src, size_t count, hipStream_t stream) {
  const bool bnf = variant == MI_NTT64_BNF;
  hipError_t e = hipSuccess;
  if (twisted_ext_applies(plan, variant, k, base_log, level))
    e = mi::launch_prepare_tw_key(dst, src, count / plan->n, plan->n_inv, bnf ? 1 : 0, stream);
  else if (bnf)
    e = mi::launch_scale(dst, src, count, plan->n_inv, stream);
  else if (dst != src)
    e = hipMemcpyAsync(dst, src, count * sizeof(u64), hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "bootstrap key preparation");
}

extern "C" {

int mi_pbs_ntt64_key_create(const mi_ntt64_plan* plan, const uint64_t* bsk_ntt, size_t n_lwe, int k, int base_log,
                            int level, int variant, void* stream, mi_pbs_ntt64_key** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  int st = check_pbs_shape(plan, k, base_log, level, variant);
  if (st != MI_OK) return st;
  if (n_lwe == 0 || n_lwe > 0xFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "n_lwe out of range");
  if (!bsk_ntt) return fail(MI_ERR_INVALID_ARG, "bsk is NULL");
  mi_pbs_ntt64_key* key = new (std::nothrow) mi_pbs_ntt64_key;
  if (!key) return fail(MI_ERR_OOM, "host allocation failed");
  key->plan = plan;
  key->n_lwe = n_lwe;
  key->k = k;
  key->base_log = base_log;
  key->level = level;
  key->variant = variant;
  key->bsk = bsk_ntt;
  if (pbs_key_needs_copy(plan, variant, k, base_log, level)) {
    const size_t count = n_lwe * (size_t)(k + 1) * (k + 1) * level * plan->n;
    DeviceGuard g(plan->device);
    if (hipMalloc(&key->owned, count * sizeof(u64)) != hipSuccess) {
      delete key;
      return fail(MI_ERR_OOM, "bootstrap key copy allocation failed");
    }
    // ordered after the work that produced bsk_ntt on `stream` (the caller's stream)
    st = prepare_pbs_key(plan, variant, k, base_log, level, key->owned, bsk_ntt, count, (hipStream_t)stream);
    if (st != MI_OK) {
      (void)hipFree(key->owned);
      delete key;
      return st;
    }
    key->bsk = key->owned;
  }
  *out_key = key;
  return MI_OK;
}

int mi_pbs_ntt64_key_destroy(mi_pbs_ntt64_key* key) {
  if (!key) return MI_OK;
  if (key->owned) {
    DeviceGuard g(key->plan->device);
    (void)hipFree(key->owned);
  }
  delete key;
  return MI_OK;
}

}  // extern "C"

// every NTT bootstrap entry point: the accumulator's start and the output form come in `io` (ntt64_launch.hpp PbsIo);
// lwe_out is ignored when io.glwe_out is set
static int pbs_common(const mi_pbs_ntt64_key* key, uint64_t* lwe_out, const uint64_t* lwe_in, mi::PbsIo io,
                      size_t batch, int ms_mode, void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (ms_mode != MI_MS_STANDARD && ms_mode != MI_MS_CENTERED && ms_mode != MI_MS_PRE_SWITCHED)
    return fail(MI_ERR_INVALID_ARG, "unknown ms_mode");
  if (ms_mode == MI_MS_CENTERED && key->variant != MI_NTT64_BNF)
    return fail(MI_ERR_INVALID_ARG, "centered modulus switch applies to native-modulus (BNF) inputs");
  if (batch == 0) return MI_OK;
  if ((!lwe_out && !io.glwe_out) || !lwe_in || !io.lut) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0x7FFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const mi_ntt64_plan* plan = key->plan;
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(plan->device);
  if (key->variant == MI_NTT64_SOLINAS && twisted_ext_applies(plan, key->variant, key->k, key->base_log, key->level)) {
    // Solinas on the twisted engine: the body reads switched values (the caller's, or switched here
    // into stream-ordered scratch by ms_non_native)
    const size_t count = batch * (key->n_lwe + 1);
    u64* sw = nullptr;
    if (ms_mode != MI_MS_PRE_SWITCHED) {
      if (mi::scratch_alloc((void**)&sw, count * sizeof(u64), s) != hipSuccess)
        return fail(MI_ERR_OOM, "scratch allocation failed");
      hipError_t e = mi::launch_ms_non_native(sw, lwe_in, count, s);
      if (e != hipSuccess) {
        (void)mi::scratch_free(sw, s);
        return hip_fail(e, "modulus switch launch");
      }
    }
    hipError_t e = mi::launch_pbs_tw_sol(lwe_out, sw ? sw : lwe_in, io, key->bsk, key->n_lwe, batch, key->base_log,
                                         plan->d_twist_f, s);
    if (sw) (void)mi::scratch_free(sw, s);
    return e == hipSuccess ? MI_OK : hip_fail(e, "pbs launch");
  }
  u64* lifted = nullptr;  // PRE_SWITCHED: stream-ordered copy lifted back to the standard switch
  if (ms_mode == MI_MS_PRE_SWITCHED) {
    const size_t count = batch * (key->n_lwe + 1);
    if (mi::scratch_alloc((void**)&lifted, count * sizeof(u64), s) != hipSuccess)
      return fail(MI_ERR_OOM, "scratch allocation failed");
    hipError_t e = mi::launch_lift_switched(lifted, lwe_in, count, key->variant == MI_NTT64_BNF, plan->logn, s);
    if (e != hipSuccess) {
      (void)mi::scratch_free(lifted, s);
      return hip_fail(e, "lift launch");
    }
    lwe_in = lifted;
    ms_mode = MI_MS_STANDARD;
  }
  hipError_t e;
  if (twisted_ext_applies(plan, key->variant, key->k, key->base_log, key->level))
    e = mi::launch_pbs_tw(lwe_out, lwe_in, io, key->bsk, key->n_lwe, batch, key->base_log, plan->d_twist_f,
                          ms_mode == MI_MS_CENTERED, s);
  else if (plan->logn >= LARGE_PATH_MIN_LOGN)
    e = mi::launch_pbs_large(plan->logn, key->k, key->variant == MI_NTT64_BNF, key->level, lwe_out, lwe_in, io,
                             key->bsk, key->n_lwe, batch, key->base_log, plan->d_twid, plan->d_inv_twid,
                             ms_mode == MI_MS_CENTERED, s, split_of(plan));
  else
    e = mi::launch_pbs(plan->logn, key->k, key->variant == MI_NTT64_BNF, key->level, lwe_out, lwe_in, io, key->bsk, key->n_lwe, batch,
                       key->base_log, plan->d_twid, plan->d_inv_twid, ms_mode == MI_MS_CENTERED, s);
  if (lifted) (void)mi::scratch_free(lifted, s);
  return e == hipSuccess ? MI_OK : hip_fail(e, "pbs launch");
}

extern "C" {

int mi_pbs_ntt64_batch(const mi_pbs_ntt64_key* key, uint64_t* lwe_out, const uint64_t* lwe_in, const uint64_t* lut,
                       size_t batch, int ms_mode, void* stream) {
  mi::PbsIo io;
  io.lut = lut;
  if (!lwe_out && batch) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  return pbs_common(key, lwe_out, lwe_in, io, batch, ms_mode, stream);
}

int mi_pbs_ntt64_batch_lut_indexed(const mi_pbs_ntt64_key* key, uint64_t* lwe_out, const uint64_t* lwe_in,
                                   const uint64_t* lut_list, const uint32_t* lut_index, size_t n_lut, size_t batch,
                                   int ms_mode, void* stream) {
  if (batch && !lwe_out) return fail(MI_ERR_INVALID_ARG, "lwe_out is NULL");
  if (n_lut == 0 || n_lut > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "n_lut out of range");
  if (!lut_index && n_lut < batch) return fail(MI_ERR_INVALID_ARG, "per-item LUTs: n_lut < batch");
  mi::PbsIo io;
  io.lut = lut_list;
  io.lut_idx = lut_index;
  io.n_lut = (uint32_t)n_lut;
  io.per_item = lut_index ? 0 : 1;  // no index array: item b uses GLWE b
  return pbs_common(key, lwe_out, lwe_in, io, batch, ms_mode, stream);
}

int mi_blind_rotate_ntt64_batch(const mi_pbs_ntt64_key* key, uint64_t* acc_glwe, const uint64_t* lwe_in, size_t batch,
                                int ms_mode, void* stream) {
  if (batch && !acc_glwe) return fail(MI_ERR_INVALID_ARG, "acc_glwe is NULL");
  mi::PbsIo io;
  io.lut = acc_glwe;
  io.per_item = 1;
  io.glwe_out = acc_glwe;
  return pbs_common(key, nullptr, lwe_in, io, batch, ms_mode, stream);
}

int mi_sample_extract_batch(uint64_t* lwe_out, const uint64_t* glwe, size_t polynomial_size, int k, size_t batch,
                            size_t nth_first, size_t nth_stride, size_t nth_count, uint64_t modulus, int device,
                            void* stream) {
  if (polynomial_size < 2 || (polynomial_size & (polynomial_size - 1)) != 0 || polynomial_size > ((size_t)1 << 31))
    return fail(MI_ERR_INVALID_ARG, "polynomial size must be a power of two in [2, 2^31]");
  if (k < 1) return fail(MI_ERR_INVALID_ARG, "GLWE dimension must be >= 1");
  if (batch == 0 || nth_count == 0) return MI_OK;
  if (!lwe_out || !glwe) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  // glwe_sample_extraction.rs:89-160 takes MonomialDegree < N (opposite_count = N - nth - 1 would underflow)
  if (nth_first >= polynomial_size || (nth_count > 1 && nth_stride > (polynomial_size - 1 - nth_first) / (nth_count - 1)))
    return fail(MI_ERR_INVALID_ARG, "a monomial degree is >= the polynomial size");
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_HIP, "hipSetDevice failed");
  const hipError_t e = mi::launch_sample_extract(lwe_out, glwe, __builtin_ctzll(polynomial_size), k, batch, nth_first,
                                                 nth_stride, nth_count, modulus, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "sample extraction launch");
}

}  // extern "C"
