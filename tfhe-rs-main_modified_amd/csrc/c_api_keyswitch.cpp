// c_api_keyswitch.cpp — the keyswitch family of the C ABI: the four prepared keys (mi_lwe_ksk, mi_lwe_ksk32,
// mi_lwe_pksk, mi_lwe_pfpksk_list) over one shared core, the two LWE modulus switches, the packing keyswitch and the GLWE compression
// (kernels: keyswitch.hip, packing_keyswitch.hip), and their u128 twins of the noise-squashing compression
// (mi_lwe_pksk128, packing_keyswitch128.hip).
#include <new>
#include <string>

#include "scratch.hpp"
#include "keyswitch_launch.hpp"
#include "c_api_internal.hpp"

namespace mi {
namespace capi {

// what the three keys are: the shape lives in `geo` alone (the *_info entries answer from it)
struct KsKey {
  int device = 0;
  mi::KsGeometry geo;    // what the launches are told
  void* frag = nullptr;  // byte-plane MFMA fragments (keyswitch.hip)
};

}  // namespace capi
}  // namespace mi

using namespace mi::capi;

struct mi_lwe_ksk {
  KsKey core;  // KsMode::Native
};

struct mi_lwe_ksk32 {
  KsKey core;  // KsMode::Ks32: the fragments of the zero-extended u32 key words
};

struct mi_lwe_pksk {
  KsKey core;  // KsMode::Packing: (k + 1) N key columns, the body at column k N
  int glwe_dim = 0;
  size_t polynomial_size = 0;
};

struct mi_lwe_pfpksk_list {
  KsKey core;  // KsMode::Pfpks: n_keys (k + 1) N key columns over in_dim + 1 blocks, no body column
  int glwe_dim = 0;
  size_t polynomial_size = 0;
};

struct mi_lwe_pksk128 {
  int device = 0;
  mi::Pks128Geometry geo;
  void* frag = nullptr;  // 16 signed-byte planes per key word (packing_keyswitch128.hip)
  int glwe_dim = 0;
  size_t polynomial_size = 0;
};

namespace {

// The range rules of the three creates, in their common order.  `own` is the message of the caller's own failed rule
// (the output dimension, the KS32 output modulus, the GLWE shape) or nullptr: those rules sit between the input
// dimension and the decomposition.  `top`: the largest base_log * level of the key kind.
// `blocks`: the key's blocks of `level` rows, the GEMM's depth in digits: in_dim, or in_dim + 1 where the body word is
// decomposed too (0: in_dim).
int check_ks_range(size_t in_dim, const char* own, int base_log, int level, int top, size_t blocks = 0) {
  if (in_dim == 0 || in_dim > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "lwe dimension out of range");
  if (own) return fail(MI_ERR_INVALID_ARG, own);
  // SignedDecomposer::new (decomposer.rs): base_log * level < Scalar::BITS, both >= 1; KS32 (lwe_keyswitch.rs:
  // 378-384): base_log * level <= OutputScalar::BITS
  if (base_log < 1 || level < 1 || level > top || base_log * level > top)
    return fail(MI_ERR_INVALID_ARG, "decomposition base_log * level must be in [1, " + std::to_string(top) + "]");
  // u128 keys only (top = 127): a digit is held in an int64 and split into at most 8 signed bytes
  if (base_log > 63) return fail(MI_ERR_UNSUPPORTED, "base_log above 63 is not supported (a digit must fit 64 bits)");
  // exact int32 accumulation on the int8 matrix cores: GEMM depth in_dim * level * bytes-per-digit < 2^17
  if ((double)(blocks ? blocks : in_dim) * level * mi::ks_digit_bytes_per_term(base_log) >= 131072.0)
    return fail(MI_ERR_UNSUPPORTED, blocks ? "(in_dim + 1) * level * ceil((base_log + 1) / 8) must stay below 2^17"
                                           : "in_dim * level * ceil((base_log + 1) / 8) must stay below 2^17");
  return MI_OK;
}

// Fills k from the key words in the reference layout: the fragments are prepared on `s`, ordered after the work that
// produced `words` there, and `s` is synchronised.  `what` names the key in the messages.  On failure k owns nothing.
int ks_key_init(KsKey& k, const void* words, const mi::KsGeometry& geo, int device, hipStream_t s, const char* what) {
  k.device = device;
  k.geo = geo;
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  if (hipMalloc(&k.frag, mi::ks_key_bytes(geo)) != hipSuccess) {
    k.frag = nullptr;
    return fail(MI_ERR_OOM, std::string(what) + " allocation failed");
  }
  hipError_t e = mi::launch_ksk_prepare(k.frag, words, geo, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(k.frag);
    k.frag = nullptr;
    return hip_fail(e, (std::string(what) + " preparation").c_str());
  }
  return MI_OK;
}

// the tail of the three creates: the handle, its prepared key, the unwind
template <class Handle>
int ks_create(Handle** out_key, const void* words, const mi::KsGeometry& geo, int device, void* stream,
              const char* what) {
  Handle* key = new (std::nothrow) Handle;
  if (!key) return fail(MI_ERR_OOM, "host allocation failed");
  const int st = ks_key_init(key->core, words, geo, device, (hipStream_t)stream, what);
  if (st != MI_OK) {
    delete key;
    return st;
  }
  *out_key = key;
  return MI_OK;
}

template <class Handle>
int ks_destroy(Handle* key) {
  if (!key) return MI_OK;
  {
    DeviceGuard g(key->core.device);
    if (key->core.frag) (void)hipFree(key->core.frag);
  }
  delete key;
  return MI_OK;
}

// out: u64 (Native) or u32 (Ks32) rows, as k.geo.mode says
int run_keyswitch(const KsKey& k, void* out, const uint64_t* in, size_t batch, void* stream) {
  if (batch == 0) return MI_OK;
  if (!out || !in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0x3FFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(k.device);
  mi::ScratchBuf digits(mi::ks_digit_bytes(k.geo, batch), s);  // int8 digit fragments, stream-ordered scratch
  if (!digits.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  const hipError_t e = mi::launch_keyswitch(out, in, k.frag, digits.ptr(), batch, k.geo, s);
  return e == hipSuccess ? MI_OK : hip_fail(e, "keyswitch launch");
}

// shared checks of the two LWE modulus switches: the standard switch is defined for 1 <= log_modulus <= BITS (identity at
// BITS, fft_impl/common.rs:10-23); the centered one computes 1 << (BITS - log_modulus - 1) (modulus_switch.rs:95), so
// it needs log_modulus < BITS (the reference's shift underflows there)
int check_lwe_ms(const void* switched, const void* lwe_in, size_t lwe_dim, size_t batch, int log_modulus, int ms_mode,
                 int bits) {
  if (!switched || !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (lwe_dim == 0 || lwe_dim > 0xFFFFFFull || batch > 0xFFFFFFFFull)
    return fail(MI_ERR_INVALID_ARG, "lwe dimension or batch out of range");
  if (ms_mode != MI_MS_STANDARD && ms_mode != MI_MS_CENTERED)
    return fail(MI_ERR_INVALID_ARG, "ms_mode must be MI_MS_STANDARD or MI_MS_CENTERED");
  const int top = ms_mode == MI_MS_CENTERED ? bits - 1 : bits;
  if (log_modulus < 1 || log_modulus > top)
    return fail(MI_ERR_INVALID_ARG, "log_modulus must be in [1, " + std::to_string(top) + "] for this ms_mode");
  return MI_OK;
}

// compress's asserts (compressed_modulus_switched_glwe_ciphertext.rs:191-203) and PackedIntegers::pack's
// (packed_integers.rs:43-44)
int check_glwe_compress(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus, int bits = 64) {
  if (polynomial_size == 0 || glwe_dim < 1 || polynomial_size > 0xFFFFFFull ||
      ((size_t)glwe_dim + 1) * polynomial_size > 0xFFFFFFull)
    return fail(MI_ERR_INVALID_ARG, "glwe size out of range");
  if (bodies_count > polynomial_size) return fail(MI_ERR_INVALID_ARG, "bodies_count must be <= polynomial_size");
  if (log_modulus < 1 || log_modulus > bits)
    return fail(MI_ERR_INVALID_ARG, "log_modulus must be in [1, " + std::to_string(bits) + "]");
  return MI_OK;
}

}  // namespace

extern "C" {

// ---- LWE keyswitch (tfhe/src/core_crypto/algorithms/lwe_keyswitch.rs:137-227) -----------------------

int mi_lwe_ksk_create(const uint64_t* ksk, size_t in_dim, size_t out_dim, int base_log, int level, int device,
                      void* stream, mi_lwe_ksk** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!ksk) return fail(MI_ERR_INVALID_ARG, "ksk is NULL");
  const char* own = out_dim == 0 || out_dim > 0xFFFFFFull ? "lwe dimension out of range" : nullptr;
  const int st = check_ks_range(in_dim, own, base_log, level, 63);
  if (st != MI_OK) return st;
  const mi::KsGeometry geo{mi::KsMode::Native, in_dim, out_dim + 1, base_log, level, 64, out_dim};
  return ks_create(out_key, ksk, geo, device, stream, "keyswitch key");
}

int mi_lwe_ksk_destroy(mi_lwe_ksk* key) { return ks_destroy(key); }

int mi_lwe_ksk_info(const mi_lwe_ksk* key, size_t* in_dim, size_t* out_dim, int* base_log, int* level) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  const mi::KsGeometry& g = key->core.geo;
  if (in_dim) *in_dim = g.in_dim;
  if (out_dim) *out_dim = g.out_size - 1;
  if (base_log) *base_log = g.base_log;
  if (level) *level = g.level;
  return MI_OK;
}

int mi_lwe_keyswitch_batch(const mi_lwe_ksk* key, uint64_t* lwe_out, const uint64_t* lwe_in, size_t batch,
                           void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  return run_keyswitch(key->core, lwe_out, lwe_in, batch, stream);
}

// ---- KS32: keyswitch_lwe_ciphertext_with_scalar_change (lwe_keyswitch.rs:331-447) ------------------------------
// The keyswitch of the HPU KS32 parameter sets (shortint/parameters/v1_5/hpu.rs:57-76: 2048 -> 879, base 2^2, 8
// levels, post_keyswitch_ciphertext_modulus 2^21): u64 input LWEs of the native modulus, u32 key and output words
// with the power-of-two output modulus 2^out_modulus_log encoded in the MSBs, as the reference stores it.

int mi_lwe_ksk32_create(const uint32_t* ksk, size_t in_dim, size_t out_dim, int base_log, int level,
                        int out_modulus_log, int device, void* stream, mi_lwe_ksk32** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!ksk) return fail(MI_ERR_INVALID_ARG, "ksk is NULL");
  const char* own = nullptr;
  if (out_dim == 0 || out_dim > 0xFFFFFFull)
    own = "lwe dimension out of range";
  else if (out_modulus_log < 1 || out_modulus_log > 32)
    own = "output modulus must be 2^w with 1 <= w <= 32";
  const int st = check_ks_range(in_dim, own, base_log, level, 32);
  if (st != MI_OK) return st;
  const mi::KsGeometry geo{mi::KsMode::Ks32, in_dim, out_dim + 1, base_log, level, out_modulus_log, out_dim};
  return ks_create(out_key, ksk, geo, device, stream, "keyswitch key");
}

int mi_lwe_ksk32_destroy(mi_lwe_ksk32* key) { return ks_destroy(key); }

int mi_lwe_ksk32_info(const mi_lwe_ksk32* key, size_t* in_dim, size_t* out_dim, int* base_log, int* level,
                      int* out_modulus_log) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  const mi::KsGeometry& g = key->core.geo;
  if (in_dim) *in_dim = g.in_dim;
  if (out_dim) *out_dim = g.out_size - 1;
  if (base_log) *base_log = g.base_log;
  if (level) *level = g.level;
  if (out_modulus_log) *out_modulus_log = g.out_log;
  return MI_OK;
}

int mi_lwe_keyswitch32_batch(const mi_lwe_ksk32* key, uint32_t* lwe_out, const uint64_t* lwe_in, size_t batch,
                             void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  return run_keyswitch(key->core, lwe_out, lwe_in, batch, stream);
}

int mi_lwe_modulus_switch32_batch(uint64_t* switched, const uint32_t* lwe_in, size_t lwe_dim, size_t batch,
                                  int log_modulus, int ms_mode, int device, void* stream) {
  if (batch == 0) return MI_OK;
  int st = check_lwe_ms(switched, lwe_in, lwe_dim, batch, log_modulus, ms_mode, 32);
  if (st != MI_OK) return st;
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  hipError_t e = mi::launch_lwe_ms32(switched, lwe_in, lwe_dim, batch, log_modulus, ms_mode == MI_MS_CENTERED,
                                     (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "modulus switch launch");
}

int mi_lwe_modulus_switch_batch(uint64_t* switched, const uint64_t* lwe_in, size_t lwe_dim, size_t batch,
                                int log_modulus, int ms_mode, int device, void* stream) {
  if (batch == 0) return MI_OK;
  int st = check_lwe_ms(switched, lwe_in, lwe_dim, batch, log_modulus, ms_mode, 64);
  if (st != MI_OK) return st;
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  hipError_t e = mi::launch_lwe_ms64(switched, lwe_in, lwe_dim, batch, log_modulus, ms_mode == MI_MS_CENTERED,
                                     (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "modulus switch launch");
}

// ---- LWE packing keyswitch (tfhe/src/core_crypto/algorithms/lwe_packing_keyswitch.rs:102-187, 296-379) ----------

int mi_lwe_pksk_create(const uint64_t* pksk, size_t in_dim, int glwe_dim, size_t polynomial_size, int base_log,
                       int level, int device, void* stream, mi_lwe_pksk** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!pksk) return fail(MI_ERR_INVALID_ARG, "pksk is NULL");
  const size_t n = polynomial_size;
  const char* own = nullptr;
  if (n == 0 || (n & (n - 1)) != 0)
    own = "polynomial size must be a power of two";
  else if (glwe_dim < 1 || n > 0xFFFFFFull || ((size_t)glwe_dim + 1) * n > 0xFFFFFFull)
    own = "glwe size out of range";
  int st = check_ks_range(in_dim, own, base_log, level, 63);
  if (st != MI_OK) return st;
  const mi::KsGeometry geo{mi::KsMode::Packing, in_dim, ((size_t)glwe_dim + 1) * n, base_log, level, 64,
                           (size_t)glwe_dim * n};
  st = ks_create(out_key, pksk, geo, device, stream, "packing keyswitch key");
  if (st != MI_OK) return st;
  (*out_key)->glwe_dim = glwe_dim;
  (*out_key)->polynomial_size = n;
  return MI_OK;
}

int mi_lwe_pksk_destroy(mi_lwe_pksk* key) { return ks_destroy(key); }

int mi_lwe_pksk_info(const mi_lwe_pksk* key, size_t* in_dim, int* glwe_dim, size_t* polynomial_size, int* base_log,
                     int* level) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (in_dim) *in_dim = key->core.geo.in_dim;
  if (glwe_dim) *glwe_dim = key->glwe_dim;
  if (polynomial_size) *polynomial_size = key->polynomial_size;
  if (base_log) *base_log = key->core.geo.base_log;
  if (level) *level = key->core.geo.level;
  return MI_OK;
}

int mi_lwe_packing_keyswitch_batch(const mi_lwe_pksk* key, uint64_t* glwe_out, const uint64_t* lwe_in, size_t n_lwe,
                                   size_t lwe_per_glwe, void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  // lwe_packing_keyswitch.rs:358-360: lwe_ciphertext_count <= polynomial_size
  if (lwe_per_glwe == 0 || lwe_per_glwe > key->polynomial_size)
    return fail(MI_ERR_INVALID_ARG, "lwe_per_glwe must be in [1, polynomial_size]");
  if (n_lwe == 0) return MI_OK;
  if (!glwe_out || !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (n_lwe > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const hipStream_t s = (hipStream_t)stream;
  const KsKey& k = key->core;
  DeviceGuard g(k.device);
  const mi::PksPlan plan = mi::pks_plan(k.geo, n_lwe, lwe_per_glwe);
  // stream-ordered scratch: the GEMM's rows, its int8 digit fragments, the rotate-and-sum pass's partial sums
  mi::ScratchBuf t(s), digits(s), partials(s);
  if (!t.alloc(plan.t_bytes) || !digits.alloc(plan.digit_bytes) ||
      (plan.partial_bytes != 0 && !partials.alloc(plan.partial_bytes)))
    return fail(MI_ERR_OOM, "scratch allocation failed");
  const hipError_t e = mi::launch_packing_keyswitch(glwe_out, lwe_in, k.frag, t.ptr(), digits.ptr(), partials.ptr(),
                                                    n_lwe, lwe_per_glwe, key->polynomial_size, k.geo, plan, s);
  return e == hipSuccess ? MI_OK : hip_fail(e, "packing keyswitch launch");
}

// ---- LWE private functional packing keyswitch against a key list (tfhe/src/core_crypto/algorithms/
// lwe_private_functional_packing_keyswitch.rs:20-88; the list: entities/lwe_private_functional_packing_keyswitch_key_
// list.rs; the circuit bootstrap's use of it: fft_impl/fft64/crypto/wop_pbs/mod.rs:390-435) ------------------------

int mi_lwe_pfpksk_list_create(const uint64_t* pfpksk_list, size_t n_keys, size_t in_dim, int glwe_dim,
                              size_t polynomial_size, int base_log, int level, int device, void* stream,
                              mi_lwe_pfpksk_list** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!pfpksk_list) return fail(MI_ERR_INVALID_ARG, "pfpksk_list is NULL");
  const size_t n = polynomial_size;
  const char* own = nullptr;
  if (n == 0 || (n & (n - 1)) != 0)
    own = "polynomial size must be a power of two";
  else if (glwe_dim < 1 || n > 0xFFFFFFull || ((size_t)glwe_dim + 1) * n > 0xFFFFFFull)
    own = "glwe size out of range";
  else if (n_keys == 0 || n_keys > 0xFFFFFFull || n_keys * ((size_t)glwe_dim + 1) * n > 0xFFFFFFull)
    own = "n_keys * (glwe_dim + 1) * polynomial_size must be in [1, 2^24)";
  int st = check_ks_range(in_dim, own, base_log, level, 63, in_dim + 1);
  if (st != MI_OK) return st;
  mi::KsGeometry geo{mi::KsMode::Pfpks, in_dim, n_keys * ((size_t)glwe_dim + 1) * n, base_log, level, 64, 0, n_keys};
  st = ks_create(out_key, pfpksk_list, geo, device, stream, "private functional packing keyswitch key list");
  if (st != MI_OK) return st;
  (*out_key)->glwe_dim = glwe_dim;
  (*out_key)->polynomial_size = n;
  return MI_OK;
}

int mi_lwe_pfpksk_list_destroy(mi_lwe_pfpksk_list* key) { return ks_destroy(key); }

int mi_lwe_pfpksk_list_info(const mi_lwe_pfpksk_list* key, size_t* n_keys, size_t* in_dim, int* glwe_dim,
                            size_t* polynomial_size, int* base_log, int* level) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (n_keys) *n_keys = key->core.geo.n_keys;
  if (in_dim) *in_dim = key->core.geo.in_dim;
  if (glwe_dim) *glwe_dim = key->glwe_dim;
  if (polynomial_size) *polynomial_size = key->polynomial_size;
  if (base_log) *base_log = key->core.geo.base_log;
  if (level) *level = key->core.geo.level;
  return MI_OK;
}

// One GEMM: the rows are the input LWEs, the columns the n_keys GLWEs of every row back to back, which is the output's
// own layout (glwe_out[b * n_keys + j]).
int mi_lwe_pfpks_batch(const mi_lwe_pfpksk_list* key, uint64_t* glwe_out, const uint64_t* lwe_in, size_t n_lwe,
                       void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  return run_keyswitch(key->core, glwe_out, lwe_in, n_lwe, stream);
}

// ---- CompressedModulusSwitchedGlweCiphertext (entities/compressed_modulus_switched_glwe_ciphertext.rs:169-256) ---

int mi_glwe_compressed_words(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus,
                             size_t* words) {
  if (!words) return fail(MI_ERR_INVALID_ARG, "words is NULL");
  const int st = check_glwe_compress(polynomial_size, glwe_dim, bodies_count, log_modulus);
  if (st != MI_OK) return st;
  *words = mi::glwe_compressed_words(polynomial_size, glwe_dim, bodies_count, log_modulus);
  return MI_OK;
}

int mi_glwe_compress_batch(uint64_t* packed, const uint64_t* glwe, size_t polynomial_size, int glwe_dim,
                           size_t bodies_count, int log_modulus, size_t batch, int device, void* stream) {
  const int st = check_glwe_compress(polynomial_size, glwe_dim, bodies_count, log_modulus);
  if (st != MI_OK) return st;
  if (batch == 0) return MI_OK;
  if (!packed || !glwe) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e = mi::launch_glwe_compress(packed, glwe, polynomial_size, glwe_dim, bodies_count, log_modulus,
                                                batch, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "glwe compression launch");
}

int mi_glwe_extract_batch(uint64_t* glwe, const uint64_t* packed, size_t polynomial_size, int glwe_dim,
                          size_t bodies_count, int log_modulus, size_t batch, int device, void* stream) {
  const int st = check_glwe_compress(polynomial_size, glwe_dim, bodies_count, log_modulus);
  if (st != MI_OK) return st;
  if (batch == 0) return MI_OK;
  if (!packed || !glwe) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e = mi::launch_glwe_extract(glwe, packed, polynomial_size, glwe_dim, bodies_count, log_modulus,
                                               batch, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "glwe extraction launch");
}

// ---- The u128 twins: shortint's compression of noise-squashed ciphertexts (shortint/list_compression/
// noise_squashing_compression.rs:23-118) over lwe_packing_keyswitch.rs:102-187, 296-379 and
// compressed_modulus_switched_glwe_ciphertext.rs:169-256 at Scalar = u128 ------------------------------------------

int mi_lwe_pksk128_create(const uint64_t* pksk, size_t in_dim, int glwe_dim, size_t polynomial_size, int base_log,
                          int level, int device, void* stream, mi_lwe_pksk128** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!pksk) return fail(MI_ERR_INVALID_ARG, "pksk is NULL");
  const size_t n = polynomial_size;
  const char* own = nullptr;
  if (n == 0 || (n & (n - 1)) != 0)
    own = "polynomial size must be a power of two";
  else if (glwe_dim < 1 || n > 0xFFFFFFull || ((size_t)glwe_dim + 1) * n > 0xFFFFFFull)
    own = "glwe size out of range";
  // SignedDecomposer::<u128>::new: base_log * level in [1, 127]; then base_log <= 63 and the 2^17 depth rule, whose
  // bytes per digit are this GEMM's too
  const int st = check_ks_range(in_dim, own, base_log, level, 127);
  if (st != MI_OK) return st;
  mi_lwe_pksk128* key = new (std::nothrow) mi_lwe_pksk128;
  if (!key) return fail(MI_ERR_OOM, "host allocation failed");
  key->device = device;
  key->geo.in_dim = in_dim;
  key->geo.out_size = ((size_t)glwe_dim + 1) * n;
  key->geo.base_log = base_log;
  key->geo.level = level;
  key->geo.body_col = (size_t)glwe_dim * n;
  key->glwe_dim = glwe_dim;
  key->polynomial_size = n;
  DeviceGuard g(device);
  if (!g.ok) {
    delete key;
    return fail(MI_ERR_INVALID_ARG, "bad device");
  }
  if (hipMalloc(&key->frag, mi::pks128_key_bytes(key->geo)) != hipSuccess) {
    delete key;
    return fail(MI_ERR_OOM, "packing keyswitch key allocation failed");
  }
  hipError_t e = mi::launch_pksk128_prepare(key->frag, pksk, key->geo, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) {
    (void)hipFree(key->frag);
    delete key;
    return hip_fail(e, "packing keyswitch key preparation");
  }
  *out_key = key;
  return MI_OK;
}

int mi_lwe_pksk128_destroy(mi_lwe_pksk128* key) {
  if (!key) return MI_OK;
  {
    DeviceGuard g(key->device);
    if (key->frag) (void)hipFree(key->frag);
  }
  delete key;
  return MI_OK;
}

int mi_lwe_pksk128_info(const mi_lwe_pksk128* key, size_t* in_dim, int* glwe_dim, size_t* polynomial_size,
                        int* base_log, int* level) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (in_dim) *in_dim = key->geo.in_dim;
  if (glwe_dim) *glwe_dim = key->glwe_dim;
  if (polynomial_size) *polynomial_size = key->polynomial_size;
  if (base_log) *base_log = key->geo.base_log;
  if (level) *level = key->geo.level;
  return MI_OK;
}

int mi_lwe_packing_keyswitch128_batch(const mi_lwe_pksk128* key, uint64_t* glwe_out, const uint64_t* lwe_in,
                                      size_t n_lwe, size_t lwe_per_glwe, void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  // lwe_packing_keyswitch.rs:358-360: lwe_ciphertext_count <= polynomial_size
  if (lwe_per_glwe == 0 || lwe_per_glwe > key->polynomial_size)
    return fail(MI_ERR_INVALID_ARG, "lwe_per_glwe must be in [1, polynomial_size]");
  if (n_lwe == 0) return MI_OK;
  if (!glwe_out || !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (n_lwe > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  mi::PksPlan plan = mi::pks_plan_rows(key->geo.out_size, 16, n_lwe, lwe_per_glwe);
  plan.digit_bytes = mi::pks128_digit_bytes(key->geo, plan.rows);
  // stream-ordered scratch: the GEMM's rows, its int8 digit fragments, the rotate-and-sum pass's partial sums
  mi::ScratchBuf t(s), digits(s), partials(s);
  if (!t.alloc(plan.t_bytes) || !digits.alloc(plan.digit_bytes) ||
      (plan.partial_bytes != 0 && !partials.alloc(plan.partial_bytes)))
    return fail(MI_ERR_OOM, "scratch allocation failed");
  const hipError_t e = mi::launch_packing_keyswitch128(glwe_out, lwe_in, key->frag, t.ptr(), digits.ptr(),
                                                       partials.ptr(), n_lwe, lwe_per_glwe, key->polynomial_size,
                                                       key->geo, plan, s);
  return e == hipSuccess ? MI_OK : hip_fail(e, "packing keyswitch launch");
}

int mi_glwe_compressed_words128(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus,
                                size_t* words) {
  if (!words) return fail(MI_ERR_INVALID_ARG, "words is NULL");
  const int st = check_glwe_compress(polynomial_size, glwe_dim, bodies_count, log_modulus, 128);
  if (st != MI_OK) return st;
  *words = mi::glwe_compressed_words128(polynomial_size, glwe_dim, bodies_count, log_modulus);
  return MI_OK;
}

int mi_glwe_compress128_batch(uint64_t* packed, const uint64_t* glwe, size_t polynomial_size, int glwe_dim,
                              size_t bodies_count, int log_modulus, size_t batch, int device, void* stream) {
  const int st = check_glwe_compress(polynomial_size, glwe_dim, bodies_count, log_modulus, 128);
  if (st != MI_OK) return st;
  if (batch == 0) return MI_OK;
  if (!packed || !glwe) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e = mi::launch_glwe_compress128(packed, glwe, polynomial_size, glwe_dim, bodies_count, log_modulus,
                                                   batch, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "glwe compression launch");
}

int mi_glwe_extract128_batch(uint64_t* glwe, const uint64_t* packed, size_t polynomial_size, int glwe_dim,
                             size_t bodies_count, int log_modulus, size_t batch, int device, void* stream) {
  const int st = check_glwe_compress(polynomial_size, glwe_dim, bodies_count, log_modulus, 128);
  if (st != MI_OK) return st;
  if (batch == 0) return MI_OK;
  if (!packed || !glwe) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e = mi::launch_glwe_extract128(glwe, packed, polynomial_size, glwe_dim, bodies_count, log_modulus,
                                                  batch, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "glwe extraction launch");
}

}  // extern "C"
