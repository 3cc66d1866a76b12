// c_api_pbs128.cpp — the 128-bit bootstrap family of the C ABI: the limb plan, the prepared u128 bootstrap key, the
// external product, CMUX, blind rotation and PBS over Z_{2^128}[X]/(X^N + 1) (kernels and step loop: pbs128.hip), and
// the multi-bit key, blind rotation and PBS (pbs128_multi_bit.hip).
#include <new>
#include <string>
#include <vector>

#include "scratch.hpp"
#include "c_api_internal.hpp"

using namespace mi::capi;

struct mi_pbs128_key {
  const mi_ntt64_plan* plan = nullptr;
  size_t n_ggsw = 0;
  mi::Pbs128Shape shape;
  u64* prepared = nullptr;  // n_ggsw x level (k + 1)^2 n_limbs transformed limb polynomials, N^-1 folded in
};

struct mi_pbs128_multi_bit_key {
  const mi_ntt64_plan* plan = nullptr;
  size_t n_lwe = 0;
  int grouping_factor = 0;
  mi::Pbs128Shape shape;    // limb_bits / n_limbs of the multi-bit limb rule
  u64* prepared = nullptr;  // (n_lwe / g) 2^g GGSWs, each as mi_pbs128_key's
  u64* roots = nullptr;     // psi^j, j < 2N: the phases of X^d in the transform domain
};

namespace {

constexpr int MAX_LIMBS = 16;
// the multi-bit limb is up to 4 bits narrower (2^g GGSWs per column): 32 limbs there are the classic bootstrap's 16
constexpr int MAX_LIMBS_MULTI_BIT = 32;

// The limb rule: w = the largest width with R N 2^(B-1) (2^w - 1) <= (p - 1) / 2, R = (k + 1) level; n_limbs =
// ceil(128 / w) (0 limbs when not even w = 1 fits).  The arguments are valid.  The multi-bit rule sums 2^g GGSWs in
// one column: the same with 2^g R rows (g = 0: the classic rule).
void limb_rule(size_t n, int k, int base_log, int level, int g, int* limb_bits, int* n_limbs) {
  const u128 half = (u128)((0xFFFFFFFF00000001ull - 1) / 2);
  int logn = 0;
  while (((size_t)1 << logn) < n) ++logn;
  int w = 0;
  if (base_log - 1 + logn + g < 63) {  // else R N 2^(B-1) alone exceeds (p - 1) / 2
    const u128 d = ((u128)(k + 1) * (u128)level) << (base_log - 1 + logn + g);
    const u128 q = half / d;  // 2^w - 1 <= q
    while (w < 63 && (((u128)1 << (w + 1)) - 1) <= q) ++w;
  }
  *limb_bits = w;
  *n_limbs = w ? (128 + w - 1) / w : 0;
}

// the argument rules of mi_pbs128_limb_plan, shared with the key: where SignedDecomposer::<u128>::new asserts
// (decomposer.rs:86-90: BITS > base_log * level), N a power of two, k >= 1
int check_limb_args(size_t n, int k, int base_log, int level) {
  if (n == 0 || (n & (n - 1)) != 0) return fail(MI_ERR_INVALID_ARG, "polynomial size must be a power of two");
  if (n > ((size_t)1 << 31)) return fail(MI_ERR_INVALID_ARG, "polynomial size must be at most 2^31");  // as the plans
  if (k < 1) return fail(MI_ERR_INVALID_ARG, "glwe dimension must be >= 1");
  if (k > 0xFFFF) return fail(MI_ERR_INVALID_ARG, "glwe dimension must be at most 65535");  // R stays far below 2^32
  if (base_log < 1 || level < 1 || base_log > 127 || level > 127 || base_log * level > 127)
    return fail(MI_ERR_INVALID_ARG, "decomposition base_log * level must be in [1, 127]");
  return MI_OK;
}

int check_grouping_factor(int g) {
  return g >= 2 && g <= 4 ? MI_OK : fail(MI_ERR_INVALID_ARG, "grouping factor must be 2, 3 or 4");
}

int limb_plan(size_t n, int k, int base_log, int level, int g, int* limb_bits, int* n_limbs) {
  const int st = check_limb_args(n, k, base_log, level);
  if (st != MI_OK) return st;
  limb_rule(n, k, base_log, level, g, limb_bits, n_limbs);
  if (g != 0 && (*n_limbs == 0 || *n_limbs > MAX_LIMBS_MULTI_BIT))
    return fail(MI_ERR_UNSUPPORTED, "the multi-bit limb plan needs more than 32 limbs");
  if (g == 0 && (*n_limbs == 0 || *n_limbs > MAX_LIMBS))
    return fail(MI_ERR_UNSUPPORTED, "the limb plan needs more than 16 limbs");
  return MI_OK;
}

mi::Ntt128Route route_of(const mi_ntt64_plan* plan) {
  mi::Ntt128Route r;
  r.logn = plan->logn;
  r.twisted = plan->twisted;
  r.split = plan->d_split != nullptr;
  r.tw = plan->d_twid;
  r.itw = plan->d_inv_twid;
  r.twist_f = plan->d_twist_f;
  r.twist_i = plan->d_twist_i;
  if (r.split) r.st = plan->split;
  r.n_inv = plan->n_inv;
  return r;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// out += GGSW (.) in, or the CMUX: the checks the two entries share
int ext_common(const mi_pbs128_key* key, bool cmux, size_t ggsw_index, uint64_t* out, uint64_t* in, size_t batch,
               void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (ggsw_index >= key->n_ggsw) return fail(MI_ERR_INVALID_ARG, "ggsw_index must be < n_ggsw");
  if (batch == 0) return MI_OK;
  if (!out || !in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (!aligned16(out) || !aligned16(in)) return fail(MI_ERR_INVALID_ARG, "u128 buffers must be 16-byte aligned");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  // the recombination writes `out` after `in` was read by another pass: overlapping operands would not give the
  // reference's result
  const uintptr_t bytes = (uintptr_t)batch * ((size_t)key->shape.k + 1) * key->plan->n * 16;
  if (overlap(out, bytes, in, bytes)) return fail(MI_ERR_INVALID_ARG, "buffers overlap");
  DeviceGuard g(key->plan->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e = mi::launch_ext_product128(cmux, out, in, key->prepared + ggsw_index * mi::pbs128_ggsw_words(key->shape),
                                                 batch, key->shape, route_of(key->plan), (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, cmux ? "cmux launch" : "external product launch");
}

// the blind rotation behind mi_blind_rotate128_batch (lut NULL, in place) and mi_pbs128_batch
int rotate_common(const mi_pbs128_key* key, uint64_t* lwe_out, uint64_t* acc_glwe, const uint64_t* lut,
                  const uint64_t* lwe_in, size_t batch, int ms_mode, void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (ms_mode != MI_MS_STANDARD && ms_mode != MI_MS_CENTERED && ms_mode != MI_MS_PRE_SWITCHED)
    return fail(MI_ERR_INVALID_ARG, "unknown ms_mode");
  if (batch == 0) return MI_OK;
  if ((!lwe_out && !acc_glwe) || !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (!aligned16(lwe_out) || !aligned16(acc_glwe) || !aligned16(lut))
    return fail(MI_ERR_INVALID_ARG, "u128 buffers must be 16-byte aligned");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  DeviceGuard g(key->plan->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e =
      mi::launch_blind_rotate128(lwe_out, acc_glwe, lut, lwe_in, key->prepared, key->n_ggsw, batch,
                                 ms_mode == MI_MS_CENTERED, ms_mode == MI_MS_PRE_SWITCHED, key->shape,
                                 route_of(key->plan), (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, lut ? "pbs launch" : "blind rotation launch");
}

// the multi-bit blind rotation behind mi_pbs128_multi_bit_blind_rotate_batch (lut NULL, in place) and
// mi_pbs128_multi_bit_batch
int multi_bit_common(const mi_pbs128_multi_bit_key* key, uint64_t* lwe_out, uint64_t* acc_glwe, const uint64_t* lut,
                     const uint64_t* lwe_in, size_t batch, void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (batch == 0) return MI_OK;
  if ((!lwe_out && !acc_glwe) || !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (!aligned16(lwe_out) || !aligned16(acc_glwe) || !aligned16(lut))
    return fail(MI_ERR_INVALID_ARG, "u128 buffers must be 16-byte aligned");
  if (batch > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  // the output is written while the LWEs (every step reads its mask group) and the LUT are still read
  const size_t n = key->plan->n, kp1 = (size_t)key->shape.k + 1;
  const size_t in_bytes = batch * (key->n_lwe + 1) * 8, glwe_bytes = kp1 * n * 16;
  const void* out = lwe_out ? (const void*)lwe_out : (const void*)acc_glwe;
  const size_t out_bytes = lwe_out ? batch * ((kp1 - 1) * n + 1) * 16 : batch * glwe_bytes;
  if (overlap(out, out_bytes, lwe_in, in_bytes) || (lut && overlap(out, out_bytes, lut, glwe_bytes)))
    return fail(MI_ERR_INVALID_ARG, "buffers overlap");
  DeviceGuard g(key->plan->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const hipError_t e = mi::launch_multi_bit_blind_rotate128(lwe_out, acc_glwe, lut, lwe_in, key->prepared, key->roots,
                                                            key->n_lwe, key->grouping_factor, batch, key->shape,
                                                            route_of(key->plan), (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, lut ? "multi-bit pbs launch" : "multi-bit blind rotation launch");
}

void free_multi_bit_key(mi_pbs128_multi_bit_key* key) {
  if (key->prepared) (void)hipFree(key->prepared);
  if (key->roots) (void)hipFree(key->roots);
  delete key;
}

}  // namespace

extern "C" {

int mi_pbs128_limb_plan(size_t polynomial_size, int k, int base_log, int level, int* limb_bits, int* n_limbs) {
  int w = 0, nl = 0;
  const int st = limb_plan(polynomial_size, k, base_log, level, 0, &w, &nl);
  if (st == MI_ERR_INVALID_ARG) return st;
  if (limb_bits) *limb_bits = w;
  if (n_limbs) *n_limbs = nl;
  return st;
}

int mi_pbs128_key_create(const mi_ntt64_plan* plan, const uint64_t* bsk_std, size_t n_ggsw, int k,
                         size_t polynomial_size, int base_log, int level, void* stream, mi_pbs128_key** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (!bsk_std) return fail(MI_ERR_INVALID_ARG, "bsk_std is NULL");
  if (n_ggsw == 0 || n_ggsw > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "lwe dimension out of range");
  int st = check_limb_args(polynomial_size, k, base_log, level);
  if (st != MI_OK) return st;
  if (!plan->goldilocks || plan->n != polynomial_size)
    return fail(MI_ERR_UNSUPPORTED, "the plan must be the Goldilocks plan of the key's polynomial size");
  if (k > 3) return fail(MI_ERR_UNSUPPORTED, "the 128-bit bootstrap runs for glwe dimensions 1 to 3");
  mi::Pbs128Shape shape;
  shape.logn = plan->logn;
  shape.k = k;
  shape.base_log = base_log;
  shape.level = level;
  st = limb_plan(polynomial_size, k, base_log, level, 0, &shape.limb_bits, &shape.n_limbs);
  if (st != MI_OK) return st;
  if (!aligned16(bsk_std)) return fail(MI_ERR_INVALID_ARG, "u128 buffers must be 16-byte aligned");
  mi_pbs128_key* key = new (std::nothrow) mi_pbs128_key;
  if (!key) return fail(MI_ERR_OOM, "host allocation failed");
  key->plan = plan;
  key->n_ggsw = n_ggsw;
  key->shape = shape;
  DeviceGuard g(plan->device);
  if (!g.ok) {
    delete key;
    return fail(MI_ERR_INVALID_ARG, "bad device");
  }
  if (hipMalloc((void**)&key->prepared, n_ggsw * mi::pbs128_ggsw_words(shape) * sizeof(u64)) != hipSuccess) {
    delete key;
    return fail(MI_ERR_OOM, "bootstrap key allocation failed");
  }
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = mi::launch_pbs128_key_prepare(key->prepared, bsk_std, n_ggsw, shape, route_of(plan), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(key->prepared);
    delete key;
    return hip_fail(e, "bootstrap key preparation");
  }
  *out_key = key;
  return MI_OK;
}

int mi_pbs128_key_destroy(mi_pbs128_key* key) {
  if (!key) return MI_OK;
  {
    DeviceGuard g(key->plan->device);
    if (key->prepared) (void)hipFree(key->prepared);
  }
  delete key;
  return MI_OK;
}

int mi_pbs128_key_info(const mi_pbs128_key* key, size_t* n_ggsw, int* k, size_t* polynomial_size, int* base_log,
                       int* level, int* limb_bits, int* n_limbs) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (n_ggsw) *n_ggsw = key->n_ggsw;
  if (k) *k = key->shape.k;
  if (polynomial_size) *polynomial_size = key->plan->n;
  if (base_log) *base_log = key->shape.base_log;
  if (level) *level = key->shape.level;
  if (limb_bits) *limb_bits = key->shape.limb_bits;
  if (n_limbs) *n_limbs = key->shape.n_limbs;
  return MI_OK;
}

int mi_ext_product128_batch(const mi_pbs128_key* key, size_t ggsw_index, uint64_t* out_glwe, const uint64_t* in_glwe,
                            size_t batch, void* stream) {
  return ext_common(key, false, ggsw_index, out_glwe, const_cast<uint64_t*>(in_glwe), batch, stream);
}

int mi_cmux128_batch(const mi_pbs128_key* key, size_t ggsw_index, uint64_t* ct0, uint64_t* ct1, size_t batch,
                     void* stream) {
  return ext_common(key, true, ggsw_index, ct0, ct1, batch, stream);
}

int mi_blind_rotate128_batch(const mi_pbs128_key* key, uint64_t* acc_glwe, const uint64_t* lwe_in, size_t batch,
                             int ms_mode, void* stream) {
  if (key && batch && !acc_glwe) return fail(MI_ERR_INVALID_ARG, "acc_glwe is NULL");
  return rotate_common(key, nullptr, acc_glwe, nullptr, lwe_in, batch, ms_mode, stream);
}

int mi_pbs128_batch(const mi_pbs128_key* key, uint64_t* lwe_out, const uint64_t* lwe_in, const uint64_t* lut,
                    size_t batch, int ms_mode, void* stream) {
  if (key && batch && (!lwe_out || !lut)) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  return rotate_common(key, lwe_out, nullptr, lut, lwe_in, batch, ms_mode, stream);
}

int mi_pbs128_multi_bit_limb_plan(size_t polynomial_size, int k, int base_log, int level, int grouping_factor,
                                  int* limb_bits, int* n_limbs) {
  int w = 0, nl = 0;
  int st = check_grouping_factor(grouping_factor);
  if (st != MI_OK) return st;
  st = limb_plan(polynomial_size, k, base_log, level, grouping_factor, &w, &nl);
  if (st == MI_ERR_INVALID_ARG) return st;
  if (limb_bits) *limb_bits = w;
  if (n_limbs) *n_limbs = nl;
  return st;
}

int mi_pbs128_multi_bit_key_create(const mi_ntt64_plan* plan, const uint64_t* bsk_std, size_t n_lwe, int k,
                                   size_t polynomial_size, int base_log, int level, int grouping_factor, void* stream,
                                   mi_pbs128_multi_bit_key** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (!bsk_std) return fail(MI_ERR_INVALID_ARG, "bsk_std is NULL");
  int st = check_grouping_factor(grouping_factor);
  if (st != MI_OK) return st;
  if (n_lwe == 0 || n_lwe > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "lwe dimension out of range");
  if (n_lwe % (size_t)grouping_factor)
    return fail(MI_ERR_INVALID_ARG, "lwe dimension must be a multiple of the grouping factor");
  st = check_limb_args(polynomial_size, k, base_log, level);
  if (st != MI_OK) return st;
  if (!plan->goldilocks || plan->n != polynomial_size)
    return fail(MI_ERR_UNSUPPORTED, "the plan must be the Goldilocks plan of the key's polynomial size");
  if (k > 3) return fail(MI_ERR_UNSUPPORTED, "the 128-bit bootstrap runs for glwe dimensions 1 to 3");
  mi::Pbs128Shape shape;
  shape.logn = plan->logn;
  shape.k = k;
  shape.base_log = base_log;
  shape.level = level;
  st = limb_plan(polynomial_size, k, base_log, level, grouping_factor, &shape.limb_bits, &shape.n_limbs);
  if (st != MI_OK) return st;
  if (!aligned16(bsk_std)) return fail(MI_ERR_INVALID_ARG, "u128 buffers must be 16-byte aligned");
  mi_pbs128_multi_bit_key* key = new (std::nothrow) mi_pbs128_multi_bit_key;
  if (!key) return fail(MI_ERR_OOM, "host allocation failed");
  key->plan = plan;
  key->n_lwe = n_lwe;
  key->grouping_factor = grouping_factor;
  key->shape = shape;
  DeviceGuard g(plan->device);
  if (!g.ok) {
    delete key;
    return fail(MI_ERR_INVALID_ARG, "bad device");
  }
  const size_t n = plan->n, n_ggsw = (n_lwe / (size_t)grouping_factor) << grouping_factor;
  if (hipMalloc((void**)&key->prepared, n_ggsw * mi::pbs128_ggsw_words(shape) * sizeof(u64)) != hipSuccess ||
      hipMalloc((void**)&key->roots, 2 * n * sizeof(u64)) != hipSuccess) {
    free_multi_bit_key(key);
    return fail(MI_ERR_OOM, "bootstrap key allocation failed");
  }
  // psi^j from the plan's forward twiddles (twid[bitrev(j)] = psi^j, j < N); psi^(N + j) = -psi^j
  std::vector<u64> roots(2 * n);
  for (size_t j = 0; j < n; ++j) {
    size_t r = 0;
    for (int b = 0; b < plan->logn; ++b) r |= ((j >> b) & 1) << (plan->logn - 1 - b);
    roots[j] = plan->twid[r];
    roots[n + j] = plan->p - roots[j];
  }
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(key->roots, roots.data(), 2 * n * sizeof(u64), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = mi::launch_pbs128_key_prepare(key->prepared, bsk_std, n_ggsw, shape, route_of(plan), s);
  const hipError_t es = hipStreamSynchronize(s);  // also on an error: `roots` is read by the copy
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    free_multi_bit_key(key);
    return hip_fail(e, "multi-bit bootstrap key preparation");
  }
  *out_key = key;
  return MI_OK;
}

int mi_pbs128_multi_bit_key_destroy(mi_pbs128_multi_bit_key* key) {
  if (!key) return MI_OK;
  DeviceGuard g(key->plan->device);
  free_multi_bit_key(key);
  return MI_OK;
}

int mi_pbs128_multi_bit_key_info(const mi_pbs128_multi_bit_key* key, size_t* n_lwe, int* k, size_t* polynomial_size,
                                 int* base_log, int* level, int* grouping_factor, int* limb_bits, int* n_limbs) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (n_lwe) *n_lwe = key->n_lwe;
  if (k) *k = key->shape.k;
  if (polynomial_size) *polynomial_size = key->plan->n;
  if (base_log) *base_log = key->shape.base_log;
  if (level) *level = key->shape.level;
  if (grouping_factor) *grouping_factor = key->grouping_factor;
  if (limb_bits) *limb_bits = key->shape.limb_bits;
  if (n_limbs) *n_limbs = key->shape.n_limbs;
  return MI_OK;
}

int mi_pbs128_multi_bit_blind_rotate_batch(const mi_pbs128_multi_bit_key* key, uint64_t* acc_glwe,
                                           const uint64_t* lwe_in, size_t batch, void* stream) {
  if (key && batch && !acc_glwe) return fail(MI_ERR_INVALID_ARG, "acc_glwe is NULL");
  return multi_bit_common(key, nullptr, acc_glwe, nullptr, lwe_in, batch, stream);
}

int mi_pbs128_multi_bit_batch(const mi_pbs128_multi_bit_key* key, uint64_t* lwe_out, const uint64_t* lwe_in,
                              const uint64_t* lut, size_t batch, void* stream) {
  if (key && batch && (!lwe_out || !lut)) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  return multi_bit_common(key, lwe_out, nullptr, lut, lwe_in, batch, stream);
}

}  // extern "C"
