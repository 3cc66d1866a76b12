// c_api_shortint.cpp — the first slice of the shortint / integer layer of the C ABI: the linear algebra of LWE
// ciphertexts, the shortint atomic pattern (keyswitch, modulus switch, bootstrap through a lookup table) and radix
// integer addition.  Reference paths relative to tfhe/src:
//   lwe_ciphertext_add / _sub / _opposite / _cleartext_mul / _plaintext_add   core_crypto/algorithms/lwe_linear_algebra.rs
//   fill_accumulator_with_encoding                 shortint/engine/mod.rs:80-141
//   apply_lookup_table / apply_programmable_bootstrap   shortint/server_key/mod.rs:935-960, :1542
//   unchecked_apply_lookup_table_bivariate         shortint/server_key/bivariate_pbs.rs:141-190
//   compute_prefix_sum_hillis_steele               integer/server_key/radix_parallel/add.rs:1452-1487
//   full_propagate_parallelized                    integer/server_key/radix_parallel/mod.rs:228 (:91-201)
//   host_propagate_single_carry                    backends/tfhe-cuda-backend/cuda/src/integer/integer.cuh
//
// Every composite is a fixed sequence of public calls with nothing fused across a stage boundary, so it equals that
// sequence bit for bit.  LC below is mi_lwe_linear_combination_batch, KS mi_lwe_keyswitch_batch, DRIFT
// mi_lwe_ms_noise_improve_and_switch_batch, PBS the key's *_pbs_batch_lut_indexed; index arrays are written on the
// device by the rules of lwe_linear_algebra_launch.hpp (nothing is copied from the host).
//
//   APPLY(out, in, n_in, in_index, luts, lut_index, n_lut, n_items) = mi_shortint_apply_lut_batch:
//     1. KS     ks[n_in] = keyswitch(in[n_in])
//     2. DRIFT  sw[n_in] = improve_and_switch(ks, log2(2 N))             only with an ms-noise key; then sw replaces ks
//     3. LC     g[n_items] = ks[in_index[j]], one term, coefficient 1     only with in_index; then g replaces ks and
//               lut_index[j] is replaced by 0xFFFFFFFF where in_index[j] >= n_in
//     4. PBS    out[j] = pbs(ks[j], luts[lut_index[j]]), ms_mode the key's (MI_MS_PRE_SWITCHED after DRIFT)
//
//   mi_radix_propagate_single_carry_batch on T = I x B blocks (work = msg[T] | st[T] in scratch; key LUTs MSG x mod m,
//   STATE0 x >= m, STATE (x >= m) + 2 (x == m - 1), SCAN (cur, prev) -> cur == 2 ? prev : cur):
//     1. APPLY  work[2 T] <- radix[T], in_index j % T, LUT MSG for j < T, else STATE0 for block 0 and STATE for the others
//        (B = 1: radix <- msg, carry_out <- st; done)
//     2. for s = 1, 2, 4, ... < B, on the I (B - s) blocks b >= s:
//          LC     pack[c] = m * st[i, b] + st[i, b - s]
//          APPLY  st[T] <- pack, in_index = the packed row of (i, b), 0xFFFFFFFF for b < s (kept), LUT SCAN
//     3. LC     sum[i, b] = msg[i, b] + st[i, b - 1]   (b = 0: msg alone)
//        APPLY  radix[T] <- sum[T], LUT MSG
//     4. LC     carry_out[i] = st[i, B - 1]            only with carry_out
//
//   mi_radix_full_propagate_batch:
//     1. APPLY  work[2 T] <- radix[T], in_index j % T, LUT MSG for j < T, else CARRY
//     2. LC     radix[i, b] = msg[i, b] + carry[i, b - 1]   (b = 0: msg alone)
//     3. mi_radix_propagate_single_carry_batch(radix); where that is unsupported, steps 1 and 2 again B - 1 times: each
//        moves every carry one block up, which leaves the blocks the sequential loop of radix_parallel/mod.rs:187-199
//        leaves
//
//   mi_radix_add_batch: lhs and rhs copied into one scratch list (two device-to-device copies), LC out[j] = l[j] +
//   r[j], mi_radix_propagate_single_carry_batch(out, carry_out).
#include <string>
#include <vector>

#include "c_api_internal.hpp"
#include "lwe_linear_algebra_launch.hpp"
#include "scratch.hpp"
#include "shortint_internal.hpp"

using namespace mi::capi;
using namespace mi::shortint;

namespace {

bool pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }

// block values up to 2 (m - 1) and the packed scan operand 2 m + 2 must stay below m c
bool single_carry_supported(uint64_t m, uint64_t c) { return m * c >= 16 && c <= m && 2 * m + 2 < m * c; }

int single_carry_unsupported() {
  return fail(MI_ERR_UNSUPPORTED,
              "single carry propagation needs message_modulus * carry_modulus >= 16, carry_modulus <= "
              "message_modulus and 2 * message_modulus + 2 < message_modulus * carry_modulus");
}

int pbs_call(const mi_shortint_key* key, uint64_t* out, const uint64_t* in, const uint64_t* luts, const uint32_t* idx,
             size_t n_lut, size_t items, int ms_mode, void* stream) {
  switch (key->engine) {
    case MI_SHORTINT_PBS_NTT64:
      return mi_pbs_ntt64_batch_lut_indexed((const mi_pbs_ntt64_key*)key->pbs, out, in, luts, idx, n_lut, items, ms_mode,
                                            stream);
    case MI_SHORTINT_PBS_FFT64:
      return mi_fft64_pbs_batch_lut_indexed((const mi_fft64_pbs_key*)key->pbs, out, in, luts, idx, n_lut, items, ms_mode,
                                            stream);
    default:
      return mi_fft64_multi_bit_pbs_batch_lut_indexed((const mi_fft64_multi_bit_pbs_key*)key->pbs, out, in, luts, idx,
                                                      n_lut, items, stream);
  }
}

// out[j] = in[j] + in[T + j - 1] for block b >= 1, in[j] for block 0, over in = msg[T] | carry-like[T]
int add_previous(const RadixStages& sg, uint64_t* out, const uint64_t* work, size_t blocks, size_t total) {
  const uint32_t T = (uint32_t)total, B = (uint32_t)blocks;
  return sg.combine2(out, work, 2 * total, total, {T, T, 0, 0, 0, 0}, {T, B, 1, T, B, 1});
}

}  // namespace

extern "C" {

int mi_lwe_linear_combination_batch(uint64_t* lwe_out, const uint64_t* lwe_in, size_t lwe_dim, size_t n_in,
                                    size_t n_out, size_t terms, const uint32_t* index, const int64_t* coeff,
                                    const uint64_t* plaintext, int device, void* stream) {
  if (lwe_dim < 1 || lwe_dim >= ((size_t)1 << 24)) return fail(MI_ERR_INVALID_ARG, "lwe dimension out of range");
  if (n_in > 0x7FFFFFFFull || n_out > 0x7FFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  if (terms > 0xFFFFull) return fail(MI_ERR_INVALID_ARG, "terms out of range");
  if (n_out == 0) return MI_OK;
  if (!lwe_out) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (terms != 0 && !index) return fail(MI_ERR_INVALID_ARG, "index is NULL");
  if (terms != 0 && n_in != 0 && !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const size_t row = (lwe_dim + 1) * sizeof(uint64_t);
  if (terms != 0 && overlap(lwe_out, n_out * row, lwe_in, n_in * row))
    return fail(MI_ERR_INVALID_ARG, "lwe_out overlaps lwe_in");
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  return hip_status(mi::launch_lwe_linear_combination(lwe_out, lwe_in, lwe_dim + 1, terms ? n_in : 0, n_out, terms,
                                                      index, coeff, plaintext, (hipStream_t)stream),
                    "linear combination launch");
}

int mi_shortint_key_check(size_t ksk_in_dim, size_t ksk_out_dim, size_t pbs_n_lwe, int k, size_t polynomial_size,
                          int pbs_engine, int ntt_variant, int has_ms_noise, size_t ms_noise_lwe_dim, int ms_mode,
                          uint64_t message_modulus, uint64_t carry_modulus) {
  if (pbs_engine != MI_SHORTINT_PBS_NTT64 && pbs_engine != MI_SHORTINT_PBS_FFT64 &&
      pbs_engine != MI_SHORTINT_PBS_FFT64_MULTI_BIT)
    return fail(MI_ERR_INVALID_ARG, "unknown pbs engine");
  if (pbs_engine == MI_SHORTINT_PBS_NTT64 && ntt_variant != MI_NTT64_BNF)
    return fail(MI_ERR_UNSUPPORTED, "a Solinas-variant NTT key does not take a native LWE: use the BNF variant");
  if (ksk_out_dim != pbs_n_lwe)
    return fail(MI_ERR_INVALID_ARG, "the keyswitch key's output dimension must be the bootstrap key's input dimension");
  if (k < 1 || ksk_in_dim != (size_t)k * polynomial_size)
    return fail(MI_ERR_INVALID_ARG, "the keyswitch key's input dimension must be k * N of the bootstrap key");
  if (!pow2(message_modulus) || !pow2(carry_modulus))
    return fail(MI_ERR_INVALID_ARG, "message_modulus and carry_modulus must be powers of two");
  if (message_modulus > polynomial_size || carry_modulus > polynomial_size ||
      message_modulus * carry_modulus > polynomial_size / 2)
    return fail(MI_ERR_INVALID_ARG, "message_modulus * carry_modulus must be at most N / 2");
  if (ms_mode != MI_MS_STANDARD && ms_mode != MI_MS_CENTERED)
    return fail(MI_ERR_INVALID_ARG, "ms_mode must be MI_MS_STANDARD or MI_MS_CENTERED");
  if (has_ms_noise && pbs_engine == MI_SHORTINT_PBS_FFT64_MULTI_BIT)
    return fail(MI_ERR_INVALID_ARG, "the multi-bit engine switches its own input: no ms-noise key");
  if (pbs_engine == MI_SHORTINT_PBS_FFT64_MULTI_BIT && ms_mode != MI_MS_STANDARD)
    return fail(MI_ERR_INVALID_ARG, "the multi-bit engine has the standard modulus switch only");
  if (has_ms_noise && ms_mode != MI_MS_STANDARD)
    return fail(MI_ERR_INVALID_ARG, "the drift technique ends in the standard modulus switch");
  if (has_ms_noise && ms_noise_lwe_dim != ksk_out_dim)
    return fail(MI_ERR_INVALID_ARG, "the ms-noise key's dimension must be the keyswitch key's output dimension");
  return MI_OK;
}

int mi_shortint_lut_fill(uint64_t* glwe_host, size_t polynomial_size, int k, uint64_t message_modulus,
                         uint64_t carry_modulus, const uint64_t* table, size_t table_len) {
  if (!glwe_host || !table) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (k < 1 || !pow2(polynomial_size)) return fail(MI_ERR_INVALID_ARG, "polynomial size must be a power of two, k >= 1");
  if (!pow2(message_modulus) || !pow2(carry_modulus))
    return fail(MI_ERR_INVALID_ARG, "message_modulus and carry_modulus must be powers of two");
  if (message_modulus > polynomial_size || carry_modulus > polynomial_size ||
      message_modulus * carry_modulus > polynomial_size / 2)
    return fail(MI_ERR_INVALID_ARG, "message_modulus * carry_modulus must be at most N / 2");
  const uint64_t sup = message_modulus * carry_modulus;
  if (table_len != sup) return fail(MI_ERR_INVALID_ARG, "table_len must be message_modulus * carry_modulus");
  const size_t n = polynomial_size, box = n / sup, half = box / 2;
  const uint64_t delta = ((uint64_t)1 << 63) / sup;
  uint64_t* body = glwe_host + (size_t)k * n;
  for (size_t i = 0; i < (size_t)k * n; ++i) glwe_host[i] = 0;
  // box i of the unrotated accumulator holds table[i] delta, the first half box negated; rotate_left(half)
  for (size_t j = 0; j < n; ++j) {
    const size_t src = (j + half) % n;
    const uint64_t v = table[src / box] * delta;
    body[j] = src < half ? (uint64_t)0 - v : v;
  }
  return MI_OK;
}

int mi_shortint_key_create(const mi_lwe_ksk* ksk, int pbs_engine, const void* pbs_key, const mi_ms_noise_key* ms_noise,
                           int ms_mode, uint64_t message_modulus, uint64_t carry_modulus, mi_shortint_key** out_key) {
  if (!out_key) return fail(MI_ERR_INVALID_ARG, "out_key is NULL");
  *out_key = nullptr;
  if (!ksk || !pbs_key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  size_t ks_in = 0, ks_out = 0, n_lwe = 0, n = 0, ms_dim = 0;
  int k = 1, variant = MI_NTT64_BNF, device = 0;
  MI_TRY(mi_lwe_ksk_info(ksk, &ks_in, &ks_out, nullptr, nullptr));
  if (pbs_engine == MI_SHORTINT_PBS_NTT64) {
    const mi_pbs_ntt64_key* p = (const mi_pbs_ntt64_key*)pbs_key;
    n_lwe = p->n_lwe, k = p->k, n = p->plan->n, variant = p->variant, device = p->plan->device;
  } else if (pbs_engine == MI_SHORTINT_PBS_FFT64) {
    const mi_fft64_pbs_key* p = (const mi_fft64_pbs_key*)pbs_key;
    n_lwe = p->n_lwe, k = p->k, n = p->plan->n, device = p->plan->device;
  } else if (pbs_engine == MI_SHORTINT_PBS_FFT64_MULTI_BIT) {
    const mi_fft64_multi_bit_pbs_key* p = (const mi_fft64_multi_bit_pbs_key*)pbs_key;
    n_lwe = p->n_lwe, k = p->k, n = p->plan->n, device = p->plan->device;
  } else {
    return fail(MI_ERR_INVALID_ARG, "unknown pbs engine");
  }
  if (ms_noise) MI_TRY(mi_ms_noise_key_info(ms_noise, &ms_dim, nullptr, nullptr, nullptr, nullptr));
  MI_TRY(mi_shortint_key_check(ks_in, ks_out, n_lwe, k, n, pbs_engine, variant, ms_noise != nullptr, ms_dim, ms_mode,
                               message_modulus, carry_modulus));
  // the lookup tables of the radix drivers
  const uint64_t m = message_modulus, sup = message_modulus * carry_modulus;
  const size_t per = ((size_t)k + 1) * n;
  std::vector<uint64_t> luts(N_KEY_LUTS * per), table(sup);
  for (int l = 0; l < N_KEY_LUTS; ++l) {
    for (uint64_t x = 0; x < sup; ++x) {
      const uint64_t cur = (x / m) % m, prev = x % m;
      table[x] = l == LUT_MSG      ? x % m
                 : l == LUT_CARRY  ? x / m
                 : l == LUT_STATE0 ? (uint64_t)(x >= m)
                 : l == LUT_STATE  ? (x >= m ? 1 : x == m - 1 ? 2 : 0)
                 : l == LUT_SCAN   ? (cur == 2 ? prev : cur)
                 : l == LUT_MUL_LSB ? (cur * prev) % m
                                    : (cur * prev) / m;
    }
    MI_TRY(mi_shortint_lut_fill(luts.data() + l * per, n, k, message_modulus, carry_modulus, table.data(), sup));
  }
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  mi_shortint_key* key = new mi_shortint_key;
  if (hipMalloc((void**)&key->d_luts, luts.size() * sizeof(uint64_t)) != hipSuccess) {
    delete key;
    return fail(MI_ERR_OOM, "device allocation failed");
  }
  const hipError_t e = hipMemcpy(key->d_luts, luts.data(), luts.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(key->d_luts);
    delete key;
    return hip_fail(e, "lookup table upload");
  }
  key->ksk = ksk, key->engine = pbs_engine, key->pbs = pbs_key, key->ms_noise = ms_noise, key->ms_mode = ms_mode;
  key->m = message_modulus, key->c = carry_modulus, key->big = ks_in, key->small_ = ks_out, key->n = n, key->k = k;
  key->device = device;
  *out_key = key;
  return MI_OK;
}

int mi_shortint_key_destroy(mi_shortint_key* key) {
  if (!key) return MI_OK;
  if (key->d_luts) {
    DeviceGuard g(key->device);
    (void)hipFree(key->d_luts);
  }
  delete key;
  return MI_OK;
}

int mi_shortint_key_info(const mi_shortint_key* key, int* pbs_engine, int* ms_mode, int* has_ms_noise,
                         uint64_t* message_modulus, uint64_t* carry_modulus, size_t* big_lwe_dim,
                         size_t* small_lwe_dim) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (pbs_engine) *pbs_engine = key->engine;
  if (ms_mode) *ms_mode = key->ms_mode;
  if (has_ms_noise) *has_ms_noise = key->ms_noise != nullptr;
  if (message_modulus) *message_modulus = key->m;
  if (carry_modulus) *carry_modulus = key->c;
  if (big_lwe_dim) *big_lwe_dim = key->big;
  if (small_lwe_dim) *small_lwe_dim = key->small_;
  return MI_OK;
}

int mi_shortint_apply_lut_batch(const mi_shortint_key* key, uint64_t* lwe_out, const uint64_t* lwe_in, size_t n_in,
                                const uint32_t* in_index, const uint64_t* lut_list, const uint32_t* lut_index,
                                size_t n_lut, size_t n_items, void* stream) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (n_in > MAX_ITEMS || n_items > MAX_ITEMS) return fail(MI_ERR_INVALID_ARG, "batch too large");
  if (!in_index && n_items != n_in)
    return fail(MI_ERR_INVALID_ARG, "without in_index every input is one item: n_items must equal n_in");
  if (n_items == 0) return MI_OK;
  if (!lwe_out || !lut_list || (n_in != 0 && !lwe_in)) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (!lut_index && n_lut < n_items)
    return fail(MI_ERR_INVALID_ARG, "without lut_index item b uses lookup table b: n_lut must be at least n_items");
  const size_t big1 = key->big + 1, small1 = key->small_ + 1;
  if (lwe_out != lwe_in && overlap(lwe_out, n_items * big1 * 8, lwe_in, n_in * big1 * 8))
    return fail(MI_ERR_INVALID_ARG, "lwe_out partially overlaps lwe_in");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  if (n_in == 0) return MI_OK;  // every in_index is out of range: every item is left untouched
  const bool drift = key->ms_noise != nullptr, indexed = in_index != nullptr;
  MI_CARVED_SCRATCH(mi::ApplyWork, w, s, n_in, n_items, small1, drift, indexed);
  const uint64_t* cur = w.ks;
  int mode = key->ms_mode;
  MI_TRY(mi_lwe_keyswitch_batch(key->ksk, w.ks, lwe_in, n_in, stream));
  if (drift) {
    int log2n = 0;
    while (((size_t)1 << log2n) < 2 * key->n) ++log2n;
    MI_TRY(mi_lwe_ms_noise_improve_and_switch_batch(key->ms_noise, w.sw, w.ks, n_in, log2n, stream));
    cur = w.sw, mode = MI_MS_PRE_SWITCHED;
  }
  const uint32_t* idx = lut_index;
  if (indexed) {
    MI_TRY(mi_lwe_linear_combination_batch(w.gathered, cur, key->small_, n_in, n_items, 1, in_index, nullptr, nullptr,
                                           key->device, stream));
    MI_TRY_HIP(mi::launch_mask_lut_index(w.eff, in_index, lut_index, n_in, n_items, s), "apply lut index launch");
    cur = w.gathered, idx = w.eff;
  }
  return pbs_call(key, lwe_out, cur, lut_list, idx, n_lut, n_items, mode, stream);
}

int mi_radix_propagate_single_carry_batch(const mi_shortint_key* key, uint64_t* radix, uint64_t* carry_out,
                                          size_t n_blocks, size_t n_integers, void* stream) {
  MI_TRY(check_radix(key, radix, n_blocks, n_integers));
  if (n_blocks > 1 && !single_carry_supported(key->m, key->c)) return single_carry_unsupported();
  if (n_integers == 0) return MI_OK;
  const size_t B = n_blocks, I = n_integers, T = I * B, big1 = key->big + 1;
  // carry_out is written after radix: an overlap would destroy blocks
  if (carry_out && overlap(carry_out, I * big1 * 8, radix, T * big1 * 8))
    return fail(MI_ERR_INVALID_ARG, "carry_out overlaps radix");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const uint32_t t32 = (uint32_t)T, b32 = (uint32_t)B;
  MI_CARVED_SCRATCH(mi::SingleCarryWork, w, s, T, big1);
  const RadixStages sg{key, s, w.ix};
  uint64_t* st = w.work + T * big1;
  const mi::IndexRule row_mod_t = {t32, t32, 0, 0, 0, 0};
  // 1. the message and the state of every block, one keyswitch per block (the state only where something reads it)
  const size_t items1 = B > 1 || carry_out ? 2 * T : T;
  MI_TRY(sg.apply(w.work, radix, T, items1, &row_mod_t, T, LUT_MSG, B, LUT_STATE0, LUT_STATE));
  if (B == 1) {  // nothing to propagate into: the message, and the state of block 0 is the carry
    MI_TRY(sg.gather(radix, w.work, T, T, row_mod_t));
    if (carry_out) MI_TRY(sg.gather(carry_out, w.work, 2 * T, T, {t32, t32, 0, t32, 0, 0}));
    return MI_OK;
  }
  // 2. the scan rounds
  for (size_t sp = 1; sp < B; sp *= 2) {
    const uint32_t s32 = (uint32_t)sp, rem = b32 - s32, c32 = (uint32_t)(I * (B - sp));
    MI_TRY(sg.combine2(w.pack, w.work, 2 * T, c32, {c32, rem, 0, t32 + s32, b32, 0}, {c32, rem, 0, t32, b32, 0},
                       (int64_t)key->m, 1));
    const mi::IndexRule packed_row = {t32, b32, s32, 0, rem, s32};
    MI_TRY(sg.apply(st, w.pack, c32, T, &packed_row, T, LUT_SCAN, 1, LUT_SCAN, LUT_SCAN));
  }
  // 3. message + carry of the block below
  MI_TRY(add_previous(sg, w.pack, w.work, B, T));
  MI_TRY(sg.apply(radix, w.pack, T, T, nullptr, T, LUT_MSG, 1, LUT_MSG, LUT_MSG));
  if (carry_out)  // 4.
    MI_TRY(sg.gather(carry_out, w.work, 2 * T, I, {(uint32_t)I, 1, 0, t32 + b32 - 1, b32, 0}));
  return MI_OK;
}

int mi_radix_full_propagate_batch(const mi_shortint_key* key, uint64_t* radix, size_t n_blocks, size_t n_integers,
                                  void* stream) {
  MI_TRY(check_radix(key, radix, n_blocks, n_integers));
  if (n_integers == 0) return MI_OK;
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  const size_t B = n_blocks, T = n_integers * B, big1 = key->big + 1;
  const bool single = B == 1 || single_carry_supported(key->m, key->c);
  MI_CARVED_SCRATCH(mi::TwoListWork, w, s, T, big1, 2 * T);
  const RadixStages sg{key, s, w.ix};
  const mi::IndexRule row_mod_t = {(uint32_t)T, (uint32_t)T, 0, 0, 0, 0};
  for (size_t r = 0; r < (single ? 1 : B); ++r) {
    MI_TRY(sg.apply(w.both, radix, T, 2 * T, &row_mod_t, T, LUT_MSG, 1, LUT_CARRY, LUT_CARRY));  // 1.
    MI_TRY(add_previous(sg, radix, w.both, B, T));                                                // 2.
  }
  if (single && B > 1) return mi_radix_propagate_single_carry_batch(key, radix, nullptr, B, n_integers, stream);  // 3.
  return MI_OK;
}

int mi_radix_add_batch(const mi_shortint_key* key, uint64_t* radix_out, const uint64_t* lhs, const uint64_t* rhs,
                       uint64_t* carry_out, size_t n_blocks, size_t n_integers, void* stream) {
  MI_TRY(check_radix(key, radix_out, n_blocks, n_integers));
  if (n_blocks > 1 && !single_carry_supported(key->m, key->c)) return single_carry_unsupported();
  if (n_integers == 0) return MI_OK;
  if (!lhs || !rhs) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const size_t T = n_integers * n_blocks, big1 = key->big + 1, bytes = T * big1 * sizeof(uint64_t);
  for (const uint64_t* p : {lhs, rhs})
    if (p != radix_out && overlap(radix_out, bytes, p, bytes))
      return fail(MI_ERR_INVALID_ARG, "radix_out partially overlaps an operand");
  for (const uint64_t* p : {(const uint64_t*)radix_out, lhs, rhs})
    if (carry_out && overlap(carry_out, n_integers * big1 * 8, p, bytes))
      return fail(MI_ERR_INVALID_ARG, "carry_out overlaps radix_out or an operand");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  {
    MI_CARVED_SCRATCH(mi::TwoListWork, w, s, T, big1, (size_t)0);
    const RadixStages sg{key, s, w.ix};
    const uint32_t t32 = (uint32_t)T;
    MI_TRY(stage_pair(w.both, lhs, rhs, bytes, "radix add copy", s));
    MI_TRY(sg.combine2(radix_out, w.both, 2 * T, T, {t32, t32, 0, 0, 0, 0}, {t32, t32, 0, t32, 0, 0}));
  }
  return mi_radix_propagate_single_carry_batch(key, radix_out, carry_out, n_blocks, n_integers, stream);
}

}  // extern "C"
