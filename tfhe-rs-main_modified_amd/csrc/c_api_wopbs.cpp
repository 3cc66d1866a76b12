// c_api_wopbs.cpp — the bootstrap without padding bit (WoP-PBS) of the C ABI: bit extraction, circuit bootstrap, CMUX
// tree, rotation, vertical packing and their composition.  Reference paths relative to tfhe/src/core_crypto:
//   extract_bits                          fft_impl/fft64/crypto/wop_pbs/mod.rs:61-220
//   circuit_bootstrap_boolean             fft_impl/fft64/crypto/wop_pbs/mod.rs:238-339 (homomorphic_shift_boolean :360-435)
//   cmux_tree_memory_optimized            fft_impl/fft64/crypto/wop_pbs/mod.rs:459-583
//   circuit_bootstrap_boolean_vertical_packing   :638-732      vertical_packing :771-825      blind_rotate_assign :838-863
//   the public face                       algorithms/lwe_wopbs.rs
// Every stage is the sequence of the library's public batched entry points that the reference's loop is, with the
// word-wise passes of wopbs.hip in between: nothing is fused across a stage boundary, so each composite equals its
// stages bit for bit.  Scratch is stream-ordered (scratch.hpp) and returned before each entry returns.
#include <string>

#include "c_api_internal.hpp"
#include "carve.hpp"
#include "scratch.hpp"
#include "wopbs_launch.hpp"

using namespace mi::capi;

namespace {

// The CMUX tree's working set: whole trees (2^r GLWEs each) up to this many bytes per chunk, at least one tree.
constexpr size_t WOP_TREE_CAP_BYTES = (size_t)256 << 20;

// what the tree, the rotation and the packing ask of their GGSW list: batch x ggsw_stride GGSWs indexed by a u32
int check_ggsw_list(const mi_fft64_plan* plan, size_t n_outputs, size_t ggsw_stride, size_t first, size_t count,
                    size_t batch) {
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (n_outputs == 0 || n_outputs > 0xFFFFFFull) return fail(MI_ERR_INVALID_ARG, "n_outputs out of range");
  if (first > ggsw_stride || count > ggsw_stride - first)
    return fail(MI_ERR_INVALID_ARG, "the GGSW range exceeds the GGSWs of an item");
  if (batch > 0xFFFFFFull || (batch && ggsw_stride > 0xFFFFFFFFull / batch))
    return fail(MI_ERR_INVALID_ARG, "batch too large");
  return MI_OK;
}

// the argument rules of the vertical packing; *r = the GGSWs that go to the tree
int check_packing(const mi_fft64_plan* plan, size_t n_polys, size_t n_outputs, size_t n_ggsw, int k, int base_log,
                  int level, size_t batch, size_t* r) {
  MI_TRY(check_ggsw_list(plan, n_outputs, n_ggsw, 0, n_ggsw, batch));
  if (n_polys == 0) return fail(MI_ERR_INVALID_ARG, "n_polys is 0");
  if (k < 1) return fail(MI_ERR_INVALID_ARG, "GLWE dimension must be >= 1");
  if (n_ggsw != 0) MI_TRY(check_fft64_shape(plan, k, base_log, level));  // the shape rules of the CMUX
  // :798-811: floor(log2(n_polys)) GGSWs go to the tree, or none when the list is shorter; the tree then asserts that
  // it was given 2^r polynomials
  *r = 63 - (size_t)__builtin_clzll((unsigned long long)n_polys);
  if (*r > n_ggsw) *r = 0;
  if (n_polys != (size_t)1 << *r)
    return fail(MI_ERR_INVALID_ARG, *r ? "the polynomial count of an output must be a power of two"
                                       : "more than one polynomial per output and too few GGSWs for the tree");
  return MI_OK;
}

// the argument rules of the circuit bootstrap (wop_pbs/mod.rs:258-304); fills the pfpksk's shape
struct CbsShape {
  size_t n_keys = 0, pf_in = 0, pf_n = 0;
  int pf_k = 0;
};
int check_cbs(const mi_fft64_pbs_key* bsk, const mi_lwe_pfpksk_list* pfpksk, const mi_fft64_plan* out_plan,
              bool fourier, int delta_log, int base_log_cbs, int level_cbs, CbsShape* sh) {
  if (!bsk || !pfpksk) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  MI_TRY(mi_lwe_pfpksk_list_info(pfpksk, &sh->n_keys, &sh->pf_in, &sh->pf_k, &sh->pf_n, nullptr, nullptr));
  if (level_cbs < 1 || base_log_cbs < 1 || base_log_cbs * level_cbs > 63)
    return fail(MI_ERR_INVALID_ARG, "circuit bootstrap base_log * level must be in [1, 63]");
  if (delta_log < 0 || delta_log > 63) return fail(MI_ERR_INVALID_ARG, "delta_log must be in [0, 63]");
  if (sh->pf_in != (size_t)bsk->k * bsk->plan->n)
    return fail(MI_ERR_INVALID_ARG, "the pfpksk's input dimension must be k * N of the bootstrap key");
  if (sh->n_keys != (size_t)sh->pf_k + 1) return fail(MI_ERR_INVALID_ARG, "the pfpksk list must hold glwe_dim + 1 keys");
  if (fourier && (!out_plan || out_plan->n != sh->pf_n))
    return fail(MI_ERR_INVALID_ARG, "out_plan must be a plan of the pfpksk's polynomial size");
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_fft64_extract_bits_batch(const mi_fft64_pbs_key* bsk, const mi_lwe_ksk* ksk, uint64_t* lwe_list_out,
                                const uint64_t* lwe_in, int delta_log, size_t n_bits, size_t batch, void* stream) {
  if (!bsk || !ksk) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  size_t ks_in = 0, ks_out = 0;
  MI_TRY(mi_lwe_ksk_info(ksk, &ks_in, &ks_out, nullptr, nullptr));
  const size_t big = (size_t)bsk->k * bsk->plan->n;  // the bootstrap's output dimension
  // wop_pbs/mod.rs:102-113
  if (ks_in != big) return fail(MI_ERR_INVALID_ARG, "the keyswitch key's input dimension must be k * N of the bootstrap key");
  if (ks_out != bsk->n_lwe)
    return fail(MI_ERR_INVALID_ARG, "the keyswitch key's output dimension must be the bootstrap key's input dimension");
  // :81-89; bit 0's accumulator holds 2^(delta_log - 1)
  if (delta_log < 0 || n_bits > 64 || (size_t)delta_log + n_bits > 64 || (n_bits > 1 && delta_log < 1))
    return fail(MI_ERR_INVALID_ARG, "delta_log + n_bits must be <= 64 (delta_log >= 1 for more than one bit)");
  if (batch == 0 || n_bits == 0) return MI_OK;
  if (!lwe_list_out || !lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (batch > 0x3FFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(bsk->plan->device);
  const size_t big1 = big + 1, small1 = ks_out + 1, per = ((size_t)bsk->k + 1) * bsk->plan->n;
  MI_CARVED_SCRATCH(mi::ExtractBitsWork, w, s, batch, big1, small1, per);
  const char* what = "extract bits launch";
  MI_TRY_HIP(mi::launch_wop_copy_rows(w.cur, big1, lwe_in, big1, batch, s), what);
  for (size_t bit = 0; bit < n_bits; ++bit) {
    MI_TRY_HIP(mi::launch_wop_lwe_shift(w.tmp, w.cur, big1, batch, 1, 64 - delta_log - (int)bit - 1, 0, s), what);
    MI_TRY(mi_lwe_keyswitch_batch(ksk, w.ks, w.tmp, batch, stream));  // then stored, the MSB at index 0
    MI_TRY_HIP(mi::launch_wop_copy_rows(lwe_list_out + (n_bits - 1 - bit) * small1, n_bits * small1, w.ks, small1,
                                        batch, s),
               what);
    if (bit + 1 == n_bits) break;
    MI_TRY_HIP(mi::launch_wop_body_add(w.ks, small1, batch, 1, 62, 0, s), what);
    MI_TRY_HIP(mi::launch_wop_fill_acc(w.acc, (size_t)bsk->k, bsk->plan->n, 1, delta_log - 1 + (int)bit, 0, s), what);
    MI_TRY(mi_fft64_pbs_batch(bsk, w.tmp, w.ks, w.acc, batch, MI_MS_STANDARD, stream));
    MI_TRY_HIP(mi::launch_wop_body_add(w.tmp, big1, batch, 1, delta_log + (int)bit - 1, 0, s), what);
    MI_TRY_HIP(mi::launch_wop_sub_assign(w.cur, w.tmp, batch * big1, s), what);
  }
  return MI_OK;
}

int mi_fft64_circuit_bootstrap_boolean_batch(const mi_fft64_pbs_key* bsk, const mi_lwe_pfpksk_list* pfpksk,
                                             const mi_fft64_plan* out_plan, uint64_t* ggsw_std_out,
                                             double* ggsw_fourier_out, const uint64_t* lwe_in, size_t batch,
                                             int delta_log, int base_log_cbs, int level_cbs, void* stream) {
  CbsShape sh;
  MI_TRY(check_cbs(bsk, pfpksk, out_plan, ggsw_fourier_out != nullptr, delta_log, base_log_cbs, level_cbs, &sh));
  if (batch == 0) return MI_OK;
  if (!ggsw_std_out && !ggsw_fourier_out) return fail(MI_ERR_INVALID_ARG, "both outputs are NULL");
  const size_t n_keys = sh.n_keys, pf_in = sh.pf_in, pf_n = sh.pf_n;
  if (!lwe_in) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const size_t lv = (size_t)level_cbs;
  if (batch > 0x3FFFFFull / lv) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(bsk->plan->device);
  const size_t items = batch * lv, small1 = bsk->n_lwe + 1, big1 = pf_in + 1;
  const size_t per = ((size_t)bsk->k + 1) * bsk->plan->n, ggsw_words = lv * n_keys * n_keys * pf_n;
  const bool std_out = ggsw_std_out != nullptr;
  MI_CARVED_SCRATCH(mi::CircuitBootstrapWork, w, s, batch, lv, small1, big1, per, ggsw_words, std_out);
  uint64_t* std_ = std_out ? ggsw_std_out : w.ggsw_std;
  // item b * level + output_index: lwe_in[b] 2^(63 - delta_log) + q/4, the accumulator of decomposition level
  // level_cbs - output_index, body constant -2^(63 - base_log (level_cbs - output_index)) (:389-418)
  const int exp0 = 63 - base_log_cbs * level_cbs;
  const char* what = "circuit bootstrap launch";
  MI_TRY_HIP(mi::launch_wop_lwe_shift(w.shifted, lwe_in, small1, batch, lv, 63 - delta_log, (uint64_t)1 << 62, s), what);
  MI_TRY_HIP(mi::launch_wop_fill_acc(w.acc, (size_t)bsk->k, bsk->plan->n, lv, exp0, base_log_cbs, s), what);
  MI_TRY_HIP(mi::launch_wop_iota_mod(w.idx, items, lv, s), what);
  MI_TRY(mi_fft64_pbs_batch_lut_indexed(bsk, w.boot, w.shifted, w.acc, w.idx, lv, items, MI_MS_STANDARD, stream));
  MI_TRY_HIP(mi::launch_wop_body_add(w.boot, big1, items, lv, exp0, base_log_cbs, s), what);
  MI_TRY(mi_lwe_pfpks_batch(pfpksk, std_, w.boot, items, stream));
  if (ggsw_fourier_out)  // fill_with_forward_fourier
    return mi_bsk_to_fourier64(out_plan, std_, ggsw_fourier_out, items * n_keys * n_keys, stream);
  return MI_OK;
}

int mi_fft64_cmux_tree_batch(const mi_fft64_plan* plan, uint64_t* glwe_out, const uint64_t* lut_polys, size_t n_polys,
                             size_t n_outputs, const double* ggsw_fourier_list, size_t ggsw_stride, size_t ggsw_first,
                             size_t r, int k, int base_log, int level, size_t batch, void* stream) {
  MI_TRY(check_ggsw_list(plan, n_outputs, ggsw_stride, ggsw_first, r, batch));
  // cmux_tree_memory_optimized asserts polynomial_count == 1 << ggsw count (:466)
  if (r > 40 || n_polys != (size_t)1 << r)
    return fail(MI_ERR_INVALID_ARG, "the tree takes 2^r polynomials for its r GGSWs");
  if (k < 1) return fail(MI_ERR_INVALID_ARG, "GLWE dimension must be >= 1");
  if (r != 0) MI_TRY(check_fft64_shape(plan, k, base_log, level));  // the shape rules of the CMUX
  if (batch == 0) return MI_OK;
  if (!glwe_out || !lut_polys || (r != 0 && !ggsw_fourier_list)) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(plan->device);
  const int logn = __builtin_ctzll((unsigned long long)plan->n);
  const size_t per = ((size_t)k + 1) * plan->n, total = batch * n_outputs;
  if (r == 0)  // the trivial GLWE of the one polynomial (:577-581): the leaves are the output
    return hip_status(mi::launch_wop_tree_leaves(glwe_out, lut_polys, (size_t)k, logn, 1, 0, total, 0, n_outputs, s),
                      "cmux tree launch");
  const size_t tree_bytes = (per * sizeof(uint64_t)) << r;
  size_t chunk = WOP_TREE_CAP_BYTES / tree_bytes;
  chunk = chunk < 1 ? 1 : chunk > total ? total : chunk;
  const size_t half0 = (size_t)1 << (r - 1);
  if (chunk * half0 > 0x7FFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  mi::ScratchBuf nodes(chunk * tree_bytes, s), idx(chunk * half0 * sizeof(uint32_t), s);
  if (!nodes.ok() || !idx.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  uint64_t* buf = (uint64_t*)nodes.ptr();
  for (size_t t0 = 0; t0 < total; t0 += chunk) {
    const size_t trees = chunk < total - t0 ? chunk : total - t0;
    MI_TRY_HIP(mi::launch_wop_tree_leaves(buf, lut_polys, (size_t)k, logn, n_polys, (int)r, trees, t0, n_outputs, s),
               "cmux tree launch");
    // layer j: the last GGSW first (.rev(), :534); ct0 = the first half of the positions, ct1 = the second
    for (size_t j = 0; j < r; ++j) {
      const size_t items = trees << (r - 1 - j);
      MI_TRY_HIP(mi::launch_wop_ggsw_index((uint32_t*)idx.ptr(), items, trees, t0, n_outputs, ggsw_stride,
                                           ggsw_first + r - 1 - j, s),
                 "cmux tree launch");
      MI_TRY(mi_fft64_cmux_batch_indexed(plan, buf, buf + items * per, ggsw_fourier_list, (const uint32_t*)idx.ptr(),
                                         batch * ggsw_stride, k, base_log, level, items, stream));
    }
    MI_TRY_HIP(mi::launch_wop_copy_rows(glwe_out + t0 * per, per, buf, per, trees, s), "cmux tree launch");
  }
  return MI_OK;
}

int mi_fft64_wop_blind_rotate_batch(const mi_fft64_plan* plan, uint64_t* glwe, size_t n_outputs,
                                    const double* ggsw_fourier_list, size_t ggsw_stride, size_t ggsw_first,
                                    size_t n_rot, int k, int base_log, int level, size_t batch, void* stream) {
  MI_TRY(check_ggsw_list(plan, n_outputs, ggsw_stride, ggsw_first, n_rot, batch));
  if (k < 1) return fail(MI_ERR_INVALID_ARG, "GLWE dimension must be >= 1");
  MI_TRY(check_fft64_shape(plan, k, base_log, level));  // the shape rules of the CMUX
  if (batch == 0 || n_rot == 0) return MI_OK;
  if (!glwe || !ggsw_fourier_list) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(plan->device);
  const int logn = __builtin_ctzll((unsigned long long)plan->n);
  const size_t per = ((size_t)k + 1) * plan->n, items = batch * n_outputs;
  if (items > 0x7FFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  mi::ScratchBuf ct1(items * per * sizeof(uint64_t), s), idx(items * sizeof(uint32_t), s);
  if (!ct1.ok() || !idx.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  const char* what = "wop blind rotate launch";
  // from the last GGSW to the first: ct1 = ct0 / X^d, d <- 2 d from 1, CMUX (:844-862); the degree acts mod 2N, and the
  // reference's shifted usize is 0 from 2^64 on as well
  for (size_t i = 0; i < n_rot; ++i) {
    const uint64_t degree = i < 64 ? (uint64_t)1 << i : 0;
    MI_TRY_HIP(mi::launch_wop_monomial_div((uint64_t*)ct1.ptr(), glwe, items * ((size_t)k + 1), logn, degree, s), what);
    MI_TRY_HIP(mi::launch_wop_ggsw_index((uint32_t*)idx.ptr(), items, items, 0, n_outputs, ggsw_stride,
                                         ggsw_first + n_rot - 1 - i, s),
               what);
    MI_TRY(mi_fft64_cmux_batch_indexed(plan, glwe, (uint64_t*)ct1.ptr(), ggsw_fourier_list, (const uint32_t*)idx.ptr(),
                                       batch * ggsw_stride, k, base_log, level, items, stream));
  }
  return MI_OK;
}

int mi_fft64_vertical_packing_batch(const mi_fft64_plan* plan, uint64_t* lwe_out, const uint64_t* lut_polys,
                                    size_t n_polys, size_t n_outputs, const double* ggsw_fourier_list, size_t n_ggsw,
                                    int k, int base_log, int level, size_t batch, void* stream) {
  size_t r = 0;
  MI_TRY(check_packing(plan, n_polys, n_outputs, n_ggsw, k, base_log, level, batch, &r));
  if (batch == 0) return MI_OK;
  if (!lwe_out || !lut_polys || (n_ggsw != 0 && !ggsw_fourier_list)) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(plan->device);
  const size_t per = ((size_t)k + 1) * plan->n, items = batch * n_outputs;
  mi::ScratchBuf glwe(items * per * sizeof(uint64_t), s);
  if (!glwe.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  uint64_t* acc = (uint64_t*)glwe.ptr();
  MI_TRY(mi_fft64_cmux_tree_batch(plan, acc, lut_polys, n_polys, n_outputs, ggsw_fourier_list, n_ggsw, 0, r, k, base_log,
                                  level, batch, stream));
  MI_TRY(mi_fft64_wop_blind_rotate_batch(plan, acc, n_outputs, ggsw_fourier_list, n_ggsw, r, n_ggsw - r, k, base_log,
                                         level, batch, stream));
  return mi_sample_extract_batch(lwe_out, acc, plan->n, k, items, 0, 0, 1, 0, plan->device, stream);
}

int mi_fft64_circuit_bootstrap_boolean_vertical_packing_batch(
    const mi_fft64_pbs_key* bsk, const mi_lwe_pfpksk_list* pfpksk, const mi_fft64_plan* out_plan, uint64_t* lwe_out,
    const uint64_t* lwe_list_in, size_t n_bits, const uint64_t* big_lut, size_t n_polys, size_t n_outputs,
    int base_log_cbs, int level_cbs, size_t batch, void* stream) {
  // the argument rules of both stages, before any work (the packing's at batch 0: the batch is checked below)
  CbsShape sh;
  MI_TRY(check_cbs(bsk, pfpksk, out_plan, true, 63, base_log_cbs, level_cbs, &sh));
  const size_t n_keys = sh.n_keys, pf_n = sh.pf_n;
  const int pf_k = sh.pf_k;
  size_t r = 0;
  MI_TRY(check_packing(out_plan, n_polys, n_outputs, n_bits, pf_k, base_log_cbs, level_cbs, 0, &r));
  if (batch == 0) return MI_OK;
  if (!lwe_out || !big_lut || (n_bits != 0 && !lwe_list_in)) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (n_bits != 0 && batch > 0x3FFFFFull / n_bits) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(out_plan->device);
  // the Fourier GGSW list (:676-697): one GGSW per input bit, DeltaLog(63) (:712)
  const size_t ggsw_doubles = (size_t)level_cbs * n_keys * n_keys * pf_n;  // N / 2 complex per polynomial
  mi::ScratchBuf ggsw(s);
  if (n_bits != 0) {
    if (!ggsw.alloc(batch * n_bits * ggsw_doubles * sizeof(double))) return fail(MI_ERR_OOM, "scratch allocation failed");
    MI_TRY(mi_fft64_circuit_bootstrap_boolean_batch(bsk, pfpksk, out_plan, nullptr, (double*)ggsw.ptr(), lwe_list_in,
                                                    batch * n_bits, 63, base_log_cbs, level_cbs, stream));
  }
  return mi_fft64_vertical_packing_batch(out_plan, lwe_out, big_lut, n_polys, n_outputs, (const double*)ggsw.ptr(),
                                         n_bits, pf_k, base_log_cbs, level_cbs, batch, stream);
}

}  // extern "C"
