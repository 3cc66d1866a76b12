/*
 * tfhe_ntt_amd.h — C ABI of the MI355X-native negacyclic NTT engine.
 *
 * Drop-in boundary for the tfhe-ntt `prime64::Plan` hot path (reference paths relative to
 * /root/reference).  Every entry point is `extern "C"`, takes plain pointers and sizes, never
 * aborts, and returns an `mi_status` (0 = OK).  Buffers are caller-owned; device pointers are
 * HIP device allocations on the plan's device; `stream` is a `hipStream_t` passed as `void*`
 * (NULL = the legacy default stream).  All `_batch` calls are asynchronous on `stream`.
 *
 * Batch layout: `batch` polynomials of `n` u64 coefficients, polynomial b starting at
 * `buf + b * stride` (stride >= n, in u64 units).  Values must be canonical (< p): inputs >= p
 * are outside the reference's domain (the reference test asserts it, prime64.rs:1328-1333).
 */
#ifndef TFHE_NTT_AMD_H
#define TFHE_NTT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mi_status {
    MI_OK = 0,
    MI_ERR_INVALID_ARG = 1, /* N not a power of two / N < 16 / bad pointer or stride  */
    MI_ERR_NOT_PRIME = 2,   /* modulus fails is_prime64 (prime.rs:76-128)             */
    MI_ERR_NO_ROOT = 3,     /* no primitive 2N-th root of unity mod p (roots.rs:68-91) */
    MI_ERR_HIP = 4,         /* a HIP runtime call failed (see mi_last_error_message)  */
    MI_ERR_OOM = 5,         /* device allocation failed                               */
    MI_ERR_UNSUPPORTED = 6  /* valid request outside what this build implements       */
} mi_status;

typedef struct mi_ntt64_plan mi_ntt64_plan;

/* Human-readable text for a status code, and the detail of the last error on this thread. */
const char *mi_status_string(int status);
const char *mi_last_error_message(void);
/* Build provenance (no reference counterpart): sha256 of the sources this library was built from
 * (tools/source_hash.py: csrc sources and headers, the asm-body generators, this header, the Makefile), so a
 * caller can tell whether the loaded library matches the tree beside it. */
const char *mi_build_source_hash(void);

/* ---- Plan -------------------------------------------------------------------------------
 * Replaces tfhe_ntt::prime64::Plan::try_new (tfhe-ntt/src/prime64.rs:764-862): the reference
 * returns None for N < 16, N not a power of two, p not prime, or no 2N-th root; here those are
 * MI_ERR_INVALID_ARG / MI_ERR_NOT_PRIME / MI_ERR_NO_ROOT.  Twiddles are built on the host exactly
 * as init_negacyclic_twiddles (prime64.rs:159-204) and uploaded to `device`.  A plan is immutable
 * after creation and may be shared by any number of streams / host threads.  Sizes 16 <= N <= 2^31
 * (the Solinas field's 2N-th roots end at 2N = 2^32, roots.rs:96-107); N > 2^14 runs as passes of
 * top stages through HBM plus 2^14-element blocks. */
int mi_ntt64_plan_create(size_t n, uint64_t p, int device, mi_ntt64_plan **out_plan);
int mi_ntt64_plan_destroy(mi_ntt64_plan *plan);

/* The process-wide plan cache of Ntt64::new (tfhe/src/core_crypto/commons/math/ntt/ntt64.rs:27-79):
 * one immutable plan per (n, p, device), built on first use (concurrent first callers build it once)
 * and shared by every later caller and thread; later lookups are a read-locked map probe.  Cached
 * plans live until process exit, as the reference's static PLANS map; mi_ntt64_plan_destroy on one
 * is a no-op.  Same status codes as mi_ntt64_plan_create (the reference panics where it is None). */
int mi_ntt64_plan_cached(size_t n, uint64_t p, int device, const mi_ntt64_plan **out_plan);

/* Plan::ntt_size / Plan::modulus (prime64.rs:870-878); also the device the plan lives on. */
int mi_ntt64_plan_info(const mi_ntt64_plan *plan, size_t *n, uint64_t *p, int *device);

/* Host copies of the canonical twiddle tables (twid[bitrev(k)] = w^k, inv_twid as prime64.rs:193-199)
 * and N^{-1} mod p (prime64.rs:844).  Each table has n entries.  Any pointer may be NULL. */
int mi_ntt64_plan_twiddles(const mi_ntt64_plan *plan, uint64_t *twid, uint64_t *inv_twid, uint64_t *n_inv);

/* ---- Transforms (device pointers, async) -----------------------------------------------
 * Plan::fwd (prime64.rs:897-968): natural order in, bit-reversed NTT order out, in place.
 * Plan::inv (prime64.rs:975-1046): bit-reversed in, natural order out, unnormalised (x N). */
int mi_ntt64_fwd_batch(const mi_ntt64_plan *plan, uint64_t *buf, size_t batch, size_t stride, void *stream);
int mi_ntt64_inv_batch(const mi_ntt64_plan *plan, uint64_t *buf, size_t batch, size_t stride, void *stream);

/* ---- Pointwise ops (device pointers, async), all in the NTT domain -----------------------
 * Plan::normalize            (prime64.rs:1137-1179): x   = x * N^{-1}             mod p
 * Plan::mul_assign_normalize (prime64.rs:1050-1133): lhs = lhs * rhs * N^{-1}     mod p
 * Plan::mul_accumulate       (prime64.rs:1182-1222): acc = acc + lhs * rhs        mod p
 * The three operands of a call share one `stride`. */
int mi_ntt64_normalize_batch(const mi_ntt64_plan *plan, uint64_t *buf, size_t batch, size_t stride, void *stream);
int mi_ntt64_mul_assign_normalize_batch(const mi_ntt64_plan *plan, uint64_t *lhs, const uint64_t *rhs,
                                        size_t batch, size_t stride, void *stream);
int mi_ntt64_mul_accumulate_batch(const mi_ntt64_plan *plan, uint64_t *acc, const uint64_t *lhs,
                                  const uint64_t *rhs, size_t batch, size_t stride, void *stream);

/* ---- The Ntt64View layer (tfhe/src/core_crypto/commons/math/ntt/ntt64.rs:81-266), batched -------------------
 * The per-polynomial helpers every tfhe-rs NTT consumer calls (ntt64_pbs.rs:600-663, ntt64_bnf_pbs.rs:596-681,
 * lwe_bootstrap_key_conversion.rs:294-365), over `batch` polynomials of the plan's size `stride` u64 apart in both
 * operands (device pointers, async on `stream`).  Any plan; the Solinas N = 2048 plan runs them as one fused launch
 * each.  Results equal the reference's bit for bit, including what it leaves in its buffers.
 *   forward             Ntt64View::forward (:89-95):            ntt = fwd(standard)
 *   forward_normalized  Ntt64View::forward_normalized (:97-108): ntt = normalize(fwd(standard))
 *   forward_from_power_of_two_modulus (:201-214): ntt = fwd(switch(standard)), switch x -> ((x >> (64 - w)) p
 *                       + 2^(w-1)) >> w (modswitch_from_power_of_two_to_ntt_prime, :166-177), w in [1, 64]
 *   forward_from_decomp (:221-240): ntt = fwd(d), d = x + p (wrapping) where x < 0 as an i64, else x
 * For these four `ntt` may equal the input buffer (in place) or be disjoint from it.
 *   add_backward (:110-131): ntt = inv(ntt) (in place, as Plan::inv), standard = wrapping_add_custom_mod(standard,
 *                       ntt, p) (commons/numeric/unsigned.rs:174-187); standard canonical (< p)
 *   add_backward_on_power_of_two_modulus (:244-266): ntt = switch(inv(ntt)) with switch v -> (((v << w) | p >> 1) / p)
 *                       << (64 - w) (modswitch_from_ntt_prime_to_power_of_two, :184-196: an OR, not an add), then
 *                       standard += ntt (wrapping), w in [1, 64]
 * For these two `standard` and `ntt` must be disjoint.  A width outside [1, 64] (the reference's shifts overflow there)
 * or overlapping operands are MI_ERR_INVALID_ARG. */
int mi_ntt64_forward_batch(const mi_ntt64_plan *plan, uint64_t *ntt, const uint64_t *standard, size_t batch,
                           size_t stride, void *stream);
int mi_ntt64_forward_normalized_batch(const mi_ntt64_plan *plan, uint64_t *ntt, const uint64_t *standard, size_t batch,
                                      size_t stride, void *stream);
int mi_ntt64_forward_from_power_of_two_modulus_batch(const mi_ntt64_plan *plan, unsigned input_modulus_width,
                                                     uint64_t *ntt, const uint64_t *standard, size_t batch,
                                                     size_t stride, void *stream);
int mi_ntt64_forward_from_decomp_batch(const mi_ntt64_plan *plan, uint64_t *ntt, const uint64_t *decomp, size_t batch,
                                       size_t stride, void *stream);
int mi_ntt64_add_backward_batch(const mi_ntt64_plan *plan, uint64_t *standard, uint64_t *ntt, size_t batch,
                                size_t stride, void *stream);
int mi_ntt64_add_backward_on_power_of_two_modulus_batch(const mi_ntt64_plan *plan, unsigned output_modulus_width,
                                                        uint64_t *standard, uint64_t *ntt, size_t batch, size_t stride,
                                                        void *stream);

/* ---- Host-pointer convenience (copy in, run, copy out, synchronise) ---------------------
 * The single-polynomial `&mut [u64]` form of Plan::fwd / Plan::inv, batched; used by config 1
 * plumbing and the tests.  `buf` holds batch * n contiguous u64 on the host. */
int mi_ntt64_fwd_host(const mi_ntt64_plan *plan, uint64_t *buf, size_t batch);
int mi_ntt64_inv_host(const mi_ntt64_plan *plan, uint64_t *buf, size_t batch);
/* The same host form of the pointwise ops, on `batch` contiguous polynomials per operand, through the pooled
 * staging slots of mi_ntt64_fwd_host (no allocation, no device synchronisation in the steady state):
 * Plan::normalize (prime64.rs:1137-1179), Plan::mul_assign_normalize (prime64.rs:1050-1133),
 * Plan::mul_accumulate (prime64.rs:1182-1222) — what Ntt64View's update_with_fmadd reaches per polynomial
 * (ntt64_pbs.rs:683-702). */
int mi_ntt64_normalize_host(const mi_ntt64_plan *plan, uint64_t *buf, size_t batch);
int mi_ntt64_mul_assign_normalize_host(const mi_ntt64_plan *plan, uint64_t *lhs, const uint64_t *rhs, size_t batch);
int mi_ntt64_mul_accumulate_host(const mi_ntt64_plan *plan, uint64_t *acc, const uint64_t *lhs, const uint64_t *rhs,
                                 size_t batch);

/* ---- Synthetic input (device, async) ----------------------------------------------------
 * Fills `count` u64 with the counter-based generator of SURVEY.md §8d (splitmix64 finaliser over
 * seed + (i+1)*G + k*H, top bits dropped to bitlen(p), rejection to [0,p); p = 0: full u64 range).  Identical stream to
 * the oracle's ora_fill_uniform, so GPU-generated batches can be checked on the host. */
int mi_fill_uniform(uint64_t *buf, size_t count, uint64_t seed, uint64_t p, int device, void *stream);

/* ---- External product / CMUX / PBS (core_crypto consumers of the plan) -------------------
 * Reference paths below are relative to /root/reference/tfhe/src/core_crypto.  These run for the
 * Solinas plan (p = 2^64 - 2^32 + 1), any decomposition with base_log * level < 64, at the shapes
 *   N in {1024, 2048, 4096} with GLWE dimension k in {1, 2};
 *   N = 512 with k in {1, 4}        (shortint PARAM_MESSAGE_1_CARRY_1: N 512, k 4);
 *   N in {8192, ..., 131072} with k in {1, 2} (PARAM_MESSAGE_3_CARRY_3: N 8192, 4_4: N 65536; the accumulators of
 *                                    a chunk of ciphertexts live in HBM and each CMUX step is a sequence of
 *                                    device-wide passes);
 * other plans / shapes return MI_ERR_UNSUPPORTED.  The N = 2048, k = 1, level-1 shapes run on the hand-scheduled
 * engine, N <= 4096 on the fused one-workgroup-per-ciphertext kernels.
 * Layouts are the reference's entity layouts, contiguous:
 *   GLWE       : (k+1) polynomials of N u64 (mask then body)
 *   GGSW (NTT) : level-major, highest level first; per level (k+1) rows x (k+1) columns of N u64,
 *                each polynomial in the plan's forward (bit-reversed) NTT order
 *   BSK  (NTT) : n_lwe GGSWs back to back ((k+1)^2 * level * N u64 each)
 *   LWE        : mask (dimension u64) then body
 * Variant MI_NTT64_SOLINAS works modulo p (algorithms/lwe_programmable_bootstrapping/ntt64_pbs.rs);
 * MI_NTT64_BNF works on native 2^64 ciphertexts with the back-and-forth modulus switch
 * (ntt64_bnf_pbs.rs). */
typedef enum mi_ntt64_variant { MI_NTT64_SOLINAS = 0, MI_NTT64_BNF = 1 } mi_ntt64_variant;

/* Modulus switch of the PBS input: standard rounding (fft_impl/common.rs:10-23, as
 * ntt64_bnf_pbs.rs:512; ntt64_pbs.rs:540-549 for Solinas), the centered-binary variant the shortint
 * parameters use (BNF only, algorithms/modulus_switch.rs:35-104), or PRE_SWITCHED: lwe_in already
 * holds the switched values in [0, 2N) (the ModulusSwitchedLweCiphertext input of
 * blind_rotate_ntt64[_bnf]_assign_mem_optimized, ntt64_bnf_pbs.rs:208-266 / ntt64_pbs.rs:213-286). */
typedef enum mi_ms_mode { MI_MS_STANDARD = 0, MI_MS_CENTERED = 1, MI_MS_PRE_SWITCHED = 2 } mi_ms_mode;

/* convert_standard_lwe_bootstrap_key_to_ntt64 (algorithms/lwe_bootstrap_key_conversion.rs:294-365)
 * over `n_polys` polynomials (= n_lwe * (k+1)^2 * level): bsk_ntt = fwd(switch(bsk_std)) [* N^{-1}],
 * where switch = forward_from_power_of_two_modulus (commons/math/ntt/ntt64.rs:166-178) from a
 * 2^in_modulus_width modulus when in_modulus_width > 0, identity when 0 (Solinas-modulus keys).
 * normalize != 0 is NttLweBootstrapKeyOption::Normalize.  Device pointers, may not alias. */
int mi_bsk_to_ntt64(const mi_ntt64_plan *plan, const uint64_t *bsk_std, uint64_t *bsk_ntt, size_t n_polys,
                    unsigned in_modulus_width, int normalize, void *stream);

/* out_glwe[b] += GGSW (.) in_glwe[b] for b < batch, one shared NTT-domain GGSW:
 * add_external_product_ntt64_assign (ntt64_pbs.rs:553-663) or, for MI_NTT64_BNF,
 * add_external_product_ntt64_bnf_assign (ntt64_bnf_pbs.rs:541-681; GGSW converted Raw). */
int mi_ext_product_ntt64_batch(const mi_ntt64_plan *plan, uint64_t *out_glwe, const uint64_t *in_glwe,
                               const uint64_t *ggsw_ntt, int k, int base_log, int level, size_t batch, int variant,
                               void *stream);

/* CMUX, per item: ct1[b] -= ct0[b]; ct0[b] += GGSW (.) ct1[b] — cmux_ntt64_assign (ntt64_pbs.rs:669-680)
 * / cmux_ntt64_bnf_assign (ntt64_bnf_pbs.rs:683-705); like the reference, ct1 is left holding ct1 - ct0. */
int mi_cmux_ntt64_batch(const mi_ntt64_plan *plan, uint64_t *ct0, uint64_t *ct1, const uint64_t *ggsw_ntt, int k,
                        int base_log, int level, size_t batch, int variant, void *stream);
/* The same with one GGSW per item ("one shared GGSW or a per-item GGSW index array"): item b uses
 * GGSW ggsw_index[b] of the n_ggsw GGSWs stored back to back in ggsw_list (device u32 array of `batch` entries);
 * an item whose index is >= n_ggsw is left untouched (both its GLWEs), so a bad index never reads outside the
 * list.  Useful for batched CMUX trees and per-ciphertext selectors. */
int mi_ext_product_ntt64_batch_indexed(const mi_ntt64_plan *plan, uint64_t *out_glwe, const uint64_t *in_glwe,
                                       const uint64_t *ggsw_list, const uint32_t *ggsw_index, size_t n_ggsw, int k,
                                       int base_log, int level, size_t batch, int variant, void *stream);
int mi_cmux_ntt64_batch_indexed(const mi_ntt64_plan *plan, uint64_t *ct0, uint64_t *ct1, const uint64_t *ggsw_list,
                                const uint32_t *ggsw_index, size_t n_ggsw, int k, int base_log, int level,
                                size_t batch, int variant, void *stream);

/* A GGSW list made ready for repeated external products / CMUXes (the reference's NttGgswCiphertext[List] kept in the
 * NTT domain, entities/ntt_ggsw_ciphertext_list.rs): n_ggsw GGSWs back to back (layout above) on the plan's device.
 * The fused N = 2048, k = 1, level-1 bodies read their GGSW in their own coefficient order (pbs_tw.hip), so for that
 * shape the list is permuted once into a private copy (on `stream`, synchronised before returning; the caller's
 * buffer may then be freed); every other shape references the caller's list (keep it alive).  The raw-pointer calls
 * above permute a twisted-shape GGSW on every call. */
typedef struct mi_ntt64_ggsw mi_ntt64_ggsw;
int mi_ntt64_ggsw_create(const mi_ntt64_plan *plan, const uint64_t *ggsw_list, size_t n_ggsw, int k, int base_log,
                         int level, int variant, void *stream, mi_ntt64_ggsw **out);
int mi_ntt64_ggsw_destroy(mi_ntt64_ggsw *ggsw);
int mi_ntt64_ggsw_info(const mi_ntt64_ggsw *ggsw, size_t *n_ggsw, int *k, int *base_log, int *level, int *variant);
/* mi_ext_product_ntt64_batch / mi_cmux_ntt64_batch on a prepared list: ggsw_index NULL = GGSW 0 for every item, else
 * item b uses GGSW ggsw_index[b] (an index >= n_ggsw leaves the item untouched, as the _indexed calls). */
int mi_ext_product_ntt64_prepared_batch(const mi_ntt64_ggsw *ggsw, uint64_t *out_glwe, const uint64_t *in_glwe,
                                        const uint32_t *ggsw_index, size_t batch, void *stream);
int mi_cmux_ntt64_prepared_batch(const mi_ntt64_ggsw *ggsw, uint64_t *ct0, uint64_t *ct1, const uint32_t *ggsw_index,
                                 size_t batch, void *stream);

/* A bootstrap key made ready for mi_pbs_ntt64_batch on the plan's device.  MI_NTT64_BNF keys
 * (converted Raw, as ntt64_bnf_pbs.rs tests do) are copied once with N^{-1} folded in — the
 * reference normalises each product at run time (ntt64_bnf_pbs.rs:670); in exact mod-p arithmetic
 * both orders give identical values.  Keys of the fused N = 2048, k = 1, level-1 engine (either variant) are
 * copied once in the order its blind rotation reads (pbs_tw.hip prepare_tw_key_kernel); other
 * MI_NTT64_SOLINAS keys are referenced, not copied (the caller keeps `bsk_ntt` alive).  Replaces the
 * reference's PodStack scratch (ntt64_pbs.rs:705-751). */
typedef struct mi_pbs_ntt64_key mi_pbs_ntt64_key;
/* The copy runs on `stream` (the stream that produced bsk_ntt) and synchronises it before returning. */
int mi_pbs_ntt64_key_create(const mi_ntt64_plan *plan, const uint64_t *bsk_ntt, size_t n_lwe, int k, int base_log,
                            int level, int variant, void *stream, mi_pbs_ntt64_key **out_key);
int mi_pbs_ntt64_key_destroy(mi_pbs_ntt64_key *key);
/* n_lwe, k, base_log, level, variant of a key (any pointer may be NULL). */
int mi_pbs_ntt64_key_info(const mi_pbs_ntt64_key *key, size_t *n_lwe, int *k, int *base_log, int *level,
                          int *variant);

/* ---- On-disk NTT bootstrap key (entities/ntt_lwe_bootstrap_key.rs:26-33) -----------------------
 * MI_NTT_BSK_PLAIN     = bincode::serialize(&NttLweBootstrapKey<ABox<[u64]>>) (bincode 1.3, fixint,
 *                        little-endian): u64 count, count u64 (n_lwe, level, k+1, k+1, N NTT-domain
 *                        coefficients), polynomial_size, glwe_size, level, base_log as u64, the
 *                        SerializableCiphertextModulus (u128 modulus, u64 scalar_bits = 64).
 * MI_NTT_BSK_VERSIONED = bincode of key.versionize() (tfhe-versionable; the type has no `Named` impl,
 *                        so this is its whole versioned form): u32 1 (NttLweBootstrapKeyVersions::V1),
 *                        u32 1 (NttGgswCiphertextListVersions::V1), the data sequence, then every scalar
 *                        field behind its own u32 version tag 0 (PolynomialSizeVersions::V0, ...,
 *                        SerializableCiphertextModulusVersions::V0).
 * An NTT key's modulus is the NTT prime for both PBS variants (ntt64_bnf_pbs.rs:44-94; Ntt64::new
 * asserts a custom modulus, ntt64.rs:38); whether the values are Raw (BNF) or Normalize (Solinas) is not
 * stored, so loaders take the variant explicitly. */
typedef enum mi_ntt_bsk_format { MI_NTT_BSK_PLAIN = 0, MI_NTT_BSK_VERSIONED = 1 } mi_ntt_bsk_format;
typedef struct mi_ntt_bsk_header {
    uint64_t polynomial_size, glwe_size, level, base_log;
    uint64_t modulus_lo, modulus_hi; /* u128 ciphertext modulus (0 = native 2^64)                   */
    uint64_t input_lwe_dimension;    /* count / (level * glwe_size^2 * polynomial_size)              */
    uint64_t count;                  /* u64 elements of the key data                                 */
    uint64_t data_offset;            /* byte offset of the first element in the serialised buffer    */
} mi_ntt_bsk_header;
/* Parses and validates `len` bytes (truncated / trailing bytes, unknown version tags, scalar_bits != 64
 * as the reference's TryFrom<SerializableCiphertextModulus>, a modulus above 2^64, data that is not a
 * whole number of GGSWs, size fields whose product overflows): MI_ERR_INVALID_ARG with the reason in
 * mi_last_error_message.  A modulus of 2^64 is canonicalised to 0 (native), as TryFrom does. */
int mi_ntt_bsk_parse(const uint8_t *bytes, size_t len, int format, mi_ntt_bsk_header *out);
/* Bytes `mi_ntt_bsk_write` produces for header `h` (h->count elements; data_offset ignored). */
int mi_ntt_bsk_serialized_size(const mi_ntt_bsk_header *h, int format, size_t *out_len);
/* Serialises host `data` (h->count u64) into `out` (exactly the serialized size). */
int mi_ntt_bsk_write(const mi_ntt_bsk_header *h, const uint64_t *data, int format, uint8_t *out, size_t out_len);
/* Loads serialised key bytes (host memory) straight into HBM on the plan's device (one host-to-device
 * copy on `stream`, no re-layout) and makes a PBS key of `variant` that owns the upload: the stored
 * polynomial size must equal the plan's, glwe_size 2, and the modulus the plan's prime. */
int mi_pbs_ntt64_key_load(const mi_ntt64_plan *plan, const uint8_t *bytes, size_t len, int format, int variant,
                          void *stream, mi_pbs_ntt64_key **out_key);

/* Batched programmable bootstrap: lwe_out[b] = SampleExtract_0(BlindRotate(lut, lwe_in[b])).
 * programmable_bootstrap_ntt64_bnf_lwe_ciphertext_mem_optimized (ntt64_bnf_pbs.rs:469-540) or
 * programmable_bootstrap_ntt64_lwe_ciphertext_mem_optimized (ntt64_pbs.rs:482-538).
 * lwe_in: batch x (n_lwe + 1) u64; lut: one GLWE shared by the batch; lwe_out: batch x (k*N + 1). */
int mi_pbs_ntt64_batch(const mi_pbs_ntt64_key *key, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *lut,
                       size_t batch, int ms_mode, void *stream);

/* The same bootstrap with one LUT per item (the CUDA backend's lut_indexes, backends/tfhe-cuda-backend/cuda/include/
 * pbs/programmable_bootstrap.h:41; the shortint many-LUT / per-block LUT batches): lut_list holds n_lut GLWEs
 * ((k+1) N u64 each), item b uses GLWE lut_index[b] (device u32 array of `batch` entries).  An item whose index is
 * >= n_lut is left untouched (lwe_out[b] not written).  lut_index NULL: item b uses GLWE b (n_lut >= batch). */
int mi_pbs_ntt64_batch_lut_indexed(const mi_pbs_ntt64_key *key, uint64_t *lwe_out, const uint64_t *lwe_in,
                                   const uint64_t *lut_list, const uint32_t *lut_index, size_t n_lut, size_t batch,
                                   int ms_mode, void *stream);

/* Batched GLWE-output blind rotation, in place: acc_glwe[b] <- BlindRotate(acc_glwe[b], lwe_in[b]) for b < batch,
 * every item rotating its own accumulator (one LUT per ciphertext).
 *   MI_NTT64_BNF     : blind_rotate_ntt64_bnf_assign[_mem_optimized] (ntt64_bnf_pbs.rs:174-266): the CMUX loop over
 *                      the switched mask, then the division by X^ms(body).  The reference takes a
 *                      ModulusSwitchedLweCiphertext; here lwe_in is the native LWE switched inside the kernel
 *                      (MI_MS_STANDARD = lwe_ciphertext_modulus_switch, MI_MS_CENTERED = the centered binary switch,
 *                      algorithms/modulus_switch.rs) or already switched (MI_MS_PRE_SWITCHED, values in [0, 2N)).
 *   MI_NTT64_SOLINAS : blind_rotate_ntt64_assign[_mem_optimized] (ntt64_pbs.rs:176-286): the division by
 *                      X^ms(body) first, then the loop; lwe_in modulo p (MI_MS_STANDARD) or PRE_SWITCHED.
 * acc_glwe: batch x (k+1) x N u64 on the key's device.  Same shapes as mi_pbs_ntt64_batch. */
int mi_blind_rotate_ntt64_batch(const mi_pbs_ntt64_key *key, uint64_t *acc_glwe, const uint64_t *lwe_in, size_t batch,
                                int ms_mode, void *stream);

/* extract_lwe_sample_from_glwe_ciphertext (algorithms/glwe_sample_extraction.rs:89-160) at
 * MonomialDegree(nth_first + j * nth_stride) for j < nth_count, over a batch of GLWEs (k+1 polynomials of
 * polynomial_size u64): lwe_out[b * nth_count + j] (k * polynomial_size + 1 u64).  The many-LUT extraction of a
 * rotated accumulator is one call (e.g. mockups/tfhe-hpu-mockup/src/lib.rs:736-761: nth_stride = fn_stride,
 * nth_count = lut_nb).  modulus 0 = native 2^64 (wrapping opposite), else the custom modulus q.  Every degree must be
 * < polynomial_size (MI_ERR_INVALID_ARG otherwise).  Device pointers on `device`, async on `stream`. */
int mi_sample_extract_batch(uint64_t *lwe_out, const uint64_t *glwe, size_t polynomial_size, int k, size_t batch,
                            size_t nth_first, size_t nth_stride, size_t nth_count, uint64_t modulus, int device,
                            void *stream);

/* ---- Scratch pool (no reference counterpart: the reference's PodStack / ComputationBuffers) -----------------------
 * Batched entry points that need temporary device memory take it from a per-device pool of blocks kept for reuse,
 * ordered by events (a block is reissued only behind the last kernel that used it, on any stream; a call that reuses a
 * pooled block never blocks the host).  A call whose request no idle block fits grows the pool and does block: it
 * allocates a new block and first frees the idle blocks too small for it, each after its last user has retired.  _trim
 * frees the idle blocks of `device` (-1: every device) once their last users retired; _bytes reports what the pool
 * holds. */
int mi_scratch_trim(int device, size_t *released);
int mi_scratch_bytes(int device, size_t *bytes);

/* ---- Multi-GPU helpers (single process, several devices) ----------------------------------------
 * The analogue of the CUDA backend's helper_multi_gpu (backends/tfhe-cuda-backend/cuda/src/utils/
 * helper_multi_gpu.cu:10-98, helper_multi_gpu.cuh:150-265) for a host that drives several GPUs from one
 * process (as tfhe-rs's CudaStreams do).  Bootstraps and transforms are independent, so the data path has
 * no collective: batches are split contiguously (the first total % count devices take one more; with
 * fewer units than devices the first `total` take one each), read-only state is broadcast once and LWE
 * batches are scattered from / gathered to the first device with peer-to-peer copies (xGMI links on
 * MI355X).  A device may appear more than once in a set (e.g. {0, 0} rehearses the split on one GPU).
 * All copies are asynchronous: ordered after `stream` (on devices[0]) and, for gather / PBS, `stream`
 * is ordered after them. */
typedef struct mi_multi_gpu mi_multi_gpu;
/* cuda_setup_multi_gpu (helper_multi_gpu.cu:11-40): enables peer access between devices[0] and every other
 * device of the set, and creates one non-blocking stream per entry. */
int mi_multi_gpu_create(const int *devices, int count, mi_multi_gpu **out);
int mi_multi_gpu_destroy(mi_multi_gpu *m);
int mi_multi_gpu_count(const mi_multi_gpu *m, int *count);
/* device and stream (hipStream_t as void*) of entry `index` (either pointer may be NULL) */
int mi_multi_gpu_info(const mi_multi_gpu *m, int index, int *device, void **stream);
int mi_multi_gpu_synchronize(const mi_multi_gpu *m);
/* get_active_gpu_count (helper_multi_gpu.cu:42-49): min(ceil(num_inputs / 12), gpu_count), at least 1 */
int mi_multi_gpu_active_count(uint32_t num_inputs, uint32_t gpu_count, uint32_t *out);
/* get_gpu_offset / get_num_inputs_on_gpu (helper_multi_gpu.cu:51-98): entry `index`'s [offset, offset + n) */
int mi_multi_gpu_shard(size_t total, int index, int count, size_t *offset, size_t *n);
/* dsts[i] (on devices[i]) <- `bytes` at src (devices[0]); an entry equal to src is skipped */
int mi_multi_gpu_broadcast(mi_multi_gpu *m, const void *src, void *const *dsts, size_t bytes, void *stream);
/* multi_gpu_scatter_lwe_async, trivial index: dsts[i] <- shard i of `total` units of unit_bytes at src */
int mi_multi_gpu_scatter(mi_multi_gpu *m, const void *src, void *const *dsts, size_t total, size_t unit_bytes,
                         void *stream);
/* multi_gpu_gather_lwe_async, trivial index: shard i of dst (devices[0]) <- srcs[i] */
int mi_multi_gpu_gather(mi_multi_gpu *m, void *dst, const void *const *srcs, size_t total, size_t unit_bytes,
                        void *stream);
/* Batched PBS over the device set: scatter lwe_in (devices[0]), mi_pbs_ntt64_batch on every active device
 * with keys[i] / luts[i] (bound to devices[i], same shape), gather into lwe_out (devices[0]).  Only the first
 * get_active_gpu_count(batch, count) entries are active (helper_multi_gpu.cu:42-49, min(ceil(batch / 12),
 * count), as the reference's CudaStreams::active_gpu_subset, helper_multi_gpu.h:74-79); the keys / LUTs of
 * inactive entries are not read and may be NULL.  Shard 0 runs in place on `stream`; the others use
 * stream-ordered scratch on their device.
 * _ordered: producer_streams[i] is the stream of devices[i] that produced keys[i] / luts[i] (NULL array or
 * entry: that device's legacy null stream).  Shard i starts after the work queued on it and it is ordered
 * after shard i's last read, so the caller may release / reuse the LUT on that stream right away.
 * mi_pbs_ntt64_multi_gpu is _ordered with producer_streams = NULL. */
int mi_pbs_ntt64_multi_gpu(mi_multi_gpu *m, const mi_pbs_ntt64_key *const *keys, uint64_t *lwe_out,
                           const uint64_t *lwe_in, const uint64_t *const *luts, size_t batch, int ms_mode,
                           void *stream);
int mi_pbs_ntt64_multi_gpu_ordered(mi_multi_gpu *m, const mi_pbs_ntt64_key *const *keys, uint64_t *lwe_out,
                                   const uint64_t *lwe_in, const uint64_t *const *luts, size_t batch, int ms_mode,
                                   void *stream, void *const *producer_streams);

/* ---- f64-FFT PBS (the default shortint PBS path) ----------------------------
 * Reference paths relative to /root/reference/tfhe/src/core_crypto.  The negacyclic f64 FFT of
 * fft_impl/fft64/math/fft/mod.rs (Twisties :58-76, forward_as_torus / forward_as_integer / backward_as_torus
 * :406-511): N real u64 coefficients -> N/2 complex values x[n] + i x[n + N/2], twisted by exp(i pi n / N),
 * transformed with an N/2-point DFT (exp(-2 pi i / (N/2)) kernel).  Fourier buffers hold interleaved
 * (re, im) doubles, N/2 complex per polynomial, in this engine's order: position p holds frequency
 * freq[p] (mi_fft64_fourier_order).  The reference's tfhe-fft "unordered" in-memory order is implementation
 * defined, but its serialised order is the natural one: mi_fft64_to/from_standard_order convert to and from
 * it.  Results are f64 computations: parity with the reference is decryption-exact and within the FFT error bound,
 * not bit-exact.  This build: 32 <= N <= 2^18; N = 2048 runs the one-wave engine (GLWE dimension k in {1, 2}), every
 * other N the shape-generic engine (1 <= k <= 16; multi-kernel, accumulators in HBM); any decomposition with
 * base_log * level < 64. */
typedef struct mi_fft64_plan mi_fft64_plan;
/* Fft::new (fft_impl/fft64/math/fft/mod.rs:170-223): MI_ERR_INVALID_ARG if n is not a power of two,
 * MI_ERR_UNSUPPORTED for sizes this build does not compile.  _cached: one plan per (n, device), kept until
 * process exit as the reference's PLANS map (destroy is a no-op on it). */
int mi_fft64_plan_create(size_t n, int device, mi_fft64_plan **out_plan);
int mi_fft64_plan_cached(size_t n, int device, const mi_fft64_plan **out_plan);
int mi_fft64_plan_destroy(mi_fft64_plan *plan);
int mi_fft64_plan_info(const mi_fft64_plan *plan, size_t *n, int *device);
/* freq[p] for p < n/2: the DFT frequency stored at Fourier position p (host call) */
int mi_fft64_fourier_order(const mi_fft64_plan *plan, uint32_t *freq);
/* The reference's serialised Fourier order (FourierPolynomialList's serde, fft_impl/fft64/math/fft/mod.rs:642-690,
 * through tfhe-fft's Plan::serialize_fourier_buffer / deserialize_fourier_buffer, tfhe-fft/src/unordered.rs:943-1020):
 * element i of a serialised polynomial is DFT frequency i, whatever the plan's internal order.  These convert
 * `polys` polynomials of n/2 complex between that natural order and this engine's (device pointers, async; in place
 * when the two pointers are equal), so a FourierLweBootstrapKey / FourierGgswCiphertext deserialised by the
 * reference's own serde loads with one call, and a key converted here serialises as the reference expects. */
int mi_fft64_to_standard_order(const mi_fft64_plan *plan, double *standard_order, const double *fourier, size_t polys,
                               void *stream);
int mi_fft64_from_standard_order(const mi_fft64_plan *plan, double *fourier, const double *standard_order,
                                 size_t polys, void *stream);
/* FftView::forward_as_torus / backward_as_torus (add != 0: add_backward_as_torus), per polynomial over a
 * batch of contiguous polynomials (device pointers, async): fourier = batch x n/2 x 2 doubles. */
int mi_fft64_forward_torus_batch(const mi_fft64_plan *plan, double *fourier, const uint64_t *standard, size_t batch,
                                 void *stream);
int mi_fft64_backward_torus_batch(const mi_fft64_plan *plan, uint64_t *standard, const double *fourier, size_t batch,
                                  int add, void *stream);
/* convert_standard_lwe_bootstrap_key_to_fourier (algorithms/lwe_bootstrap_key_conversion.rs:20-43): every
 * polynomial of the standard key (n_polys = n_lwe (k+1)^2 level) through forward_as_torus. */
int mi_bsk_to_fourier64(const mi_fft64_plan *plan, const uint64_t *bsk_std, double *bsk_fourier, size_t n_polys,
                        void *stream);
/* add_external_product_assign / cmux_assign (algorithms/lwe_programmable_bootstrapping/fft64_pbs.rs:270-330,
 * 510-560; fft_impl/fft64/crypto/ggsw.rs:483-603): native 2^64 GLWEs, one shared Fourier GGSW (level x (k+1)
 * x (k+1) x n/2 complex, highest level first).  CMUX leaves ct1 holding ct1 - ct0, as the reference. */
int mi_fft64_ext_product_batch(const mi_fft64_plan *plan, uint64_t *out_glwe, const uint64_t *in_glwe,
                               const double *ggsw_fourier, int k, int base_log, int level, size_t batch, void *stream);
int mi_fft64_cmux_batch(const mi_fft64_plan *plan, uint64_t *ct0, uint64_t *ct1, const double *ggsw_fourier, int k,
                        int base_log, int level, size_t batch, void *stream);
/* A Fourier bootstrap key (FourierLweBootstrapKey, referenced: the caller keeps `fbsk` alive) and the batched
 * programmable_bootstrap_lwe_ciphertext (fft64_pbs.rs:924-1060; blind rotation fft_impl/fft64/crypto/
 * bootstrap.rs:294-381, 481-521).  ms_mode as mi_pbs_ntt64_batch. */
typedef struct mi_fft64_pbs_key mi_fft64_pbs_key;
int mi_fft64_pbs_key_create(const mi_fft64_plan *plan, const double *fbsk, size_t n_lwe, int k, int base_log,
                            int level, mi_fft64_pbs_key **out_key);
int mi_fft64_pbs_key_destroy(mi_fft64_pbs_key *key);
int mi_fft64_pbs_key_info(const mi_fft64_pbs_key *key, size_t *n_lwe, int *k, int *base_log, int *level);
int mi_fft64_pbs_batch(const mi_fft64_pbs_key *key, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *lut,
                       size_t batch, int ms_mode, void *stream);
/* One accumulator per item: lut_index NULL = batch_programmable_bootstrap_lwe_ciphertext_mem_optimized
 * (fft64_pbs.rs:1055-1127: item b bootstraps through GLWE b of lut_list, n_lut >= batch); otherwise item b uses GLWE
 * lut_index[b] (device u32) and an index >= n_lut leaves lwe_out[b] untouched. */
int mi_fft64_pbs_batch_lut_indexed(const mi_fft64_pbs_key *key, uint64_t *lwe_out, const uint64_t *lwe_in,
                                   const uint64_t *lut_list, const uint32_t *lut_index, size_t n_lut, size_t batch,
                                   int ms_mode, void *stream);
/* blind_rotate_assign[_mem_optimized] (fft64_pbs.rs:186-250; FourierLweBootstrapKey::blind_rotate_assign,
 * fft_impl/fft64/crypto/bootstrap.rs:294-381), batched and in place: acc_glwe[b] ((k+1) N u64) is divided by
 * X^ms(body) and rotated through the CMUX loop over lwe_in[b].  ms_mode as mi_pbs_ntt64_batch (the reference's
 * ModulusSwitchedLweCiphertext input: MI_MS_PRE_SWITCHED, or the native LWE switched on the device). */
int mi_fft64_blind_rotate_batch(const mi_fft64_pbs_key *key, uint64_t *acc_glwe, const uint64_t *lwe_in, size_t batch,
                                int ms_mode, void *stream);
/* The multi-bit programmable bootstrap on the f64-FFT path (algorithms/lwe_multi_bit_programmable_bootstrapping.rs:
 * multi_bit_deterministic_blind_rotate_assign :644-869, prepare_multi_bit_ggsw_mem_optimized :115-154,
 * modulus_switch_multi_bit :30-51, selection_bit :55-65; key layout lwe_multi_bit_bootstrap_key_generation.rs:398-421).
 * The key is referenced (the caller keeps `fbsk` alive): (n_lwe / g) x 2^g x level x (k+1) x (k+1) x N/2 complex,
 * group-major, each GGSW in this engine's order with the highest level first as for mi_fft64_pbs_key_create
 * (mi_bsk_to_fourier64 converts the standard key, whatever its polynomial count); GGSW idx of group i encrypts
 * prod_m (s[i g + m] XOR NOT bit_m(idx)), bit_m(idx) = (idx >> (g - 1 - m)) & 1.  One blind-rotation step handles g mask
 * elements: n_lwe / g external products.  _create: MI_ERR_INVALID_ARG for a NULL argument, a grouping factor outside
 * {2, 3, 4}, n_lwe not a multiple of it, base_log * level outside [1, 63]; MI_ERR_UNSUPPORTED for N != 2048 or k
 * outside {1, 2}.  The input is always the native LWE, switched on the device with the standard switch of the wrapping
 * sum of each subset of a group's mask elements (there is no ms_mode); the rotation order is fixed, so this is the
 * reference's deterministic variant. */
typedef struct mi_fft64_multi_bit_pbs_key mi_fft64_multi_bit_pbs_key;
int mi_fft64_multi_bit_pbs_key_create(const mi_fft64_plan *plan, const double *fbsk, size_t n_lwe, int k, int base_log,
                                      int level, int grouping_factor, mi_fft64_multi_bit_pbs_key **out_key);
int mi_fft64_multi_bit_pbs_key_destroy(mi_fft64_multi_bit_pbs_key *key);
int mi_fft64_multi_bit_pbs_key_info(const mi_fft64_multi_bit_pbs_key *key, size_t *n_lwe, int *k, int *base_log,
                                    int *level, int *grouping_factor);
/* multi_bit_programmable_bootstrap_lwe_ciphertext (lwe_multi_bit_programmable_bootstrapping.rs:1029-1126): one shared
 * accumulator `lut` ((k+1) N u64), sample 0 of the rotated accumulator into lwe_out[b] (k N + 1 u64). */
int mi_fft64_multi_bit_pbs_batch(const mi_fft64_multi_bit_pbs_key *key, uint64_t *lwe_out, const uint64_t *lwe_in,
                                 const uint64_t *lut, size_t batch, void *stream);
/* As mi_fft64_pbs_batch_lut_indexed: lut_index NULL = one accumulator per item (n_lut >= batch); otherwise item b uses
 * GLWE lut_index[b] (device u32) and an index >= n_lut leaves lwe_out[b] untouched. */
int mi_fft64_multi_bit_pbs_batch_lut_indexed(const mi_fft64_multi_bit_pbs_key *key, uint64_t *lwe_out,
                                             const uint64_t *lwe_in, const uint64_t *lut_list,
                                             const uint32_t *lut_index, size_t n_lut, size_t batch, void *stream);
/* multi_bit_blind_rotate_assign (:644-869), batched and in place, GLWE in and GLWE out as mi_fft64_blind_rotate_batch:
 * acc_glwe[b] is divided by X^ms(body) and taken through the n_lwe / g steps acc <- bundle (.) acc. */
int mi_fft64_multi_bit_blind_rotate_batch(const mi_fft64_multi_bit_pbs_key *key, uint64_t *acc_glwe,
                                          const uint64_t *lwe_in, size_t batch, void *stream);
/* The multi-GPU bootstrap of mi_pbs_ntt64_multi_gpu[_ordered] (same sharding, active-GPU count, scatter / gather and
 * producer-stream ordering) on the f64-FFT path: keys[i] (bound to a plan of devices[i], same shape) and luts[i] on
 * devices[i], lwe_in / lwe_out on devices[0]. */
int mi_fft64_pbs_multi_gpu(mi_multi_gpu *m, const mi_fft64_pbs_key *const *keys, uint64_t *lwe_out,
                           const uint64_t *lwe_in, const uint64_t *const *luts, size_t batch, int ms_mode,
                           void *stream);
int mi_fft64_pbs_multi_gpu_ordered(mi_multi_gpu *m, const mi_fft64_pbs_key *const *keys, uint64_t *lwe_out,
                                   const uint64_t *lwe_in, const uint64_t *const *luts, size_t batch, int ms_mode,
                                   void *stream, void *const *producer_streams);
/* The reference's serialised FourierLweBootstrapKey (fft_impl/fft64/crypto/bootstrap.rs:30-39, the list's custom
 * Serialize fft_impl/fft64/math/fft/mod.rs:642-690, bincode 1.3 defaults as for the NTT key): format
 * MI_NTT_BSK_PLAIN = bincode::serialize(&key): u64 (2 + P), u64 polynomial_size, u64 P, then P polynomials each as
 * u64 (N/2) and N/2 (re, im) f64 pairs in the natural DFT order (tfhe-fft/src/unordered.rs:943-964), then
 * input_lwe_dimension, glwe_size, decomposition_base_log, decomposition_level_count as u64;
 * MI_NTT_BSK_VERSIONED = bincode of key.versionize(): u32 1 (FourierLweBootstrapKeyVersions::V1), u32 0
 * (FourierPolynomialListVersioned::V0), the same list, a u32 0 before each scalar field
 * (backward_compatibility/fft_impl/mod.rs:14-70).  _load validates the bytes (length, tags, per-polynomial length,
 * P = n_lwe level glwe_size^2, the plan's polynomial size), uploads them with one strided copy and reorders them
 * into this engine's order on `stream` (synchronised before returning); the key owns that device copy.  _write
 * produces exactly mi_fft64_bsk_serialized_size bytes from any key (a loaded one or one over a caller tensor). */
int mi_fft64_bsk_serialized_size(size_t polynomial_size, size_t n_lwe, int k, int level, int format,
                                 size_t *out_len);
int mi_fft64_pbs_key_load(const mi_fft64_plan *plan, const uint8_t *bytes, size_t len, int format, void *stream,
                          mi_fft64_pbs_key **out_key);
int mi_fft64_pbs_key_write(const mi_fft64_pbs_key *key, int format, uint8_t *out, size_t out_len, void *stream);

/* ---- prime32::Plan (tfhe-ntt/src/prime32.rs:632-1025) ----------------------------------------
 * The same negacyclic transform and pointwise ops on u32 buffers for a prime p < 2^32.  try_new
 * (prime32.rs:662-671) returns None for N < 32, N not a power of two, p not prime, no 2N-th root:
 * here MI_ERR_INVALID_ARG / MI_ERR_NOT_PRIME / MI_ERR_NO_ROOT.  Twiddles follow
 * init_negacyclic_twiddles (prime32.rs:223-246), outputs are canonical (< p) as the reference's
 * tests assert (prime32.rs:1114-1133). */
typedef struct mi_ntt32_plan mi_ntt32_plan;
int mi_ntt32_plan_create(size_t n, uint32_t p, int device, mi_ntt32_plan **out_plan);
int mi_ntt32_plan_destroy(mi_ntt32_plan *plan);
int mi_ntt32_plan_info(const mi_ntt32_plan *plan, size_t *n, uint32_t *p, int *device);
/* Plan::fwd / Plan::inv (prime32.rs:797-898) */
int mi_ntt32_fwd_batch(const mi_ntt32_plan *plan, uint32_t *buf, size_t batch, size_t stride, void *stream);
int mi_ntt32_inv_batch(const mi_ntt32_plan *plan, uint32_t *buf, size_t batch, size_t stride, void *stream);
/* Plan::normalize / mul_assign_normalize / mul_accumulate (prime32.rs:900-1025) */
int mi_ntt32_normalize_batch(const mi_ntt32_plan *plan, uint32_t *buf, size_t batch, size_t stride, void *stream);
int mi_ntt32_mul_assign_normalize_batch(const mi_ntt32_plan *plan, uint32_t *lhs, const uint32_t *rhs,
                                        size_t batch, size_t stride, void *stream);
int mi_ntt32_mul_accumulate_batch(const mi_ntt32_plan *plan, uint32_t *acc, const uint32_t *lhs,
                                  const uint32_t *rhs, size_t batch, size_t stride, void *stream);

/* ---- Exact native-modulus negacyclic products over a CRT of NTT primes ----------------------
 * negacyclic_polymul of native32.rs:410-500, native64.rs:1041-1160, native128.rs:297-320 and the
 * binary-RHS plans native_binary{32,64,128}.rs (rhs coefficients in {0,1}): prod = lhs * rhs in
 * Z_{2^W}[X]/(X^N + 1), W = 32 / 64 / 128 (u128 = two little-endian u64 words).  The prime sets are
 * the reference's (lib.rs primes32 / primes52).  Plan52 kinds exist in the reference only on CPUs
 * with AVX-512 IFMA (their try_new returns None otherwise); here they always exist. */
typedef enum mi_native_kind {
    MI_NATIVE32_PLAN32 = 0,        /* native32::Plan32           P0..P2 (32-bit)  */
    MI_NATIVE32_PLAN52 = 1,        /* native32::Plan52           P0..P1 (52-bit)  */
    MI_NATIVE64_PLAN32 = 2,        /* native64::Plan32           P0..P4 (32-bit)  */
    MI_NATIVE64_PLAN52 = 3,        /* native64::Plan52           P0..P2 (52-bit)  */
    MI_NATIVE128_PLAN32 = 4,       /* native128::Plan32          P0..P9 (32-bit)  */
    MI_NATIVE_BINARY32_PLAN32 = 5, /* native_binary32::Plan32    P0..P1 (32-bit)  */
    MI_NATIVE_BINARY32_PLAN52 = 6, /* native_binary32::Plan52    P0     (52-bit)  */
    MI_NATIVE_BINARY64_PLAN32 = 7, /* native_binary64::Plan32    P0..P2 (32-bit)  */
    MI_NATIVE_BINARY64_PLAN52 = 8, /* native_binary64::Plan52    P0..P1 (52-bit)  */
    MI_NATIVE_BINARY128_PLAN32 = 9 /* native_binary128::Plan32   P0..P4 (32-bit)  */
} mi_native_kind;
typedef struct mi_native_plan mi_native_plan;
/* Plan32/Plan52::try_new(n) (e.g. native64.rs:932-941): None when a component prime plan is. */
int mi_native_plan_create(int kind, size_t n, int device, mi_native_plan **out_plan);
int mi_native_plan_destroy(mi_native_plan *plan);
int mi_native_plan_info(const mi_native_plan *plan, size_t *n, int *width_bits, int *num_primes);
/* Batched negacyclic_polymul: `batch` contiguous polynomials of n words each in prod/lhs/rhs
 * (device pointers, async on `stream`; scratch is stream-ordered and freed before return). */
int mi_native_polymul_batch(const mi_native_plan *plan, void *prod, const void *lhs, const void *rhs, size_t batch,
                            void *stream);

/* ---- LWE keyswitch (tfhe/src/core_crypto/algorithms/lwe_keyswitch.rs) ---------------------------
 * The keyswitch in front of the PBS in the shortint KS-PBS order (PARAM_MESSAGE_2_CARRY_2:
 * 2048 -> 918, base 2^4, 4 levels; shortint/parameters/v1_4/classic/tuniform/p_fail_2_minus_128/ks_pbs.rs:29-47).
 * mi_lwe_ksk_create takes the reference's LweKeyswitchKey layout as a device pointer: in_dim blocks of
 * `level` LWE ciphertexts of out_dim + 1 u64, levels stored as generate_lwe_keyswitch_key writes them
 * (lwe_keyswitch_key_generation.rs:169-199), and prepares a private device copy (the caller's buffer
 * may be freed afterwards; the preparation runs on `stream`, the stream that produced `ksk`, and synchronises
 * it).  MI_ERR_INVALID_ARG where SignedDecomposer::new would assert
 * (base_log * level >= 64); MI_ERR_UNSUPPORTED when in_dim * level * ceil((base_log + 1) / 8) >= 2^17
 * (beyond the exact int32 accumulation of the int8 matrix-core path). */
typedef struct mi_lwe_ksk mi_lwe_ksk;
int mi_lwe_ksk_create(const uint64_t *ksk, size_t in_dim, size_t out_dim, int base_log, int level, int device,
                      void *stream, mi_lwe_ksk **out_key);
int mi_lwe_ksk_destroy(mi_lwe_ksk *key);
int mi_lwe_ksk_info(const mi_lwe_ksk *key, size_t *in_dim, size_t *out_dim, int *base_log, int *level);
/* keyswitch_lwe_ciphertext_native_mod_compatible (lwe_keyswitch.rs:137-227) over a batch:
 * lwe_out[b] (out_dim + 1 u64) = keyswitch(lwe_in[b] (in_dim + 1 u64)), native 2^64 modulus, bit-exact.
 * Device pointers, async on `stream` (stream-ordered scratch, freed before return). */
int mi_lwe_keyswitch_batch(const mi_lwe_ksk *key, uint64_t *lwe_out, const uint64_t *lwe_in, size_t batch,
                           void *stream);

/* ---- KS32: the keyswitch with a scalar change of the HPU KS32 parameter sets ----------------------------------
 * keyswitch_lwe_ciphertext_with_scalar_change (lwe_keyswitch.rs:331-447), as V1_5_HPU_PARAM_MESSAGE_2_CARRY_2_KS32_
 * PBS_TUNIFORM_2M128 runs it (shortint/parameters/v1_5/hpu.rs:57-76: 2048 -> 879, ks base 2^2, 8 levels,
 * post_keyswitch_ciphertext_modulus 2^21; mockups/tfhe-hpu-mockup/src/lib.rs:720-736): u64 input LWEs (native
 * modulus) -> u32 output LWEs of modulus 2^out_modulus_log, power-of-two encoded in the MSBs of the u32 words, as the
 * reference stores non-native power-of-two moduli.  The key: in_dim blocks of `level` u32 LWE ciphertexts of
 * out_dim + 1 words (the LweKeyswitchKey<Vec<u32>> layout, levels as generate_lwe_keyswitch_key writes them).
 * The body is closest_representable(b) at out_modulus_log bits, shifted down by 32; every mask digit of the u64
 * SignedDecomposer (base_log, level) times its key row is subtracted with wrapping u32 arithmetic.
 * MI_ERR_INVALID_ARG where the reference asserts (base_log * level > 32) or out_modulus_log is outside [1, 32];
 * the same 2^17 GEMM-depth bound as mi_lwe_ksk_create.  Bit-exact. */
typedef struct mi_lwe_ksk32 mi_lwe_ksk32;
int mi_lwe_ksk32_create(const uint32_t *ksk, size_t in_dim, size_t out_dim, int base_log, int level,
                        int out_modulus_log, int device, void *stream, mi_lwe_ksk32 **out_key);
int mi_lwe_ksk32_destroy(mi_lwe_ksk32 *key);
int mi_lwe_ksk32_info(const mi_lwe_ksk32 *key, size_t *in_dim, size_t *out_dim, int *base_log, int *level,
                      int *out_modulus_log);
int mi_lwe_keyswitch32_batch(const mi_lwe_ksk32 *key, uint32_t *lwe_out, const uint64_t *lwe_in, size_t batch,
                             void *stream);
/* The modulus switch of u32 LWEs (lwe_dim mask words + body) to [0, 2^log_modulus): MI_MS_STANDARD =
 * lwe_ciphertext_modulus_switch, MI_MS_CENTERED = lwe_ciphertext_centered_binary_modulus_switch
 * (algorithms/modulus_switch.rs:14-104, at Scalar = u32), materialised as the ModulusSwitchedLweCiphertext values
 * (entities/modulus_switched_lwe_ciphertext.rs:150-175): switched[b] = lwe_dim + 1 u64 in [0, 2^log_modulus), the
 * MI_MS_PRE_SWITCHED input of mi_blind_rotate_ntt64_batch / mi_pbs_ntt64_batch (log_modulus = log2(2N)). */
int mi_lwe_modulus_switch32_batch(uint64_t *switched, const uint32_t *lwe_in, size_t lwe_dim, size_t batch,
                                  int log_modulus, int ms_mode, int device, void *stream);
/* The same switch of u64 LWEs (the native 2^64 ciphertexts in front of every other blind rotation):
 * lwe_ciphertext_modulus_switch / lwe_ciphertext_centered_binary_modulus_switch (algorithms/modulus_switch.rs:14-104)
 * at Scalar = u64, materialised as the LazyStandardModulusSwitchedLweCiphertext reads them
 * (entities/modulus_switched_lwe_ciphertext.rs:150-175) — what the HPU mockup runs before blind_rotate_ntt64_bnf_assign
 * (mockups/tfhe-hpu-mockup/src/lib.rs:725-736).  Both forms: log_modulus in [1, BITS] for MI_MS_STANDARD (identity at
 * BITS, fft_impl/common.rs:10-23) and [1, BITS - 1] for MI_MS_CENTERED, whose half_case shift (modulus_switch.rs:95)
 * underflows at BITS in the reference; anything else is MI_ERR_INVALID_ARG.  BITS = 32 for the u32 call above. */
int mi_lwe_modulus_switch_batch(uint64_t *switched, const uint64_t *lwe_in, size_t lwe_dim, size_t batch,
                                int log_modulus, int ms_mode, int device, void *stream);

/* ---- Modulus switch noise reduction: the drift technique ------------------------------------------------------
 * ModulusSwitchConfiguration::DriftTechniqueNoiseReduction (shortint/server_key/modulus_switch_noise_reduction.rs:
 * 325-383), what every classic *_KS_PBS_TUNIFORM_2M128 parameter set runs between its keyswitch and its bootstrap
 * (shortint/parameters/v1_1/classic/tuniform/p_fail_2_minus_128/ks_pbs.rs:29-122; https://eprint.iacr.org/2024/1718):
 * core_crypto/algorithms/modulus_switch_noise_reduction.rs.  An input LWE whose modulus switch noise measure exceeds
 * ms_bound gets the first of the key's encryptions of zero added that brings the measure under the bound, or, when
 * none does, the first one with the smallest measure (the unmodified input wins ties).  The measure's two f64 sums
 * run over the mask in the reference's order with a separate multiply and add, so the measures, the chosen
 * candidates and the outputs are the reference's bit for bit.  Native u64 modulus only, as the reference asserts
 * (:131-136).
 * mi_ms_noise_key_create takes the ModulusSwitchNoiseReductionKey's modulus_switch_zeros in the LweCiphertextList
 * layout as a device pointer, zeros_count rows of lwe_dim + 1 u64, and prepares a private device copy on `stream`
 * (the stream that produced `zeros`), which it synchronises; the caller's buffer may be freed afterwards.  The
 * modular variance of the measure is ms_input_variance * 2^64 * 2^64 (dispersion.rs:258-262).  Checked before any
 * device call, the first failing rule answering, all MI_ERR_INVALID_ARG: "zeros is NULL"; "out_key is NULL";
 * lwe_dim outside [1, 2^24): "lwe dimension out of range"; zeros_count == 0: "expected at least one encryption of
 * zero" (the reference's assert, :126-130); zeros_count >= 2^32: "zeros_count out of range"; a NaN among the three
 * doubles: "ms_bound, ms_r_sigma_factor and ms_input_variance must not be NaN"; ms_r_sigma_factor < 0 or
 * ms_input_variance < 0: "ms_r_sigma_factor and ms_input_variance must not be negative".  +inf is a legal bound.
 * Every batch entry: device pointers, async on `stream`; a NULL key is MI_ERR_INVALID_ARG "key is NULL"; log_modulus
 * outside [1, 64] is MI_ERR_INVALID_ARG (at 64 the rounding is the identity and every error 0, fft_impl/common.rs:
 * 10-23); batch = 0 is MI_OK. */
typedef struct mi_ms_noise_key mi_ms_noise_key;
int mi_ms_noise_key_create(const uint64_t *zeros, size_t lwe_dim, size_t zeros_count, double ms_bound,
                           double ms_r_sigma_factor, double ms_input_variance, int device, void *stream,
                           mi_ms_noise_key **out_key);
int mi_ms_noise_key_destroy(mi_ms_noise_key *key);
int mi_ms_noise_key_info(const mi_ms_noise_key *key, size_t *lwe_dim, size_t *zeros_count, double *ms_bound,
                         double *ms_r_sigma_factor, double *ms_input_variance);
/* measure_modulus_switch_noise_estimation_for_binary_key (:71-86): measures[b * stride] for lwe_in[b]; with
 * all_candidates != 0 stride = 1 + zeros_count and measures[b * stride + 1 + c] is the measure of lwe_in[b] + zero[c];
 * else stride = 1. */
int mi_lwe_ms_noise_measure_batch(const mi_ms_noise_key *key, double *measures, const uint64_t *lwe_in, size_t batch,
                                  int log_modulus, int all_candidates, void *stream);
/* choose_candidate_to_improve_modulus_switch_noise_for_binary_key (:99-195): candidate[b] = -1 (NoAddition) or the
 * index; satisfied[b] = 1 (SatisfyingBound) or 0 (BestNotSatisfyingBound). */
int mi_lwe_ms_noise_choose_batch(const mi_ms_noise_key *key, int64_t *candidate, int32_t *satisfied,
                                 const uint64_t *lwe_in, size_t batch, int log_modulus, void *stream);
/* improve_lwe_ciphertext_modulus_switch_noise_for_binary_key (:202-242); lwe_out may be lwe_in (the reference's
 * in-place form); candidate / satisfied may be NULL. */
int mi_lwe_ms_noise_improve_batch(const mi_ms_noise_key *key, uint64_t *lwe_out, const uint64_t *lwe_in, size_t batch,
                                  int log_modulus, int64_t *candidate, int32_t *satisfied, void *stream);
/* ModulusSwitchNoiseReductionKey::improve_noise_and_modulus_switch (shortint/server_key/
 * modulus_switch_noise_reduction.rs:102-118), materialised: the improved LWE through the standard switch of
 * mi_lwe_modulus_switch_batch, values in [0, 2^log_modulus), the MI_MS_PRE_SWITCHED input of every blind rotation /
 * PBS entry. */
int mi_lwe_ms_noise_improve_and_switch_batch(const mi_ms_noise_key *key, uint64_t *switched, const uint64_t *lwe_in,
                                             size_t batch, int log_modulus, void *stream);

/* ---- LWE packing keyswitch and GLWE compression ---------------------------------------------------------------
 * What shortint's CompressedCiphertextList is built on (COMP_PARAM_MESSAGE_2_CARRY_2: 2048 -> k = 4, N = 256,
 * base 2^4, 3 levels, 256 LWEs per GLWE, storage log modulus 12; shortint/parameters/v1_4/list_compression/).
 * mi_lwe_pksk_create takes the reference's LwePackingKeyswitchKey layout as a device pointer: in_dim blocks of `level`
 * GLWE ciphertexts of (glwe_dim + 1) * polynomial_size u64, levels stored as generate_lwe_packing_keyswitch_key
 * writes them (lwe_packing_keyswitch_key_generation.rs:129-156), and prepares a private device copy (the caller's
 * buffer may be freed afterwards; the preparation runs on `stream` and synchronises it).  polynomial_size a power of
 * two, (glwe_dim + 1) * polynomial_size < 2^24; MI_ERR_INVALID_ARG where SignedDecomposer::new asserts
 * (base_log * level outside [1, 63]); MI_ERR_UNSUPPORTED beyond the 2^17 GEMM-depth bound of mi_lwe_ksk_create. */
typedef struct mi_lwe_pksk mi_lwe_pksk;
int mi_lwe_pksk_create(const uint64_t *pksk, size_t in_dim, int glwe_dim, size_t polynomial_size, int base_log,
                       int level, int device, void *stream, mi_lwe_pksk **out_key);
int mi_lwe_pksk_destroy(mi_lwe_pksk *key);
int mi_lwe_pksk_info(const mi_lwe_pksk *key, size_t *in_dim, int *glwe_dim, size_t *polynomial_size, int *base_log,
                     int *level);
/* keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext (lwe_packing_keyswitch.rs:296-379) over a list of lists:
 * n_lwe ciphertexts (in_dim + 1 u64 each), lwe_per_glwe <= polynomial_size per output GLWE;
 * ceil(n_lwe / lwe_per_glwe) GLWEs of (glwe_dim + 1) * polynomial_size u64 are written, the last one holding the
 * remainder (shortint's chunks(lwe_per_glwe)).  GLWE g = sum_d X^d * keyswitch_lwe_ciphertext_into_glwe_ciphertext(
 * lwe_in[g * lwe_per_glwe + d]) (:102-187: the mask is rounded with closest_representable before it is decomposed),
 * so lwe_per_glwe = 1 is that function over a batch.  Native 2^64 modulus, bit-exact.  Device pointers, async on
 * `stream`; stream-ordered scratch of at most 64 MiB of keyswitched rows (or one row, if larger) plus their digits,
 * freed before return: larger calls run in chunks.  n_lwe = 0 is MI_OK. */
int mi_lwe_packing_keyswitch_batch(const mi_lwe_pksk *key, uint64_t *glwe_out, const uint64_t *lwe_in, size_t n_lwe,
                                   size_t lwe_per_glwe, void *stream);
/* The u64 words of one CompressedModulusSwitchedGlweCiphertext's PackedIntegers:
 * ceil((glwe_dim * polynomial_size + bodies_count) * log_modulus / 64)
 * (compressed_modulus_switched_glwe_ciphertext.rs:229-232).  bodies_count <= polynomial_size and
 * 1 <= log_modulus <= 64, as compress asserts (:191-203); else MI_ERR_INVALID_ARG, here and below. */
int mi_glwe_compressed_words(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus,
                             size_t *words);
/* CompressedModulusSwitchedGlweCiphertext::compress (:169-220) over a batch of native-modulus GLWEs: the first
 * glwe_dim * polynomial_size + bodies_count words of glwe[b], each through modulus_switch (fft_impl/common.rs:10-23),
 * packed log_modulus bits each, little end first, as PackedIntegers::pack does (entities/packed_integers.rs:39-130),
 * into packed[b] (mi_glwe_compressed_words u64).  Device pointers, async on `stream`. */
int mi_glwe_compress_batch(uint64_t *packed, const uint64_t *glwe, size_t polynomial_size, int glwe_dim,
                           size_t bodies_count, int log_modulus, size_t batch, int device, void *stream);
/* CompressedModulusSwitchedGlweCiphertext::extract (:226-256): glwe[b] ((glwe_dim + 1) * polynomial_size u64) = the
 * unpacked values (PackedIntegers::unpack, packed_integers.rs:132-222) shifted left by 64 - log_modulus, then
 * polynomial_size - bodies_count zeros. */
int mi_glwe_extract_batch(uint64_t *glwe, const uint64_t *packed, size_t polynomial_size, int glwe_dim,
                          size_t bodies_count, int log_modulus, size_t batch, int device, void *stream);

/* ---- The exact 128-bit programmable bootstrap (shortint noise squashing) -----------------------------------------
 * programmable_bootstrap_f128_lwe_ciphertext (algorithms/lwe_programmable_bootstrapping/fft128_pbs.rs:174;
 * fft_impl/fft128_u128/crypto/{bootstrap,ggsw}.rs) over Z_{2^128}[X]/(X^N + 1), as V1_4_NOISE_SQUASHING_PARAM_MESSAGE_2_
 * CARRY_2_KS_PBS_TUNIFORM_2M128 runs it before threshold decryption (k = 2, N = 2048, base 2^24, 3 levels, native u128,
 * centered modulus switch; shortint/parameters/v1_4/noise_squashing/p_fail_2_minus_128/mod.rs:8-19): the u64 LWE the
 * keyswitch produces (dimension 918) is bootstrapped into a u128 LWE.  The reference multiplies with a double-double FFT;
 * here the products run on the Goldilocks NTT and are exact: every u128 key coefficient is split into limbs of
 * limb_bits bits, narrow enough that a whole column sum of digit x limb products stays below p / 2 and is read back as
 * the integer it is.  The results are the reference's algorithm with its transform error removed: bit for bit the
 * integer arithmetic mod 2^128 (SignedDecomposer<u128>, decomposer.rs:156-185 / collect_next_term_split_scalar,
 * ggsw.rs:517-567; the exact negacyclic product).  Every u128 crosses this ABI as two little-endian u64 words (lo, hi),
 * as mi_native_polymul_batch takes them; u128 buffers are 16-byte aligned device pointers.
 * Not provided: non-native power-of-two moduli below 2^128 (the closest_representable step of blind_rotate_u128,
 * bootstrap.rs:217-231), u32 / u128 input LWEs, a LUT index per item, the C++ mirror,
 * and the serialised Fourier128LweBootstrapKey format (it holds the output of the reference's own FFT and has no
 * meaning here).  The multi-bit variant follows the classic entries; the packing keyswitch and the compression of
 * its results are the next section.
 *
 * mi_pbs128_limb_plan (no reference counterpart, needs no device): limb_bits = the largest w with
 * R N 2^(base_log - 1) (2^w - 1) <= (p - 1) / 2, R = (k + 1) level, p = 2^64 - 2^32 + 1; n_limbs = ceil(128 / w)
 * (w = 25, 6 limbs at the shape above).  MI_ERR_INVALID_ARG where SignedDecomposer::<u128>::new asserts (decomposer.rs:
 * 86-90: base_log * level outside [1, 127]), for N not a power of two or above 2^31 and for k < 1 or above 65535, each
 * with its own message;
 * MI_ERR_UNSUPPORTED when n_limbs > 16 (the outputs are still written; both 0 when no width fits).  Either output may
 * be NULL. */
int mi_pbs128_limb_plan(size_t polynomial_size, int k, int base_log, int level, int *limb_bits, int *n_limbs);
/* The bootstrap key.  bsk_std: the reference's LweBootstrapKey<u128> layout as a device pointer (n_ggsw GGSWs of
 * `level` level matrices of (k + 1) GLWE rows of (k + 1) polynomials of polynomial_size u128, the level matrices in
 * the order ggsw.into_levels() yields them, ggsw.rs:112-116, as the u64 keys).  A private prepared copy is made on
 * `stream`, which is synchronised (the caller's buffer may be freed afterwards): limb polynomials through the plan's
 * forward transform, N^-1 folded in, n_limbs x 8 bytes per coefficient, converted GGSW by GGSW straight into place (no
 * second key-sized buffer).  `plan` must be the Goldilocks plan of polynomial_size (else MI_ERR_UNSUPPORTED), k <= 3;
 * the argument rules and the limb bound of mi_pbs128_limb_plan apply.  The key borrows `plan` (its device and
 * twiddle tables are read by every later call, mi_pbs128_key_destroy included): the plan must outlive the key; a plan
 * from mi_ntt64_plan_cached always does. */
typedef struct mi_pbs128_key mi_pbs128_key;
int mi_pbs128_key_create(const mi_ntt64_plan *plan, const uint64_t *bsk_std, size_t n_ggsw, int k,
                         size_t polynomial_size, int base_log, int level, void *stream, mi_pbs128_key **out_key);
int mi_pbs128_key_destroy(mi_pbs128_key *key);
int mi_pbs128_key_info(const mi_pbs128_key *key, size_t *n_ggsw, int *k, size_t *polynomial_size, int *base_log,
                       int *level, int *limb_bits, int *n_limbs);
/* add_external_product_assign_split (ggsw.rs:17): out_glwe[b] += GGSW (.) in_glwe[b] for `batch` GLWEs of
 * (k + 1) polynomial_size u128, GGSW number ggsw_index of the key shared by the batch (an index >= n_ggsw is
 * MI_ERR_INVALID_ARG and nothing is written).  cmux_split (ggsw.rs:621-675): ct1 -= ct0, then ct0 += GGSW (.) ct1;
 * ct1 is left holding the difference, as the reference leaves it.  The two operands of a call are disjoint buffers
 * (overlapping ones are MI_ERR_INVALID_ARG: the sum is written after the input was read by an earlier pass); so are
 * the buffers of the two entries below.  Async on `stream`, stream-ordered scratch (at most
 * ~4 GiB per chunk of the batch; the environment variable MI_PBS128_CHUNK, read per call, lowers the chunk's item
 * count).  batch = 0 is MI_OK. */
int mi_ext_product128_batch(const mi_pbs128_key *key, size_t ggsw_index, uint64_t *out_glwe, const uint64_t *in_glwe,
                            size_t batch, void *stream);
int mi_cmux128_batch(const mi_pbs128_key *key, size_t ggsw_index, uint64_t *ct0, uint64_t *ct1, size_t batch,
                     void *stream);
/* blind_rotate_assign_split (bootstrap.rs:60-150), batched and in place: acc_glwe[b] ((k + 1) polynomial_size u128) is
 * divided by X^ms(body) and rotated through the CMUX loop over lwe_in[b] (n_ggsw + 1 u64 at the native 2^64 modulus;
 * ms_mode as mi_pbs_ntt64_batch, log modulus log2(2N): switched on the device, or MI_MS_PRE_SWITCHED values in
 * [0, 2N)).  A mask element that switches to 0 contributes exactly nothing, as the reference's skip. */
int mi_blind_rotate128_batch(const mi_pbs128_key *key, uint64_t *acc_glwe, const uint64_t *lwe_in, size_t batch,
                             int ms_mode, void *stream);
/* programmable_bootstrap_f128_lwe_ciphertext / blind_rotate_u128 (bootstrap.rs:152-247) over a batch: the blind
 * rotation of the one shared LUT GLWE `lut`, then extract_lwe_sample_from_glwe_ciphertext at degree 0:
 * lwe_out[b] = k polynomial_size + 1 u128. */
int mi_pbs128_batch(const mi_pbs128_key *key, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *lut,
                    size_t batch, int ms_mode, void *stream);
/* The multi-bit 128-bit bootstrap (algorithms/lwe_multi_bit_programmable_bootstrapping.rs:
 * multi_bit_programmable_bootstrap_f128_lwe_ciphertext, multi_bit_f128_deterministic_blind_rotate_assign,
 * prepare_multi_bit_fourier_128_ggsw_mem_optimized :2257-2700; the std_* forms :1849-2255 build the bundle in the
 * standard domain), what V1_3_NOISE_SQUASHING_PARAM_GPU_MULTI_BIT_GROUP_4_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128 runs
 * (k = 2, N = 2048, base 2^23, 3 levels, grouping factor 4, native u128;
 * shortint/parameters/v1_3/noise_squashing/p_fail_2_minus_128/mod.rs:65-77).  Exact as the classic entries above: bit
 * for bit the integer arithmetic mod 2^128 of
 *   acc /= X^ms(body);  per group: bundle = G_0 + sum_idx X^(d_idx) G_idx,  acc <- 0 + bundle (.) acc  (not a CMUX),
 * d_idx = the standard switch to log2(2N) bits of the wrapping sum of the group's mask elements that idx selects,
 * idx = 1 .. 2^g - 1 (StandardMultiBitModulusSwitchedCt: the sum is switched, not each element), SignedDecomposer<u128>
 * as above.  The bundle is never formed: X^d is a pointwise factor in the transform domain, so a step is one
 * multiply-accumulate over the 2^g GGSWs of the group.
 * Not provided: non-native moduli, a LUT index per item, the C++ mirror, and the serialised
 * Fourier128LweMultiBitBootstrapKey format.
 *
 * mi_pbs128_multi_bit_limb_plan (no reference counterpart, needs no device): a column now sums 2^g GGSWs, so limb_bits
 * = the largest w with 2^g R N 2^(base_log - 1) (2^w - 1) <= (p - 1) / 2, R = (k + 1) level; n_limbs = ceil(128 / w)
 * (w = 22, 6 limbs at the shape above).  grouping_factor outside {2, 3, 4} is MI_ERR_INVALID_ARG; the other argument
 * rules and the outputs are those of mi_pbs128_limb_plan, which it leaves as it is.  MI_ERR_UNSUPPORTED when n_limbs >
 * 32: the width is up to 4 bits below the classic one, so 32 limbs here are the 16 of mi_pbs128_limb_plan and every
 * shape that has a classic key has a multi-bit one (base 2^42, 3 levels, k = 1, N = 2048, g = 2: 22 limbs of 6 bits). */
int mi_pbs128_multi_bit_limb_plan(size_t polynomial_size, int k, int base_log, int level, int grouping_factor,
                                  int *limb_bits, int *n_limbs);
/* The multi-bit bootstrap key.  bsk_std: the reference's LweMultiBitBootstrapKey<u128> in standard form as a device
 * pointer: n_lwe / g groups of 2^g GGSWs, group-major, each GGSW in the level, row and polynomial layout
 * mi_pbs128_key_create takes; GGSW idx of group i encrypts prod_m (s[i g + m] XOR NOT bit_m(idx)), bit_m(idx) =
 * (idx >> (g - 1 - m)) & 1, as documented for mi_fft64_multi_bit_pbs_key_create
 * (lwe_multi_bit_bootstrap_key_generation.rs:398-421).  A private prepared copy is made on `stream`, which is
 * synchronised, as mi_pbs128_key_create makes it (with the multi-bit limb width; in place, no second key-sized
 * buffer), and with it the table of the 2N powers of the plan's 2N-th root (16 N bytes).  MI_ERR_INVALID_ARG for a
 * NULL argument, a grouping factor outside {2, 3, 4}, n_lwe that is 0 or no multiple of it, and where
 * mi_pbs128_limb_plan says so; MI_ERR_UNSUPPORTED for a plan that is not the Goldilocks plan of polynomial_size, k > 3
 * and more than 32 limbs.  The key borrows `plan`, which must outlive it. */
typedef struct mi_pbs128_multi_bit_key mi_pbs128_multi_bit_key;
int mi_pbs128_multi_bit_key_create(const mi_ntt64_plan *plan, const uint64_t *bsk_std, size_t n_lwe, int k,
                                   size_t polynomial_size, int base_log, int level, int grouping_factor,
                                   void *stream, mi_pbs128_multi_bit_key **out_key);
int mi_pbs128_multi_bit_key_destroy(mi_pbs128_multi_bit_key *key);
int mi_pbs128_multi_bit_key_info(const mi_pbs128_multi_bit_key *key, size_t *n_lwe, int *k, size_t *polynomial_size,
                                 int *base_log, int *level, int *grouping_factor, int *limb_bits, int *n_limbs);
/* multi_bit_f128_deterministic_blind_rotate_assign (:2257-2700), batched and in place: acc_glwe[b] ((k + 1)
 * polynomial_size u128) is divided by X^ms(body) and taken through the n_lwe / g steps acc <- bundle (.) acc.
 * lwe_in[b]: n_lwe + 1 u64 at the native 2^64 modulus, switched on the device (there is no ms_mode, as in the f64
 * multi-bit entries).  Async on `stream`, stream-ordered scratch, chunked as mi_blind_rotate128_batch
 * (MI_PBS128_CHUNK); batch = 0 is MI_OK.  The buffers of a call are disjoint (overlapping ones are
 * MI_ERR_INVALID_ARG and nothing is written). */
int mi_pbs128_multi_bit_blind_rotate_batch(const mi_pbs128_multi_bit_key *key, uint64_t *acc_glwe,
                                           const uint64_t *lwe_in, size_t batch, void *stream);
/* multi_bit_programmable_bootstrap_f128_lwe_ciphertext over a batch: that rotation of the one shared LUT GLWE `lut`,
 * then extract_lwe_sample_from_glwe_ciphertext at degree 0: lwe_out[b] = k polynomial_size + 1 u128. */
int mi_pbs128_multi_bit_batch(const mi_pbs128_multi_bit_key *key, uint64_t *lwe_out, const uint64_t *lwe_in,
                              const uint64_t *lut, size_t batch, void *stream);

/* ---- The 128-bit packing keyswitch and compression of noise squashing ---------------------------------------------
 * What shortint does with the u128 LWEs of the bootstrap above: compress_noise_squashed_ciphertexts_into_list
 * (shortint/list_compression/noise_squashing_compression.rs:23-118) packs them into GLWEs with
 * par_keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext at Scalar = u128 and stores them through
 * CompressedModulusSwitchedGlweCiphertext::compress (CompressedSquashedNoiseCiphertextList).  V1_4_NOISE_SQUASHING_COMP_
 * PARAM_MESSAGE_2_CARRY_2_KS_PBS_TUNIFORM_2M128 (shortint/parameters/v1_4/noise_squashing/p_fail_2_minus_128/mod.rs:
 * 21-32): base 2^61, 1 level, k = 6, N = 1024, 128 LWEs per GLWE, native u128 modulus, input LWE dimension 4096.
 * Integer-only and bit-exact; every u128 is two little-endian u64 words (lo, hi), u128 buffers are 16-byte aligned
 * device pointers, as in the section above.
 * Not provided: sample extraction of u128 LWEs at a monomial degree (the list's unpack, a client-side step),
 * non-native u128 moduli, the C++ mirror, serialised formats, and a digit pass fused into
 * the GEMM.
 *
 * mi_lwe_pksk128_create takes the reference's LwePackingKeyswitchKey<u128> layout as a device pointer: in_dim blocks
 * of `level` GLWE ciphertexts of (glwe_dim + 1) * polynomial_size u128, levels stored as
 * generate_lwe_packing_keyswitch_key writes them (lwe_packing_keyswitch_key_generation.rs:129-156), and prepares a
 * private device copy of the same size (16 signed bytes per word, for the int8 matrix cores); the preparation runs
 * on `stream` and synchronises it.  The argument rules of mi_lwe_pksk_create, except: MI_ERR_INVALID_ARG where
 * SignedDecomposer::<u128>::new asserts (decomposer.rs:86-90: base_log * level outside [1, 127]); MI_ERR_UNSUPPORTED
 * for base_log > 63 (a digit is held in 64 bits), then beyond the 2^17 GEMM-depth bound of mi_lwe_ksk_create,
 * in_dim * level * ceil((base_log + 1) / 8) < 2^17. */
typedef struct mi_lwe_pksk128 mi_lwe_pksk128;
int mi_lwe_pksk128_create(const uint64_t *pksk, size_t in_dim, int glwe_dim, size_t polynomial_size, int base_log,
                          int level, int device, void *stream, mi_lwe_pksk128 **out_key);
int mi_lwe_pksk128_destroy(mi_lwe_pksk128 *key);
int mi_lwe_pksk128_info(const mi_lwe_pksk128 *key, size_t *in_dim, int *glwe_dim, size_t *polynomial_size,
                        int *base_log, int *level);
/* keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext (lwe_packing_keyswitch.rs:296-379, calling :102-187) at
 * Scalar = u128 over a list of lists, as mi_lwe_packing_keyswitch_batch: n_lwe ciphertexts of in_dim + 1 u128,
 * ceil(n_lwe / lwe_per_glwe) GLWEs of (glwe_dim + 1) * polynomial_size u128 out, the last one holding the remainder;
 * lwe_per_glwe = 1 is the single keyswitch over a batch; lwe_per_glwe of 0 or above polynomial_size is
 * MI_ERR_INVALID_ARG; n_lwe = 0 is MI_OK.  Async on `stream`; stream-ordered scratch of at most 64 MiB of keyswitched
 * rows (or one row, if larger) plus their digits, freed before return: larger calls run in chunks. */
int mi_lwe_packing_keyswitch128_batch(const mi_lwe_pksk128 *key, uint64_t *glwe_out, const uint64_t *lwe_in,
                                      size_t n_lwe, size_t lwe_per_glwe, void *stream);
/* The u128 words (two u64 each) of one CompressedModulusSwitchedGlweCiphertext<u128>'s PackedIntegers:
 * ceil((glwe_dim * polynomial_size + bodies_count) * log_modulus / 128)
 * (compressed_modulus_switched_glwe_ciphertext.rs:229-232).  PackedIntegers<u128> packs into 128-bit words
 * (packed_integers.rs:39-130); as (lo, hi) u64 pairs that is the same bit string the u64 packer writes, rounded up to
 * an even u64 word count.  bodies_count <= polynomial_size and 1 <= log_modulus <= 128, as compress asserts
 * (:191-203); else MI_ERR_INVALID_ARG, here and below. */
int mi_glwe_compressed_words128(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus,
                                size_t *words);
/* CompressedModulusSwitchedGlweCiphertext::compress (:169-220) at Scalar = u128 over a batch: the first
 * glwe_dim * polynomial_size + bodies_count words of glwe[b] through modulus_switch (fft_impl/common.rs:10-23; the
 * identity at the production log_modulus 128, where the packing is a copy of those words), packed log_modulus bits
 * each, little end first, into packed[b] (mi_glwe_compressed_words128 u128).  Device pointers, async on `stream`. */
int mi_glwe_compress128_batch(uint64_t *packed, const uint64_t *glwe, size_t polynomial_size, int glwe_dim,
                              size_t bodies_count, int log_modulus, size_t batch, int device, void *stream);
/* CompressedModulusSwitchedGlweCiphertext::extract (:226-256) at Scalar = u128: glwe[b] ((glwe_dim + 1) *
 * polynomial_size u128) = the unpacked values (packed_integers.rs:132-222) shifted left by 128 - log_modulus, then
 * polynomial_size - bodies_count zeros. */
int mi_glwe_extract128_batch(uint64_t *glwe, const uint64_t *packed, size_t polynomial_size, int glwe_dim,
                             size_t bodies_count, int log_modulus, size_t batch, int device, void *stream);

/* ---- WoP-PBS: the bootstrap without padding bit on the f64-FFT path -------------------------------------------
 * The device counterpart of fft_impl/fft64/crypto/wop_pbs/mod.rs (public face: algorithms/lwe_wopbs.rs), what
 * shortint::wopbs and integer::wopbs are built on: bit extraction, circuit bootstrap, CMUX tree, rotation and vertical
 * packing, each batched over independent evaluations.  Native 2^64 modulus only, as the reference asserts.  Device
 * pointers, async on `stream`; stream-ordered scratch from the pool, returned before each call returns; batch = 0 is
 * MI_OK; a NULL argument, or a shape the reference would assert on, is MI_ERR_INVALID_ARG.  Every composite is the
 * sequence of the public stages named with it and equals that sequence bit for bit.
 * Not provided: key generation on the device, non-native moduli, the NTT-path twins, the C++ mirror.
 *
 * The private functional packing keyswitch (private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext,
 * algorithms/lwe_private_functional_packing_keyswitch.rs:20-88) against a key list:
 *   out = - sum_{i <= in_dim} sum_l digit_l(closest_representable(lwe[i])) * key[i][l]
 * The body word lwe[in_dim] is decomposed like the mask (a key has in_dim + 1 blocks) and nothing is added to the
 * output.  mi_lwe_pfpksk_list_create takes the reference's LwePrivateFunctionalPackingKeyswitchKeyList layout as a
 * device pointer: n_keys keys back to back, each in_dim + 1 blocks of `level` GLWEs of (glwe_dim + 1) *
 * polynomial_size u64, levels stored as generate_lwe_private_functional_packing_keyswitch_key writes them
 * (lwe_private_functional_packing_keyswitch_key_generation.rs:98-130), and prepares a private device copy (the
 * caller's buffer may be freed afterwards; the preparation runs on `stream` and synchronises it).  The argument rules
 * of mi_lwe_pksk_create, and: n_keys * (glwe_dim + 1) * polynomial_size in [1, 2^24); MI_ERR_UNSUPPORTED when
 * (in_dim + 1) * level * ceil((base_log + 1) / 8) >= 2^17 (the GEMM-depth bound of mi_lwe_ksk_create with the body
 * block counted). */
typedef struct mi_lwe_pfpksk_list mi_lwe_pfpksk_list;
int mi_lwe_pfpksk_list_create(const uint64_t *pfpksk_list, size_t n_keys, size_t in_dim, int glwe_dim,
                              size_t polynomial_size, int base_log, int level, int device, void *stream,
                              mi_lwe_pfpksk_list **out_key);
int mi_lwe_pfpksk_list_destroy(mi_lwe_pfpksk_list *key);
int mi_lwe_pfpksk_list_info(const mi_lwe_pfpksk_list *key, size_t *n_keys, size_t *in_dim, int *glwe_dim,
                            size_t *polynomial_size, int *base_log, int *level);
/* Every key of the list applied to every input: glwe_out[b * n_keys + j] ((glwe_dim + 1) * polynomial_size u64) is
 * key j applied to lwe_in[b] (in_dim + 1 u64), one GEMM on the int8 matrix cores whose digit operand all keys share.
 * With n_keys = glwe_dim + 1 the n_keys GLWEs of an input are one GGSW level matrix.  Bit-exact. */
int mi_lwe_pfpks_batch(const mi_lwe_pfpksk_list *key, uint64_t *glwe_out, const uint64_t *lwe_in, size_t n_lwe,
                       void *stream);

/* mi_fft64_ext_product_batch / mi_fft64_cmux_batch with one Fourier GGSW per item, the semantics of
 * mi_ext_product_ntt64_batch_indexed / mi_cmux_ntt64_batch_indexed: item b uses GGSW ggsw_index[b] (device u32 array of
 * `batch` entries) of the n_ggsw GGSWs stored back to back in ggsw_fourier_list; an item whose index is >= n_ggsw is
 * left untouched (both its GLWEs).  Both engines; per item the arithmetic of the shared-GGSW call, bit for bit. */
int mi_fft64_ext_product_batch_indexed(const mi_fft64_plan *plan, uint64_t *out_glwe, const uint64_t *in_glwe,
                                       const double *ggsw_fourier_list, const uint32_t *ggsw_index, size_t n_ggsw,
                                       int k, int base_log, int level, size_t batch, void *stream);
int mi_fft64_cmux_batch_indexed(const mi_fft64_plan *plan, uint64_t *ct0, uint64_t *ct1,
                                const double *ggsw_fourier_list, const uint32_t *ggsw_index, size_t n_ggsw, int k,
                                int base_log, int level, size_t batch, void *stream);

/* extract_bits (wop_pbs/mod.rs:61-220) over a batch: lwe_in[b] (k N + 1 u64 of the bootstrap key's output) gives
 * lwe_list_out[b * n_bits + j] (ksk output size, n + 1 u64), j = 0 the most significant of the n_bits bits from bit
 * delta_log up, each encoded in the top bit.  Per bit from the least significant: left shift by
 * 64 - delta_log - bit - 1, mi_lwe_keyswitch_batch, store, + 2^62 on the body, mi_fft64_pbs_batch (standard modulus
 * switch) with the trivial accumulator of body -2^(delta_log - 1 + bit), + 2^(delta_log + bit - 1) on the output body,
 * subtract from the running input; the last bit stops after the keyswitch.  All items advance one bit per step.
 * ksk: k N -> n of bsk; delta_log + n_bits <= 64, delta_log >= 1 when n_bits > 1. */
int mi_fft64_extract_bits_batch(const mi_fft64_pbs_key *bsk, const mi_lwe_ksk *ksk, uint64_t *lwe_list_out,
                                const uint64_t *lwe_in, int delta_log, size_t n_bits, size_t batch, void *stream);
/* circuit_bootstrap_boolean + homomorphic_shift_boolean (:238-435) over a batch of boolean LWEs (n + 1 u64, the bit at
 * delta_log).  ggsw_std_out[b]: level_cbs x n_keys GLWEs of the pfpksk's output size, output index 0 = decomposition
 * level level_cbs (the layout the f64 external product reads); ggsw_fourier_out[b]: the same through forward_as_torus
 * in out_plan's order (fill_with_forward_fourier), level_cbs * n_keys^2 * N / 2 complex.  Either may be NULL, not
 * both.  The sequence: one mi_fft64_pbs_batch_lut_indexed over batch * level_cbs items, item b * level_cbs + i =
 * lwe_in[b] * 2^(63 - delta_log) with 2^62 added to the body, accumulator body -2^(63 - base_log_cbs * (level_cbs -
 * i)), the same constant added to the output body; one mi_lwe_pfpks_batch over those LWEs; mi_bsk_to_fourier64.
 * pfpksk: in_dim = k N of bsk, n_keys = glwe_dim + 1; out_plan: the pfpksk's polynomial size. */
int mi_fft64_circuit_bootstrap_boolean_batch(const mi_fft64_pbs_key *bsk, const mi_lwe_pfpksk_list *pfpksk,
                                             const mi_fft64_plan *out_plan, uint64_t *ggsw_std_out,
                                             double *ggsw_fourier_out, const uint64_t *lwe_in, size_t batch,
                                             int delta_log, int base_log_cbs, int level_cbs, void *stream);
/* The GGSW lists of the three calls below: batch x ggsw_stride Fourier GGSWs, item b's at b * ggsw_stride; a call
 * reads GGSWs [ggsw_first, ggsw_first + count) of each item (batch * ggsw_stride < 2^32) and nothing of the others,
 * so the result equals the call on the contiguous list of those GGSWs alone (ggsw_stride = count, ggsw_first = 0), bit
 * for bit.  count is r for the tree and n_rot for the rotation; ggsw_first + count > ggsw_stride is
 * MI_ERR_INVALID_ARG ("the GGSW range exceeds the GGSWs of an item"), checked before any buffer is read; count = 0 with
 * ggsw_first = ggsw_stride is the empty range at the item's end.  Every item evaluates n_outputs functions with the
 * same GGSWs.
 *
 * cmux_tree_memory_optimized (:459-583): lut_polys holds n_outputs x n_polys polynomials (N u64, shared by the batch),
 * n_polys = 2^r (else MI_ERR_INVALID_ARG); glwe_out[b * n_outputs + o] = the tree over output o's polynomials as trivial
 * GLWEs, layer j doing 2^(r-1-j) CMUXes t0 + G (.) (t1 - t0) with GGSW ggsw_first + r - 1 - j of the item; r = 0 writes
 * the trivial GLWE.  Breadth-first: a layer of all trees in the chunk is one mi_fft64_cmux_batch_indexed call, in
 * place; the chunk is the whole trees (2^r GLWEs each) that fit 256 MiB of scratch, at least one tree. */
int mi_fft64_cmux_tree_batch(const mi_fft64_plan *plan, uint64_t *glwe_out, const uint64_t *lut_polys, size_t n_polys,
                             size_t n_outputs, const double *ggsw_fourier_list, size_t ggsw_stride, size_t ggsw_first,
                             size_t r, int k, int base_log, int level, size_t batch, void *stream);
/* blind_rotate_assign (:838-863), in place on glwe[b * n_outputs + o]: from GGSW ggsw_first + n_rot - 1 down to
 * ggsw_first, ct1 = ct0 / X^d (polynomial_wrapping_monic_monomial_div_assign: d acts mod 2N), d <- 2 d from d = 1, then
 * mi_fft64_cmux_batch_indexed(ct0, ct1). */
int mi_fft64_wop_blind_rotate_batch(const mi_fft64_plan *plan, uint64_t *glwe, size_t n_outputs,
                                    const double *ggsw_fourier_list, size_t ggsw_stride, size_t ggsw_first,
                                    size_t n_rot, int k, int base_log, int level, size_t batch, void *stream);
/* vertical_packing (:771-825): mi_fft64_cmux_tree_batch over the first floor(log2(n_polys)) GGSWs of each item (none
 * when the item has fewer), mi_fft64_wop_blind_rotate_batch over the rest, mi_sample_extract_batch at degree 0;
 * lwe_out is batch x n_outputs x (k N + 1).  Where the reference would panic (n_polys not a power of two; no tree but
 * more than one polynomial) MI_ERR_INVALID_ARG. */
int mi_fft64_vertical_packing_batch(const mi_fft64_plan *plan, uint64_t *lwe_out, const uint64_t *lut_polys,
                                    size_t n_polys, size_t n_outputs, const double *ggsw_fourier_list, size_t n_ggsw,
                                    int k, int base_log, int level, size_t batch, void *stream);
/* circuit_bootstrap_boolean_vertical_packing (:638-732; circuit_bootstrap_boolean_vertical_packing_lwe_ciphertext_
 * list_mem_optimized, algorithms/lwe_wopbs.rs:644-698): mi_fft64_circuit_bootstrap_boolean_batch of each item's n_bits
 * input LWEs (lwe_list_in: batch x n_bits x (n + 1), most significant first, as extract_bits writes them) at
 * delta_log = 63 into a Fourier GGSW list in scratch, then mi_fft64_vertical_packing_batch of the n_outputs chunks of
 * n_polys polynomials of big_lut (shared by the batch) in out_plan; lwe_out: batch x n_outputs x (k' N' + 1) of the
 * pfpksk's GLWE shape. */
int mi_fft64_circuit_bootstrap_boolean_vertical_packing_batch(
    const mi_fft64_pbs_key *bsk, const mi_lwe_pfpksk_list *pfpksk, const mi_fft64_plan *out_plan, uint64_t *lwe_out,
    const uint64_t *lwe_list_in, size_t n_bits, const uint64_t *big_lut, size_t n_polys, size_t n_outputs,
    int base_log_cbs, int level_cbs, size_t batch, void *stream);

/* ---- LWE linear algebra with gather (core_crypto/algorithms/lwe_linear_algebra.rs) -----------------------------
 * lwe_out[i] = sum_t coeff[i * terms + t] * lwe_in[index[i * terms + t]] + (0, ..., 0, plaintext[i]) for i < n_out, on
 * rows of lwe_dim + 1 u64, native modulus with wrapping u64 arithmetic.  A term whose index is >= n_in contributes
 * nothing (ragged term counts, trivial ciphertexts); terms = 0 gives the trivial ciphertexts of `plaintext` (lwe_in is
 * not read).  index (u32) and coeff (i64) are device arrays of n_out * terms entries; coeff NULL: every coefficient 1;
 * plaintext: device array of n_out u64 or NULL (nothing added).  With the right index and coefficients this one call
 * is lwe_ciphertext_add[_assign] (:67, :190), lwe_ciphertext_sub[_assign] (:702, :789), lwe_ciphertext_opposite_assign
 * (:490), lwe_ciphertext_cleartext_mul[_assign] (:555, :624), lwe_ciphertext_plaintext_add_assign (:275) and
 * _plaintext_sub_assign (:383), shortint's bivariate packing lhs * factor + rhs (shortint/server_key/
 * bivariate_pbs.rs:152-167), and the gather / scatter of the CUDA backend's lwe_indexes_in / lwe_indexes_out
 * (backends/tfhe-cuda-backend/cuda/include/pbs/programmable_bootstrap.h).  Device pointers on `device`, async on
 * `stream`; n_out = 0 is MI_OK; lwe_out overlapping lwe_in is MI_ERR_INVALID_ARG ("lwe_out overlaps lwe_in"), as are
 * lwe_dim outside [1, 2^24), n_in or n_out >= 2^31 and terms >= 2^16. */
int mi_lwe_linear_combination_batch(uint64_t *lwe_out, const uint64_t *lwe_in, size_t lwe_dim, size_t n_in,
                                    size_t n_out, size_t terms, const uint32_t *index, const int64_t *coeff,
                                    const uint64_t *plaintext, int device, void *stream);

/* ---- shortint: lookup tables and the KS -> MS -> PBS atomic pattern --------------------------------------------
 * Reference paths relative to tfhe/src/shortint.  A mi_shortint_key bundles what shortint::ServerKey holds for the
 * KS-PBS order (server_key/mod.rs, atomic_pattern/standard.rs): borrowed handles (the caller keeps them alive) of a
 * keyswitch key k N -> n, one bootstrap key of `pbs_engine` (mi_pbs_ntt64_key of the BNF variant, mi_fft64_pbs_key or
 * mi_fft64_multi_bit_pbs_key, passed as const void *) and, optionally, a mi_ms_noise_key (ModulusSwitchConfiguration::
 * DriftTechniqueNoiseReduction); the modulus switch of the bootstrap (MI_MS_STANDARD or MI_MS_CENTERED); and
 * message_modulus / carry_modulus.  It owns the seven lookup tables of the radix calls below (uploaded with a blocking
 * copy at creation).
 * mi_shortint_key_check states the argument rules on plain numbers, the first failing rule answering:
 * MI_ERR_INVALID_ARG "unknown pbs engine"; MI_ERR_UNSUPPORTED for a Solinas-variant NTT key (its input is not a native
 * LWE); MI_ERR_INVALID_ARG for ksk out_dim != the bootstrap key's n_lwe, ksk in_dim != k N, moduli that are not powers
 * of two or with message_modulus * carry_modulus > N / 2, an ms_mode other than the two above, an ms-noise key together
 * with the multi-bit engine, a centered switch with the multi-bit engine or with an ms-noise key (both end in the
 * standard switch), an ms-noise key of another dimension than n.  mi_shortint_key_create answers "out_key is NULL",
 * "key is NULL", then those rules read off its handles. */
typedef enum mi_shortint_pbs_engine {
    MI_SHORTINT_PBS_NTT64 = 0,
    MI_SHORTINT_PBS_FFT64 = 1,
    MI_SHORTINT_PBS_FFT64_MULTI_BIT = 2
} mi_shortint_pbs_engine;
typedef struct mi_shortint_key mi_shortint_key;
int mi_shortint_key_check(size_t ksk_in_dim, size_t ksk_out_dim, size_t pbs_n_lwe, int k, size_t polynomial_size,
                          int pbs_engine, int ntt_variant, int has_ms_noise, size_t ms_noise_lwe_dim, int ms_mode,
                          uint64_t message_modulus, uint64_t carry_modulus);
int mi_shortint_key_create(const mi_lwe_ksk *ksk, int pbs_engine, const void *pbs_key, const mi_ms_noise_key *ms_noise,
                           int ms_mode, uint64_t message_modulus, uint64_t carry_modulus, mi_shortint_key **out_key);
int mi_shortint_key_destroy(mi_shortint_key *key);
int mi_shortint_key_info(const mi_shortint_key *key, int *pbs_engine, int *ms_mode, int *has_ms_noise,
                         uint64_t *message_modulus, uint64_t *carry_modulus, size_t *big_lwe_dim,
                         size_t *small_lwe_dim);
/* fill_accumulator_with_encoding (engine/mod.rs:80-141), a host function: glwe_host ((k + 1) N u64) gets a zero mask
 * and the body of boxes of N / (m c) coefficients, box i holding table[i] * (2^63 / (m c)) (wrapping), the first half
 * box negated and the whole rotated left by half a box.  table_len must be m c.  The caller evaluates the function:
 * table[i] = f(i) is generate_lookup_table (server_key/mod.rs:805, :1649), table[i] = f((i / m) % m, i % m) is
 * generate_lookup_table_bivariate_with_factor at factor m (server_key/bivariate_pbs.rs:57-108). */
int mi_shortint_lut_fill(uint64_t *glwe_host, size_t polynomial_size, int k, uint64_t message_modulus,
                         uint64_t carry_modulus, const uint64_t *table, size_t table_len);
/* apply_lookup_table (server_key/mod.rs:935-960), apply_programmable_bootstrap (:1542), message_extract
 * (:1189), carry_extract (:1111) and, after one packing call to mi_lwe_linear_combination_batch, unchecked_apply_lookup_table_bivariate
 * (server_key/bivariate_pbs.rs:141-190), batched: lwe_in holds n_in LWEs of k N + 1 u64, lwe_out n_items.  The sequence:
 * mi_lwe_keyswitch_batch of all n_in inputs; with an ms-noise key mi_lwe_ms_noise_improve_and_switch_batch at
 * log2(2 N), the bootstrap then running MI_MS_PRE_SWITCHED; with in_index (device u32, n_items entries) the gather
 * mi_lwe_linear_combination_batch of the small LWEs, item j taking input in_index[j] (one input may feed several lookup
 * tables for one keyswitch), without it n_items must equal n_in; the engine's *_pbs_batch_lut_indexed with lut_list
 * (n_lut GLWEs) and lut_index (device u32; NULL: item j uses GLWE j).  An item with in_index >= n_in or lut_index >=
 * n_lut is left untouched.  lwe_out == lwe_in is the reference's _assign form; a partial overlap is
 * MI_ERR_INVALID_ARG.  Async on `stream`, stream-ordered scratch. */
int mi_shortint_apply_lut_batch(const mi_shortint_key *key, uint64_t *lwe_out, const uint64_t *lwe_in, size_t n_in,
                                const uint32_t *in_index, const uint64_t *lut_list, const uint32_t *lut_index,
                                size_t n_lut, size_t n_items, void *stream);

/* ---- Radix integers (tfhe/src/integer) --------------------------------------------------------------------------
 * A radix batch is n_integers x n_blocks LWEs of k N + 1 u64, the least significant block first.  All three calls are
 * in place on device memory, async on `stream`, and fixed sequences of mi_lwe_linear_combination_batch and
 * mi_shortint_apply_lut_batch (written out at the top of csrc/c_api_shortint.cpp); n_integers = 0 is MI_OK, n_blocks =
 * 0 MI_ERR_INVALID_ARG.
 * mi_radix_propagate_single_carry_batch: blocks of value <= 2 (m - 1) -> blocks < m, the Hillis-Steele prefix scan of
 * compute_prefix_sum_hillis_steele (integer/server_key/radix_parallel/add.rs:1452-1487) as the CUDA backend's
 * host_propagate_single_carry runs it (backends/tfhe-cuda-backend/cuda/src/integer/integer.cuh).  Round 1: one
 * keyswitch per block and two lookup tables, the message x mod m and the state NONE 0 / GENERATED 1 (x >= m) /
 * PROPAGATED 2 (x = m - 1; never for block 0); ceil(log2 n_blocks) scan rounds, round r combining block i >= 2^r with
 * block i - 2^r through one bivariate table on m * cur + prev (cur = PROPAGATED takes prev); a last round (message_i
 * + carry_{i-1}) mod m: 2 + ceil(log2 n_blocks) bootstrap rounds, one at n_blocks = 1.  carry_out (n_integers LWEs, or
 * NULL) receives the carry out of the top block.  MI_ERR_UNSUPPORTED unless m c >= 16, c <= m and 2 m + 2 < m c (the
 * packed scan operand has to stay under the padding bit), for n_blocks > 1.
 * mi_radix_full_propagate_batch (full_propagate_parallelized, radix_parallel/mod.rs:228; partial_propagate :91-201): blocks of any value
 * < m c.  One round of message_extract and carry_extract on every block, each carry added into the next block, then the
 * single-carry propagation (:140-158); where that is unsupported, the extract-and-add round n_blocks - 1 more times,
 * which ends in the blocks of the sequential loop (:187-199).
 * mi_radix_add_batch: radix_out = lhs + rhs blockwise (radix_out may be lhs or rhs), then the single-carry propagation:
 * add_parallelized on clean inputs (radix_parallel/add.rs), and with carry_out unsigned_overflowing_add_parallelized.
 * carry_out (n_integers LWEs) is written last and is disjoint from every other buffer of the call: one that overlaps
 * radix (propagation), or radix_out, lhs or rhs (addition), is MI_ERR_INVALID_ARG before any device call. */
int mi_radix_propagate_single_carry_batch(const mi_shortint_key *key, uint64_t *radix, uint64_t *carry_out,
                                          size_t n_blocks, size_t n_integers, void *stream);
int mi_radix_full_propagate_batch(const mi_shortint_key *key, uint64_t *radix, size_t n_blocks, size_t n_integers,
                                  void *stream);
int mi_radix_add_batch(const mi_shortint_key *key, uint64_t *radix_out, const uint64_t *lhs, const uint64_t *rhs,
                       uint64_t *carry_out, size_t n_blocks, size_t n_integers, void *stream);

/* ---- Radix sum of ciphertexts and multiplication (tfhe/src/integer/server_key/radix_parallel) -------------------
 * unchecked_partial_sum_ciphertexts_vec_parallelized (sum.rs:14-147), unchecked_sum_ciphertexts_vec_parallelized
 * (sum.rs:155-166), sum_ciphertexts_parallelized (sum.rs:183), compute_terms_for_mul_low (mul.rs:333-400),
 * unchecked_mul_assign_parallelized (mul.rs:437-460) and mul_parallelized (mul.rs:599-608) on clean operands, batched.
 * Both calls are fixed sequences of mi_lwe_linear_combination_batch and mi_shortint_apply_lut_batch (written out at
 * the top of csrc/c_api_radix_mul.cpp) driven by one data-independent schedule; their index arrays are written on
 * the device from descriptors passed as kernel arguments, so nothing is copied from the host and no call
 * synchronises.  The two lookup tables of the multiplication, (x, y) -> (x y) mod m and (x y) / m on m x + y, are the
 * key's sixth and seventh.
 *
 * mi_radix_sum_schedule, a host function: the schedule of the sum of n_terms radix terms of n_blocks blocks, term t
 * being identically zero below block first_block[t] (the blocks the reference skips by degree == 0; NULL: all 0).
 * s = (m c - 1) / (m - 1) = max_sum_size(Degree(m - 1)) (shortint/server_key/mod.rs) rows of value <= m - 1 fill a
 * block.  Column b starts as block b of every term with first_block[t] <= b, in term order.  While some column holds
 * more than s rows, a round runs: every column of at least s rows (exactly s too) gives len / s chunks of its first
 * rows, in order; each chunk is summed, the sum gives its message (x mod m) and, unless the column is the last, its
 * carry (x / m); the next list of column b is its last len % s rows, the carries of column b - 1's chunks in chunk
 * order, the messages of its own chunks in chunk order; columns of fewer than s rows pass through.  At the end block
 * b is the sum of column b's rows (an empty column: a trivial zero).  *n_rounds gets the round count R; column_len
 * ((R + 1) x n_blocks, or NULL) the length of every column at the start of round r and, row R, at the end;
 * column_chunks (R x n_blocks, or NULL) the chunks of every column in round r; rounds_capacity is the R the arrays
 * have room for (MI_ERR_INVALID_ARG when it is below R; call with NULL arrays first).  MI_ERR_UNSUPPORTED unless m >=
 * 2 and 2 <= c <= m (with c > m a carry can pass m - 1 and a later chunk m c - 1); MI_ERR_INVALID_ARG for n_blocks =
 * 0, first_block[t] > n_blocks and n_blocks * n_terms >= 2^22.  n_terms = 0 is valid (no rounds, empty columns). */
int mi_radix_sum_schedule(size_t n_blocks, size_t n_terms, const uint32_t *first_block, uint64_t message_modulus,
                          uint64_t carry_modulus, size_t *n_rounds, uint32_t *column_len, uint32_t *column_chunks,
                          size_t rounds_capacity);
/* unchecked_sum_ciphertexts_vec_parallelized over a batch: radix_out (n_integers x n_blocks LWEs) = the sum mod
 * m^n_blocks of n_terms radix batches stored back to back (term t at row t * n_integers * n_blocks of `terms`), every
 * block clean (< m).  first_block is a host array (read before the call returns) or NULL; rows below first_block[t]
 * are never read.  The sequence: one linear combination gathers the live rows into the scratch pool; per round of the
 * schedule one linear combination with terms = s forms every chunk sum of every integer and one
 * mi_shortint_apply_lut_batch gives every chunk its message and (not in the last column) its carry for one keyswitch;
 * one linear combination (terms = s, ragged rows padded with 0xFFFFFFFF) forms the block sums into radix_out; then
 * mi_radix_full_propagate_batch(radix_out).  n_terms = 0 writes trivial zeros (nothing to propagate); n_terms = 1 and 2
 * go the general way (the reference's shortcut through add_parallelized gives the same values).  radix_out may not
 * overlap terms (MI_ERR_INVALID_ARG).  Async on `stream`, stream-ordered scratch; the limits of mi_radix_add_batch, and
 * MI_ERR_INVALID_ARG "batch too large" for n_terms * n_integers * n_blocks >= 2^31; MI_ERR_UNSUPPORTED as the schedule,
 * and above 128 blocks (the per-column descriptors of a round are one kernel argument).  n_integers = 0 is MI_OK.
 * Scratch: per integer the rows of the terms plus two rows per chunk of every round; the integers run in passes whose
 * scratch block stays under 512 MiB (a pass holds at least one integer), each pass the call on its integers, bit for
 * bit.  mi_radix_sum_pass_integers / mi_radix_mul_pass_integers answer how many integers a pass of such a call holds
 * (host functions; at most n_integers). */
int mi_radix_sum_batch(const mi_shortint_key *key, uint64_t *radix_out, const uint64_t *terms, size_t n_terms,
                       const uint32_t *first_block, size_t n_blocks, size_t n_integers, void *stream);
int mi_radix_sum_pass_integers(const mi_shortint_key *key, size_t n_terms, const uint32_t *first_block,
                               size_t n_blocks, size_t n_integers, size_t *pass_integers);
/* mul_parallelized on clean operands over a batch: radix_out = lhs * rhs mod m^n_blocks.  With B = n_blocks: one
 * linear combination packs m * lhs[x] + rhs[y] for the B (B + 1) / 2 pairs with x + y < B of every integer (lhs and
 * rhs staged in one list by two device-to-device copies); one mi_shortint_apply_lut_batch gives every pair its lsb
 * (x y) mod m and, at m > 2 and x + y < B - 1, its msb (x y) / m, written as the columns of the 2 B - 1 (B at m = 2)
 * shifted terms of compute_terms_for_mul_low in its chain order, the zero blocks of the shifts never made: the lsb
 * term of rhs block y starts at block y and holds lsb(lhs[b - y], rhs[y]), the msb term of rhs block y < B - 1 starts
 * at block y + 1 and holds msb(lhs[b - y - 1], rhs[y]); then the rounds, block sums and propagation of
 * mi_radix_sum_batch on those columns.  The result equals, bit for bit, the pack, the lookup, a scatter of its
 * outputs into dense terms and mi_radix_sum_batch with that first_block.  radix_out may be lhs or rhs (it is written
 * last) and lhs may be rhs; a partial overlap of radix_out with an operand is MI_ERR_INVALID_ARG before any device
 * call.  MI_ERR_UNSUPPORTED unless 2 <= c = m (the packed operand needs c >= m, the schedule c <= m) and n_blocks <=
 * 128.  Scratch per integer: the B^2 product rows (B (B + 1) / 2 at m = 2), then the packed pairs and the staged
 * operands (B (B + 1) / 2 + 2 B rows) or two rows per chunk of every round, whichever is more (1808 rows, 29.6 MB,
 * per 64-bit integer at m = c = 4, N = 2048: 18 integers per pass), in passes as above. */
int mi_radix_mul_batch(const mi_shortint_key *key, uint64_t *radix_out, const uint64_t *lhs, const uint64_t *rhs,
                       size_t n_blocks, size_t n_integers, void *stream);
int mi_radix_mul_pass_integers(const mi_shortint_key *key, size_t n_blocks, size_t n_integers, size_t *pass_integers);
/* The index arrays the multiplication driver writes on the device for a pass of n_integers integers, into the
 * caller's device arrays (for tests, and for a port that issues the stages itself).  Rows are numbered slot-major: slot
 * v of integer i is row v * n_integers + i of the pool, of the chunk sums and of the packed pairs alike; the pool's
 * first slots are the products, column by column in the order given with mi_radix_mul_batch (column b at slot b^2, at
 * b (b + 1) / 2 when m = 2); round r's outputs take the next slots, column by column: the carries of column b - 1's
 * chunks, then the messages of column b's chunks.  step = 0, the product round: index and coeff (2 entries per packed
 * row) = the pack's index and coefficient arrays, pair p = d (d + 1) / 2 + y for (x, y), d = x + y, over lhs[I B] |
 * rhs[I B]; in_index / lut_index (one entry per product row) = the pair's packed row and table 5 (lsb) or 6 (msb).
 * step = r + 1, round r of the schedule: index (s entries per chunk sum, chunks numbered column by column) = the
 * pool rows of the chunk; in_index / lut_index (one entry per output row) = the chunk-sum row and table 0 (message)
 * or 1 (carry).  step = rounds + 1, the block sums: index (s entries per row i * n_blocks + b, padded with
 * 0xFFFFFFFF); no items.  *n_index / *n_items get the entries written.  `capacity` is the entries each array holds
 * (coeff too); every step up to `step` is run through the arrays, and MI_ERR_INVALID_ARG answers before any launch
 * when one needs more.  Async on `stream`. */
int mi_radix_mul_index_arrays(uint64_t message_modulus, uint64_t carry_modulus, size_t n_blocks, size_t n_integers,
                              size_t step, uint32_t *index, int64_t *coeff, uint32_t *in_index, uint32_t *lut_index,
                              size_t capacity, size_t *n_index, size_t *n_items, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TFHE_NTT_AMD_H */
