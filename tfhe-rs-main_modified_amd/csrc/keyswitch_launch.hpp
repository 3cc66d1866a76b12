// keyswitch_launch.hpp — host entry points of keyswitch.hip and packing_keyswitch.hip (kept out of ntt64_launch.hpp,
// which every kernel source includes).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mi {

// Which keyswitch a prepared key serves.  The key object states it; the launch infers nothing from the parameters.
enum class KsMode {
  Native,   // keyswitch_lwe_ciphertext (lwe_keyswitch.rs:137-227): u64 key, 8 byte planes, u64 rows
  Ks32,     // keyswitch_lwe_ciphertext_with_scalar_change (:331-447): u32 key, 4 byte planes, u32 rows mod 2^out_log
  Packing,  // keyswitch_lwe_ciphertext_into_glwe_ciphertext (lwe_packing_keyswitch.rs:102-187): u64 key of (k+1) N
            // columns, digits of the pre-rounded mask, the body at column k N
  Pfpks,    // private_functional_keyswitch_lwe_ciphertext_into_glwe_ciphertext (lwe_private_functional_packing_
            // keyswitch.rs:20-88) against a key list: in_dim + 1 blocks per key (the body word is decomposed like the
            // mask, pre-rounded), n_keys (k+1) N columns, nothing added to the output
};

// The geometry of one prepared key: in_dim blocks of `level` rows of out_size words.
struct KsGeometry {
  KsMode mode = KsMode::Native;
  size_t in_dim = 0, out_size = 0;  // out_size: out_dim + 1 (Native, Ks32) or (k + 1) N (Packing)
  int base_log = 0, level = 0;
  int out_log = 64;     // Ks32: the output modulus 2^out_log (1 <= out_log <= 32)
  size_t body_col = 0;  // the output column that receives the input body: out_size - 1, or k N when packing
  size_t n_keys = 1;    // Pfpks: keys of the list, out_size / n_keys columns each (in_dim + 1 blocks of `level` rows)
};

// keyswitch.hip — the keyswitches on the int8 matrix cores.
size_t ks_key_bytes(const KsGeometry& g);   // the prepared key (byte-plane MFMA fragments)
int ks_digit_bytes_per_term(int base_log);  // signed bytes per decomposition digit
size_t ks_digit_bytes(const KsGeometry& g, size_t batch);  // the digit fragments of `batch` input rows
// ksk: u64 words (Native, Packing) or u32 words (Ks32) in the reference layout
hipError_t launch_ksk_prepare(void* frag, const void* ksk, const KsGeometry& g, hipStream_t s);
// out: batch rows of out_size u64 (Native, Packing) or u32 (Ks32) words
hipError_t launch_keyswitch(void* out, const uint64_t* lwe_in, const void* frag, void* digits, size_t batch,
                            const KsGeometry& g, hipStream_t s);
// the (centered binary) modulus switch of u32 LWEs of dimension dim to [0, 2^log_mod): (dim + 1) u64 per ciphertext
hipError_t launch_lwe_ms32(uint64_t* out, const uint32_t* in, size_t dim, size_t batch, int log_mod, bool centered,
                           hipStream_t st);
// the same for u64 LWEs (the native-modulus ciphertexts): (dim + 1) u64 per ciphertext in [0, 2^log_mod)
hipError_t launch_lwe_ms64(uint64_t* out, const uint64_t* in, size_t dim, size_t batch, int log_mod, bool centered,
                           hipStream_t st);

// packing_keyswitch.hip — keyswitch_lwe_ciphertext_list_and_pack_in_glwe_ciphertext (lwe_packing_keyswitch.rs:
// 296-379) and CompressedModulusSwitchedGlweCiphertext (compressed_modulus_switched_glwe_ciphertext.rs:169-256).
// One call's scratch: `rows` ciphertexts go through the GEMM at a time (whole GLWEs while one fits PKS_ROW_CAP_BYTES).
static constexpr size_t PKS_ROW_CAP_BYTES = (size_t)64 << 20;
struct PksPlan {
  size_t rows = 0;      // ciphertexts per GEMM launch
  bool piecewise = false;  // one GLWE's rows exceed the cap: `rows` rows of it at a time, summed into the output
  size_t part = 0;      // partial-sum slices of the rotate-and-sum pass per GLWE (1: written directly)
  size_t t_bytes = 0, digit_bytes = 0, partial_bytes = 0;
};
PksPlan pks_plan(const KsGeometry& g, size_t n_lwe, size_t lwe_per_glwe);
// the same plan for rows of out_size words of word_bytes bytes; digit_bytes is left 0 (the caller's GEMM sizes it)
PksPlan pks_plan_rows(size_t out_size, size_t word_bytes, size_t n_lwe, size_t lwe_per_glwe);
// glwe_out: ceil(n_lwe / lwe_per_glwe) GLWEs of out_size words; t / digits / partials: scratch of the plan's sizes
hipError_t launch_packing_keyswitch(uint64_t* glwe_out, const uint64_t* lwe_in, const void* frag, void* t, void* digits,
                                    void* partials, size_t n_lwe, size_t lwe_per_glwe, size_t polynomial_size,
                                    const KsGeometry& g, const PksPlan& plan, hipStream_t s);
// u64 words of one compressed GLWE: ceil((k N + bodies) log_modulus / 64)
size_t glwe_compressed_words(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus);
hipError_t launch_glwe_compress(uint64_t* packed, const uint64_t* glwe, size_t polynomial_size, int glwe_dim,
                                size_t bodies_count, int log_modulus, size_t batch, hipStream_t s);
hipError_t launch_glwe_extract(uint64_t* glwe, const uint64_t* packed, size_t polynomial_size, int glwe_dim,
                               size_t bodies_count, int log_modulus, size_t batch, hipStream_t s);

// packing_keyswitch128.hip — the same two operations at Scalar = u128 (shortint's noise-squashing compression):
// every u128 is two little-endian u64 words, 16-byte aligned.
struct Pks128Geometry {
  size_t in_dim = 0, out_size = 0;  // out_size = (k + 1) N u128 key columns
  int base_log = 0, level = 0;      // base_log <= 63
  size_t body_col = 0;              // k N
};
size_t pks128_key_bytes(const Pks128Geometry& g);                // the prepared key (16 signed-byte planes)
size_t pks128_digit_bytes(const Pks128Geometry& g, size_t rows);  // the digit fragments of `rows` input rows
hipError_t launch_pksk128_prepare(void* frag, const uint64_t* pksk, const Pks128Geometry& g, hipStream_t s);
// plan: pks_plan_rows(out_size, 16, ...) with digit_bytes = pks128_digit_bytes(g, plan.rows)
hipError_t launch_packing_keyswitch128(uint64_t* glwe_out, const uint64_t* lwe_in, const void* frag, void* t,
                                       void* digits, void* partials, size_t n_lwe, size_t lwe_per_glwe,
                                       size_t polynomial_size, const Pks128Geometry& g, const PksPlan& plan,
                                       hipStream_t s);
// u128 words of one compressed GLWE: ceil((k N + bodies) log_modulus / 128)
size_t glwe_compressed_words128(size_t polynomial_size, int glwe_dim, size_t bodies_count, int log_modulus);
hipError_t launch_glwe_compress128(uint64_t* packed, const uint64_t* glwe, size_t polynomial_size, int glwe_dim,
                                   size_t bodies_count, int log_modulus, size_t batch, hipStream_t s);
hipError_t launch_glwe_extract128(uint64_t* glwe, const uint64_t* packed, size_t polynomial_size, int glwe_dim,
                                  size_t bodies_count, int log_modulus, size_t batch, hipStream_t s);

}  // namespace mi
