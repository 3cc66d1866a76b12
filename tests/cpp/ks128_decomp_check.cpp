// Host check of the 128-bit packing keyswitch's digit functions (csrc/core_scalar.hpp: the pre-rounded decomp_init and
// decomp_next at u128, read as int64_t as the kernel does; csrc/ks128_decomp.hpp: digit_byte, signed_bytes16) against a
// plain restatement of the reference's decomposition in unsigned __int128 (commons/math/decomposition/
// decomposer.rs:25-49 closest representable, :156-185 init, iter.rs:131-151 one level) and against digits computed
// elsewhere.
// Input (stdin), one case per line: base_log level word_hi(hex) word_lo(hex) term_0 .. term_{level-1} (signed decimal,
// least significant level first: the digits of closest_representable(word)).
// Per case: every digit equals the restatement's and the listed one, its nd = ceil((B + 1) / 8) signed bytes recompose
// to it, and the word's 16 signed bytes recompose to the word mod 2^128.  On top of the listed cases: every base_log
// 1..63 at one level on the words around 0 and 2^127 and on random words.  On every one of these words the plain form
// (pre_rounded = false: the 128-bit bootstraps' use, read as they read it) must equal the restatement's digits of the
// word itself too.
// Build: hipcc -O2 -x hip ks128_decomp_check.cpp -o ks128_decomp_check (host code only, no GPU needed).
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <random>

#include "../../tfhe-rs-main_modified_amd/csrc/ks128_decomp.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;

static u128 closest(u128 x, int base_log, int level) {
  const unsigned shift = 128u - (unsigned)(base_log * level) - 1u;
  return (((x >> shift) + 1u) & ~(u128)1) << shift;
}
static u128 init_native(u128 input, int base_log, int level) {
  const unsigned rep = base_log * level, non_rep = 128u - rep;
  u128 res = input >> (non_rep - 1);
  const u128 rounding_bit = res & 1u;
  res += 1;
  res >>= 1;
  res &= (~(u128)0) >> (128u - rep);
  const u128 need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
  return res - (need_balance << rep);
}
static i128 one_level(int base_log, u128& state) {
  const u128 mask = ((u128)1 << base_log) - 1;
  const u128 res = state & mask;
  state = (u128)((i128)state >> base_log);
  const u128 carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return (i128)(res - (carry << base_log));
}

static long checked = 0, bad = 0;

static void report(const char* what, int B, int L, u128 x, int l) {
  if (bad++ < 20)
    printf("%s: B=%d L=%d x=%016" PRIx64 "%016" PRIx64 " level %d\n", what, B, L, (uint64_t)(x >> 64), (uint64_t)x, l);
}

// the digits of one word as the kernels compute them; `listed` may be null
static void check(int B, int L, u128 x, const int64_t* listed) {
  u128 want_state = init_native(closest(x, B, L), B, L);
  u128 state = mi::core::decomp_init<u128>(x, B, L, true);
  const int nd = mi::ks128::digit_bytes(B);
  if (nd != (B + 1 + 7) / 8 || nd > 8) report("digit_bytes", B, L, x, -1);
  for (int l = 0; l < L; ++l) {
    const i128 want = one_level(B, want_state);
    const int64_t got = (int64_t)(i128)mi::core::decomp_next<u128>(B, state);
    i128 from_bytes = 0;  // sum_s e_s 256^s, as the GEMM recomposes the digit
    for (int s = 0; s < nd; ++s) from_bytes += (i128)mi::ks128::digit_byte(got, s) * ((i128)1 << (8 * s));
    ++checked;
    if ((i128)got != want || (listed && got != listed[l]) || from_bytes != want) report("digit", B, L, x, l);
  }
  u128 want_plain = init_native(x, B, L), plain = mi::core::decomp_init<u128>(x, B, L);
  for (int l = 0; l < L; ++l) {
    const i128 want = one_level(B, want_plain);
    const int64_t got = (int64_t)(uint64_t)mi::core::decomp_next<u128>(B, plain);
    ++checked;
    if ((i128)got != want) report("plain digit", B, L, x, l);
  }
  int8_t b[16];
  mi::ks128::signed_bytes16(x, b);
  u128 back = 0;  // sum_t s_t 2^(8t) mod 2^128
  for (int t = 0; t < 16; ++t) back += (u128)(i128)b[t] << (8 * t);
  if (back != x) report("key bytes", B, L, x, -1);
}

int main() {
  int B, L;
  uint64_t hi, lo;
  long listed_cases = 0;
  while (scanf("%d %d %" SCNx64 " %" SCNx64, &B, &L, &hi, &lo) == 4) {
    int64_t terms[128];
    if (B < 1 || B > 63 || L < 1 || B * L > 127) return 2;
    for (int l = 0; l < L; ++l)
      if (scanf("%" SCNd64, &terms[l]) != 1) return 2;
    check(B, L, ((u128)hi << 64) | lo, terms);
    ++listed_cases;
  }
  std::mt19937_64 rng(11);
  for (B = 1; B <= 63; ++B) {
    const u128 half = (u128)1 << (127 - B);
    for (u128 c : {(u128)0, (u128)1 << 127, (u128)1 << 64}) {
      for (u128 d : {(u128)0, (u128)1, ~(u128)0, half, half - 1, (u128)0 - half, (u128)0 - half - 1, 2 * half,
                     (u128)0 - 2 * half})
        check(B, 1, c + d, nullptr);
    }
    for (int i = 0; i < 2000; ++i) {
      const u128 x = ((u128)rng() << 64) | rng();
      check(B, 1, x, nullptr);
    }
  }
  printf("%ld listed cases, %ld digits checked, %ld mismatches\n", listed_cases, checked, bad);
  return bad ? 1 : 0;
}
