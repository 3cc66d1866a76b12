// Host check of the keyswitch digit functions (csrc/core_scalar.hpp: decomp_init, decomp_next at u64, read as int64_t as
// the kernels do; csrc/ks_decomp.hpp: signed_byte) against a plain restatement of the reference's native decomposition
// (commons/math/decomposition/decomposer.rs:25-49 closest representable, :156-185 init, iter.rs:131-151 one level) and
// against digits computed elsewhere.
// Input (stdin), one case per line: base_log level pre_rounded word(hex) term_0 .. term_{level-1} (signed decimal,
// least significant level first; pre_rounded 1 = the packing keyswitch's digits of closest_representable(word)).
// Per case: every digit equals the restatement's and the listed one, and its nd = ceil((B + 1) / 8) signed bytes, the
// form in which the digit kernels hand it to the int8 GEMM, recompose to it.  On top of the listed cases: every
// base_log 1..63 at one level on the words around 0 and 2^63 and on random words.
// Build: hipcc -O2 -x hip ks_decomp_check.cpp -o ks_decomp_check (host code only, no GPU needed).
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <random>

#include "../../tfhe-rs-main_modified_amd/csrc/ks_decomp.hpp"

static uint64_t closest(uint64_t x, int base_log, int level) {
  const unsigned shift = 64u - (unsigned)(base_log * level) - 1u;
  return (((x >> shift) + 1u) & ~(uint64_t)1) << shift;
}
static uint64_t init_native(uint64_t input, int base_log, int level) {
  const unsigned rep = base_log * level, non_rep = 64u - rep;
  uint64_t res = input >> (non_rep - 1);
  const uint64_t rounding_bit = res & 1u;
  res += 1;
  res >>= 1;
  res &= (~0ull) >> (64u - rep);
  const uint64_t need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
  return res - (need_balance << rep);
}
static int64_t one_level(int base_log, uint64_t& state) {
  const uint64_t mask = (1ull << base_log) - 1;
  const uint64_t res = state & mask;
  state = (uint64_t)((int64_t)state >> base_log);
  const uint64_t carry = (((res - 1) | state) & res) >> (base_log - 1);
  state += carry;
  return (int64_t)(res - (carry << base_log));
}

static long checked = 0, bad = 0;

// the digits of one word as the kernels compute them; `listed` may be null
static void check(int B, int L, bool pre, uint64_t x, const int64_t* listed) {
  uint64_t want_state = init_native(pre ? closest(x, B, L) : x, B, L);
  uint64_t state = mi::core::decomp_init<uint64_t>(x, B, L, pre);
  const int nd = (B + 1 + 7) / 8;
  for (int l = 0; l < L; ++l) {
    const int64_t want = one_level(B, want_state);
    const int64_t got = (int64_t)mi::core::decomp_next<uint64_t>(B, state);
    uint64_t from_bytes = 0;  // sum_s e_s 256^s mod 2^64, as the GEMM's key rows shifted by 8 s recompose it
    for (int s = 0; s < nd; ++s)
      from_bytes += (uint64_t)(int64_t)mi::ks::signed_byte((uint64_t)got, s) << (8 * s);
    ++checked;
    if (got != want || (listed && got != listed[l]) || (int64_t)from_bytes != want) {
      if (bad++ < 20)
        printf("B=%d L=%d pre=%d x=%016" PRIx64 " level %d: want %" PRId64 " listed %" PRId64 " got %" PRId64
               " bytes %" PRId64 "\n", B, L, (int)pre, x, l, want, listed ? listed[l] : want, got, (int64_t)from_bytes);
    }
  }
}

int main() {
  int B, L, pre;
  uint64_t x;
  long listed_cases = 0;
  while (scanf("%d %d %d %" SCNx64, &B, &L, &pre, &x) == 4) {
    int64_t terms[64];
    if (B < 1 || L < 1 || B * L > 63) return 2;
    for (int l = 0; l < L; ++l)
      if (scanf("%" SCNd64, &terms[l]) != 1) return 2;
    check(B, L, pre != 0, x, terms);
    ++listed_cases;
  }
  std::mt19937_64 rng(11);
  for (B = 1; B <= 63; ++B) {
    const uint64_t half = 1ull << (63 - B);
    for (int p = 0; p < 2; ++p) {
      for (uint64_t c : {0ull, 1ull << 63}) {
        for (uint64_t d : {(uint64_t)0, (uint64_t)1, ~(uint64_t)0, half, half - 1, (uint64_t)0 - half,
                           (uint64_t)0 - half - 1, 2 * half, (uint64_t)0 - 2 * half})
          check(B, 1, p != 0, c + d, nullptr);
      }
      for (int i = 0; i < 2000; ++i) check(B, 1, p != 0, rng(), nullptr);
    }
  }
  printf("%ld listed cases, %ld digits checked, %ld mismatches\n", listed_cases, checked, bad);
  return bad ? 1 : 0;
}
