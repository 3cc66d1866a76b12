// Host check of the NTT paths' digit stream (csrc/core_scalar.hpp: NttDigits<BNF>, the text pbs_kernels.hip and
// pbs_large.hip compile) against digits computed elsewhere.
// Input (stdin), one case per line: bnf base_log level word(hex) digit_0 .. digit_{level-1} (residues in [0, p),
// decimal, least significant level first; bnf 1 = the native word's SignedDecomposer, 0 = the word modulo p through
// SignedDecomposerNonNative).  Every digit must equal the listed one.
// Build: hipcc -O2 -x hip ntt_digits_check.cpp -o ntt_digits_check (host code only, no GPU needed).
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include "../../tfhe-rs-main_modified_amd/csrc/core_scalar.hpp"

static long checked = 0, bad = 0;

template <bool BNF>
static void check(int B, int L, uint64_t x, const uint64_t* listed) {
  mi::core::NttDigits<BNF> d;
  d.init(x, B, L);
  for (int l = 0; l < L; ++l) {
    const uint64_t got = d.next(B);
    ++checked;
    if (got != listed[l] && bad++ < 20)
      printf("bnf=%d B=%d L=%d x=%016" PRIx64 " level %d: listed %" PRIu64 " got %" PRIu64 "\n", (int)BNF, B, L, x, l,
             listed[l], got);
  }
}

int main() {
  int bnf, B, L;
  uint64_t x;
  long listed_cases = 0;
  while (scanf("%d %d %d %" SCNx64, &bnf, &B, &L, &x) == 4) {
    uint64_t digits[64];
    if (B < 1 || L < 1 || B * L > 63) return 2;
    for (int l = 0; l < L; ++l)
      if (scanf("%" SCNu64, &digits[l]) != 1) return 2;
    if (bnf) check<true>(B, L, x, digits);
    else check<false>(B, L, x, digits);
    ++listed_cases;
  }
  printf("%ld listed cases, %ld digits checked, %ld mismatches\n", listed_cases, checked, bad);
  return bad ? 1 : 0;
}
