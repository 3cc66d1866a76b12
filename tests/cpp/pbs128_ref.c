// pbs128_ref.c — a compiled twin of two loops of tests/pbs128_helpers.py, so that the 128-bit bootstrap tests compute
// their expected values in seconds at N = 2048: the signed decomposition of u128 words and the schoolbook negacyclic
// column sums of an external product, both in plain unsigned __int128 arithmetic (no transform, no limbs).  Test
// infrastructure only: tests/test_pbs128_oracle.py pins both functions to the Python-integer forms.
// Built by pbs128_helpers.accelerator(): cc -O2 -fopenmp -shared -fPIC.
#include <stdint.h>

typedef unsigned __int128 u128;
typedef __int128 i128;

// SignedDecomposer<u128>: init_decomposer_state (decomposer.rs:156-185), then decompose_one_level (iter.rs:131-151)
// `level` times; digits[li * count + i] = digit li (least significant level first) of words[2 i] | words[2 i + 1] << 64
void pbs128_decompose(int64_t* digits, const uint64_t* words, int64_t count, int base_log, int level, int threads) {
  const unsigned rep = (unsigned)(base_log * level);
#pragma omp parallel for num_threads(threads)
  for (int64_t i = 0; i < count; ++i) {
    const u128 input = (u128)words[2 * i] | ((u128)words[2 * i + 1] << 64);
    u128 res = input >> (128u - rep - 1u);
    const u128 rounding_bit = res & 1u;
    res += 1;
    res >>= 1;
    res &= ~(u128)0 >> (128u - rep);
    const u128 need_balance = (((res - 1) | (rounding_bit << (rep - 1))) & res) >> (rep - 1);
    u128 state = res - (need_balance << rep);
    const u128 mask = ((u128)1 << base_log) - 1;
    for (int li = 0; li < level; ++li) {
      const u128 r = state & mask;
      state = (u128)((i128)state >> base_log);
      const u128 carry = (((r - 1) | state) & r) >> (base_log - 1);
      state += carry;
      digits[(int64_t)li * count + i] = (int64_t)(uint64_t)(r - (carry << base_log));
    }
  }
}

// out[c][i] = sum_r sum_j digits[r][j] * ggsw[r][c][(i - j) mod n] (negated where j > i) mod 2^128: the k + 1 column
// polynomials of sum_r digits_r * ggsw_{r, c} in Z_{2^128}[X]/(X^n + 1).  digits: rows x n; ggsw: rows x kp1 x n x 2
// words; out: kp1 x n x 2 words.
void pbs128_column_sums(uint64_t* out, const int64_t* digits, const uint64_t* ggsw, int rows, int kp1, int n,
                        int threads) {
#pragma omp parallel for num_threads(threads) schedule(static)
  for (int t = 0; t < kp1 * n; ++t) {
    const int c = t / n, i = t % n;
    u128 acc = 0;
    for (int r = 0; r < rows; ++r) {
      const int64_t* d = digits + (int64_t)r * n;
      const uint64_t* g = ggsw + ((int64_t)r * kp1 + c) * n * 2;
      for (int j = 0; j <= i; ++j) {
        const int e = i - j;
        acc += (u128)(i128)d[j] * ((u128)g[2 * e] | ((u128)g[2 * e + 1] << 64));
      }
      for (int j = i + 1; j < n; ++j) {
        const int e = n + i - j;
        acc -= (u128)(i128)d[j] * ((u128)g[2 * e] | ((u128)g[2 * e + 1] << 64));
      }
    }
    out[2 * t] = (uint64_t)acc;
    out[2 * t + 1] = (uint64_t)(acc >> 64);
  }
}
