// Host check of the modular arithmetic of csrc/mi_arith.hpp (Goldilocks, Montgomery, Shoup32) against unsigned __int128,
// on the limb-corner operand grid of tests/arith_corners.py (restated here) plus random operands.  Next to each
// primitive its branch predicates are restated and the outcomes counted: the program fails when a result differs OR
// when an arm was never taken, unless the arm is listed below with the argument that makes it unreachable.
// Build: hipcc -O2 -x hip arith_check.cpp -o arith_check (host code only, no GPU needed).
//
// Unreachable arms (kept out of the "every arm taken" requirement):
//  * Montgomery::mul `ov1` and `t < s` for p < 2^63: REDC's u = (a b + m p) / 2^64 = thi + mhi + c is below
//    ((p - 1)^2 + (2^64 - 1) p) / 2^64 < 2 p <= 2^64, so neither 64-bit sum can wrap.
//  * Montgomery::mul `t >= p` for p < 2^32: u >= p needs m = 2^64 - k with 1 <= k < p, and a b + m p = 0 mod 2^64
//    gives a b = k p mod 2^64; both sides are below p^2 < 2^64, so a b = k p, p | a b, hence a b = 0 and k = 0.
//  * For p > 2^63 the `t < s` arm (thi + mhi = 2^64 - 1 and c = 1, i.e. u = 2^64 exactly) IS reachable and is
//    reached by construction: for a < p, m = 2^128 p^-1 mod a and b = (2^128 - m p) / a solve a b + m p = 2^128.
//  * Shoup32::mul `r == p` for canonical x: r = x w - q p = p needs x w = 0 mod p with 0 < x, w < p.  The product's
//    stated domain is any x < 2^32, where x = p reaches it, so the arm is required on that domain.
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../tfhe-rs-main_modified_amd/csrc/mi_arith.hpp"

typedef unsigned __int128 u128;
typedef uint64_t u64;
typedef uint32_t u32;
using mi::Goldilocks;

static const u64 P = mi::GL_P, EPS = mi::GL_EPS;
static long checked = 0, bad = 0;
static std::map<std::string, long> arms;            // arm name -> times taken (insertion as "required")
static std::map<std::string, const char*> excused;  // arm name -> unreachability argument

static void need(const std::string& arm) { arms.emplace(arm, 0); }
static void hit(const std::string& arm) { ++arms[arm]; }
static void excuse(const std::string& arm, const char* why) { arms.emplace(arm, 0); excused[arm] = why; }

static void expect(bool ok, const char* what, u64 a, u64 b, u64 got, u64 want) {
  ++checked;
  if (!ok && bad++ < 20)
    printf("MISMATCH %s a=%016llx b=%016llx got=%016llx want=%016llx\n", what, (unsigned long long)a,
           (unsigned long long)b, (unsigned long long)got, (unsigned long long)want);
}

// tests/arith_corners.py values(p)
static std::vector<u64> values(u64 p) {
  const bool small = p < (1ull << 32);
  const u64 l32[7] = {0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF};
  const u64 l16[7] = {0, 1, 2, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF};
  const u64* l = small ? l16 : l32;
  const int half = small ? 16 : 32;
  std::vector<u64> base, out;
  for (int h = 0; h < 7; ++h)
    for (int k = 0; k < 7; ++k) base.push_back(((l[h] << half) | l[k]) % p);
  const size_t nb = base.size();
  for (size_t i = 0; i < nb; ++i) base.push_back((p - base[i]) % p);
  for (u64 v : base) {
    bool seen = false;
    for (u64 w : out) seen |= w == v;
    if (!seen) out.push_back(v);
  }
  return out;
}

static u64 pow_mod(u64 b, u64 e, u64 p) {
  u64 r = 1 % p;
  for (b %= p; e; e >>= 1, b = (u64)((u128)b * b % p))
    if (e & 1) r = (u64)((u128)r * b % p);
  return r;
}

// ---- Goldilocks ---------------------------------------------------------------------------------------------------
static void gl_add(u64 a, u64 b) {
  const u64 s = a + b;
  hit(s < a ? "gl.add carry" : s >= P ? "gl.add >=P without carry" : "gl.add plain");
  const u64 want = (u64)(((u128)a + b) % P);
  expect(Goldilocks::add(a, b) == want, "gl.add", a, b, Goldilocks::add(a, b), want);
}
static void gl_sub(u64 a, u64 b) {
  hit(a < b ? "gl.sub borrow" : "gl.sub plain");
  const u64 want = (u64)(((u128)a + P - b) % P);
  expect(Goldilocks::sub(a, b) == want, "gl.sub", a, b, Goldilocks::sub(a, b), want);
}
static void gl_reduce(u64 lo, u64 hi, const char* who) {
  const u64 hh = hi >> 32, hl = hi & EPS;
  u64 t0 = lo - hh;
  const bool borrow = lo < hh;
  if (borrow) t0 -= EPS;
  const u64 t1 = (hl << 32) - hl, r = t0 + t1;
  hit(borrow ? "gl.reduce128 borrow" : "gl.reduce128 no borrow");
  hit(r < t1 ? "gl.reduce128 carry" : r >= P ? "gl.reduce128 >=P without carry" : "gl.reduce128 plain");
  const u64 want = (u64)((((u128)hi << 64) | lo) % P);
  expect(Goldilocks::reduce128(lo, hi) == want, who, lo, hi, Goldilocks::reduce128(lo, hi), want);
}
static void gl_mul(u64 a, u64 b) {
  const u128 t = (u128)a * b;
  u64 lo, hi;
  mi::mul64x64(a, b, lo, hi);
  expect(lo == (u64)t && hi == (u64)(t >> 64), "mul64x64", a, b, hi, (u64)(t >> 64));
  gl_reduce((u64)t, (u64)(t >> 64), "gl.reduce128(mul)");
  const u64 want = (u64)(t % P);
  expect(Goldilocks::mul(a, b) == want, "gl.mul", a, b, Goldilocks::mul(a, b), want);
}
static void gl_lazy(u64 a, u64 t) {  // a: any 64-bit word, t canonical
  const u128 s = (u128)a + t;
  hit((s >> 64) ? "gl.add_lazy carry" : "gl.add_lazy plain");
  const u64 ga = Goldilocks::add_lazy(a, t);
  // congruent, and the folded carry did not wrap a second time: the value is a + t (- 2^64 + EPS)
  expect((u128)ga == ((s >> 64) ? s - ((u128)1 << 64) + EPS : s), "gl.add_lazy", a, t, ga, (u64)(s % P));
  hit(a < t ? "gl.sub_lazy borrow" : "gl.sub_lazy plain");
  const u64 gs = Goldilocks::sub_lazy(a, t);
  const u128 d = a < t ? (u128)a + ((u128)1 << 64) - t - EPS : (u128)a - t;
  expect((u128)gs == d && gs % P == (u64)(((u128)a + P - t) % P), "gl.sub_lazy", a, t, gs, (u64)d);
  hit(a >= P ? "gl.canon >=P" : "gl.canon plain");
  expect(Goldilocks::canon(a) == a % P, "gl.canon", a, 0, Goldilocks::canon(a), a % P);
}
static void gl_pow2(u64 x, int e) {  // x: any 64-bit word
  const bool neg = e >= 96;
  const int f = neg ? e - 96 : e;
  hit(neg ? "gl.mul_pow2 negative" : "gl.mul_pow2 positive");
  if (f == 0) hit(x >= P ? "gl.mul_pow2 f=0 x>=P" : "gl.mul_pow2 f=0 plain");
  else if (f < 64) hit("gl.mul_pow2 f<64");
  else hit(f == 64 ? "gl.mul_pow2 f=64" : "gl.mul_pow2 f>64");
  bool ng = !neg;
  const u64 t = Goldilocks::mul_pow2(x, e, ng);
  const u64 full = (u64)((u128)(x % P) * pow_mod(2, (u64)e, P) % P);
  const u64 want = neg ? (P - full) % P : full;  // x 2^e = neg ? -t : t
  expect(t == want && ng == neg, "gl.mul_pow2", x, (u64)e, t, want);
}

static void goldilocks(std::mt19937_64& rng) {
  for (const char* a : {"gl.add carry", "gl.add >=P without carry", "gl.add plain", "gl.sub borrow", "gl.sub plain",
                        "gl.reduce128 borrow", "gl.reduce128 no borrow", "gl.reduce128 carry",
                        "gl.reduce128 >=P without carry", "gl.reduce128 plain", "gl.add_lazy carry", "gl.add_lazy plain",
                        "gl.sub_lazy borrow", "gl.sub_lazy plain", "gl.canon >=P", "gl.canon plain",
                        "gl.mul_pow2 negative", "gl.mul_pow2 positive", "gl.mul_pow2 f=0 x>=P", "gl.mul_pow2 f=0 plain",
                        "gl.mul_pow2 f<64", "gl.mul_pow2 f=64", "gl.mul_pow2 f>64"})
    need(a);
  const std::vector<u64> v = values(P);
  if (v.size() != 73) { printf("values(P): %zu, expected 73\n", v.size()); ++bad; }
  // non-canonical first operands of the lazy forms: every limb-corner word up to 2^64 - 1
  std::vector<u64> words;
  const u64 l32[7] = {0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF};
  for (u64 h : l32)
    for (u64 l : l32) words.push_back((h << 32) | l);
  words.push_back(P);
  words.push_back(P + 1);
  for (u64 a : v)
    for (u64 b : v) {
      gl_add(a, b);
      gl_sub(a, b);
      gl_mul(a, b);
    }
  for (u64 a : words)
    for (u64 t : v) gl_lazy(a, t);
  for (u64 lo : words)  // every 128-bit limb-corner value through the reduction on its own
    for (u64 hi : words) gl_reduce(lo, hi, "gl.reduce128");
  for (int e = 0; e < 192; ++e) {
    for (u64 x : v) gl_pow2(x, e);
    for (u64 x : words) gl_pow2(x, e);
    for (int i = 0; i < 8; ++i) gl_pow2(rng(), e);
  }
  for (int i = 0; i < 4000; ++i) {
    const u64 a = rng() % P, b = rng() % P, w = rng();
    gl_add(a, b);
    gl_sub(a, b);
    gl_mul(a, b);
    gl_lazy(w, b);
    gl_reduce(rng(), w, "gl.reduce128");
  }
}

// ---- Montgomery ---------------------------------------------------------------------------------------------------
static u64 neg_inv64(u64 p) {  // -p^-1 mod 2^64 (Newton)
  u64 x = p;
  for (int i = 0; i < 6; ++i) x *= 2 - p * x;
  return (u64)0 - x;
}
static u64 inv_mod(u64 a, u64 m) {  // a^-1 mod m, gcd(a, m) = 1 (extended Euclid on signed 128-bit)
  __int128 r0 = m, r1 = a % m, s0 = 0, s1 = 1;
  while (r1) {
    const __int128 q = r0 / r1, r2 = r0 - q * r1, s2 = s0 - q * s1;
    r0 = r1; r1 = r2; s0 = s1; s1 = s2;
  }
  return (u64)((s0 % (__int128)m + m) % m);
}

static void mont_one(const mi::Montgomery& M, const std::string& tag, u64 a, u64 b) {
  const u64 p = M.p;
  const u128 T = (u128)a * b;
  const u64 tlo = (u64)T, thi = (u64)(T >> 64), m = tlo * M.pinv, mhi = (u64)(((u128)m * p) >> 64);
  const u64 s = thi + mhi, t = s + (tlo != 0);
  hit(tag + (s < thi ? " mul ov1" : t < s ? " mul t<s" : t >= p ? " mul t>=p" : " mul plain"));
  const u64 got = M.mul(a, b);
  // got R = a b (mod p), canonical
  expect(got < p && (u64)((((u128)got) << 64) % p) == (u64)(T % p), "mont.mul", a, b, got, p);
  hit(tag + (a >= p - b ? " add wrap" : " add plain"));
  expect(M.add(a, b) == (u64)(((u128)a + b) % p), "mont.add", a, b, M.add(a, b), p);
  hit(tag + (a >= b ? " sub plain" : " sub borrow"));
  expect(M.sub(a, b) == (u64)(((u128)a + p - b) % p), "mont.sub", a, b, M.sub(a, b), p);
}

static void montgomery(u64 p, const char* name, std::mt19937_64& rng) {
  const std::string tag = std::string("mont.") + name;
  const u64 r1 = (u64)((((u128)1) << 64) % p);
  const mi::Montgomery M{p, neg_inv64(p), (u64)((u128)r1 * r1 % p)};
  for (const char* a : {" mul plain", " add wrap", " add plain", " sub plain", " sub borrow"}) need(tag + a);
  if (p >> 32) need(tag + " mul t>=p");
  else
    excuse(tag + " mul t>=p", "p < 2^32: u >= p needs m = 2^64 - k, 1 <= k < p, and a b = k p mod 2^64; both sides are "
                              "below p^2 < 2^64, so a b = k p, p | a b, a b = 0, k = 0");
  if (p >> 63) {
    need(tag + " mul ov1");
    need(tag + " mul t<s");
  } else {
    const char* why = "p < 2^63: u = (a b + m p) / 2^64 < 2 p <= 2^64, no 64-bit sum of REDC wraps";
    excuse(tag + " mul ov1", why);
    excuse(tag + " mul t<s", why);
  }
  const std::vector<u64> v = values(p);
  for (u64 a : v)
    for (u64 b : v) mont_one(M, tag, a, b);
  if (p >> 63) {  // a b + m p = 2^128: the t < s arm
    const u64 as[6] = {p - 1, p - 2, (1ull << 63) + 1, P % p, p - 0x10001, (p >> 1) | (1ull << 63)};
    for (u64 a : as) {
      const u64 two64 = (u64)((((u128)1) << 64) % a), two128 = (u64)((u128)two64 * two64 % a);
      const u64 m = (u64)((u128)two128 * inv_mod(p % a, a) % a);
      const u128 T = (u128)0 - (u128)m * p;  // 2^128 - m p (mod 2^128)
      if (m == 0 || T % a) continue;
      const u128 b = T / a;
      if (b < p) mont_one(M, tag, a, (u64)b);
    }
  }
  for (int i = 0; i < 3000; ++i) mont_one(M, tag, rng() % p, rng() % p);
}

// ---- Shoup32 ------------------------------------------------------------------------------------------------------
static void shoup_mul(const mi::Shoup32& S, const std::string& tag, u64 x, u64 w) {
  const u64 p = S.p, wq = (w << 32) / p, q = (x * wq) >> 32, r = x * w - q * p;
  hit(tag + (r == p ? " mul r==p" : r > p ? " mul r>p" : " mul plain"));
  const u64 got = S.mul(x, w | (wq << 32));
  expect(got == x * w % p, "shoup.mul", x, w, got, x * w % p);
}
static void shoup32(u32 p, std::mt19937_64& rng) {
  const std::string tag = "shoup." + std::to_string(p);
  const mi::Shoup32 S{p};
  for (const char* a : {" mul r==p", " mul r>p", " mul plain", " add wrap", " add plain", " sub plain", " sub borrow"})
    need(tag + a);
  std::vector<u64> v = values(p), xs = v;
  // the product's domain is any x < 2^32 (its bound r < 2 p does not need x < p): the words at and above p
  for (u64 x : {(u64)p, (u64)p + 1, 2 * (u64)p, 2 * (u64)p - 1, (u64)0xFFFFFFFF, (u64)0xFFFFFFFE, (u64)0x80000000})
    if (x <= 0xFFFFFFFFull) xs.push_back(x);
  for (u64 w : v) {
    for (u64 x : xs) shoup_mul(S, tag, x, w);
    for (u64 a : v) {
      hit(tag + (a >= p - w ? " add wrap" : " add plain"));
      expect(S.add(a, w) == (a + w) % p, "shoup.add", a, w, S.add(a, w), (a + w) % p);
      hit(tag + (a >= w ? " sub plain" : " sub borrow"));
      expect(S.sub(a, w) == (a + p - w) % p, "shoup.sub", a, w, S.sub(a, w), (a + p - w) % p);
    }
  }
  for (int i = 0; i < 3000; ++i) shoup_mul(S, tag, (u32)rng(), rng() % p);
}

int main() {
  std::mt19937_64 rng(0x61726974);
  goldilocks(rng);
  // the primes of tests/test_ntt_gpu.py (_primes) and tests/test_native_gpu.py (_primes32); printed for the pytest,
  // which compares them with the oracle's
  const u64 p64[] = {0xffffffffffe40001ull, 0x7fffffffffef0001ull, 0x3fffffffffff0001ull, 0x3ffffffdf0001ull, 1062862849ull};
  const char* n64[] = {"p64", "p63", "p62", "p50", "p30"};
  for (int i = 0; i < 5; ++i) {
    printf("montgomery %s %llu\n", n64[i], (unsigned long long)p64[i]);
    montgomery(p64[i], n64[i], rng);
  }
  for (u32 p : {1062862849u, 1073479681u, 0x7ffe0001u, 0xfff00001u}) {
    printf("shoup32 %u\n", p);
    shoup32(p, rng);
  }
  long untaken = 0;
  for (const auto& kv : arms) {
    const auto ex = excused.find(kv.first);
    if (ex != excused.end()) {
      if (kv.second) { printf("EXCUSED ARM TAKEN %s (%ld): %s\n", kv.first.c_str(), kv.second, ex->second); ++untaken; }
      continue;
    }
    printf("arm %-40s %ld\n", kv.first.c_str(), kv.second);
    if (!kv.second) { printf("ARM NEVER TAKEN %s\n", kv.first.c_str()); ++untaken; }
  }
  printf("%ld checked, %ld mismatches, %ld arms untaken\n", checked, bad, untaken);
  return bad || untaken ? 1 : 0;
}
