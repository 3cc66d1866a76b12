// ntt64_plan_tables.hpp — the host arithmetic of a prime64 plan as pure functions: every table and constant that
// plan_create (c_api_plan.cpp) uploads, in the layout and with the values the kernels read.  Host-only and
// header-only; no HIP runtime call, so tests/cpp/plan_tables_check.cpp pins the words without a GPU.
#pragma once
#include <cstddef>
#include <optional>
#include <vector>

#include "host_math.hpp"
#include "mi_arith.hpp"  // tower_exp
#include "ntt64_tw_tables.hpp"

namespace mi {
namespace host {

// ---- base tables (prime64.rs:159-204, 844) ---------------------------------------------------------------------

// prime64.rs:162-182: Solinas uses the hard-coded friendly root tower, other primes the Tonelli-Shanks root
// (`ts_root` = find_primitive_root64(p, 2 n), which the caller has checked first, as the reference does)
inline std::optional<u64> plan_root(size_t n, u64 p, u64 ts_root) {
  if (p == SOLINAS_P) return solinas_root(n);
  return ts_root;
}

struct BaseTables {
  std::vector<u64> twid, inv_twid;  // canonical host tables (reference layout)
  u64 n_inv = 0;
};

// the tables of the 2N-th root w for n = 2^logn
inline BaseTables base_tables(size_t n, u64 p, u64 w) {
  const int logn = __builtin_ctzll(n);
  BaseTables t;
  t.twid.assign(n, 0);
  t.inv_twid.assign(n, 0);
  u64 wk = 1;
  for (size_t k = 0; k < n; ++k) {  // prime64.rs:184-203
    t.twid[bit_rev(logn, k)] = wk;
    const unsigned inv_idx = bit_rev(logn, (n - k) % n);
    t.inv_twid[inv_idx] = (k == 0) ? wk : p - wk;
    wk = mul_mod(wk, w, p);
  }
  t.n_inv = exp_mod((u64)n, p - 2, p);  // prime64.rs:844
  return t;
}

// ---- device-form constants --------------------------------------------------------------------------------------

// the Montgomery constants of an odd p (R = 2^64): what mi::MontParams and the CRT constants (native_crt.hip) carry
struct MontConsts {
  u64 p = 0, pinv = 0, r1 = 0, r2 = 0;  // pinv = -p^-1 mod 2^64, r1 = R mod p, r2 = R^2 mod p
};

inline MontConsts mont_consts(u64 p) {
  u64 inv = p;  // Newton: p * inv == 1 mod 2^64
  for (int i = 0; i < 6; ++i) inv *= 2 - p * inv;
  MontConsts m;
  m.p = p;
  m.pinv = (u64)0 - inv;
  m.r1 = (u64)(((u128)1 << 64) % p);
  m.r2 = mul_mod(m.r1, m.r1, p);
  return m;
}

inline u64 mont_form(u64 x, u64 p) { return (u64)(((u128)x << 64) % p); }

// what the window kernels and the pointwise ops read: the Solinas plan the canonical tables and N^-1 (mont stays
// zero), every other prime its tables in Montgomery form with the ops' constants pre-scaled to match
struct DeviceForm {
  std::vector<u64> tw, itw;
  MontConsts mont;
  u64 c_normalize = 0, c_man = 0, c_macc = 0;  // device constants of the pointwise ops
};

inline DeviceForm device_form(const BaseTables& t, u64 p) {
  DeviceForm d;
  d.tw = t.twid;
  d.itw = t.inv_twid;
  if (p == SOLINAS_P) {
    d.c_normalize = t.n_inv;
    d.c_man = t.n_inv;
    d.c_macc = 0;
  } else {
    d.mont = mont_consts(p);
    for (size_t k = 0; k < d.tw.size(); ++k) {
      d.tw[k] = mont_form(d.tw[k], p);
      d.itw[k] = mont_form(d.itw[k], p);
    }
    d.c_normalize = mont_form(t.n_inv, p);
    d.c_man = mont_form(mont_form(t.n_inv, p), p);
    d.c_macc = d.mont.r2;
  }
  return d;
}

// ---- Shoup32 tables (mi_arith.hpp Shoup32) ----------------------------------------------------------------------

inline bool shoup32_applies(u64 p) { return p != SOLINAS_P && p < ((u64)1 << 32); }

// 2 N words, w | floor(w 2^32 / p) << 32, forward then inverse
inline std::vector<u64> shoup32_tables(const BaseTables& t, u64 p) {
  const size_t n = t.twid.size();
  std::vector<u64> t32(2 * n);
  for (size_t k = 0; k < n; ++k) {
    t32[k] = t.twid[k] | ((u64)(((u128)t.twid[k] << 32) / p) << 32);
    t32[n + k] = t.inv_twid[k] | ((u64)(((u128)t.inv_twid[k] << 32) / p) << 32);
  }
  return t32;
}

// ---- the twist table of the N = 2048 Solinas plan (ntt64_tw.hip, pbs_tw.hip) --------------------------------------

// The twisted factorisation needs the reference's first five stages to use power-of-two twiddles (the Solinas root
// tower, psi^64 = 8); check it against the tables it was built from.
inline bool twist_tower_ok(const BaseTables& t, u64 p) {
  for (int st = 0; st < 5; ++st)
    for (int g = 0; g < (1 << st); ++g)
      if (t.twid[(1u << st) + g] != exp_mod(2, (u64)tw::G1_FWD[st][g], p)) return false;
  return true;
}

// One table of 4 (n + 32) + 32 words, n = 2048: [fwd | inverse | inverse with N^-1 folded into the untwist rows | the
// inverse's last-DIT-stage twiddles (32) | fwd with N^-1 folded into the twist rows].  fwd and inverse hold
// rho_i^j and rho_i^-j at 64 i + j, then the 32 twiddles of the lane-pair stage.  The PBS / external-product bodies
// address the first three from one base (pbs_tw.hip), the standalone inverse its untwist rows and the fourth region,
// the normalising key conversion the last (ntt64_tw.hip).
inline std::vector<u64> twist_table(const BaseTables& t, u64 p) {
  const size_t n = t.twid.size(), region = n + 32;
  const u64 psi = t.twid[bit_rev(__builtin_ctzll(n), 1)];
  std::vector<u64> tab(4 * region + 32);
  u64* tf = tab.data();
  u64* ti = tf + region;
  u64* tn = tf + 2 * region;
  u64* tl = tf + 3 * region;
  u64* tfn = tl + 32;
  for (int g = 0; g < 32; ++g) {  // twiddles of the lane-pair stage (ntt64_tw.hip)
    tf[n + g] = exp_mod(2, (u64)tw::CYC_FWD[5][g], p);
    ti[n + g] = exp_mod(2, (u64)tw::CYC_INV[5][g], p);
  }
  for (unsigned i = 0; i < 32; ++i) {
    const u64 rho = exp_mod(psi, 2 * (u64)bit_rev(5, i) + 1, p);
    const u64 rho_inv = exp_mod(rho, p - 2, p);
    u64 f = 1, b = 1;
    for (unsigned j = 0; j < 64; ++j) {
      // the forward bodies' scale plan (ntt64_tw_tables.hpp, tools/tw_scale_plan.py): the five G1 stages leave
      // block i scaled by 2^TW_G1_OUT_SCALE[i], the cyclic stages take element j scaled by 2^TW_CYC_IN_SCALE[j >> 1]
      const int sc = (tw::TW_CYC_IN_SCALE[0][j >> 1] - tw::TW_G1_OUT_SCALE[0][i] + 192) % 192;
      tf[64 * i + j] = sc ? mul_mod(f, exp_mod(2, (u64)sc, p), p) : f;
      ti[64 * i + j] = b;
      f = mul_mod(f, rho, p);
      b = mul_mod(b, rho_inv, p);
    }
  }
  // the untwist rows times N^-1 (lane-pair twiddles unscaled)
  for (size_t e = 0; e < region; ++e) tn[e] = e < n ? mul_mod(ti[e], t.n_inv, p) : ti[e];
  // the standalone inverse's last DIT stage (joins j and j + 32 across a lane pair): entry m + 16 par is
  // 2^e with e = -3 (2 m + par) mod 192 = omega^-(2 m + par) (tools/gen_tw_kernel.py inv_last_exp)
  for (unsigned m = 0; m < 16; ++m)
    for (unsigned par = 0; par < 2; ++par)
      tl[m + 16 * par] = exp_mod(2, (u64)((192 - 3 * (2 * m + par) % 192) % 192), p);
  // the normalising key conversion's forward twist (lane-pair twiddles unscaled)
  for (size_t e = 0; e < region; ++e) tfn[e] = e < n ? mul_mod(tf[e], t.n_inv, p) : tf[e];
  return tab;
}

// ---- the block-twist table of the split transform (launch_ntt_split) ---------------------------------------------

// the top passes at stage 0 multiply by shifts (Goldilocks::mul_pow2): entries 1 .. 31 of both tables must be the
// powers of two tower_exp names
inline bool split_pow2_ok(const BaseTables& t, u64 p) {
  bool ok = true;
  for (int st = 0; st < 5; ++st)
    for (int g = 0; g < (1 << st); ++g) {
      const size_t i = ((size_t)1 << st) + g;
      ok = ok && t.twid[i] == exp_mod(2, (u64)tower_exp(true, st, g), p) &&
           t.inv_twid[i] == exp_mod(2, (u64)tower_exp(false, st, g), p);
    }
  return ok;
}

// the root tower psi_N^(N / 2048) = psi_2048 (prime64.rs:166-177); psi_2048 = the 2048 plan's twid[bitrev_11(1)]
inline bool split_root_ok(const BaseTables& t, u64 p, u64 psi_2048) {
  const size_t n = t.twid.size();
  const u64 psi = t.twid[bit_rev(__builtin_ctzll(n), 1)];
  return exp_mod(psi, (u64)(n / 2048), p) == psi_2048;
}

// 2 N words for N = 2^(11 + t): alpha_b^j at b 2048 + j, then alpha_b^-j at N + b 2048 + j
inline std::vector<u64> split_block_table(const BaseTables& tb, u64 p) {
  const size_t n = tb.twid.size();
  const int logn = __builtin_ctzll(n), t = logn - 11;
  const u64 psi = tb.twid[bit_rev(logn, 1)];
  std::vector<u64> blk(2 * n);
  for (size_t b = 0; b < ((size_t)1 << t); ++b) {
    // alpha_b = psi^(2 bitrev_t(b) + 1 - 2^t mod 2N)
    const u64 e = (2 * (u64)bit_rev(t, (unsigned)b) + 1 + 2 * (u64)n - ((u64)1 << t)) % (2 * (u64)n);
    const u64 a = exp_mod(psi, e, p), ai = exp_mod(a, p - 2, p);
    u64 f = 1, g = 1;
    for (size_t j = 0; j < 2048; ++j) {
      blk[b * 2048 + j] = f;
      blk[n + b * 2048 + j] = g;
      f = mul_mod(f, a, p);
      g = mul_mod(g, ai, p);
    }
  }
  return blk;
}

}  // namespace host
}  // namespace mi
