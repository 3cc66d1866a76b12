// plan_tables_check.cpp — dumps the host tables of a prime64 plan (csrc/ntt64_plan_tables.hpp: what plan_create
// uploads) for tests/test_plan_tables_host.py, which compares every word against restatements in Python.  Host only:
//   hipcc -O2 -x hip plan_tables_check.cpp -o plan_tables_check && ./plan_tables_check N P OUT
// OUT is a sequence of sections, each an 8-byte name (zero padded), a u64 word count and that many little-endian u64
// words.  A section is written only where plan_create would build its table.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tfhe-rs-main_modified_amd/csrc/ntt64_plan_tables.hpp"

using namespace mi::host;

static FILE* out;

static void section(const char* name, const u64* words, size_t count) {
  char tag[8] = {};
  std::strncpy(tag, name, 8);
  const u64 c = count;
  std::fwrite(tag, 1, 8, out);
  std::fwrite(&c, 8, 1, out);
  std::fwrite(words, 8, count, out);
}
static void section(const char* name, const std::vector<u64>& v) { section(name, v.data(), v.size()); }
static void flag(const char* name, bool b) {
  const u64 w = b;
  section(name, &w, 1);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const size_t n = std::strtoull(argv[1], nullptr, 10);
  const u64 p = std::strtoull(argv[2], nullptr, 10);
  if (n < 16 || (n & (n - 1)) != 0 || !is_prime64(p)) return 3;
  const auto ts_root = find_primitive_root64(p, 2 * (u64)n);
  if (!ts_root) return 3;
  const auto w = plan_root(n, p, *ts_root);
  if (!w) return 3;
  out = std::fopen(argv[3], "wb");
  if (!out) return 4;
  const bool solinas = p == SOLINAS_P;
  const int logn = __builtin_ctzll(n);

  const BaseTables t = base_tables(n, p, *w);
  section("twid", t.twid);
  section("inv_twid", t.inv_twid);
  section("n_inv", &t.n_inv, 1);

  const DeviceForm d = device_form(t, p);
  const u64 mont[4] = {d.mont.p, d.mont.pinv, d.mont.r1, d.mont.r2};
  const u64 consts[3] = {d.c_normalize, d.c_man, d.c_macc};
  section("mont", mont, 4);
  section("dev_tw", d.tw);
  section("dev_itw", d.itw);
  section("consts", consts, 3);
  if (!solinas) {  // mont_form itself, as mi_native_plan_create calls it
    std::vector<u64> m(t.twid);
    for (u64& x : m) x = mont_form(x, p);
    section("montform", m);
  }

  if (shoup32_applies(p)) section("shoup32", shoup32_tables(t, p));

  if (solinas && n == 2048) {
    flag("tower_ok", twist_tower_ok(t, p));
    section("twist", twist_table(t, p));
  }
  if (solinas && logn >= 12) {
    const BaseTables sub = base_tables(2048, p, *solinas_root(2048));
    flag("pow2_ok", split_pow2_ok(t, p));
    flag("root_ok", split_root_ok(t, p, sub.twid[bit_rev(11, 1)]));
    section("blk", split_block_table(t, p));
    BaseTables bad = t;  // the negative case: entry 1 is stage 0's twiddle 2^48
    bad.twid[1] ^= 1;
    flag("pow2_bad", split_pow2_ok(bad, p));
  }
  return std::fclose(out) == 0 ? 0 : 4;
}
