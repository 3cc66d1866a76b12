// Host check of csrc/carve.hpp: the carver and the workspace description of every composite driver.  For each
// description the counting pass must equal the closed form the driver allocated before the carver existed (written out
// here on plain numbers), and on a heap block of exactly that size every carved array must be aligned to its type, lie
// in order, be disjoint from the others and take a sentinel in its first and its last element (built with
// -fsanitize=address,undefined: one element past the block is a report).  Prints "driver layouts: N cases, 0 failures".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "carve.hpp"

namespace {

int g_cases = 0, g_failures = 0;

void expect(bool ok, const char* what, size_t a = 0, size_t b = 0) {
  if (ok) return;
  ++g_failures;
  printf("FAIL %s (%zu, %zu)\n", what, a, b);
}

struct Span {
  void* p;
  size_t count, size, align;
};
template <typename T>
Span span(T* p, size_t count) {
  return {(void*)p, count, sizeof(T), alignof(T)};
}

// the arrays of a workspace carved on `base`, in the order of the description, fill `bytes` exactly
void walk(const char* name, char* base, size_t bytes, const std::vector<Span>& spans) {
  size_t end = 0;
  for (const Span& s : spans) {
    const size_t off = (size_t)((char*)s.p - base);
    expect((uintptr_t)s.p % s.align == 0, name, off, s.align);
    expect(off >= end, name, off, end);  // in order and disjoint
    end = off + s.count * s.size;
    expect(end <= bytes, name, end, bytes);
    if (s.count == 0) continue;
    for (size_t e : {(size_t)0, s.count - 1})
      for (size_t i = 0; i < s.size; ++i) ((volatile unsigned char*)s.p)[e * s.size + i] = 0xA5;
  }
  expect(end == bytes, name, end, bytes);
}

template <typename W, typename Spans, typename... A>
void check(const char* name, size_t want_bytes, Spans spans_of, const A&... shape) {
  ++g_cases;
  const size_t bytes = mi::carved_bytes<W>(shape...);
  expect(bytes == want_bytes, name, bytes, want_bytes);
  char* block = (char*)malloc(bytes ? bytes : 1);
  const W w = mi::carve_on<W>(block, shape...);
  walk(name, block, bytes, spans_of(w));
  free(block);
}

// the rounds of the sum schedule on column lengths: s rows fill a chunk, a chunk gives a message to its column and a
// carry to the next (none out of the last)
struct Sched {
  size_t n_initial = 0, n_slots = 0, max_chunks = 0, max_items = 0, s = 0, B = 0;
};
Sched schedule(std::vector<size_t> len, size_t m, size_t c) {
  Sched sc;
  sc.s = (m * c - 1) / (m - 1), sc.B = len.size();
  for (size_t l : len) sc.n_initial += l;
  sc.n_slots = sc.n_initial;
  while (std::any_of(len.begin(), len.end(), [&](size_t l) { return l > sc.s; })) {
    size_t chunks = 0, items = 0, below = 0;
    for (size_t& l : len) {
      const size_t q = l >= sc.s ? l / sc.s : 0;
      l = l - q * sc.s + below + q;
      chunks += q, items += below + q, below = q;
    }
    sc.n_slots += items;
    sc.max_chunks = std::max(sc.max_chunks, chunks), sc.max_items = std::max(sc.max_items, items);
  }
  return sc;
}
std::vector<size_t> mul_columns(size_t B, size_t m) {
  std::vector<size_t> len(B);
  for (size_t b = 0; b < B; ++b) len[b] = m > 2 ? 2 * b + 1 : b + 1;
  return len;
}

// the per-integer byte count of a pass as the drivers computed it before the carver
size_t pass_bytes(const Sched& sc, size_t big1, bool mul) {
  const size_t B = sc.B, pairs = mul ? B * (B + 1) / 2 : 0;
  const size_t tail_rows = std::max<size_t>((sc.n_slots - sc.n_initial) + sc.max_chunks, mul ? pairs + 2 * B : 0);
  const size_t rows = sc.n_initial + tail_rows;
  const size_t sum_idx = std::max<size_t>(sc.max_chunks, B) * sc.s;
  const size_t item_idx = std::max<size_t>(sc.max_items, mul ? sc.n_initial : 0);
  const size_t list_len = sc.n_initial, pack_idx = 2 * pairs, gather_idx = mul ? 0 : sc.n_initial;
  return rows * big1 * sizeof(uint64_t) + pack_idx * sizeof(int64_t) +
         (sum_idx + 2 * item_idx + pack_idx + gather_idx + 2 * list_len) * sizeof(uint32_t);
}

void check_pass(const char* name, const Sched& sc, size_t big1, bool mul) {
  const mi::PassLayout p =
      mi::pass_layout(sc.n_initial, sc.n_slots, sc.max_chunks, sc.max_items, sc.s, sc.B, big1, mul);
  expect(p.bytes == pass_bytes(sc, big1, mul), name, p.bytes, pass_bytes(sc, big1, mul));
  for (size_t I : {(size_t)1, (size_t)3}) {
    // the block of a pass is bytes * I: the lists are counted once per integer and carved once
    const size_t want = pass_bytes(sc, big1, mul) * I - (I - 1) * 2 * sc.n_initial * sizeof(uint32_t);
    check<mi::PassWork>(
        name, want,
        [&](const mi::PassWork& w) {
          return std::vector<Span>{span(w.pool, sc.n_initial * I * big1), span(w.tail, p.tail_rows * I * big1),
                                   span(w.pack_coeff, p.pack_idx * I),   span(w.sum_idx, p.sum_idx * I),
                                   span(w.in_idx, p.item_idx * I),       span(w.lut_idx, p.item_idx * I),
                                   span(w.pack_idx, p.pack_idx * I),     span(w.gather_idx, p.gather_idx * I),
                                   span(w.list[0], p.list_len),          span(w.list[1], p.list_len)};
        },
        p, big1, I);
    expect(want <= p.bytes * I, name, want, p.bytes * I);
  }
}

}  // namespace

int main() {
  for (size_t T : {1, 2, 5, 96}) {
    for (size_t big1 : {2, 1025, 2049}) {
      check<mi::SingleCarryWork>(
          "single carry", 3 * T * big1 * 8 + 2 * T * 8 + 8 * T * 4,
          [&](const mi::SingleCarryWork& w) {
            return std::vector<Span>{span(w.work, 2 * T * big1), span(w.pack, T * big1),   span(w.ix.coeff, 2 * T),
                                     span(w.ix.in_idx, 2 * T),   span(w.ix.lut_idx, 2 * T), span(w.ix.ia, T),
                                     span(w.ix.ib, T),           span(w.ix.pairs, 2 * T)};
          },
          T, big1);
      // full propagate applies on 2 T items, add on none; neither combines with coefficients
      for (size_t items : {2 * T, (size_t)0})
        check<mi::TwoListWork>(
            items ? "full propagate" : "add", 2 * T * big1 * 8 + (items ? 8 : 4) * T * 4,
            [&](const mi::TwoListWork& w) {
              expect(w.ix.coeff == nullptr, "no coefficients without a weighted stage");
              return std::vector<Span>{span(w.both, 2 * T * big1), span(w.ix.in_idx, items), span(w.ix.lut_idx, items),
                                       span(w.ix.ia, T),           span(w.ix.ib, T),         span(w.ix.pairs, 2 * T)};
            },
            T, big1, items);
      // the apply: T inputs of small1 = big1 words, n_items of {T, 2 T + 1}
      for (size_t n_items : {T, 2 * T + 1})
        for (bool drift : {false, true})
          for (bool indexed : {false, true}) {
            const size_t small1 = big1, rows = T * (drift ? 2 : 1) + (indexed ? n_items : 0);
            check<mi::ApplyWork>(
                "apply", rows * small1 * 8 + (indexed ? n_items * 4 : 0),
                [&](const mi::ApplyWork& w) {
                  return std::vector<Span>{span(w.ks, T * small1), span(w.sw, drift ? T * small1 : 0),
                                           span(w.gathered, indexed ? n_items * small1 : 0),
                                           span(w.eff, indexed ? n_items : 0)};
                },
                T, n_items, small1, drift, indexed);
          }
      // extract bits and the circuit bootstrap: batch = T, a small LWE of 7 + 1 words, a GLWE of `per` words
      const size_t batch = T, small1 = 8, per = 2 * 16;
      check<mi::ExtractBitsWork>(
          "extract bits", (batch * (2 * big1 + small1) + per) * 8,
          [&](const mi::ExtractBitsWork& w) {
            return std::vector<Span>{span(w.cur, batch * big1), span(w.tmp, batch * big1), span(w.ks, batch * small1),
                                     span(w.acc, per)};
          },
          batch, big1, small1, per);
      for (size_t lv : {1, 3})
        for (bool std_out : {false, true}) {
          const size_t items = batch * lv, ggsw_words = lv * 2 * 2 * 16;
          check<mi::CircuitBootstrapWork>(
              "circuit bootstrap",
              (items * (small1 + big1) + lv * per + (std_out ? 0 : batch * ggsw_words)) * 8 + items * 4,
              [&](const mi::CircuitBootstrapWork& w) {
                return std::vector<Span>{span(w.shifted, items * small1), span(w.boot, items * big1),
                                         span(w.acc, lv * per), span(w.ggsw_std, std_out ? 0 : batch * ggsw_words),
                                         span(w.idx, items)};
              },
              batch, lv, small1, big1, per, ggsw_words, std_out);
        }
    }
  }

  // the sum and mul passes: B = 2 and B = 32 at m = c = 4, B = 5 at m = c = 2 (no msb rows), a sum of 13 terms
  for (size_t big1 : {2, 2049}) {
    check_pass("mul pass B 2 (4, 4)", schedule(mul_columns(2, 4), 4, 4), big1, true);
    check_pass("mul pass B 32 (4, 4)", schedule(mul_columns(32, 4), 4, 4), big1, true);
    check_pass("mul pass B 5 (2, 2)", schedule(mul_columns(5, 2), 2, 2), big1, true);
    check_pass("sum pass B 2 (4, 4)", schedule({13, 13}, 4, 4), big1, false);
    check_pass("sum pass B 32 (4, 4)", schedule(std::vector<size_t>(32, 13), 4, 4), big1, false);
    check_pass("sum pass B 3 (2, 2)", schedule({13, 9, 4}, 2, 2), big1, false);
  }

  // a mis-ordered description: the u64 after three u32 starts at the next multiple of 8
  {
    ++g_cases;
    mi::Carver count;
    count.take<uint32_t>(3);
    count.take<uint64_t>(1);
    expect(count.bytes == 24, "mis-ordered total", count.bytes, 24);
    char* block = (char*)malloc(count.bytes);
    mi::Carver c{block};
    uint32_t* a = c.take<uint32_t>(3);
    uint64_t* b = c.take<uint64_t>(1);
    expect((char*)a == block && (char*)b == block + 16 && (uintptr_t)b % 8 == 0, "mis-ordered pointers");
    a[0] = a[2] = 1, *b = 2;
    expect(c.bytes == 24, "mis-ordered carve", c.bytes, 24);
    free(block);
  }

  printf("driver layouts: %d cases, %d failures\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
