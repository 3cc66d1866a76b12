// carve.hpp — the one scratch block of each composite driver of the C ABI, described once: a struct of pointers whose
// carve() takes every array from a Carver in order.  carved_bytes<W>() runs it on no memory for the block's size and
// carve_on<W>() on the block for the pointers.  No HIP: tests/cpp/driver_layout_check.cpp checks every description.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mi {

// A bump allocator over a byte range; without a base it only counts.  take() first rounds the offset up to alignof(T).
struct Carver {
  char* base = nullptr;
  size_t bytes = 0;
  template <typename T>
  T* take(size_t count) {
    bytes = (bytes + alignof(T) - 1) / alignof(T) * alignof(T);
    T* p = base ? (T*)(base + bytes) : nullptr;
    bytes += count * sizeof(T);
    return p;
  }
};

template <typename W, typename... A>
W carve_on(void* base, const A&... shape) {
  Carver c{(char*)base};
  W w;
  w.carve(c, shape...);
  return w;
}
template <typename W, typename... A>
size_t carved_bytes(const A&... shape) {
  Carver c;
  W().carve(c, shape...);
  return c.bytes;
}

// mi_shortint_apply_lut_batch: keyswitched, switched (drift key only), gathered with its LUT indices (in_index only)
struct ApplyWork {
  uint64_t *ks, *sw, *gathered;
  uint32_t* eff;
  void carve(Carver& c, size_t n_in, size_t n_items, size_t small1, bool drift, bool indexed) {
    ks = c.take<uint64_t>(n_in * small1), sw = c.take<uint64_t>(drift ? n_in * small1 : 0);
    gathered = c.take<uint64_t>(indexed ? n_items * small1 : 0), eff = c.take<uint32_t>(indexed ? n_items : 0);
  }
};

// The index arrays of RadixStages (shortint_internal.hpp), as wide as the composite's widest stages: coeff 2 count
// (NULL unless it combines with coefficients), in_idx and lut_idx `items`, ia and ib `count`, pairs 2 count
struct StageIndex {
  int64_t* coeff = nullptr;
  uint32_t *in_idx = nullptr, *lut_idx = nullptr, *ia = nullptr, *ib = nullptr, *pairs = nullptr;
  void carve(Carver& c, size_t count, size_t items, bool weighted) {
    coeff = weighted ? c.take<int64_t>(2 * count) : nullptr;
    in_idx = c.take<uint32_t>(items), lut_idx = c.take<uint32_t>(items);
    ia = c.take<uint32_t>(count), ib = c.take<uint32_t>(count), pairs = c.take<uint32_t>(2 * count);
  }
};

// mi_radix_propagate_single_carry_batch on T blocks: work = msg[T] | st[T], one list of 2 T rows; pack / sum [T]
struct SingleCarryWork {
  uint64_t *work, *pack;
  StageIndex ix;
  void carve(Carver& c, size_t T, size_t big1) {
    work = c.take<uint64_t>(2 * T * big1), pack = c.take<uint64_t>(T * big1), ix.carve(c, T, 2 * T, true);
  }
};

// mi_radix_full_propagate_batch (both = msg[T] | carry[T], apply_items 2 T) and mi_radix_add_batch (lhs[T] | rhs[T], 0)
struct TwoListWork {
  uint64_t* both;
  StageIndex ix;
  void carve(Carver& c, size_t T, size_t big1, size_t apply_items) {
    both = c.take<uint64_t>(2 * T * big1), ix.carve(c, T, apply_items, false);
  }
};

// What a pass of the radix sum / multiplication holds per integer, in rows of big1 words and in u32 / pair entries
struct PassLayout {
  size_t list_len = 0;   // the initial columns: their rows, and the entries of a list
  size_t tail_rows = 0;  // rows after them: the rounds' outputs and chunk sums, or the staged operands and the pairs
  size_t sum_idx = 0, item_idx = 0, pack_idx = 0, gather_idx = 0, bytes = 0;  // bytes: of a pass of one integer
};

// A pass over I integers.  They share the two lists, so PassLayout::bytes (this at I = 1) times the integers of a pass
// over-counts 8 list_len bytes per further integer: deliberate here, mi_radix_{sum,mul}_pass_integers derive from it.
struct PassWork {
  uint64_t *pool, *tail;
  int64_t* pack_coeff;
  uint32_t *sum_idx, *in_idx, *lut_idx, *pack_idx, *gather_idx, *list[2];
  void carve(Carver& c, const PassLayout& p, size_t big1, size_t I) {
    pool = c.take<uint64_t>(p.list_len * I * big1), tail = c.take<uint64_t>(p.tail_rows * I * big1);
    pack_coeff = c.take<int64_t>(p.pack_idx * I), sum_idx = c.take<uint32_t>(p.sum_idx * I);
    in_idx = c.take<uint32_t>(p.item_idx * I), lut_idx = c.take<uint32_t>(p.item_idx * I);
    pack_idx = c.take<uint32_t>(p.pack_idx * I), gather_idx = c.take<uint32_t>(p.gather_idx * I);
    list[0] = c.take<uint32_t>(p.list_len), list[1] = c.take<uint32_t>(p.list_len);
  }
};

// from the schedule: initial slots, all slots, the most chunks and items of a round, s rows to a chunk, B columns
inline PassLayout pass_layout(size_t n_initial, size_t n_slots, size_t max_chunks, size_t max_items, size_t s, size_t B,
                              size_t big1, bool mul) {
  const auto most = [](size_t a, size_t b) { return a > b ? a : b; };
  const size_t pairs = mul ? B * (B + 1) / 2 : 0;
  PassLayout p;
  p.list_len = n_initial, p.pack_idx = 2 * pairs, p.gather_idx = mul ? 0 : n_initial;
  p.tail_rows = most((n_slots - n_initial) + max_chunks, mul ? pairs + 2 * B : 0);
  p.sum_idx = most(max_chunks, B) * s, p.item_idx = most(max_items, mul ? n_initial : 0);
  p.bytes = carved_bytes<PassWork>(p, big1, (size_t)1);
  return p;
}

// mi_fft64_extract_bits_batch: the running input, its shifted copy / the bootstrap's output, the keyswitched LWEs, acc
struct ExtractBitsWork {
  uint64_t *cur, *tmp, *ks, *acc;
  void carve(Carver& c, size_t batch, size_t big1, size_t small1, size_t per) {
    cur = c.take<uint64_t>(batch * big1), tmp = c.take<uint64_t>(batch * big1);
    ks = c.take<uint64_t>(batch * small1), acc = c.take<uint64_t>(per);
  }
};

// mi_fft64_circuit_bootstrap_boolean_batch on batch * lv items; ggsw_std only where the caller takes no standard GGSWs
struct CircuitBootstrapWork {
  uint64_t *shifted, *boot, *acc, *ggsw_std;
  uint32_t* idx;
  void carve(Carver& c, size_t batch, size_t lv, size_t small1, size_t big1, size_t per, size_t ggsw_words,
             bool std_out) {
    shifted = c.take<uint64_t>(batch * lv * small1), boot = c.take<uint64_t>(batch * lv * big1);
    acc = c.take<uint64_t>(lv * per), ggsw_std = c.take<uint64_t>(std_out ? 0 : batch * ggsw_words);
    idx = c.take<uint32_t>(batch * lv);
  }
};

}  // namespace mi
