// c_api_radix_mul.cpp — the radix sum of ciphertexts and the radix multiplication of the C ABI.  Reference paths
// relative to tfhe/src/integer/server_key/radix_parallel:
//   unchecked_partial_sum_ciphertexts_vec_parallelized   sum.rs:14-147
//   unchecked_sum_ciphertexts_vec_parallelized           sum.rs:155-166
//   compute_terms_for_mul_low                            mul.rs:333-400
//   unchecked_mul_assign_parallelized / mul_parallelized mul.rs:437-460, :599-608
//   max_sum_size                                         shortint/server_key/mod.rs
//
// Both calls are fixed sequences of public calls (LC = mi_lwe_linear_combination_batch, APPLY =
// mi_shortint_apply_lut_batch, as in c_api_shortint.cpp) and equal them bit for bit.  The time is in the keyswitches and
// bootstraps of APPLY and, far behind, in the row sums of LC; the kernels of radix_sum_index.hip only write the index
// arrays on the device, from descriptors passed by value (nothing is copied from the host, nothing synchronises).
//
// The schedule (mi_radix_sum_schedule) is data-independent: s = (m c - 1) / (m - 1) rows of value <= m - 1 fill a block.
// Column b starts as block b of every term that lives there, in term order.  While some column has more than s rows,
// a round: every column of >= s rows gives len / s chunks of its first rows; a chunk's sum gives its message to its
// own column and its carry to the next (none out of the last column); the next list of a column is its len % s rows
// left, the carries of the column below in chunk order, its own messages in chunk order.
//
// A pass works on I integers (all of them unless the scratch cap cuts the batch) in one scratch block: the pool of
// block rows, slot v of integer i at row v I + i, the first slots being the initial columns, column-major; every
// round's outputs take the next n_items slots.
//
//   mi_radix_sum_batch (n_terms = 0: LC with no terms writes trivial zeros, done):
//     1. LC     pool[slot of (t, b)] = terms[t, i, b], one term, for b >= first_block[t]    (the gather; rows below
//               first_block are not read)
//     2. per round:
//          LC     sums[chunk I + i] = the s pool rows of the chunk, coefficients 1
//          APPLY  pool[out_base I ...] <- sums, in_index = the item's chunk, LUT MSG, or CARRY for the carries
//     3. LC     radix_out[i, b] = the (at most s) rows left in column b, terms = s padded with 0xFFFFFFFF
//     4. mi_radix_full_propagate_batch(radix_out)
//
//   mi_radix_mul_batch (pairs (x, y) = (lhs block, rhs block) with x + y < B, pair p = d (d + 1) / 2 + y, d = x + y):
//     1. lhs and rhs of the pass copied into one list (two device-to-device copies)
//        LC     pack[p I + i] = m * lhs[i, x] + rhs[i, y]
//     2. APPLY  pool[0 ...] <- pack, LUT MUL_LSB for the lsb rows and MUL_MSB for the msb rows (m > 2, x + y < B - 1);
//               column b: lsb of (b - y, y), y = 0 .. b, then msb of (b - 1 - y, y), y = 0 .. b - 1: the columns of the
//               2 B - 1 shifted terms in the reference's chain order, their zero blocks never made
//     3. steps 2 to 4 of the sum on those columns
#include <algorithm>
#include <vector>

#include "c_api_internal.hpp"
#include "lwe_linear_algebra_launch.hpp"
#include "radix_sum_index_launch.hpp"
#include "scratch.hpp"
#include "shortint_internal.hpp"

using namespace mi::capi;
using namespace mi::shortint;

namespace {

// A pass's scratch block stays under this many bytes (a pass holds at least one integer): 18 integers of 32 blocks at
// m = c = 4 and N = 2048 (1808 rows, 29.6 MB each).  The rounds after the product round are hundreds of rows per
// integer and latency-bound, so a pass wants many integers: at 128 MiB (4 integers per pass) a 64-bit multiplication
// measured 99 ms at 4 and at 16 per call.  The wop-pbs trees use 256 MiB (WOP_TREE_CAP_BYTES).
constexpr size_t RADIX_SUM_CAP_BYTES = (size_t)512 << 20;
constexpr size_t MAX_ROUNDS = 4096;

struct Round {
  std::vector<mi::SumColumn> col;
  uint32_t n_chunks = 0, n_items = 0, new_total = 0, out_base = 0;
};

struct Schedule {
  uint32_t n_cols = 0, s = 0;
  uint32_t n_initial = 0, n_slots = 0;  // slots of the initial columns, of the whole pool
  std::vector<Round> rounds;
  std::vector<mi::SumColumn> last;  // list_off and len of the columns after the rounds
  uint32_t max_chunks = 0, max_items = 0;
  mi::PassLayout lay;   // of a pass, and the integers of one (plan_passes)
  size_t per_pass = 0;
};

int schedule_rules(uint64_t m, uint64_t c) {
  if (m < 2 || c < 2 || c > m)
    return fail(MI_ERR_UNSUPPORTED,
                "the radix sum needs message_modulus >= 2 and 2 <= carry_modulus <= message_modulus (a carry has to "
                "be a row of value <= message_modulus - 1)");
  return MI_OK;
}

// the rounds of sum.rs:75-126 on column lengths
int build_schedule(const std::vector<uint32_t>& len0, uint64_t m, uint64_t c, Schedule& out) {
  const uint32_t B = (uint32_t)len0.size(), s = (uint32_t)((m * c - 1) / (m - 1));
  out.n_cols = B, out.s = s;
  std::vector<mi::SumColumn> cur(B);
  uint32_t off = 0;
  for (uint32_t b = 0; b < B; ++b) {
    cur[b] = {off, len0[b], 0, 0, 0};
    off += len0[b];
  }
  out.n_initial = out.n_slots = off;
  while (std::any_of(cur.begin(), cur.end(), [s](const mi::SumColumn& x) { return x.len > s; })) {
    if (out.rounds.size() >= MAX_ROUNDS) return fail(MI_ERR_UNSUPPORTED, "the radix sum schedule has too many rounds");
    Round r;
    r.out_base = out.n_slots;
    std::vector<mi::SumColumn> next(B);
    uint32_t below = 0;  // the chunks of column b - 1: their carries arrive in column b
    for (uint32_t b = 0; b < B; ++b) {
      const uint32_t q = cur[b].len >= s ? cur[b].len / s : 0, new_len = cur[b].len - q * s + below + q;
      cur[b].chunk_off = r.n_chunks, cur[b].item_off = r.n_items, cur[b].new_off = r.new_total;
      next[b] = {r.new_total, new_len, 0, 0, 0};
      r.n_chunks += q;
      r.n_items += below + q;
      r.new_total += new_len;
      below = q;
    }
    r.col = cur;
    cur = next;
    out.n_slots += r.n_items;
    out.max_chunks = std::max(out.max_chunks, r.n_chunks);
    out.max_items = std::max(out.max_items, r.n_items);
    out.rounds.push_back(std::move(r));
  }
  out.last = cur;
  return MI_OK;
}

int initial_lengths(size_t n_blocks, size_t n_terms, const uint32_t* first_block, std::vector<uint32_t>& len0) {
  if (n_blocks == 0) return fail(MI_ERR_INVALID_ARG, "n_blocks is 0");
  if (n_blocks > MAX_ITEMS || (n_terms && n_blocks > MAX_ITEMS / n_terms))
    return fail(MI_ERR_INVALID_ARG, "batch too large");
  std::vector<uint32_t> starts(n_blocks + 1, 0);
  for (size_t t = 0; t < n_terms; ++t) {
    const uint32_t f = first_block ? first_block[t] : 0;
    if (f > n_blocks) return fail(MI_ERR_INVALID_ARG, "first_block is past the end of the integer");
    ++starts[f];
  }
  len0.assign(n_blocks, 0);
  uint32_t live = 0;
  for (size_t b = 0; b < n_blocks; ++b) len0[b] = (live += starts[b]);
  return MI_OK;
}

// the columns of compute_terms_for_mul_low's terms: b + 1 lsb rows and, at m > 2, b msb rows
std::vector<uint32_t> mul_lengths(size_t n_blocks, uint64_t m) {
  std::vector<uint32_t> len0(n_blocks);
  for (size_t b = 0; b < n_blocks; ++b) len0[b] = (uint32_t)(m > 2 ? 2 * b + 1 : b + 1);
  return len0;
}

// after an entry point's own checks: the schedule, the layout of a pass (carve.hpp) and the integers one pass takes
int plan_passes(uint64_t m, uint64_t c, size_t big1, const std::vector<uint32_t>& len0, bool mul, size_t n_integers,
                Schedule& sc) {
  MI_TRY(build_schedule(len0, m, c, sc));
  const mi::PassLayout& p = sc.lay = mi::pass_layout(sc.n_initial, sc.n_slots, sc.max_chunks, sc.max_items, sc.s,
                                                     sc.n_cols, big1, mul);
  const size_t widest = std::max<size_t>({p.list_len + p.tail_rows, p.sum_idx, p.item_idx, p.pack_idx, 1});
  if (widest > MAX_ITEMS) return fail(MI_ERR_INVALID_ARG, "batch too large");
  const size_t n = std::min(std::max<size_t>(RADIX_SUM_CAP_BYTES / p.bytes, 1), MAX_ITEMS / widest);
  sc.per_pass = std::min(n, std::max<size_t>(n_integers, 1));
  return MI_OK;
}

// the descriptor of round r of a schedule, or of the block sums at r = the round count
mi::SumRound round_descriptor(const Schedule& sc, size_t r, size_t I) {
  const bool last = r == sc.rounds.size();
  const std::vector<mi::SumColumn>& col = last ? sc.last : sc.rounds[r].col;
  mi::SumRound d = {};
  d.n_cols = sc.n_cols, d.s = sc.s, d.integers = (uint32_t)I, d.final_round = last;
  std::copy(col.begin(), col.end(), d.col);
  if (!last) d.n_chunks = sc.rounds[r].n_chunks, d.n_items = sc.rounds[r].n_items;
  if (!last) d.new_total = sc.rounds[r].new_total, d.out_base = sc.rounds[r].out_base;
  return d;
}

// The first n rounds of a schedule (the round count + 1: the block sums too).  Each writes its index arrays: a round
// sum_idx, in_idx, lut_idx and its next list from the list before, the block sums sum_idx alone.  With a key (steps 2
// to 4 of the sum, on a filled pool) each launch is followed by its LC and APPLY, the last by the propagation.
int run_rounds(const mi_shortint_key* key, uint64_t* radix_out, const Schedule& sc, const mi::PassWork& w, size_t n,
               size_t I, void* stream) {
  const uint32_t* prev = nullptr;  // round 0: the pool is column-major, a list entry is its own slot
  for (size_t r = 0; r < n; ++r) {
    const bool last = r == sc.rounds.size();
    const mi::SumRound d = round_descriptor(sc, r, I);
    uint32_t* next = last ? nullptr : w.list[r & 1];
    MI_TRY_HIP(mi::launch_radix_sum_round(w.sum_idx, last ? nullptr : w.in_idx, last ? nullptr : w.lut_idx, next, prev,
                                          d, LUT_MSG, LUT_CARRY, (hipStream_t)stream),
               "radix sum index launch");
    prev = next;
    if (!key) continue;
    const size_t big1 = key->big + 1, slots = last ? sc.n_slots : d.out_base;
    const size_t n_sums = last ? I * sc.n_cols : (size_t)d.n_chunks * I;
    uint64_t* sums = last ? radix_out : w.pool + (size_t)sc.n_slots * I * big1;
    MI_TRY(mi_lwe_linear_combination_batch(sums, w.pool, key->big, slots * I, n_sums, sc.s, w.sum_idx, nullptr, nullptr,
                                           key->device, stream));
    if (!last)
      MI_TRY(mi_shortint_apply_lut_batch(key, w.pool + slots * I * big1, sums, n_sums, w.in_idx, key->d_luts, w.lut_idx,
                                         N_KEY_LUTS, (size_t)d.n_items * I, stream));
  }
  return key ? mi_radix_full_propagate_batch(key, radix_out, sc.n_cols, I, stream) : MI_OK;  // 4.
}

int too_many_blocks() {
  return fail(MI_ERR_UNSUPPORTED, "the radix sum and multiplication take at most 128 blocks per integer");
}

}  // namespace

extern "C" {

int mi_radix_sum_schedule(size_t n_blocks, size_t n_terms, const uint32_t* first_block, uint64_t message_modulus,
                          uint64_t carry_modulus, size_t* n_rounds, uint32_t* column_len, uint32_t* column_chunks,
                          size_t rounds_capacity) {
  MI_TRY(schedule_rules(message_modulus, carry_modulus));
  std::vector<uint32_t> len0;
  MI_TRY(initial_lengths(n_blocks, n_terms, first_block, len0));
  Schedule sc;
  MI_TRY(build_schedule(len0, message_modulus, carry_modulus, sc));
  if (n_rounds) *n_rounds = sc.rounds.size();
  if (!column_len && !column_chunks) return MI_OK;
  if (rounds_capacity < sc.rounds.size()) return fail(MI_ERR_INVALID_ARG, "rounds_capacity is below the round count");
  for (size_t r = 0; r <= sc.rounds.size(); ++r) {
    const std::vector<mi::SumColumn>& col = r < sc.rounds.size() ? sc.rounds[r].col : sc.last;
    for (size_t b = 0; b < n_blocks; ++b) {
      if (column_len) column_len[r * n_blocks + b] = col[b].len;
      if (column_chunks && r < sc.rounds.size())
        column_chunks[r * n_blocks + b] = col[b].len >= sc.s ? col[b].len / sc.s : 0;
    }
  }
  return MI_OK;
}

int mi_radix_sum_pass_integers(const mi_shortint_key* key, size_t n_terms, const uint32_t* first_block, size_t n_blocks,
                               size_t n_integers, size_t* pass_integers) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (!pass_integers) return fail(MI_ERR_INVALID_ARG, "pass_integers is NULL");
  MI_TRY(schedule_rules(key->m, key->c));
  std::vector<uint32_t> len0;
  MI_TRY(initial_lengths(n_blocks, n_terms, first_block, len0));
  if (n_blocks > mi::RADIX_MAX_BLOCKS) return too_many_blocks();
  Schedule sc;
  MI_TRY(plan_passes(key->m, key->c, key->big + 1, len0, false, n_integers, sc));
  *pass_integers = sc.per_pass;
  return MI_OK;
}

int mi_radix_mul_pass_integers(const mi_shortint_key* key, size_t n_blocks, size_t n_integers, size_t* pass_integers) {
  if (!key) return fail(MI_ERR_INVALID_ARG, "key is NULL");
  if (!pass_integers) return fail(MI_ERR_INVALID_ARG, "pass_integers is NULL");
  if (n_blocks == 0) return fail(MI_ERR_INVALID_ARG, "n_blocks is 0");
  MI_TRY(schedule_rules(key->m, key->c));
  if (n_blocks > mi::RADIX_MAX_BLOCKS) return too_many_blocks();
  Schedule sc;
  MI_TRY(plan_passes(key->m, key->c, key->big + 1, mul_lengths(n_blocks, key->m), true, n_integers, sc));
  *pass_integers = sc.per_pass;
  return MI_OK;
}

int mi_radix_sum_batch(const mi_shortint_key* key, uint64_t* radix_out, const uint64_t* terms, size_t n_terms,
                       const uint32_t* first_block, size_t n_blocks, size_t n_integers, void* stream) {
  MI_TRY(check_radix(key, radix_out, n_blocks, n_integers));
  MI_TRY(schedule_rules(key->m, key->c));
  std::vector<uint32_t> len0;
  MI_TRY(initial_lengths(n_blocks, n_terms, first_block, len0));
  if (n_blocks > mi::RADIX_MAX_BLOCKS) return too_many_blocks();
  const size_t B = n_blocks, NI = n_integers, big1 = key->big + 1, T = NI * B;
  if (n_terms && T > 0x7FFFFFFFull / n_terms) return fail(MI_ERR_INVALID_ARG, "batch too large");
  if (NI == 0) return MI_OK;
  if (n_terms && !terms) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (overlap(radix_out, T * big1 * 8, terms, n_terms * T * big1 * 8))
    return fail(MI_ERR_INVALID_ARG, "radix_out overlaps terms");
  Schedule sc;
  MI_TRY(plan_passes(key->m, key->c, big1, len0, false, NI, sc));
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  if (n_terms == 0)  // None in the reference: the caller's trivial zero, which has nothing to propagate
    return mi_lwe_linear_combination_batch(radix_out, nullptr, key->big, 0, T, 0, nullptr, nullptr, nullptr, key->device,
                                           stream);
  mi::ScratchBuf buf(sc.lay.bytes * sc.per_pass, s);
  if (!buf.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  for (size_t i0 = 0; i0 < NI; i0 += sc.per_pass) {
    const size_t I = std::min(sc.per_pass, NI - i0);
    const mi::PassWork w = mi::carve_on<mi::PassWork>(buf.ptr(), sc.lay, big1, I);
    // 1. the gather: the live rows of the terms into the column-major pool
    std::vector<uint32_t> rank(B, 0);
    for (size_t t0 = 0; t0 < n_terms; t0 += mi::RADIX_GATHER_TERMS) {
      mi::SumGather ga = {};
      ga.n_cols = (uint32_t)B, ga.n_terms = (uint32_t)std::min<size_t>(mi::RADIX_GATHER_TERMS, n_terms - t0);
      ga.t0 = (uint32_t)t0, ga.integers = (uint32_t)I, ga.n_integers = (uint32_t)NI, ga.i0 = (uint32_t)i0;
      for (uint32_t b = 0, off = 0; b < B; off += len0[b], ++b) ga.col_base[b] = off + rank[b];
      for (uint32_t u = 0; u < ga.n_terms; ++u) {
        ga.first[u] = first_block ? first_block[t0 + u] : 0;
        for (size_t b = ga.first[u]; b < B; ++b) ++rank[b];
      }
      MI_TRY_HIP(mi::launch_radix_sum_gather(w.gather_idx, ga, s), "radix sum index launch");
    }
    MI_TRY(mi_lwe_linear_combination_batch(w.pool, terms, key->big, n_terms * T, (size_t)sc.n_initial * I, 1,
                                           w.gather_idx, nullptr, nullptr, key->device, stream));
    MI_TRY(run_rounds(key, radix_out + i0 * B * big1, sc, w, sc.rounds.size() + 1, I, stream));  // 2. to 4.
  }
  return MI_OK;
}

int mi_radix_mul_batch(const mi_shortint_key* key, uint64_t* radix_out, const uint64_t* lhs, const uint64_t* rhs,
                       size_t n_blocks, size_t n_integers, void* stream) {
  MI_TRY(check_radix(key, radix_out, n_blocks, n_integers));
  MI_TRY(schedule_rules(key->m, key->c));
  if (key->c != key->m)
    return fail(MI_ERR_UNSUPPORTED,
                "the radix multiplication packs message_modulus * lhs + rhs: carry_modulus must equal message_modulus");
  if (n_blocks > mi::RADIX_MAX_BLOCKS) return too_many_blocks();
  if (n_integers == 0) return MI_OK;
  if (!lhs || !rhs) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  const size_t B = n_blocks, NI = n_integers, big1 = key->big + 1, bytes = NI * B * big1 * sizeof(uint64_t);
  for (const uint64_t* p : {lhs, rhs})
    if (p != radix_out && overlap(radix_out, bytes, p, bytes))
      return fail(MI_ERR_INVALID_ARG, "radix_out partially overlaps an operand");
  Schedule sc;
  MI_TRY(plan_passes(key->m, key->c, big1, mul_lengths(B, key->m), true, NI, sc));
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(key->device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  mi::ScratchBuf buf(sc.lay.bytes * sc.per_pass, s);
  if (!buf.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  const size_t pairs = B * (B + 1) / 2;
  for (size_t i0 = 0; i0 < NI; i0 += sc.per_pass) {
    const size_t I = std::min(sc.per_pass, NI - i0), rows = I * B, row_bytes = rows * big1 * sizeof(uint64_t);
    const mi::PassWork w = mi::carve_on<mi::PassWork>(buf.ptr(), sc.lay, big1, I);
    uint64_t *staged = w.tail, *pack = staged + 2 * rows * big1;  // 1. the staged operands, then the packed pairs
    MI_TRY(stage_pair(staged, lhs + i0 * B * big1, rhs + i0 * B * big1, row_bytes, "radix mul copy", s));
    const mi::MulPairs mp = {(uint32_t)B, (uint32_t)I, key->m > 2 ? 1u : 0u, LUT_MUL_LSB, LUT_MUL_MSB, (int64_t)key->m};
    MI_TRY_HIP(mi::launch_radix_mul_pairs(w.pack_idx, w.pack_coeff, w.in_idx, w.lut_idx, mp, s),
               "radix mul index launch");
    MI_TRY(mi_lwe_linear_combination_batch(pack, staged, key->big, 2 * rows, pairs * I, 2, w.pack_idx, w.pack_coeff,
                                           nullptr, key->device, stream));
    // 2. the products
    MI_TRY(mi_shortint_apply_lut_batch(key, w.pool, pack, pairs * I, w.in_idx, key->d_luts, w.lut_idx, N_KEY_LUTS,
                                       (size_t)sc.n_initial * I, stream));
    MI_TRY(run_rounds(key, radix_out + i0 * B * big1, sc, w, sc.rounds.size() + 1, I, stream));  // 3.
  }
  return MI_OK;
}

int mi_radix_mul_index_arrays(uint64_t message_modulus, uint64_t carry_modulus, size_t n_blocks, size_t n_integers,
                              size_t step, uint32_t* index, int64_t* coeff, uint32_t* in_index, uint32_t* lut_index,
                              size_t capacity, size_t* n_index, size_t* n_items, int device, void* stream) {
  if (n_blocks == 0) return fail(MI_ERR_INVALID_ARG, "n_blocks is 0");
  MI_TRY(schedule_rules(message_modulus, carry_modulus));
  if (n_blocks > mi::RADIX_MAX_BLOCKS) return too_many_blocks();
  if (!index || !coeff || !in_index || !lut_index) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  Schedule sc;  // no pass here: the arrays are the caller's
  MI_TRY(build_schedule(mul_lengths(n_blocks, message_modulus), message_modulus, carry_modulus, sc));
  const size_t B = n_blocks, I = n_integers, R = sc.rounds.size(), pairs = B * (B + 1) / 2;
  if (step > R + 1) return fail(MI_ERR_INVALID_ARG, "step is past the block sums");
  // every step up to `step` writes into the caller's arrays
  size_t need = std::max(2 * pairs, (size_t)sc.n_initial) * I;
  for (size_t r = 0; r < std::min(step, R); ++r)
    need = std::max({need, (size_t)sc.rounds[r].n_chunks * sc.s * I, (size_t)sc.rounds[r].n_items * I});
  if (step == R + 1) need = std::max(need, B * sc.s * I);
  if (I == 0 || need > MAX_ITEMS * 16) return fail(MI_ERR_INVALID_ARG, "batch too large");
  if (need > capacity) return fail(MI_ERR_INVALID_ARG, "capacity is below the entries of a step");
  const hipStream_t s = (hipStream_t)stream;
  DeviceGuard g(device);
  if (!g.ok) return fail(MI_ERR_INVALID_ARG, "bad device");
  if (n_index) *n_index = step == 0 ? 2 * pairs * I : step <= R ? (size_t)sc.rounds[step - 1].n_chunks * sc.s * I : B * sc.s * I;
  if (n_items) *n_items = step == 0 ? (size_t)sc.n_initial * I : step <= R ? (size_t)sc.rounds[step - 1].n_items * I : 0;
  if (step == 0) {
    const mi::MulPairs mp = {(uint32_t)B, (uint32_t)I, message_modulus > 2 ? 1u : 0u, LUT_MUL_LSB, LUT_MUL_MSB,
                             (int64_t)message_modulus};
    return hip_status(mi::launch_radix_mul_pairs(index, coeff, in_index, lut_index, mp, s), "radix mul index launch");
  }
  mi::ScratchBuf buf(2 * (size_t)sc.n_initial * sizeof(uint32_t), s);  // the two lists
  if (!buf.ok()) return fail(MI_ERR_OOM, "scratch allocation failed");
  mi::PassWork w = {};  // the caller's arrays and the two lists
  w.sum_idx = index, w.in_idx = in_index, w.lut_idx = lut_index;
  w.list[0] = (uint32_t*)buf.ptr(), w.list[1] = w.list[0] + sc.n_initial;
  // steps 1 .. R are the rounds and step R + 1 the block sums: the first `step` launches, with nothing in between
  return run_rounds(nullptr, nullptr, sc, w, step, I, stream);
}

}  // extern "C"
