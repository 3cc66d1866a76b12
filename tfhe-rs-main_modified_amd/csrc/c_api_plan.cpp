// c_api_plan.cpp — construction, release and the process-wide cache of the prime64 plans (Plan::try_new,
// tfhe-ntt/src/prime64.rs:764-862).  The host tables are the pure functions of ntt64_plan_tables.hpp, uploaded once to
// the plan's device; the plan owns its device buffers and one routine releases them.
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <tuple>
#include <vector>

#include "c_api_internal.hpp"
#include "ntt64_plan_tables.hpp"

using namespace mi::capi;

namespace {

// the one place that frees a plan's device buffers: mi_ntt64_plan_destroy and, as the deleter of the half-built plan,
// every failure exit of plan_create
struct PlanRelease {
  void operator()(mi_ntt64_plan* plan) const {
    {
      DeviceGuard g(plan->device);
      if (plan->d_twid) (void)hipFree(plan->d_twid);
      if (plan->d_inv_twid) (void)hipFree(plan->d_inv_twid);
      if (plan->d_twist_f) (void)hipFree(plan->d_twist_f);  // d_twist_i and d_twist_fn point into the same allocation
      if (plan->d_split) (void)hipFree(plan->d_split);
      if (plan->d_tw32) (void)hipFree(plan->d_tw32);  // d_itw32 points into the same allocation
    }
    delete plan;
  }
};

// *dst = an allocation on the current device holding `table`.  On failure *dst is NULL if the allocation failed and
// set if the copy did; the plan that holds *dst releases it either way.
hipError_t upload(u64** dst, const std::vector<u64>& table) {
  const hipError_t e = hipMalloc(dst, table.size() * sizeof(u64));
  if (e != hipSuccess) {
    *dst = nullptr;
    return e;
  }
  return hipMemcpy(*dst, table.data(), table.size() * sizeof(u64), hipMemcpyHostToDevice);
}

}  // namespace

extern "C" {

static int plan_create(size_t n, uint64_t p, int device, mi_ntt64_plan** out_plan) {
  namespace H = mi::host;
  // 1. validate: prime64.rs:769-775 — same order of checks as the reference
  if (!out_plan) return fail(MI_ERR_INVALID_ARG, "out_plan is NULL");
  *out_plan = nullptr;
  if (n < 16 || (n & (n - 1)) != 0) return fail(MI_ERR_INVALID_ARG, "polynomial size must be a power of two >= 16");
  if (!H::is_prime64(p)) return fail(MI_ERR_NOT_PRIME, "modulus is not prime");
  const auto ts_root = H::find_primitive_root64(p, 2 * (u64)n);
  if (!ts_root) return fail(MI_ERR_NO_ROOT, "no primitive 2N-th root of unity");
  const int logn = __builtin_ctzll(n);
  // N > 2^14 runs as passes of <= 4 top stages + 2^(logn - 14) blocks (ntt64_kernels.hip dispatch_large); the
  // reference's Solinas root exists up to 2N = 2^32 (roots.rs:96-107), other primes need 2N | p - 1 (checked above)
  if (logn > 31) return fail(MI_ERR_UNSUPPORTED, "this build runs N <= 2^31 on device");
  const bool goldilocks = (p == H::SOLINAS_P);
  const auto w = H::plan_root(n, p, *ts_root);
  if (!w) return fail(MI_ERR_NO_ROOT, "no Solinas root for this size");

  // 2. the host tables (ntt64_plan_tables.hpp), all of them before this plan's first device allocation
  H::BaseTables base = H::base_tables(n, p, *w);
  const H::DeviceForm dev = H::device_form(base, p);
  std::vector<u64> t32, twist, blk;
  if (H::shoup32_applies(p)) t32 = H::shoup32_tables(base, p);
  if (goldilocks && n == 2048 && H::twist_tower_ok(base, p)) twist = H::twist_table(base, p);
  const mi_ntt64_plan* sub = nullptr;
  if (goldilocks && logn >= 12 && logn <= MI_SPLIT_MAX_LOGN && H::split_pow2_ok(base, p)) {
    // the split transform (launch_ntt_split) needs the 2048 plan's twisted body and the root tower, checked against
    // the tables both plans were built from.  A failure to build the cached 2048 sub-plan (e.g. a transient OOM) fails
    // this plan too, with the sub-plan's status and message, instead of quietly leaving it on the slower window kernels
    // for its lifetime
    const int rc = mi_ntt64_plan_cached(2048, p, device, &sub);
    if (rc != MI_OK) return rc;
    if (sub->twisted && H::split_root_ok(base, p, sub->twid[H::bit_rev(11, 1)])) blk = H::split_block_table(base, p);
  }

  // 3. allocate and upload: the plan owns each buffer from its allocation on, so every exit releases what exists
  DeviceGuard g(device);
  if (!g.ok) { return fail(MI_ERR_HIP, "hipSetDevice failed"); }
  std::unique_ptr<mi_ntt64_plan, PlanRelease> plan(new (std::nothrow) mi_ntt64_plan);
  if (!plan) return fail(MI_ERR_OOM, "host allocation failed");
  plan->n = n;
  plan->logn = logn;
  plan->p = p;
  plan->device = device;
  plan->goldilocks = goldilocks;
  plan->twid = std::move(base.twid);
  plan->inv_twid = std::move(base.inv_twid);
  plan->n_inv = base.n_inv;
  plan->mp.p = dev.mont.p;
  plan->mp.pinv = dev.mont.pinv;
  plan->mp.r2 = dev.mont.r2;
  plan->c_normalize = dev.c_normalize;
  plan->c_man = dev.c_man;
  plan->c_macc = dev.c_macc;

  const auto twiddle_fail = [](const u64* d, hipError_t e) {
    return d ? hip_fail(e, "twiddle upload") : fail(MI_ERR_OOM, "twiddle allocation failed");
  };
  hipError_t e = upload(&plan->d_twid, dev.tw);
  if (e != hipSuccess) return twiddle_fail(plan->d_twid, e);
  e = upload(&plan->d_inv_twid, dev.itw);
  if (e != hipSuccess) return twiddle_fail(plan->d_inv_twid, e);
  if (!t32.empty()) {
    e = upload(&plan->d_tw32, t32);
    if (e != hipSuccess) return hip_fail(e, "twiddle upload");
    plan->d_itw32 = plan->d_tw32 + n;
  }
  if (!twist.empty()) {
    if (upload(&plan->d_twist_f, twist) != hipSuccess) return fail(MI_ERR_OOM, "twist table allocation failed");
    plan->d_twist_i = plan->d_twist_f + n + 32;
    plan->d_twist_fn = plan->d_twist_f + 3 * (n + 32) + 32;
  }
  plan->twisted = plan->d_twist_f != nullptr;
  if (!blk.empty()) {
    if (upload(&plan->d_split, blk) != hipSuccess)
      return plan->d_split ? fail(MI_ERR_HIP, "split-transform table upload failed")
                           : fail(MI_ERR_OOM, "split-transform table allocation failed");
    plan->sub2048 = sub;
    plan->split.blk_fwd = plan->d_split;
    plan->split.blk_inv = plan->d_split + n;
    plan->split.body_fwd = sub->d_twist_f;
    plan->split.body_inv = sub->d_twist_i;
  }

  // 4. publish
  *out_plan = plan.release();
  return MI_OK;
}

// the host tables (2 x N u64 plus their device-form copies: ~64 GiB at N = 2^31) are std::vectors: an allocation
// failure is returned as MI_ERR_OOM instead of unwinding through the C ABI (plan_create holds the plan in a
// unique_ptr, and every device allocation comes after the large host tables)
int mi_ntt64_plan_create(size_t n, uint64_t p, int device, mi_ntt64_plan** out_plan) {
  try {
    return plan_create(n, p, device, out_plan);
  } catch (const std::bad_alloc&) {
    if (out_plan) *out_plan = nullptr;
    return fail(MI_ERR_OOM, "host allocation of the twiddle tables failed");
  }
}

int mi_ntt64_plan_destroy(mi_ntt64_plan* plan) {
  if (!plan || plan->cached) return MI_OK;
  PlanRelease()(plan);
  return MI_OK;
}

// Ntt64::new's PLANS map (ntt64.rs:27-79): a read-locked probe, then one slot per key whose plan is built under
// that slot's own mutex, so concurrent first users of one (n, p, device) build it once and other keys are not
// blocked behind that build.  A failed build is not cached (the reference's map only ever holds built plans):
// the slot stays empty and the next caller retries, so a transient failure (e.g. an OOM while uploading the
// tables) does not make the key unusable for the rest of the process.
int mi_ntt64_plan_cached(size_t n, uint64_t p, int device, const mi_ntt64_plan** out_plan) {
  if (!out_plan) return fail(MI_ERR_INVALID_ARG, "out_plan is NULL");
  *out_plan = nullptr;
  struct Slot {
    std::mutex build;
    std::atomic<mi_ntt64_plan*> plan{nullptr};
  };
  static std::shared_mutex mu;
  static std::map<std::tuple<size_t, uint64_t, int>, std::unique_ptr<Slot>>* plans =
      new std::map<std::tuple<size_t, uint64_t, int>, std::unique_ptr<Slot>>;  // never destroyed, like PLANS
  const auto key = std::make_tuple(n, p, device);
  Slot* slot = nullptr;
  {
    std::shared_lock<std::shared_mutex> rd(mu);
    auto it = plans->find(key);
    if (it != plans->end()) slot = it->second.get();
  }
  if (!slot) {
    std::unique_lock<std::shared_mutex> wr(mu);
    auto& ent = (*plans)[key];
    if (!ent) ent.reset(new Slot);
    slot = ent.get();
  }
  mi_ntt64_plan* built = slot->plan.load(std::memory_order_acquire);
  if (!built) {
    std::lock_guard<std::mutex> lk(slot->build);
    built = slot->plan.load(std::memory_order_acquire);
    if (!built) {
      const int st = mi_ntt64_plan_create(n, p, device, &built);
      if (st != MI_OK) return st;  // last_error() already holds the reason; nothing is cached
      built->cached = true;
      slot->plan.store(built, std::memory_order_release);
    }
  }
  *out_plan = built;
  return MI_OK;
}

int mi_ntt64_plan_info(const mi_ntt64_plan* plan, size_t* n, uint64_t* p, int* device) {
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (n) *n = plan->n;
  if (p) *p = plan->p;
  if (device) *device = plan->device;
  return MI_OK;
}

int mi_ntt64_plan_twiddles(const mi_ntt64_plan* plan, uint64_t* twid, uint64_t* inv_twid, uint64_t* n_inv) {
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (twid) std::memcpy(twid, plan->twid.data(), plan->n * sizeof(u64));
  if (inv_twid) std::memcpy(inv_twid, plan->inv_twid.data(), plan->n * sizeof(u64));
  if (n_inv) *n_inv = plan->n_inv;
  return MI_OK;
}

}  // extern "C"
