// c_api.cpp — the extern "C" boundary declared in include/tfhe_ntt_amd.h.
//
// Owns the error state, the transform routing of a prime64 plan, the pointwise, Ntt64View and host-slice entries and
// argument validation; never aborts, every failure is a status code plus a thread-local message.  Plan construction,
// the external product / PBS family, the prime32 and native CRT plans, the f64-FFT path, the serialised keys, the
// keyswitch family, the multi-GPU helpers and the 128-bit bootstrap have their own files (c_api_plan.cpp,
// c_api_pbs.cpp, c_api_native.cpp, c_api_fft.cpp, c_api_keys.cpp, c_api_keyswitch.cpp, c_api_multi_gpu.cpp,
// c_api_pbs128.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "scratch.hpp"
#include "build_info.hpp"  // build/ (Makefile): MI_SOURCE_HASH
#include "c_api_internal.hpp"

namespace mi {
namespace capi {
std::string& last_error() {
  thread_local std::string msg;
  return msg;
}
}  // namespace capi
}  // namespace mi

using namespace mi::capi;

extern "C" {

const char* mi_status_string(int status) {
  switch (status) {
    case MI_OK: return "ok";
    case MI_ERR_INVALID_ARG: return "invalid argument";
    case MI_ERR_NOT_PRIME: return "modulus is not prime";
    case MI_ERR_NO_ROOT: return "no primitive 2N-th root of unity for this modulus";
    case MI_ERR_HIP: return "HIP runtime error";
    case MI_ERR_OOM: return "device out of memory";
    case MI_ERR_UNSUPPORTED: return "unsupported by this build";
    default: return "unknown status";
  }
}

const char* mi_last_error_message(void) { return last_error().c_str(); }

const char* mi_build_source_hash(void) { return MI_SOURCE_HASH; }

}  // extern "C"

int mi::capi::check_batch(const mi_ntt64_plan* plan, const void* buf, size_t batch, size_t stride) {
  if (!plan) return fail(MI_ERR_INVALID_ARG, "plan is NULL");
  if (batch == 0) return MI_OK;
  if (!buf) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  if (stride < plan->n) return fail(MI_ERR_INVALID_ARG, "stride < ntt size");
  if (batch > 0xFFFFFFFFull) return fail(MI_ERR_INVALID_ARG, "batch too large");
  return MI_OK;
}

// Kernel routing: the twisted shift-twiddle kernel for the Solinas N = 2048 plan, the split transform (top passes +
// that kernel on 2048-blocks) for Solinas 2^12 <= N <= 2^MI_SPLIT_MAX_LOGN, else the register-window kernels (Shoup32
// arithmetic for p < 2^32, Montgomery above).  One kernel per plan shape; nothing in the environment changes it.
static hipError_t launch_transform(bool fwd, const mi_ntt64_plan* plan, uint64_t* buf, size_t batch, size_t stride,
                                   hipStream_t s) {
  if (plan->twisted)
    return mi::launch_ntt_tw(fwd, buf, batch, stride, fwd ? plan->d_twist_f : plan->d_twist_i, s);
  if (plan->d_split)
    return mi::launch_ntt_split(fwd, plan->logn, buf, batch, stride, fwd ? plan->d_twid : plan->d_inv_twid,
                                plan->split, s);
  if (plan->d_tw32)
    return mi::launch_ntt_shoup32(fwd, plan->logn, (uint32_t)plan->p, buf, nullptr, batch, stride,
                                  fwd ? plan->d_tw32 : plan->d_itw32, s);
  return mi::launch_ntt(fwd, plan->logn, plan->goldilocks, plan->mp, buf, batch, stride,
                        fwd ? plan->d_twid : plan->d_inv_twid, s);
}

int mi::capi::run_ntt(bool fwd, const mi_ntt64_plan* plan, uint64_t* buf, size_t batch, size_t stride, void* stream) {
  int st = check_batch(plan, buf, batch, stride);
  if (st != MI_OK || batch == 0) return st;
  DeviceGuard g(plan->device);
  hipError_t e = launch_transform(fwd, plan, buf, batch, stride, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, fwd ? "fwd launch" : "inv launch");
}

extern "C" {

int mi_ntt64_fwd_batch(const mi_ntt64_plan* plan, uint64_t* buf, size_t batch, size_t stride, void* stream) {
  return run_ntt(true, plan, buf, batch, stride, stream);
}

int mi_ntt64_inv_batch(const mi_ntt64_plan* plan, uint64_t* buf, size_t batch, size_t stride, void* stream) {
  return run_ntt(false, plan, buf, batch, stride, stream);
}

}  // extern "C"

int mi::capi::run_pw(int op, const mi_ntt64_plan* plan, uint64_t* out, const uint64_t* a, const uint64_t* b,
                     size_t batch, size_t stride, void* stream) {
  int st = check_batch(plan, out, batch, stride);
  if (st != MI_OK || batch == 0) return st;
  if (op >= 1 && !b) return fail(MI_ERR_INVALID_ARG, "rhs is NULL");
  if (op == 2 && !a) return fail(MI_ERR_INVALID_ARG, "lhs is NULL");
  const u64 c = op == 0 ? plan->c_normalize : (op == 1 ? plan->c_man : plan->c_macc);
  DeviceGuard g(plan->device);
  hipError_t e = mi::launch_pointwise(op, plan->goldilocks, plan->mp, out, a, b, plan->n, batch, stride, c,
                                      (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "pointwise launch");
}

extern "C" {

int mi_ntt64_normalize_batch(const mi_ntt64_plan* plan, uint64_t* buf, size_t batch, size_t stride, void* stream) {
  return run_pw(0, plan, buf, nullptr, nullptr, batch, stride, stream);
}

int mi_ntt64_mul_assign_normalize_batch(const mi_ntt64_plan* plan, uint64_t* lhs, const uint64_t* rhs, size_t batch,
                                        size_t stride, void* stream) {
  return run_pw(1, plan, lhs, nullptr, rhs, batch, stride, stream);
}

int mi_ntt64_mul_accumulate_batch(const mi_ntt64_plan* plan, uint64_t* acc, const uint64_t* lhs, const uint64_t* rhs,
                                  size_t batch, size_t stride, void* stream) {
  return run_pw(2, plan, acc, lhs, rhs, batch, stride, stream);
}

// ---- the Ntt64View layer (tfhe/src/core_crypto/commons/math/ntt/ntt64.rs:89-266), batched ------------------------
// The Solinas N = 2048 plan runs the fused twisted bodies (ntt64_view.hip: one launch, conversions at load / store);
// every other plan an elementwise pass around its own transform.  Two operands of one call are either the same buffer
// (forward forms only) or disjoint.
static bool view_overlap(const uint64_t* a, const uint64_t* b, size_t n, size_t batch, size_t stride) {
  const size_t span = (batch - 1) * stride + n;
  return a < b + span && b < a + span;
}

static int run_view_fwd(const mi_ntt64_plan* plan, int kind, unsigned width, bool normalized, uint64_t* ntt,
                        const uint64_t* standard, size_t batch, size_t stride, void* stream) {
  int st = check_batch(plan, ntt, batch, stride);
  if (st != MI_OK || batch == 0) return st;
  if (!standard) return fail(MI_ERR_INVALID_ARG, "standard buffer is NULL");
  if (kind == 1 && (width < 1 || width > 64))
    return fail(MI_ERR_INVALID_ARG, "input_modulus_width must be in [1, 64]");
  if (ntt != standard && view_overlap(ntt, standard, plan->n, batch, stride))
    return fail(MI_ERR_INVALID_ARG, "ntt and standard must be the same buffer or disjoint");
  DeviceGuard g(plan->device);
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  if (plan->twisted) {
    e = mi::launch_view_fwd_tw(kind, ntt, standard, batch, stride, width,
                               normalized ? plan->d_twist_fn : plan->d_twist_f, s);
  } else {
    if (kind != 0 || ntt != standard)
      e = mi::launch_view_pre(kind, ntt, standard, plan->n, batch, stride, width, plan->p, s);
    if (e == hipSuccess) e = launch_transform(true, plan, ntt, batch, stride, s);
    if (e == hipSuccess && normalized)
      e = mi::launch_pointwise(0, plan->goldilocks, plan->mp, ntt, nullptr, nullptr, plan->n, batch, stride,
                               plan->c_normalize, s);
  }
  return e == hipSuccess ? MI_OK : hip_fail(e, "Ntt64View forward launch");
}

int mi_ntt64_forward_batch(const mi_ntt64_plan* plan, uint64_t* ntt, const uint64_t* standard, size_t batch,
                           size_t stride, void* stream) {
  return run_view_fwd(plan, 0, 0, false, ntt, standard, batch, stride, stream);
}

int mi_ntt64_forward_normalized_batch(const mi_ntt64_plan* plan, uint64_t* ntt, const uint64_t* standard, size_t batch,
                                      size_t stride, void* stream) {
  return run_view_fwd(plan, 0, 0, true, ntt, standard, batch, stride, stream);
}

int mi_ntt64_forward_from_power_of_two_modulus_batch(const mi_ntt64_plan* plan, unsigned input_modulus_width,
                                                     uint64_t* ntt, const uint64_t* standard, size_t batch,
                                                     size_t stride, void* stream) {
  return run_view_fwd(plan, 1, input_modulus_width, false, ntt, standard, batch, stride, stream);
}

int mi_ntt64_forward_from_decomp_batch(const mi_ntt64_plan* plan, uint64_t* ntt, const uint64_t* decomp, size_t batch,
                                       size_t stride, void* stream) {
  return run_view_fwd(plan, 2, 0, false, ntt, decomp, batch, stride, stream);
}

// width 0: add_backward (custom modulus); else add_backward_on_power_of_two_modulus with that output width
static int run_view_add(const mi_ntt64_plan* plan, unsigned width, uint64_t* standard, uint64_t* ntt, size_t batch,
                        size_t stride, void* stream) {
  int st = check_batch(plan, ntt, batch, stride);
  if (st != MI_OK || batch == 0) return st;
  if (!standard) return fail(MI_ERR_INVALID_ARG, "standard buffer is NULL");
  if (view_overlap(ntt, standard, plan->n, batch, stride))
    return fail(MI_ERR_INVALID_ARG, "standard and ntt must be disjoint");
  DeviceGuard g(plan->device);
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if (plan->twisted && (width == 0 || width == 64)) {
    e = mi::launch_view_inv_tw(width == 64, standard, ntt, batch, stride, plan->d_twist_i, s);
  } else {
    e = launch_transform(false, plan, ntt, batch, stride, s);
    if (e == hipSuccess) e = mi::launch_view_post(standard, ntt, plan->n, batch, stride, width, plan->p, s);
  }
  return e == hipSuccess ? MI_OK : hip_fail(e, "Ntt64View add_backward launch");
}

int mi_ntt64_add_backward_batch(const mi_ntt64_plan* plan, uint64_t* standard, uint64_t* ntt, size_t batch,
                                size_t stride, void* stream) {
  return run_view_add(plan, 0, standard, ntt, batch, stride, stream);
}

int mi_ntt64_add_backward_on_power_of_two_modulus_batch(const mi_ntt64_plan* plan, unsigned output_modulus_width,
                                                        uint64_t* standard, uint64_t* ntt, size_t batch, size_t stride,
                                                        void* stream) {
  if (output_modulus_width < 1 || output_modulus_width > 64)
    return fail(MI_ERR_INVALID_ARG, "output_modulus_width must be in [1, 64]");
  return run_view_add(plan, output_modulus_width, standard, ntt, batch, stride, stream);
}

// The `&mut [u64]` host form (Plan::fwd / Plan::inv on a caller slice, as Ntt64View::forward / add_backward call
// it per polynomial, ntt64.rs:89-137).  Each call borrows a staging slot of the plan's device from a process-wide
// pool: a private non-blocking stream of the highest priority, a device buffer and a mapped, coherent pinned host buffer, all grown on
// demand and reused.  Up to ZERO_COPY_BYTES the transform runs in place on the pinned buffer itself (the kernel
// reads and writes host memory over PCIe: one launch and one wait per call instead of two copies around the
// launch); above it a call is memcpy -> async H2D -> transform -> async D2H -> wait -> memcpy.  No allocation in the
// steady state, and nothing else of the process is synchronised (no hipDeviceSynchronize), so concurrent callers
// (rayon workers) each run on their own slot and stream.
}  // extern "C"

namespace {
struct HostSlot {
  int device = 0;
  hipStream_t stream = nullptr;
  u64* dbuf = nullptr;
  u64* hbuf = nullptr;   // pinned, mapped, coherent
  u64* hdev = nullptr;   // hbuf's device address
  size_t cap = 0;        // u64 elements of both buffers
};

// in-place transform on the mapped host buffer up to this size (profiles/r3/host_path_zero_copy.json against the
// staged rows of profiles/r3/bench_line_driver_cmd.json: faster up to 2 MiB per call — 39.8 vs 46.8 us for one
// N = 1024 round trip, 51.6 vs 87.5 us at 16 polynomials — and level with the staged call at 4 MiB)
constexpr size_t ZERO_COPY_BYTES = (size_t)2 << 20;

struct HostSlotPool {
  std::mutex mu;
  std::vector<HostSlot*> free;  // slots are never destroyed: the pool lives until process exit, as PLANS does
};

HostSlotPool& host_pool() {
  static HostSlotPool* p = new HostSlotPool;
  return *p;
}

HostSlot* acquire_slot(int device) {
  HostSlotPool& pool = host_pool();
  {
    std::lock_guard<std::mutex> lk(pool.mu);
    for (size_t i = 0; i < pool.free.size(); ++i)
      if (pool.free[i]->device == device) {
        HostSlot* s = pool.free[i];
        pool.free[i] = pool.free.back();
        pool.free.pop_back();
        return s;
      }
  }
  HostSlot* s = new (std::nothrow) HostSlot;
  if (!s) return nullptr;
  s->device = device;
  // the highest stream priority: a per-polynomial host call is latency-bound, and a high-priority stream gets
  // hardware queues of its own, so it is never queued behind bulk work of the process's normal-priority streams
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
  if (hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, greatest) != hipSuccess) {
    delete s;
    return nullptr;
  }
  return s;
}

void release_slot(HostSlot* s) {
  HostSlotPool& pool = host_pool();
  std::lock_guard<std::mutex> lk(pool.mu);
  pool.free.push_back(s);
}

hipError_t slot_reserve(HostSlot* s, size_t elems) {
  if (elems <= s->cap) return hipSuccess;
  hipError_t e = hipStreamSynchronize(s->stream);
  if (s->dbuf) (void)hipFree(s->dbuf);
  if (s->hbuf) (void)hipHostFree(s->hbuf);
  s->dbuf = s->hbuf = s->hdev = nullptr;
  s->cap = 0;
  if (e == hipSuccess) e = hipMalloc(&s->dbuf, elems * sizeof(u64));
  if (e == hipSuccess)
    e = hipHostMalloc(&s->hbuf, elems * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->hdev, s->hbuf, 0);
  if (e == hipSuccess) s->cap = elems;
  return e;
}
}  // namespace

extern "C" {

static int run_host(bool fwd, const mi_ntt64_plan* plan, uint64_t* buf, size_t batch) {
  int st = check_batch(plan, buf, batch, plan ? plan->n : 0);
  if (st != MI_OK || batch == 0) return st;
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(MI_ERR_HIP, "hipSetDevice failed");
  HostSlot* slot = acquire_slot(plan->device);
  if (!slot) return fail(MI_ERR_HIP, "staging stream creation failed");
  const size_t elems = batch * plan->n, bytes = elems * sizeof(u64);
  hipError_t e = slot_reserve(slot, elems);
  if (e != hipSuccess) {
    release_slot(slot);
    return fail(MI_ERR_OOM, std::string("staging buffer allocation failed: ") + hipGetErrorString(e));
  }
  std::memcpy(slot->hbuf, buf, bytes);
  if (bytes <= ZERO_COPY_BYTES) {
    e = launch_transform(fwd, plan, slot->hdev, batch, plan->n, slot->stream);
  } else {
    e = hipMemcpyAsync(slot->dbuf, slot->hbuf, bytes, hipMemcpyHostToDevice, slot->stream);
    if (e == hipSuccess) e = launch_transform(fwd, plan, slot->dbuf, batch, plan->n, slot->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(slot->hbuf, slot->dbuf, bytes, hipMemcpyDeviceToHost, slot->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(slot->stream);
  if (e == hipSuccess) std::memcpy(buf, slot->hbuf, bytes);
  release_slot(slot);
  return e == hipSuccess ? MI_OK : hip_fail(e, "host transform");
}

int mi_ntt64_fwd_host(const mi_ntt64_plan* plan, uint64_t* buf, size_t batch) { return run_host(true, plan, buf, batch); }

// The host form of the pointwise ops (Plan::normalize / mul_assign_normalize / mul_accumulate on `&mut [u64]`,
// prime64.rs:1050-1222; update_with_fmadd's per-polynomial calls, ntt64_pbs.rs:683-702): the operands go into one
// pooled staging slot (operand k at k * batch * n), the kernel runs on the slot's stream — in place on the mapped
// pinned buffer up to ZERO_COPY_BYTES, staged through the slot's device buffer above — and the result comes back.
// Same slot pool as run_host: no allocation and no device-wide synchronisation in the steady state.
static int run_host_pw(int op, const mi_ntt64_plan* plan, uint64_t* out, const uint64_t* a, const uint64_t* b,
                       size_t batch) {
  int st = check_batch(plan, out, batch, plan ? plan->n : 0);
  if (st != MI_OK || batch == 0) return st;
  if (op >= 1 && !b) return fail(MI_ERR_INVALID_ARG, "rhs is NULL");
  if (op == 2 && !a) return fail(MI_ERR_INVALID_ARG, "lhs is NULL");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(MI_ERR_HIP, "hipSetDevice failed");
  HostSlot* slot = acquire_slot(plan->device);
  if (!slot) return fail(MI_ERR_HIP, "staging stream creation failed");
  const size_t elems = batch * plan->n, bytes = elems * sizeof(u64);
  const size_t nops = op == 0 ? 1 : (op == 1 ? 2 : 3);
  hipError_t e = slot_reserve(slot, nops * elems);
  if (e != hipSuccess) {
    release_slot(slot);
    return fail(MI_ERR_OOM, std::string("staging buffer allocation failed: ") + hipGetErrorString(e));
  }
  // operand order in the slot: out, then a (mul_accumulate's lhs), then b (the rhs)
  std::memcpy(slot->hbuf, out, bytes);
  if (op == 2) std::memcpy(slot->hbuf + elems, a, bytes);
  if (op >= 1) std::memcpy(slot->hbuf + (nops - 1) * elems, b, bytes);
  const bool zero_copy = nops * bytes <= ZERO_COPY_BYTES;
  u64* base = zero_copy ? slot->hdev : slot->dbuf;
  if (!zero_copy) e = hipMemcpyAsync(slot->dbuf, slot->hbuf, nops * bytes, hipMemcpyHostToDevice, slot->stream);
  const u64 c = op == 0 ? plan->c_normalize : (op == 1 ? plan->c_man : plan->c_macc);
  if (e == hipSuccess)
    e = mi::launch_pointwise(op, plan->goldilocks, plan->mp, base, op == 2 ? base + elems : nullptr,
                             op >= 1 ? base + (nops - 1) * elems : nullptr, plan->n, batch, plan->n, c, slot->stream);
  if (e == hipSuccess && !zero_copy) e = hipMemcpyAsync(slot->hbuf, slot->dbuf, bytes, hipMemcpyDeviceToHost, slot->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(slot->stream);
  if (e == hipSuccess) std::memcpy(out, slot->hbuf, bytes);
  release_slot(slot);
  return e == hipSuccess ? MI_OK : hip_fail(e, "host pointwise op");
}

int mi_ntt64_normalize_host(const mi_ntt64_plan* plan, uint64_t* buf, size_t batch) {
  return run_host_pw(0, plan, buf, nullptr, nullptr, batch);
}

int mi_ntt64_mul_assign_normalize_host(const mi_ntt64_plan* plan, uint64_t* lhs, const uint64_t* rhs, size_t batch) {
  return run_host_pw(1, plan, lhs, nullptr, rhs, batch);
}

int mi_ntt64_mul_accumulate_host(const mi_ntt64_plan* plan, uint64_t* acc, const uint64_t* lhs, const uint64_t* rhs,
                                 size_t batch) {
  return run_host_pw(2, plan, acc, lhs, rhs, batch);
}

int mi_ntt64_inv_host(const mi_ntt64_plan* plan, uint64_t* buf, size_t batch) { return run_host(false, plan, buf, batch); }

int mi_fill_uniform(uint64_t* buf, size_t count, uint64_t seed, uint64_t p, int device, void* stream) {
  if (count == 0) return MI_OK;
  if (!buf) return fail(MI_ERR_INVALID_ARG, "buffer is NULL");
  DeviceGuard g(device);
  hipError_t e = mi::launch_fill_uniform(buf, count, seed, p, (hipStream_t)stream);
  return e == hipSuccess ? MI_OK : hip_fail(e, "fill launch");
}

int mi_scratch_trim(int device, size_t* released) {
  const size_t b = mi::scratch_trim(device);
  if (released) *released = b;
  return MI_OK;
}

int mi_scratch_bytes(int device, size_t* bytes) {
  if (!bytes) return fail(MI_ERR_INVALID_ARG, "bytes is NULL");
  *bytes = mi::scratch_bytes(device);
  return MI_OK;
}

}  // extern "C"
