// Host shim: device contexts, their pool, the per-call lease and pinned staging.
#pragma once

#include <cstring>
#include <mutex>
#include <vector>

#include "host_index.h"

// device contexts: a HIP stream, events and reusable scratch.  Calls borrow a
// context from a process-wide pool and return it when they finish, so the
// number of contexts (and their device memory) is bounded by the peak number
// of concurrent calls, whatever threads make them (zfpy builds a new thread
// pool per call).  zfp_hip_release_scratch() frees the idle ones.
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
};

struct Ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  hipStream_t side[2] = {nullptr, nullptr};  // host slab pipeline: uploads, downloads
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // [4], [5]: index scan
  Scratch field, words, status, partials, misc, ovf, fpbuf;
  Scratch scan_bm, scan_seg, scan_tiles, scan_pos;  // index scan of a stream without index
  zfp_hip_index scan_index;                         // index built by the scan
  Scratch chk;                                      // index verification word (DecodeArgs::idx_bad)
  Scratch boxes;                                    // batched region decode: the records and wave_first
  uint32_t* idx_chk = nullptr;                      // set while a caller's index is being verified
  char* pin = nullptr;                              // pinned staging of small host copies (pin_take)
  size_t pin_used = 0;                              // bytes of it handed out in the current call
  // Compress with field and stream both on the device: nothing is queued before
  // or after the encode kernel's own events, so the call records those two only
  // and record_timing reads the call time from them as well.
  bool one_pair = false;
  bool single_kernel = false;  // set by launch_encode when it queued exactly ev[1], one kernel, ev[2]
};

struct Timing {
  double kernel_ms = 0, total_ms = 0, scan_ms = 0;
  int scan_passes = 0;
  bool timed = false;
  bool stale_index = false;  // the last decompress found its index stale and scanned (zfp_hip_last_stale_index)
};
static thread_local Timing t_timing;

static std::mutex g_pool_mu;
static std::vector<Ctx*> g_idle;

static void free_scratch(Scratch& s)
{
  if (s.p)
    (void)hipFree(s.p);
  s.p = nullptr;
  s.bytes = 0;
}

static void destroy_ctx(Ctx* c)
{
  (void)hipSetDevice(c->device);
  for (Scratch* s : {&c->field, &c->words, &c->status, &c->partials, &c->misc, &c->ovf, &c->fpbuf, &c->scan_bm,
                     &c->scan_seg, &c->scan_tiles, &c->scan_pos, &c->chk, &c->boxes})
    free_scratch(*s);
  index_release(&c->scan_index);
  if (c->pin)
    (void)hipHostFree(c->pin);
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->stream)
    (void)hipStreamDestroy(c->stream);
  for (auto& q : c->side)
    if (q) (void)hipStreamDestroy(q);
  delete c;
}

static int ensure(Scratch& s, size_t bytes)
{
  if (s.bytes >= bytes)
    return 1;
  free_scratch(s);
  // size classes (powers of two up to 256 MiB, then 64 MiB steps): calls of
  // slightly different sizes reuse a context's buffers instead of regrowing them
  size_t want = 64 << 10;
  if (bytes > ((size_t)256 << 20))
    want = (bytes + ((size_t)64 << 20) - 1) & ~(((size_t)64 << 20) - 1);
  else
    while (want < bytes) want <<= 1;
  hipError_t e = hipMalloc(&s.p, want);
  if (e != hipSuccess) {
    s.p = nullptr;
    return fail("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
  }
  s.bytes = want;
  return 1;
}

// Small host copies go through pinned staging: a pageable hipMemcpyAsync of a
// few KB costs ~19 us (a runtime copy kernel plus a bounce buffer), a pinned
// one a few.  A call takes regions of its context's 1 MiB buffer and frees
// them all by ending (a lease ends with the context's streams synchronized:
// CtxLease); requests that do not fit take the pageable path.  (Block-API calls and array cache
// line fills are made of such copies: include/zfp/hip/array.hpp.)
constexpr size_t kPinBytes = (size_t)1 << 20;
constexpr size_t kPinSmall = (size_t)256 << 10;

static char* pin_take(Ctx* c, size_t bytes)
{
  bytes = (bytes + 63) & ~(size_t)63;
  if (bytes > kPinSmall || c->pin_used + bytes > kPinBytes)
    return nullptr;
  if (!c->pin) {
    if (hipHostMalloc((void**)&c->pin, kPinBytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      c->pin = nullptr;
      return nullptr;
    }
  }
  char* r = c->pin + c->pin_used;
  c->pin_used += bytes;
  return r;
}

// host -> device, staged through pinned memory when small
static int h2d(Ctx* c, void* d, const void* h, size_t bytes, hipStream_t q)
{
  if (char* s = pin_take(c, bytes)) {
    memcpy(s, h, bytes);
    HIP_TRY(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, q));
    return 1;
  }
  HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, q));
  return 1;
}


static Ctx* acquire_ctx(int device)
{
  // (already current, the usual case: no runtime call beyond the query)
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess)
    cur = -1;
  if (device < 0)
    device = cur < 0 ? 0 : cur;
  if (cur != device && hipSetDevice(device) != hipSuccess) {
    fail("hipSetDevice(%d) failed", device);
    return nullptr;
  }
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = g_idle.size(); i-- > 0;)  // most recently returned first
      if (g_idle[i]->device == device) {
        Ctx* c = g_idle[i];
        g_idle.erase(g_idle.begin() + (long)i);
        // Per-call state starts over.  The staging is free: a context comes
        // back to the pool only through ~CtxLease, after the previous call's
        // last synchronize or, when that call failed, the lease's own, so no
        // queued copy can still read or write the pinned bytes.
        c->pin_used = 0;
        c->idx_chk = nullptr;
        c->one_pair = false;
        c->single_kernel = false;
        return c;
      }
  }
  Ctx* c = new Ctx;
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    fail("hipStreamCreate failed");
    delete c;
    return nullptr;
  }
  for (auto& e : c->ev)
    (void)hipEventCreate(&e);
  return c;
}

static void release_ctx(Ctx* c)
{
  if (!c)
    return;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_idle.push_back(c);
}

// Borrows a context for the lifetime of one API call (open_call), and is the
// one place where a call's use of it ends.  An entry point returns through
// done(rc): every successful call has synchronized the streams it queued work
// on after queueing the last of it.  Any other way out -- a failed validation
// after work was queued, a HIP_TRY -- may leave copies queued that read or
// write the pinned staging, the scratch buffers or the caller's memory, so the
// lease synchronizes the streams itself before the context goes back to the
// pool, where the next call would reuse all of these.
struct CtxLease {
  Ctx* c = nullptr;
  bool synced = false;
  CtxLease() = default;
  int done(int rc) { synced = rc != 0; return rc; }
  ~CtxLease()
  {
    if (c && !synced)
      for (hipStream_t q : {c->stream, c->side[0], c->side[1]})
        if (q) (void)hipStreamSynchronize(q);
    release_ctx(c);
  }
  CtxLease(const CtxLease&) = delete;
  CtxLease& operator=(const CtxLease&) = delete;
};

static bool is_device_ptr(const void* p)
{
  if (!p)
    return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice;
}
