// Host shim: the skeleton of a call -- how it opens once its arguments are
// valid, the check word of a variable-rate decode, and what a decoder does
// when that word says the index was stale.
#pragma once

#include "host_ctx.h"

// What follows an entry's validation: a device to run on, a context for the
// call and fresh per-call timing.  Nothing before it makes a GPU call.
static int open_call(CtxLease& lease, const char* who, int device)
{
  if (zfp_hip_device_count() <= 0)
    return fail("%s: no HIP device available", who);
  lease.c = acquire_ctx(device);
  if (!lease.c)
    return 0;
  t_timing = Timing{};
  return 1;
}

// Every variable-rate index is verified exactly by the decode kernels, every
// block's decoded length against its entry (DecodeArgs::idx_bad): a caller's
// that passed the (sampled) fingerprint, and the scan's own (its
// plausible-start heuristic and refusals must never decode garbage silently).
// arm() before the call's first event, queue() after its last kernel,
// verdict() after its last synchronize.
namespace {  // (internal, as the shim's static functions: the library exports the C API only)
struct CheckWord {
  Ctx* c;
  const uint32_t* fetched = nullptr;  // the word, copied with the call's last synchronize

  // zeroes the word and sets c->idx_chk for the launchers; nothing for fixed rate
  int arm(bool fixed)
  {
    c->idx_chk = nullptr;
    if (fixed)
      return 1;
    if (!ensure(c->chk, 8))
      return 0;
    HIP_TRY(hipMemsetAsync(c->chk.p, 0, 4, c->stream));
    c->idx_chk = (uint32_t*)c->chk.p;
    return 1;
  }
  int queue()
  {
    uint32_t* q = c->idx_chk ? (uint32_t*)pin_take(c, 4) : nullptr;
    if (q) {
      HIP_TRY(hipMemcpyAsync(q, c->chk.p, 4, hipMemcpyDeviceToHost, c->stream));
      fetched = q;
    }
    return 1;
  }
  // *stale is set when a decoded length disagreed; with nothing queued (the
  // slab pipeline, no pinned staging left) the word is fetched here
  int verdict(bool* stale)
  {
    if (!c->idx_chk)
      return 1;
    uint32_t bad = 0;
    c->idx_chk = nullptr;
    if (fetched) {
      bad = *fetched;
    } else {
      HIP_TRY(hipMemcpyAsync(&bad, c->chk.p, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (bad)
      *stale = true;
    return 1;
  }
};
}  // namespace

// A decode with the caller's index and, when the decoded block lengths
// disagree with it (*stale), again: a caller's index (it passed the
// fingerprint) is replaced by the scan's, a scan-built one (*scanned) by a scan
// of plain passes (no plausible starts, no refusals).
// once(index, plain_scan, &stale, &scanned) is one decode; index nullptr: the
// stream is scanned.
template <typename Once>
static int with_stale_retry(const char* who, const zfp_hip_index* index, Once&& once)
{
  bool stale = false, scanned = false;
  auto run = [&](const zfp_hip_index* x, bool plain) {
    stale = false;
    return once(x, plain, &stale, &scanned);
  };
  int ok = run(index, false);
  if (ok && stale) {
    const bool plain = scanned;
    ok = run(nullptr, plain);
    if (ok && stale && !plain)
      ok = run(nullptr, true);
    t_timing.stale_index = true;
    if (ok && stale)
      return fail("%s: decoded block lengths disagree with the stream's plain scan (corrupt stream)", who);
  }
  return ok;
}
