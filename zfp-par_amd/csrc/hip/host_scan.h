// Host shim: driver of the index scan (scan.h) for a stream without an index.
#pragma once

#include <chrono>

#include "host_index_match.h"

// Index scan (scan.h): block starts of a variable-rate stream resident on the
// device at d_in (word 0 holds bit g0 of the first block), written into `x`.
// Segment length and pass-1 lead-in (ZFP_HIP_SCAN_SEG_BITS / _LEAD_BITS):
// a speculative chain resynchronises after ~116-205 Kbit on average (DESIGN.md
// §3.5), so short segments cost one pass per segment of every unsynchronised
// stretch.  A lead-in cuts the passes of f64 precision-32 streams (512^3: 18 ->
// 5 at 128 Kbit segments and 512 Kbit lead-in, 45 -> 41 ms) but not of 4D
// reversible ones, whose unsynchronised stretches run for megabits (128^4: 91
// passes at 64 Kbit without, 42 at 128 Kbit with, 145 -> 236 ms), so it is off
// by default (profiles/r3_scan_lead.txt).  Since pass 1 starts chains at
// plausible block starts (round 5) almost every segment is settled in pass 1,
// whose time is the slowest lane's start search plus its parse: 32 Kbit
// segments measured faster than 64 (128^4 reversible 38.2-39.6 -> 36.4-37.5 ms,
// 512^3 f64 precision 32 9.7-9.8 -> 7.8-8.0 ms) and 16 Kbit slower again
// (profiles/r5sg_scan_seg.txt, r5sg2_scan_seg_ab.txt).
#ifndef ZFP_SCAN_MIN_SEG_BITS
#define ZFP_SCAN_MIN_SEG_BITS 32768
#endif
#ifndef ZFP_SCAN_LEAD_BITS
#define ZFP_SCAN_LEAD_BITS 0
#endif
constexpr uint64_t kScanMinSegBits = ZFP_SCAN_MIN_SEG_BITS, kScanLeadBits = ZFP_SCAN_LEAD_BITS;

static uint64_t scan_seg_bits(uint64_t limit)
{
  if (const char* e = getenv("ZFP_HIP_SCAN_SEG_BITS")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 64)
      return v & ~63ull;
  }
  // about 2^18 lanes at most
  uint64_t L = (limit + (1ull << 18) - 1) >> 18;
  L = std::max<uint64_t>(L, kScanMinSegBits);
  return (L + 63) & ~63ull;
}

// pass-1 lead-in (scan.h): long enough that a speculative chain has almost
// always met the true one before its segment starts
static uint64_t scan_lead_bits()
{
  if (const char* e = getenv("ZFP_HIP_SCAN_LEAD_BITS"))
    return strtoull(e, nullptr, 10);
  return kScanLeadBits;
}

static void launch_scan_dispatch(Ctx* c, const Plan& p, const ScanArgs& a)
{
  launch_scan_pass(p.type, p.dims, p.cp.minexp < kMinExp, dim3((unsigned)((a.nseg + 255) / 256)), c->stream, a);
}

// plain: ordinary passes only (every chain starts at its segment's first bit,
// no refusals) -- the fallback when the decoders' length check rejects an
// index the heuristic scan built (decompress_once).
static int scan_index(Ctx* c, const Plan& p, const uint64_t* d_in, uint64_t in_words, uint32_t g0,
                      zfp_hip_index* x, bool plain = false)
{
  const uint64_t nb = p.g.nblocks;
  const uint64_t avail = in_words * 64 > g0 ? in_words * 64 - g0 : 0;
  const uint64_t extent = std::min<uint64_t>(avail, nb * (uint64_t)p.max_len);
  const uint64_t limit = extent + 1;  // bit positions 0..extent may start a block (or end the last)
  const uint64_t seg = scan_seg_bits(limit);
  const uint64_t nseg = (limit + seg - 1) / seg;
  const uint64_t bm_words = (limit + 63) / 64;
  const uint64_t ntiles = (bm_words + kTileWords - 1) / kTileWords;
  if (!ensure(c->scan_bm, bm_words * 8) || !ensure(c->scan_seg, nseg * 4 * 8 + 64) ||
      !ensure(c->scan_tiles, ntiles * 8 + 64) || !ensure(c->scan_pos, (nb + 1) * 8) ||
      !index_reserve(x, nb, p.nwaves))
    return 0;
  hipEvent_t e0 = c->ev[4], e1 = c->ev[5];
  HIP_TRY(hipEventRecord(e0, c->stream));
  uint64_t* bm = (uint64_t*)c->scan_bm.p;
  uint64_t* used = (uint64_t*)c->scan_seg.p;
  uint64_t* xs = used + nseg;
  uint64_t* xsnap = xs + nseg;
  uint64_t* plaus = xsnap + nseg;
  uint32_t* moved = (uint32_t*)(plaus + nseg);
  uint32_t* refused = moved + 1;
  HIP_TRY(hipMemsetAsync(bm, 0, bm_words * 8, c->stream));
  HIP_TRY(hipMemsetAsync(used, 0xff, nseg * 8, c->stream));
  ScanArgs a{};
  a.in = d_in;
  a.in_words = in_words;
  a.g0 = g0;
  a.first = 1;
  a.seg_bits = seg;
  a.lead = scan_lead_bits();
  a.nseg = nseg;
  a.limit = limit;
  a.bm = bm;
  a.entry_used = used;
  a.xsnap = xsnap;
  a.x = xs;
  a.moved = moved;
  a.sp = ScanParams{p.cp.minbits, p.cp.maxbits, p.cp.maxprec, p.cp.minexp};
  // float streams: pass 1 starts each chain at a plausible block start (scan.h);
  // ZFP_HIP_SCAN_PLAUSIBLE=0 starts them at the segment's first bit instead
  const char* pl = getenv("ZFP_HIP_SCAN_PLAUSIBLE");
  if ((p.type == 3 || p.type == 4) && !plain && !(pl && pl[0] == '0')) {
    int32_t* win = reinterpret_cast<int32_t*>(moved + 2);
    launch_scan_window(p.type, p.dims, p.cp.minexp < kMinExp, c->stream, a, win);
    HIP_TRY(hipGetLastError());
    a.win = win;
    a.plaus = plaus;
    a.refused = refused;
  }
  launch_scan_dispatch(c, p, a);
  HIP_TRY(hipGetLastError());
  a.first = 0;
  int passes = 1;
  // ZFP_HIP_SCAN_TRACE=1: per-pass wall time and moved exits on stderr (diagnostics)
  const bool trace = getenv("ZFP_HIP_SCAN_TRACE") != nullptr;
  auto tp = std::chrono::steady_clock::now();
  if (trace) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    fprintf(stderr, "scan: %llu segments of %llu bits, pass 1 %.3f ms\n", (unsigned long long)nseg,
            (unsigned long long)seg, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count());
    tp = std::chrono::steady_clock::now();
  }
  // phase A (plausible starts only): passes that refuse implausible chains at
  // segments still holding their plausible chain; phase B: ordinary passes,
  // which settle whatever phase A left inconsistent (scan.h)
  a.refuse = a.plaus ? 1u : 0u;
  // Phase A has its own pass budget: refusals can hold a segment back beyond
  // the one-segment-per-pass settling of ordinary passes, so a slow phase A
  // hands over to phase B (with a fresh budget) rather than failing the call.
  int phase_start = passes;
  for (;;) {
    uint32_t host_cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(xsnap, xs, nseg * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(moved, 0, 8, c->stream));
    launch_scan_dispatch(c, p, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_cnt, moved, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    passes++;
    if (trace) {
      const auto t = std::chrono::steady_clock::now();
      fprintf(stderr, "scan: pass %d%s %.3f ms, %u exits moved, %u refused\n", passes, a.refuse ? " (A)" : "",
              std::chrono::duration<double, std::milli>(t - tp).count(), host_cnt[0], host_cnt[1]);
      tp = t;
    }
    if (!host_cnt[0]) {
      if (!a.refuse || !host_cnt[1])
        break;
      a.refuse = 0;  // phase A settled with refusals outstanding: ordinary passes
      phase_start = passes;
      continue;
    }
    if (a.refuse && (uint64_t)(passes - phase_start) > nseg + 2) {
      a.refuse = 0;  // phase A too slow: ordinary passes from here
      phase_start = passes;
      continue;
    }
    if ((uint64_t)(passes - phase_start) > 2 * nseg + 4)
      return fail("zfp_hip: index scan did not converge after %d passes", passes);
  }
  // Test knob (tests/test_gpu_scan.py): corrupt the heuristic scan's result so
  // that every wave start and the total stay right -- two adjacent lengths
  // moved by 3 bits -- and only the decoders' exact length check can see it.
  const bool corrupt = !plain && nb >= 3 && getenv("ZFP_HIP_TEST_SCAN_CORRUPT");
  // bitmap -> positions -> index
  uint64_t* tiles = (uint64_t*)c->scan_tiles.p;
  uint64_t* sum = tiles + ntiles;
  uint64_t* pos = (uint64_t*)c->scan_pos.p;
  hipLaunchKernelGGL(bm_tile_count, dim3((unsigned)ntiles), dim3(256), 0, c->stream, bm, bm_words, tiles);
  hipLaunchKernelGGL(tile_scan, dim3(1), dim3(1024), 0, c->stream, tiles, ntiles, sum);
  hipLaunchKernelGGL(bm_tile_emit, dim3((unsigned)ntiles), dim3(256), 0, c->stream, bm, bm_words, tiles, nb, pos);
  hipLaunchKernelGGL(index_from_pos, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream, pos, nb, p.per_wave,
                     x->d_len, x->d_base);
  HIP_TRY(hipGetLastError());
  uint64_t host[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&host[0], sum, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&host[1], pos + nb, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(e1, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (host[0] < nb + 1)
    return fail("zfp_hip: stream holds %llu of %llu blocks (truncated or not a stream of this field/mode)",
                (unsigned long long)(host[0] ? host[0] - 1 : 0), (unsigned long long)nb);
  float ms = 0;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
    t_timing.scan_ms = ms;
  t_timing.scan_passes = passes;
  index_layout(x, c, p);
  x->total_bits = host[1];
  if (corrupt) {
    uint16_t l[2];
    HIP_TRY(hipMemcpyAsync(l, x->d_len + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int d = l[1] >= 3 ? 3 : -3;
    l[0] = (uint16_t)(l[0] + d);
    l[1] = (uint16_t)(l[1] - d);
    HIP_TRY(hipMemcpyAsync(x->d_len + 1, l, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return 1;
}
