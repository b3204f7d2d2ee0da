// Host shim: the encode and decode launchers.
#pragma once

#include <cstdlib>

#include "host_index_match.h"

// launchers

// The stream word holding an encode's first bit (bits below g0 belong to what
// precedes it): `val` ORed in (the host's pending bits), or with `keep` the bits
// already in the device word are kept (a host slab pipeline: what the previous
// slab wrote).  `idx_add` is added to the per-wave index bases (the launch's
// bit offset within its chunk).
struct Head {
  uint64_t val = 0;
  bool keep = false;
  uint64_t idx_add = 0;
};

// f(tag) with a null pointer of the field's scalar type
template <typename F>
static int by_type(const Plan& p, F&& f)
{
  switch (p.type) {
    case 1: return f((int32_t*)nullptr);
    case 2: return f((int64_t*)nullptr);
    case 3: return f((float*)nullptr);
    default: return f((double*)nullptr);
  }
}

static uint64_t head_keep_mask(const Head& h, uint32_t g0) { return h.keep && g0 ? (1ull << g0) - 1 : 0ull; }

// double with maxprec <= 32: the kernels that code planes 32..63 only
template <typename S>
static bool hi_planes(const Plan& p)
{
  return std::is_same<S, double>::value && p.dims == 3 && p.cp.maxprec <= kHiPlanesMaxPrec;
}

// 1D/2D blocks and integer fields: the generic per-lane codec (blockn.h),
// instantiated in zfp_hip_n32.hip / zfp_hip_n64.hip (separate translation
// units, compiled in parallel)
template <typename S, int D>
static void launch_enc_generic(Ctx* c, const Plan& p, const S* d_field, dim3 grid, dim3 block, size_t lds,
                               const GeneralArgs& a)
{
  launch_encode_n(p.type, D, p.cp.minexp < kMinExp, c->stream, grid, block, lds, d_field, p.g, p.cp, a);
}

template <typename S, int D>
static void launch_dec_generic(Ctx* c, const Plan& p, S* d_field, dim3 grid, dim3 block, size_t lds,
                               const DecodeArgs& a)
{
  launch_decode_n(p.type, D, p.cp.minexp < kMinExp, c->stream, grid, block, lds, d_field, p.g, p.cp, a);
}

template <typename S, bool HI>
static void launch_general3(Ctx* c, const Plan& p, const S* d_field, dim3 grid, dim3 block, size_t lds,
                            const GeneralArgs& a)
{
  if (p.dims == 1) return launch_enc_generic<S, 1>(c, p, d_field, grid, block, lds, a);
  if (p.dims == 2) return launch_enc_generic<S, 2>(c, p, d_field, grid, block, lds, a);
  if constexpr (kIntField<S>)
    launch_enc_generic<S, 3>(c, p, d_field, grid, block, lds, a);
  else
    launch_encode3_general(Launch{grid, block, lds, c->stream}, p.vec, p.cp.minexp < kMinExp, HI, d_field, p.g,
                           p.cp, a);
}

template <typename S, bool HI>
static void run_decode3(Ctx* c, const Plan& p, S* d_field, dim3 grid, dim3 block, size_t lds, const DecodeArgs& a)
{
  if (p.dims == 1) return launch_dec_generic<S, 1>(c, p, d_field, grid, block, lds, a);
  if (p.dims == 2) return launch_dec_generic<S, 2>(c, p, d_field, grid, block, lds, a);
  if constexpr (kIntField<S>)
    launch_dec_generic<S, 3>(c, p, d_field, grid, block, lds, a);
  else  // short staging slots (a.ovf) exist for the f64 planes-32..63 decoder only
    launch_decode3(Launch{grid, block, lds, c->stream}, p.vec, p.cp.minexp < kMinExp, HI, HI && a.ovf != nullptr,
                   d_field, p.g, p.cp, a);
}

// Arguments of the packing encoders (encode3_general, encode4): fix-up
// partials, look-back state and, for a variable-rate stream with an index, the
// index buffers.  Queues the look-back resets on the stream.
static int general_args(Ctx* c, const Plan& p, uint32_t swp, uint64_t* d_out, uint32_t g0, const IndexView* index,
                        uint64_t idx_add, GeneralArgs& a)
{
  const bool var = !p.fixed;
  const uint64_t nwaves = p.nwaves;
  // misc: [0] total bits, [1] ticket|error
  if (!ensure(c->partials, nwaves * 2 * sizeof(Partial)) || !ensure(c->misc, 64) ||
      (var && !ensure(c->status, nwaves * 8)))
    return 0;
  a = GeneralArgs{};
  a.out = d_out;
  a.g0 = g0;
  a.swp = swp;
  a.var = var ? 1 : 0;
  a.maxbits = p.cp.maxbits;
  a.status = (uint64_t*)c->status.p;
  a.total_bits = (uint64_t*)c->misc.p;
  a.ticket = (uint32_t*)((char*)c->misc.p + 8);
  a.error = (uint32_t*)((char*)c->misc.p + 12);
  a.partials = (Partial*)c->partials.p;
  a.idx_add = idx_add;
  if (var && index) {  // the caller made room (index_begin) and publishes it once the encode succeeded
    a.idx_len = index->d_len;
    a.idx_base = index->d_base;
  }
  HIP_TRY(hipMemsetAsync(c->misc.p, 0, 64, c->stream));
  if (var)
    HIP_TRY(hipMemsetAsync(c->status.p, 0, nwaves * 8, c->stream));
  return 1;
}

// After a packing encoder: merge the words shared by neighbouring waves; for a
// variable-rate stream read back its length (and the look-back health flag).
// kRedoFullSlots: the overflow pool of a short-slot launch ran out, the launch
// must be repeated with full-size slots.
constexpr int kRedoFullSlots = 2;

// merge the words shared by neighbouring waves, and the stream's first word with the head
static void launch_fixups(Ctx* c, const Plan& p, Partial* parts, uint64_t* d_out, uint32_t g0, const Head& head)
{
  const unsigned fg = (unsigned)((2 * p.nwaves + 255) / 256);
  hipLaunchKernelGGL(fixup_zero, dim3(fg), dim3(256), 0, c->stream, parts, 2 * p.nwaves, d_out, 0ull,
                     g0 ? head.val : 0ull, head_keep_mask(head, g0));
  hipLaunchKernelGGL(fixup_or, dim3(fg), dim3(256), 0, c->stream, parts, 2 * p.nwaves, d_out);
}

static int finish_general(Ctx* c, const Plan& p, uint64_t* d_out, uint32_t g0, const Head& head,
                          const GeneralArgs& a, IndexView* index, uint64_t* total_bits)
{
  launch_fixups(c, p, a.partials, d_out, g0, head);
  HIP_TRY(hipGetLastError());
  if (!p.fixed) {
    uint64_t host[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(host, c->misc.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t err = (uint32_t)(host[1] >> 32);
    if (err & 1u)
      return fail("zfp_hip: look-back timed out (GPU scheduling anomaly)");
    if (err & 2u)
      return kRedoFullSlots;
    *total_bits = host[0];
    if (index)
      index->total_bits = host[0];
  } else {
    *total_bits = p.g.nblocks * (uint64_t)p.cp.maxbits;
  }
  return 1;
}

// Short LDS slots for the variable-rate 3D encoders.  A slot sized for the
// block's worst case (C3: 2,123 bits, 35 words) limits the CU to two
// workgroups; the kernels' registers allow three (f64 planes 32..63: <= 168
// VGPRs) or four (f32 lossy).  The slot is cut to what that
// many workgroups can hold; blocks that code longer take the overflow pool.
// Fixed rate, 1D/2D and integer fields keep full-size slots.
template <typename S>
static uint32_t short_slot_words(const Plan& p)
{
  if (p.fixed || p.dims != 3 || kIntField<S> || getenv("ZFP_HIP_FULL_SLOTS"))
    return ~0u;
  const bool rev = p.cp.minexp < kMinExp;
  // f32 reversible: 177 VGPRs (two waves per SIMD whatever the slots); measured
  // slower at three with spills
  int groups;
  if (sizeof(S) == 4)
    groups = rev ? 2 : 4;
  else
    groups = hi_planes<S>(p) ? 3 : 2;
  if (const char* e = getenv("ZFP_HIP_SLOT_WORDS"))  // tests: force overflows
    return (uint32_t)atoi(e) | 1u;
  const int64_t words = ((int64_t)(160 * 1024) / groups - (int64_t)kLutBytes) / 8 / kWavesPerGroup;
  int64_t swp = (words - 96) / 64;
  if ((swp & 1) == 0)
    swp--;
  return swp < 3 ? ~0u : (uint32_t)swp;
}

// Short slots for the variable-rate 4D encoder (f32 fields): the region of 16
// slots sized for the worst case (f32 reversible: 8,462 bits, 17.3 KB) limits
// the CU to 8 one-wave workgroups (2 waves per SIMD), where the registers allow
// 3 (f32 reversible).  f32 reversible slots are cut to what 12 waves per CU
// leave (93 words, 5,856 intact bits); a block that codes longer -- on the C5 field,
// the blocks that fail the reversible cast test, about 8,300 bits each -- is
// packed with its first bits and listed, and encode4_patch codes it again with
// a full slot.  The overflow pool holds a quarter of the blocks (the round-4
// first try sized it for 1/16 of them: more overflowed on C5 and the launch
// was redone with full slots, 46 -> 90 ms).  C5 chunk 46.4 -> 43.1 ms;
// 128^4 1.51 -> 1.55 ms (profiles/r4o_4d_slots.txt).  Lossy f32 modes keep
// full slots (not measured).  ZFP_HIP_SLOT_WORDS=n forces n-word slots (tests
// of the overflow and patch path), ZFP_HIP_FULL_SLOTS=1 full ones.
// Data whose blocks mostly overflow (noise-like fields) would pay the redo on
// every call: after a redo the next kFullSlotCalls4 calls of the same thread
// take full slots directly, then short slots are tried again.  The backoff is
// per thread (a caller looping over its own noisy data), so calls of other
// threads -- other zfp_parallel chunks, other devices -- are not slowed.
constexpr uint32_t kShortSlotWords4 = 93;
constexpr int kFullSlotCalls4 = 16;
static thread_local int t_full_slot_calls4 = 0;
template <typename S>
static uint32_t short_slot_words4(const Plan& p)
{
  if (p.fixed || kIntField<S> || sizeof(S) == 8 || getenv("ZFP_HIP_FULL_SLOTS"))
    return ~0u;
  if (const char* e = getenv("ZFP_HIP_SLOT_WORDS"))  // tests: force overflows
    return (uint32_t)atoi(e) | 1u;
  if (p.cp.minexp >= kMinExp)
    return ~0u;
  if (t_full_slot_calls4 > 0) {
    t_full_slot_calls4--;
    return ~0u;
  }
  return kShortSlotWords4;
}

template <typename S>
static void launch_encode4_kernel(Ctx* c, const Plan& p, const S* d_field, dim3 grid, size_t lds, const GeneralArgs& a,
                                  bool half)
{
  const bool rev = p.cp.minexp < kMinExp;
  if constexpr (kIntField<S>) {
    launch_encode4_int(p.type, rev, p.vec, c->stream, grid, dim3(64), lds, d_field, p.g, p.cp, a);
  } else {
    launch_encode4(Launch{grid, dim3(64), lds, c->stream}, p.vec, rev, half, d_field, p.g, p.cp, a);
  }
}

// 4D: encode4 for every mode (one 64-thread workgroup per 16 blocks)
template <typename S>
static int run_encode4(Ctx* c, const Plan& p, const S* d_field, uint64_t* d_out, uint32_t g0,
                          const Head& head, IndexView* index, uint64_t* total_bits)
{
  using Int = typename Traits<S>::Int;
  const uint64_t nwaves = p.nwaves;
  if (nwaves > 0x7fffffffull)
    return fail("zfp_hip: field too large for one launch");
  const uint32_t swp_full = slot_words4(p.bound_bits);
  const size_t xfull = (size_t)kBlocks4PerWave * kXStride * sizeof(Int);
  const bool half = !kIntField<S>;  // f32/f64: exchange areas shared by two quads
  const uint32_t swp_short = short_slot_words4<S>(p);
  for (int attempt = 0; attempt < 2; attempt++) {
    const uint32_t swp = attempt == 0 ? std::min(swp_full, swp_short) : swp_full;
    const size_t region = std::max<size_t>((size_t)kBlocks4PerWave * swp * 8, half ? xfull / 2 : xfull);
    const size_t lds = (size_t)kEnc4HeadWords * 8 + region;
    if (lds > 160 * 1024)
      return fail("zfp_hip: 4D block bound %u bits too large for LDS", p.bound_bits);
    GeneralArgs a{};
    if (!general_args(c, p, swp, d_out, g0, index, head.idx_add, a))
      return 0;
    if (swp < swp_full) {
      // a quarter of the blocks (C5: about 1/20 overflow); more makes the
      // launch redo itself with full slots (correct, slower)
      uint64_t cap = std::min<uint64_t>(p.g.nblocks, std::max<uint64_t>(65536, p.g.nblocks / 4));
      if (const char* e = getenv("ZFP_HIP_OVF_POOL"))  // tests: force the full-slot redo
        cap = std::max<uint64_t>(1, std::min<uint64_t>(p.g.nblocks, (uint64_t)atoll(e)));
      if (!ensure(c->ovf, cap * sizeof(OvfEntry)))
        return 0;
      a.ovf = (uint64_t*)c->ovf.p;
      a.ovf_count = (uint32_t*)((char*)c->misc.p + 16);
      a.ovf_cap = (uint32_t)cap;
      a.ovf_swp = swp_full;
      a.cap_bits = slot_cap_bits4(swp);  // clamped writes of an outrun slot land in its last three dwords
    }
#ifdef ZFP_EXP4_TRACE
    const size_t ntr = (nwaves + 63) / 64 * 8;
    uint64_t* d_tr = nullptr;
    if (getenv("ZFP_HIP_TRACE4")) {
      HIP_TRY(hipMalloc(&d_tr, ntr * 8));
      HIP_TRY(hipMemsetAsync(d_tr, 0, ntr * 8, c->stream));
    }
    a.trace = d_tr;
#endif
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    launch_encode4_kernel<S>(c, p, d_field, dim3((unsigned)nwaves), lds, a, half);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
#ifdef ZFP_EXP4_TRACE
    if (d_tr) {
      std::vector<uint64_t> h(ntr);
      HIP_TRY(hipMemcpyAsync(h.data(), d_tr, ntr * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipFree(d_tr));
      // phases: 0 ticket, 1 gather landed, 2 cast+lifts+exchange, 3 transposes+coder, 4 look-back, 5 pack
      double sum[6] = {0}, t0min = 1e30, t0max = 0;
      size_t cnt = 0;
      for (size_t i = 0; i + 8 <= ntr; i += 8) {
        if (!h[i + 6]) continue;
        cnt++;
        uint64_t prev = 0;
        for (int k = 0; k < 6; k++) { sum[k] += (double)(h[i + k] - prev); prev = h[i + k]; }
        t0min = std::min(t0min, (double)h[i + 6]);
        t0max = std::max(t0max, (double)h[i + 6]);
      }
      fprintf(stderr, "trace4 waves %zu (100 MHz ticks, mean): ticket %.1f gather %.1f cast+lift+xchg %.1f coder %.1f lookback %.1f pack %.1f | launch span %.0f\n",
              cnt, sum[0] / cnt, sum[1] / cnt, sum[2] / cnt, sum[3] / cnt, sum[4] / cnt, sum[5] / cnt, t0max - t0min);
    }
#endif
    const int rc = finish_general(c, p, d_out, g0, head, a, index, total_bits);
    if (rc == kRedoFullSlots) {
      if (!getenv("ZFP_HIP_SLOT_WORDS") && !getenv("ZFP_HIP_OVF_POOL"))
        t_full_slot_calls4 = kFullSlotCalls4;
      continue;
    }
    if (rc != 1 || !a.ovf)
      return rc;
    if constexpr (!kIntField<S>) {
      uint32_t n = 0;
      HIP_TRY(hipMemcpyAsync(&n, a.ovf_count, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (n) {
        const size_t plds = (size_t)kEnc4HeadWords * 8 + std::max<size_t>((size_t)kBlocks4PerWave * swp_full * 8, xfull);
        const dim3 pg((n + kBlocks4PerWave - 1) / kBlocks4PerWave), pb(64);
        const OvfEntry* list = (const OvfEntry*)a.ovf;
        launch_encode4_patch(Launch{pg, pb, plds, c->stream}, p.vec, p.cp.minexp < kMinExp, d_field, p.g, p.cp, d_out,
                             list, n, swp_full);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev[2], c->stream));
      }
    }
    return 1;
  }
  return fail("zfp_hip: overflow pool exhausted with full-size slots");
}

// LDS slots of the aligned kernels: one of sdw dwords per lane (dwords from 2 sw on are spare)
static uint32_t aligned_slot_dwords(const Plan& p) { return slot_dwords_for(p.cp.maxbits) | 1u; }
static size_t aligned_lds_bytes(const Plan& p) { return (size_t)kWavesPerGroup * 64 * aligned_slot_dwords(p) * 4; }

// launch_encode queues one kernel between ev[1] and ev[2] and nothing else:
// the aligned fixed-rate path (the condition below) at a word-aligned start.
// A block too long for the aligned slots (above 77 words: float rate 80) takes the
// general path, whose slots are sized by what a block can code, not by its padding.
static bool aligned_encode(const Plan& p)
{
  return p.type >= 3 && p.fixed && (p.cp.maxbits % 64) == 0 && p.dims == 3 &&
         (p.dbl ? fixed_rate_coder_applies<double>(p.cp) : fixed_rate_coder_applies<float>(p.cp)) &&
         aligned_lds_bytes(p) + sizeof(CoderTables) <= 160 * 1024;  // the kernels' static LDS: the coder tables
}

static bool one_kernel_encode(const Plan& p, uint32_t g0) { return g0 == 0 && aligned_encode(p); }

template <typename S>
static int launch_encode(Ctx* c, const Plan& p, const S* d_field, uint64_t* d_out, uint32_t g0,
                         const Head& head, IndexView* index, uint64_t* total_bits)
{
  if (p.dims == 4)
    return run_encode4<S>(c, p, d_field, d_out, g0, head, index, total_bits);
  const uint64_t nwaves = p.nwaves;
  const uint64_t ngroups = (nwaves + kWavesPerGroup - 1) / kWavesPerGroup;
  if (ngroups > 0x7fffffffull)
    return fail("zfp_hip: field too large for one launch");
  dim3 grid((unsigned)ngroups), block(256);
  // aligned fixed-rate kernel: word-multiple blocks and no precision limit
  // below the integer width (its coder runs every plane until the budget)
  if constexpr (!kIntField<S>)
  if (aligned_encode(p)) {
    const uint32_t sw = p.cp.maxbits / 64;
    const uint32_t sdw = aligned_slot_dwords(p);
    auto magic_of = [](uint32_t d) { return d > 1 ? (uint32_t)((0x100000000ull + d - 1) / d) : 0u; };
    const uint32_t magic_w = magic_of(sw), magic_c = (sw & 1) ? 0u : magic_of(sw / 2);
    const size_t lds = aligned_lds_bytes(p);
    Partial* parts = nullptr;
    if (g0) {
      if (!ensure(c->partials, nwaves * 2 * sizeof(Partial)))
        return 0;
      parts = (Partial*)c->partials.p;
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    launch_encode3_aligned(Launch{grid, block, lds, c->stream}, p.vec, d_field, p.g, p.cp, d_out, sw, sdw, magic_w,
                           magic_c, g0, parts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    if (g0) {
      launch_fixups(c, p, parts, d_out, g0, head);
      HIP_TRY(hipGetLastError());
    }
    *total_bits = p.g.nblocks * (uint64_t)p.cp.maxbits;
    c->single_kernel = g0 == 0;
    return 1;
  }
  // general path
  const uint32_t swp_full = (uint32_t)slot_words_odd(p.bound_bits);
  const uint32_t swp_short = short_slot_words<S>(p);
  for (int attempt = 0; attempt < 2; attempt++) {
    const uint32_t swp = attempt == 0 ? std::min(swp_full, swp_short) : swp_full;
    size_t lds = (size_t)kWavesPerGroup * gen_wave_words(swp) * 8;
    if (lds + kLutBytes > 160 * 1024)
      return fail("zfp_hip: block bound %u bits too large for LDS", p.bound_bits);
    GeneralArgs a{};
    if (!general_args(c, p, swp, d_out, g0, index, head.idx_add, a))
      return 0;
    if (swp < swp_full) {
      // overflow pool: a sixteenth of the blocks (at least 64K, at most all)
      uint64_t cap = std::min<uint64_t>(p.g.nblocks, std::max<uint64_t>(65536, p.g.nblocks / 16));
      if (const char* e = getenv("ZFP_HIP_OVF_POOL"))  // tests: force the full-slot redo
        cap = std::max<uint64_t>(1, std::min<uint64_t>(cap, (uint64_t)atoll(e)));
      if (!ensure(c->ovf, cap * swp_full * 8))
        return 0;
      a.ovf = (uint64_t*)c->ovf.p;
      a.ovf_count = (uint32_t*)((char*)c->misc.p + 16);
      a.ovf_cap = (uint32_t)cap;
      a.ovf_swp = swp_full;
      a.cap_bits = 64 * swp - 96;  // the clamped writes of an outrun slot land in its last three dwords
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if constexpr (sizeof(S) == 8) {
      if (hi_planes<S>(p))
        launch_general3<S, true>(c, p, d_field, grid, block, lds, a);
      else
        launch_general3<S, false>(c, p, d_field, grid, block, lds, a);
    } else {
      launch_general3<S, false>(c, p, d_field, grid, block, lds, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    const int rc = finish_general(c, p, d_out, g0, head, a, index, total_bits);
    if (rc != kRedoFullSlots)
      return rc;
  }
  return fail("zfp_hip: overflow pool exhausted with full-size slots");
}

// What every decode launch is given: the stream, the rate and, for a
// variable-rate stream, the index with its check word.  W: words staged per block.
static DecodeArgs decode_args(const Ctx* c, const Plan& p, const uint64_t* d_in, uint64_t in_words, uint32_t g0,
                              const IndexView* index, uint32_t W)
{
  DecodeArgs a{};
  a.in = d_in;
  a.in_words = in_words;
  a.g0 = g0;
  a.var = p.fixed ? 0 : 1;
  a.maxbits = p.cp.maxbits;
  a.idx_bad = p.fixed ? nullptr : c->idx_chk;
  a.W = W;
  a.swp = a.W | 1;
  a.wmagic = (uint32_t)((0x100000000ull + a.W - 1) / a.W);
  if (!p.fixed) {
    a.idx_len = index->d_len;
    a.idx_base = index->d_base;
  }
  return a;
}

template <typename S>
static int run_decode4(Ctx* c, const Plan& p, S* d_field, const uint64_t* d_in, uint64_t in_words, uint32_t g0,
                          const IndexView* index)
{
  using Int = typename Traits<S>::Int;
  const uint64_t nwaves = p.nwaves;
  if (nwaves > 0x7fffffffull)
    return fail("zfp_hip: field too large for one launch");
  if (!p.fixed && index->nwaves != nwaves)
    return fail("zfp_hip: block index has %llu waves, the 4D layout needs %llu", (unsigned long long)index->nwaves,
                (unsigned long long)nwaves);
  const uint32_t per_block = p.fixed ? p.cp.maxbits : p.max_len;
  // peek64 at the budget end reads one word past it
  DecodeArgs a = decode_args(c, p, d_in, in_words, g0, index, (per_block + 63) / 64 + 1);
  // f32/f64: exchange areas shared by quad pairs (HALF), as in the encoder
  const bool half = !kIntField<S>;
  const size_t xfull = (size_t)kBlocks4PerWave * kXStride * sizeof(Int);
  // variable rate, f32/f64: the wave's segment (its 16 blocks, contiguous in
  // the stream) staged back to back in what the kernel's VGPR-bound number of
  // waves per CU leaves of the LDS (kDec4WavesPerCu); the staging reads only
  // the segment's words, where padded slots read 16 worst-case blocks' worth
  // for every wave.  A wave whose segment does not fit (runs of long blocks: on
  // the C5 field 2.6 % of the waves at 16 waves per CU) goes on a list that a
  // second launch decodes with padded slots.  ZFP_HIP_PACK_WORDS=n stages n words instead
  // (tests: many waves take the second launch); ZFP_HIP_FULL_SLOTS=1 padded
  // slots only.
  uint32_t packw = 0;
  if (!p.fixed && half && !getenv("ZFP_HIP_FULL_SLOTS")) {
    const uint32_t waves_per_cu = kDec4WavesPerCu<S>;
    const uint32_t fit = (uint32_t)(((160u * 1024u) / waves_per_cu - kDec4HeadWords * 8) / 8);
    const uint32_t worst = (uint32_t)((126ull + (uint64_t)kBlocks4PerWave * per_block) / 64 + 1);
    packw = std::min(fit, worst);
    // incompressible data (a reversible stream of noise: every block ~8,300
    // bits) puts nearly every wave past `fit`, and the second launch would
    // redo all of them: when the index's mean segment does not fit, stage
    // segments of the mean + 1/6 in the first launch, widened to what its
    // number of waves per CU allows (128^4 f32 noise, reversible: 2.44 ->
    // 1.8 ms; the smooth C5 field keeps `fit`)
    const uint64_t mean = index->total_bits / std::max<uint64_t>(nwaves, 1) / 64 + 2;
    if (mean * 10 > (uint64_t)packw * 9) {
      const uint64_t want = std::min<uint64_t>(worst, mean + mean / 6 + 8);
      const uint64_t per_cu = std::max<uint64_t>(1, (160u * 1024u) / ((uint64_t)kDec4HeadWords * 8 + want * 8));
      packw = (uint32_t)std::min<uint64_t>(worst, ((160u * 1024u) / per_cu - (uint64_t)kDec4HeadWords * 8) / 8);
    }
    if (const char* e = getenv("ZFP_HIP_PACK_WORDS"))
      packw = (uint32_t)atoi(e);
    if ((size_t)packw * 8 < xfull / 2)
      packw = (uint32_t)(xfull / 16);  // the exchange areas need that much anyway
    if ((size_t)kDec4HeadWords * 8 + (size_t)packw * 8 > 160 * 1024)
      packw = 0;
  }
  const bool rev = p.cp.minexp < kMinExp;
  auto launch = [&](uint32_t pw, dim3 grid) -> int {
    a.packw = pw;
    const size_t region = pw ? std::max<size_t>((size_t)pw * 8, xfull / 2)
                             : std::max<size_t>((size_t)kBlocks4PerWave * a.swp * 8, half ? xfull / 2 : xfull);
    const size_t lds = (size_t)kDec4HeadWords * 8 + region;
    if (lds > 160 * 1024)
      return fail("zfp_hip: 4D block size too large for LDS staging (%u bits)", per_block);
    if constexpr (kIntField<S>)
      launch_decode4_int(p.type, rev, p.vec, c->stream, grid, dim3(64), lds, d_field, p.g, p.cp, a);
    else
      launch_decode4(Launch{grid, dim3(64), lds, c->stream}, p.vec, rev, d_field, p.g, p.cp, a);
    HIP_TRY(hipGetLastError());
    return 1;
  };
#ifdef ZFP_EXP4_TRACE
  const size_t ntr = (nwaves + 63) / 64 * 8;
  uint64_t* d_tr = nullptr;
  if (getenv("ZFP_HIP_TRACE4")) {
    HIP_TRY(hipMalloc(&d_tr, ntr * 8));
    HIP_TRY(hipMemsetAsync(d_tr, 0, ntr * 8, c->stream));
  }
  a.trace = d_tr;
  struct TraceDump {
    Ctx* c; uint64_t* d; size_t n;
    ~TraceDump() {
      if (!d) return;
      std::vector<uint64_t> h(n);
      if (hipMemcpyAsync(h.data(), d, n * 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
          hipStreamSynchronize(c->stream) == hipSuccess) {
        // slots: 0 staged, 2..5 decode_block4 marks (parse, planes->coefficients, exchange, lift),
        // 1 decoded, 7 scattered
        const int order[7] = {0, 2, 3, 4, 5, 1, 7};
        double sum[7] = {0};
        size_t cnt = 0;
        for (size_t i = 0; i + 8 <= n; i += 8) {
          if (!h[i + 6]) continue;
          cnt++;
          uint64_t prev = 0;
          for (int k = 0; k < 7; k++) { sum[k] += (double)(h[i + order[k]] - prev); prev = h[i + order[k]]; }
        }
        if (cnt)
          fprintf(stderr, "dtrace4 waves %zu (100 MHz ticks, mean): stage %.1f parse %.1f planes->coeffs %.1f "
                  "exchange %.1f lift %.1f cast %.1f scatter %.1f\n", cnt, sum[0] / cnt, sum[1] / cnt,
                  sum[2] / cnt, sum[3] / cnt, sum[4] / cnt, sum[5] / cnt, sum[6] / cnt);
      }
      (void)hipFree(d);
    }
  } dump{c, d_tr, ntr};
#endif
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  if (!packw) {
    if (!launch(0, dim3((unsigned)nwaves)))
      return 0;
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    return 1;
  }
  // misc: [12] error, [16] list count; ovf: the wave list
  if (!ensure(c->misc, 64) || !ensure(c->ovf, nwaves * 4))
    return 0;
  HIP_TRY(hipMemsetAsync(c->misc.p, 0, 64, c->stream));
  a.error = (uint32_t*)((char*)c->misc.p + 12);
  a.ovf_count = (uint32_t*)((char*)c->misc.p + 16);
  a.wave_ovf = (uint32_t*)c->ovf.p;
  a.ovf_cap = (uint32_t)nwaves;
  if (!launch(packw, dim3((unsigned)nwaves)))
    return 0;
  uint32_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, a.ovf_count, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n) {
    // the listed waves again, their segments staged whole: sized for sixteen
    // worst-case blocks, so every segment fits (a wave that still did not --
    // an index entry past the block bound -- flags an error instead of
    // listing itself); fewer waves per CU, but only the segment's words are
    // read, where padded slots read sixteen worst-case blocks' worth
    const uint32_t worst = (uint32_t)((126ull + (uint64_t)kBlocks4PerWave * per_block) / 64 + 1);
    const bool packed2 = packw && (size_t)kDec4HeadWords * 8 + (size_t)worst * 8 <= 160 * 1024 &&
                         !getenv("ZFP_HIP_OVF_PADDED");
    if (getenv("ZFP_HIP_VERBOSE"))
      fprintf(stderr, "zfp_hip: decode4: %u of %llu wave segments past %u staged words, decoded %s\n", n,
              (unsigned long long)nwaves, packw, packed2 ? "from whole segments" : "with padded slots");
    a.wave_list = a.wave_ovf;
    a.ovf_cap = 0;
    if (!launch(packed2 ? worst : 0u, dim3(n)))
      return 0;
    a.wave_list = nullptr;
    // a listed wave whose segment still did not fit was left undecoded: its
    // index entries exceed the block bound.  With the index under check
    // (always, for variable rate) the kernel has marked it stale, and the
    // caller rescans; otherwise the call fails.
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, a.error, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err && !c->idx_chk)
      return fail("zfp_hip: decode4: a wave segment exceeds sixteen worst-case blocks (corrupt index)");
  }
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  return 1;
}


// Short staging slots for the variable-rate 3D decoder (the encoder's rule,
// short_slot_words): words staged per block such that the kernel's VGPR-bound
// number of workgroups fits the CU's LDS; longer blocks are staged in global
// memory.  ~0u: full size.
template <typename S>
static uint32_t short_stage_words(const Plan& p)
{
  if (p.fixed || p.dims != 3 || kIntField<S> || getenv("ZFP_HIP_FULL_SLOTS"))
    return ~0u;
  if (!hi_planes<S>(p))  // the only decoder instantiated with short slots
    return ~0u;
  if (const char* e = getenv("ZFP_HIP_SLOT_WORDS"))  // tests: force overflows
    return (uint32_t)atoi(e) | 1u;
  const int groups = 3;
  const int64_t words = ((int64_t)(160 * 1024) / groups - (int64_t)kLutBytes - kWavesPerGroup * 64 * 4) / 8 /
                        (kWavesPerGroup * 64);
  const int64_t W = (words & 1) ? words : words - 1;
  return W < 3 ? ~0u : (uint32_t)W;
}

template <typename S>
static int launch_decode(Ctx* c, const Plan& p, S* d_field, const uint64_t* d_in, uint64_t in_words, uint32_t g0,
                         const IndexView* index)
{
  if (p.dims == 4)
    return run_decode4<S>(c, p, d_field, d_in, in_words, g0, index);
  const uint64_t nwaves = p.nwaves;
  if (!p.fixed && index->nwaves != nwaves)
    return fail("zfp_hip: block index has %llu waves, the 3D layout needs %llu", (unsigned long long)index->nwaves,
                (unsigned long long)nwaves);
  const uint64_t ngroups = (nwaves + kWavesPerGroup - 1) / kWavesPerGroup;
  // what a block can code: the decoder reads no further (minbits or fixed-rate
  // padding past it is skipped, not read), so the padding is not staged
  const uint32_t per_block = p.bound_bits;
  const uint32_t W_full = (per_block + 63) / 64 + 1;  // peek64 at the budget end reads one word past it
  const uint32_t W_short = short_stage_words<S>(p);
  for (int attempt = 0; attempt < 2; attempt++) {
    DecodeArgs a = decode_args(c, p, d_in, in_words, g0, index, attempt == 0 ? std::min(W_full, W_short) : W_full);
    size_t lds = (size_t)kWavesPerGroup * 64 * a.swp * 8;
    if (lds + kLutBytes + kWavesPerGroup * 64 * 4 > 160 * 1024)
      return fail("zfp_hip: block size too large for LDS staging (%u bits)", per_block);
    if (a.W < W_full) {
      uint64_t cap = std::min<uint64_t>(p.g.nblocks, std::max<uint64_t>(65536, p.g.nblocks / 16));
      if (const char* e = getenv("ZFP_HIP_OVF_POOL"))
        cap = std::max<uint64_t>(1, std::min<uint64_t>(cap, (uint64_t)atoll(e)));
      if (!ensure(c->ovf, cap * W_full * 8) || !ensure(c->misc, 64))
        return 0;
      HIP_TRY(hipMemsetAsync(c->misc.p, 0, 64, c->stream));
      a.ovf = (uint64_t*)c->ovf.p;
      a.ovf_count = (uint32_t*)((char*)c->misc.p + 16);
      a.error = (uint32_t*)((char*)c->misc.p + 12);
      a.ovf_cap = (uint32_t)cap;
      a.ovf_W = W_full;
      a.cap_bits = (a.W - 1) * 64;
    }
    dim3 grid((unsigned)ngroups), block(256);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if constexpr (sizeof(S) == 8) {
      if (hi_planes<S>(p))
        run_decode3<S, true>(c, p, d_field, grid, block, lds, a);
      else
        run_decode3<S, false>(c, p, d_field, grid, block, lds, a);
    } else {
      run_decode3<S, false>(c, p, d_field, grid, block, lds, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    if (!a.ovf)
      return 1;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, a.error, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!(err & 2u))
      return 1;
  }
  return fail("zfp_hip: decode overflow pool exhausted with full-size slots");
}

static void record_timing(Ctx* c)
{
  float k = 0, t = 0;
  if (hipEventElapsedTime(&k, c->ev[1], c->ev[2]) == hipSuccess &&
      hipEventElapsedTime(&t, c->ev[c->one_pair ? 1 : 0], c->ev[c->one_pair ? 2 : 3]) == hipSuccess) {
    t_timing.kernel_ms = k;
    t_timing.total_ms = t;
    t_timing.timed = true;
  }
}
