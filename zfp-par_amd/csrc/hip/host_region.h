// Host shim: region decode (zfp_hip_decompress_region) and what the batched
// decode and the region encode share with it -- validation against the coded
// box, the cached start table of a block index, staging of a host stream's
// needed words, the slot geometry, the dense image and the strided copy of a
// host array, and the one launch-and-finish of the two decoders.
#pragma once

#include "host_call.h"
#include "host_pipeline.h"
#include "host_rows.h"
#include "host_scan.h"
#include "kernels_region.h"

// The coded box of a region call: `j` is the job without its strides (every
// destination or source has its own), `p` its plan.  4D is refused.
static int plan_coded_box(const char* who, const char* what, const zfp_hip_job* job, Plan& p, zfp_hip_job& j)
{
  j = *job;
  for (int a = 0; a < 4; a++)
    j.s[a] = 0;
  if (!plan_job(&j, nullptr, p))
    return 0;
  if (p.dims == 4)
    return fail("%s: 4D region %s is not supported (1D to 3D fields only)", who, what);
  return 1;
}

// [lo, hi) must be a non-empty part of the coded box on every axis.
// entry_prefix: "" or the batch's "regions[i] (entry i+1 of n): ".
static int check_region_box(const char* who, const char* entry_prefix, const zfp_hip_job& j, int dims,
                            const uint64_t* lo, const uint64_t* hi)
{
  for (int a = 0; a < dims; a++)
    if (!(j.f[a] <= lo[a] && lo[a] < hi[a] && hi[a] <= j.e[a]))
      return fail("%s: %sregion [%llu, %llu) on axis %d is empty or not inside the coded box [%llu, %llu)", who,
                  entry_prefix, (unsigned long long)lo[a], (unsigned long long)hi[a], a, (unsigned long long)j.f[a],
                  (unsigned long long)j.e[a]);
  return 1;
}

// Everything that is checked before any GPU call: pointers, the job, the
// region against the coded box, the dimensionality and the block count.
// (`mem`: the destination, or the region encoder's source.)
static int plan_region(const zfp_hip_job* job, const uint64_t* lo, const uint64_t* hi, const void* mem,
                       const int64_t* mem_stride, const uint64_t* words, Plan& p, RegionGeom& rg,
                       const char* who = "zfp_hip_decompress_region", const char* what = "decode",
                       const char* mem_name = "destination")
{
  if (!job || !lo || !hi || !mem || !mem_stride || !words)
    return fail("%s: null job, region, %s, stride or stream pointer", who, mem_name);
  zfp_hip_job j;
  if (!plan_coded_box(who, what, job, p, j) || !check_region_box(who, "", j, p.dims, lo, hi))
    return 0;
  rg = make_region_geom(p.g, p.dims, lo, hi, mem_stride);
  if (rg.nrblocks > 0xffffffffull)  // (three factors below 2^32 whose product divides the box's block count)
    return fail("%s: %llu region blocks in one call (at most 2^32 - 1)", who, (unsigned long long)rg.nrblocks);
  return 1;
}

// The start table of `x` (kernels_region.h), built on first use and kept until
// the index is refilled (index_reserve) or released.  Calls on different
// threads may share an index: one of them builds, under the lock, and has
// synchronized before the others read the table from their own streams.
static std::mutex g_start_mu;

static int ensure_start_table(Ctx* c, const zfp_hip_index* x)
{
  std::lock_guard<std::mutex> lk(g_start_mu);
  if (x->start_valid)
    return 1;
  if (x->cap_start < x->nblocks) {
    if (x->d_start) (void)hipFree(x->d_start);
    x->d_start = nullptr;
    x->cap_start = 0;
    if (hipMalloc(&x->d_start, std::max<uint64_t>(x->nblocks, 1) * sizeof(uint64_t)) != hipSuccess)
      return fail("hipMalloc of the start table (%llu blocks) failed", (unsigned long long)x->nblocks);
    x->cap_start = x->nblocks;
  }
  launch_start_table(c->stream, x->d_len, x->d_base, x->nblocks, x->nwaves, x->per_wave, x->d_start);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  x->start_valid = true;
  return 1;
}

// The dense image of a region (x fastest, no gaps): rg.ds becomes its
// strides; returns its bytes.
static size_t dense_image(RegionGeom& rg, int dims, size_t es)
{
  uint64_t count = 1;
  for (int k = 0; k < dims; k++) {
    rg.ds[k] = (int64_t)count;
    count *= rg.hi[k] - rg.lo[k];
  }
  return (size_t)count * es;
}

// The region's extents for host_rows.h; returns the bytes of its dense image.
static size_t region_extents(const RegionGeom& rg, int dims, size_t es, uint64_t ext[3])
{
  for (int a = 0; a < 3; a++)
    ext[a] = a < dims ? rg.hi[a] - rg.lo[a] : 1;
  return (size_t)(ext[0] * ext[1] * ext[2]) * es;
}

// Dense device image of the region -> the host destination with its strides.
// (copy_box is not used: it needs the device image laid out with the host's
// strides, and the span of a thin region inside a large array is nearly the
// whole array.)  Other threads may be writing neighbouring elements of the
// same array: only the region's bytes are written.
static int region_to_host(Ctx* c, const Plan& p, const RegionGeom& rg, const int64_t* hs, void* h_dst,
                          const void* d_img)
{
  uint64_t ext[3];
  const size_t bytes = region_extents(rg, p.dims, p.es, ext);
  if (region_is_dense(ext, p.dims, hs))
    return copy_to_host_exact(h_dst, d_img, bytes, c->stream, c);
  std::vector<char> tmp(bytes);
  HIP_TRY(hipMemcpyAsync(tmp.data(), d_img, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  region_rows(ext, p.dims, p.es, hs, h_dst, tmp.data(), true);
  return 1;
}

// First and last block of the region in the stream (raster order of the coded box)
static void region_block_span(const Plan& p, const RegionGeom& rg, uint64_t* Blo, uint64_t* Bhi)
{
  uint64_t mul = 1;
  *Blo = *Bhi = 0;
  for (int k = 0; k < 3; k++) {
    *Blo += mul * rg.rb0[k];
    *Bhi += mul * (rg.rb0[k] + rg.rnb[k] - 1);
    mul *= p.g.nb[k];
  }
}

// A fixed-rate host stream goes to the device from the first word of block
// Blo (*Wf) to the last word of block Bhi, *n words in c->words, with the
// position rebased to them (*bit0).  lookahead: plus the decoder's one
// look-ahead word, cut at the capacity; the encoder's span is not cut
// (plan_region_enc: it lies below the capacity).
static int stage_fixed_span(Ctx* c, const Plan& p, uint64_t Blo, uint64_t Bhi, const uint64_t* words,
                            uint64_t capacity_words, uint64_t bit_offset, bool lookahead, uint64_t* Wf, uint64_t* n,
                            uint64_t* bit0)
{
  *Wf = (bit_offset + Blo * (uint64_t)p.cp.maxbits) >> 6;
  uint64_t We = (bit_offset + (Bhi + 1) * (uint64_t)p.cp.maxbits + 63) >> 6;
  if (lookahead)
    We = std::min<uint64_t>(We + 1, capacity_words);
  *n = We > *Wf ? We - *Wf : 0;
  if (!ensure(c->words, *n * 8 + 8))
    return 0;
  if (*n && !h2d(c, c->words.p, words + *Wf, *n * 8, c->stream))
    return 0;
  *bit0 = bit_offset - 64 * *Wf;  // modulo 2^64 (RegionArgs::bit0)
  return 1;
}

// One LDS slot per lane: W words hold a block of per_block_bits and the word
// peek64 reads past its end, the stride swp is odd and at least
// min_slot_words (the encoder's coder), lds the launch's dynamic LDS.
// table_bytes: the kernel's static coder tables.
struct RegionSlots {
  uint32_t W, swp, wmagic;
  size_t lds;
};

static int region_slots(uint32_t per_block_bits, size_t min_slot_words, size_t table_bytes, RegionSlots& s)
{
  s.W = (per_block_bits + 63) / 64 + 1;
  s.swp = (uint32_t)std::max<size_t>(min_slot_words, s.W) | 1u;
  s.wmagic = (uint32_t)((0x100000000ull + s.W - 1) / s.W);
  s.lds = (size_t)kWavesPerGroup * 64 * s.swp * 8;
  if (s.lds + table_bytes + kWavesPerGroup * 64 * 8 > 160 * 1024)
    return fail("zfp_hip: block size too large for LDS staging (%u bits)", per_block_bits);
  return 1;
}

// The stream and the index of one attempt of a decode (with_stale_retry):
// index nullptr: the stream is scanned; *stale and *scanned as decompress_once.
struct DecodeTry {
  const uint64_t* words;
  uint64_t capacity_words, bit_offset;
  const zfp_hip_index* index;
  bool plain_scan;
  bool* stale;
  bool* scanned;
};

// The stream side of a region decode: the check word of a variable-rate
// index, ev[0], the stream on the device and the kernel's RegionArgs.
// [Blo, Bhi]: the lowest and highest stream block needed.  A fixed-rate host
// stream is staged by stage_fixed_span; a variable-rate one whole, and its
// index is the caller's when it matches, the scan's otherwise (*t.scanned),
// with its start table.  *lds: the dynamic LDS of the launch.
static int region_stream(Ctx* c, const Plan& p, const DecodeTry& t, CheckWord& chk, uint64_t Blo, uint64_t Bhi,
                         RegionArgs& a, size_t* lds)
{
  const uint64_t* words = t.words;
  const zfp_hip_index* index = t.index;
  const bool dev_stream = is_device_ptr(words);
  const bool have_index = !p.fixed && index_matches(c, index, p, words, dev_stream, t.capacity_words, t.bit_offset);
  const bool scan = !p.fixed && !have_index;
  *t.scanned = scan;
  if (!chk.arm(p.fixed))
    return 0;
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  a = RegionArgs{};
  a.var = p.fixed ? 0 : 1;
  a.maxbits = p.cp.maxbits;
  a.idx_bad = c->idx_chk;
  if (p.fixed) {
    a.in = words;
    a.in_words = t.capacity_words;
    a.bit0 = t.bit_offset;
    if (!dev_stream) {
      uint64_t Wf;
      if (!stage_fixed_span(c, p, Blo, Bhi, words, t.capacity_words, t.bit_offset, true, &Wf, &a.in_words, &a.bit0))
        return 0;
      a.in = (const uint64_t*)c->words.p;
    }
  } else {
    const StreamPos at(t.bit_offset, t.capacity_words);
    const uint64_t nwords = at.decode_words(have_index ? index->total_bits : p.g.nblocks * (uint64_t)p.max_len);
    const uint64_t* d_in = words + at.W0;
    if (!dev_stream) {  // (a variable-rate host stream is staged whole)
      if (!ensure(c->words, nwords * 8 + 8))
        return 0;
      if (!h2d(c, c->words.p, words + at.W0, nwords * 8, c->stream))
        return 0;
      d_in = (const uint64_t*)c->words.p;
    }
    if (scan) {
      if (!scan_index(c, p, d_in, nwords, at.g0, &c->scan_index, t.plain_scan))
        return 0;
      c->scan_index.start_bit = t.bit_offset;
      index = &c->scan_index;
    }
    if (index->nwaves != p.nwaves)
      return fail("zfp_hip: block index has %llu waves, the layout needs %llu", (unsigned long long)index->nwaves,
                  (unsigned long long)p.nwaves);
    if (!ensure_start_table(c, index))
      return 0;
    a.in = d_in;
    a.in_words = nwords;
    a.bit0 = at.g0;
    a.idx_len = index->d_len;
    a.start = index->d_start;
  }
  RegionSlots s;
  if (!region_slots(p.fixed ? p.cp.maxbits : p.max_len, 0, kLutBytes, s))
    return 0;
  a.W = s.W;
  a.swp = s.swp;
  a.wmagic = s.wmagic;
  *lds = s.lds;
  return 1;
}

// One attempt of a region decode, single or batched, for the blocks [Blo, Bhi]
// of the stream: the stream side, prepare() (the destinations: device memory
// and whatever the kernel needs to find them), ev[1], launch(a, lds), ev[2],
// the check word's copy, copy_out() (host destinations), ev[3], the
// synchronize, the timing and the check word's verdict.
template <typename Prepare, typename Launch, typename CopyOut>
static int region_decode_once(Ctx* c, const Plan& p, const DecodeTry& t, uint64_t Blo, uint64_t Bhi, Prepare&& prepare,
                              Launch&& launch, CopyOut&& copy_out)
{
  CheckWord chk{c};
  RegionArgs a;
  size_t lds;
  if (!region_stream(c, p, t, chk, Blo, Bhi, a, &lds) || !prepare())
    return 0;
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  launch(a, lds);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  if (!chk.queue() || !copy_out())
    return 0;
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  record_timing(c);
  return chk.verdict(t.stale);
}

// One region decode: the destination is the caller's device array, or a dense
// image of the region that is copied out with the caller's strides.
static int region_once(Ctx* c, const Plan& p, RegionGeom rg, void* dst, const int64_t* dst_stride, const DecodeTry& t)
{
  const bool dev_dst = is_device_ptr(dst);
  uint64_t Blo, Bhi;
  region_block_span(p, rg, &Blo, &Bhi);
  void* d_dst = dst;
  return region_decode_once(
      c, p, t, Blo, Bhi,
      [&] {
        if (!dev_dst) {
          if (!ensure(c->field, dense_image(rg, p.dims, p.es)))
            return 0;
          d_dst = c->field.p;
        }
        rg.vec = region_vec_ok(rg, p.dims, d_dst) ? 1u : 0u;
        return 1;
      },
      [&](const RegionArgs& a, size_t lds) {
        const dim3 grid((unsigned)((rg.nrblocks + 64 * kWavesPerGroup - 1) / (64 * kWavesPerGroup)));
        launch_decode_region(p.type, p.dims, p.cp.minexp < kMinExp, hi_planes<double>(p) && p.type == 4, c->stream, grid,
                             lds, d_dst, p.g, p.cp, rg, a);
      },
      [&] { return dev_dst ? 1 : region_to_host(c, p, rg, dst_stride, dst, d_dst); });
}
