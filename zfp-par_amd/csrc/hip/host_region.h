// Host shim: region decode (zfp_hip_decompress_region) -- validation, the
// cached start table of a block index, staging of a host stream's needed
// words, the launch and the copy-out of a host destination.
#pragma once

#include "host_pipeline.h"
#include "host_scan.h"
#include "kernels_region.h"

// Everything that is checked before any GPU call: pointers, the job, the
// region against the coded box, the dimensionality and the block count.
static int plan_region(const zfp_hip_job* job, const uint64_t* lo, const uint64_t* hi, const void* dst,
                       const int64_t* dst_stride, const uint64_t* words, Plan& p, RegionGeom& rg,
                       const char* who = "zfp_hip_decompress_region", const char* what = "decode")
{
  if (!job || !lo || !hi || !dst || !dst_stride || !words)
    return fail("%s: null job, region, destination, stride or stream pointer", who);
  zfp_hip_job j = *job;  // (job->s is not used: the destination has its own strides)
  for (int a = 0; a < 4; a++)
    j.s[a] = 0;
  if (!plan_job(&j, nullptr, p))
    return 0;
  for (int a = 0; a < p.dims; a++)
    if (!(j.f[a] <= lo[a] && lo[a] < hi[a] && hi[a] <= j.e[a]))
      return fail("%s: region [%llu, %llu) on axis %d is empty or not inside the coded box [%llu, %llu)", who,
                  (unsigned long long)lo[a], (unsigned long long)hi[a], a, (unsigned long long)j.f[a],
                  (unsigned long long)j.e[a]);
  if (p.dims == 4)
    return fail("%s: 4D region %s is not supported (1D to 3D fields only)", who, what);
  rg = make_region_geom(p.g, p.dims, lo, hi, dst_stride);
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

// Dense device image of the region -> the host destination with its strides.
// (copy_box is not used: it needs the device image laid out with the host's
// strides, and the span of a thin region inside a large array is nearly the
// whole array.)  Other threads may be writing neighbouring elements of the
// same array: only the region's bytes are written.
static int region_to_host(Ctx* c, const Plan& p, const RegionGeom& rg, const int64_t* hs, void* h_dst,
                          const void* d_img)
{
  uint64_t ext[3] = {1, 1, 1};
  for (int a = 0; a < p.dims; a++)
    ext[a] = rg.hi[a] - rg.lo[a];
  const size_t es = p.es, row = (size_t)ext[0] * es, bytes = row * ext[1] * ext[2];
  const bool dense = hs[0] == 1 && (p.dims < 2 || hs[1] == (int64_t)ext[0]) &&
                     (p.dims < 3 || hs[2] == (int64_t)(ext[0] * ext[1]));
  if (dense)
    return copy_to_host_exact(h_dst, d_img, bytes, c->stream, c);
  std::vector<char> tmp(bytes);
  HIP_TRY(hipMemcpyAsync(tmp.data(), d_img, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int64_t sy = p.dims > 1 ? hs[1] : 0, sz = p.dims > 2 ? hs[2] : 0;
  for (uint64_t z = 0; z < ext[2]; z++)
    for (uint64_t y = 0; y < ext[1]; y++) {
      const char* s = tmp.data() + (z * ext[1] + y) * row;
      char* d = (char*)h_dst + ((int64_t)y * sy + (int64_t)z * sz) * (int64_t)es;
      if (hs[0] == 1)
        memcpy(d, s, row);
      else
        for (uint64_t x = 0; x < ext[0]; x++)
          memcpy(d + (int64_t)x * hs[0] * (int64_t)es, s + x * es, es);
    }
  return 1;
}

// The stream side of a region decode, shared by the single and the batched
// call: the check word of a variable-rate index, ev[0], the stream on the
// device and the kernel's RegionArgs.  [Blo, Bhi]: the lowest and highest
// stream block needed.  A fixed-rate host stream is staged from Blo's first
// word to Bhi's last plus the decoder's one look-ahead word, with bit0 rebased;
// a variable-rate one whole, and its index is the caller's when it matches,
// the scan's otherwise (*scanned), with its start table.  *lds: the dynamic
// LDS of the launch.
static int region_stream(Ctx* c, const Plan& p, uint64_t Blo, uint64_t Bhi, const uint64_t* words,
                         uint64_t capacity_words, uint64_t bit_offset, const zfp_hip_index* index, bool plain_scan,
                         bool* scanned, RegionArgs& a, size_t* lds)
{
  const bool dev_stream = is_device_ptr(words);
  const bool have_index = !p.fixed && index_matches(c, index, p, words, dev_stream, capacity_words, bit_offset);
  const bool scan = !p.fixed && !have_index;
  *scanned = scan;
  c->idx_chk = nullptr;
  if (!p.fixed) {
    if (!ensure(c->chk, 8))
      return 0;
    HIP_TRY(hipMemsetAsync(c->chk.p, 0, 4, c->stream));
    c->idx_chk = (uint32_t*)c->chk.p;
  }
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  a = RegionArgs{};
  a.var = p.fixed ? 0 : 1;
  a.maxbits = p.cp.maxbits;
  a.idx_bad = c->idx_chk;
  if (p.fixed) {
    a.in = words;
    a.in_words = capacity_words;
    a.bit0 = bit_offset;
    if (!dev_stream) {
      const uint64_t Wf = (bit_offset + Blo * (uint64_t)p.cp.maxbits) >> 6;
      const uint64_t We = std::min<uint64_t>(((bit_offset + (Bhi + 1) * (uint64_t)p.cp.maxbits + 63) >> 6) + 1,
                                             capacity_words);
      const uint64_t n = We > Wf ? We - Wf : 0;
      if (!ensure(c->words, n * 8 + 8))
        return 0;
      if (n && !h2d(c, c->words.p, words + Wf, n * 8, c->stream))
        return 0;
      a.in = (const uint64_t*)c->words.p;
      a.in_words = n;
      a.bit0 = bit_offset - 64 * Wf;  // modulo 2^64 (RegionArgs::bit0)
    }
  } else {
    const StreamPos at(bit_offset, capacity_words);
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
      if (!scan_index(c, p, d_in, nwords, at.g0, &c->scan_index, plain_scan))
        return 0;
      c->scan_index.start_bit = bit_offset;
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
  const uint32_t per_block = p.fixed ? p.cp.maxbits : p.max_len;
  a.W = (per_block + 63) / 64 + 1;  // peek64 at the budget end reads one word past it
  a.swp = a.W | 1;
  a.wmagic = (uint32_t)((0x100000000ull + a.W - 1) / a.W);
  *lds = (size_t)kWavesPerGroup * 64 * a.swp * 8;
  if (*lds + kLutBytes + kWavesPerGroup * 64 * 8 > 160 * 1024)
    return fail("zfp_hip: block size too large for LDS staging (%u bits)", per_block);
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

// After the launch (ev[2] recorded): the check word's copy is queued, to be
// fetched with the call's last synchronize (*pchk; nullptr: region_finish
// fetches it with a copy of its own).
static int region_queue_check(Ctx* c, const uint32_t** pchk)
{
  *pchk = nullptr;
  if (c->idx_chk) {
    uint32_t* q = (uint32_t*)pin_take(c, 4);
    if (q) {
      HIP_TRY(hipMemcpyAsync(q, c->chk.p, 4, hipMemcpyDeviceToHost, c->stream));
      *pchk = q;
    }
  }
  return 1;
}

// The end of a region decode: ev[3], the synchronize, the timing and the
// verdict of the check word (*stale).
static int region_finish(Ctx* c, const uint32_t* pchk, bool* stale)
{
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  record_timing(c);
  if (c->idx_chk) {
    uint32_t bad = 0;
    c->idx_chk = nullptr;
    if (pchk) {
      bad = *pchk;
    } else {
      HIP_TRY(hipMemcpyAsync(&bad, c->chk.p, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (bad)
      *stale = true;
  }
  return 1;
}

// One region decode with the given index (nullptr: the stream is scanned);
// *stale and *scanned as decompress_once.
static int region_once(Ctx* c, const Plan& p, RegionGeom rg, void* dst, const int64_t* dst_stride,
                       const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                       const zfp_hip_index* index, bool plain_scan, bool* stale, bool* scanned)
{
  const bool dev_dst = is_device_ptr(dst);
  uint64_t Blo, Bhi;
  region_block_span(p, rg, &Blo, &Bhi);
  RegionArgs a;
  size_t lds;
  if (!region_stream(c, p, Blo, Bhi, words, capacity_words, bit_offset, index, plain_scan, scanned, a, &lds))
    return 0;
  // destination: the caller's device array, or a dense image of the region
  void* d_dst = dst;
  if (!dev_dst) {
    uint64_t count = 1;
    for (int k = 0; k < p.dims; k++) {
      rg.ds[k] = (int64_t)count;
      count *= rg.hi[k] - rg.lo[k];
    }
    if (!ensure(c->field, count * p.es))
      return 0;
    d_dst = c->field.p;
  }
  rg.vec = region_vec_ok(rg, p.dims, d_dst) ? 1u : 0u;
  const dim3 grid((unsigned)((rg.nrblocks + 64 * kWavesPerGroup - 1) / (64 * kWavesPerGroup)));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  launch_decode_region(p.type, p.dims, p.cp.minexp < kMinExp, hi_planes<double>(p) && p.type == 4, c->stream, grid,
                       lds, d_dst, p.g, p.cp, rg, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  const uint32_t* pchk;
  if (!region_queue_check(c, &pchk))
    return 0;
  if (!dev_dst && !region_to_host(c, p, rg, dst_stride, dst, d_dst))
    return 0;
  return region_finish(c, pchk, stale);
}
