// Host shim: region encode (zfp_hip_compress_region) -- validation, the dense
// device image of a host source, staging of a host stream's needed words, the
// launch and the copy-back of those words.
#pragma once

#include "host_region.h"
#include "kernels_region_enc.h"

// Everything that is checked before any GPU call: plan_region's checks, fixed
// rate, and that the stream holds the last needed block's last bit.
static int plan_region_enc(const zfp_hip_job* job, const uint64_t* lo, const uint64_t* hi, const void* src,
                           const int64_t* src_stride, const uint64_t* words, uint64_t capacity_words,
                           uint64_t bit_offset, Plan& p, RegionGeom& rg)
{
  const char* who = "zfp_hip_compress_region";
  if (!job || !lo || !hi || !src || !src_stride || !words)
    return fail("%s: null job, region, source, stride or stream pointer", who);
  if (!plan_region(job, lo, hi, src, src_stride, words, p, rg, who, "encode"))
    return 0;
  if (!p.fixed)
    return fail("%s: a region can be rewritten in a fixed-rate stream only (minbits == maxbits, not reversible): "
                "in a variable-rate stream a block of another length moves every later block", who);
  uint64_t Blo, Bhi;
  region_block_span(p, rg, &Blo, &Bhi);
  // (Bhi + 1) maxbits < 2^32 * 2^32; the sum is checked for wrap-around
  const uint64_t end = bit_offset + (Bhi + 1) * (uint64_t)p.cp.maxbits;
  if (end < bit_offset || capacity_words > (~0ull >> 6) || end > capacity_words * 64)
    return fail("%s: the stream's %llu words end before bit %llu, the end of the region's last block", who,
                (unsigned long long)capacity_words, (unsigned long long)end);
  return 1;
}

// The host source with its strides -> a dense device image of the region (x
// fastest) in the context's field scratch: the inverse of region_to_host.
// `tmp` holds the packed rows of a source that is not dense until the call's
// synchronize.
static int region_from_host(Ctx* c, const Plan& p, const RegionGeom& rg, const int64_t* hs, const void* h_src,
                            void* d_img, std::vector<char>& tmp)
{
  uint64_t ext[3] = {1, 1, 1};
  for (int a = 0; a < p.dims; a++)
    ext[a] = rg.hi[a] - rg.lo[a];
  const size_t es = p.es, row = (size_t)ext[0] * es, bytes = row * ext[1] * ext[2];
  const bool dense = hs[0] == 1 && (p.dims < 2 || hs[1] == (int64_t)ext[0]) &&
                     (p.dims < 3 || hs[2] == (int64_t)(ext[0] * ext[1]));
  if (dense)
    return h2d(c, d_img, h_src, bytes, c->stream);
  tmp.resize(bytes);
  const int64_t sy = p.dims > 1 ? hs[1] : 0, sz = p.dims > 2 ? hs[2] : 0;
  for (uint64_t z = 0; z < ext[2]; z++)
    for (uint64_t y = 0; y < ext[1]; y++) {
      char* d = tmp.data() + (z * ext[1] + y) * row;
      const char* s = (const char*)h_src + ((int64_t)y * sy + (int64_t)z * sz) * (int64_t)es;
      if (hs[0] == 1)
        memcpy(d, s, row);
      else
        for (uint64_t x = 0; x < ext[0]; x++)
          memcpy(d + x * es, s + (int64_t)x * hs[0] * (int64_t)es, es);
    }
  return h2d(c, d_img, tmp.data(), bytes, c->stream);
}

static int region_enc_once(Ctx* c, const Plan& p, RegionGeom rg, const void* src, const int64_t* src_stride,
                           uint64_t* words, uint64_t capacity_words, uint64_t bit_offset)
{
  const bool dev_src = is_device_ptr(src);
  const bool dev_stream = is_device_ptr(words);
  std::vector<char> tmp;
  RegionEncArgs a{};
  a.maxbits = p.cp.maxbits;
  // one LDS slot per lane for the decoder (its look-ahead word included) and
  // the coder; checked before anything is queued
  a.W = (p.cp.maxbits + 63) / 64 + 1;
  a.swp = (uint32_t)std::max<size_t>(slot_words_for(p.bound_bits), a.W) | 1u;
  a.wmagic = (uint32_t)((0x100000000ull + a.W - 1) / a.W);
  const size_t lds = (size_t)kWavesPerGroup * 64 * a.swp * 8;
  if (lds + 2 * kLutBytes + kWavesPerGroup * 64 * 8 > 160 * 1024)
    return fail("zfp_hip: block size too large for LDS staging (%u bits)", p.cp.maxbits);
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  a.out = words;
  a.out_words = capacity_words;
  a.bit0 = bit_offset;
  uint64_t Wf = 0, nspan = 0;
  if (!dev_stream) {
    // the words from the first needed block's first word to the last needed
    // block's last word (plan_region_enc: below the capacity)
    uint64_t Blo, Bhi;
    region_block_span(p, rg, &Blo, &Bhi);
    Wf = (bit_offset + Blo * (uint64_t)p.cp.maxbits) >> 6;
    const uint64_t We = (bit_offset + (Bhi + 1) * (uint64_t)p.cp.maxbits + 63) >> 6;
    nspan = We - Wf;
    if (!ensure(c->words, nspan * 8 + 8))
      return 0;
    if (!h2d(c, c->words.p, words + Wf, nspan * 8, c->stream))
      return 0;
    a.out = (uint64_t*)c->words.p;
    a.out_words = nspan;
    a.bit0 = bit_offset - 64 * Wf;  // modulo 2^64 (RegionArgs::bit0)
  }
  // source: the caller's device array, or a dense image of the region
  const void* d_src = src;
  if (!dev_src) {
    uint64_t count = 1;
    for (int k = 0; k < p.dims; k++) {
      rg.ds[k] = (int64_t)count;
      count *= rg.hi[k] - rg.lo[k];
    }
    if (!ensure(c->field, count * p.es))
      return 0;
    if (!region_from_host(c, p, rg, src_stride, src, c->field.p, tmp))
      return 0;
    d_src = c->field.p;
  }
  rg.vec = region_vec_ok(rg, p.dims, d_src) ? 1u : 0u;
  const dim3 grid((unsigned)((rg.nrblocks + 64 * kWavesPerGroup - 1) / (64 * kWavesPerGroup)));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  launch_encode_region(p.type, p.dims, hi_planes<double>(p) && p.type == 4, c->stream, grid, lds, d_src, p.g, p.cp, rg,
                       a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  if (!dev_stream && !copy_to_host_exact(words + Wf, c->words.p, nspan * 8, c->stream, c))
    return 0;
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  record_timing(c);
  return 1;
}
