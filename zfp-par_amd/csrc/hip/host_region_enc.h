// Host shim: region encode (zfp_hip_compress_region) -- what it checks beyond
// plan_region, the dense device image of a host source, and the call: the
// needed words of a host stream staged, the launch, the same words copied back.
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
  if (!plan_region(job, lo, hi, src, src_stride, words, p, rg, who, "encode", "source"))
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
  uint64_t ext[3];
  const size_t bytes = region_extents(rg, p.dims, p.es, ext);
  if (region_is_dense(ext, p.dims, hs))
    return h2d(c, d_img, h_src, bytes, c->stream);
  tmp.resize(bytes);
  region_rows(ext, p.dims, p.es, hs, const_cast<void*>(h_src), tmp.data(), false);
  return h2d(c, d_img, tmp.data(), bytes, c->stream);
}

static int region_enc_once(Ctx* c, const Plan& p, RegionGeom rg, const void* src, const int64_t* src_stride,
                           uint64_t* words, uint64_t capacity_words, uint64_t bit_offset)
{
  const bool dev_src = is_device_ptr(src);
  const bool dev_stream = is_device_ptr(words);
  std::vector<char> tmp;
  // one LDS slot per lane for the decoder (its look-ahead word included) and
  // the coder; checked before anything is queued
  RegionSlots s;
  if (!region_slots(p.cp.maxbits, slot_words_for(p.bound_bits), 2 * kLutBytes, s))
    return 0;
  RegionEncArgs a{};
  a.maxbits = p.cp.maxbits;
  a.W = s.W;
  a.swp = s.swp;
  a.wmagic = s.wmagic;
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  a.out = words;
  a.out_words = capacity_words;
  a.bit0 = bit_offset;
  uint64_t Wf = 0, nspan = 0;  // a host stream's span: staged, merged on the device, copied back
  if (!dev_stream) {
    uint64_t Blo, Bhi;
    region_block_span(p, rg, &Blo, &Bhi);
    if (!stage_fixed_span(c, p, Blo, Bhi, words, capacity_words, bit_offset, false, &Wf, &nspan, &a.bit0))
      return 0;
    a.out = (uint64_t*)c->words.p;
    a.out_words = nspan;
  }
  // source: the caller's device array, or a dense image of the region
  const void* d_src = src;
  if (!dev_src) {
    if (!ensure(c->field, dense_image(rg, p.dims, p.es)))
      return 0;
    if (!region_from_host(c, p, rg, src_stride, src, c->field.p, tmp))
      return 0;
    d_src = c->field.p;
  }
  rg.vec = region_vec_ok(rg, p.dims, d_src) ? 1u : 0u;
  const dim3 grid((unsigned)((rg.nrblocks + 64 * kWavesPerGroup - 1) / (64 * kWavesPerGroup)));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  launch_encode_region(p.type, p.dims, hi_planes<double>(p) && p.type == 4, c->stream, grid, s.lds, d_src, p.g, p.cp,
                       rg, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  if (!dev_stream && !copy_to_host_exact(words + Wf, c->words.p, nspan * 8, c->stream, c))
    return 0;
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  record_timing(c);
  return 1;
}
