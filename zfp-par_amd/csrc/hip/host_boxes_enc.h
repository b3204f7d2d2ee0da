// Host shim: batched region encode (zfp_hip_compress_regions) -- validation of
// every entry and of the batch (no block in two entries: host_disjoint.h), and
// region_enc_once's sequence for a batch: one staged span of a host stream,
// the sources' dense images, the table of region records and wave_first, one
// launch, the span copied back.
#pragma once

#include "host_boxes.h"
#include "host_disjoint.h"
#include "host_region_enc.h"
#include "kernels_boxes_enc.h"

// Everything that is checked before any GPU call.  One bad entry fails the call.
// bp.rec[i].dst holds entry i's source.
static int plan_regions_enc(const zfp_hip_job* job, const zfp_hip_src_region* regions, uint64_t nregions,
                            const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset, Plan& p,
                            BoxesPlan& bp)
{
  const char* who = "zfp_hip_compress_regions";
  if (!job || !regions || !words)
    return fail("%s: null job, regions or stream pointer", who);
  zfp_hip_job j;
  if (!plan_coded_box(who, "encode", job, p, j))
    return 0;
  if (!p.fixed)
    return fail("%s: a region can be rewritten in a fixed-rate stream only (minbits == maxbits, not reversible): "
                "in a variable-rate stream a block of another length moves every later block", who);
  if (nregions > kMaxRegions)
    return fail("%s: %llu regions in one call (at most %llu)", who, (unsigned long long)nregions,
                (unsigned long long)kMaxRegions);
  bp.rec.resize(nregions);
  bp.wave_first.resize(nregions + 1);
  std::vector<BlockBox> box(nregions);
  uint64_t waves = 0, top = 0, top_entry = 0;  // the highest needed block and the entry that needs it
  for (uint64_t i = 0; i < nregions; i++) {
    const zfp_hip_src_region& r = regions[i];
    char entry[96];  // a failing entry's name: written when one fails
    auto named = [&](const char* colon) {
      snprintf(entry, sizeof entry, "regions[%llu] (entry %llu of %llu)%s", (unsigned long long)i,
               (unsigned long long)(i + 1), (unsigned long long)nregions, colon);
      return entry;
    };
    if (!r.src)
      return fail("%s: %s has a null source", who, named(""));
    if (!check_region_box(who, "", j, p.dims, r.lo, r.hi))  // (failed: once more, for the message with the entry)
      return check_region_box(who, named(": "), j, p.dims, r.lo, r.hi);
    RegionGeom& rg = bp.rec[i].rg;
    rg = make_region_geom(p.g, p.dims, r.lo, r.hi, r.src_stride);
    bp.rec[i].dst = const_cast<void*>(r.src);
    bp.wave_first[i] = (uint32_t)waves;
    waves += box_waves(rg.nrblocks);  // (a region has at most the box's blocks, fewer than 2^32)
    bp.blocks += rg.nrblocks;
    if (waves * 64 > 0xffffffffull)
      return fail("%s: the regions take %llu lanes or more, padded to whole waves (at most 2^32 - 1)", who,
                  (unsigned long long)(waves * 64));
    for (int a = 0; a < 3; a++) {
      box[i].b0[a] = rg.rb0[a];
      box[i].nb[a] = rg.rnb[a];
    }
    uint64_t Blo, Bhi;
    region_block_span(p, rg, &Blo, &Bhi);
    if (Bhi >= top) {
      top = Bhi;
      top_entry = i;
    }
  }
  bp.wave_first[nregions] = (uint32_t)waves;
  if (nregions) {
    // (top + 1) maxbits < 2^32 * 2^32; the sum is checked for wrap-around
    const uint64_t end = bit_offset + (top + 1) * (uint64_t)p.cp.maxbits;
    if (end < bit_offset || capacity_words > (~0ull >> 6) || end > capacity_words * 64)
      return fail("%s: the stream's %llu words end before bit %llu, the end of the last block of regions[%llu]", who,
                  (unsigned long long)capacity_words, (unsigned long long)end, (unsigned long long)top_entry);
  }
  size_t ia, ib;
  if (first_shared_block(box.data(), (size_t)nregions, p.dims - 1, &ia, &ib))
    return fail("%s: regions[%llu] and regions[%llu] both intersect block (%llu, %llu, %llu) of the coded box: the "
                "block sets of a batch must be pairwise disjoint (merge the entries or make two calls)", who,
                (unsigned long long)ia, (unsigned long long)ib,
                (unsigned long long)std::max(box[ia].b0[0], box[ib].b0[0]),
                (unsigned long long)std::max(box[ia].b0[1], box[ib].b0[1]),
                (unsigned long long)std::max(box[ia].b0[2], box[ib].b0[2]));
  return 1;
}

// One batched encode; `bp.rec` holds the caller's sources and strides and is
// left as it is, `rec` is the table as the kernel reads it, `tmp` the packed
// rows of host sources that are not dense (both live until the caller's lease
// has ended, so past the synchronize).
static int regions_enc_once(Ctx* c, const Plan& p, const BoxesPlan& bp, std::vector<BoxRecord>& rec,
                            std::vector<std::vector<char>>& tmp, const zfp_hip_src_region* regions, uint64_t* words,
                            uint64_t capacity_words, uint64_t bit_offset)
{
  const size_t n = bp.rec.size();
  bool dev_src = false;
  for (size_t i = 0; i < n; i++) {
    const bool d = is_device_ptr(bp.rec[i].dst);
    if (i && d != dev_src)
      return fail("zfp_hip_compress_regions: regions[%llu] has its source in %s memory, the entries before it in %s "
                  "memory (one call takes one kind)",
                  (unsigned long long)i, d ? "device" : "host", dev_src ? "device" : "host");
    dev_src = d;
  }
  const bool dev_stream = is_device_ptr(words);
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
    // one span of the stream for all regions
    uint64_t Blo = ~0ull, Bhi = 0;
    for (size_t i = 0; i < n; i++) {
      uint64_t lo, hi;
      region_block_span(p, bp.rec[i].rg, &lo, &hi);
      Blo = std::min(Blo, lo);
      Bhi = std::max(Bhi, hi);
    }
    if (!stage_fixed_span(c, p, Blo, Bhi, words, capacity_words, bit_offset, false, &Wf, &nspan, &a.bit0))
      return 0;
    a.out = (uint64_t*)c->words.p;
    a.out_words = nspan;
  }
  // sources: the caller's device arrays, or dense images of the regions back
  // to back in the field scratch, each from a 16-byte boundary on
  rec = bp.rec;
  if (!dev_src) {
    std::vector<size_t> img(n);
    size_t bytes = 0;
    for (size_t i = 0; i < n; i++) {
      img[i] = bytes;
      bytes += (dense_image(rec[i].rg, p.dims, p.es) + 15) & ~(size_t)15;
    }
    if (!ensure(c->field, bytes))
      return 0;
    tmp.resize(n);
    for (size_t i = 0; i < n; i++) {
      rec[i].dst = (char*)c->field.p + img[i];
      if (!region_from_host(c, p, rec[i].rg, regions[i].src_stride, regions[i].src, rec[i].dst, tmp[i]))
        return 0;
    }
  }
  for (size_t i = 0; i < n; i++)
    rec[i].rg.vec = region_vec_ok(rec[i].rg, p.dims, rec[i].dst) ? 1u : 0u;
  // the table: the records, then wave_first
  const size_t rec_bytes = n * sizeof(BoxRecord), wf_bytes = (n + 1) * sizeof(uint32_t);
  if (!ensure(c->boxes, rec_bytes + wf_bytes) || !h2d(c, c->boxes.p, rec.data(), rec_bytes, c->stream) ||
      !h2d(c, (char*)c->boxes.p + rec_bytes, bp.wave_first.data(), wf_bytes, c->stream))
    return 0;
  BoxesArgs b;
  b.rec = (const BoxRecord*)c->boxes.p;
  b.wave_first = (const uint32_t*)((const char*)c->boxes.p + rec_bytes);
  b.n = (uint32_t)n;
  const uint64_t waves = bp.wave_first[n];
  const dim3 grid((unsigned)((waves + kWavesPerGroup - 1) / kWavesPerGroup));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  launch_encode_boxes(p.type, p.dims, hi_planes<double>(p) && p.type == 4, c->stream, grid, s.lds, b, p.g, p.cp, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  if (!dev_stream && !copy_to_host_exact(words + Wf, c->words.p, nspan * 8, c->stream, c))
    return 0;
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  record_timing(c);
  return 1;
}
