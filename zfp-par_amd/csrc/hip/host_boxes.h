// Host shim: batched region decode (zfp_hip_decompress_regions) -- validation
// of every entry, and region_decode_once with the batch's destinations (the
// table of region records and wave_first), its one launch and its copy-outs.
#pragma once

#include "host_region.h"
#include "kernels_boxes.h"

constexpr uint64_t kMaxRegions = 65536;  // (a record is 144 bytes: a table of at most 9.3 MB)

// What a batch is once it has passed validation.
struct BoxesPlan {
  std::vector<BoxRecord> rec;  // rg from the entry's lo, hi and strides; dst the entry's
  std::vector<uint32_t> wave_first;     // nregions + 1
  uint64_t blocks = 0;                  // sum of the regions' blocks
};

// Everything that is checked before any GPU call.  One bad entry fails the call.
static int plan_regions(const zfp_hip_job* job, const zfp_hip_region* regions, uint64_t nregions,
                        const uint64_t* words, Plan& p, BoxesPlan& bp)
{
  const char* who = "zfp_hip_decompress_regions";
  if (!job || !regions || !words)
    return fail("%s: null job, regions or stream pointer", who);
  zfp_hip_job j;
  if (!plan_coded_box(who, "decode", job, p, j))
    return 0;
  if (nregions > kMaxRegions)
    return fail("%s: %llu regions in one call (at most %llu)", who, (unsigned long long)nregions,
                (unsigned long long)kMaxRegions);
  bp.rec.resize(nregions);
  bp.wave_first.resize(nregions + 1);
  uint64_t waves = 0;
  for (uint64_t i = 0; i < nregions; i++) {
    const zfp_hip_region& r = regions[i];
    char entry[96];  // a failing entry's name: written when one fails
    auto named = [&](const char* colon) {
      snprintf(entry, sizeof entry, "regions[%llu] (entry %llu of %llu)%s", (unsigned long long)i,
               (unsigned long long)(i + 1), (unsigned long long)nregions, colon);
      return entry;
    };
    if (!r.dst)
      return fail("%s: %s has a null destination", who, named(""));
    if (!check_region_box(who, "", j, p.dims, r.lo, r.hi))  // (failed: once more, for the message with the entry)
      return check_region_box(who, named(": "), j, p.dims, r.lo, r.hi);
    RegionGeom& rg = bp.rec[i].rg;
    rg = make_region_geom(p.g, p.dims, r.lo, r.hi, r.dst_stride);
    bp.rec[i].dst = r.dst;
    bp.wave_first[i] = (uint32_t)waves;
    waves += box_waves(rg.nrblocks);  // (a region has at most the box's blocks, fewer than 2^32)
    bp.blocks += rg.nrblocks;
    if (waves * 64 > 0xffffffffull)
      return fail("%s: the regions take %llu lanes or more, padded to whole waves (at most 2^32 - 1)", who,
                  (unsigned long long)(waves * 64));
  }
  bp.wave_first[nregions] = (uint32_t)waves;
  return 1;
}

// One batched decode; `bp.rec` holds the caller's destinations and strides
// and is left as it is, `rec` is the table as the kernel reads it.
static int regions_once(Ctx* c, const Plan& p, const BoxesPlan& bp, std::vector<BoxRecord>& rec,
                        const zfp_hip_region* regions, const DecodeTry& t)
{
  const size_t n = bp.rec.size();
  bool dev_dst = false;
  for (size_t i = 0; i < n; i++) {
    const bool d = is_device_ptr(bp.rec[i].dst);
    if (i && d != dev_dst)
      return fail("zfp_hip_decompress_regions: regions[%llu] has its destination in %s memory, the entries before "
                  "it in %s memory (one call takes one kind)",
                  (unsigned long long)i, d ? "device" : "host", dev_dst ? "device" : "host");
    dev_dst = d;
  }
  // one span of the stream for all regions
  uint64_t Blo = ~0ull, Bhi = 0;
  for (size_t i = 0; i < n; i++) {
    uint64_t lo, hi;
    region_block_span(p, bp.rec[i].rg, &lo, &hi);
    Blo = std::min(Blo, lo);
    Bhi = std::max(Bhi, hi);
  }
  const size_t rec_bytes = n * sizeof(BoxRecord), wf_bytes = (n + 1) * sizeof(uint32_t);
  return region_decode_once(
      c, p, t, Blo, Bhi,
      [&] {
        // destinations: the caller's device arrays, or dense images of the regions
        // back to back in the field scratch, each from a 16-byte boundary on
        rec = bp.rec;
        if (!dev_dst) {
          std::vector<size_t> img(n);
          size_t bytes = 0;
          for (size_t i = 0; i < n; i++) {
            img[i] = bytes;
            bytes += (dense_image(rec[i].rg, p.dims, p.es) + 15) & ~(size_t)15;
          }
          if (!ensure(c->field, bytes))
            return 0;
          for (size_t i = 0; i < n; i++)
            rec[i].dst = (char*)c->field.p + img[i];
        }
        for (size_t i = 0; i < n; i++)
          rec[i].rg.vec = region_vec_ok(rec[i].rg, p.dims, rec[i].dst) ? 1u : 0u;
        // the table: the records, then wave_first
        if (!ensure(c->boxes, rec_bytes + wf_bytes) || !h2d(c, c->boxes.p, rec.data(), rec_bytes, c->stream) ||
            !h2d(c, (char*)c->boxes.p + rec_bytes, bp.wave_first.data(), wf_bytes, c->stream))
          return 0;
        return 1;
      },
      [&](const RegionArgs& a, size_t lds) {
        BoxesArgs b;
        b.rec = (const BoxRecord*)c->boxes.p;
        b.wave_first = (const uint32_t*)((const char*)c->boxes.p + rec_bytes);
        b.n = (uint32_t)n;
        const uint64_t waves = bp.wave_first[n];
        const dim3 grid((unsigned)((waves + kWavesPerGroup - 1) / kWavesPerGroup));
        launch_decode_boxes(p.type, p.dims, p.cp.minexp < kMinExp, hi_planes<double>(p) && p.type == 4, c->stream, grid,
                            lds, b, p.g, p.cp, a);
      },
      [&] {
        if (!dev_dst)
          for (size_t i = 0; i < n; i++)
            if (!region_to_host(c, p, rec[i].rg, regions[i].dst_stride, regions[i].dst, rec[i].dst))
              return 0;
        return 1;
      });
}
