// Batched region decode: any number of sub-boxes ("regions") of one coded box,
// each into its own destination, in one launch.
//
//  decode3_boxes   the waves of the launch are dealt out to the regions in
//                  order: region r with nrblocks[r] blocks owns
//                  ceil(nrblocks[r] / 64) consecutive waves, one region block
//                  per lane as in decode3_region.  A wave never spans two
//                  regions; the lanes past a region's last block are inactive.
//                  A wave finds its region from its global number W in
//                  wave_first[0..n] (the exclusive prefix of the waves per
//                  region; wave_first[n] is the total) by bisection, reads the
//                  region's record -- its RegionGeom and its destination --
//                  and runs region_wave (kernels_region.h) on it.  W is
//                  wave-uniform (readfirstlane), so the bisection and the
//                  record are scalar loads and the geometry sits in SGPRs, as
//                  decode3_region's by-value argument does.
//
// The first part of this header (the wave -> region mapping) compiles on the
// host behind the stub runtime of tests/emu (ZFP_REGION_MAPPING_ONLY).
#pragma once

#include "kernels_region.h"

namespace zfp_amd {

// One region of a batch, in device memory.
struct BoxRecord {
  RegionGeom rg;
  void* dst;  // element lo of the region lands here
};
static_assert(sizeof(BoxRecord) % 8 == 0, "records are read as dwords from an array");

// waves a region of `nrblocks` blocks owns
__host__ __device__ inline uint64_t box_waves(uint64_t nrblocks) { return (nrblocks + 63) / 64; }

struct BoxWave {
  uint32_t r;      // the wave's region; n: the wave lies past the last region
  uint64_t first;  // the wave's first region block (lane l takes first + l)
};

// Wave W of the batch.  wave_first[0] = 0 < wave_first[1] < ... <
// wave_first[n] (every region has a block): the region is the last r with
// wave_first[r] <= W, found with at most ceil(log2(n + 1)) loads.
__host__ __device__ inline BoxWave box_wave(const uint32_t* wave_first, uint32_t n, uint32_t W)
{
  uint32_t lo = 0, hi = n;  // the region lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (wave_first[mid] <= W)
      lo = mid;
    else
      hi = mid - 1;
  }
  BoxWave w;
  w.r = lo;
  w.first = 0;
  if (lo < n)
    w.first = (uint64_t)(W - wave_first[lo]) * 64;
  return w;
}

}  // namespace zfp_amd

#ifndef ZFP_REGION_MAPPING_ONLY

namespace zfp_amd {

struct BoxesArgs {
  const BoxRecord* rec;        // n records
  const uint32_t* wave_first;  // n + 1 entries
  uint32_t n;
};

template <typename S, bool REV, bool HI = false, int D = 3>
__global__ __launch_bounds__(256, 1) void decode3_boxes(BoxesArgs b, Geometry g, CodecParams cp, RegionArgs a)
{
  __shared__ uint32_t sq[256];
  __shared__ uint64_t spos[kWavesPerGroup * 64];
  extern __shared__ uint64_t lds[];
  // (threadIdx.x >> 6 is uniform in a wave, which the compiler cannot see)
  const uint32_t W =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6)));
  const BoxWave w = box_wave(b.wave_first, b.n, W);
  if (w.r >= b.n)  // (wave-uniform; the waves of a workgroup meet at no barrier)
    return;
  const int lane = threadIdx.x & 63;
  // every wave writes the whole (identical) table: no workgroup barrier below
#pragma unroll
  for (int k = 0; k < 4; k++)
    sq[lane + 64 * k] = squeeze_entry(lane + 64 * k);
  const RegionGeom rg = b.rec[w.r].rg;
  region_wave<S, REV, HI, D>((S*)b.rec[w.r].dst, g, cp, rg, a, w.first, true, lane, threadIdx.x >> 6, sq, spos, lds);
}

// Launcher (zfp_boxes.hip holds every instantiation: those of zfp_region.hip).
void launch_decode_boxes(int type, int dims, bool rev, bool hi, hipStream_t stream, dim3 grid, size_t lds,
                         const BoxesArgs& b, const Geometry& g, const CodecParams& cp, const RegionArgs& a);

}  // namespace zfp_amd

#endif  // ZFP_REGION_MAPPING_ONLY
