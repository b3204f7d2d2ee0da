// Batched region encode: any number of sub-boxes ("regions") of one fixed-rate
// coded box, each from its own source, rewritten in place in one launch.
//
//  encode3_boxes   decode3_boxes' dealing (kernels_boxes.h): region r with
//                  nrblocks[r] blocks owns ceil(nrblocks[r] / 64) consecutive
//                  waves, a wave finds its region from its global number in
//                  wave_first by scalar bisection, reads the region's record --
//                  its RegionGeom and its source (BoxRecord::dst) -- and runs
//                  region_enc_wave (kernels_region_enc.h) on it.  A wave never
//                  spans two regions; its lanes past the region's last block
//                  code that block again and take no part in the copy-out, as
//                  in encode3_region.
//
// The block sets of the regions must be pairwise disjoint (the host refuses
// anything else, host_disjoint.h).  The merge's invariant -- no block's bits
// are read by any wave but its own, before that wave's writes -- then holds
// across regions as it does across the waves of one region: a block that
// belonged to two regions would be staged by one wave while another merges it,
// and the result would depend on their order.  Blocks of different regions
// that share a stream word (rate 3.25, a 96-bit header) are fine: their masks
// are disjoint and the and/or pairs commute.
#pragma once

#include "kernels_boxes.h"
#include "kernels_region_enc.h"

#ifndef ZFP_REGION_MAPPING_ONLY

namespace zfp_amd {

template <typename S, bool HI = false, int D = 3>
__global__ __launch_bounds__(256, 1) void encode3_boxes(BoxesArgs b, Geometry g, CodecParams cp, RegionEncArgs a)
{
  __shared__ uint32_t lut[256];
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
  const int wv = threadIdx.x >> 6;
  uint64_t* wslot = lds + (size_t)wv * 64 * a.swp;
  // every wave writes both (identical) tables and zeroes its own slots
#pragma unroll
  for (int k = 0; k < 4; k++) {
    sq[lane + 64 * k] = squeeze_entry(lane + 64 * k);
    lut[lane + 64 * k] = kCoderTables.dbl[lane + 64 * k];
  }
  for (uint32_t i = lane; i < 64 * a.swp; i += 64)
    wslot[i] = 0;
  const RegionGeom rg = b.rec[w.r].rg;
  region_enc_wave<S, HI, D>((const S*)b.rec[w.r].dst, g, cp, rg, a, w.first, lane, wv, lut, sq, spos, lds);
}

// Launcher (zfp_boxes_enc.hip holds every instantiation: those of
// zfp_region_enc.hip).
void launch_encode_boxes(int type, int dims, bool hi, hipStream_t stream, dim3 grid, size_t lds, const BoxesArgs& b,
                         const Geometry& g, const CodecParams& cp, const RegionEncArgs& a);

}  // namespace zfp_amd

#endif  // ZFP_REGION_MAPPING_ONLY
