// Region decode: any element-granular sub-box [lo, hi) of a coded box, decoding
// only the blocks that intersect it and writing only the region's elements.
//
//  decode3_region     one region block per lane, in raster order over the
//                     region's block grid (x fastest).  The lane maps its
//                     region block to the block's number in the stream, takes
//                     its own 64-bit stream position (fixed rate: analytic;
//                     variable rate: the per-block start table), the wave
//                     stages its blocks into LDS slots cooperatively, each
//                     lane decodes with decode_block3 / decode_block_n and
//                     stores the part of its block that lies in the region.
//                     The body is region_wave, which decode3_boxes
//                     (kernels_boxes.h) runs per region of a batch.
//  build_start_table  the start bit of every block from the block index's
//                     per-block lengths and per-wave bases.
//
// The first part of this header (mapping, clipped scatter, start-table
// arithmetic) needs block3.h only and compiles on the host behind the stub
// runtime of tests/emu (ZFP_REGION_MAPPING_ONLY).
#pragma once

#include "block3.h"

namespace zfp_amd {

// A region of the coded box of a Geometry.  Coordinates are relative to the
// box's origin f: block i of an axis covers [4 i, 4 i + 4).
struct RegionGeom {
  uint64_t lo[3];     // low corner
  uint64_t hi[3];     // exclusive high corner
  uint32_t rb0[3];    // first region block per axis in the box's block grid
  uint32_t rnb[3];    // region blocks per axis
  FastDiv rdv[2];     // division by rnb[0], rnb[1] (region block -> coordinates)
  int64_t ds[3];      // destination element strides; element x lands at x - lo
  uint64_t nrblocks;  // < 2^32 (checked by the host)
  uint32_t vec;       // 16-byte row stores for blocks inside the region (region_vec_ok)
};

struct RegionPos {
  uint64_t B;   // the block's number in the stream (raster order of the coded box)
  int64_t off;  // destination element offset of the block's origin (before the
                // destination's first element when the block starts below lo)
  int c0[3], c1[3];  // window of the block that is written, per axis
  bool full;         // the whole block
};

// lo, hi: absolute field coordinates, f <= lo < hi <= e per axis (the host
// checks); axes from `dims` on are one block thick
__host__ __device__ inline RegionGeom make_region_geom(const Geometry& g, int dims, const uint64_t* lo,
                                                       const uint64_t* hi, const int64_t* ds)
{
  RegionGeom r{};
  r.nrblocks = 1;
  for (int a = 0; a < 3; a++) {
    const bool in = a < dims;
    r.lo[a] = in ? lo[a] - g.f[a] : 0;
    r.hi[a] = in ? hi[a] - g.f[a] : 1;
    r.rb0[a] = (uint32_t)(r.lo[a] / 4);
    r.rnb[a] = (uint32_t)((r.hi[a] - 1) / 4 - r.lo[a] / 4 + 1);
    r.ds[a] = in ? ds[a] : 0;
    r.nrblocks *= r.rnb[a];
  }
  r.rdv[0] = make_fastdiv(r.rnb[0]);
  r.rdv[1] = make_fastdiv(r.rnb[1]);
  return r;
}

// 16-byte row stores: unit x stride, the other strides multiples of 4
// elements, a 16-byte aligned destination, and the region's low x a block
// boundary (every row of a block inside the region then starts 4 elements,
// 16 or 32 bytes, from an aligned address)
__host__ __device__ inline bool region_vec_ok(const RegionGeom& r, int dims, const void* dst)
{
  if (r.ds[0] != 1 || (r.lo[0] & 3) != 0 || (reinterpret_cast<uintptr_t>(dst) & 15) != 0)
    return false;
  for (int a = 1; a < dims && a < 3; a++)
    if (r.ds[a] % 4 != 0)
      return false;
  return true;
}

// Region block q (raster order over the region's block grid) -> its block in
// the coded box, the part of it inside the region and where that lands.  One
// division chain, as block_pos.  The window is cut by the region's low and
// high ends and by the field's edge (a partial block).
template <int D>
__device__ __forceinline__ RegionPos region_pos(const Geometry& g, const RegionGeom& rg, uint32_t q)
{
  RegionPos p;
  p.B = 0;
  p.off = 0;
  p.full = true;
  uint64_t mul = 1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    p.c0[a] = 0;
    p.c1[a] = 1;
    if (a < D) {
      uint32_t ri = q;
      if (a < D - 1) {
        const uint32_t t = fastdiv(q, rg.rdv[a]);
        ri = q - t * rg.rnb[a];
        q = t;
      }
      const uint32_t bi = rg.rb0[a] + ri;
      const uint64_t x0 = 4ull * bi;
      p.B += mul * bi;
      mul *= g.nb[a];
      const uint64_t edge = g.n[a] - g.f[a];
      const uint64_t left = (rg.hi[a] < edge ? rg.hi[a] : edge) - x0;
      p.c1[a] = left < 4 ? (int)left : 4;
      p.c0[a] = rg.lo[a] > x0 ? (int)(rg.lo[a] - x0) : 0;
      p.full = p.full && p.c0[a] == 0 && left >= 4;
      p.off += ((int64_t)x0 - (int64_t)rg.lo[a]) * rg.ds[a];
    }
  }
  return p;
}

// Store the window of a decoded 4^D block (x fastest).  Compile-time indices
// into v[] throughout, so that v[] stays in registers.
template <typename S, int D>
__device__ __forceinline__ void region_scatter(const S (&v)[64], S* __restrict__ dst, const RegionGeom& rg,
                                               const RegionPos& p)
{
  constexpr int N = 1 << (2 * D);
  S* o = dst + p.off;
  const int64_t sx = rg.ds[0], sy = D > 1 ? rg.ds[1] : 0, sz = D > 2 ? rg.ds[2] : 0;
  if (p.full && rg.vec) {
#pragma unroll
    for (int row = 0; row < N / 4; row++) {
      S* r = o + (row & 3) * sy + (row >> 2) * sz;
      if constexpr (sizeof(S) == 4) {
        Vec16<S, 4> q;
#pragma unroll
        for (int i = 0; i < 4; i++)
          q.v[i] = v[4 * row + i];
        store16<S, 4>(r, q);
      } else {
        Vec16<S, 2> q0, q1;
        q0.v[0] = v[4 * row + 0];
        q0.v[1] = v[4 * row + 1];
        q1.v[0] = v[4 * row + 2];
        q1.v[1] = v[4 * row + 3];
        store16<S, 2>(r, q0);
        store16<S, 2>(r + 2, q1);
      }
    }
  } else {
    const int x0 = p.c0[0], x1 = p.c1[0];
    const int y0 = D > 1 ? p.c0[1] : 0, y1 = D > 1 ? p.c1[1] : 1;
    const int z0 = D > 2 ? p.c0[2] : 0, z1 = D > 2 ? p.c1[2] : 1;
#pragma unroll
    for (int idx = 0; idx < N; idx++) {
      const int i = idx & 3, j = (idx >> 2) & 3, k = idx >> 4;
      if (i >= x0 && i < x1 && j >= y0 && j < y1 && k >= z0 && k < z1)
        o[i * sx + j * sy + k * sz] = v[idx];
    }
  }
}

// Start table: start[b] = bit of block b relative to the stream's first block,
// from the block index (per-block lengths, one base per index wave of
// `per_wave` blocks: 64 for 1D-3D, 16 for 4D).  One 64-lane wave per index
// wave: lane l < per_wave takes block w per_wave + l, and the entry is the
// wave's base plus the exclusive prefix sum of the lengths.
__host__ __device__ inline bool start_lane_block(uint64_t w, uint32_t per_wave, uint32_t lane, uint64_t nblocks,
                                                 uint64_t* b)
{
  *b = w * per_wave + lane;
  return lane < per_wave && *b < nblocks;
}

__host__ __device__ inline uint64_t start_entry(uint64_t wave_base, uint32_t incl, uint32_t len)
{
  return wave_base + (incl - len);
}

}  // namespace zfp_amd

#ifndef ZFP_REGION_MAPPING_ONLY

#include "blockn.h"
#include "kernels3.h"

namespace zfp_amd {

static __global__ __launch_bounds__(256) void build_start_table(const uint16_t* __restrict__ len,
                                                               const uint64_t* __restrict__ base, uint64_t nblocks,
                                                               uint64_t nwaves, uint32_t per_wave,
                                                               uint64_t* __restrict__ start)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (w >= nwaves)  // (wave-uniform: whole waves take part in the scan)
    return;
  uint64_t b;
  const bool act = start_lane_block(w, per_wave, lane, nblocks, &b);
  const uint32_t l = act ? len[b] : 0u;
  const uint32_t incl = wave_incl_scan(l);
  if (act)
    start[b] = start_entry(base[w], incl, l);
}

struct RegionArgs {
  const uint64_t* in;   // stream words
  uint64_t in_words;    // readable words from `in`
  // bit of the coded box's block 0 relative to bit 0 of in[0], modulo 2^64:
  // the words may begin after it (a host stream staged from the first needed
  // block on); the position of every block of the region is >= 0
  uint64_t bit0;
  uint32_t var;
  uint32_t maxbits;
  uint32_t W;       // words staged per block (block bound + 1)
  uint32_t swp;     // LDS slot stride (odd, >= W)
  uint32_t wmagic;  // ceil(2^32 / W)
  const uint16_t* idx_len;  // variable rate: per-block length (the index's)
  const uint64_t* start;    // variable rate: the start table
  uint32_t* idx_bad;        // as DecodeArgs::idx_bad
};

// One wave's share of a region: its 64 region blocks from `first` on (`live`:
// first < rg.nrblocks, wave-uniform), as lane `lane` of wave `wv` of the
// workgroup.  `sq` is the workgroup's squeeze table,
// `spos` its kWavesPerGroup * 64 positions, `lds` the staging slots.
//
// The staging is decode3's: thread t copies word j of block l for t = l W + j,
// funnel-shifted so the block starts at bit 0 of its slot.  A block's first
// word and shift come from the lane's own 64-bit position, kept in LDS: the
// blocks of a wave are x-runs of the region's rows, not one stream segment.
template <typename S, bool REV, bool HI, int D>
__device__ __forceinline__ void region_wave(S* __restrict__ dst, const Geometry& g, const CodecParams& cp,
                                            const RegionGeom& rg, const RegionArgs& a, uint64_t first, bool live,
                                            int lane, int wv, const uint32_t* sq, uint64_t* spos, uint64_t* lds)
{
  uint64_t* wslot = lds + (size_t)wv * 64 * a.swp;
  const uint64_t q = first + lane;
  const bool act = q < rg.nrblocks;
  uint64_t pos = 0;
  uint32_t len = 0;
  if (act) {
    const uint64_t B = region_pos<D>(g, rg, (uint32_t)q).B;
    if (a.var) {
      len = a.idx_len[B];
      pos = a.bit0 + a.start[B];
    } else {
      pos = a.bit0 + B * (uint64_t)a.maxbits;
    }
  }
  spos[threadIdx.x] = pos;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint64_t nb = live ? ((rg.nrblocks - first) < 64 ? (rg.nrblocks - first) : 64) : 0;
  const uint32_t pairs = (uint32_t)nb * a.W;
  auto slot_of = [&](uint32_t t) -> uint64_t* {
    const uint32_t l = __umulhi(t, a.wmagic);
    return wslot + (size_t)l * a.swp + (t - l * a.W);
  };
  __builtin_amdgcn_s_setprio(ZFP_DEC_STAGE_PRIO);
  if (!__any(act && (pos & 63) != 0)) {
    // every block of the wave starts on a word (wave-uniform): no funnel shift
    stage_batched(
        pairs,
        [&](uint32_t t) {
          const uint32_t l = __umulhi(t, a.wmagic);
          const uint64_t gw = (spos[wv * 64 + l] >> 6) + (t - l * a.W);
          return gw < a.in_words ? a.in[gw] : 0ull;
        },
        [&](uint32_t t, uint64_t v) { *slot_of(t) = v; });
  } else {
    stage_batched(
        pairs,
        [&](uint32_t t) {
          const uint32_t l = __umulhi(t, a.wmagic);
          const uint64_t sb = spos[wv * 64 + l];
          const uint64_t gw = (sb >> 6) + (t - l * a.W);
          const uint32_t sh = (uint32_t)sb & 63u;
          const uint64_t lo = gw < a.in_words ? a.in[gw] : 0ull;
          const uint64_t hi = gw + 1 < a.in_words ? a.in[gw + 1] : 0ull;
          return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        },
        [&](uint32_t t, uint64_t v) { *slot_of(t) = v; });
  }
  __builtin_amdgcn_s_setprio(0);
  // the staged slots and the table are this wave's own writes
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  if (!act)
    return;
  S v[64];
  uint32_t used;
  WordReader r;
  r.w = wslot + (size_t)lane * a.swp;
  r.pos = 0;
  if constexpr (D == 3 && !kIntField<S>)
    used = decode_block3<S, REV, HI>(r, sq, v, cp);
  else
    used = decode_block_n<S, D, REV>(r, sq, v, cp);
  // (the block's window is computed after the decode, not held across it)
  region_scatter<S, D>(v, dst, rg, region_pos<D>(g, rg, (uint32_t)q));
  if (a.idx_bad && used != len)
    atomicOr(a.idx_bad, 1u);
}

template <typename S, bool REV, bool HI = false, int D = 3>
__global__ __launch_bounds__(256, 1) void decode3_region(S* __restrict__ dst, Geometry g, CodecParams cp,
                                                        RegionGeom rg, RegionArgs a)
{
  __shared__ uint32_t sq[256];
  __shared__ uint64_t spos[kWavesPerGroup * 64];
  extern __shared__ uint64_t lds[];
  const int lane = threadIdx.x & 63;
  // every wave writes the whole (identical) table: no workgroup barrier below
#pragma unroll
  for (int k = 0; k < 4; k++)
    sq[lane + 64 * k] = squeeze_entry(lane + 64 * k);
  const int wv = threadIdx.x >> 6;
  const uint64_t first = ((uint64_t)blockIdx.x * kWavesPerGroup + wv) * 64;
  region_wave<S, REV, HI, D>(dst, g, cp, rg, a, first, first < rg.nrblocks, lane, wv, sq, spos, lds);
}

// Launchers (zfp_region.hip holds every instantiation).  type: zfp_type (1
// int32, 2 int64, 3 float, 4 double); dims 1..3; hi: the f64 3D decoder of
// planes 32..63 (maxprec <= 32).
void launch_decode_region(int type, int dims, bool rev, bool hi, hipStream_t stream, dim3 grid, size_t lds, void* dst,
                          const Geometry& g, const CodecParams& cp, const RegionGeom& rg, const RegionArgs& a);
void launch_start_table(hipStream_t stream, const uint16_t* len, const uint64_t* base, uint64_t nblocks,
                        uint64_t nwaves, uint32_t per_wave, uint64_t* start);

}  // namespace zfp_amd

#endif  // ZFP_REGION_MAPPING_ONLY
