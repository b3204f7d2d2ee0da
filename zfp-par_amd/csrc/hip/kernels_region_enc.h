// Region encode: rewrite any element-granular sub-box [lo, hi) of a fixed-rate
// stream in place, coding only the blocks that intersect it and leaving every
// other bit of the stream as it was.
//
//  encode3_region   one region block per lane, in raster order over the
//                   region's block grid (x fastest), as decode3_region.  Fixed
//                   rate only: block B sits at bit0 + B maxbits, so it can be
//                   replaced without moving any other.
//
//   covered block   every element of the block that lies inside the field is
//                   inside the region: coded from the source alone (the
//                   reference's pad rule at the field's edge), its old bits are
//                   never read.
//   partly covered  the region cuts through the block, or the block lies at a
//                   chunk end that is neither a multiple of 4 from the chunk's
//                   origin nor the field's edge: the old block is decoded, the
//                   region's elements are overlaid and the block is coded again
//                   (read-modify-write, what the reference's compressed arrays
//                   do when one element of a cached block is written).  The
//                   elements kept this way go through one more lossy round.
//
// Copy-out is a merge, not a store: a stream word that lies wholly inside one
// block's bit range gets a plain store, every other word an atomic and (clear
// the block's bits) followed by an atomic or (set them) from the same thread.
// Masks of different blocks are disjoint, so the pairs of different threads,
// waves and workgroups commute; no word is written by both a plain store and
// an atomic; no block's bits are read by any lane but its own wave's, before
// that wave's writes.
//
// The first part of this header (the covered rule, the overlay, the merge's
// word and mask arithmetic) needs kernels_region.h's mapping only and compiles
// on the host behind the stub runtime of tests/emu (ZFP_REGION_MAPPING_ONLY).
#pragma once

#include "kernels_region.h"

namespace zfp_amd {

// region_pos and what the encoder adds to it
struct RegionEncPos {
  RegionPos p;
  int fc[3];     // elements of the block inside the field, per axis (1..4)
  bool covered;  // every element inside the field is inside the region
  bool infield;  // the whole block lies inside the field (no padding)
};

// Per axis the block is covered when its window starts at 0 and ends where the
// field does (or at 4): c0 == 0 && c1 == min(4, n - f - 4 bi).
template <int D>
__device__ __forceinline__ RegionEncPos region_enc_pos(const Geometry& g, const RegionGeom& rg, uint32_t q)
{
  RegionEncPos e;
  e.p = region_pos<D>(g, rg, q);
  e.covered = true;
  e.infield = true;
  uint32_t t = q;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    e.fc[a] = 1;
    if (a < D) {
      uint32_t ri = t;
      if (a < D - 1) {
        const uint32_t u = fastdiv(t, rg.rdv[a]);
        ri = t - u * rg.rnb[a];
        t = u;
      }
      const uint64_t left = (g.n[a] - g.f[a]) - 4ull * (rg.rb0[a] + ri);
      e.fc[a] = left < 4 ? (int)left : 4;
      e.infield = e.infield && left >= 4;
      e.covered = e.covered && e.p.c0[a] == 0 && e.p.c1[a] == e.fc[a];
    }
  }
  return e;
}

// Overlay: the region's elements of a partly covered block, from the source
// (element x of the region at (x - lo) . ds), over the decoded block.  The
// mirror of region_scatter's scalar branch: compile-time indices into v[].
template <typename S, int D>
__device__ __forceinline__ void region_overlay(S (&v)[64], const S* __restrict__ src, const RegionGeom& rg,
                                               const RegionPos& p)
{
  constexpr int N = 1 << (2 * D);
  const S* o = src + p.off;
  const int64_t sx = rg.ds[0], sy = D > 1 ? rg.ds[1] : 0, sz = D > 2 ? rg.ds[2] : 0;
  const int x0 = p.c0[0], x1 = p.c1[0];
  const int y0 = D > 1 ? p.c0[1] : 0, y1 = D > 1 ? p.c1[1] : 1;
  const int z0 = D > 2 ? p.c0[2] : 0, z1 = D > 2 ? p.c1[2] : 1;
#pragma unroll
  for (int idx = 0; idx < N; idx++) {
    const int i = idx & 3, j = (idx >> 2) & 3, k = idx >> 4;
    if (i >= x0 && i < x1 && j >= y0 && j < y1 && k >= z0 && k < z1)
      v[idx] = o[i * sx + j * sy + k * sz];
  }
}

// The merge.  A block of `maxbits` bits whose first bit is bit `sh` of its
// first stream word: the part of the block that stream word j (counted from
// that first word) holds.  Bits [x0, x0 + cnt) of the block land at bit `shl`
// of the word; `mask` selects them.  cnt == 64 (mask all ones): the word lies
// wholly inside the block and takes a plain store; any other word is shared
// with a neighbouring block or with what lies outside the stream's blocks and
// takes and(~mask), or(bits << shl).  Returns false for a word that holds
// nothing of the block.
struct MergeWord {
  uint32_t x0, cnt, shl;
  uint64_t mask;
  __host__ __device__ bool plain() const { return cnt == 64; }
};

__host__ __device__ inline bool merge_word(uint32_t maxbits, uint32_t sh, uint32_t j, MergeWord* m)
{
  const int64_t lo = (int64_t)64 * j - sh, hi = lo + 64;
  const int64_t a = lo > 0 ? lo : 0, b = hi < (int64_t)maxbits ? hi : (int64_t)maxbits;
  if (b <= a)
    return false;
  m->x0 = (uint32_t)a;
  m->cnt = (uint32_t)(b - a);
  m->shl = (uint32_t)(a - lo);
  m->mask = (m->cnt >= 64 ? ~0ull : ((1ull << m->cnt) - 1)) << m->shl;
  return true;
}

// stream words a block can touch: ceil((63 + maxbits) / 64)
__host__ __device__ inline uint32_t merge_words(uint32_t maxbits) { return (maxbits + 126u) / 64u; }

}  // namespace zfp_amd

#ifndef ZFP_REGION_MAPPING_ONLY

namespace zfp_amd {

struct RegionEncArgs {
  uint64_t* out;       // stream words (read for partly covered blocks, merged into)
  uint64_t out_words;  // readable words from `out`; every word written lies below it (host check)
  uint64_t bit0;       // as RegionArgs::bit0
  uint32_t maxbits;
  uint32_t W;       // words staged per block (block bound + 1) >= merge_words(maxbits)
  uint32_t swp;     // LDS slot stride (odd, >= W and >= the coder's slot)
  uint32_t wmagic;  // ceil(2^32 / W)
};

// One wave's share of a region: its 64 region blocks from `first` on
// (first < rg.nrblocks, wave-uniform), as lane `lane` of wave `wv` of the
// workgroup.  `lut` and `sq` are the workgroup's coder and squeeze tables,
// `spos` its kWavesPerGroup * 64 positions, `lds` the slots; the wave's own
// slots are zero on entry.  The body of encode3_region, which encode3_boxes
// (kernels_boxes_enc.h) runs per region of a batch.
// Lanes past the region's last block code that last block again (so that every
// wave is whole where the coder's wave-uniform branches stage cooperatively)
// and take no part in the copy-out.
// (The structs come by value: by reference the same body took 4 to 7 VGPRs
// more, and three instantiations of encode3_region lost a wave per SIMD.)
template <typename S, bool HI, int D>
__device__ __forceinline__ void region_enc_wave(const S* __restrict__ src, const Geometry g, const CodecParams cp,
                                                const RegionGeom rg, const RegionEncArgs a, const uint64_t first,
                                                const int lane, const int wv, const uint32_t* lut, const uint32_t* sq,
                                                uint64_t* spos, uint64_t* lds)
{
  uint64_t* wslot = lds + (size_t)wv * 64 * a.swp;
  const uint64_t nb = (rg.nrblocks - first) < 64 ? (rg.nrblocks - first) : 64;
  const bool act = (uint64_t)lane < nb;
  const uint32_t q = (uint32_t)(act ? first + lane : rg.nrblocks - 1);

  bool need;  // the lane's block is read, overlaid and coded again
  {
    const RegionEncPos e = region_enc_pos<D>(g, rg, q);
    need = !e.covered;
    spos[threadIdx.x] = a.bit0 + e.p.B * (uint64_t)a.maxbits;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const bool rmw = __any(need);  // (wave-uniform: interior waves of a large region never stage)
  const uint32_t pairs = (uint32_t)nb * a.W;
  auto slot_of = [&](uint32_t t) -> uint64_t* {
    const uint32_t l = __umulhi(t, a.wmagic);
    return wslot + (size_t)l * a.swp + (t - l * a.W);
  };
  uint64_t* myslot = wslot + (size_t)lane * a.swp;

  // the block to code: the source's elements, over the old block's where the
  // region does not cover it
  auto image = [&](S (&v)[64]) __attribute__((always_inline)) {
    if (rmw) {
      // decode3_region's staging (the words of covered blocks are staged too
      // and not used)
      stage_batched(
          pairs,
          [&](uint32_t t) {
            const uint32_t l = __umulhi(t, a.wmagic);
            const uint64_t sb = spos[wv * 64 + l];
            const uint64_t gw = (sb >> 6) + (t - l * a.W);
            const uint32_t sh = (uint32_t)sb & 63u;
            const uint64_t lo = gw < a.out_words ? a.out[gw] : 0ull;
            const uint64_t hi = sh && gw + 1 < a.out_words ? a.out[gw + 1] : 0ull;
            return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
          },
          [&](uint32_t t, uint64_t x) { *slot_of(t) = x; });
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __builtin_amdgcn_wave_barrier();
      if (need) {
        WordReader r;
        r.w = myslot;
        r.pos = 0;
        if constexpr (D == 3 && !kIntField<S>)
          decode_block3<S, false, HI>(r, sq, v, cp);
        else
          decode_block_n<S, D, false>(r, sq, v, cp);
      }
      // the slot is the coder's next: zeroed
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = 0; i < a.swp; i++)
        myslot[i] = 0;
    }
    const RegionEncPos e = region_enc_pos<D>(g, rg, q);
    Geometry sg;
    sg.s[0] = rg.ds[0];
    sg.s[1] = rg.ds[1];
    sg.s[2] = rg.ds[2];
    BlockPos bp;
    bp.off = e.p.off;
    bp.cnt[0] = e.fc[0];
    bp.cnt[1] = e.fc[1];
    bp.cnt[2] = e.fc[2];
    bp.cnt[3] = 1;
    bp.full = e.infield;
    if (e.covered) {
      if constexpr (D == 3 && !kIntField<S>) {
        if (rg.vec && e.infield)
          gather3<S, true, true>(v, src, sg, bp);
        else
          gather3<S, false>(v, src, sg, bp);
      } else {
        gather_n<S, D>(v, src, sg, bp);
      }
    } else {
      region_overlay<S, D>(v, src, rg, e.p);
      if (!e.infield) {
        // the pad rule over the decoded block's values past the field's edge
        // (gather3 / gather_n's lines)
        const int cx = e.fc[0], cy = e.fc[1], cz = e.fc[2];
#pragma unroll
        for (int k = 0; k < (D > 2 ? 4 : 1); k++)
#pragma unroll
          for (int j = 0; j < (D > 1 ? 4 : 1); j++)
            if (k < cz && j < cy) pad_line(v, 16 * k + 4 * j, 1, cx);
        if constexpr (D > 1) {
#pragma unroll
          for (int k = 0; k < (D > 2 ? 4 : 1); k++)
#pragma unroll
            for (int i = 0; i < 4; i++)
              if (k < cz) pad_line(v, 16 * k + i, 4, cy);
        }
        if constexpr (D > 2) {
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++)
              pad_line(v, 4 * j + i, 16, cz);
        }
      }
    }
  };

  {
    S v[64];
#pragma unroll
    for (int i = 0; i < 64; i++)
      v[i] = (S)0;
    image(v);
    OrSlot os{myslot, 2 * a.swp - 1};
    if constexpr (D == 3 && !kIntField<S>)
      encode_block3<S, false, false, HI>(os, lut, v, cp, [&](S (&r)[64]) __attribute__((always_inline)) { image(r); });
    else
      encode_block_n<S, D, false>(os, lut, v, cp);
  }
  // the slots are this wave's own: LDS ops of a wave complete in order
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();

  const uint32_t wl = wv * 64;
  const uint32_t lane2 = lane_id_fresh();
  if ((a.maxbits & 63u) == 0 && !__any((spos[wl + lane2] & 63) != 0)) {
    // every block of the wave starts and ends on a word (wave-uniform): plain
    // stores only, consecutive in t within a block and across an x-run
    const uint32_t sw = a.maxbits >> 6;
    const uint32_t n = (uint32_t)nb * sw;
    for (uint32_t t = lane2; t < n; t += 64) {
      const uint32_t l = t / sw, j = t - l * sw;
      a.out[(spos[wl + l] >> 6) + j] = wslot[(size_t)l * a.swp + j];
    }
    return;
  }
  for (uint32_t t = lane2; t < pairs; t += 64) {
    const uint32_t l = __umulhi(t, a.wmagic), j = t - l * a.W;
    const uint64_t sb = spos[wl + l];
    MergeWord m;
    if (!merge_word(a.maxbits, (uint32_t)sb & 63u, j, &m))
      continue;
    const uint64_t bits = slot_bits(wslot + (size_t)l * a.swp, m.x0, m.cnt) << m.shl;
    uint64_t* w = a.out + (sb >> 6) + j;
    if (m.plain()) {
      *w = bits;
    } else {
      (void)__hip_atomic_fetch_and(w, ~m.mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_or(w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// HI: double with maxprec <= 32.  D: block dimensionality; 1D/2D blocks and
// integer fields take the generic per-lane codec (blockn.h).
template <typename S, bool HI = false, int D = 3>
__global__ __launch_bounds__(256, 1) void encode3_region(const S* __restrict__ src, Geometry g, CodecParams cp,
                                                        RegionGeom rg, RegionEncArgs a)
{
  __shared__ uint32_t lut[256];
  __shared__ uint32_t sq[256];
  __shared__ uint64_t spos[kWavesPerGroup * 64];
  extern __shared__ uint64_t lds[];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  uint64_t* wslot = lds + (size_t)wv * 64 * a.swp;
  // every wave writes both (identical) tables and zeroes its own slots: no
  // workgroup barrier
#pragma unroll
  for (int k = 0; k < 4; k++) {
    sq[lane + 64 * k] = squeeze_entry(lane + 64 * k);
    lut[lane + 64 * k] = kCoderTables.dbl[lane + 64 * k];
  }
  for (uint32_t i = lane; i < 64 * a.swp; i += 64)
    wslot[i] = 0;
  const uint64_t first = ((uint64_t)blockIdx.x * kWavesPerGroup + wv) * 64;
  if (first >= rg.nrblocks)  // (wave-uniform)
    return;
  region_enc_wave<S, HI, D>(src, g, cp, rg, a, first, lane, wv, lut, sq, spos, lds);
}

// Launcher (zfp_region_enc.hip holds every instantiation).  type: zfp_type;
// dims 1..3; hi: the f64 3D coder of planes 32..63 (maxprec <= 32).
void launch_encode_region(int type, int dims, bool hi, hipStream_t stream, dim3 grid, size_t lds, const void* src,
                          const Geometry& g, const CodecParams& cp, const RegionGeom& rg, const RegionEncArgs& a);

}  // namespace zfp_amd

#endif  // ZFP_REGION_MAPPING_ONLY
