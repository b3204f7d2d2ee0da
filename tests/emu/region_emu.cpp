// Host run of the region decoder's mapping, clipped scatter and start-table
// arithmetic (kernels_region.h) against direct enumeration.
//
// Mapping and scatter: for every field, every coded box [f, e) with
// block-aligned f and every region [lo, hi) inside it (extents <= 9 in 1D,
// <= (9, 6) in 2D, <= (9, 6, 5) in 3D), every region block is "decoded" to a
// block whose values are their own field coordinates and scattered into a
// destination with a guard band.  Every region element must hold its own
// coordinates, nothing else may be written, the windows' volumes must add up
// to the region's (so no element is written twice), and the stream block
// numbers visited must be the blocks that intersect the region.
//
// Start table: start_lane_block / start_entry with the wave scan run as the
// GPU's shuffle steps, against a serial prefix sum of random 16-bit lengths.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#define ZFP_REGION_MAPPING_ONLY
#include "kernels_region.h"
using namespace zfp_amd;

static long g_cases = 0, g_bad = 0;

static int32_t code_of(uint64_t x, uint64_t y, uint64_t z) { return (int32_t)(x | (y << 8) | (z << 16)); }

template <int D>
static void run_region(const uint64_t* n, const uint64_t* f, const uint64_t* e, const uint64_t* lo, const uint64_t* hi)
{
  Geometry g{};
  g.nblocks = 1;
  for (int a = 0; a < 4; a++) {
    g.n[a] = a < D ? n[a] : 1;
    g.f[a] = a < D ? f[a] : 0;
    g.nb[a] = a < D ? (uint32_t)((e[a] - f[a] + 3) / 4) : 1;
    g.nblocks *= g.nb[a];
  }
  for (int a = 0; a < 3; a++)
    g.dv[a] = make_fastdiv(g.nb[a]);
  // destination: guard band of 4 in x and 1 elsewhere, strides multiples of 4,
  // 16-byte aligned first element (so 16-byte rows are taken when lo - f is a
  // block boundary in x, scalar stores otherwise)
  uint64_t ext[3] = {1, 1, 1};
  for (int a = 0; a < D; a++)
    ext[a] = hi[a] - lo[a];
  const int64_t sy = (int64_t)((ext[0] + 8 + 3) & ~3ull), sz = sy * (int64_t)(ext[1] + 2);
  const size_t total = (size_t)sz * (ext[2] + 2);
  alignas(16) static int32_t buf[32 * 16 * 16];
  if (total > sizeof buf / sizeof buf[0]) {
    printf("buffer too small\n");
    exit(2);
  }
  std::fill(buf, buf + total, -1);
  int32_t* dst = buf + 4 + (D > 1 ? sy : 0) + (D > 2 ? sz : 0);
  const int64_t ds[3] = {1, sy, sz};
  RegionGeom rg = make_region_geom(g, D, lo, hi, ds);
  rg.vec = region_vec_ok(rg, D, dst) ? 1u : 0u;
  uint64_t want_blocks = 1;
  for (int a = 0; a < D; a++)
    want_blocks *= (hi[a] - 1 - f[a]) / 4 - (lo[a] - f[a]) / 4 + 1;
  bool ok = rg.nrblocks == want_blocks;
  std::vector<uint64_t> seen;
  uint64_t volume = 0;
  for (uint32_t q = 0; ok && q < rg.nrblocks; q++) {
    const RegionPos p = region_pos<D>(g, rg, q);
    seen.push_back(p.B);
    // the block's coordinates from its stream number, as the encoder laid it out
    uint64_t b = p.B, bc[3] = {0, 0, 0};
    for (int a = 0; a < D; a++) {
      bc[a] = b % g.nb[a];
      b /= g.nb[a];
    }
    int32_t v[64];
    for (int idx = 0; idx < 64; idx++)
      v[idx] = code_of(f[0] + 4 * bc[0] + (idx & 3), D > 1 ? f[1] + 4 * bc[1] + ((idx >> 2) & 3) : 0,
                       D > 2 ? f[2] + 4 * bc[2] + (idx >> 4) : 0);
    uint64_t vol = 1;
    for (int a = 0; a < D; a++) {
      ok = ok && p.c0[a] >= 0 && p.c0[a] < p.c1[a] && p.c1[a] <= 4;
      vol *= (uint64_t)(p.c1[a] - p.c0[a]);
    }
    ok = ok && p.full == (vol == (1ull << (2 * D)));
    volume += vol;
    if (ok)
      region_scatter<int32_t, D>(v, dst, rg, p);
  }
  ok = ok && volume == ext[0] * ext[1] * ext[2];
  // the blocks that intersect the region, by enumeration
  std::vector<uint64_t> want;
  for (uint64_t bz = 0; bz < g.nb[2]; bz++)
    for (uint64_t by = 0; by < g.nb[1]; by++)
      for (uint64_t bx = 0; bx < g.nb[0]; bx++) {
        const uint64_t bc[3] = {bx, by, bz};
        bool hit = true;
        for (int a = 0; a < D; a++)
          hit = hit && f[a] + 4 * bc[a] < hi[a] && f[a] + 4 * bc[a] + 4 > lo[a];
        if (hit)
          want.push_back(bx + g.nb[0] * (by + g.nb[1] * bz));
      }
  std::sort(seen.begin(), seen.end());
  ok = ok && seen == want;
  // every element of the buffer: its coordinates inside the region, the sentinel outside
  for (size_t i = 0; ok && i < total; i++) {
    const int64_t x = (int64_t)(i % (size_t)sy) - 4;
    const int64_t y = (int64_t)(i / (size_t)sy % (ext[1] + 2)) - (D > 1 ? 1 : 0);
    const int64_t z = (int64_t)(i / (size_t)sz) - (D > 2 ? 1 : 0);
    const bool in = x >= 0 && x < (int64_t)ext[0] && y >= 0 && y < (int64_t)ext[1] && z >= 0 && z < (int64_t)ext[2];
    const int32_t expect = in ? code_of(lo[0] + x, D > 1 ? lo[1] + y : 0, D > 2 ? lo[2] + z : 0) : -1;
    ok = buf[i] == expect;
  }
  g_cases++;
  if (!ok && g_bad++ < 5) {
    printf("BAD %dD n", D);
    for (int a = 0; a < D; a++)
      printf(" %llu", (unsigned long long)n[a]);
    for (int a = 0; a < D; a++)
      printf(" box[%llu,%llu) region[%llu,%llu)", (unsigned long long)f[a], (unsigned long long)e[a],
             (unsigned long long)lo[a], (unsigned long long)hi[a]);
    printf("\n");
  }
}

// every (n, f, e, lo, hi) of one axis with n <= maxn
struct Axis {
  uint64_t n, f, e, lo, hi;
};

static std::vector<Axis> axis_cases(uint64_t maxn)
{
  std::vector<Axis> v;
  for (uint64_t n = 1; n <= maxn; n++)
    for (uint64_t f = 0; f < n; f += 4)
      for (uint64_t e = f + 1; e <= n; e++)
        for (uint64_t lo = f; lo < e; lo++)
          for (uint64_t hi = lo + 1; hi <= e; hi++)
            v.push_back(Axis{n, f, e, lo, hi});
  return v;
}

template <int D>
static void run_all(const uint64_t* maxn)
{
  std::vector<Axis> ax[3];
  for (int a = 0; a < 3; a++)
    ax[a] = a < D ? axis_cases(maxn[a]) : std::vector<Axis>{Axis{1, 0, 1, 0, 1}};
  const long before = g_cases;
  for (const Axis& z : ax[2])
    for (const Axis& y : ax[1])
      for (const Axis& x : ax[0]) {
        const uint64_t n[3] = {x.n, y.n, z.n}, f[3] = {x.f, y.f, z.f}, e[3] = {x.e, y.e, z.e};
        const uint64_t lo[3] = {x.lo, y.lo, z.lo}, hi[3] = {x.hi, y.hi, z.hi};
        run_region<D>(n, f, e, lo, hi);
      }
  printf("%dD: %ld regions\n", D, g_cases - before);
}

// wave_incl_scan's shuffle steps over the 64 lanes of one wave
static void emu_wave_incl_scan(uint32_t (&x)[64])
{
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t y[64];
    for (int l = 0; l < 64; l++)
      y[l] = l >= d ? x[l - d] : 0;
    for (int l = 0; l < 64; l++)
      if (l >= d)
        x[l] += y[l];
  }
}

static long start_table_mismatches()
{
  long bad = 0;
  std::mt19937_64 rng(7);
  for (uint32_t per_wave : {64u, 16u})
    for (uint64_t nb : {1ull, 63ull, 64ull, 65ull, 1000ull}) {
      std::vector<uint16_t> len(nb);
      std::vector<uint64_t> truth(nb);
      uint64_t p = 0;
      for (uint64_t b = 0; b < nb; b++) {
        len[b] = (uint16_t)rng();
        truth[b] = p;
        p += len[b];
      }
      const uint64_t nwaves = (nb + per_wave - 1) / per_wave;
      std::vector<uint64_t> base(nwaves), start(nb, ~0ull);
      for (uint64_t w = 0; w < nwaves; w++)
        base[w] = truth[w * per_wave];
      for (uint64_t w = 0; w < nwaves; w++) {
        uint32_t l[64], incl[64];
        uint64_t blk[64];
        bool act[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
          act[lane] = start_lane_block(w, per_wave, lane, nb, &blk[lane]);
          l[lane] = incl[lane] = act[lane] ? len[blk[lane]] : 0u;
        }
        emu_wave_incl_scan(incl);
        for (uint32_t lane = 0; lane < 64; lane++)
          if (act[lane]) {
            if (start[blk[lane]] != ~0ull)
              bad++;  // written twice
            start[blk[lane]] = start_entry(base[w], incl[lane], l[lane]);
          }
      }
      for (uint64_t b = 0; b < nb; b++)
        bad += start[b] != truth[b];
    }
  return bad;
}

int main()
{
  const uint64_t m1[3] = {9, 1, 1}, m2[3] = {9, 6, 1}, m3[3] = {9, 6, 5};
  run_all<1>(m1);
  run_all<2>(m2);
  run_all<3>(m3);
  printf("region mismatches %ld of %ld\n", g_bad, g_cases);
  const long sb = start_table_mismatches();
  printf("start table mismatches %ld\n", sb);
  return g_bad || sb ? 1 : 0;
}
