// Host run of the batched region decoder's wave -> region mapping
// (kernels_boxes.h) against direct enumeration, and of the scatter through it.
//
// Mapping: for a list of regions given by their block counts, wave_first is
// built as the host builds it; box_wave must agree with a linear scan for every
// wave number up to and including the first wave past the end, and the lanes of
// all waves together (lane l of a wave takes block first + l of its region,
// active when that is below the region's block count, as region_wave decides)
// must visit every (region, block) pair exactly once.
//
// Scatter: two or three regions of one field, overlapping ones included, each
// with its own guarded destination; every lane "decodes" a block whose values
// are their own field coordinates and scatters it with region_scatter through
// its region's record.  Every region element must hold its own coordinates in
// its region's destination and nothing else may be written.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define ZFP_REGION_MAPPING_ONLY
#include "kernels_boxes.h"
using namespace zfp_amd;

static long g_lists = 0, g_bad = 0;

static std::vector<uint32_t> make_wave_first(const std::vector<uint64_t>& nrblocks)
{
  std::vector<uint32_t> wf(nrblocks.size() + 1);
  uint64_t waves = 0;
  for (size_t i = 0; i < nrblocks.size(); i++) {
    wf[i] = (uint32_t)waves;
    waves += box_waves(nrblocks[i]);
  }
  wf[nrblocks.size()] = (uint32_t)waves;
  return wf;
}

static void run_list(const std::vector<uint64_t>& nrblocks)
{
  const uint32_t n = (uint32_t)nrblocks.size();
  const std::vector<uint32_t> wf = make_wave_first(nrblocks);
  const uint32_t total = wf[n];
  std::vector<std::vector<int>> seen(n);
  for (uint32_t r = 0; r < n; r++)
    seen[r].assign(nrblocks[r], 0);
  bool ok = true;
  uint64_t active = 0, want_active = 0;
  for (uint32_t W = 0; W <= total; W++) {
    // linear scan: the last r with wave_first[r] <= W
    uint32_t r = 0;
    while (r < n && wf[r + 1] <= W)
      r++;
    const BoxWave w = box_wave(wf.data(), n, W);
    ok = ok && w.r == r && (r == n) == (W == total);
    if (!ok || r == n)
      continue;
    ok = ok && w.first == (uint64_t)(W - wf[r]) * 64 && w.first < nrblocks[r];
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint64_t q = w.first + lane;
      if (q < nrblocks[r]) {  // (act)
        seen[r][q]++;
        active++;
      }
    }
  }
  for (uint32_t r = 0; r < n; r++) {
    want_active += nrblocks[r];
    for (int s : seen[r])
      ok = ok && s == 1;
  }
  ok = ok && active == want_active;
  g_lists++;
  if (!ok && g_bad++ < 5) {
    printf("BAD list");
    for (uint64_t b : nrblocks)
      printf(" %llu", (unsigned long long)b);
    printf("\n");
  }
}

static void mapping_lists()
{
  const uint64_t counts[6] = {1, 63, 64, 65, 128, 257};
  for (int len = 1; len <= 4; len++) {
    int total = 1;
    for (int k = 0; k < len; k++)
      total *= 6;
    for (int code = 0; code < total; code++) {
      std::vector<uint64_t> l;
      for (int k = 0, c = code; k < len; k++, c /= 6)
        l.push_back(counts[c % 6]);
      run_list(l);
    }
  }
  for (size_t ones : {1u, 2u, 64u, 65u, 1000u})
    run_list(std::vector<uint64_t>(ones, 1));
}

// ---- scatter through the mapping ----
struct Box {
  uint64_t lo[3], hi[3];
};

static int32_t code_of(uint64_t x, uint64_t y, uint64_t z) { return (int32_t)(x | (y << 8) | (z << 16)); }

static long g_sets = 0, g_sbad = 0;

static void run_set(const uint64_t* n, const std::vector<Box>& boxes)
{
  Geometry g{};
  g.nblocks = 1;
  for (int a = 0; a < 4; a++) {
    g.n[a] = a < 3 ? n[a] : 1;
    g.f[a] = 0;
    g.nb[a] = a < 3 ? (uint32_t)((n[a] + 3) / 4) : 1;
    g.nblocks *= g.nb[a];
  }
  for (int a = 0; a < 3; a++)
    g.dv[a] = make_fastdiv(g.nb[a]);
  // per region: a destination with a guard band of 4 in x and 1 elsewhere,
  // strides multiples of 4, a 16-byte aligned first element
  const size_t nr = boxes.size();
  std::vector<std::vector<int32_t>> store(nr);
  std::vector<BoxRecord> rec(nr);
  std::vector<uint64_t> nrblocks(nr);
  std::vector<int64_t> sy(nr), sz(nr);
  for (size_t i = 0; i < nr; i++) {
    uint64_t ext[3];
    for (int a = 0; a < 3; a++)
      ext[a] = boxes[i].hi[a] - boxes[i].lo[a];
    sy[i] = (int64_t)((ext[0] + 8 + 3) & ~3ull);
    sz[i] = sy[i] * (int64_t)(ext[1] + 2);
    store[i].assign((size_t)sz[i] * (ext[2] + 2) + 4, -1);
    int32_t* base = store[i].data();
    while (reinterpret_cast<uintptr_t>(base) & 15)
      base++;
    const int64_t ds[3] = {1, sy[i], sz[i]};
    rec[i].rg = make_region_geom(g, 3, boxes[i].lo, boxes[i].hi, ds);
    rec[i].dst = base + 4 + sy[i] + sz[i];
    rec[i].rg.vec = region_vec_ok(rec[i].rg, 3, rec[i].dst) ? 1u : 0u;
    nrblocks[i] = rec[i].rg.nrblocks;
  }
  const std::vector<uint32_t> wf = make_wave_first(nrblocks);
  for (uint32_t W = 0; W < wf[nr]; W++) {
    const BoxWave w = box_wave(wf.data(), (uint32_t)nr, W);
    const RegionGeom& rg = rec[w.r].rg;
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint64_t q = w.first + lane;
      if (q >= rg.nrblocks)
        continue;
      const RegionPos p = region_pos<3>(g, rg, (uint32_t)q);
      uint64_t b = p.B, bc[3];
      for (int a = 0; a < 3; a++) {
        bc[a] = b % g.nb[a];
        b /= g.nb[a];
      }
      int32_t v[64];
      for (int idx = 0; idx < 64; idx++)
        v[idx] = code_of(4 * bc[0] + (idx & 3), 4 * bc[1] + ((idx >> 2) & 3), 4 * bc[2] + (idx >> 4));
      region_scatter<int32_t, 3>(v, (int32_t*)rec[w.r].dst, rg, p);
    }
  }
  bool ok = true;
  for (size_t i = 0; i < nr; i++) {
    uint64_t ext[3];
    for (int a = 0; a < 3; a++)
      ext[a] = boxes[i].hi[a] - boxes[i].lo[a];
    const int32_t* base = (const int32_t*)rec[i].dst - 4 - sy[i] - sz[i];
    const size_t total = (size_t)sz[i] * (ext[2] + 2);
    for (size_t k = 0; ok && k < total; k++) {
      const int64_t x = (int64_t)(k % (size_t)sy[i]) - 4;
      const int64_t y = (int64_t)(k / (size_t)sy[i] % (ext[1] + 2)) - 1;
      const int64_t z = (int64_t)(k / (size_t)sz[i]) - 1;
      const bool in = x >= 0 && x < (int64_t)ext[0] && y >= 0 && y < (int64_t)ext[1] && z >= 0 && z < (int64_t)ext[2];
      const int32_t expect = in ? code_of(boxes[i].lo[0] + x, boxes[i].lo[1] + y, boxes[i].lo[2] + z) : -1;
      ok = base[k] == expect;
    }
    for (const int32_t* q = store[i].data(); ok && q < base; q++)
      ok = *q == -1;
  }
  g_sets++;
  if (!ok && g_sbad++ < 5)
    printf("BAD set of %zu regions, field %llu %llu %llu\n", nr, (unsigned long long)n[0], (unsigned long long)n[1],
           (unsigned long long)n[2]);
}

static void scatter_sets()
{
  const uint64_t fields[3][3] = {{9, 6, 5}, {8, 4, 4}, {5, 6, 3}};
  for (const auto& n : fields) {
    // the whole field, its block-aligned low corner, an unaligned interior box,
    // one element, an x row, a z column, the high corner, a box sharing blocks
    // with most of the others
    std::vector<Box> pool;
    auto add = [&](uint64_t x0, uint64_t x1, uint64_t y0, uint64_t y1, uint64_t z0, uint64_t z1) {
      Box b{{std::min(x0, n[0] - 1), std::min(y0, n[1] - 1), std::min(z0, n[2] - 1)},
            {std::min(x1, n[0]), std::min(y1, n[1]), std::min(z1, n[2])}};
      for (int a = 0; a < 3; a++)
        if (b.hi[a] <= b.lo[a])
          b.hi[a] = b.lo[a] + 1;
      pool.push_back(b);
    };
    add(0, 99, 0, 99, 0, 99);
    add(0, 4, 0, 4, 0, 4);
    add(1, 7, 1, 5, 1, 4);
    add(5, 6, 2, 3, 3, 4);
    add(0, 99, 3, 4, 1, 2);
    add(2, 3, 4, 5, 0, 99);
    add(4, 99, 4, 99, 2, 99);
    add(3, 9, 0, 6, 0, 3);
    for (size_t i = 0; i < pool.size(); i++)
      for (size_t j = 0; j < pool.size(); j++) {
        run_set(n, {pool[i], pool[j]});
        for (size_t k = 0; k < pool.size(); k++)
          run_set(n, {pool[i], pool[j], pool[k]});
      }
  }
}

int main()
{
  mapping_lists();
  printf("mapping mismatches %ld of %ld lists\n", g_bad, g_lists);
  scatter_sets();
  printf("scatter mismatches %ld of %ld region sets\n", g_sbad, g_sets);
  return g_bad || g_sbad ? 1 : 0;
}
