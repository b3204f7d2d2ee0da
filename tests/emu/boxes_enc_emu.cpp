// Host run of the batched region encoder's host-compilable parts: the
// disjointness test of host_disjoint.h against the all-pairs brute force, and
// batches of regions through box_wave (kernels_boxes.h) and the merge
// decisions (region_enc_pos, merge_word of kernels_region_enc.h).
//
// Disjointness: random sets of 1 to 40 boxes in 1D, 2D and 3D on small grids,
// and the edge cases -- boxes touching at a face, sharing exactly one corner
// block, identical, nested, 1000 coplanar one-block boxes with and without one
// duplicate.  A reported pair must be a true intersection of two different
// entries; "none" must mean the brute force finds none.
//
// Merge: batches of two and three regions with pairwise disjoint block sets,
// at 208 bits per block from bit 0 and from bit 96, so that blocks of
// different regions share stream words.  The waves of the batch are run
// serially in forward and in reversed order; every active lane merges its
// block's words as the kernel decides (plain store, or and/or with the mask).
// Every stream bit of a touched block must be written exactly once, by the
// block that owns it; no other bit may be written; the words must equal the
// old words with the touched blocks replaced.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#define ZFP_REGION_MAPPING_ONLY
#include "host_disjoint.h"
#include "kernels_boxes_enc.h"
using namespace zfp_amd;

// ---- disjointness ----
static long g_sets = 0, g_bad = 0;

static bool brute(const std::vector<BlockBox>& b)
{
  for (size_t i = 0; i < b.size(); i++)
    for (size_t j = i + 1; j < b.size(); j++)
      if (block_boxes_meet(b[i], b[j]))
        return true;
  return false;
}

static bool meet_by_enumeration(const BlockBox& p, const BlockBox& q)
{
  for (uint32_t z = p.b0[2]; z < p.b0[2] + p.nb[2]; z++)
    for (uint32_t y = p.b0[1]; y < p.b0[1] + p.nb[1]; y++)
      for (uint32_t x = p.b0[0]; x < p.b0[0] + p.nb[0]; x++)
        if (x >= q.b0[0] && x < q.b0[0] + q.nb[0] && y >= q.b0[1] && y < q.b0[1] + q.nb[1] && z >= q.b0[2] &&
            z < q.b0[2] + q.nb[2])
          return true;
  return false;
}

// expect: -1 compare with the brute force only, 0 disjoint, 1 some pair meets
static void run_set(const std::vector<BlockBox>& b, int dims, int expect, const char* name)
{
  bool ok = true;
  const bool want = brute(b);
  for (int axis = 0; axis < 3; axis++) {  // (the library sweeps along dims - 1; every axis must be right)
    size_t ia = ~(size_t)0, ib = ~(size_t)0;
    const bool got = first_shared_block(b.data(), b.size(), axis, &ia, &ib);
    ok = ok && got == want;
    if (got)
      ok = ok && ia < ib && ib < b.size() && meet_by_enumeration(b[ia], b[ib]);
  }
  if (expect >= 0)
    ok = ok && want == (expect == 1);
  (void)dims;
  g_sets++;
  if (!ok && g_bad++ < 5)
    printf("BAD set %s (%zu boxes)\n", name, b.size());
}

static BlockBox bb(uint32_t x0, uint32_t nx, uint32_t y0 = 0, uint32_t ny = 1, uint32_t z0 = 0, uint32_t nz = 1)
{
  return BlockBox{{x0, y0, z0}, {nx, ny, nz}};
}

static void disjoint_sets()
{
  std::mt19937 rng(7);
  for (int dims = 1; dims <= 3; dims++)
    for (int grid : {6, 12, 40})
      for (int rep = 0; rep < 400; rep++) {
        const size_t n = 1 + rng() % 40;
        const uint32_t maxext = 1 + rng() % 4;
        std::vector<BlockBox> b(n);
        for (auto& x : b)
          for (int a = 0; a < 3; a++) {
            x.b0[a] = a < dims ? rng() % grid : 0;
            x.nb[a] = a < dims ? 1 + rng() % maxext : 1;
          }
        run_set(b, dims, -1, "random");
      }
  run_set({bb(0, 2, 0, 2, 0, 2)}, 3, 0, "single");
  run_set({bb(0, 2, 0, 2, 0, 2), bb(2, 2, 0, 2, 0, 2)}, 3, 0, "touching at an x face");
  run_set({bb(0, 2, 0, 2, 0, 2), bb(0, 2, 2, 2, 0, 2)}, 3, 0, "touching at a y face");
  run_set({bb(0, 2, 0, 2, 0, 2), bb(0, 2, 0, 2, 2, 2)}, 3, 0, "touching at a z face");
  run_set({bb(0, 2, 0, 2, 0, 2), bb(2, 2, 2, 2, 2, 2)}, 3, 0, "touching at a corner");
  run_set({bb(0, 2, 0, 2, 0, 2), bb(1, 2, 1, 2, 1, 2)}, 3, 1, "sharing one corner block");
  run_set({bb(3, 2, 1, 2, 0, 2), bb(3, 2, 1, 2, 0, 2)}, 3, 1, "identical");
  run_set({bb(0, 8, 0, 8, 0, 8), bb(3, 1, 4, 2, 5, 1)}, 3, 1, "nested");
  run_set({bb(3, 1, 4, 2, 5, 1), bb(9, 1, 9, 1, 9, 1), bb(0, 8, 0, 8, 0, 8)}, 3, 1, "nested, given last");
  {
    std::vector<BlockBox> b;
    for (uint32_t i = 0; i < 1000; i++)
      b.push_back(bb(i % 40, 1, i / 40, 1, 3, 1));
    run_set(b, 3, 0, "1000 coplanar");
    b.push_back(b[517]);
    run_set(b, 3, 1, "1000 coplanar and one duplicate");
    std::swap(b[0], b[1000]);
    run_set(b, 3, 1, "1000 coplanar and one duplicate, given first");
  }
}

// ---- merge through the batch's mapping ----
struct Box {
  uint64_t lo[3], hi[3];
};

static bool get_bit(const std::vector<uint64_t>& w, uint64_t i) { return (w[i >> 6] >> (i & 63)) & 1u; }
static void set_bit(std::vector<uint64_t>& w, uint64_t i, bool b)
{
  w[i >> 6] = (w[i >> 6] & ~(1ull << (i & 63))) | ((uint64_t)b << (i & 63));
}

static long g_batches = 0, g_mbad = 0, g_shared = 0;  // g_shared: batches in which two regions met in a word

static void run_batch(const uint64_t* n, const std::vector<Box>& boxes, uint32_t maxbits, uint64_t bit0, bool reversed)
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
  const size_t nr = boxes.size();
  std::vector<RegionGeom> rg(nr);
  std::vector<BlockBox> bbx(nr);
  std::vector<uint32_t> wf(nr + 1);
  uint64_t waves = 0;
  const int64_t ds[3] = {1, 64, 4096};
  for (size_t i = 0; i < nr; i++) {
    rg[i] = make_region_geom(g, 3, boxes[i].lo, boxes[i].hi, ds);
    for (int a = 0; a < 3; a++) {
      bbx[i].b0[a] = rg[i].rb0[a];
      bbx[i].nb[a] = rg[i].rnb[a];
    }
    wf[i] = (uint32_t)waves;
    waves += box_waves(rg[i].nrblocks);
  }
  wf[nr] = (uint32_t)waves;
  bool ok = true;
  size_t ia, ib;
  ok = ok && !first_shared_block(bbx.data(), nr, 2, &ia, &ib);  // (the batches here are legal ones)

  std::mt19937_64 rng(maxbits * 131 + bit0 + nr);
  const uint64_t nwords = (bit0 + g.nblocks * maxbits + 63) / 64 + 1;  // (one word past the blocks)
  std::vector<uint64_t> old(nwords);
  for (auto& w : old)
    w = rng();
  const uint32_t sw = maxbits / 64 + 2;
  std::vector<std::vector<uint64_t>> slot(g.nblocks, std::vector<uint64_t>(sw));
  for (auto& s : slot)
    for (auto& w : s)
      w = rng();

  std::vector<uint64_t> w = old, want = old;
  std::vector<uint8_t> writes(nwords * 64, 0), plain(nwords, 0), masked(nwords, 0), touched(g.nblocks, 0);
  const uint32_t Wn = merge_words(maxbits);
  bool shared_word = false;  // a word that holds bits of blocks of two different regions
  std::vector<int> word_region(nwords, -1);
  for (uint64_t k = 0; k < waves; k++) {
    const uint32_t W = (uint32_t)(reversed ? waves - 1 - k : k);
    const BoxWave bw = box_wave(wf.data(), (uint32_t)nr, W);
    ok = ok && bw.r < nr;
    if (bw.r >= nr)
      break;
    const RegionGeom& r = rg[bw.r];
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint64_t q = bw.first + lane;
      if (q >= r.nrblocks)  // (padding lanes take no part in the copy-out)
        continue;
      const RegionEncPos e = region_enc_pos<3>(g, r, (uint32_t)q);
      const uint64_t B = e.p.B;
      ok = ok && B < g.nblocks && !touched[B];
      touched[B] = 1;
      const uint64_t pos = bit0 + B * maxbits;
      for (uint32_t j = 0; j < Wn; j++) {
        MergeWord m;
        if (!merge_word(maxbits, (uint32_t)(pos & 63), j, &m))
          continue;
        uint64_t bits = 0;
        for (uint32_t i = 0; i < m.cnt; i++)
          bits |= (uint64_t)get_bit(slot[B], m.x0 + i) << i;
        bits <<= m.shl;
        const uint64_t gw = (pos >> 6) + j;
        if (word_region[gw] >= 0 && word_region[gw] != (int)bw.r)
          shared_word = true;
        word_region[gw] = (int)bw.r;
        for (uint32_t i = 0; i < m.cnt; i++) {
          // the stream bit and the block that owns it
          const uint64_t sb = gw * 64 + m.shl + i;
          ok = ok && sb >= bit0 && (sb - bit0) / maxbits == B && (sb - bit0) % maxbits == m.x0 + i;
          writes[sb]++;
        }
        if (m.plain()) {
          plain[gw]++;
          w[gw] = bits;
        } else {
          masked[gw] = 1;
          w[gw] = (w[gw] & ~m.mask) | bits;
        }
      }
    }
  }
  uint64_t nblocks_touched = 0, want_blocks = 0;
  for (size_t i = 0; i < nr; i++)
    want_blocks += rg[i].nrblocks;
  for (uint64_t B = 0; B < g.nblocks; B++) {
    nblocks_touched += touched[B];
    if (touched[B])
      for (uint32_t i = 0; i < maxbits; i++)
        set_bit(want, bit0 + B * maxbits + i, get_bit(slot[B], i));
  }
  ok = ok && nblocks_touched == want_blocks;
  for (uint64_t sb = 0; sb < nwords * 64; sb++) {
    const bool in = sb >= bit0 && (sb - bit0) / maxbits < g.nblocks && touched[(sb - bit0) / maxbits];
    ok = ok && writes[sb] == (in ? 1 : 0);
  }
  for (uint64_t i = 0; i < nwords; i++)
    ok = ok && !(plain[i] && masked[i]) && plain[i] <= 1;
  ok = ok && w == want;
  for (uint64_t i = 0; i < nwords; i++)
    if (word_region[i] < 0)
      ok = ok && w[i] == old[i];
  g_shared += shared_word;
  g_batches++;
  if (!ok && g_mbad++ < 5)
    printf("BAD batch of %zu regions, maxbits %u bit0 %llu reversed %d\n", nr, maxbits, (unsigned long long)bit0,
           (int)reversed);
}

static void merge_batches()
{
  // 10 x 5 x 3 blocks
  const uint64_t n[3] = {40, 20, 12};
  const std::vector<std::vector<Box>> batches = {
      // x neighbours in one row of blocks
      {{{0, 0, 0}, {4, 4, 4}}, {{4, 0, 0}, {8, 4, 4}}},
      // a region longer than one wave (100 blocks) and a cut one above it
      {{{0, 0, 0}, {40, 20, 8}}, {{3, 2, 9}, {30, 11, 12}}},
      // one element, a cut box next to it, a slab
      {{{17, 9, 5}, {18, 10, 6}}, {{20, 8, 4}, {27, 13, 7}}, {{0, 0, 8}, {40, 20, 12}}},
      // three x neighbours that are not block aligned in their elements but are in their blocks
      {{{1, 1, 1}, {3, 3, 3}}, {{5, 1, 1}, {12, 3, 3}}, {{12, 0, 0}, {40, 4, 4}}},
      // interleaved rows: y neighbours over the full x extent
      {{{0, 0, 0}, {40, 4, 4}}, {{0, 4, 0}, {40, 8, 4}}, {{0, 8, 0}, {40, 12, 4}}},
  };
  for (const auto& b : batches)
    for (uint32_t maxbits : {208u})
      for (uint64_t bit0 : {0ull, 96ull})
        for (int rev = 0; rev < 2; rev++) {
          run_batch(n, b, maxbits, bit0, rev != 0);
          std::vector<Box> r(b.rbegin(), b.rend());  // the entries the other way round as well
          run_batch(n, r, maxbits, bit0, rev != 0);
        }
}

int main()
{
  disjoint_sets();
  printf("disjointness mismatches %ld of %ld sets\n", g_bad, g_sets);
  merge_batches();
  printf("merge mismatches %ld of %ld batches, %ld with a word shared by two regions\n", g_mbad, g_batches, g_shared);
  return g_bad || g_mbad || g_shared * 2 < g_batches ? 1 : 0;
}
