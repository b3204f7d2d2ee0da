// Host run of the region encoder's covered rule, overlay and merge arithmetic
// (the host-compilable part of kernels_region_enc.h) against direct enumeration.
//
// Covered rule and overlay: for every field, every coded box [f, e) with
// block-aligned f and every region [lo, hi) inside it (extents <= 9 in 1D,
// <= (9, 6) in 2D, <= (9, 6, 5) in 3D), every region block starts as a block of
// sentinels and is overlaid from a strided source whose elements hold their own
// field coordinates.  `covered`, `infield` and the in-field counts must equal
// direct enumeration; every position of the block inside the region must hold
// its own coordinates and every other position the sentinel; the positions
// written must add up to the region's volume (each element exactly once).
//
// Merge: for every (maxbits, bit0) a row of 70 blocks over random old words and
// every run [a, b] of blocks: the plain-store and and/or decisions of
// merge_word, applied serially in two different block orders, must both give
// the old words with exactly the run's bits replaced, and no word may receive
// both a plain store and a masked update (nor two plain stores).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#define ZFP_REGION_MAPPING_ONLY
#include "kernels_region_enc.h"
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
  // source: the region's elements with a guard band, each its own coordinates
  uint64_t ext[3] = {1, 1, 1};
  for (int a = 0; a < D; a++)
    ext[a] = hi[a] - lo[a];
  const int64_t sy = (int64_t)(ext[0] + 3), sz = sy * (int64_t)(ext[1] + 2);
  const size_t total = (size_t)sz * (ext[2] + 2);
  static int32_t buf[16 * 16 * 16];
  if (total > sizeof buf / sizeof buf[0]) {
    printf("buffer too small\n");
    exit(2);
  }
  std::fill(buf, buf + total, -2);
  int32_t* src = buf + 1 + (D > 1 ? sy : 0) + (D > 2 ? sz : 0);
  for (uint64_t z = 0; z < ext[2]; z++)
    for (uint64_t y = 0; y < ext[1]; y++)
      for (uint64_t x = 0; x < ext[0]; x++)
        src[(int64_t)x + (int64_t)y * sy + (int64_t)z * sz] =
            code_of(lo[0] + x, D > 1 ? lo[1] + y : 0, D > 2 ? lo[2] + z : 0);
  const int64_t ds[3] = {1, sy, sz};
  const RegionGeom rg = make_region_geom(g, D, lo, hi, ds);
  bool ok = true;
  uint64_t written = 0;
  for (uint32_t q = 0; ok && q < rg.nrblocks; q++) {
    const RegionEncPos p = region_enc_pos<D>(g, rg, q);
    uint64_t b = p.p.B, bc[3] = {0, 0, 0};
    for (int a = 0; a < D; a++) {
      bc[a] = b % g.nb[a];
      b /= g.nb[a];
    }
    // direct enumeration: the block's elements inside the field, and whether all lie in the region
    bool covered = true, infield = true;
    for (int a = 0; a < D; a++) {
      const uint64_t x0 = f[a] + 4 * bc[a];
      int cnt = 0;
      for (uint64_t x = x0; x < x0 + 4; x++) {
        if (x >= n[a]) {
          infield = false;
          continue;
        }
        cnt++;
        covered = covered && x >= lo[a] && x < hi[a];
      }
      ok = ok && p.fc[a] == cnt;
    }
    ok = ok && p.covered == covered && p.infield == infield;
    int32_t v[64];
    for (int idx = 0; idx < 64; idx++)
      v[idx] = -1;
    region_overlay<int32_t, D>(v, src, rg, p.p);
    for (int idx = 0; idx < 64; idx++) {
      const uint64_t c[3] = {f[0] + 4 * bc[0] + (idx & 3), D > 1 ? f[1] + 4 * bc[1] + ((idx >> 2) & 3) : 0,
                             D > 2 ? f[2] + 4 * bc[2] + (idx >> 4) : 0};
      bool in = idx < (1 << (2 * D));
      for (int a = 0; a < D; a++)
        in = in && c[a] >= lo[a] && c[a] < hi[a];
      ok = ok && v[idx] == (in ? code_of(c[0], c[1], c[2]) : -1);
      written += in;
    }
  }
  ok = ok && written == ext[0] * ext[1] * ext[2];
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

// ---- merge ----
static bool get_bit(const std::vector<uint64_t>& w, uint64_t i) { return (w[i >> 6] >> (i & 63)) & 1u; }
static void set_bit(std::vector<uint64_t>& w, uint64_t i, bool b)
{
  w[i >> 6] = (w[i >> 6] & ~(1ull << (i & 63))) | ((uint64_t)b << (i & 63));
}

static long g_merge_cases = 0;

static long merge_mismatches()
{
  long bad = 0;
  std::mt19937_64 rng(13);
  constexpr uint32_t NB = 70;
  for (uint32_t maxbits : {9u, 13u, 32u, 52u, 64u, 208u, 320u, 512u})
    for (uint64_t bit0 : {0ull, 1ull, 32ull, 63ull, 96ull}) {
      const uint64_t nwords = (bit0 + (uint64_t)NB * maxbits + 63) / 64 + 1;  // (one word past the blocks)
      std::vector<uint64_t> old(nwords);
      for (auto& w : old)
        w = rng();
      // every block's new bits: a slot as the coder leaves it, with overhang past maxbits
      const uint32_t sw = maxbits / 64 + 2;
      std::vector<std::vector<uint64_t>> slot(NB, std::vector<uint64_t>(sw));
      for (auto& s : slot)
        for (auto& w : s)
          w = rng();
      const uint32_t W = merge_words(maxbits);
      for (uint32_t a = 0; a < NB; a++)
        for (uint32_t b = a; b < NB; b++) {
          std::vector<uint64_t> want = old;
          for (uint32_t l = a; l <= b; l++)
            for (uint32_t i = 0; i < maxbits; i++)
              set_bit(want, bit0 + (uint64_t)l * maxbits + i, get_bit(slot[l], i));
          for (int order = 0; order < 2; order++) {
            std::vector<uint32_t> seq;
            for (uint32_t l = a; l <= b; l++)
              seq.push_back(l);
            if (order)  // odd blocks downwards, then even blocks upwards
              std::stable_sort(seq.begin(), seq.end(), [](uint32_t x, uint32_t y) {
                return (x & 1) != (y & 1) ? (x & 1) > (y & 1) : (x & 1) ? x > y : x < y;
              });
            std::vector<uint64_t> w = old;
            std::vector<uint8_t> plain(nwords, 0), masked(nwords, 0);
            uint64_t covered_bits = 0;
            for (uint32_t l : seq) {
              const uint64_t pos = bit0 + (uint64_t)l * maxbits;
              for (uint32_t j = 0; j < W + 1; j++) {  // (one past: must hold nothing)
                MergeWord m;
                if (!merge_word(maxbits, (uint32_t)(pos & 63), j, &m)) {
                  continue;
                }
                if (j >= W) {
                  bad++;
                  continue;
                }
                uint64_t bits = 0;
                for (uint32_t i = 0; i < m.cnt; i++)
                  bits |= (uint64_t)get_bit(slot[l], m.x0 + i) << i;
                bits <<= m.shl;
                const uint64_t gw = (pos >> 6) + j;
                covered_bits += m.cnt;
                if ((bits & ~m.mask) != 0)
                  bad++;
                if (m.plain()) {
                  bad += m.mask != ~0ull;
                  plain[gw]++;
                  w[gw] = bits;
                } else {
                  masked[gw] = 1;
                  w[gw] &= ~m.mask;
                  w[gw] |= bits;
                }
              }
            }
            bad += covered_bits != (uint64_t)(b - a + 1) * maxbits;
            for (uint64_t i = 0; i < nwords; i++)
              bad += (plain[i] && masked[i]) || plain[i] > 1;
            bad += w != want;
            g_merge_cases++;
          }
        }
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
  const long mb = merge_mismatches();
  printf("merge mismatches %ld of %ld\n", mb, g_merge_cases);
  return g_bad || mb ? 1 : 0;
}
