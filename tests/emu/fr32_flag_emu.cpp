// The fixed-rate f32 coder (codec_dev.h code_planes_fr32) on the planes a
// narrow wave hands it, and its first plane, on one lane.  (Written for a
// wave-uniform "narrow" flag as a trailing parameter of the coder; the flag
// measured slower on the GPU and was not kept, DESIGN 4.2, so the coder has its
// seven arguments and the flagged call is not here.  What the flag must not
// have changed is what the coder must still do.)
//  1. planes whose high half is zero from plane 8 up (what the narrow builder
//     makes): the coder writes the same slot words over the budget as
//     code_planes<32, false>.  Random and adversarial low halves: 0xffff
//     units, tops past bit 15, n reaching 32 inside planes 31..8 (the only way
//     such a wave leaves the 32-bit form there), empty planes, plane 31 zero
//     and non-zero (its verbatim write is not issued: n == 0), budgets cut
//     anywhere;
//  2. planes with something in the high half of a plane >= 8: the same.
// Both with the wave-level branches as a lone lane takes them and with every
// one entered (emu_any_all: some other lane needs it).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "codec_dev.h"
using namespace zfp_amd;

static std::vector<uint64_t> arena(8192, 0);
static uint32_t* lut;

static uint32_t bitlen32(uint32_t x) { return x ? 32u - (uint32_t)__builtin_clz(x) : 0u; }

// low half of plane k of a block of the given kind
static uint32_t low_plane(std::mt19937_64& rng, int kind, int k)
{
  const uint64_t r = rng();
  switch (kind) {
    case 0: return (uint32_t)r;                                                            // dense
    case 1: return (rng() % 3 == 0) ? (uint32_t)(r & rng()) : 0u;                          // sparse, empty planes
    case 2: return (rng() % 4 == 0) ? (uint32_t)(0xffffull << (rng() % 17)) : (uint32_t)(r & 0xffff);  // 0xffff units
    case 3: return (rng() % 5 == 0) ? 0x80000000u : (uint32_t)(r & 0xff);                  // n jumps to 32
    case 4: return (k % 7 == 0) ? 0xffffffffu : 0u;
    case 5: return (uint32_t)r >> (rng() % 32);
    case 6: return (k > 24) ? 1u << (rng() % 32) : (uint32_t)(r & (r >> 5));
    case 7: return (rng() % 2) ? 0xffff0000u | (uint32_t)(r & 0xffff) : (uint32_t)(r & 0xffff) << 16;  // tops past bit 15
    case 8: return (k == 8 + (int)(r % 24)) ? 0xc0000000u : (uint32_t)(r & 0x3f);          // n reaches 32 in one plane >= 8
    default: return (k > 15) ? (uint32_t)(r & 0xffff) : (uint32_t)r;                       // n stays below 32 down to plane 15
  }
}

// 0 when the slots agree over bits [0, lim)
static int slots_differ(const uint64_t* a, const uint64_t* b, uint32_t lim)
{
  for (uint32_t i = 0; i < (lim + 63) / 64; i++) {
    const uint64_t m = (i == lim / 64 && (lim & 63)) ? ((1ull << (lim & 63)) - 1) : ~0ull;
    if ((a[i] ^ b[i]) & m)
      return 1;
  }
  return 0;
}

// code_planes_fr32 against code_planes<32, false> on one set of planes
static int coders_differ(const uint32_t (&Pl)[32], const uint32_t (&Ph)[32], uint32_t pos, uint32_t lim)
{
  uint64_t* s0 = arena.data() + 1024;
  uint64_t* s1 = arena.data() + 2048;
  std::fill(s0, s0 + 2 * 1024, 0ull);
  code_planes_fr32(reinterpret_cast<uint32_t*>(s0), 399, lut, pos, lim, Pl, Ph);
  OrSlot os{s1, 399};
  code_planes<32, false>(os, lut, pos, lim, 32u, Pl, Ph);
  return slots_differ(s0, s1, lim);
}

static int run_narrow(std::mt19937_64& rng, int trials)
{
  int bad = 0, n32 = 0, top0 = 0, top1 = 0;
  for (int t = 0; t < trials; t++) {
    const int kind = t % 10;
    uint32_t Pl[32], Ph[32];
    for (int k = 0; k < 32; k++) {
      Pl[k] = low_plane(rng, kind, k);
      // the narrow builder's high half: planes 0..7 only (dense, sparse or empty)
      Ph[k] = k >= 8 ? 0u : (t & 16) ? 0u : (t & 32) ? (uint32_t)(rng() & rng()) : (uint32_t)rng();
    }
    if (t % 3 == 0)
      Pl[31] = 0;
    else if (t % 3 == 1)
      Pl[31] |= 1u << (rng() % 32);
    (Pl[31] ? top1 : top0)++;
    uint32_t n = 0;
    for (int k = 31; k >= 8; k--)
      n = std::max(n, bitlen32(Pl[k]));
    n32 += n == 32;
    const uint32_t pos = 1 + (uint32_t)(rng() % 40);
    const uint32_t budgets[3] = {4096, 64 + (uint32_t)(rng() % 1500), 1 + (uint32_t)(rng() % 300)};
    for (uint32_t b : budgets)
      if (coders_differ(Pl, Ph, pos, pos + b) && bad++ < 5)
        printf("narrow trial %d kind %d budget %u: slots differ\n", t, kind, b);
  }
  if (n32 < trials / 20 || top0 < trials / 4 || top1 < trials / 4) {
    printf("narrow sets do not cover the cases (n reaches 32 above plane 8: %d, plane 31 zero %d, non-zero %d)\n", n32,
           top0, top1);
    bad++;
  }
  printf("narrow planes mismatches %d (n reaches 32 in planes 31..8: %d of %d sets)\n", bad, n32, trials);
  return bad;
}

static int run_wide(std::mt19937_64& rng, int trials)
{
  int bad = 0;
  for (int t = 0; t < trials; t++) {
    const int kind = t % 10;
    uint32_t Pl[32], Ph[32];
    for (int k = 0; k < 32; k++) {
      Pl[k] = low_plane(rng, kind, k);
      Ph[k] = (t & 16) ? 0u : (uint32_t)(rng() & rng());
    }
    // something in the high half of a plane >= 8: one bit, or a dense word
    const int kw = 8 + (int)(rng() % 24);
    Ph[kw] |= (t & 1) ? 1u << (rng() % 32) : (uint32_t)rng() | 1u;
    if (t % 3 == 0)
      Pl[31] = 0;
    const uint32_t pos = 1 + (uint32_t)(rng() % 40);
    const uint32_t budgets[3] = {4096, 64 + (uint32_t)(rng() % 1500), 1 + (uint32_t)(rng() % 300)};
    for (uint32_t b : budgets)
      if (coders_differ(Pl, Ph, pos, pos + b) && bad++ < 5)
        printf("wide trial %d kind %d plane %d budget %u: slots differ\n", t, kind, kw, b);
  }
  printf("wide planes mismatches %d\n", bad);
  return bad;
}

int main()
{
  zfp_emu_lds_base = reinterpret_cast<char*>(arena.data());
  lut = reinterpret_cast<uint32_t*>(arena.data()) + 64;  // dbl[256], lead[256]
  for (int b = 0; b < 256; b++) lut[b] = kCoderTables.dbl[b], lut[256 + b] = kCoderTables.lead[b];
  std::mt19937_64 rng(31008);
  int bad = 0;
  for (int all : {0, 1}) {
    emu_any_all = all;
    bad += run_narrow(rng, 20000);
    bad += run_wide(rng, 10000);
  }
  emu_any_all = false;
  printf("mismatches %d\n", bad);
  return bad != 0;
}
