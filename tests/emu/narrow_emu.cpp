// Narrow high half of the float32 plane builder (block3.h high_half_narrow,
// planes_from_coeffs_narrow, planes_from_coeffs_auto) on one lane:
//  1. the narrow and the full builder give the same 64 plane words whenever
//     coefficients 32..63 (coding order) lie in [-170, 85]: random blocks, the
//     edges 85 and -170 in single positions, an all-zero high half;
//  2. the test is exact: 86 and -171 in any single position fail it;
//  3. the fixed-rate coder writes the same slot from either builder's planes
//     (the coder has one form: a narrow copy of it cost the kernel its
//     occupancy), and encode_block3_fixed gives the oracle's stream whether the
//     block takes the narrow path (a wave of one narrow lane) or the full one
//     (emu_any_all: some other lane of the wave is wide).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "block3.h"
using namespace zfp_amd;

extern "C" {
typedef struct { uint32_t minbits, maxbits, maxprec; int32_t minexp; } oz_params;
typedef struct { int32_t type, pad_; oz_params p; uint64_t n[4]; int64_t s[4]; uint64_t f[4]; uint64_t e[4]; } oz_job;
uint64_t oz_compress(const oz_job* j, const void* data, uint64_t* words, uint64_t bitpos);
}

static std::vector<uint64_t> arena(8192, 0);
static uint32_t* lut;

// both builders on q: 0 when the 64 plane words agree
static int builders_differ(const int32_t (&q)[64])
{
  uint32_t Pl[32], Ph[32], Nl[32], Nh[32];
  planes_from_coeffs(Pl, Ph, q);
  planes_from_coeffs_narrow(Nl, Nh, q);
  return std::memcmp(Pl, Nl, sizeof Pl) != 0 || std::memcmp(Ph, Nh, sizeof Ph) != 0;
}

// the coder on the narrow builder's planes, on the builder the encoders call
// and on the full builder's planes: 0 when the three slots agree over the budget
static int coders_differ(const int32_t (&q)[64], uint32_t pos, uint32_t lim)
{
  uint32_t Pl[32], Ph[32], Nl[32], Nh[32], Al[32], Ah[32];
  planes_from_coeffs(Pl, Ph, q);
  planes_from_coeffs_narrow(Nl, Nh, q);
  planes_from_coeffs_auto(Al, Ah, q);
  uint64_t* s0 = arena.data() + 1024;
  uint64_t* s1 = arena.data() + 2048;
  uint64_t* s2 = arena.data() + 3072;
  std::fill(s0, s0 + 3 * 1024, 0ull);
  code_planes_fr32(reinterpret_cast<uint32_t*>(s0), 399, lut, pos, lim, Pl, Ph);
  code_planes_fr32(reinterpret_cast<uint32_t*>(s1), 399, lut, pos, lim, Nl, Nh);
  code_planes_fr32(reinterpret_cast<uint32_t*>(s2), 399, lut, pos, lim, Al, Ah);
  int bad = 0;
  for (uint32_t i = 0; i < (lim + 63) / 64; i++) {
    const uint64_t m = (i == lim / 64 && (lim & 63)) ? ((1ull << (lim & 63)) - 1) : ~0ull;
    bad |= ((s0[i] ^ s1[i]) & m) != 0 || ((s0[i] ^ s2[i]) & m) != 0;
  }
  return bad;
}

static void random_block(std::mt19937_64& rng, int32_t (&q)[64], int kind)
{
  for (int i = 0; i < 32; i++) {
    const uint32_t r = (uint32_t)rng();
    q[kPerm3[i]] = kind == 0 ? (int32_t)r : kind == 1 ? (int32_t)(r >> (rng() % 32)) - (int32_t)(rng() % 3) : (int32_t)(r % 1000) - 500;
  }
  for (int i = 32; i < 64; i++) {
    const int span = kind == 2 ? 8 : 256;  // the whole range, or a few bits
    q[kPerm3[i]] = (int32_t)(rng() % span) - (span == 256 ? 170 : 4);
  }
}

static int run_builders(std::mt19937_64& rng)
{
  int bad = 0;
  int32_t q[64];
  // random narrow blocks
  for (int t = 0; t < 20000; t++) {
    random_block(rng, q, t % 3);
    const int b = !high_half_narrow(q) || builders_differ(q);
    if (b && bad++ < 5)
      printf("random narrow block %d: %s\n", t, high_half_narrow(q) ? "planes differ" : "test failed");
    if (t % 10 == 0) {
      const uint32_t pos = 1 + (uint32_t)(rng() % 40), lim = pos + (t % 20 == 0 ? 1015u : 1u + (uint32_t)(rng() % 1500));
      if (coders_differ(q, pos, lim) && bad++ < 5)
        printf("random narrow block %d: coded slots differ (pos %u lim %u)\n", t, pos, lim);
    }
  }
  // all-zero high half (low half zero and random)
  for (int t = 0; t < 100; t++) {
    random_block(rng, q, 0);
    for (int i = 32; i < 64; i++) q[kPerm3[i]] = 0;
    if (t == 0)
      for (int i = 0; i < 32; i++) q[kPerm3[i]] = 0;
    if ((!high_half_narrow(q) || builders_differ(q) || coders_differ(q, 9, 1024)) && bad++ < 5)
      printf("zero high half %d: mismatch\n", t);
  }
  // edges in single positions: first, last, an even and an odd index
  const int where[4] = {32, 63, 40, 47};
  for (int w : where)
    for (int base : {0, 1}) {  // the other high coefficients zero, or random narrow
      for (int val : {85, -170, 86, -171}) {
        random_block(rng, q, 1);
        if (!base)
          for (int i = 32; i < 64; i++) q[kPerm3[i]] = 0;
        q[kPerm3[w]] = val;
        const bool want = val == 85 || val == -170;
        const bool got = high_half_narrow(q);
        if (got != want && bad++ < 20)
          printf("edge %d at coefficient %d: narrow test says %d, expected %d\n", val, w, got, want);
        if (want && (builders_differ(q) || coders_differ(q, 9, 1024)) && bad++ < 20)
          printf("edge %d at coefficient %d: planes or streams differ\n", val, w);
      }
    }
  // wide values anywhere never pass
  for (int t = 0; t < 2000; t++) {
    random_block(rng, q, t % 3);
    const int32_t big = (int32_t)((uint32_t)rng() | 0x100u);
    q[kPerm3[32 + rng() % 32]] = (t & 1) ? 86 + (big & 0x7fffff) : -171 - (big & 0x7fffff);
    if (high_half_narrow(q) && bad++ < 5)
      printf("wide block %d passed the narrow test\n", t);
  }
  printf("builders mismatches %d\n", bad);
  return bad;
}

// the lossy transform's coefficients of a block (what encode_block3_fixed tests)
static bool block_is_narrow(const float (&orig)[64], const CodecParams& cp)
{
  float v[64];
  int32_t q[64];
  uint32_t mp;
  std::memcpy(v, orig, sizeof v);
  lossy_emax_cast(q, v, cp, mp, [&](float (&r)[64]) { std::memcpy(r, orig, sizeof r); });
  xform<3, false, false>(q);
  return high_half_narrow(q);
}

static int run_blocks(std::mt19937_64& rng, const CodecParams& cp, const char* name)
{
  int bad = 0, narrow = 0, wide = 0;
  std::normal_distribution<double> nd(0, 1);
  for (int t = 0; t < 4000; t++) {
    float orig[64];
    // smooth fields with noise of growing size: from every block narrow to none
    const double eps = t % 8 == 0 ? 0.0 : std::pow(10.0, -9.0 + (t % 8));
    const double ph = 0.01 * t, fx = 0.02 + 0.001 * (t % 37), sc = std::pow(10.0, (double)(t % 11) - 5);
    for (int k = 0; k < 4; k++)
      for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++)
          orig[16 * k + 4 * j + i] = (float)(sc * (std::sin(ph + fx * i + 0.7 * fx * j) * std::cos(0.5 * fx * k + ph) + eps * nd(rng)));
    if (t % 97 == 0)
      for (float& x : orig) x = 0.0f;  // the all-zero block ("0" + padding)
    oz_job j{};
    j.type = 3;
    j.p = {cp.minbits, cp.maxbits, cp.maxprec, cp.minexp};
    for (int a = 0; a < 3; a++) j.n[a] = 4, j.f[a] = 0, j.e[a] = 4;
    j.s[0] = 1, j.s[1] = 4, j.s[2] = 16;
    std::vector<uint64_t> ow(64, 0);
    const uint64_t oend = oz_compress(&j, orig, ow.data(), 0);
    const bool nar = block_is_narrow(orig, cp);
    (nar ? narrow : wide)++;
    for (int all : {0, 1}) {  // 0: the block's own path; 1: the full path (another lane is wide)
      emu_any_all = all;
      float v[64];
      std::memcpy(v, orig, sizeof v);
      uint64_t* slot = arena.data() + 1024;
      std::fill(slot, slot + 64, 0ull);
      OrSlot os{slot, 127};
      encode_block3_fixed<true>(os, lut, v, cp, [&](float (&r)[64]) { std::memcpy(r, orig, sizeof r); }, [] {});
      emu_any_all = false;
      bool ok = oend == cp.maxbits;
      for (uint32_t i = 0; ok && i < cp.maxbits / 64; i++)
        ok = slot[i] == ow[i];
      if (!ok && bad++ < 5)
        printf("%s block %d (%s, %s path): stream differs from the oracle\n", name, t, nar ? "narrow" : "wide",
               all ? "full" : "own");
    }
  }
  printf("%s: %d narrow, %d wide blocks, %d bad\n", name, narrow, wide, bad);
  if (narrow < 500 || wide < 500) {
    printf("%s: the blocks do not cover both paths\n", name);
    bad++;
  }
  return bad;
}

int main()
{
  zfp_emu_lds_base = reinterpret_cast<char*>(arena.data());
  lut = reinterpret_cast<uint32_t*>(arena.data()) + 64;  // dbl[256], lead[256]
  for (int b = 0; b < 256; b++) lut[b] = kCoderTables.dbl[b], lut[256 + b] = kCoderTables.lead[b];
  std::mt19937_64 rng(2024);
  int bad = run_builders(rng);
  bad += run_blocks(rng, CodecParams{1024, 1024, 64, -1074}, "rate16");
  bad += run_blocks(rng, CodecParams{512, 512, 64, -1074}, "rate8");
  printf("mismatches %d\n", bad);
  return bad != 0;
}
