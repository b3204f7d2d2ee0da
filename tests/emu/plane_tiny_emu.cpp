// Class T of the fixed-rate f32 coder (codec_dev.h: CoderTables::tiny,
// code_planes_fr32 with PlaneClass::kT; block3.h: the scan of
// planes_from_coeffs_auto<P3, CLS = true>) on waves of 64 emulated lanes.  The
// stub's wave is one lane, so the builder returns each lane's own thresholds;
// the wave's are their maxima, and every lane is coded with them.
//  1. the 80 table entries against code_planes<32, false> run on one plane with
//     n coefficients significant, for every (n, Pl): bits and length;
//  2. crafted waves: the widest of coefficients 4..63 set to every width 0..32
//     by one lane alone (lane 0, 31 or 63), so kT takes every value up to 32
//     and every position relative to the groups 31..29, 28..26, 25..23, 22..20;
//     kT == kS (the width set through coefficients 15..30); coefficients 0..3
//     all topped in plane 31 (n reaches 4 in the first class-T plane); one
//     all-zero block per wave (position pinned at the budget end); thresholds
//     raised by 1..3; budgets of 64, 128, 256 and 1024 bits, the cuts of the
//     64- and 128-bit budgets counted inside and just after the class-T planes
//     (twelve such planes are at most 9 + 11 * 5 = 64 bits from bit 9 on, so only
//     the 64-bit budget can end inside them).  The
//     coder's slot must equal code_planes<32, false> over the budget and
//     nothing is written beyond slot_words_for(lim) words;
//  3. the scan: kT of every lane against bitlen of the OR over nb(c4..63)
//     (crafted: equal; never smaller), on the crafted and on random lanes.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "block3.h"
using namespace zfp_amd;

static std::vector<uint64_t> arena(8192, 0);
static uint32_t* lut;
static const uint32_t K = 0xaaaaaaaau;

static uint32_t blen(uint32_t x) { return x ? 32u - (uint32_t)__builtin_clz(x) : 0u; }

static uint64_t slot_bits_at(const uint64_t* s, uint32_t pos, uint32_t cnt)
{
  uint64_t v = 0;
  for (uint32_t i = 0; i < cnt; i++)
    v |= ((s[(pos + i) >> 6] >> ((pos + i) & 63)) & 1ull) << i;
  return v;
}

// 1. every table entry against the general coder on that one plane
static int run_table()
{
  int bad = 0;
  uint64_t* s = arena.data() + 1024;
  for (uint32_t n = 0; n <= 4; n++)
    for (uint32_t p = 0; p < 16; p++) {
      std::fill(s, s + 64, 0ull);
      uint32_t Pl[32] = {}, Ph[32] = {};
      Pl[0] = p;
      OrSlot os{s, 99};
      const uint32_t pos = 9, end = code_planes<32, false>(os, lut, pos, 1024, 32u, Pl, Ph, 0, n);
      const uint32_t e = kCoderTables.tiny[(4 - n) * 16 + p];
      const uint32_t len = e >> 16, v = e & 0xffffu;
      const uint32_t n1 = std::max(n, blen(p));
      if (len != end - pos || len > 9 || len > 2 * n1 + 1 - n || v != slot_bits_at(s, pos, len) ||
          slot_bits_at(s, pos + len, 40) != 0 || (v >> len) != 0) {
        if (bad++ < 10)
          printf("table entry (n %u, plane %#x): %#x len %u, coder %#llx len %u\n", n, p, v, len,
                 (unsigned long long)slot_bits_at(s, pos, end - pos), end - pos);
      }
    }
  printf("table entries 80 mismatches %d\n", bad);
  return bad;
}

// a coefficient whose negabinary form has at most (exact: exactly) w bits
static int32_t coeff_of_width(std::mt19937_64& rng, uint32_t w, bool exact)
{
  if (w == 0)
    return 0;
  uint32_t u = (uint32_t)rng();
  if (rng() % 4 == 0)
    u &= (uint32_t)rng();
  if (rng() % 16 == 0)
    u = ~0u;
  u = w >= 32 ? u : u & ((1u << w) - 1u);
  if (exact)
    u |= 1u << (w - 1);
  return (int32_t)((u ^ K) - K);
}

struct Lane {
  int32_t q[64];
  uint32_t Pl[32], Ph[32];
  PlaneClass pc;  // the lane's own thresholds (the builder's return)
  uint32_t wantT; // bitlen of the OR over nb(c4..63)
  bool zero;      // an all-zero block: coded with its position at the budget end
};

// planes and thresholds of a lane; 1 when the builder's planes differ from the
// plain builder's or kT is below the width of coefficients 4..63
static int finish(Lane& L, bool exact)
{
  uint32_t Fl[32], Fh[32];
  planes_from_coeffs(Fl, Fh, L.q);
  L.pc = planes_from_coeffs_auto<true, true>(L.Pl, L.Ph, L.q);
  uint32_t o = 0;
  L.zero = true;
  for (int i = 0; i < 64; i++) {
    if (i >= 4)
      o |= ((uint32_t)L.q[kPerm3[i]] + K) ^ K;
    L.zero = L.zero && L.q[i] == 0;
  }
  L.wantT = blen(o);
  int bad = std::memcmp(Fl, L.Pl, sizeof Fl) != 0 || std::memcmp(Fh, L.Ph, sizeof Fh) != 0;
  if (L.pc.ksw != kPlanesTested) {
    const bool ok = exact ? (uint32_t)L.pc.kT == L.wantT : (uint32_t)L.pc.kT >= L.wantT;
    if (!ok || L.pc.kT < L.pc.kS || L.pc.kS <= L.pc.ksw || L.pc.kT > 32) {
      printf("scan: kT %d kS %d ksw %d, coefficients 4..63 are %u wide\n", L.pc.kT, L.pc.kS, L.pc.ksw, L.wantT);
      bad++;
    }
  }
  return bad;
}

static PlaneClass wave_class(const Lane* const* L)
{
  PlaneClass pc{-1, 0, 0};
  for (int l = 0; l < 64; l++) {
    if (L[l]->pc.ksw == kPlanesTested)
      return PlaneClass{kPlanesTested, 32, 32};
    pc.ksw = std::max(pc.ksw, L[l]->pc.ksw);
    pc.kS = std::max(pc.kS, L[l]->pc.kS);
    pc.kT = std::max(pc.kT, L[l]->pc.kT);
  }
  return pc;
}

// planes the class coder takes from the table under threshold kT (whole groups)
static int tiny_lowest(const PlaneClass& pc)
{
  int low = 32;
  for (int hi = 31; hi >= kTinyLowest + 2; hi -= 3)
    if (pc.ksw < hi && hi - 2 >= pc.kT)
      low = hi - 2;
    else
      break;
  return low;
}

static const uint32_t kBudgets[4] = {64, 128, 256, 1024};
static long t_planes = 0, t_cut_in = 0, t_cut_after = 0, zero_blocks = 0, n4_first = 0;

// one lane with the wave's classes against code_planes<32, false> over the
// budget; nothing is written beyond the slot
static int coders_differ(const Lane& L, const PlaneClass& pc, uint32_t lim)
{
  const uint32_t words = slot_words_for(lim), guard = 8;
  const uint32_t pos = L.zero ? lim : 9u;  // (encode_block3_fixed: e ? 1 + kE : maxbits)
  uint64_t* s0 = arena.data() + 1024;
  uint64_t* s2 = arena.data() + 3072;
  std::fill(s0, s0 + 3 * 1024, 0ull);
  const uint32_t jmax = 2 * words - 1;
  code_planes_fr32(reinterpret_cast<uint32_t*>(s0), jmax, lut, pos, lim, L.Pl, L.Ph, pc);
  OrSlot os{s2, 399};
  code_planes<32, false>(os, lut, pos, lim, 32u, L.Pl, L.Ph);
  int bad = 0;
  for (uint32_t i = 0; i < (lim + 63) / 64; i++) {
    const uint64_t m = (i == lim / 64 && (lim & 63)) ? ((1ull << (lim & 63)) - 1) : ~0ull;
    bad |= ((s0[i] ^ s2[i]) & m) != 0;
    if (L.zero)
      bad |= (s0[i] & m) != 0;
  }
  for (uint32_t i = words; i < words + guard; i++)
    bad |= s0[i] != 0;
  return bad;
}

// where the budget [9, lim) of this lane ends relative to the class-T planes:
// 1 inside one of them, 2 inside the plane after the last of them
static int cut_at(const Lane& L, const PlaneClass& pc, uint32_t lim)
{
  const int low = tiny_lowest(pc);
  uint32_t n = 0, pos = 9;
  for (int k = 31; k >= 0 && k >= low - 1; k--) {
    const uint32_t xs = L.Pl[k] >> n;
    const uint32_t end = pos + n + blen(xs) + (uint32_t)__builtin_popcount(xs) + 1u;
    if (pos < lim && end > lim)
      return k >= low ? 1 : 2;
    pos = end;
    n += blen(xs);
  }
  return 0;
}

static int code_wave(const Lane* const* L, const PlaneClass& pc, bool raise)
{
  int bad = 0;
  if (pc.ksw == kPlanesTested)
    return 0;
  for (int l = 0; l < 64; l++)
    for (int bi = 0; bi < 4; bi++) {
      const uint32_t b = kBudgets[bi];
      bad += coders_differ(*L[l], pc, b);
      if (b <= 128 && !L[l]->zero) {
        const int c = cut_at(*L[l], pc, b);
        t_cut_in += c == 1;
        t_cut_after += c == 2;
      }
      if (raise)
        for (int r = 1; r <= 3; r++)
          bad += coders_differ(*L[l], PlaneClass{pc.ksw, pc.kS, std::min(32, pc.kT + r)}, b);
      // without class T: the same words
      bad += coders_differ(*L[l], PlaneClass{pc.ksw, pc.kS, 32}, b);
    }
  t_planes += 32 - tiny_lowest(pc);
  for (int l = 0; l < 64; l++) {
    zero_blocks += L[l]->zero;
    n4_first += tiny_lowest(pc) <= 29 && L[l]->Pl[31] == 0xfu;
  }
  return bad;
}

// widths: coefficients 0..3, 4..14, 15..30, 31 and 32..63 (coding order); `ex`
// bit j: group j has one coefficient of exactly that width (bit 0: all of 0..3;
// bit 5: all of 4..14, a long first plane after class T)
static void craft(std::mt19937_64& rng, Lane& L, uint32_t w0, uint32_t w4, uint32_t w15, uint32_t w31, uint32_t wh,
                  uint32_t ex)
{
  const int e4 = 4 + (int)(rng() % 11), e15 = 15 + (int)(rng() % 16), eh = 32 + (int)(rng() % 32);
  for (int i = 0; i < 64; i++) {
    const uint32_t w = i < 4 ? w0 : i < 15 ? w4 : i < 31 ? w15 : i == 31 ? w31 : wh;
    const bool x = (i < 4 && (ex & 1)) || (i == e4 && (ex & 2)) || (i >= 4 && i < 15 && (ex & 32)) || (i == e15 && (ex & 4)) || (i == 31 && (ex & 8)) ||
                   (i == eh && (ex & 16));
    L.q[kPerm3[i]] = coeff_of_width(rng, x ? w : (uint32_t)(rng() % (w + 1)), x);
  }
}

static int run_crafted(std::mt19937_64& rng)
{
  int bad = 0, waves = 0;
  bool seenT[33] = {}, seenEq[33] = {};
  std::vector<Lane> lanes(64);
  const Lane* L[64];
  for (int l = 0; l < 64; l++) L[l] = &lanes[l];
  const int whos[3] = {0, 31, 63};
  for (int rep = 0; rep < 6; rep++)
    for (int kT = 0; kT <= 32; kT++)
      for (int via = 0; via < 3; via++) {
        // via 0: coefficients 4..14 are kT wide (kS below); 1: coefficients 15..30
        // are (kT == kS); 2: coefficient 31 is
        const int who = whos[waves % 3];
        const uint32_t w0 = (rep & 1) ? 32u : (uint32_t)std::min(32, kT + (int)(rng() % 12));
        const uint32_t hi8 = (uint32_t)std::min(kT, 8);
        for (int l = 0; l < 64; l++) {
          Lane& X = lanes[l];
          const bool me = l == who || (rep >= 4 && via == 0);  // (rep 4, 5: every lane sets it)
          const uint32_t low = kT ? (uint32_t)(rng() % kT) : 0u;  // the others stay below
          const uint32_t wl = me ? (uint32_t)kT : low;
          const uint32_t wS = (uint32_t)(rng() % (wl + 1));
          if (l == (who + 7) % 64 && rep >= 2) {
            std::memset(X.q, 0, sizeof X.q);  // an all-zero block
          } else if (via == 0) {
            craft(rng, X, w0, wl, wS, (uint32_t)(rng() % (wS + 1)), std::min(wS, hi8), (rep & 1) | (me ? 2u : 0u) | (me && rep >= 4 ? 32u : 0u));
          } else if (via == 1) {
            craft(rng, X, w0, (uint32_t)(rng() % (wl + 1)), wl, (uint32_t)(rng() % (wl + 1)), std::min(wl, hi8),
                  (rep & 1) | (me ? 4u : 0u));
          } else {
            craft(rng, X, w0, wS, wS, wl, std::min(wS, hi8), (rep & 1) | (me ? 8u : 0u));
          }
          bad += finish(X, true);
        }
        const PlaneClass pc = wave_class(L);
        if (pc.ksw == kPlanesTested || pc.kT != kT) {
          if (bad++ < 10)
            printf("crafted wave via %d lane %d: kT %d (ksw %d), expected %d\n", via, who, pc.kT, pc.ksw, kT);
        } else {
          seenT[kT] = true;
          if (pc.kT == pc.kS)
            seenEq[kT] = true;
        }
        bad += code_wave(L, pc, waves % 3 == 0);
        waves++;
      }
  for (int i = 0; i <= 32; i++)
    if (!seenT[i] || (i >= 1 && !seenEq[i])) {
      printf("crafted waves do not cover kT = %d (or kT == kS there)\n", i);
      bad++;
    }
  printf("crafted waves %d mismatches %d\n", waves, bad);
  return bad;
}

// random lanes from smooth to dense: the scan never gives a threshold below the
// width of coefficients 4..63, and the coder agrees
static int run_random(std::mt19937_64& rng)
{
  int bad = 0;
  std::vector<Lane> lanes(64);
  const Lane* L[64];
  for (int l = 0; l < 64; l++) L[l] = &lanes[l];
  long classed = 0;
  for (int t = 0; t < 300; t++) {
    const int decay = 4 + t % 5;
    const uint32_t top = 24u + (uint32_t)(rng() % 9);
    for (int l = 0; l < 64; l++) {
      for (int i = 0; i < 64; i++) {
        const int lg = (int)blen((uint32_t)i + 1u);
        int w = (int)top - (decay * lg * (int)(8 + rng() % 5)) / 10 + (int)(rng() % 3) - 1;
        w = std::max(0, std::min(32, w));
        lanes[l].q[kPerm3[i]] = coeff_of_width(rng, (uint32_t)w, false);
      }
      bad += finish(lanes[l], false);
    }
    const PlaneClass pc = wave_class(L);
    classed += pc.ksw != kPlanesTested;
    bad += code_wave(L, pc, t % 10 == 0);
  }
  printf("random waves 300 (%ld with classes) mismatches %d\n", classed, bad);
  if (classed < 100) {
    printf("random waves do not reach the class coder\n");
    bad++;
  }
  return bad;
}

int main()
{
  zfp_emu_lds_base = reinterpret_cast<char*>(arena.data());
  lut = reinterpret_cast<uint32_t*>(arena.data()) + 64;  // dbl[256], lead[256], tiny[80]
  for (int b = 0; b < 256; b++) lut[b] = kCoderTables.dbl[b], lut[256 + b] = kCoderTables.lead[b];
  for (int b = 0; b < kTinyEntries; b++) lut[512 + b] = kCoderTables.tiny[b];
  std::mt19937_64 rng(4711);
  int bad = run_table();
  bad += run_crafted(rng);
  bad += run_random(rng);
  printf("class-T planes coded %ld; 64/128-bit budgets cut inside them in %ld lanes, just after them in %ld; "
         "all-zero blocks %ld; lanes with n = 4 after plane 31 in a class-T group %ld\n",
         t_planes, t_cut_in, t_cut_after, zero_blocks, n4_first);
  if (t_planes < 1000 || t_cut_in < 100 || t_cut_after < 100 || zero_blocks < 100 || n4_first < 100) {
    printf("the waves do not cover the class-T cases\n");
    bad++;
  }
  printf("mismatches %d\n", bad);
  return bad != 0;
}
