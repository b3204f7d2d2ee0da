// Plane classes of the fixed-rate f32 coder (block3.h planes_from_coeffs_auto
// <P3, CLS = true>, codec_dev.h code_planes_fr32 with a PlaneClass) on waves of
// 64 emulated lanes.  The stub's wave is one lane, so the builder returns each
// lane's own thresholds; the wave's are their maxima (bitlen of an OR is the
// largest bitlen; one wide lane makes the wave wide), and every lane is then
// coded with them.
//  1. crafted waves: kS at every value 0..32 and ksw at every value -1..31, each
//     set by one lane alone (lane 0, 31 or 63), through the high half, through
//     coefficient 31, and (ksw above 7) on the planes of wide waves, which the
//     builder leaves without classes (kPlanesTested: the coder that tests every
//     plane) and which are also coded with the thresholds their planes have;
//     the thresholds must be exactly the targets, and the coder's slot must equal code_planes<32, false> over the
//     budget, and so must the seven-argument code_planes_fr32; nothing is
//     written beyond slot_words_for(lim) words;
//  2. a lane with n' = 15 and xs = 0x7fff at n = 0 (31 bits in one write), in
//     plane 31 and below it (plane 31 zero);
//  3. thresholds raised by 1..3 give the same words;
//  4. budgets of 64, 128, 256 and 1024 bits: cuts inside class-S planes (counted:
//     at least 1000 lanes for each of the three short budgets);
//  5. 10^5 random waves drawn from lanes whose width profiles range from smooth
//     to dense: every plane classed S or M meets that body's preconditions in
//     every lane, checked on the planes themselves (S: no high bits, n' <= 15
//     so xs <= 0x7fff, verbatim and group bits within 31; M: no high bits,
//     n <= 31).
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
  PlaneClass pc;       // the lane's own thresholds (the builder's return)
  uint32_t sOK, mOK;   // planes that meet the class-S / class-M body's preconditions
};

// widths: coefficients 0..14, 15..30, 31 and 32..63 (coding order); `ex` bit j:
// group j has one coefficient of exactly that width
static void craft(std::mt19937_64& rng, Lane& L, uint32_t w0, uint32_t w15, uint32_t w31, uint32_t wh, uint32_t ex)
{
  const int e0 = (int)(rng() % 15), e15 = 15 + (int)(rng() % 16), eh = (rng() % 3 == 0) ? 63 : 32 + (int)(rng() % 32);
  for (int i = 0; i < 64; i++) {
    const uint32_t w = i < 15 ? w0 : i < 31 ? w15 : i == 31 ? w31 : wh;
    const bool x = (i == e0 && (ex & 1)) || (i == e15 && (ex & 2)) || (i == 31 && (ex & 4)) || (i == eh && (ex & 8));
    L.q[kPerm3[i]] = coeff_of_width(rng, x ? w : (uint32_t)(rng() % (w + 1)), x);
  }
}

// width profile from smooth (decay 7) to dense (decay 0)
static void random_lane(std::mt19937_64& rng, Lane& L, int decay, uint32_t top)
{
  for (int i = 0; i < 64; i++) {
    const int lg = (int)blen((uint32_t)i + 1u);
    int w = (int)top - (decay * lg * (int)(8 + rng() % 5)) / 10 + (int)(rng() % 3) - 1;
    w = std::max(0, std::min(32, w));
    L.q[kPerm3[i]] = coeff_of_width(rng, (uint32_t)w, false);
  }
}

// planes, thresholds and per-plane facts of a lane; 1 when the builder's planes
// differ from the plain builder's
static int finish(Lane& L)
{
  uint32_t Fl[32], Fh[32];
  planes_from_coeffs(Fl, Fh, L.q);
  L.pc = planes_from_coeffs_auto<true, true>(L.Pl, L.Ph, L.q);
  L.sOK = L.mOK = 0;
  uint32_t n = 0;
  for (int k = 31; k >= 0; k--) {
    const uint32_t pl = L.Pl[k];
    const bool m = L.Ph[k] == 0 && n <= 31;
    if (m) {
      const uint32_t xs = pl >> n;
      const uint32_t bits = n + blen(xs) + (uint32_t)__builtin_popcount(xs) + 1u;
      L.mOK |= 1u << k;
      if (xs <= 0x7fffu && bits <= 31u)
        L.sOK |= 1u << k;
    }
    n = std::max(n, std::max(blen(pl), L.Ph[k] ? 32u + blen(L.Ph[k]) : 0u));
  }
  return std::memcmp(Fl, L.Pl, sizeof Fl) != 0 || std::memcmp(Fh, L.Ph, sizeof Fh) != 0;
}

static PlaneClass wave_class(const Lane* const* L)
{
  PlaneClass pc{-1, 0};
  for (int l = 0; l < 64; l++) {
    // one wide lane makes the wave wide: no classes, the coder that tests every plane
    if (L[l]->pc.ksw == kPlanesTested)
      return PlaneClass{kPlanesTested, 32};
    pc.ksw = std::max(pc.ksw, L[l]->pc.ksw);
    pc.kS = std::max(pc.kS, L[l]->pc.kS);
  }
  return pc;
}

// planes of class S (k >= kS) and M (kS > k > ksw) as masks
static uint32_t mask_from(int k) { return k >= 32 ? 0u : k <= 0 ? ~0u : ~0u << k; }

// 0 when every lane's S and M planes meet their body's preconditions
static int class_violations(const Lane* const* L, const PlaneClass& pc)
{
  if (pc.ksw == kPlanesTested)
    return 0;
  if (pc.kS <= pc.ksw)
    return 1;
  const uint32_t s = mask_from(pc.kS), m = mask_from(pc.ksw + 1) & ~s;
  int bad = 0;
  for (int l = 0; l < 64; l++)
    bad += (s & ~L[l]->sOK) != 0 || (m & ~L[l]->mOK) != 0;
  return bad;
}

static long s_planes = 0, m_planes = 0, w_planes = 0;

// one lane with the wave's classes against code_planes<32, false> and the coder
// without classes, over the budget; nothing is written beyond the slot
static int coders_differ(const Lane& L, const PlaneClass& pc, uint32_t pos, uint32_t lim)
{
  const uint32_t words = slot_words_for(lim), guard = 8;
  uint64_t* s0 = arena.data() + 1024;
  uint64_t* s1 = arena.data() + 2048;
  uint64_t* s2 = arena.data() + 3072;
  std::fill(s0, s0 + 3 * 1024, 0ull);
  const uint32_t jmax = 2 * words - 1;
  if (pc.ksw != kPlanesTested)  // (as encode_block3_fixed chooses)
    code_planes_fr32(reinterpret_cast<uint32_t*>(s0), jmax, lut, pos, lim, L.Pl, L.Ph, pc);
  else
    code_planes_fr32(reinterpret_cast<uint32_t*>(s0), jmax, lut, pos, lim, L.Pl, L.Ph);
  code_planes_fr32(reinterpret_cast<uint32_t*>(s1), jmax, lut, pos, lim, L.Pl, L.Ph);
  OrSlot os{s2, 399};
  code_planes<32, false>(os, lut, pos, lim, 32u, L.Pl, L.Ph);
  int bad = 0;
  for (uint32_t i = 0; i < (lim + 63) / 64; i++) {
    const uint64_t m = (i == lim / 64 && (lim & 63)) ? ((1ull << (lim & 63)) - 1) : ~0ull;
    bad |= ((s0[i] ^ s2[i]) & m) != 0 || ((s0[i] ^ s1[i]) & m) != 0;
  }
  // (the spare words may differ: a lone lane leaves the plane loop once its own
  // budget is spent, at another plane under another threshold)
  for (uint32_t i = words; i < words + guard; i++)
    bad |= s0[i] != 0;
  return bad;
}

static const uint32_t kBudgets[4] = {64, 128, 256, 1024};
static long s_cuts[4] = {0, 0, 0, 0};  // lanes whose budget ended inside a class-S plane, per budget

// the budget [pos, lim) of this lane ends inside a plane of class S
static bool cut_in_class_s(const Lane& L, const PlaneClass& pc, uint32_t pos, uint32_t lim)
{
  uint32_t n = 0;
  for (int k = 31; k >= pc.kS && pc.ksw != kPlanesTested; k--) {
    const uint32_t xs = L.Pl[k] >> n;
    const uint32_t end = pos + n + blen(xs) + (uint32_t)__builtin_popcount(xs) + 1u;
    if (pos < lim && end > lim)
      return true;
    pos = end;
    n += blen(xs);
  }
  return false;
}

// every lane of the wave with the wave's classes, all budgets; `raise`: also
// with the thresholds raised by 1..3
static int code_wave(const Lane* const* L, const PlaneClass& pc, bool raise)
{
  int bad = 0;
  for (int l = 0; l < 64; l++)
    for (int bi = 0; bi < 4; bi++) {
      const uint32_t b = kBudgets[bi];
      bad += coders_differ(*L[l], pc, 9, b);
      s_cuts[bi] += cut_in_class_s(*L[l], pc, 9, b);
      if (raise && pc.ksw != kPlanesTested)
        for (int r = 1; r <= 3; r++) {
          const int s = std::min(32, pc.kS + r), w = std::min(31, pc.ksw + r);
          bad += coders_differ(*L[l], PlaneClass{pc.ksw, s}, 9, b);
          if (w < s)
            bad += coders_differ(*L[l], PlaneClass{w, s}, 9, b);
          if (w < pc.kS)
            bad += coders_differ(*L[l], PlaneClass{w, pc.kS}, 9, b);
        }
    }
  if (pc.ksw != kPlanesTested) {
    s_planes += 32 - pc.kS;
    m_planes += pc.kS - pc.ksw - 1;
    w_planes += pc.ksw + 1;
  }
  return bad;
}

// crafted waves: the thresholds (ksw, kS) set by lane `who` alone
static int run_crafted(std::mt19937_64& rng)
{
  int bad = 0, waves = 0;
  bool seenS[33] = {}, seenW[33] = {};
  std::vector<Lane> lanes(64);
  const Lane* L[64];
  for (int l = 0; l < 64; l++) L[l] = &lanes[l];
  const int whos[3] = {0, 31, 63};
  for (int kS = 0; kS <= 32; kS++)
    for (int ksw = -1; ksw < kS && ksw <= 31; ksw++)
      for (int via = 0; via < 3; via++) {
        // via 0: the high half is ksw + 1 wide (narrow: at most 8); 1: coefficient
        // 31 is ksw + 2 wide; 2: a wide wave (the high half more than 8 wide, kS = 32)
        if ((via == 0 && ksw > 7) || (via == 1 && (ksw + 2 > kS || ksw < 0)) || (via == 2 && (kS != 32 || ksw < 8)))
          continue;
        const int who = whos[waves % 3];
        const uint32_t wS = (uint32_t)kS;
        for (int l = 0; l < 64; l++) {
          Lane& X = lanes[l];
          const bool me = l == who;
          // the other lanes stay below both thresholds
          const uint32_t wh = via == 1 ? (uint32_t)std::min(8, std::max(0, ksw)) : (uint32_t)(ksw + 1);
          const uint32_t w31 = via == 1 ? (uint32_t)(ksw + 2) : (uint32_t)std::min(kS, ksw + 1);
          const uint32_t w0 = waves % 2 ? 32u : (uint32_t)(rng() % 33);
          if (via == 2) {
            // wide: lane `who` has the widest high half; coefficient 31 may come first
            craft(rng, X, w0, 32, (uint32_t)std::min(32, ksw + 1), me ? wh : (uint32_t)(rng() % wh), me ? 8u : 0u);
          } else if (me) {
            craft(rng, X, w0, wS, w31, wh, 2u | (via == 1 ? 4u : 8u));
          } else {
            craft(rng, X, w0, wS ? (uint32_t)(rng() % wS) : 0u, w31 ? (uint32_t)(rng() % w31) : 0u,
                  wh ? (uint32_t)(rng() % wh) : 0u, 0u);
          }
          bad += finish(X);
        }
        const PlaneClass pc = wave_class(L);
        // exact: the crafted widths are the thresholds' definitions
        // (a wide wave has no classes; the classes it would have are run below)
        const int wantS = kS, wantW = via == 2 ? kPlanesTested : ksw;
        if (pc.kS != wantS || pc.ksw != wantW) {
          if (bad++ < 10)
            printf("crafted wave via %d lane %d: thresholds (%d, %d), expected (%d, %d)\n", via, who, pc.ksw, pc.kS,
                   wantW, wantS);
        }
        bad += class_violations(L, pc);
        bad += code_wave(L, pc, waves % 4 == 0);
        if (via == 2) {
          // the coder with the thresholds such a wave's planes have: kS = 32, ksw up to 31
          const PlaneClass wide{ksw, 32};
          bad += class_violations(L, wide);
          bad += code_wave(L, wide, waves % 4 == 0);
          seenS[32] = true;
          seenW[ksw + 1] = true;
        } else {
          seenS[pc.kS] = true;
          seenW[pc.ksw + 1] = true;
        }
        waves++;
      }
  for (int i = 0; i <= 32; i++)
    if (!seenS[i] || !seenW[i]) {
      printf("crafted waves do not cover kS = %d or ksw = %d\n", i, i - 1);
      bad++;
    }
  printf("crafted waves %d mismatches %d\n", waves, bad);
  return bad;
}

// a lane with coefficients 0..14 all topped in one plane and nothing else up
// there: n' = 15, xs = 0x7fff at n = 0, 31 bits in one class-S write
static int run_full15(std::mt19937_64& rng)
{
  int bad = 0, hit = 0;
  std::vector<Lane> lanes(64);
  const Lane* L[64];
  for (int l = 0; l < 64; l++) L[l] = &lanes[l];
  for (int top = 32; top >= 2; top -= (top > 28 ? 1 : 5)) {
    for (int l = 0; l < 64; l++) {
      Lane& X = lanes[l];
      const uint32_t w15 = (uint32_t)(rng() % top), w31 = (uint32_t)(rng() % top);
      craft(rng, X, (uint32_t)top, w15, w31, (uint32_t)(rng() % std::min(top, 9)), 0u);
      if (l % 7 == 0)
        for (int i = 0; i < 15; i++)
          X.q[kPerm3[i]] = coeff_of_width(rng, (uint32_t)top, true);
      bad += finish(X);
      if (l % 7 == 0) {
        uint32_t above = 0;
        for (int k = top; k < 32; k++) above |= X.Pl[k] | X.Ph[k];
        // n = 0, xs = 0x7fff: 15 + 15 + 1 = 31 bits
        if (above != 0 || X.Pl[top - 1] != 0x7fffu || X.Ph[top - 1] != 0 || !((X.sOK >> (top - 1)) & 1u)) {
          printf("full-15 lane: plane %d is %#x\n", top - 1, X.Pl[top - 1]);
          bad++;
        }
        hit++;
      }
    }
    const PlaneClass pc = wave_class(L);
    if (pc.kS > top - 1) {
      printf("full-15 wave: plane %d is not class S (kS %d)\n", top - 1, pc.kS);
      bad++;
    }
    bad += class_violations(L, pc);
    bad += code_wave(L, pc, true);
  }
  printf("full-15 lanes %d mismatches %d\n", hit, bad);
  return bad;
}

// 10^5 random waves out of a pool of lanes; some are coded
static int run_random(std::mt19937_64& rng)
{
  const int kPool = 8192, kProfiles = 8, kPer = kPool / kProfiles;
  int bad = 0, coded = 0;
  std::vector<Lane> pool(kPool);
  for (int i = 0; i < kPool; i++) {
    const int decay = 7 - i / kPer;  // profile 0 smooth .. 7 dense
    random_lane(rng, pool[i], decay, 18u + (uint32_t)(rng() % 15));
    bad += finish(pool[i]);
  }
  long viol = 0, hist[3] = {0, 0, 0}, tested = 0;
  for (int t = 0; t < 100000; t++) {
    const Lane* L[64];
    const int prof = t % kProfiles;
    for (int l = 0; l < 64; l++) {
      // a wave of one profile, sometimes with a lane or two of a rougher one
      const int p = (rng() % 40 == 0) ? (int)(rng() % kProfiles) : prof;
      L[l] = &pool[p * kPer + (int)(rng() % kPer)];
    }
    const PlaneClass pc = wave_class(L);
    viol += class_violations(L, pc);
    if (pc.ksw == kPlanesTested) {
      tested++;
    } else {
      hist[0] += 32 - pc.kS;
      hist[1] += pc.kS - pc.ksw - 1;
      hist[2] += pc.ksw + 1;
    }
    if (t % 400 == 0) {
      bad += code_wave(L, pc, false);
      coded++;
    }
  }
  bad += viol != 0;
  printf("random waves 100000 precondition violations %ld (planes S %ld M %ld wide %ld; %ld waves without classes), "
         "coded %d, mismatches %d\n", viol, hist[0], hist[1], hist[2], tested, coded, bad);
  if (hist[0] < 30000 || hist[1] < 30000 || hist[2] < 30000 || tested < 10000) {
    printf("random waves do not cover the three classes\n");
    bad++;
  }
  return bad;
}

int main()
{
  zfp_emu_lds_base = reinterpret_cast<char*>(arena.data());
  lut = reinterpret_cast<uint32_t*>(arena.data()) + 64;  // dbl[256], lead[256]
  for (int b = 0; b < 256; b++) lut[b] = kCoderTables.dbl[b], lut[256 + b] = kCoderTables.lead[b];
  std::mt19937_64 rng(90210);
  int bad = run_crafted(rng);
  bad += run_full15(rng);
  bad += run_random(rng);
  printf("coded planes: S %ld M %ld wide %ld\n", s_planes, m_planes, w_planes);
  printf("budget cuts inside a class-S plane: %ld %ld %ld %ld lanes (64, 128, 256, 1024 bits)\n", s_cuts[0], s_cuts[1],
         s_cuts[2], s_cuts[3]);
  for (int bi = 0; bi < 3; bi++)
    if (s_cuts[bi] < 1000) {
      printf("the budgets do not cut inside class-S planes\n");
      bad++;
    }
  printf("mismatches %d\n", bad);
  return bad != 0;
}
