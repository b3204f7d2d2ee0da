/* Experiment (not product, not test): how the C2 field's blocks (1024^3 f32
 * F1, rate 16: 1024 bits per block) are decoded by decode_planes32 -- planes
 * per block, and per wave of 64 blocks along x how many planes run in the
 * 32-bit body before some lane has more than 31 significant coefficients (the
 * switch to decode_plane64 for the rest of the block), and how often a
 * section reaches past the 31-bit window.  Oracle restatement of the cast,
 * transform and order.
 * `c2stats classes [zstep]`: the encoder's plane classes (code_planes_fr32 with
 * a PlaneClass, codec_dev.h) on every wave of the field (every zstep-th layer
 * of blocks): per plane the share of waves in class S, M and the wide form,
 * the spread of the thresholds, kT included (class T: the planes of
 * coefficients 0..3 from one table), and the class-T planes a wave codes in
 * whole groups of three.
 * build: gcc -O2 -I../../oracle c2stats.c -lm -o /tmp/c2stats */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../oracle/zfp_oracle.c"

static double F(int x, int y, int z, int n)
{
  return sin(0.05 * x) * cos(0.03 * y) + 0.5 * sin(0.02 * z + 0.01 * x * y / n);
}

static int bitlen_u32(uint32_t x)
{
  int b = 0;
  while (x) b++, x >>= 1;
  return b;
}

/* thresholds of planes_from_coeffs_auto<P3, true> (block3.h) from the widths of
 * a wave's coefficients in negabinary: ksw = bitlen(c32..63 | c31 >> 1) - 1,
 * kS = bitlen(c15..63) for a narrow wave (every c32..63 below 2^8), else 32;
 * kT = bitlen(c4..63), at least kS */
static int classes(int n, int zstep)
{
  long nw = 0, narrow = 0, cls[32][3] = {{0}}, hS[34] = {0}, hW[34] = {0}, hT[34] = {0}, hG[5] = {0};
  for (int bz = 0; bz < n / 4; bz += zstep)
    for (int by = 0; by < n / 4; by++)
      for (int bx0 = 0; bx0 < n / 4; bx0 += 64) {
        uint32_t A = 0, B = 0, W = 0, T = 0;
        for (int l = 0; l < 64; l++) {
          float v[64];
          for (int i = 0; i < 64; i++)
            v[i] = (float)F(4 * (bx0 + l) + (i & 3), 4 * by + ((i >> 2) & 3), 4 * bz + (i >> 4), n);
          int emax = oz_emax_f(v, 64);
          int32_t q[64];
          oz_cast_fwd_f(q, v, 64, emax);
          oz_xform_f(q, 3, 0, 0);
          for (int i = 4; i < 64; i++) {
            const uint32_t u = oz_to_nb_f(q[oz_perm3[i]]);
            T |= u;
            if (i < 15) continue;
            W |= u;
            if (i == 31) B = B | u;
            if (i >= 32) A |= u;
          }
        }
        const int nar = A < 256u;
        const int ksw = bitlen_u32(A | (B >> 1)) - 1;
        int kS = nar ? bitlen_u32(W) : 32;
        if (kS <= ksw) kS = ksw + 1;
        int kT = nar ? bitlen_u32(T) : 32;
        if (kT < kS) kT = kS;
        int groups = 0; /* whole groups 31..29, 28..26, 25..23, 22..20 at or above kT */
        while (groups < 4 && 29 - 3 * groups >= kT) groups++;
        hT[kT]++;
        hG[groups]++;
        nw++;
        narrow += nar;
        hS[kS]++;
        hW[ksw + 1]++;
        for (int k = 0; k < 32; k++) cls[k][k >= kS ? 0 : k > ksw ? 1 : 2]++;
      }
  printf("waves %ld, narrow %ld (%.2f %%)\n", nw, narrow, 100.0 * narrow / nw);
  printf("plane  S %%     M %%     wide %%\n");
  for (int k = 31; k >= 0; k--)
    printf("%5d  %6.2f  %6.2f  %6.2f\n", k, 100.0 * cls[k][0] / nw, 100.0 * cls[k][1] / nw, 100.0 * cls[k][2] / nw);
  printf("kS (waves):");
  for (int i = 0; i <= 32; i++) if (hS[i]) printf(" %d:%ld", i, hS[i]);
  printf("\nkT (waves):");
  for (int i = 0; i <= 32; i++) if (hT[i]) printf(" %d:%ld (%.1f %%)", i, hT[i], 100.0 * hT[i] / nw);
  printf("\nclass-T groups of three planes (waves):");
  for (int i = 0; i <= 4; i++) if (hG[i]) printf(" %d:%ld (%.1f %%)", i, hG[i], 100.0 * hG[i] / nw);
  printf("\nksw (waves):");
  for (int i = 0; i <= 32; i++) if (hW[i]) printf(" %d:%ld", i - 1, hW[i]);
  printf("\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc > 1 && !strcmp(argv[1], "classes"))
    return classes(1024, argc > 2 ? atoi(argv[2]) : 1);
  const int n = 1024, waves = argc > 1 ? atoi(argv[1]) : 400;
  srand(3);
  double planes_sum = 0, p32_sum = 0, wmax_planes = 0, long_sec = 0, slow32 = 0;
  long hist_switch[40] = {0};
  for (int wv = 0; wv < waves; wv++) {
    int by = rand() % (n / 4), bz = rand() % (n / 4), bx0 = (rand() % (n / 4 / 64)) * 64;
    uint32_t nk[64] = {0}, bits[64], prec[64];
    uint32_t u[64][64];
    for (int l = 0; l < 64; l++) {
      float v[64];
      for (int i = 0; i < 64; i++)
        v[i] = (float)F(4 * (bx0 + l) + (i & 3), 4 * by + ((i >> 2) & 3), 4 * bz + (i >> 4), n);
      int emax = oz_emax_f(v, 64);
      int32_t q[64];
      oz_cast_fwd_f(q, v, 64, emax);
      oz_xform_f(q, 3, 0, 0);
      for (int i = 0; i < 64; i++) u[l][i] = oz_to_nb_f(q[oz_perm3[i]]);
      bits[l] = 1024 - 9;
      int p = emax - (-1074) + 2 * 3 + 2;
      prec[l] = p < 0 ? 0 : (p > 32 ? 32 : p);
    }
    /* planes in lockstep, as decode_planes32 runs them */
    int kswitch = -1, planes_w = 0;
    for (int k = 31; k >= 0; k--) {
      int any = 0, any_big = 0;
      for (int l = 0; l < 64; l++) if (nk[l] > 31) any_big = 1;
      if (any_big && kswitch < 0) kswitch = 31 - k;
      for (int l = 0; l < 64; l++) {
        if (!bits[l] || (uint32_t)k < 32 - prec[l]) continue;
        any = 1;
        uint32_t m = nk[l] < bits[l] ? nk[l] : bits[l];
        bits[l] -= m;
        uint32_t nn = nk[l], used = 0;
        /* group section: simulate the reference loop */
        for (; bits[l] && nn < 64; nn++) {
          int more = 0;
          for (uint32_t i = nn; i < 64; i++) if ((u[l][i] >> k) & 1u) { more = 1; break; }
          bits[l]--; used++;
          if (!more) break;
          for (; bits[l] && nn < 63; nn++) { uint32_t b = (u[l][nn] >> k) & 1u; bits[l]--; used++; if (b) break; }
        }
        if (used > 32) long_sec++;
        if (kswitch < 0 && (used > 32 || bits[l] < 64)) slow32++;
        nk[l] = nn;
        planes_sum++;
      }
      if (any) planes_w++;
    }
    if (kswitch < 0) kswitch = planes_w;
    hist_switch[kswitch < 39 ? kswitch : 39]++;
    p32_sum += kswitch;
    wmax_planes += planes_w;
  }
  printf("C2 blocks: planes per block %.2f; per wave: planes %.2f, of them in the 32-bit body %.2f\n",
         planes_sum / (64.0 * waves), wmax_planes / waves, p32_sum / waves);
  printf("block-planes with a section past 32 bits %.2f per block; lanes taking decode_plane64 inside the 32-bit phase %.2f per wave\n",
         long_sec / (64.0 * waves), slow32 / waves);
  printf("32-bit planes per wave (hist):");
  for (int i = 0; i < 40; i++) if (hist_switch[i]) printf(" %d:%ld", i, hist_switch[i]);
  printf("\n");
  return 0;
}
