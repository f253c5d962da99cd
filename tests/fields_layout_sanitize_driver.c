/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_fields_convert_layout under the host
 * sanitizers: the shapes of tests/fields_layout_cases.py over the four storage pairs, both directions and
 * the two forwarded pairs, every array an exact-size heap block (so AddressSanitizer's red zones are the
 * guard margins around every destination), every destination element checked against the index rule.
 * Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/fields_layout_sanitize_driver.c -o obj/fl_driver.o
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -I../include -Icsrc obj/fl_driver.o csrc/cloudsc_transpose.hip \
 *       csrc/cloudsc_convert.hip -L. -lcloudsc_amd -Wl,-rpath,$PWD -o obj/fl_driver && obj/fl_driver
 *
 * (clang: the one hipcc drives, so both objects share one sanitizer runtime.  libcloudsc_amd.so only
 * supplies the error-text helper the device entry points refer to; the conversion code under test is the
 * instrumented copy linked into the program: a definition in the executable comes before a shared
 * library's in the symbol search order, for the program's own calls and for the calls between the two
 * instrumented units alike, and neither unit is reached through the library.  The guard margins around
 * every destination are AddressSanitizer's red zones around these exact-size blocks; the padding lanes
 * inside a blocked destination are checked byte by byte below.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cloudsc_amd.h"
#include "cloudsc_fields.def"

#define KIND_ROW(n, N, k, d, i) CLOUDSC_FK_##k,
#define INT_ROW(n, N, k, d, i) i,
static const int kinds[] = {CLOUDSC_FIELDS(KIND_ROW)};
static const int is_int[] = {CLOUDSC_FIELDS(INT_ROW)};

static long rows_of(int m, int klev, int outputs) {
  const int kind = kinds[m];
  if (outputs == CLOUDSC_OUTPUTS_SURFACE && m >= CLOUDSC_M_pfplsl && m <= CLOUDSC_M_pfhpsn) return 1;
  return kind == CLOUDSC_FK_LEVEL ? klev : kind == CLOUDSC_FK_HALF ? klev + 1 : kind == CLOUDSC_FK_SPECIES ? 5L * klev : 1;
}
static size_t esize(int m, int precision) { return is_int[m] ? 4 : precision == CLOUDSC_FP64 ? 8 : 4; }
static double value(int m, long row, long g) { return (double)(((long)(m % 16) << 20) + (row << 9) + g); }   /* < 2^24: exact in float */

static void put(void *a, int m, int precision, size_t i, double v) {
  if (is_int[m]) ((int *)a)[i] = (int)v;
  else if (precision == CLOUDSC_FP64) ((double *)a)[i] = v;
  else ((float *)a)[i] = (float)v;
}
static double get(const void *a, int m, int precision, size_t i) {
  if (is_int[m]) return ((const int *)a)[i];
  return precision == CLOUDSC_FP64 ? ((const double *)a)[i] : ((const float *)a)[i];
}
/* np 0: the LEVELS layout */
static size_t elems(long ngptot, long rows, long np) { return (size_t)(np ? (ngptot + np - 1) / np * rows * np : ngptot * rows); }
static size_t at(long g, long r, long rows, long np) {
  return (size_t)(np ? (g / np * rows + r) * np + g % np : g * rows + r);
}

static int run_case(int ngptot, int snp, int dnp, int sp, int dp, int klev, int outputs, int nthreads) {
  cloudsc_fields_t src, dst;
  void **s = (void **)&src, **d = (void **)&dst;
  int bad = 0;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    const long rows = rows_of(m, klev, outputs);
    const size_t sn = elems(ngptot, rows, snp) * esize(m, sp), dn = elems(ngptot, rows, dnp) * esize(m, dp);
    s[m] = malloc(sn);
    d[m] = malloc(dn);
    if (!s[m] || !d[m]) return 1;
    memset(s[m], 0x11, sn);
    memset(d[m], 0x5A, dn);
    for (long g = 0; g < ngptot; g++)
      for (long r = 0; r < rows; r++) put(s[m], m, sp, at(g, r, rows, snp), value(m, r, g));
  }
  const int rc = cloudsc_cpu_fields_convert_layout(nthreads, ngptot, klev, outputs, sp,
                                                   snp ? CLOUDSC_LAYOUT_BLOCKED : CLOUDSC_LAYOUT_LEVELS, snp, &src, dp,
                                                   dnp ? CLOUDSC_LAYOUT_BLOCKED : CLOUDSC_LAYOUT_LEVELS, dnp, &dst);
  if (rc) { printf("rc %d\n", rc); bad++; }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    const long rows = rows_of(m, klev, outputs);
    const size_t n = elems(ngptot, rows, dnp);
    size_t live = 0;
    for (long g = 0; g < ngptot; g++)
      for (long r = 0; r < rows; r++, live++) bad += get(d[m], m, dp, at(g, r, rows, dnp)) != value(m, r, g);
    /* the padding lanes of a blocked destination: untouched */
    for (long b = 0; dnp && b < (ngptot + dnp - 1) / dnp; b++)
      for (long r = 0; r < rows; r++)
        for (long j = 0; j < dnp; j++)
          if (b * dnp + j >= ngptot) {
            const unsigned char *p = (const unsigned char *)d[m] + (size_t)((b * rows + r) * dnp + j) * esize(m, dp);
            for (size_t k = 0; k < esize(m, dp); k++) bad += p[k] != 0x5A;
            live++;
          }
    bad += live != n;
    free(s[m]);
    free(d[m]);
  }
  return bad;
}

int main(void) {
  /* (ngptot, NPROMA of the blocked side, klev) */
  static const int shapes[][3] = {{1, 64, 3}, {1, 5, 17}, {63, 64, 15}, {63, 16, 16}, {64, 64, 16}, {64, 5, 3},
                                  {65, 64, 17}, {65, 16, 15}, {65, 300, 137}, {255, 64, 3}, {255, 300, 16},
                                  {257, 16, 17}, {257, 5, 15}, {300, 64, 137}, {300, 16, 3}, {300, 5, 17},
                                  {300, 300, 15}, {300, 64, 16}};
  static const int storage[][2] = {{CLOUDSC_FP64, CLOUDSC_FP64}, {CLOUDSC_FP64, CLOUDSC_MIXED},
                                   {CLOUDSC_MIXED, CLOUDSC_FP64}, {CLOUDSC_FP32, CLOUDSC_FP32}};
  int bad = 0, cases = 0;
  for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); i++)
    for (unsigned p = 0; p < 4; p++) {
      const int n = shapes[i][0], np = shapes[i][1], klev = shapes[i][2], sp = storage[p][0], dp = storage[p][1];
      const int nthreads = 1 + (int)((i + p) % 3);
      bad += run_case(n, np, 0, sp, dp, klev, CLOUDSC_OUTPUTS_ALL, nthreads);   /* BLOCKED -> LEVELS */
      bad += run_case(n, 0, np, sp, dp, klev, CLOUDSC_OUTPUTS_ALL, nthreads);   /* LEVELS -> BLOCKED */
      cases += 2;
    }
  /* the surface selection, and the two forwarded pairs */
  bad += run_case(300, 24, 0, CLOUDSC_FP64, CLOUDSC_MIXED, 17, CLOUDSC_OUTPUTS_SURFACE, 2);
  bad += run_case(300, 0, 24, CLOUDSC_MIXED, CLOUDSC_FP64, 17, CLOUDSC_OUTPUTS_SURFACE, 2);
  bad += run_case(300, 0, 0, CLOUDSC_FP64, CLOUDSC_MIXED, 17, CLOUDSC_OUTPUTS_SURFACE, 2);
  bad += run_case(300, 24, 64, CLOUDSC_FP64, CLOUDSC_MIXED, 17, CLOUDSC_OUTPUTS_SURFACE, 2);
  cases += 4;
  /* argument rules: refused before anything is touched */
  cloudsc_fields_t none;
  memset(&none, 0, sizeof(none));
  bad += cloudsc_cpu_fields_convert_layout(1, 10, 3, 0, CLOUDSC_FP64, 1, 0, &none, CLOUDSC_FP64, 0, 8, &none) != CLOUDSC_EINVAL;
  bad += cloudsc_cpu_fields_convert_layout(1, 10, 3, 0, CLOUDSC_FP64, 1, 10, NULL, CLOUDSC_FP64, 0, 8, &none) != CLOUDSC_EINVAL;
  bad += cloudsc_cpu_fields_convert_layout(1, 10, 3, 0, CLOUDSC_FP64, 2, 0, NULL, CLOUDSC_FP64, 0, 8, &none) != CLOUDSC_EINVAL;
  printf("%d cases, %d mismatches: %s\n", cases, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
