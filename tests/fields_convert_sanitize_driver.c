/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_fields_convert under the host
 * sanitizers: the shape table of tests/fields_convert_cases.py over the four storage pairs, every array
 * an exact-size heap block (so AddressSanitizer sees any access past an array), every destination
 * element checked against the index rule.  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/fields_convert_sanitize_driver.c -o obj/fc_driver.o
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -I../include -Icsrc obj/fc_driver.o csrc/cloudsc_convert.hip \
 *       -L. -lcloudsc_amd -Wl,-rpath,$PWD -o obj/fc_driver && obj/fc_driver
 *
 * (clang: the one hipcc drives, so both objects share one sanitizer runtime.)
 *
 * (libcloudsc_amd.so only supplies the error-text helper the device entry point refers to; the
 * conversion code under test is the instrumented copy linked into the program.) */
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

static long rows_of(int kind, int klev) {
  return kind == CLOUDSC_FK_LEVEL ? klev : kind == CLOUDSC_FK_HALF ? klev + 1 : kind == CLOUDSC_FK_SPECIES ? 5L * klev : 1;
}
static size_t esize(int m, int precision) { return is_int[m] ? 4 : precision == CLOUDSC_FP64 ? 8 : 4; }
static double value(int m, long row, long g) { return (double)((m << 18) + (row << 8) + g); }

static void put(void *a, int m, int precision, size_t i, double v) {
  if (is_int[m]) ((int *)a)[i] = (int)v;
  else if (precision == CLOUDSC_FP64) ((double *)a)[i] = v;
  else ((float *)a)[i] = (float)v;
}
static double get(const void *a, int m, int precision, size_t i) {
  if (is_int[m]) return ((const int *)a)[i];
  return precision == CLOUDSC_FP64 ? ((const double *)a)[i] : ((const float *)a)[i];
}

static int run_case(int ngptot, int snp, int dnp, int sp, int dp, int klev, int nthreads) {
  cloudsc_fields_t src, dst;
  void **s = (void **)&src, **d = (void **)&dst;
  const long snb = (ngptot + snp - 1) / snp, dnb = (ngptot + dnp - 1) / dnp;
  int bad = 0;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    const long rows = rows_of(kinds[m], klev);
    s[m] = malloc((size_t)(snb * rows * snp) * esize(m, sp));
    d[m] = malloc((size_t)(dnb * rows * dnp) * esize(m, dp));
    if (!s[m] || !d[m]) return 1;
    memset(s[m], 0x11, (size_t)(snb * rows * snp) * esize(m, sp));
    memset(d[m], 0x5A, (size_t)(dnb * rows * dnp) * esize(m, dp));
    for (long g = 0; g < ngptot; g++)
      for (long r = 0; r < rows; r++) put(s[m], m, sp, (size_t)((g / snp * rows + r) * snp + g % snp), value(m, r, g));
  }
  const int rc = cloudsc_cpu_fields_convert(nthreads, ngptot, klev, sp, snp, &src, dp, dnp, &dst);
  if (rc) { printf("rc %d\n", rc); bad++; }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    const long rows = rows_of(kinds[m], klev);
    for (long b = 0; b < dnb; b++)
      for (long r = 0; r < rows; r++)
        for (long j = 0; j < dnp; j++) {
          const long g = b * dnp + j;
          const size_t i = (size_t)((b * rows + r) * dnp + j);
          if (g < ngptot) bad += get(d[m], m, dp, i) != value(m, r, g);
          else bad += ((const unsigned char *)d[m])[i * esize(m, dp)] != 0x5A;   /* a padding lane: untouched */
        }
    free(s[m]);
    free(d[m]);
  }
  return bad;
}

int main(void) {
  static const int shapes[][3] = {{150, 8, 64}, {150, 64, 8}, {150, 24, 64}, {150, 64, 24},
                                  {100, 100, 64}, {130, 1, 64}, {64, 64, 64}, {150, 32, 150}};
  static const int storage[][2] = {{CLOUDSC_FP64, CLOUDSC_FP64}, {CLOUDSC_FP64, CLOUDSC_MIXED},
                                   {CLOUDSC_MIXED, CLOUDSC_FP64}, {CLOUDSC_FP32, CLOUDSC_FP32}};
  int bad = 0, cases = 0;
  for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); i++)
    for (unsigned p = 0; p < 4; p++)
      for (int nthreads = 1; nthreads <= 3; nthreads += 2, cases++)
        bad += run_case(shapes[i][0], shapes[i][1], shapes[i][2], storage[p][0], storage[p][1], 3, nthreads);
  bad += run_case(150, 24, 64, CLOUDSC_FP64, CLOUDSC_MIXED, 137, 4);
  /* argument rules: refused before anything is touched */
  cloudsc_fields_t none;
  memset(&none, 0, sizeof(none));
  bad += cloudsc_cpu_fields_convert(1, 10, 3, CLOUDSC_FP64, 8, &none, CLOUDSC_FP64, 8, &none) != CLOUDSC_EINVAL;
  bad += cloudsc_cpu_fields_convert(1, 10, 3, CLOUDSC_FP64, 8, NULL, CLOUDSC_FP64, 8, &none) != CLOUDSC_EINVAL;
  printf("%d cases, %d mismatches: %s\n", cases + 1, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
