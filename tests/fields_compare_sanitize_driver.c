/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_fields_compare under the host
 * sanitizers: three shapes over the four storage pairs, every array an exact-size heap block (so
 * AddressSanitizer sees any access past an array), padding lanes poisoned with values that would show
 * in every statistic, one element of b changed per member, every record checked against the index
 * rule.  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/fields_compare_sanitize_driver.c -o obj/cmp_driver.o
 *   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -I../include -Icsrc obj/cmp_driver.o csrc/cloudsc_compare.hip \
 *       -L. -lcloudsc_amd -Wl,-rpath,$PWD -o obj/cmp_driver && obj/cmp_driver
 *
 * (clang: the one hipcc drives, so both objects share one sanitizer runtime.  libcloudsc_amd.so only
 * supplies the error-text helper the device entry points refer to; the comparison code under test is
 * the instrumented copy linked into the program.) */
#include <float.h>
#include <math.h>
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
static double value(int m, long row, long g) { return (double)(((m % 16) << 20) + (row << 10) + g); }

static void put(void *a, int m, int precision, size_t i, double v) {
  if (is_int[m]) ((int *)a)[i] = (int)v;
  else if (precision == CLOUDSC_FP64) ((double *)a)[i] = v;
  else ((float *)a)[i] = (float)v;
}

/* a set in block layout: value() in the active lanes, `poison` in the padding lanes */
static void *make(int m, int precision, int ngptot, int np, int klev, double poison) {
  const long rows = rows_of(kinds[m], klev), nb = (ngptot + np - 1) / np;
  void *a = malloc((size_t)(nb * rows * np) * esize(m, precision));
  if (!a) return NULL;
  for (long b = 0; b < nb; b++)
    for (long r = 0; r < rows; r++)
      for (long j = 0; j < np; j++)
        put(a, m, precision, (size_t)((b * rows + r) * np + j), b * np + j < ngptot ? value(m, r, b * np + j) : poison);
  return a;
}

static int run_case(int ngptot, int anp, int bnp, int ap, int bp, int klev, int nthreads) {
  cloudsc_fields_t fa, fb;
  void **a = (void **)&fa, **b = (void **)&fb;
  cloudsc_field_diff_t *diff = (cloudsc_field_diff_t *)malloc(sizeof(cloudsc_field_diff_t) * CLOUDSC_NFIELDS);
  int bad = 0;
  if (!diff) return 1;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    a[m] = make(m, ap, ngptot, anp, klev, -1e9);
    b[m] = make(m, bp, ngptot, bnp, klev, 1e9);
    if (!a[m] || !b[m]) return 1;
    /* b's last active column, last row: + 3 */
    const long rows = rows_of(kinds[m], klev), g = ngptot - 1, r = rows - 1;
    put(b[m], m, bp, (size_t)((g / bnp * rows + r) * bnp + g % bnp), value(m, r, g) + 3.0);
  }
  const int rc = cloudsc_cpu_fields_compare(nthreads, ngptot, klev, ap, anp, &fa, bp, bnp, &fb, diff);
  if (rc) { printf("rc %d\n", rc); bad++; }
  for (int m = 0; m < CLOUDSC_NFIELDS && !rc; m++) {
    const long rows = rows_of(kinds[m], klev);
    const cloudsc_field_diff_t *d = &diff[m];
    double refsum = 3.0;
    for (long g = 0; g < ngptot; g++)
      for (long r = 0; r < rows; r++) refsum += value(m, r, g);   /* integers below 2^53: exact */
    bad += d->compared != rows * ngptot || d->mismatches != 1 || d->first_column != ngptot - 1 || d->first_row != rows - 1;
    bad += d->stats.minval != value(m, 0, 0) || d->stats.maxval != value(m, rows - 1, ngptot - 1);
    bad += d->stats.maxerr != 3.0 || d->stats.errsum != 3.0 || d->stats.errsum_lo != 0.0;
    bad += d->stats.refsum != refsum || d->stats.refsum_lo != 0.0;
    free(a[m]);
    free(b[m]);
  }
  free(diff);
  return bad;
}

int main(void) {
  static const int shapes[][3] = {{150, 24, 64}, {333, 300, 64}, {130, 1, 64}};
  static const int storage[][2] = {{CLOUDSC_FP64, CLOUDSC_FP64}, {CLOUDSC_FP64, CLOUDSC_MIXED},
                                   {CLOUDSC_MIXED, CLOUDSC_FP64}, {CLOUDSC_FP32, CLOUDSC_FP32}};
  int bad = 0, cases = 0;
  for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); i++)
    for (unsigned p = 0; p < 4; p++)
      for (int nthreads = 1; nthreads <= 3; nthreads += 2, cases++)
        bad += run_case(shapes[i][0], shapes[i][1], shapes[i][2], storage[p][0], storage[p][1], 3, nthreads);
  bad += run_case(1000, 64, 24, CLOUDSC_FP64, CLOUDSC_MIXED, 137, 4);
  /* argument rules: refused before anything is touched */
  cloudsc_fields_t none;
  cloudsc_field_diff_t one[CLOUDSC_NFIELDS];
  memset(&none, 0, sizeof(none));
  bad += cloudsc_cpu_fields_compare(1, 10, 3, CLOUDSC_FP64, 8, &none, CLOUDSC_FP64, 8, &none, one) != CLOUDSC_EINVAL;
  bad += cloudsc_cpu_fields_compare(1, 10, 3, CLOUDSC_FP64, 8, NULL, CLOUDSC_FP64, 8, &none, one) != CLOUDSC_EINVAL;
  printf("%d cases, %d mismatches: %s\n", cases + 1, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
