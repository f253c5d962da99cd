/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_fields_compare under the host
 * sanitizers: three shapes over the four storage pairs, every array an exact-size heap block (so
 * AddressSanitizer sees any access past an array), padding lanes poisoned with values that would show
 * in every statistic, one element of b changed per member, every record checked against the index
 * rule.  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/fields_compare_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

static double value(int m, long row, long g) { return (double)(((m % 16) << 20) + (row << 10) + g); }

/* a member in block layout: value() in the active lanes, `poison` in the padding lanes */
static void *make(int m, int precision, int ngptot, int np, int klev, double poison) {
  const long rows = rows_of(kinds[m], klev), nb = nblocks(ngptot, np);
  void *a = make_member(m, precision, ngptot, rows, np, 0, value);
  for (long r = 0; r < rows; r++)
    for (long g = ngptot; g < nb * np; g++) put(a, m, precision, at(g, r, rows, np), poison);
  return a;
}

static long run_case(int ngptot, int anp, int bnp, int ap, int bp, int klev, int nthreads) {
  cloudsc_fields_t fa, fb;
  void **a = (void **)&fa, **b = (void **)&fb;
  cloudsc_field_diff_t *diff = (cloudsc_field_diff_t *)alloc_filled(sizeof(cloudsc_field_diff_t) * CLOUDSC_NFIELDS, 0);
  long bad = 0;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    a[m] = make(m, ap, ngptot, anp, klev, -1e9);
    b[m] = make(m, bp, ngptot, bnp, klev, 1e9);
    /* b's last active column, last row: + 3 */
    const long rows = rows_of(kinds[m], klev), g = ngptot - 1, r = rows - 1;
    put(b[m], m, bp, at(g, r, rows, bnp), value(m, r, g) + 3.0);
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
  }
  free(diff);
  free_set(&fa, NULL);
  free_set(&fb, NULL);
  return bad;
}

int main(void) {
  static const int shapes[][3] = {{150, 24, 64}, {333, 300, 64}, {130, 1, 64}};
  long bad = 0;
  int cases = 0;
  for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); i++)
    for (unsigned p = 0; p < 4; p++)
      for (int nthreads = 1; nthreads <= 3; nthreads += 2, cases++)
        bad += run_case(shapes[i][0], shapes[i][1], shapes[i][2], k_storage[p][0], k_storage[p][1], 3, nthreads);
  bad += run_case(1000, 64, 24, CLOUDSC_FP64, CLOUDSC_MIXED, 137, 4);
  /* argument rules: refused before anything is touched */
  cloudsc_fields_t none;
  cloudsc_field_diff_t one[CLOUDSC_NFIELDS];
  memset(&none, 0, sizeof(none));
  bad += cloudsc_cpu_fields_compare(1, 10, 3, CLOUDSC_FP64, 8, &none, CLOUDSC_FP64, 8, &none, one) != CLOUDSC_EINVAL;
  bad += cloudsc_cpu_fields_compare(1, 10, 3, CLOUDSC_FP64, 8, NULL, CLOUDSC_FP64, 8, &none, one) != CLOUDSC_EINVAL;
  return sanitize_result("fields_compare_sanitize_driver", cases + 1, bad);
}
