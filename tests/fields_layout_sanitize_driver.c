/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_fields_convert_layout under the host
 * sanitizers: the shapes of tests/fields_layout_cases.py over the four storage pairs, both directions and
 * the two forwarded pairs, every array an exact-size heap block (so AddressSanitizer's red zones are the
 * guard margins around every destination), every destination element checked against the index rule.
 * Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/fields_layout_sanitize_driver there: this driver alone)
 *
 * (The conversion code under test is the instrumented copy linked into the program: a definition in the
 * executable comes before a shared library's in the symbol search order, for the program's own calls and for
 * the calls between the two instrumented units alike, and neither unit is reached through the library.  The
 * padding lanes inside a blocked destination are checked byte by byte.) */
#include "sanitize_common.h"

static double value(int m, long row, long g) { return (double)(((long)(m % 16) << 20) + (row << 9) + g); }   /* < 2^24: exact in float */

/* snp, dnp 0: the LEVELS layout */
static long run_case(int ngptot, int snp, int dnp, int sp, int dp, int klev, int outputs, int nthreads) {
  const int surface = outputs == CLOUDSC_OUTPUTS_SURFACE;
  cloudsc_fields_t src, dst;
  void **s = (void **)&src, **d = (void **)&dst;
  long bad = 0;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    s[m] = make_member(m, sp, ngptot, rows_of(kind_of(m, surface), klev), snp, 0x11, value);
    d[m] = make_member(m, dp, ngptot, rows_of(kind_of(m, surface), klev), dnp, 0x5A, NULL);
  }
  const int rc = cloudsc_cpu_fields_convert_layout(nthreads, ngptot, klev, outputs, sp,
                                                   snp ? CLOUDSC_LAYOUT_BLOCKED : CLOUDSC_LAYOUT_LEVELS, snp, &src, dp,
                                                   dnp ? CLOUDSC_LAYOUT_BLOCKED : CLOUDSC_LAYOUT_LEVELS, dnp, &dst);
  if (rc) { printf("rc %d\n", rc); bad++; }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)   /* the values, and the padding lanes of a blocked destination untouched */
    bad += check_member(d[m], m, dp, ngptot, rows_of(kind_of(m, surface), klev), dnp, 0x5A, value);
  free_set(&src, NULL);
  free_set(&dst, NULL);
  return bad;
}

int main(void) {
  /* (ngptot, NPROMA of the blocked side, klev) */
  static const int shapes[][3] = {{1, 64, 3}, {1, 5, 17}, {63, 64, 15}, {63, 16, 16}, {64, 64, 16}, {64, 5, 3},
                                  {65, 64, 17}, {65, 16, 15}, {65, 300, 137}, {255, 64, 3}, {255, 300, 16},
                                  {257, 16, 17}, {257, 5, 15}, {300, 64, 137}, {300, 16, 3}, {300, 5, 17},
                                  {300, 300, 15}, {300, 64, 16}};
  long bad = 0;
  int cases = 0;
  for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); i++)
    for (unsigned p = 0; p < 4; p++) {
      const int n = shapes[i][0], np = shapes[i][1], klev = shapes[i][2], sp = k_storage[p][0], dp = k_storage[p][1];
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
  return sanitize_result("fields_layout_sanitize_driver", cases, bad);
}
