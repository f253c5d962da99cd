/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_run_outputs under the host sanitizers, on
 * the data set data/cloudsc100 at the shapes 100 / 16, 300 / 64 and 1 / 1, fp64 and mixed.  Every array is an
 * exact-size heap block (so AddressSanitizer sees any access past one).  Per case, with
 * CLOUDSC_OUTPUTS_PROGNOSTIC: once with the ten diagnostic flux members NULL (any access to one is a
 * NULL dereference), once with them pointing at arrays filled with a byte that must all come back
 * unchanged; the eleven kept outputs compared with cloudsc_cpu_run_precision on a second set, byte for
 * byte over the real columns, and their padding lanes must keep the fill byte.  Then CLOUDSC_OUTPUTS_ALL
 * against the same reference over all 21.  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/outputs_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = nblocks(ngptot, nproma);
  cloudsc_fields_t ref, null_set, kept_set, all_set;
  long bad = 0;
  make_set(ds, ngptot, nproma, es, 0, FILL, &ref);
  make_set(ds, ngptot, nproma, es, SET_NO_DIAG, FILL, &null_set);
  make_set(ds, ngptot, nproma, es, 0, FILL, &kept_set);
  make_set(ds, ngptot, nproma, es, 0, FILL, &all_set);
  if (cloudsc_cpu_run_precision(2, precision, ngptot, nproma, klev, &ds->params, &ref, NULL)) bad += FAILED;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &null_set))
    bad += FAILED;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &kept_set))
    bad += FAILED;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &all_set))
    bad += FAILED;
  /* ALL with a member missing is refused, not run */
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &null_set) !=
      CLOUDSC_EINVAL)
    bad += FAILED;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (!is_output(m)) continue;
    void *r = ((void **)&ref)[m], *n = ((void **)&null_set)[m], *k = ((void **)&kept_set)[m],
         *a = ((void **)&all_set)[m];
    const long rows = rows_of(kinds[m], klev);
    bad += differing(ds, m, ngptot, nproma, es, a, r);
    if (dirs[m] == CLOUDSC_FD_OUT) bad += padding_written(rows, ngptot, nproma, es, a, FILL);
    if (is_diagnostic(m)) {
      if (n) bad += FAILED;
      bad += not_fill(k, member_bytes(ds, m, nb, nproma, es, 0), FILL);   /* every byte kept */
      if (!not_fill(r, member_bytes(ds, m, nb, nproma, es, 0), FILL)) bad += FAILED;   /* the reference did write it */
    } else {
      bad += differing(ds, m, ngptot, nproma, es, n, r) + differing(ds, m, ngptot, nproma, es, k, r);
      if (dirs[m] == CLOUDSC_FD_OUT)
        bad += padding_written(rows, ngptot, nproma, es, n, FILL) + padding_written(rows, ngptot, nproma, es, k, FILL);
    }
  }
  free_set(&ref, NULL);
  free_set(&null_set, NULL);
  free_set(&kept_set, NULL);
  free_set(&all_set, NULL);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("outputs_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++, cases++) bad += run_case(&ds, k_shapes[s][0], k_shapes[s][1], k_precisions[p]);
  cloudsc_io_free(&ds);
  return sanitize_result("outputs_sanitize_driver", cases, bad);
}
