/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_run_spp under the host sanitizers, on the data
 * set data/cloudsc100 at the shapes 100 / 16, 300 / 64 (a partial last block each) and 1 / 1, fp64 and mixed.
 * Every array is an exact-size heap block, and a multiplier field ends at its last REAL column: a read of a
 * padding lane of the partial last block is a heap overflow AddressSanitizer reports.  Per case: all five
 * members all-ones against cloudsc_cpu_run_outputs(ALL), byte for byte over all 21 outputs; tuples that vary by
 * column with two members NULL, CLOUDSC_OUTPUTS_PROGNOSTIC and the ten diagnostic members NULL (any access to
 * one is a NULL dereference), against the same run with ones behind the NULL members and the diagnostic members
 * pointing at filled arrays, which must come back unchanged; padding lanes of the outputs keep the fill byte.
 * Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/spp_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

/* a multiplier field of exactly ngptot elements (block layout up to the last real column): column g holds
 * tuples[(7 g + g / 16) % 4][slot], or 1 */
static const double k_tuples[4][5] = {{1, 1, 1, 1, 1},
                                      {0.7531, 1.2519, 0.5017, 1.2483, 0.7469},
                                      {1.1203, 0.7487, 1.4989, 0.7523, 1.2511},
                                      {1.0, 1.2519, 1.0, 0.7523, 1.0}};
static void *make_mult(int ngptot, int es, int slot, int ones) {
  void *p = alloc_filled((size_t)ngptot * (size_t)es, 0);
  for (int g = 0; g < ngptot; g++) {
    const double x = ones ? 1.0 : k_tuples[(7 * g + g / 16) % 4][slot];
    if (es == 8) ((double *)p)[g] = x;
    else ((float *)p)[g] = (float)x;
  }
  return p;
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = nblocks(ngptot, nproma);
  cloudsc_fields_t ref, ones_set, null_set, kept_set;
  long bad = 0;
  make_set(ds, ngptot, nproma, es, 0, FILL, &ref);
  make_set(ds, ngptot, nproma, es, 0, FILL, &ones_set);
  make_set(ds, ngptot, nproma, es, SET_NO_DIAG, FILL, &null_set);
  make_set(ds, ngptot, nproma, es, 0, FILL, &kept_set);
  void *one[5], *mix[5];
  for (int s = 0; s < 5; s++) {
    one[s] = make_mult(ngptot, es, s, 1);
    mix[s] = make_mult(ngptot, es, s, 0);
  }
  const cloudsc_spp_t all_ones = {one[0], one[1], one[2], one[3], one[4]};
  const cloudsc_spp_t some = {mix[0], NULL, mix[2], mix[3], NULL};           /* rcldiff, rpecons: not perturbed */
  const cloudsc_spp_t some_ones = {mix[0], one[1], mix[2], mix[3], one[4]};  /* the same, said with ones */
  const cloudsc_spp_t none = {NULL, NULL, NULL, NULL, NULL};
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref)) bad += FAILED;
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ones_set, &all_ones))
    bad += FAILED;
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &null_set, &some))
    bad += FAILED;
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &kept_set,
                          &some_ones))
    bad += FAILED;
  /* refused, not run: no spp, no member, a member that is a field of the set, the surface selection */
  const cloudsc_spp_t alias = {mix[0], NULL, ref.plsm, NULL, NULL};
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref, NULL) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref, &none) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref, &alias) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &ref, &some) != CLOUDSC_EINVAL)
    bad += FAILED;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (!is_output(m)) continue;
    void *r = ((void **)&ref)[m], *o = ((void **)&ones_set)[m], *n = ((void **)&null_set)[m],
         *k = ((void **)&kept_set)[m];
    const long rows = rows_of(kinds[m], klev);
    bad += differing(ds, m, ngptot, nproma, es, o, r);
    if (dirs[m] == CLOUDSC_FD_OUT) bad += padding_written(rows, ngptot, nproma, es, o, FILL);
    if (is_diagnostic(m)) {
      if (n) bad += FAILED;
      bad += not_fill(k, member_bytes(ds, m, nb, nproma, es, 0), FILL);   /* every byte kept */
    } else {
      bad += differing(ds, m, ngptot, nproma, es, n, k);
      if (dirs[m] == CLOUDSC_FD_OUT)
        bad += padding_written(rows, ngptot, nproma, es, n, FILL) + padding_written(rows, ngptot, nproma, es, k, FILL);
    }
  }
  for (int s = 0; s < 5; s++) { free(one[s]); free(mix[s]); }
  free_set(&ref, NULL);
  free_set(&ones_set, NULL);
  free_set(&null_set, NULL);
  free_set(&kept_set, NULL);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("spp_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++, cases++) bad += run_case(&ds, k_shapes[s][0], k_shapes[s][1], k_precisions[p]);
  cloudsc_io_free(&ds);
  return sanitize_result("spp_sanitize_driver", cases, bad);
}
