/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_run_outputs and cloudsc_cpu_run_tendbuf_outputs
 * with CLOUDSC_OUTPUTS_SURFACE under the host sanitizers, on the data set data/cloudsc100 at the shapes
 * 100 / 16, 300 / 64 and 1 / 1, fp64 and mixed.  Every array is an exact-size heap block, so AddressSanitizer
 * sees any access past one: the four surface members pfplsl, pfplsn, pfhpsl, pfhpsn are nblocks * nproma
 * elements and not one more (a profile-sized store is a heap overflow).  Per case: once with the ten diagnostic
 * flux members NULL (any access to one is a NULL dereference), once with them pointing at arrays filled with a
 * byte that must all come back unchanged; once more with the tendencies in two packed buffers of 11 planes.  The
 * seven full-size outputs are compared with cloudsc_cpu_run_precision on a second set, byte for byte over the
 * real columns, the four surface fields with row klev of that set's profiles, and padding lanes must keep the
 * fill byte.  The value 4 (the surface bit alone) must be refused.  Exit status 0 and "clean" on success.  No
 * GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/outputs_surface_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

#define PLANES 11

/* the outputs of a SURFACE set s against the full step's set ref; loc_brows: rows between the blocks of the
 * tendency_loc_* members of s (0: their own rows, separate arrays) */
static long check_surface_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, const cloudsc_fields_t *s,
                              const cloudsc_fields_t *ref, int with_diag, long loc_brows) {
  const int klev = ds->klev, nb = nblocks(ngptot, nproma);
  long bad = 0;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (!is_output(m)) continue;
    const void *a = ((void *const *)s)[m], *r = ((void *const *)ref)[m];
    const long rows = rows_of(kinds[m], klev);
    if (is_diagnostic(m)) {
      if (!with_diag) bad += a ? FAILED : 0;
      else bad += not_fill(a, member_bytes(ds, m, nb, nproma, es, 0), FILL);   /* every byte kept */
    } else if (is_surface_flux(m)) {   /* one row against row klev of the profile */
      bad += differing_rows(ngptot, nproma, (size_t)es, a, 1, 0, r, rows, klev, 1);
      bad += padding_written(1, ngptot, nproma, es, a, FILL);
    } else {
      const long brows = loc_brows && is_tendency_loc(m) ? loc_brows : rows;
      bad += differing_rows(ngptot, nproma, (size_t)es, a, brows, 0, r, rows, 0, rows);
      if (dirs[m] == CLOUDSC_FD_OUT && brows == rows) bad += padding_written(rows, ngptot, nproma, es, a, FILL);
    }
  }
  return bad;
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = nblocks(ngptot, nproma);
  cloudsc_fields_t ref, null_set, kept_set, buf_set;
  long bad = 0;
  make_set(ds, ngptot, nproma, es, 0, FILL, &ref);
  make_set(ds, ngptot, nproma, es, SET_SURFACE | SET_NO_DIAG, FILL, &null_set);
  make_set(ds, ngptot, nproma, es, SET_SURFACE, FILL, &kept_set);
  make_set(ds, ngptot, nproma, es, SET_SURFACE | SET_NO_DIAG, FILL, &buf_set);
  if (cloudsc_cpu_run_precision(2, precision, ngptot, nproma, klev, &ds->params, &ref, NULL)) bad += FAILED;
  /* the surface bit alone is not a selection */
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE_BIT, ngptot, nproma, klev, &ds->params,
                              &null_set) != CLOUDSC_EINVAL)
    bad += FAILED;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &null_set))
    bad += FAILED;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &kept_set))
    bad += FAILED;
  bad += check_surface_set(ds, ngptot, nproma, es, &null_set, &ref, 0, 0);
  bad += check_surface_set(ds, ngptot, nproma, es, &kept_set, &ref, 1, 0);
  /* the packed tendency buffers: exact-size blocks too, BUFFER_TMP filled from the set's separate arrays */
  const size_t plane = (size_t)klev * nproma * es, bufb = (size_t)nb * PLANES * plane;
  char *tmp = (char *)alloc_filled(bufb, FILL), *loc = (char *)alloc_filled(bufb, FILL);
  cloudsc_fields_t g = buf_set;
  if (cloudsc_tendbuf_bind(&g, precision, nproma, klev, tmp, loc)) bad += FAILED;
  pack_tmp(&buf_set, nb, PLANES, plane, tmp);
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, PLANES, &ds->params,
                                      &g))
    bad += FAILED;
  bad += check_surface_set(ds, ngptot, nproma, es, &g, &ref, 0, (long)PLANES * klev);
  /* planes 8..10 of BUFFER_LOC are no member's: every byte kept */
  for (int b = 0; b < nb; b++) bad += not_fill(loc + ((size_t)b * PLANES + 8) * plane, 3 * plane, FILL);
  /* the set's separate tendency_loc_* arrays are not the run's */
  for (int m = CLOUDSC_M_tendency_loc_t; m <= CLOUDSC_M_tendency_loc_cld; m++)
    bad += not_fill(((void **)&buf_set)[m], member_bytes(ds, m, nb, nproma, es, 0), FILL);
  free(tmp);
  free(loc);
  free_set(&ref, NULL);
  free_set(&null_set, NULL);
  free_set(&kept_set, NULL);
  free_set(&buf_set, NULL);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("outputs_surface_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++, cases++) bad += run_case(&ds, k_shapes[s][0], k_shapes[s][1], k_precisions[p]);
  cloudsc_io_free(&ds);
  return sanitize_result("outputs_surface_sanitize_driver", cases, bad);
}
