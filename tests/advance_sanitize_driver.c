/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_run_advance and cloudsc_cpu_fields_advance under
 * the host sanitizers, on the data set data/cloudsc100 at the shapes 100 / 16, 300 / 64 (a partial last block each)
 * and 1 / 1, fp64 and mixed.  Every array is an exact-size heap block, so AddressSanitizer sees any access past
 * one; in the fused runs tendency_loc_* and the ten diagnostic flux members are NULL (any access to one is a NULL
 * dereference).  Per case: the fused form (SURFACE) in place; the same out of place into four filled blocks, which
 * must hold the in-place state in the real columns of the seven planes and keep the fill byte in the vapour plane
 * and the padding lanes, the state itself unchanged; cloudsc_cpu_run_outputs(ALL) followed by the separate pass in
 * place, in fp64 the fused state byte for byte; the pass alone in CLOUDSC_FP32 on the float set.  The error paths
 * are called with arguments that must be refused before anything is dereferenced.  Exit status 0 and "clean" on
 * success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/advance_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

static const int k_state[4] = {CLOUDSC_M_pt, CLOUDSC_M_pq, CLOUDSC_M_pa, CLOUDSC_M_pclv};

/* rows of state member i that an advancing step writes: the vapour plane (the fifth of pclv) is left alone */
static long written_rows(int i, int klev) { return i == 3 ? 4L * klev : klev; }

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = nblocks(ngptot, nproma);
  const int flags = SET_NO_DIAG | SET_NO_TEND_LOC | SET_SURFACE;
  cloudsc_fields_t fused, apart, step, pristine;
  long bad = 0;
  make_set(ds, ngptot, nproma, es, flags, FILL, &fused);
  make_set(ds, ngptot, nproma, es, flags, FILL, &apart);
  make_set(ds, ngptot, nproma, es, 0, FILL, &step);
  make_set(ds, ngptot, nproma, es, flags, FILL, &pristine);
  void *dst[4];
  for (int i = 0; i < 4; i++) dst[i] = alloc_filled(member_bytes(ds, k_state[i], nb, nproma, es, 0), FILL);
  const cloudsc_advance_t in_fused = {(void *)fused.pt, (void *)fused.pq, (void *)fused.pa, (void *)fused.pclv};
  const cloudsc_advance_t out = {dst[0], dst[1], dst[2], dst[3]};
  const cloudsc_advance_t in_step = {(void *)step.pt, (void *)step.pq, (void *)step.pa, (void *)step.pclv};
  if (cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &fused, &in_fused))
    bad += FAILED;
  if (cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &apart, &out))
    bad += FAILED;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &step)) bad += FAILED;
  if (cloudsc_cpu_fields_advance(2, precision, ngptot, nproma, klev, &ds->params, &step, &in_step)) bad += FAILED;
  for (int i = 0; i < 4; i++) {
    const int m = k_state[i];
    const long rows = rows_of(kinds[m], klev), wr = written_rows(i, klev);
    const void *f = ((void **)&fused)[m], *a = ((void **)&apart)[m], *s = ((void **)&step)[m], *p = ((void **)&pristine)[m];
    bad += differing_rows(ngptot, nproma, (size_t)es, dst[i], rows, 0, f, rows, 0, wr);     /* out of place == in place */
    bad += padding_written(rows, ngptot, nproma, es, dst[i], FILL);
    bad += memcmp(a, p, member_bytes(ds, m, nb, nproma, es, 0)) != 0;                       /* the state kept */
    if (i == 0) bad += differing_rows(ngptot, nproma, (size_t)es, f, rows, 0, p, rows, 0, wr) == 0;   /* and the step moved pt */
    if (precision == CLOUDSC_FP64) bad += differing_rows(ngptot, nproma, (size_t)es, s, rows, 0, f, rows, 0, wr);
    if (i == 3) {   /* the vapour plane: filled out of place, the input's in place */
      for (int b = 0; b < nb; b++) {
        const size_t off = ((size_t)b * 5 + 4) * klev * nproma * es, n = (size_t)klev * nproma * es;
        bad += not_fill((const char *)dst[i] + off, n, FILL);
        bad += memcmp((const char *)f + off, (const char *)p + off, n) != 0;
        bad += memcmp((const char *)s + off, (const char *)p + off, n) != 0;
      }
    }
  }
  /* the other outputs of the two fused runs are the same bytes, padding lanes filled */
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (dirs[m] == CLOUDSC_FD_OUT && !is_diagnostic(m) && !is_tendency_loc(m)) {
      bad += memcmp(((void **)&fused)[m], ((void **)&apart)[m], member_bytes(ds, m, nb, nproma, es, 1)) != 0;
      bad += padding_written(rows_of(kind_of(m, 1), klev), ngptot, nproma, es, ((void **)&fused)[m], FILL);
    }
  bad += memcmp(fused.plude, apart.plude, member_bytes(ds, CLOUDSC_M_plude, nb, nproma, es, 0)) != 0;
  /* the pass in float arithmetic, on the float set (precision code alone differs) */
  if (precision == CLOUDSC_MIXED &&
      cloudsc_cpu_fields_advance(2, CLOUDSC_FP32, ngptot, nproma, klev, &ds->params, &step, &out))
    bad += FAILED;
  /* refused, not run */
  cloudsc_advance_t w = in_fused;
  w.clv = NULL;
  if (cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &fused, NULL) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &fused, &w) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &fused, &in_fused) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_advance(2, CLOUDSC_FP32, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &fused, &in_fused) != CLOUDSC_EINVAL ||
      cloudsc_cpu_fields_advance(2, precision, ngptot, nproma, klev, &ds->params, &fused, &in_fused) != CLOUDSC_EINVAL ||   /* NULL tendency_loc_* */
      cloudsc_cpu_fields_advance(2, precision, ngptot, nproma, klev, NULL, &step, &in_step) != CLOUDSC_EINVAL)
    bad += FAILED;
  w = in_fused;
  w.t = (void *)fused.pq;      /* another state member */
  if (cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &fused, &w) != CLOUDSC_EINVAL)
    bad += FAILED;
  w = out;
  w.q = w.a;                   /* two members equal */
  if (cloudsc_cpu_run_advance(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &fused, &w) != CLOUDSC_EINVAL ||
      cloudsc_cpu_fields_advance(2, precision, ngptot, nproma, klev, &ds->params, &step, &w) != CLOUDSC_EINVAL)
    bad += FAILED;
  for (int i = 0; i < 4; i++) free(dst[i]);
  free_set(&fused, NULL);
  free_set(&apart, NULL);
  free_set(&step, NULL);
  free_set(&pristine, NULL);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("advance_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++, cases++) bad += run_case(&ds, k_shapes[s][0], k_shapes[s][1], k_precisions[p]);
  cloudsc_io_free(&ds);
  return sanitize_result("advance_sanitize_driver", cases, bad);
}
