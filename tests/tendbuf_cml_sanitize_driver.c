/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_run_tendbuf_cml and
 * cloudsc_cpu_fields_accumulate_tendbuf under the host sanitizers, on the data set data/cloudsc100 at the
 * shapes 100 / 16, 300 / 64 (partial last blocks) and 1 / 1, fp64 and mixed, PROGNOSTIC and SURFACE, 11 planes.
 * Every array is an exact-size heap block, so AddressSanitizer sees any access past one; tendency_loc_* and the
 * ten diagnostic flux members are NULL in the fused runs (any access to one is a NULL dereference).  Per case:
 * the fused form on a BUFFER_CML pre-filled with small values of both signs; cloudsc_cpu_run_tendbuf_outputs into a
 * BUFFER_LOC followed by the separate pass on a copy of the same BUFFER_CML; in fp64 the two buffers must be
 * equal byte for byte, in mixed equal in the vapour plane, planes 8..10 and the padding lanes (which must all
 * keep their fill byte in both).  The error paths of the three entry points are called with arguments that
 * must be refused before anything is dereferenced.  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/tendbuf_cml_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

#define PLANES 11

/* whether element (block b, plane p, lane l) of a buffer is one the accumulation touches */
static int touched(int b, int p, int l, int ngptot, int nproma) {
  return p < CLOUDSC_TENDBUF_CLD + CLOUDSC_NCLV - 1 && b * nproma + l < ngptot;   /* planes 0..6: T, A, Q, ql..qs */
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision, int outputs) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = nblocks(ngptot, nproma);
  const int surface = outputs == CLOUDSC_OUTPUTS_SURFACE;
  /* the sets: the inputs and the kept outputs that are not tendencies; the diagnostic fluxes and tendency_loc_* NULL */
  const int flags = SET_NO_DIAG | SET_NO_TEND_LOC | (surface ? SET_SURFACE : 0);
  const size_t plane = (size_t)klev * nproma * es, bufb = (size_t)nb * PLANES * plane;
  cloudsc_fields_t fused, step;
  long bad = 0;
  make_set(ds, ngptot, nproma, es, flags, FILL, &fused);
  make_set(ds, ngptot, nproma, es, flags, FILL, &step);
  char *tmp = (char *)alloc_filled(bufb, FILL), *loc = (char *)alloc_filled(bufb, FILL);
  char *cml1 = (char *)alloc_filled(bufb, FILL), *cml2 = (char *)alloc_filled(bufb, FILL);
  pack_tmp(&fused, nb, PLANES, plane, tmp);
  /* the touched elements: small values of both signs */
  for (int b = 0; b < nb; b++)
    for (int p = 0; p < PLANES; p++)
      for (int k = 0; k < klev; k++)
        for (int l = 0; l < nproma; l++) {
          if (!touched(b, p, l, ngptot, nproma)) continue;
          const size_t i = (((size_t)b * PLANES + p) * klev + k) * nproma + l;
          const double v = ((double)((i * 2654435761u) % 2001) - 1000.0) * 9.5367431640625e-13;
          if (es == 8) ((double *)cml1)[i] = v;
          else ((float *)cml1)[i] = (float)v;
        }
  memcpy(cml2, cml1, bufb);
  cloudsc_tend_cml_t c1, c2;
  if (cloudsc_tendbuf_bind_cml(&c1, precision, nproma, klev, cml1) || cloudsc_tendbuf_bind_cml(&c2, precision, nproma, klev, cml2))
    bad += FAILED;
  /* the fused form: tendency_loc_* NULL */
  cloudsc_fields_t g = fused;
  if (cloudsc_tendbuf_bind(&g, precision, nproma, klev, tmp, loc)) bad += FAILED;
  g.tendency_loc_t = g.tendency_loc_q = g.tendency_loc_a = g.tendency_loc_cld = NULL;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &c1)) bad += FAILED;
  bad += not_fill(loc, bufb, FILL);   /* BUFFER_LOC keeps every byte */
  /* the step into BUFFER_LOC, then the separate pass */
  cloudsc_fields_t h = step;
  if (cloudsc_tendbuf_bind(&h, precision, nproma, klev, tmp, loc)) bad += FAILED;
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &h)) bad += FAILED;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, PLANES, &h, PLANES, &c2)) bad += FAILED;
  for (int b = 0; b < nb; b++)
    for (int p = 0; p < PLANES; p++)
      for (int k = 0; k < klev; k++)
        for (int l = 0; l < nproma; l++) {
          const size_t i = ((((size_t)b * PLANES + p) * klev + k) * nproma + l) * es;
          if (!touched(b, p, l, ngptot, nproma)) bad += not_fill(cml1 + i, es, FILL) + not_fill(cml2 + i, es, FILL);
          else if (precision == CLOUDSC_FP64) bad += memcmp(cml1 + i, cml2 + i, es) != 0;
        }
  /* the other kept outputs of the two sets are the same bytes */
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (dirs[m] == CLOUDSC_FD_OUT && !is_diagnostic(m) && !is_tendency_loc(m))
      bad += memcmp(((void **)&fused)[m], ((void **)&step)[m], member_bytes(ds, m, nb, nproma, es, surface)) != 0;
  bad += memcmp(fused.plude, step.plude, (size_t)nb * plane) != 0;
  /* error paths: refused before anything is dereferenced (wild but non-NULL pointers) */
  cloudsc_tend_cml_t w = c1;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, PLANES, &ds->params, &g, &c1) != CLOUDSC_EINVAL) bad += FAILED;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, 7, &ds->params, &g, &c1) != CLOUDSC_EINVAL) bad += FAILED;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, NULL) != CLOUDSC_EINVAL) bad += FAILED;
  w.cld = NULL;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &w) != CLOUDSC_EINVAL) bad += FAILED;
  w = c1;
  w.q = (void *)g.tendency_tmp_q;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &w) != CLOUDSC_EINVAL) bad += FAILED;
  if (cloudsc_cpu_run_tendbuf_cml(2, CLOUDSC_FP32, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &c1) != CLOUDSC_EINVAL) bad += FAILED;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, 7, &h, PLANES, &c2) != CLOUDSC_EINVAL) bad += FAILED;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, PLANES, &g, PLANES, &c2) != CLOUDSC_EINVAL) bad += FAILED;   /* NULL tendency_loc_* */
  w = c2;
  w.t = h.tendency_loc_t;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, PLANES, &h, PLANES, &w) != CLOUDSC_EINVAL) bad += FAILED;
  if (cloudsc_tendbuf_bind_cml(NULL, precision, nproma, klev, cml1) != CLOUDSC_EINVAL) bad += FAILED;
  free(tmp);
  free(loc);
  free(cml1);
  free(cml2);
  free_set(&fused, NULL);
  free_set(&step, NULL);
  return bad;
}

int main(int argc, char **argv) {
  static const int selections[2] = {CLOUDSC_OUTPUTS_PROGNOSTIC, CLOUDSC_OUTPUTS_SURFACE};
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("tendbuf_cml_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++)
      for (int o = 0; o < 2; o++, cases++) bad += run_case(&ds, k_shapes[s][0], k_shapes[s][1], k_precisions[p], selections[o]);
  cloudsc_io_free(&ds);
  return sanitize_result("tendbuf_cml_sanitize_driver", cases, bad);
}
