/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for cloudsc_cpu_run_tendbuf and
 * cloudsc_cpu_fields_convert_tendbuf under the host sanitizers, on the data set data/cloudsc100 at the
 * shapes 100 / 16 and 300 / 64, fp64 and mixed, 8 and 11 planes per block.  Every array and buffer is an
 * exact-size heap block (so AddressSanitizer sees any access past one).  Per case: pack the separate
 * tendency_tmp_* arrays into BUFFER_TMP, run the step on the two buffers, unpack BUFFER_LOC, and compare
 * every output with cloudsc_cpu_run_precision on the separate arrays, byte for byte over the real
 * columns; planes no member is bound to and padding lanes must keep their fill byte.  Exit status 0 and
 * "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/tendbuf_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision, int planes, int permuted) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = nblocks(ngptot, nproma);
  const size_t buf_bytes = (size_t)nb * planes * klev * nproma * es;
  cloudsc_fields_t sep, ref, pk;
  long bad = 0;
  make_set(ds, ngptot, nproma, es, 0, FILL, &sep);
  make_set(ds, ngptot, nproma, es, 0, FILL, &ref);
  char *tmp = (char *)alloc_filled(buf_bytes, FILL_TMP), *loc = (char *)alloc_filled(buf_bytes, FILL_LOC);
  /* the reference: separate arrays */
  if (cloudsc_cpu_run_precision(2, precision, ngptot, nproma, klev, &ds->params, &ref, NULL)) bad += FAILED;
  /* pk: sep's members, the tendencies bound to the buffers */
  pk = sep;
  plane_order_t *order = bind_planes(&pk, precision, nproma, klev, planes, permuted, tmp, loc, &bad);
  /* pack tendency_tmp_* (sep -> BUFFER_TMP), run on the buffers, unpack BUFFER_LOC (-> sep's arrays) */
  cloudsc_fields_t a = tendencies_of(&sep, 0), b = tendencies_of(&pk, 0);
  if (cloudsc_cpu_fields_convert_tendbuf(2, ngptot, klev, precision, nproma, 0, &a, precision, nproma, planes, &b))
    bad += FAILED;
  if (cloudsc_cpu_run_tendbuf(2, precision, ngptot, nproma, klev, planes, &ds->params, &pk)) bad += FAILED;
  a = tendencies_of(&pk, 1);
  b = tendencies_of(&sep, 1);
  if (cloudsc_cpu_fields_convert_tendbuf(2, ngptot, klev, precision, nproma, planes, &a, precision, nproma, 0, &b))
    bad += FAILED;
  /* every output now in sep's separate arrays */
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (is_output(m)) bad += differing(ds, m, ngptot, nproma, es, ((void **)&sep)[m], ((void **)&ref)[m]);
  /* both buffers: only the bound planes written, and of those only the real columns; and something written */
  bad += touched_outside(tmp, order[0], nb, planes, klev, nproma, es, ngptot, FILL_TMP);
  bad += touched_outside(loc, order[1], nb, planes, klev, nproma, es, ngptot, FILL_LOC);
  if (!not_fill(loc, buf_bytes, FILL_LOC)) bad += FAILED;
  free(tmp);
  free(loc);
  free_set(&sep, NULL);
  free_set(&ref, NULL);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("tendbuf_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  for (int s = 0; s < 2; s++)
    for (int p = 0; p < 2; p++)
      for (int planes = 8; planes <= 11; planes += 3)
        for (int permuted = 0; permuted < 2; permuted++, cases++)
          bad += run_case(&ds, k_shapes[s][0], k_shapes[s][1], k_precisions[p], planes, permuted);
  cloudsc_io_free(&ds);
  return sanitize_result("tendbuf_sanitize_driver", cases, bad);
}
