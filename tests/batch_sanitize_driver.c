/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for the argument rules of the batched step under the host
 * sanitizers: cloudsc_batch_create, cloudsc_gpu_run_batch, cloudsc_batch_nsets, cloudsc_batch_destroy and
 * cloudsc_batch_launch_geometry with every argument error of include/cloudsc_amd.h, each of which must be
 * CLOUDSC_EINVAL before the first HIP call -- so nothing here reaches a GPU.  Every member of every set is a heap
 * block of ONE byte and the `sets` and `params` arrays are exact-size heap blocks: AddressSanitizer sees a rule
 * that dereferences a member, or reads past the nsets elements it was given (the aliasing check sorts nsets * 48
 * pointers; the largest case has 300 sets).  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   make -C dwarf-p-cloudsc_amd sanitize      (make obj/san/batch_sanitize_driver there: this driver alone) */
#include "sanitize_common.h"

#define NSETS_MAX 300

/* nsets sets of one-byte members: all 48 (aerosol inputs included), or without the five aerosol inputs */
static cloudsc_fields_t *make_sets(int nsets, int aerosols) {
  cloudsc_fields_t *s = (cloudsc_fields_t *)alloc_filled(sizeof(*s) * (size_t)nsets, 0);
  for (int i = 0; i < nsets; i++)
    for (int m = 0; m < CLOUDSC_NFIELDS; m++)
      if (aerosols || dirs[m] != CLOUDSC_FD_AEROSOL) ((void **)&s[i])[m] = alloc_filled(1, FILL);
  return s;
}
static void free_sets(cloudsc_fields_t *s, int nsets) {
  for (int i = 0; i < nsets; i++)
    for (int m = 0; m < CLOUDSC_NFIELDS; m++) free(((void **)&s[i])[m]);
  free(s);
}

static long expect_einval(int rc) { return rc == CLOUDSC_EINVAL ? 0 : FAILED; }

/* cloudsc_batch_create with one thing wrong at a time; `p`: NULL or nsets parameter sets */
static long run_case(const cloudsc_dataset_t *ds, int nsets, int precision, int outputs, int with_params) {
  const int klev = ds->klev, ngptot = 100, nproma = 16;
  long bad = 0;
  cloudsc_batch_t *b = (cloudsc_batch_t *)(uintptr_t)0x10;   /* never written: every call fails first */
  cloudsc_fields_t *s = make_sets(nsets, 0);
  cloudsc_params_t *p = NULL;
  if (with_params) {
    p = (cloudsc_params_t *)alloc_filled(sizeof(*p) * (size_t)nsets, 0);
    for (int i = 0; i < nsets; i++) p[i] = ds->params;
  }
#define CREATE(...) expect_einval(cloudsc_batch_create(__VA_ARGS__))
  bad += CREATE(NULL, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, NULL, p);
  bad += CREATE(&b, 0, precision, outputs, 0, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, -3, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, CLOUDSC_BATCH_MAX_SETS + 1, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, nsets, 0, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, 0, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, 257, klev, s, p);              /* KCACHE's widest block */
  bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, (1 << 24) + 1, klev, s, p);
  bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, 0, s, p);
  bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, 1, s, p);
  bad += CREATE(&b, 0, 99, outputs, nsets, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, 2, nsets, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, 4, nsets, ngptot, nproma, klev, s, p);
  bad += CREATE(&b, 0, precision, -1, nsets, ngptot, nproma, klev, s, p);
  /* a required member NULL in the last set: an input, the in-place plude, a selected output */
  const int required[3] = {CLOUDSC_M_pt, CLOUDSC_M_plude, CLOUDSC_M_pfplsl};
  for (int r = 0; r < 3; r++) {
    void **slot = &((void **)&s[nsets - 1])[required[r]], *keep = *slot;
    *slot = NULL;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    *slot = keep;
  }
  /* a diagnostic flux member is required by CLOUDSC_OUTPUTS_ALL alone */
  if (outputs == CLOUDSC_OUTPUTS_ALL) {
    void *keep = (void *)s[0].pfsqlf;
    s[0].pfsqlf = NULL;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    s[0].pfsqlf = keep;
  }
  /* an aerosol input in one set and not in the others */
  if (nsets > 1) {
    s[nsets - 1].pre_ice = alloc_filled(1, FILL);
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    free((void *)s[nsets - 1].pre_ice);
    s[nsets - 1].pre_ice = NULL;
  }
  /* aliasing: an output of the last set is an input of the first, an output of the first, another member of its
   * own set; plude shared */
  if (nsets > 1) {
    void *keep = (void *)s[nsets - 1].pcovptot;
    s[nsets - 1].pcovptot = (void *)s[0].pt;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    s[nsets - 1].pcovptot = (void *)s[0].pcovptot;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    s[nsets - 1].pcovptot = keep;
    keep = (void *)s[nsets - 1].plude;
    s[nsets - 1].plude = s[0].plude;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    s[nsets - 1].plude = keep;
  }
  {
    void *keep = (void *)s[0].tendency_loc_t;
    s[0].tendency_loc_t = (void *)s[0].pq;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    s[0].tendency_loc_t = (void *)s[0].tendency_loc_q;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    s[0].tendency_loc_t = keep;
  }
  /* the parameter sets: an invalid one, sets that disagree on the aerosol kernels, aerosol kernels without the inputs */
  if (p) {
    p[nsets - 1].ncldtop = 1;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    p[nsets - 1] = ds->params;
    p[nsets - 1].laericeauto = 1;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);   /* (nsets 1: no aerosol members) */
    for (int i = 0; i < nsets; i++) p[i].laericesed = 1;
    bad += CREATE(&b, 0, precision, outputs, nsets, ngptot, nproma, klev, s, p);
    for (int i = 0; i < nsets; i++) p[i] = ds->params;
  }
#undef CREATE
  if (b != (cloudsc_batch_t *)(uintptr_t)0x10) bad += FAILED;   /* a refused call leaves *batch alone */
  free(p);
  free_sets(s, nsets);
  return bad;
}

/* the entries that take a batch: the variant is judged before the batch is looked at (0x10 is no batch) */
static long run_entries(void) {
  cloudsc_batch_t *fake = (cloudsc_batch_t *)(uintptr_t)0x10;
  cloudsc_launch_geometry_t g;
  long bad = 0;
  const int variants[8] = {CLOUDSC_VARIANT_KSEG, CLOUDSC_VARIANT_SCC, CLOUDSC_VARIANT_SCC_PRIVATE, 0, 77,
                           CLOUDSC_VARIANT_KCACHE | CLOUDSC_FP32_EXACT_LIBM, CLOUDSC_VARIANT_KCACHE | 0x1000, -1};
  for (int v = 0; v < 8; v++) bad += expect_einval(cloudsc_gpu_run_batch(fake, NULL, variants[v]));
  bad += expect_einval(cloudsc_gpu_run_batch(NULL, NULL, CLOUDSC_VARIANT_KCACHE));
  bad += expect_einval(cloudsc_batch_nsets(NULL));
  if (cloudsc_batch_destroy(NULL) != CLOUDSC_OK) bad += FAILED;
  bad += expect_einval(cloudsc_batch_launch_geometry(CLOUDSC_FP64, 0, 100, 16, 137, 0, &g));
  bad += expect_einval(cloudsc_batch_launch_geometry(CLOUDSC_FP64, CLOUDSC_BATCH_MAX_SETS + 1, 100, 16, 137, 0, &g));
  bad += expect_einval(cloudsc_batch_launch_geometry(CLOUDSC_FP64, 3, 100, 257, 137, 0, &g));
  bad += expect_einval(cloudsc_batch_launch_geometry(CLOUDSC_FP64, 3, 100, 16, 137, 0, NULL));
  if (cloudsc_batch_launch_geometry(CLOUDSC_FP64, 3, 100, 32, 137, 0, &g) != CLOUDSC_OK || g.workgroups != 12 ||
      g.wg_threads != 32 || g.pack != 1)
    bad += FAILED;
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  long bad = 0;
  int cases = 0;
  const int rc = sanitize_load("batch_sanitize_driver", argc, argv, &ds);
  if (rc) return rc;
  const int nsets[3] = {1, 3, NSETS_MAX};
  const int precisions[3] = {CLOUDSC_FP64, CLOUDSC_FP32, CLOUDSC_MIXED};
  const int outputs[3] = {CLOUDSC_OUTPUTS_ALL, CLOUDSC_OUTPUTS_PROGNOSTIC, CLOUDSC_OUTPUTS_SURFACE};
  for (int n = 0; n < 3; n++)
    for (int q = 0; q < 3; q++)
      for (int w = 0; w < 2; w++, cases++) bad += run_case(&ds, nsets[n], precisions[q], outputs[q], w);
  bad += run_entries();
  cases++;
  cloudsc_io_free(&ds);
  return sanitize_result("batch_sanitize_driver", cases, bad);
}
