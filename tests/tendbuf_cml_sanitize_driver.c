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
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/tendbuf_cml_sanitize_driver.c -o obj/cml_driver.o
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c csrc/cloudsc_io.c -o obj/cml_io.o
 *   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -Xarch_host -mfma -I../include -Icsrc obj/cml_driver.o obj/cml_io.o \
 *       csrc/cloudsc_cpu.hip csrc/cloudsc_accumulate.hip -L. -lcloudsc_amd -Wl,-rpath,$PWD -ldl \
 *       -o obj/cml_driver && obj/cml_driver ../data/cloudsc100
 *
 * (clang: the one hipcc drives, so all objects share one sanitizer runtime.  libcloudsc_amd.so only
 * supplies the helpers of other translation units the files refer to; the code under test is the
 * instrumented copy linked into the program.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cloudsc_amd.h"
#include "cloudsc_fields.def"
#include "cloudsc_io.h"

#define DIR_ROW(n, N, k, d, i) CLOUDSC_FD_##d,
#define KIND_ROW(n, N, k, d, i) CLOUDSC_FK_##k,
#define INPUT_FIELD(n, N, k, d, i) CLOUDSC_IF_TEMPLATE_##d([CLOUDSC_T_##n] = CLOUDSC_M_##n, )
static const int kinds[] = {CLOUDSC_FIELDS(KIND_ROW)};
static const int dirs[] = {CLOUDSC_FIELDS(DIR_ROW)};
static const int k_input_field[CLOUDSC_IO_NIN] = {CLOUDSC_FIELDS(INPUT_FIELD)};

#define FILL 0x3C
#define PLANES 11

static int is_diagnostic(int m) { return m >= CLOUDSC_M_pfsqlf && m <= CLOUDSC_M_pfsqitur; }
static int is_surface_flux(int m) { return m >= CLOUDSC_M_pfplsl && m <= CLOUDSC_M_pfhpsn; }
static int is_tend(int m) { return (m >= CLOUDSC_M_tendency_loc_t && m <= CLOUDSC_M_tendency_loc_cld); }

/* the inputs expanded from the data set and the kept outputs that are not tendencies, exact-size heap blocks;
 * the diagnostic fluxes and tendency_loc_* stay NULL */
static int make_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, int surface, cloudsc_fields_t *f) {
  const int nb = (ngptot + nproma - 1) / nproma;
  void **fp = (void **)f;
  memset(f, 0, sizeof(*f));
  for (int i = 0; i < CLOUDSC_IO_NIN; i++) {
    const void *src = i == CLOUDSC_IO_KTYPE ? (const void *)ds->ktype : (const void *)ds->in[i];
    if (!src || i >= CLOUDSC_IO_FIRST_AEROSOL) continue;
    const int m = k_input_field[i], is_int = i == CLOUDSC_IO_KTYPE;
    const size_t bytes = (size_t)nb * (size_t)cloudsc_io_elems(kinds[m], ds->klev, nproma) * (is_int ? 4 : (size_t)es);
    if (!(fp[m] = malloc(bytes))) return 1;
    cloudsc_io_expand(src, cloudsc_io_input_kind[i], is_int, ds->klev, ds->klon, ngptot, nproma, 0, is_int ? 4 : es, fp[m]);
  }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (dirs[m] != CLOUDSC_FD_OUT || is_diagnostic(m) || is_tend(m)) continue;
    const int kind = surface && is_surface_flux(m) ? CLOUDSC_FK_SURFACE : kinds[m];
    const size_t bytes = (size_t)nb * (size_t)cloudsc_io_elems(kind, ds->klev, nproma) * (size_t)es;
    if (!(fp[m] = malloc(bytes))) return 1;
    memset(fp[m], FILL, bytes);
  }
  return 0;
}
static void free_set(cloudsc_fields_t *f) {
  void **fp = (void **)f;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) free(fp[m]);
}

/* BUFFER_TMP from the set's separate tendency_tmp_* arrays, in the reference's plane order */
static void pack_tmp(const cloudsc_fields_t *s, int nb, size_t plane, char *tmp) {
  for (int b = 0; b < nb; b++) {
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_T) * plane, (const char *)s->tendency_tmp_t + b * plane, plane);
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_A) * plane, (const char *)s->tendency_tmp_a + b * plane, plane);
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_Q) * plane, (const char *)s->tendency_tmp_q + b * plane, plane);
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_CLD) * plane,
           (const char *)s->tendency_tmp_cld + (size_t)b * CLOUDSC_NCLV * plane, CLOUDSC_NCLV * plane);
  }
}

/* whether element (block b, plane p, lane l) of a buffer is one the accumulation touches */
static int touched(int b, int p, int l, int ngptot, int nproma) {
  return p < CLOUDSC_TENDBUF_CLD + CLOUDSC_NCLV - 1 && b * nproma + l < ngptot;   /* planes 0..6: T, A, Q, ql..qs */
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision, int outputs) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = (ngptot + nproma - 1) / nproma;
  const int surface = outputs == CLOUDSC_OUTPUTS_SURFACE;
  const size_t plane = (size_t)klev * nproma * es, bufb = (size_t)nb * PLANES * plane;
  cloudsc_fields_t fused, step;
  long bad = 0;
  if (make_set(ds, ngptot, nproma, es, surface, &fused) || make_set(ds, ngptot, nproma, es, surface, &step)) return 1000000;
  char *tmp = (char *)malloc(bufb), *loc = (char *)malloc(bufb), *cml1 = (char *)malloc(bufb), *cml2 = (char *)malloc(bufb);
  if (!tmp || !loc || !cml1 || !cml2) return 1000000;
  memset(tmp, FILL, bufb);
  memset(loc, FILL, bufb);
  memset(cml1, FILL, bufb);
  pack_tmp(&fused, nb, plane, tmp);
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
    bad += 1000000;
  /* the fused form: tendency_loc_* NULL */
  cloudsc_fields_t g = fused;
  if (cloudsc_tendbuf_bind(&g, precision, nproma, klev, tmp, loc)) bad += 1000000;
  g.tendency_loc_t = g.tendency_loc_q = g.tendency_loc_a = g.tendency_loc_cld = NULL;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &c1)) bad += 1000000;
  for (size_t i = 0; i < bufb; i++) bad += ((unsigned char *)loc)[i] != FILL;   /* BUFFER_LOC keeps every byte */
  /* the step into BUFFER_LOC, then the separate pass */
  cloudsc_fields_t h = step;
  if (cloudsc_tendbuf_bind(&h, precision, nproma, klev, tmp, loc)) bad += 1000000;
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &h)) bad += 1000000;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, PLANES, &h, PLANES, &c2)) bad += 1000000;
  for (int b = 0; b < nb; b++)
    for (int p = 0; p < PLANES; p++)
      for (int k = 0; k < klev; k++)
        for (int l = 0; l < nproma; l++) {
          const size_t i = ((((size_t)b * PLANES + p) * klev + k) * nproma + l) * es;
          if (!touched(b, p, l, ngptot, nproma)) {
            for (int q = 0; q < es; q++) bad += ((unsigned char *)cml1)[i + q] != FILL || ((unsigned char *)cml2)[i + q] != FILL;
          } else if (precision == CLOUDSC_FP64) {
            bad += memcmp(cml1 + i, cml2 + i, es) != 0;
          }
        }
  /* the other kept outputs of the two sets are the same bytes */
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (dirs[m] != CLOUDSC_FD_OUT || is_diagnostic(m) || is_tend(m)) continue;
    const int kind = surface && is_surface_flux(m) ? CLOUDSC_FK_SURFACE : kinds[m];
    bad += memcmp(((void **)&fused)[m], ((void **)&step)[m], (size_t)nb * (size_t)cloudsc_io_elems(kind, klev, nproma) * es) != 0;
  }
  bad += memcmp(fused.plude, step.plude, (size_t)nb * plane) != 0;
  /* error paths: refused before anything is dereferenced (wild but non-NULL pointers) */
  cloudsc_tend_cml_t w = c1;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, PLANES, &ds->params, &g, &c1) != CLOUDSC_EINVAL) bad += 1000000;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, 7, &ds->params, &g, &c1) != CLOUDSC_EINVAL) bad += 1000000;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, NULL) != CLOUDSC_EINVAL) bad += 1000000;
  w.cld = NULL;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &w) != CLOUDSC_EINVAL) bad += 1000000;
  w = c1;
  w.q = (void *)g.tendency_tmp_q;
  if (cloudsc_cpu_run_tendbuf_cml(2, precision, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &w) != CLOUDSC_EINVAL) bad += 1000000;
  if (cloudsc_cpu_run_tendbuf_cml(2, CLOUDSC_FP32, outputs, ngptot, nproma, klev, PLANES, &ds->params, &g, &c1) != CLOUDSC_EINVAL) bad += 1000000;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, 7, &h, PLANES, &c2) != CLOUDSC_EINVAL) bad += 1000000;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, PLANES, &g, PLANES, &c2) != CLOUDSC_EINVAL) bad += 1000000;   /* NULL tendency_loc_* */
  w = c2;
  w.t = h.tendency_loc_t;
  if (cloudsc_cpu_fields_accumulate_tendbuf(2, precision, ngptot, nproma, klev, PLANES, &h, PLANES, &w) != CLOUDSC_EINVAL) bad += 1000000;
  if (cloudsc_tendbuf_bind_cml(NULL, precision, nproma, klev, cml1) != CLOUDSC_EINVAL) bad += 1000000;
  free(tmp);
  free(loc);
  free(cml1);
  free(cml2);
  free_set(&fused);
  free_set(&step);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  if (cloudsc_io_load_dir(argc > 1 ? argv[1] : "../data/cloudsc100", 0, &ds)) {
    fprintf(stderr, "tendbuf_cml_sanitize_driver: cannot load the data set: %s\n", cloudsc_io_last_error());
    return 2;
  }
  static const int shapes[3][2] = {{100, 16}, {300, 64}, {1, 1}};
  static const int precisions[2] = {CLOUDSC_FP64, CLOUDSC_MIXED};
  static const int selections[2] = {CLOUDSC_OUTPUTS_PROGNOSTIC, CLOUDSC_OUTPUTS_SURFACE};
  long bad = 0;
  int cases = 0;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++)
      for (int o = 0; o < 2; o++, cases++) bad += run_case(&ds, shapes[s][0], shapes[s][1], precisions[p], selections[o]);
  cloudsc_io_free(&ds);
  printf("tendbuf_cml_sanitize_driver: %d cases, %ld mismatches: %s\n", cases, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
