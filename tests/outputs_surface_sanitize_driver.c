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
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/outputs_surface_sanitize_driver.c -o obj/surf_driver.o
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c csrc/cloudsc_io.c -o obj/surf_io.o
 *   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -Xarch_host -mfma -I../include -Icsrc obj/surf_driver.o obj/surf_io.o \
 *       csrc/cloudsc_cpu.hip -L. -lcloudsc_amd -Wl,-rpath,$PWD -ldl -o obj/surf_driver && \
 *       obj/surf_driver ../data/cloudsc100
 *
 * (clang: the one hipcc drives, so all objects share one sanitizer runtime.  libcloudsc_amd.so only
 * supplies the helpers of other translation units the file refers to; the code under test is the
 * instrumented copy linked into the program.) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cloudsc_amd.h"
#include "cloudsc_fields.def"
#include "cloudsc_io.h"

#define KIND_ROW(n, N, k, d, i) CLOUDSC_FK_##k,
#define DIR_ROW(n, N, k, d, i) CLOUDSC_FD_##d,
#define INPUT_FIELD(n, N, k, d, i) CLOUDSC_IF_TEMPLATE_##d([CLOUDSC_T_##n] = CLOUDSC_M_##n, )
static const int kinds[] = {CLOUDSC_FIELDS(KIND_ROW)};
static const int dirs[] = {CLOUDSC_FIELDS(DIR_ROW)};
static const int k_input_field[CLOUDSC_IO_NIN] = {CLOUDSC_FIELDS(INPUT_FIELD)};

#define FILL 0x3C
#define PLANES 11

static int is_int_member(int m) { return m == CLOUDSC_M_ktype; }
static int is_diagnostic(int m) { return m >= CLOUDSC_M_pfsqlf && m <= CLOUDSC_M_pfsqitur; }
static int is_surface_flux(int m) { return m >= CLOUDSC_M_pfplsl && m <= CLOUDSC_M_pfhpsn; }
static int is_output(int m) { return dirs[m] == CLOUDSC_FD_OUT || dirs[m] == CLOUDSC_FD_INOUT; }
static int is_tend_loc(int m) { return m >= CLOUDSC_M_tendency_loc_t && m <= CLOUDSC_M_tendency_loc_cld; }
/* the shape kind of member m in a set: `surface` sets hold the four flux members as surface fields */
static int kind_of(int m, int surface) { return surface && is_surface_flux(m) ? CLOUDSC_FK_SURFACE : kinds[m]; }
static size_t member_bytes(const cloudsc_dataset_t *ds, int m, int nb, int nproma, int es, int surface) {
  return (size_t)nb * (size_t)cloudsc_io_elems(kind_of(m, surface), ds->klev, nproma) *
         (is_int_member(m) ? 4 : (size_t)es);
}

/* a field set of exact-size heap blocks: inputs expanded from the data set, outputs filled with a byte;
 * surface: the four flux members are surface fields; without_diag: the ten diagnostic flux members stay NULL */
static int make_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, int surface, int without_diag,
                    cloudsc_fields_t *f) {
  const int nb = (ngptot + nproma - 1) / nproma;
  void **fp = (void **)f;
  memset(f, 0, sizeof(*f));
  for (int i = 0; i < CLOUDSC_IO_NIN; i++) {
    const void *src = i == CLOUDSC_IO_KTYPE ? (const void *)ds->ktype : (const void *)ds->in[i];
    if (!src || i >= CLOUDSC_IO_FIRST_AEROSOL) continue;
    const int m = k_input_field[i];
    if (!(fp[m] = malloc(member_bytes(ds, m, nb, nproma, es, 0)))) return 1;
    cloudsc_io_expand(src, cloudsc_io_input_kind[i], i == CLOUDSC_IO_KTYPE, ds->klev, ds->klon, ngptot, nproma, 0,
                      i == CLOUDSC_IO_KTYPE ? 4 : es, fp[m]);
  }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (dirs[m] != CLOUDSC_FD_OUT || (without_diag && is_diagnostic(m))) continue;
    const size_t bytes = member_bytes(ds, m, nb, nproma, es, surface);
    if (!(fp[m] = malloc(bytes))) return 1;
    memset(fp[m], FILL, bytes);
  }
  return 0;
}
static void free_set(cloudsc_fields_t *f) {
  void **fp = (void **)f;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) free(fp[m]);
}

/* elements of the real columns that differ: rows [row_a, row_a + nrows) of a (arows rows per block, abrows rows
 * between blocks) against rows [row_b, ...) of b */
static long differing(int ngptot, int nproma, size_t e, const void *a, long arows, long abrows, long row_a,
                      const void *b, long brows, long row_b, long nrows) {
  long bad = 0;
  (void)arows;
  for (long g = 0; g < ngptot; g++)
    for (long r = 0; r < nrows; r++) {
      const size_t i = (size_t)((g / nproma * abrows + row_a + r) * nproma + g % nproma) * e;
      const size_t j = (size_t)((g / nproma * brows + row_b + r) * nproma + g % nproma) * e;
      bad += memcmp((const char *)a + i, (const char *)b + j, e) != 0;
    }
  return bad;
}
/* bytes of the padding lanes of the last block of a member of `rows` rows that are no longer the fill byte */
static long padding_written(long rows, int ngptot, int nproma, int es, const void *a) {
  const int nb = (ngptot + nproma - 1) / nproma, tail = ngptot - (nb - 1) * nproma;
  long bad = 0;
  for (long r = 0; r < rows; r++) {
    const unsigned char *row = (const unsigned char *)a + (size_t)(((long)(nb - 1) * rows + r) * nproma) * es;
    for (size_t i = (size_t)tail * es; i < (size_t)nproma * es; i++) bad += row[i] != FILL;
  }
  return bad;
}
static long not_fill(const void *a, size_t n) {
  long bad = 0;
  for (size_t i = 0; i < n; i++) bad += ((const unsigned char *)a)[i] != FILL;
  return bad;
}

/* the outputs of a SURFACE set s against the full step's set ref; loc_rows: rows between the blocks of the
 * tendency_loc_* members of s (their own rows: separate arrays) */
static long check_surface_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, const cloudsc_fields_t *s,
                              const cloudsc_fields_t *ref, int with_diag, long loc_brows) {
  const int klev = ds->klev, nb = (ngptot + nproma - 1) / nproma;
  long bad = 0;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (!is_output(m)) continue;
    const void *a = ((void *const *)s)[m], *r = ((void *const *)ref)[m];
    const long rows = (long)cloudsc_io_elems(kinds[m], klev, 1);
    if (is_diagnostic(m)) {
      if (!with_diag) bad += a ? 1000000 : 0;
      else bad += not_fill(a, member_bytes(ds, m, nb, nproma, es, 0));   /* every byte kept */
    } else if (is_surface_flux(m)) {   /* one row against row klev of the profile */
      bad += differing(ngptot, nproma, (size_t)es, a, 1, 1, 0, r, rows, klev, 1);
      bad += padding_written(1, ngptot, nproma, es, a);
    } else {
      const long brows = loc_brows && is_tend_loc(m) ? loc_brows : rows;
      bad += differing(ngptot, nproma, (size_t)es, a, rows, brows, 0, r, rows, 0, rows);
      if (dirs[m] == CLOUDSC_FD_OUT && brows == rows) bad += padding_written(rows, ngptot, nproma, es, a);
    }
  }
  return bad;
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = (ngptot + nproma - 1) / nproma;
  cloudsc_fields_t ref, null_set, kept_set, buf_set;
  long bad = 0;
  if (make_set(ds, ngptot, nproma, es, 0, 0, &ref) || make_set(ds, ngptot, nproma, es, 1, 1, &null_set) ||
      make_set(ds, ngptot, nproma, es, 1, 0, &kept_set) || make_set(ds, ngptot, nproma, es, 1, 1, &buf_set))
    return 1000000;
  if (cloudsc_cpu_run_precision(2, precision, ngptot, nproma, klev, &ds->params, &ref, NULL)) bad += 1000000;
  /* the surface bit alone is not a selection */
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE_BIT, ngptot, nproma, klev, &ds->params,
                              &null_set) != CLOUDSC_EINVAL)
    bad += 1000000;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &null_set))
    bad += 1000000;
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &kept_set))
    bad += 1000000;
  bad += check_surface_set(ds, ngptot, nproma, es, &null_set, &ref, 0, 0);
  bad += check_surface_set(ds, ngptot, nproma, es, &kept_set, &ref, 1, 0);
  /* the packed tendency buffers: exact-size blocks too, BUFFER_TMP filled from the set's separate arrays */
  const size_t plane = (size_t)klev * nproma * es, bufb = (size_t)nb * PLANES * plane;
  char *tmp = (char *)malloc(bufb), *loc = (char *)malloc(bufb);
  if (!tmp || !loc) return 1000000;
  memset(tmp, FILL, bufb);
  memset(loc, FILL, bufb);
  cloudsc_fields_t g = buf_set;
  if (cloudsc_tendbuf_bind(&g, precision, nproma, klev, tmp, loc)) bad += 1000000;
  for (int b = 0; b < nb; b++) {
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_T) * plane, (const char *)buf_set.tendency_tmp_t + b * plane, plane);
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_A) * plane, (const char *)buf_set.tendency_tmp_a + b * plane, plane);
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_Q) * plane, (const char *)buf_set.tendency_tmp_q + b * plane, plane);
    memcpy(tmp + ((size_t)b * PLANES + CLOUDSC_TENDBUF_CLD) * plane,
           (const char *)buf_set.tendency_tmp_cld + (size_t)b * CLOUDSC_NCLV * plane, CLOUDSC_NCLV * plane);
  }
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, PLANES, &ds->params,
                                      &g))
    bad += 1000000;
  bad += check_surface_set(ds, ngptot, nproma, es, &g, &ref, 0, (long)PLANES * klev);
  /* planes 8..10 of BUFFER_LOC are no member's: every byte kept */
  for (int b = 0; b < nb; b++) bad += not_fill(loc + ((size_t)b * PLANES + 8) * plane, 3 * plane);
  /* the set's separate tendency_loc_* arrays are not the run's */
  for (int m = CLOUDSC_M_tendency_loc_t; m <= CLOUDSC_M_tendency_loc_cld; m++)
    bad += not_fill(((void **)&buf_set)[m], member_bytes(ds, m, nb, nproma, es, 0));
  free(tmp);
  free(loc);
  free_set(&ref);
  free_set(&null_set);
  free_set(&kept_set);
  free_set(&buf_set);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  if (cloudsc_io_load_dir(argc > 1 ? argv[1] : "../data/cloudsc100", 0, &ds)) {
    fprintf(stderr, "outputs_surface_sanitize_driver: cannot load the data set: %s\n", cloudsc_io_last_error());
    return 2;
  }
  static const int shapes[3][2] = {{100, 16}, {300, 64}, {1, 1}};
  static const int precisions[2] = {CLOUDSC_FP64, CLOUDSC_MIXED};
  long bad = 0;
  int cases = 0;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++, cases++) bad += run_case(&ds, shapes[s][0], shapes[s][1], precisions[p]);
  cloudsc_io_free(&ds);
  printf("outputs_surface_sanitize_driver: %d cases, %ld mismatches: %s\n", cases, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
