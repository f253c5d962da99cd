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
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/spp_sanitize_driver.c -o obj/spp_driver.o
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c csrc/cloudsc_io.c -o obj/spp_io.o
 *   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -Xarch_host -mfma -I../include -Icsrc obj/spp_driver.o obj/spp_io.o \
 *       csrc/cloudsc_cpu.hip -L. -lcloudsc_amd -Wl,-rpath,$PWD -ldl -o obj/spp_driver && \
 *       obj/spp_driver ../data/cloudsc100
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

static int is_int_member(int m) { return m == CLOUDSC_M_ktype; }
static int is_diagnostic(int m) { return m >= CLOUDSC_M_pfsqlf && m <= CLOUDSC_M_pfsqitur; }
static int is_output(int m) { return dirs[m] == CLOUDSC_FD_OUT || dirs[m] == CLOUDSC_FD_INOUT; }
static size_t member_bytes(const cloudsc_dataset_t *ds, int m, int nb, int nproma, int es) {
  return (size_t)nb * (size_t)cloudsc_io_elems(kinds[m], ds->klev, nproma) * (is_int_member(m) ? 4 : (size_t)es);
}

/* a field set of exact-size heap blocks: inputs expanded from the data set, outputs filled with a byte;
 * without_diag: the ten diagnostic flux members stay NULL */
static int make_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, int without_diag,
                    cloudsc_fields_t *f) {
  const int nb = (ngptot + nproma - 1) / nproma;
  void **fp = (void **)f;
  memset(f, 0, sizeof(*f));
  for (int i = 0; i < CLOUDSC_IO_NIN; i++) {
    const void *src = i == CLOUDSC_IO_KTYPE ? (const void *)ds->ktype : (const void *)ds->in[i];
    if (!src || i >= CLOUDSC_IO_FIRST_AEROSOL) continue;
    const int m = k_input_field[i];
    if (!(fp[m] = malloc(member_bytes(ds, m, nb, nproma, es)))) return 1;
    cloudsc_io_expand(src, cloudsc_io_input_kind[i], i == CLOUDSC_IO_KTYPE, ds->klev, ds->klon, ngptot, nproma, 0,
                      i == CLOUDSC_IO_KTYPE ? 4 : es, fp[m]);
  }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (dirs[m] != CLOUDSC_FD_OUT || (without_diag && is_diagnostic(m))) continue;
    if (!(fp[m] = malloc(member_bytes(ds, m, nb, nproma, es)))) return 1;
    memset(fp[m], FILL, member_bytes(ds, m, nb, nproma, es));
  }
  return 0;
}
static void free_set(cloudsc_fields_t *f) {
  void **fp = (void **)f;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) free(fp[m]);
}

/* bytes of the real columns of member m that differ between two block-layout arrays */
static long differing(const cloudsc_dataset_t *ds, int m, int ngptot, int nproma, int es, const void *a,
                      const void *b) {
  const long rows = (long)cloudsc_io_elems(kinds[m], ds->klev, 1);
  const size_t e = is_int_member(m) ? 4 : (size_t)es;
  long bad = 0;
  for (long g = 0; g < ngptot; g++)
    for (long r = 0; r < rows; r++) {
      const size_t i = (size_t)((g / nproma * rows + r) * nproma + g % nproma) * e;
      bad += memcmp((const char *)a + i, (const char *)b + i, e) != 0;
    }
  return bad;
}
/* bytes of the padding lanes of the last block of an OUT member that are no longer the fill byte */
static long padding_written(const cloudsc_dataset_t *ds, int m, int ngptot, int nproma, int es, const void *a) {
  const int nb = (ngptot + nproma - 1) / nproma, tail = ngptot - (nb - 1) * nproma;
  const long rows = (long)cloudsc_io_elems(kinds[m], ds->klev, 1);
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

/* a multiplier field of exactly ngptot elements (block layout up to the last real column): column g holds
 * tuples[(7 g + g / 16) % 4][slot], or 1 */
static const double k_tuples[4][5] = {{1, 1, 1, 1, 1},
                                      {0.7531, 1.2519, 0.5017, 1.2483, 0.7469},
                                      {1.1203, 0.7487, 1.4989, 0.7523, 1.2511},
                                      {1.0, 1.2519, 1.0, 0.7523, 1.0}};
static void *make_mult(int ngptot, int es, int slot, int ones) {
  void *p = malloc((size_t)ngptot * (size_t)es);
  for (int g = 0; p && g < ngptot; g++) {
    const double x = ones ? 1.0 : k_tuples[(7 * g + g / 16) % 4][slot];
    if (es == 8) ((double *)p)[g] = x;
    else ((float *)p)[g] = (float)x;
  }
  return p;
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = (ngptot + nproma - 1) / nproma;
  cloudsc_fields_t ref, ones_set, null_set, kept_set;
  long bad = 0;
  if (make_set(ds, ngptot, nproma, es, 0, &ref) || make_set(ds, ngptot, nproma, es, 0, &ones_set) ||
      make_set(ds, ngptot, nproma, es, 1, &null_set) || make_set(ds, ngptot, nproma, es, 0, &kept_set))
    return 1000000;
  void *one[5], *mix[5];
  for (int s = 0; s < 5; s++) {
    one[s] = make_mult(ngptot, es, s, 1);
    mix[s] = make_mult(ngptot, es, s, 0);
    if (!one[s] || !mix[s]) return 1000000;
  }
  const cloudsc_spp_t all_ones = {one[0], one[1], one[2], one[3], one[4]};
  const cloudsc_spp_t some = {mix[0], NULL, mix[2], mix[3], NULL};           /* rcldiff, rpecons: not perturbed */
  const cloudsc_spp_t some_ones = {mix[0], one[1], mix[2], mix[3], one[4]};  /* the same, said with ones */
  const cloudsc_spp_t none = {NULL, NULL, NULL, NULL, NULL};
  if (cloudsc_cpu_run_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref)) bad += 1000000;
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ones_set, &all_ones))
    bad += 1000000;
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &null_set, &some))
    bad += 1000000;
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, &ds->params, &kept_set,
                          &some_ones))
    bad += 1000000;
  /* refused, not run: no spp, no member, a member that is a field of the set, the surface selection */
  const cloudsc_spp_t alias = {mix[0], NULL, ref.plsm, NULL, NULL};
  if (cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref, NULL) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref, &none) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, &ds->params, &ref, &alias) != CLOUDSC_EINVAL ||
      cloudsc_cpu_run_spp(2, precision, CLOUDSC_OUTPUTS_SURFACE, ngptot, nproma, klev, &ds->params, &ref, &some) != CLOUDSC_EINVAL)
    bad += 1000000;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (!is_output(m)) continue;
    void *r = ((void **)&ref)[m], *o = ((void **)&ones_set)[m], *n = ((void **)&null_set)[m],
         *k = ((void **)&kept_set)[m];
    bad += differing(ds, m, ngptot, nproma, es, o, r);
    if (dirs[m] == CLOUDSC_FD_OUT) bad += padding_written(ds, m, ngptot, nproma, es, o);
    if (is_diagnostic(m)) {
      if (n) bad += 1000000;
      bad += not_fill(k, member_bytes(ds, m, nb, nproma, es));   /* every byte kept */
    } else {
      bad += differing(ds, m, ngptot, nproma, es, n, k);
      if (dirs[m] == CLOUDSC_FD_OUT)
        bad += padding_written(ds, m, ngptot, nproma, es, n) + padding_written(ds, m, ngptot, nproma, es, k);
    }
  }
  for (int s = 0; s < 5; s++) { free(one[s]); free(mix[s]); }
  free_set(&ref);
  free_set(&ones_set);
  free_set(&null_set);
  free_set(&kept_set);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  if (cloudsc_io_load_dir(argc > 1 ? argv[1] : "../data/cloudsc100", 0, &ds)) {
    fprintf(stderr, "spp_sanitize_driver: cannot load the data set: %s\n", cloudsc_io_last_error());
    return 2;
  }
  static const int shapes[3][2] = {{100, 16}, {300, 64}, {1, 1}};
  static const int precisions[2] = {CLOUDSC_FP64, CLOUDSC_MIXED};
  long bad = 0;
  int cases = 0;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++, cases++) bad += run_case(&ds, shapes[s][0], shapes[s][1], precisions[p]);
  cloudsc_io_free(&ds);
  printf("spp_sanitize_driver: %d cases, %ld mismatches: %s\n", cases, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
