/* TEST INFRASTRUCTURE ONLY -- stand-alone driver for the three host twins of the prognostic step and the
 * in-place checks on packed tendency buffers -- cloudsc_cpu_run_tendbuf_outputs,
 * cloudsc_cpu_fields_compare_tendbuf and its 0 / 0 case, which is cloudsc_cpu_fields_compare -- under the
 * host sanitizers, on the data set data/cloudsc100 at the shapes 100 / 16, 300 / 64 and 1 / 1, fp64 and
 * mixed, 8 planes per block in the reference's order and 11 permuted.  Every array and buffer is an
 * exact-size heap block (so AddressSanitizer sees any access past one).  Per case: pack tendency_tmp_* into
 * BUFFER_TMP; run CLOUDSC_OUTPUTS_PROGNOSTIC on the two buffers with the ten diagnostic members NULL, and
 * again with them pointing at arrays of a fill byte that must come back unchanged; compare the eleven kept
 * outputs in place (BUFFER_LOC at its block stride) with cloudsc_cpu_run_precision on separate arrays: 0
 * mismatches, `compared` in the member's own rows; planes no member is bound to and padding lanes must keep
 * their fill byte; one flipped bit in the last real column of BUFFER_LOC is found at its column and row, one
 * in a padding lane is not; then CLOUDSC_OUTPUTS_ALL over all 21, and 0 / 0 planes against
 * cloudsc_cpu_fields_compare record for record.  Exit status 0 and "clean" on success.  No GPU, no Python:
 *
 *   cd dwarf-p-cloudsc_amd
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c ../tests/tendbuf_outputs_sanitize_driver.c -o obj/tbo_driver.o
 *   clang -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I../include -Icsrc \
 *       -c csrc/cloudsc_io.c -o obj/tbo_io.o
 *   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
 *       -Xarch_host -fno-omit-frame-pointer -Xarch_host -mfma -I../include -Icsrc obj/tbo_driver.o obj/tbo_io.o \
 *       csrc/cloudsc_cpu.hip csrc/cloudsc_convert.hip csrc/cloudsc_compare.hip -L. -lcloudsc_amd \
 *       -Wl,-rpath,$PWD -ldl -o obj/tbo_driver && obj/tbo_driver ../data/cloudsc100
 *
 * (clang: the one hipcc drives, so all objects share one sanitizer runtime.  libcloudsc_amd.so only
 * supplies the helpers of other translation units the three files refer to; the code under test is the
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

#define FILL_SEP 0x3C
#define FILL_TMP 0x5A
#define FILL_LOC 0xA5

static int is_int_member(int m) { return m == CLOUDSC_M_ktype; }
static size_t member_bytes(const cloudsc_dataset_t *ds, int m, int nb, int nproma, int es) {
  return (size_t)nb * (size_t)cloudsc_io_elems(kinds[m], ds->klev, nproma) * (is_int_member(m) ? 4 : (size_t)es);
}

/* a field set of exact-size heap blocks: inputs expanded from the data set, outputs filled with a byte */
static int make_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, cloudsc_fields_t *f) {
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
    if (dirs[m] != CLOUDSC_FD_OUT) continue;
    if (!(fp[m] = malloc(member_bytes(ds, m, nb, nproma, es)))) return 1;
    memset(fp[m], FILL_SEP, member_bytes(ds, m, nb, nproma, es));
  }
  return 0;
}
static void free_set(cloudsc_fields_t *f, const cloudsc_fields_t *keep) {
  void **fp = (void **)f;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (!keep || fp[m] != ((void *const *)keep)[m]) free(fp[m]);
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

/* first plane of (t, a, q, cld) of BUFFER_TMP and BUFFER_LOC: the reference's order and the hand-permuted ones */
static const int ref_order[2][4] = {{0, 1, 2, 3}, {0, 1, 2, 3}};
static const int perm8[2][4] = {{6, 7, 5, 0}, {6, 0, 7, 1}}, perm11[2][4] = {{10, 0, 8, 2}, {0, 10, 1, 5}};

/* bytes of a buffer [nb][planes][klev][nproma] that are not `fill` although nothing may write them: planes
 * outside the four members' (first planes p[0..3], cld five wide) and the lanes past the last column */
static long touched_outside(const char *buf, const int p[4], int nb, int planes, int klev, int nproma, int es,
                            int ngptot, int fill) {
  long bad = 0;
  for (int b = 0; b < nb; b++)
    for (int q = 0; q < planes; q++) {
      const int bound = q == p[0] || q == p[1] || q == p[2] || (q >= p[3] && q < p[3] + 5);
      const int cols = bound ? (ngptot - b * nproma < nproma ? ngptot - b * nproma : nproma) : 0;
      for (int k = 0; k < klev; k++) {
        const unsigned char *row = (const unsigned char *)buf + (((size_t)b * planes + q) * klev + k) * nproma * es;
        for (size_t i = (size_t)cols * es; i < (size_t)nproma * es; i++) bad += row[i] != fill;
      }
    }
  return bad;
}

#define FILL_DIAG 0x77

static int is_diag(int m) { return m >= CLOUDSC_M_pfsqlf && m <= CLOUDSC_M_pfsqitur; }
static int is_output(int m) { return dirs[m] == CLOUDSC_FD_OUT || dirs[m] == CLOUDSC_FD_INOUT; }

/* the output members of f (with `all`, the ten diagnostic ones too) */
static cloudsc_fields_t outputs_of(const cloudsc_fields_t *f, int all) {
  cloudsc_fields_t o;
  memset(&o, 0, sizeof(o));
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (is_output(m) && (all || !is_diag(m))) ((void **)&o)[m] = ((void *const *)f)[m];
  return o;
}

/* mismatches of pk (tendencies in the buffers) against ref (separate arrays), in place; a wrong `compared` counts */
static long compare_inplace(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision, int planes,
                            const cloudsc_fields_t *pk, const cloudsc_fields_t *ref, int all,
                            cloudsc_field_diff_t *diff) {
  const cloudsc_fields_t a = outputs_of(pk, all), b = outputs_of(ref, all);
  long bad = 0;
  if (cloudsc_cpu_fields_compare_tendbuf(2, ngptot, ds->klev, precision, nproma, planes, &a, precision, nproma, 0, &b,
                                         diff))
    return 1000000;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    const int want = is_output(m) && (all || !is_diag(m));
    const long rows = (long)cloudsc_io_elems(kinds[m], ds->klev, 1);
    if (diff[m].compared != (want ? rows * ngptot : 0)) bad += 1000000;
    bad += diff[m].mismatches;
  }
  return bad;
}

static long run_case(const cloudsc_dataset_t *ds, int ngptot, int nproma, int precision, int planes, int permuted) {
  const int es = precision == CLOUDSC_FP64 ? 8 : 4, klev = ds->klev, nb = (ngptot + nproma - 1) / nproma;
  const size_t plane = (size_t)klev * nproma * es, buf_bytes = (size_t)nb * planes * plane;
  cloudsc_fields_t sep, ref, pk;
  cloudsc_field_diff_t diff[CLOUDSC_NFIELDS], plain[CLOUDSC_NFIELDS];
  long bad = 0;
  const int (*order)[4] = ref_order;
  if (make_set(ds, ngptot, nproma, es, &sep) || make_set(ds, ngptot, nproma, es, &ref)) return 1000000;
  char *tmp = (char *)malloc(buf_bytes), *loc = (char *)malloc(buf_bytes);
  if (!tmp || !loc) return 1000000;
  memset(tmp, FILL_TMP, buf_bytes);
  memset(loc, FILL_LOC, buf_bytes);
  /* the reference: separate arrays, all 21 outputs */
  if (cloudsc_cpu_run_precision(2, precision, ngptot, nproma, klev, &ds->params, &ref, NULL)) bad += 1000000;
  /* pk: sep's members, the tendencies bound to the buffers */
  pk = sep;
  if (!permuted) {
    if (cloudsc_tendbuf_bind(&pk, precision, nproma, klev, tmp, loc)) bad += 1000000;
  } else {
    const int (*p)[4] = planes == 8 ? perm8 : perm11;
    order = p;
    pk.tendency_tmp_t = tmp + p[0][0] * plane; pk.tendency_tmp_a = tmp + p[0][1] * plane;
    pk.tendency_tmp_q = tmp + p[0][2] * plane; pk.tendency_tmp_cld = tmp + p[0][3] * plane;
    pk.tendency_loc_t = loc + p[1][0] * plane; pk.tendency_loc_a = loc + p[1][1] * plane;
    pk.tendency_loc_q = loc + p[1][2] * plane; pk.tendency_loc_cld = loc + p[1][3] * plane;
  }
  cloudsc_fields_t a, b;
  memset(&a, 0, sizeof(a)); memset(&b, 0, sizeof(b));
  a.tendency_tmp_t = sep.tendency_tmp_t; a.tendency_tmp_a = sep.tendency_tmp_a;
  a.tendency_tmp_q = sep.tendency_tmp_q; a.tendency_tmp_cld = sep.tendency_tmp_cld;
  b.tendency_tmp_t = pk.tendency_tmp_t; b.tendency_tmp_a = pk.tendency_tmp_a;
  b.tendency_tmp_q = pk.tendency_tmp_q; b.tendency_tmp_cld = pk.tendency_tmp_cld;
  if (cloudsc_cpu_fields_convert_tendbuf(2, ngptot, klev, precision, nproma, 0, &a, precision, nproma, planes, &b))
    bad += 1000000;
  /* plude is INOUT: keep the expanded values for the later runs */
  const size_t plude_bytes = member_bytes(ds, CLOUDSC_M_plude, nb, nproma, es);
  void *plude0 = malloc(plude_bytes);
  if (!plude0) return 1000000;
  memcpy(plude0, pk.plude, plude_bytes);

  /* PROGNOSTIC, the ten diagnostic members NULL */
  cloudsc_fields_t nul = pk;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (is_diag(m)) ((void **)&nul)[m] = NULL;
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, planes, &ds->params,
                                      &nul))
    bad += 1000000;
  bad += compare_inplace(ds, ngptot, nproma, precision, planes, &pk, &ref, 0, diff);
  bad += touched_outside(tmp, order[0], nb, planes, klev, nproma, es, ngptot, FILL_TMP);
  bad += touched_outside(loc, order[1], nb, planes, klev, nproma, es, ngptot, FILL_LOC);
  /* one bit in the last real column of tendency_loc_cld (species 2, the last level) is found where it is; one in a
   * padding lane of the same row (where the last block has one) is not */
  {
    const int lb = nb - 1, lane = ngptot - 1 - lb * nproma;
    char *row = (char *)pk.tendency_loc_cld + (((size_t)lb * planes + 2) * klev + (klev - 1)) * nproma * es;
    row[(size_t)lane * es] ^= 1;
    if (lane + 1 < nproma) row[(size_t)(lane + 1) * es] ^= 1;
    const long got = compare_inplace(ds, ngptot, nproma, precision, planes, &pk, &ref, 0, diff);
    const cloudsc_field_diff_t *d = &diff[CLOUDSC_M_tendency_loc_cld];
    if (got != 1 || d->mismatches != 1 || d->first_column != ngptot - 1 || d->first_row != 2L * klev + klev - 1)
      bad += 1000000;
    row[(size_t)lane * es] ^= 1;
    if (lane + 1 < nproma) row[(size_t)(lane + 1) * es] ^= 1;
  }

  /* PROGNOSTIC again, the ten members pointing at arrays of a fill byte that must come back unchanged */
  memcpy(pk.plude, plude0, plude_bytes);
  memset(loc, FILL_LOC, buf_bytes);
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (is_diag(m)) memset(((void **)&pk)[m], FILL_DIAG, member_bytes(ds, m, nb, nproma, es));
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, CLOUDSC_OUTPUTS_PROGNOSTIC, ngptot, nproma, klev, planes, &ds->params,
                                      &pk))
    bad += 1000000;
  bad += compare_inplace(ds, ngptot, nproma, precision, planes, &pk, &ref, 0, diff);
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (is_diag(m)) {
      const unsigned char *p = (const unsigned char *)((void **)&pk)[m];
      for (size_t i = 0; i < member_bytes(ds, m, nb, nproma, es); i++) bad += p[i] != FILL_DIAG;
    }
  bad += touched_outside(loc, order[1], nb, planes, klev, nproma, es, ngptot, FILL_LOC);

  /* ALL: cloudsc_cpu_run_tendbuf, all 21 outputs; with a NULL diagnostic member it is refused */
  memcpy(pk.plude, plude0, plude_bytes);
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, planes, &ds->params, &pk))
    bad += 1000000;
  bad += compare_inplace(ds, ngptot, nproma, precision, planes, &pk, &ref, 1, diff);
  if (cloudsc_cpu_run_tendbuf_outputs(2, precision, CLOUDSC_OUTPUTS_ALL, ngptot, nproma, klev, planes, &ds->params,
                                      &nul) != CLOUDSC_EINVAL)
    bad += 1000000;

  /* 0 and 0 planes is cloudsc_cpu_fields_compare, record for record (one thread: the same grouping of the sums) */
  {
    const cloudsc_fields_t x = outputs_of(&sep, 1), y = outputs_of(&ref, 1);
    memset(diff, 0, sizeof(diff)); memset(plain, 0, sizeof(plain));
    if (cloudsc_cpu_fields_compare_tendbuf(1, ngptot, klev, precision, nproma, 0, &x, precision, nproma, 0, &y, diff) ||
        cloudsc_cpu_fields_compare(1, ngptot, klev, precision, nproma, &x, precision, nproma, &y, plain))
      bad += 1000000;
    for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
      if (diff[m].compared != plain[m].compared || diff[m].mismatches != plain[m].mismatches ||
          diff[m].first_column != plain[m].first_column || diff[m].first_row != plain[m].first_row ||
          memcmp(&diff[m].stats, &plain[m].stats, sizeof(diff[m].stats)))
        bad += 1000000;
    }
    /* sep's separate tendency_loc_* were never the run's: they keep their fill, so they differ from ref's */
    if (!diff[CLOUDSC_M_tendency_loc_t].mismatches && ngptot > 1) bad += 1000000;
  }
  free(plude0);
  free(tmp); free(loc);
  free_set(&sep, NULL);
  free_set(&ref, NULL);
  return bad;
}

int main(int argc, char **argv) {
  cloudsc_dataset_t ds;
  if (cloudsc_io_load_dir(argc > 1 ? argv[1] : "../data/cloudsc100", 0, &ds)) {
    fprintf(stderr, "tendbuf_outputs_sanitize_driver: cannot load the data set: %s\n", cloudsc_io_last_error());
    return 2;
  }
  static const int shapes[3][2] = {{100, 16}, {300, 64}, {1, 1}};
  static const int precisions[2] = {CLOUDSC_FP64, CLOUDSC_MIXED};
  long bad = 0;
  int cases = 0;
  for (int s = 0; s < 3; s++)
    for (int p = 0; p < 2; p++)
      for (int permuted = 0; permuted < 2; permuted++, cases++) {
        const long b = run_case(&ds, shapes[s][0], shapes[s][1], precisions[p], permuted ? 11 : 8, permuted);
        if (b) printf("case %d / %d precision %d planes %d: %ld\n", shapes[s][0], shapes[s][1], precisions[p], permuted ? 11 : 8, b);
        bad += b;
      }
  cloudsc_io_free(&ds);
  printf("tendbuf_outputs_sanitize_driver: %d cases, %ld mismatches: %s\n", cases, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}
