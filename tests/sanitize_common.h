/* TEST INFRASTRUCTURE ONLY -- what the stand-alone host-sanitizer drivers (tests/<name>_sanitize_driver.c) share:
 * the field tables, exact-size heap field sets, the byte comparisons and fill checks, the packed tendency
 * buffers' helpers, the field-set walkers' fill and check, and the beginning and end of every main.  A driver
 * keeps its run_case, its case table and the comment that says what it checks.  Every block is an exact-size
 * heap block, so AddressSanitizer sees any access past one.  The drivers are built and run, on the CPU only, by
 *   make -C dwarf-p-cloudsc_amd sanitize */
#ifndef SANITIZE_COMMON_H
#define SANITIZE_COMMON_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cloudsc_amd.h"
#include "cloudsc_fields.def"
#include "cloudsc_io.h"

#define KIND_ROW(n, N, k, d, i) CLOUDSC_FK_##k,
#define DIR_ROW(n, N, k, d, i) CLOUDSC_FD_##d,
#define INT_ROW(n, N, k, d, i) i,
#define INPUT_FIELD(n, N, k, d, i) CLOUDSC_IF_TEMPLATE_##d([CLOUDSC_T_##n] = CLOUDSC_M_##n, )
static const int kinds[] = {CLOUDSC_FIELDS(KIND_ROW)};
static const int dirs[] = {CLOUDSC_FIELDS(DIR_ROW)};
static const int is_int[] = {CLOUDSC_FIELDS(INT_ROW)};
static const int k_input_field[CLOUDSC_IO_NIN] = {CLOUDSC_FIELDS(INPUT_FIELD)};

#define FILL 0x3C        /* the outputs of a set from make_set, before a run */
#define FILL_TMP 0x5A    /* BUFFER_TMP */
#define FILL_LOC 0xA5    /* BUFFER_LOC */
#define FAILED 1000000   /* added to a case's mismatches by a call that failed or was not refused */

static inline int is_int_member(int m) { return is_int[m]; }
static inline int is_diagnostic(int m) { return m >= CLOUDSC_M_pfsqlf && m <= CLOUDSC_M_pfsqitur; }
static inline int is_surface_flux(int m) { return m >= CLOUDSC_M_pfplsl && m <= CLOUDSC_M_pfhpsn; }
static inline int is_output(int m) { return dirs[m] == CLOUDSC_FD_OUT || dirs[m] == CLOUDSC_FD_INOUT; }
static inline int is_tendency_loc(int m) { return m >= CLOUDSC_M_tendency_loc_t && m <= CLOUDSC_M_tendency_loc_cld; }
/* the shape kind of member m in a set: `surface` sets hold the four flux members as surface fields */
static inline int kind_of(int m, int surface) { return surface && is_surface_flux(m) ? CLOUDSC_FK_SURFACE : kinds[m]; }
static inline long rows_of(int kind, int klev) {
  return kind == CLOUDSC_FK_LEVEL ? klev : kind == CLOUDSC_FK_HALF ? klev + 1 : kind == CLOUDSC_FK_SPECIES ? 5L * klev : 1;
}
static inline int nblocks(int ngptot, int nproma) { return (ngptot + nproma - 1) / nproma; }
static inline size_t esize(int m, int precision) { return is_int[m] ? 4 : precision == CLOUDSC_FP64 ? 8 : 4; }
static inline size_t member_bytes(const cloudsc_dataset_t *ds, int m, int nb, int nproma, int es, int surface) {
  return (size_t)nb * (size_t)rows_of(kind_of(m, surface), ds->klev) * (size_t)nproma * (is_int[m] ? 4 : (size_t)es);
}

/* an exact-size heap block, every byte `byte`; no memory ends the program (nothing to free on the way out) */
static inline void *alloc_filled(size_t n, int byte) {
  void *p = malloc(n);
  if (!p) {
    fprintf(stderr, "sanitize driver: out of memory\n");
    exit(2);
  }
  return memset(p, byte, n);
}

/* make_set flags */
enum {
  SET_NO_DIAG = 1,      /* the ten diagnostic flux members stay NULL */
  SET_NO_TEND_LOC = 2,  /* tendency_loc_* stay NULL */
  SET_SURFACE = 4       /* the four surface flux members are surface fields: nblocks * nproma elements */
};
/* a field set of exact-size heap blocks: inputs expanded from the data set, outputs filled with `fill` */
static inline void make_set(const cloudsc_dataset_t *ds, int ngptot, int nproma, int es, int flags, int fill,
                            cloudsc_fields_t *f) {
  const int nb = nblocks(ngptot, nproma);
  void **fp = (void **)f;
  memset(f, 0, sizeof(*f));
  for (int i = 0; i < CLOUDSC_IO_NIN; i++) {
    const void *src = i == CLOUDSC_IO_KTYPE ? (const void *)ds->ktype : (const void *)ds->in[i];
    if (!src || i >= CLOUDSC_IO_FIRST_AEROSOL) continue;
    const int m = k_input_field[i];
    fp[m] = alloc_filled(member_bytes(ds, m, nb, nproma, es, 0), 0);
    cloudsc_io_expand(src, cloudsc_io_input_kind[i], is_int[m], ds->klev, ds->klon, ngptot, nproma, 0,
                      is_int[m] ? 4 : es, fp[m]);
  }
  for (int m = 0; m < CLOUDSC_NFIELDS; m++) {
    if (dirs[m] != CLOUDSC_FD_OUT || ((flags & SET_NO_DIAG) && is_diagnostic(m)) ||
        ((flags & SET_NO_TEND_LOC) && is_tendency_loc(m)))
      continue;
    fp[m] = alloc_filled(member_bytes(ds, m, nb, nproma, es, flags & SET_SURFACE), fill);
  }
}
/* keep: a set whose members are not f's to free (NULL: none) */
static inline void free_set(cloudsc_fields_t *f, const cloudsc_fields_t *keep) {
  void **fp = (void **)f;
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (!keep || fp[m] != ((void *const *)keep)[m]) free(fp[m]);
}

/* elements of the real columns that differ: rows [row_a, row_a + nrows) of a (abrows rows between its blocks)
 * against rows [row_b, ...) of b (bbrows rows between its blocks), elements of e bytes */
static inline long differing_rows(int ngptot, int nproma, size_t e, const void *a, long abrows, long row_a,
                                  const void *b, long bbrows, long row_b, long nrows) {
  long bad = 0;
  for (long g = 0; g < ngptot; g++)
    for (long r = 0; r < nrows; r++) {
      const size_t i = (size_t)((g / nproma * abrows + row_a + r) * nproma + g % nproma) * e;
      const size_t j = (size_t)((g / nproma * bbrows + row_b + r) * nproma + g % nproma) * e;
      bad += memcmp((const char *)a + i, (const char *)b + j, e) != 0;
    }
  return bad;
}
/* elements of the real columns of member m that differ between two block-layout arrays */
static inline long differing(const cloudsc_dataset_t *ds, int m, int ngptot, int nproma, int es, const void *a,
                             const void *b) {
  const long rows = rows_of(kinds[m], ds->klev);
  return differing_rows(ngptot, nproma, is_int[m] ? 4 : (size_t)es, a, rows, 0, b, rows, 0, rows);
}
/* bytes of the padding lanes of the last block of an OUT member of `rows` rows that are no longer `fill` */
static inline long padding_written(long rows, int ngptot, int nproma, int es, const void *a, int fill) {
  const int nb = nblocks(ngptot, nproma), tail = ngptot - (nb - 1) * nproma;
  long bad = 0;
  for (long r = 0; r < rows; r++) {
    const unsigned char *row = (const unsigned char *)a + (size_t)(((long)(nb - 1) * rows + r) * nproma) * es;
    for (size_t i = (size_t)tail * es; i < (size_t)nproma * es; i++) bad += row[i] != fill;
  }
  return bad;
}
static inline long not_fill(const void *a, size_t n, int fill) {
  long bad = 0;
  for (size_t i = 0; i < n; i++) bad += ((const unsigned char *)a)[i] != fill;
  return bad;
}

/* ---- the packed tendency buffers [nb][planes][klev][nproma] ---- */

/* first plane of (t, a, q, cld) of BUFFER_TMP and BUFFER_LOC: the reference's order and the hand-permuted ones */
typedef const int plane_order_t[4];
static plane_order_t ref_order[2] = {{0, 1, 2, 3}, {0, 1, 2, 3}};
static plane_order_t perm8[2] = {{6, 7, 5, 0}, {6, 0, 7, 1}}, perm11[2] = {{10, 0, 8, 2}, {0, 10, 1, 5}};

/* bind f's eight tendency members to the two buffers: by cloudsc_tendbuf_bind, or (permuted) by hand at the first
 * planes of perm8 / perm11; returns the order bound and adds to *bad if the bind fails */
static inline plane_order_t *bind_planes(cloudsc_fields_t *f, int precision, int nproma, int klev, int planes,
                                         int permuted, char *tmp, char *loc, long *bad) {
  const size_t plane = (size_t)klev * nproma * (precision == CLOUDSC_FP64 ? 8 : 4);
  plane_order_t *p = planes == 8 ? perm8 : perm11;
  if (!permuted) {
    if (cloudsc_tendbuf_bind(f, precision, nproma, klev, tmp, loc)) *bad += FAILED;
    return ref_order;
  }
  f->tendency_tmp_t = tmp + p[0][0] * plane; f->tendency_tmp_a = tmp + p[0][1] * plane;
  f->tendency_tmp_q = tmp + p[0][2] * plane; f->tendency_tmp_cld = tmp + p[0][3] * plane;
  f->tendency_loc_t = loc + p[1][0] * plane; f->tendency_loc_a = loc + p[1][1] * plane;
  f->tendency_loc_q = loc + p[1][2] * plane; f->tendency_loc_cld = loc + p[1][3] * plane;
  return p;
}
/* a set of f's four tendency_tmp_* (loc 0) or tendency_loc_* (loc 1) members alone */
static inline cloudsc_fields_t tendencies_of(const cloudsc_fields_t *f, int loc) {
  cloudsc_fields_t o;
  memset(&o, 0, sizeof(o));
  if (loc) {
    o.tendency_loc_t = f->tendency_loc_t; o.tendency_loc_a = f->tendency_loc_a;
    o.tendency_loc_q = f->tendency_loc_q; o.tendency_loc_cld = f->tendency_loc_cld;
  } else {
    o.tendency_tmp_t = f->tendency_tmp_t; o.tendency_tmp_a = f->tendency_tmp_a;
    o.tendency_tmp_q = f->tendency_tmp_q; o.tendency_tmp_cld = f->tendency_tmp_cld;
  }
  return o;
}
/* BUFFER_TMP from the set's separate tendency_tmp_* arrays, in the reference's plane order */
static inline void pack_tmp(const cloudsc_fields_t *s, int nb, int planes, size_t plane, char *tmp) {
  for (int b = 0; b < nb; b++) {
    memcpy(tmp + ((size_t)b * planes + CLOUDSC_TENDBUF_T) * plane, (const char *)s->tendency_tmp_t + b * plane, plane);
    memcpy(tmp + ((size_t)b * planes + CLOUDSC_TENDBUF_A) * plane, (const char *)s->tendency_tmp_a + b * plane, plane);
    memcpy(tmp + ((size_t)b * planes + CLOUDSC_TENDBUF_Q) * plane, (const char *)s->tendency_tmp_q + b * plane, plane);
    memcpy(tmp + ((size_t)b * planes + CLOUDSC_TENDBUF_CLD) * plane,
           (const char *)s->tendency_tmp_cld + (size_t)b * CLOUDSC_NCLV * plane, CLOUDSC_NCLV * plane);
  }
}
/* bytes of a buffer that are not `fill` although nothing may write them: planes outside the four members'
 * (first planes p[0..3], cld five wide) and the lanes past the last column */
static inline long touched_outside(const char *buf, const int p[4], int nb, int planes, int klev, int nproma, int es,
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

/* ---- the field-set walkers: one member of synthetic values, np columns per block (np 0: the LEVELS layout) ---- */

typedef double (*value_fn)(int m, long row, long g);   /* each driver's own encoding of (member, row, column) */

static inline void put(void *a, int m, int precision, size_t i, double v) {
  if (is_int[m]) ((int *)a)[i] = (int)v;
  else if (precision == CLOUDSC_FP64) ((double *)a)[i] = v;
  else ((float *)a)[i] = (float)v;
}
static inline double get(const void *a, int m, int precision, size_t i) {
  if (is_int[m]) return ((const int *)a)[i];
  return precision == CLOUDSC_FP64 ? ((const double *)a)[i] : ((const float *)a)[i];
}
static inline size_t elems(long ngptot, long rows, long np) {
  return (size_t)(np ? (ngptot + np - 1) / np * rows * np : ngptot * rows);
}
static inline size_t at(long g, long r, long rows, long np) {
  return (size_t)(np ? (g / np * rows + r) * np + g % np : g * rows + r);
}
/* member m as an exact-size block of `byte`, and with `value`, its real columns set */
static inline void *make_member(int m, int precision, long ngptot, long rows, long np, int byte, value_fn value) {
  void *a = alloc_filled(elems(ngptot, rows, np) * esize(m, precision), byte);
  for (long g = 0; value && g < ngptot; g++)
    for (long r = 0; r < rows; r++) put(a, m, precision, at(g, r, rows, np), value(m, r, g));
  return a;
}
/* elements of a converted member that are not value(), plus bytes of the padding lanes of a blocked one that are
 * no longer `byte` */
static inline long check_member(const void *d, int m, int precision, long ngptot, long rows, long np, int byte,
                                value_fn value) {
  const size_t e = esize(m, precision);
  size_t live = 0;
  long bad = 0;
  for (long g = 0; g < ngptot; g++)
    for (long r = 0; r < rows; r++, live++) bad += get(d, m, precision, at(g, r, rows, np)) != value(m, r, g);
  for (long b = 0; np && b < (ngptot + np - 1) / np; b++)
    for (long r = 0; r < rows; r++)
      for (long j = b * np + np > ngptot ? ngptot - b * np : np; j < np; j++, live++)
        bad += not_fill((const char *)d + (size_t)((b * rows + r) * np + j) * e, e, byte);
  return bad + (live != elems(ngptot, rows, np));
}

/* ---- main ---- */

static const int k_shapes[3][2] = {{100, 16}, {300, 64}, {1, 1}};   /* ngptot / nproma: partial last blocks, one column */
static const int k_precisions[2] = {CLOUDSC_FP64, CLOUDSC_MIXED};
/* the four storage pairs of the field-set walkers */
static const int k_storage[4][2] = {{CLOUDSC_FP64, CLOUDSC_FP64}, {CLOUDSC_FP64, CLOUDSC_MIXED},
                                    {CLOUDSC_MIXED, CLOUDSC_FP64}, {CLOUDSC_FP32, CLOUDSC_FP32}};

/* whether the comparisons above find what they are for: one byte changed in the last real column, one in a
 * padding lane, of a member of two blocks (5 columns in blocks of 4) */
static inline int helpers_bite(const cloudsc_dataset_t *ds) {
  const int m = CLOUDSC_M_pcovptot, ngptot = 5, nproma = 4, es = 8;
  const long rows = rows_of(kinds[m], ds->klev);
  const size_t n = member_bytes(ds, m, 2, nproma, es, 0);
  char *a = (char *)alloc_filled(n, FILL), *b = (char *)alloc_filled(n, FILL);
  b[((rows + rows - 1) * nproma + 0) * es] ^= 1;   /* block 1, the last row, lane 0: column 4 */
  b[((rows + 0) * nproma + 3) * es + 1] ^= 1;      /* block 1, row 0, lane 3: padding */
  const int ok = differing(ds, m, ngptot, nproma, es, a, b) == 1 && differing(ds, m, ngptot, nproma, es, a, a) == 0 &&
                 padding_written(rows, ngptot, nproma, es, b, FILL) == 1 &&
                 padding_written(rows, ngptot, nproma, es, a, FILL) == 0 && not_fill(b, n, FILL) == 2 &&
                 not_fill(a, n, FILL) == 0;
  free(a);
  free(b);
  return ok;
}
/* the data set of argv[1], or of the default directory; 0, or the exit status */
static inline int sanitize_load(const char *driver, int argc, char **argv, cloudsc_dataset_t *ds) {
  if (cloudsc_io_load_dir(argc > 1 ? argv[1] : "../data/cloudsc100", 0, ds)) {
    fprintf(stderr, "%s: cannot load the data set: %s\n", driver, cloudsc_io_last_error());
    return 2;
  }
  if (helpers_bite(ds)) return 0;
  fprintf(stderr, "%s: the shared comparisons do not find a changed byte\n", driver);
  cloudsc_io_free(ds);
  return 1;
}
/* the result line; returns the exit status */
static inline int sanitize_result(const char *driver, int cases, long bad) {
  printf("%s: %d cases, %ld mismatches: %s\n", driver, cases, bad, bad ? "FAILED" : "clean");
  return bad != 0;
}

#endif /* SANITIZE_COMMON_H */
