/*
 * dwarf_cloudsc_amd.c -- the dwarf host driver for MI355X:
 *
 *   dwarf-cloudsc-amd <nthreads> <ngptot> <nproma> [options]
 *
 * Same CLI, flow and stdout format as the reference C dwarf
 * (src/cloudsc_c/dwarf_cloudsc.c:17-50, cloudsc_driver.c:33-263): load the
 * KLON-column state (load_state.c), expand it to NGPTOT columns in NPROMA
 * blocks, run CLOUDSC, print the timing table, validate the 21 output fields
 * against the reference (cloudsc_validate.c:186-216).  Differences, all on
 * purpose:
 *   - the kernel runs on the GPU(s) through libcloudsc_amd.so (include/
 *     cloudsc_amd.h); expansion and the validation statistics run on the
 *     device against the KLON-column reference with the g % klon map, so no
 *     NGPTOT-sized host arrays exist;
 *   - HDF5 files are opened read-only (load_state.c:60,499,746 open RDWR);
 *     without input.h5 the raw dataset (data/cloudsc100) is read;
 *   - validation uses fabs like the Fortran ERROR_PRINT (validate_mod.F90:
 *     263-296), not the C validator's integer abs (cloudsc_validate.c:74);
 *   - the TOTAL line's col/s is NGPTOT/time (cloudsc_driver.c:261 prints the
 *     last thread's value);
 *   - exit status 1 if any field's relative L1 error exceeds the gate
 *     (--tol; default in fp64 the dwarf's own '!!!!' line, 10*eps: the
 *     fp64 kernels reproduce the reference kernel bit for bit; fp32 is
 *     reported without a gate unless --tol is given);
 *   - --gpus N shards the columns over N devices (block-aligned contiguous
 *     ranges of the GLOBAL column index, one host thread + stream per shard,
 *     no collective); statistics are combined on the host like the
 *     MPI_Reduce of validate_mod.F90:53-55.  With fewer visible devices than
 *     shards, shard d runs on device d % ndev (the shards of one device then
 *     share it; results are the same bits, only the timing differs).
 *
 * nthreads is the host thread count of --variant cpu (the library's CPU
 * variant, BASELINE.json config 1: `1 16384 32`); for the GPU variants it is
 * accepted and printed as NUMOMP for compatibility, the host threads being
 * one per shard.
 */
#define _GNU_SOURCE
#include <float.h>
#include <limits.h>
#include <math.h>
#include <dirent.h>
#include <dlfcn.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "cloudsc_amd.h"
#include "cloudsc_fields.def"
#include "cloudsc_io.h"

#define ZHPM 12482329.0   /* HPM flop count for 100 columns (cloudsc_driver.c:101) */
#define VARIANT_CPU 0     /* --variant cpu: cloudsc_cpu_run on the host cores (config 1) */

typedef struct {
  int numomp, ngptot, nproma, ngpus, precision, variant, reps, warmup;
  int transfer, chunk_blocks, nstreams, exact_libm;
  int fields_levels;              /* --fields levels: --fields caller from and into CLOUDSC_LAYOUT_LEVELS arrays */
  int fields_caller;              /* --fields caller | tendbuf | tendbuf-inplace | tendbuf-cml (1 | 2 | 3 | 4): caller-owned field sets */
  int tend_planes;                /* --fields tendbuf: planes per block of the two tendency buffers (0: not tendbuf) */
  int outputs, outputs_given;     /* --outputs all|prognostic|surface: CLOUDSC_OUTPUTS_* */
  int spp;                        /* --spp unit: the step through the SPP form, five all-ones multiplier fields */
  int advance;                    /* --advance N: N advancing steps in place (cloudsc_*_run_advance); 0: not given */
  int batch;                      /* --batch N: N caller-owned sets of <ngptot> columns each, one batched launch per step; 0: not given */
  int place;                      /* placement search: 1 on, 0 off, -1 auto (on when reps > 1) */
  int narrow_pack;                /* NPROMA <= 32 packed into full waves: 1 on, 0 off, -1 the library's default */
  double energy_s;                /* --energy: seconds of back-to-back launches sampled for board power */
  double tol;
  int tol_given;
  const char *input_h5, *reference_h5, *data_dir, *write_h5_dir;
} options_t;

typedef struct {
  int device, ngptot, nproma, precision, variant, reps, warmup;
  int libm_bit;                   /* CLOUDSC_FP32_EXACT_LIBM or 0 */
  int caller, place_on, aerosols; /* --fields caller; its placement search; aerosol inputs allocated */
  int levels;                     /* --fields levels: caller, the set held level-contiguous at both ends */
  int tend_planes;                /* --fields tendbuf: the step runs on two packed tendency buffers of that many planes */
  int inplace;                    /* --fields tendbuf-inplace: fill, step and validation on the buffers themselves */
  int cml;                        /* --fields tendbuf-cml: inplace, the step adding its tendencies to a zeroed BUFFER_CML (no BUFFER_LOC) */
  int outputs;                    /* --outputs: CLOUDSC_OUTPUTS_* */
  int spp;                        /* --spp unit: cloudsc_gpu_run_spp with five all-ones multiplier fields */
  int advance;                    /* --advance N: the timed steps are N cloudsc_gpu_run_advance in place */
  int batch;                      /* --batch N: ngptot is N sets of ngptot / N columns, stepped by one cloudsc_gpu_run_batch */
  double energy_s;
  long long col_offset;
  const cloudsc_template_t *tmpl;
  const cloudsc_params_t *params;
  const cloudsc_reference_t *ref;
  pthread_barrier_t *barrier;
  /* results */
  int rc;
  char err[256];                  /* this shard's cloudsc_last_hip_error() (thread-local in the library) */
  double t_start, t_end;          /* seconds, CLOCK_MONOTONIC */
  float *kernel_ms;
  cloudsc_placement_t place;      /* the state's placement search and its cost */
  char power_path[512];           /* the device's hwmon power file ("" = none) */
  double board_w, energy_ms_per_step;   /* mean board power over the energy window, and its time per launch */
  int power_samples, energy_steps;
  cloudsc_stats_t stats[CLOUDSC_NVALID];
  int skipped[CLOUDSC_NVALID];    /* --outputs: validated fields the set does not hold (no row, not gated) */
} shard_t;

static const char *variant_name(int v) {
  switch (v) {
    case CLOUDSC_VARIANT_KSEG: return "kseg";
    case CLOUDSC_VARIANT_KCACHE: return "kcache";
    case CLOUDSC_VARIANT_SCC: return "scc";
    case CLOUDSC_VARIANT_SCC_PRIVATE: return "scc-private";
    default: return "cpu";
  }
}

static double now(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

static void usage(const char *prog) {
  fprintf(stderr,
          "usage: %s [<nthreads> <ngptot> <nproma>] [options]\n"
          "  --gpus N              shard the columns over N devices (default 1)\n"
          "  --precision fp64|fp32|mixed (default fp64; mixed: float fields, double arithmetic,\n"
          "                        variants kseg, kcache and cpu; validated like fp32)\n"
          "  --variant kseg|kcache|scc|scc-private|cpu (default kseg; cpu = the library's CPU variant on\n"
          "                        <nthreads> host threads, host-memory fields: BASELINE config 1)\n"
          "  --fp32-exact-libm     fp32: exp/pow with the glibc algorithms (bit-identical to the fp32\n"
          "                        restatement) instead of the default float-internal device forms\n"
          "  --reps R              timed steps (default 1)\n"
          "  --place on|off|auto   output placement search at state creation (~0.5 s, ~250 kernel\n"
          "                        launches; default auto: on when --reps > 1, off for one step)\n"
          "  --narrow-pack on|off|auto  kseg, kcache: run blocks of NPROMA <= 32 packed, 64 / NPROMA blocks\n"
          "                        per wave (same layout, same bits); auto = the measured default per width\n"
          "  --warmup W            untimed steps before the timed ones (default 1)\n"
          "  --energy S            after the timed steps, S seconds of back-to-back launches with the\n"
          "                        device's board power sampled every 10 ms (hwmon power1_input):\n"
          "                        prints an ENERGY line per shard (uJ per column)\n"
          "  --input FILE          input HDF5 file (default ./input.h5 when present)\n"
          "  --reference FILE      reference HDF5 file (default ./reference.h5 when present)\n"
          "  --data DIR            raw dataset directory (default $CLOUDSC_DATA or the\n"
          "                        repository's data/cloudsc100)\n"
          "  --tol X               relative L1 gate per field (default 10*eps = 2.2e-15 for fp64)\n"
          "  --fields state|caller state (default): the device-resident state API; caller: the reference\n"
          "                        CUDA driver's shape on caller-owned device fields, per shard\n"
          "                        cloudsc_fields_alloc, _expand, cloudsc_gpu_run, cloudsc_gpu_check,\n"
          "                        cloudsc_fields_validate (not with --transfer or --variant cpu)\n"
          "  --fields levels       caller, with the caller's data level-contiguous ([ngptot][rows]) at both ends:\n"
          "                        the template expanded into a blocked staging set and converted to LEVELS,\n"
          "                        cloudsc_fields_convert_layout LEVELS -> the placed NPROMA set, the step, the\n"
          "                        outputs -> LEVELS -> blocked, validated there (kseg and kcache only)\n"
          "  --fields tendbuf      caller, with the tendencies in the reference Fortran drivers' two packed\n"
          "                        buffers: tendency_tmp_* packed into a BUFFER_TMP, cloudsc_gpu_run_tendbuf,\n"
          "                        BUFFER_LOC unpacked before the validation (kseg and kcache only)\n"
          "  --fields tendbuf-inplace  tendbuf without the two conversions: cloudsc_fields_expand_tendbuf,\n"
          "                        cloudsc_gpu_run_tendbuf_outputs, cloudsc_fields_validate_tendbuf on BUFFER_LOC (the\n"
          "                        separate tendency arrays cloudsc_fields_alloc makes are never read or written)\n"
          "  --fields tendbuf-cml  tendbuf-inplace without a BUFFER_LOC: cloudsc_gpu_run_tendbuf_cml adds the step's\n"
          "                        tendencies to a zeroed third buffer (BUFFER_CML), whose planes are validated in\n"
          "                        place; needs --outputs prognostic|surface\n"
          "  --tend-planes N       --fields tendbuf[-inplace]: planes per block of the two buffers, 8..64 (default 8)\n"
          "  --outputs all|prognostic  --fields caller|tendbuf|tendbuf-inplace: prognostic = a step without the ten\n"
          "                        diagnostic fluxes, which are not allocated, validated or printed (kseg, kcache)\n"
          "  --outputs surface     prognostic, and PFPLSL, PFPLSN, PFHPSL, PFHPSN held at the surface only: their rows\n"
          "                        are validated against the last half level of the reference profiles (kseg and\n"
          "                        kcache as above; also --variant cpu, fp64 or mixed, without --fields)\n"
          "  --spp unit            the step through the per-column multiplier form (cloudsc_gpu_run_spp with --fields\n"
          "                        caller|levels, kseg or kcache, --outputs all|prognostic; cloudsc_cpu_run_spp with\n"
          "                        --variant cpu) on five all-ones fields: the bits of the step without the flag\n"
          "  --advance N           N >= 1 advancing steps in place instead of the timed steps: pt, pq, pa, pclv of the\n"
          "                        set are rewritten by each (cloudsc_gpu_run_advance with --fields caller, kseg or\n"
          "                        kcache, --outputs all|surface; cloudsc_cpu_run_advance with --variant cpu).  With\n"
          "                        N = 1 the fluxes, PCOVPTOT, PLUDE and PRAINFRAC_TOPRFZ are validated, the tendencies\n"
          "                        are not stored and have no row; with N > 1 nothing is validated.  One ADVANCE line\n"
          "                        follows the table: the steps taken and the time per step\n"
          "  --batch N             --fields caller --variant kcache: N field sets of <ngptot> columns each (set i the\n"
          "                        columns from i * <ngptot>), all stepped by one cloudsc_gpu_run_batch launch; every set\n"
          "                        is validated and the table is that of the N * <ngptot> columns together\n"
          "  --transfer            host-buffer path: block-layout arrays in host memory,\n"
          "                        H2D -> kernel -> D2H per chunk, overlapped on streams\n"
          "                        (TOTAL includes the transfers, like cloudsc_driver.cu)\n"
          "  --chunk B --streams S chunk size in NPROMA blocks (128) and device chunk slots (3)\n"
          "  --write-h5 DIR        write DIR/input.h5 and DIR/reference.h5 of the loaded\n"
          "                        dataset and exit\n",
          prog);
}

static int parse(int argc, char **argv, options_t *o) {
  memset(o, 0, sizeof(*o));
  o->numomp = 1; o->ngptot = 100; o->nproma = 4;     /* dwarf_cloudsc.c:25-27 defaults */
  o->ngpus = 1; o->precision = CLOUDSC_FP64; o->variant = CLOUDSC_VARIANT_KSEG;
  o->reps = 1; o->warmup = 1; o->tol = 10.0 * DBL_EPSILON; o->place = -1; o->narrow_pack = -1;
  o->chunk_blocks = 128; o->nstreams = 3;  /* chunk slots; profiles/r04/transfer_sweep_kseg_fp64.txt */
  int npos = 0;
  long pos[3] = {0, 0, 0};
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    const char *v = i + 1 < argc ? argv[i + 1] : NULL;
#define NEEDV() do { if (!v) { fprintf(stderr, "%s needs a value\n", a); return -1; } i++; } while (0)
    if (!strcmp(a, "--gpus")) { NEEDV(); o->ngpus = atoi(v); }
    else if (!strcmp(a, "--precision")) {
      NEEDV();
      if (!strcmp(v, "fp64") || !strcmp(v, "dp")) o->precision = CLOUDSC_FP64;
      else if (!strcmp(v, "fp32") || !strcmp(v, "sp")) o->precision = CLOUDSC_FP32;
      else if (!strcmp(v, "mixed") || !strcmp(v, "mp")) o->precision = CLOUDSC_MIXED;
      else { fprintf(stderr, "bad precision %s\n", v); return -1; }
    } else if (!strcmp(a, "--variant")) {
      NEEDV();
      if (!strcmp(v, "kseg")) o->variant = CLOUDSC_VARIANT_KSEG;
      else if (!strcmp(v, "kcache")) o->variant = CLOUDSC_VARIANT_KCACHE;
      else if (!strcmp(v, "scc")) o->variant = CLOUDSC_VARIANT_SCC;
      else if (!strcmp(v, "scc-private")) o->variant = CLOUDSC_VARIANT_SCC_PRIVATE;
      else if (!strcmp(v, "cpu")) o->variant = VARIANT_CPU;
      else { fprintf(stderr, "bad variant %s\n", v); return -1; }
    } else if (!strcmp(a, "--reps")) { NEEDV(); o->reps = atoi(v); }
    else if (!strcmp(a, "--warmup")) { NEEDV(); o->warmup = atoi(v); }
    else if (!strcmp(a, "--energy")) {
      NEEDV();
      char *end;
      o->energy_s = strtod(v, &end);
      if (*end || !(o->energy_s >= 0.0) || o->energy_s > 600.0) { fprintf(stderr, "bad --energy %s\n", v); return -1; }
    }
    else if (!strcmp(a, "--place")) {
      NEEDV();
      if (!strcmp(v, "on")) o->place = 1;
      else if (!strcmp(v, "off")) o->place = 0;
      else if (!strcmp(v, "auto")) o->place = -1;
      else { fprintf(stderr, "bad --place %s\n", v); return -1; }
    }
    else if (!strcmp(a, "--narrow-pack")) {
      NEEDV();
      if (!strcmp(v, "on")) o->narrow_pack = 1;
      else if (!strcmp(v, "off")) o->narrow_pack = 0;
      else if (!strcmp(v, "auto")) o->narrow_pack = -1;
      else { fprintf(stderr, "bad --narrow-pack %s\n", v); return -1; }
    }
    else if (!strcmp(a, "--input")) { NEEDV(); o->input_h5 = v; }
    else if (!strcmp(a, "--reference")) { NEEDV(); o->reference_h5 = v; }
    else if (!strcmp(a, "--data")) { NEEDV(); o->data_dir = v; }
    else if (!strcmp(a, "--tol")) { NEEDV(); o->tol = atof(v); o->tol_given = 1; }
    else if (!strcmp(a, "--write-h5")) { NEEDV(); o->write_h5_dir = v; }
    else if (!strcmp(a, "--transfer")) o->transfer = 1;
    else if (!strcmp(a, "--fields")) {
      NEEDV();
      o->fields_levels = 0;   /* the last --fields decides */
      if (!strcmp(v, "state")) o->fields_caller = 0;
      else if (!strcmp(v, "caller")) o->fields_caller = 1;
      else if (!strcmp(v, "levels")) { o->fields_caller = 1; o->fields_levels = 1; }
      else if (!strcmp(v, "tendbuf")) o->fields_caller = 2;
      else if (!strcmp(v, "tendbuf-inplace")) o->fields_caller = 3;
      else if (!strcmp(v, "tendbuf-cml")) o->fields_caller = 4;
      else { fprintf(stderr, "bad --fields %s\n", v); return -1; }
    }
    else if (!strcmp(a, "--tend-planes")) {
      NEEDV();
      o->tend_planes = atoi(v);
      if (o->tend_planes < CLOUDSC_TENDBUF_PLANES_MIN || o->tend_planes > CLOUDSC_TENDBUF_PLANES_MAX) {
        fprintf(stderr, "bad --tend-planes %s\n", v);
        return -1;
      }
    }
    else if (!strcmp(a, "--outputs")) {
      NEEDV();
      o->outputs_given = 1;
      if (!strcmp(v, "all")) o->outputs = CLOUDSC_OUTPUTS_ALL;
      else if (!strcmp(v, "prognostic")) o->outputs = CLOUDSC_OUTPUTS_PROGNOSTIC;
      else if (!strcmp(v, "surface")) o->outputs = CLOUDSC_OUTPUTS_SURFACE;
      else { fprintf(stderr, "bad --outputs %s\n", v); return -1; }
    }
    else if (!strcmp(a, "--spp")) {
      NEEDV();
      if (!strcmp(v, "unit")) o->spp = 1;
      else { fprintf(stderr, "bad --spp %s\n", v); return -1; }
    }
    else if (!strcmp(a, "--advance")) {
      NEEDV();
      char *end;
      const long n = strtol(v, &end, 10);
      if (*end || n < 1 || n > 100000) { fprintf(stderr, "bad --advance %s\n", v); return -1; }
      o->advance = (int)n;
    }
    else if (!strcmp(a, "--batch")) {
      NEEDV();
      char *end;
      const long n = strtol(v, &end, 10);
      if (*end || n < 1 || n > CLOUDSC_BATCH_MAX_SETS) { fprintf(stderr, "bad --batch %s\n", v); return -1; }
      o->batch = (int)n;
    }
    else if (!strcmp(a, "--fp32-exact-libm")) o->exact_libm = 1;
    else if (!strcmp(a, "--chunk")) { NEEDV(); o->chunk_blocks = atoi(v); }
    else if (!strcmp(a, "--streams")) { NEEDV(); o->nstreams = atoi(v); }
    else if (!strcmp(a, "-h") || !strcmp(a, "--help")) return -1;
    else if (a[0] == '-' && a[1] == '-') { fprintf(stderr, "unknown option %s\n", a); return -1; }
    else {
      if (npos >= 3) { fprintf(stderr, "too many arguments\n"); return -1; }
      char *end;
      pos[npos++] = strtol(a, &end, 10);
      if (*end) { fprintf(stderr, "not a number: %s\n", a); return -1; }
    }
#undef NEEDV
  }
  if (npos != 0 && npos != 3) {
    /* dwarf_cloudsc.c:45-48 */
    printf("Calling c-cloudsc with the right number of arguments will work better ;-) \n");
    return -1;
  }
  if (npos == 3) {
    o->numomp = (int)pos[0]; o->ngptot = (int)pos[1]; o->nproma = (int)pos[2];
    if (o->numomp <= 0) o->numomp = 1;
  }
  /* KCACHE/SCC run one workgroup of NPROMA threads per block; KSEG any NPROMA */
  const int max_nproma = (o->variant == CLOUDSC_VARIANT_KSEG || o->variant == VARIANT_CPU) ? (1 << 24) : 256;
  if (o->ngptot <= 0 || o->nproma <= 0 || o->nproma > max_nproma || o->ngpus <= 0 || o->reps <= 0 ||
      o->warmup < 0) {
    fprintf(stderr, "invalid sizes: ngptot %d nproma %d (1..%d) gpus %d reps %d\n", o->ngptot, o->nproma,
            max_nproma, o->ngpus, o->reps);
    return -1;
  }
  return 0;
}

/* the raw dataset next to the executable: <exe dir>/../data/cloudsc100 */
static void default_data_dir(char *out, size_t n) {
  const char *env = getenv("CLOUDSC_DATA");
  if (env && *env) { snprintf(out, n, "%s", env); return; }
  char exe[PATH_MAX - 64];
  ssize_t len = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
  if (len <= 0) { snprintf(out, n, "data/cloudsc100"); return; }
  exe[len] = 0;
  char *slash = strrchr(exe, '/');
  if (slash) *slash = 0;
  snprintf(out, n, "%s/../data/cloudsc100", exe);
}

static int exists(const char *p) { return access(p, R_OK) == 0; }

/* ---- board power (--energy): the reference reads energy beside its timings
 * (EC_PMON, src/common/module/ec_pmon_mod.F90, dwarf_cloudsc.F90:42-46).  On an
 * MI355X host the GPU's sensor is its hwmon power file in microwatts, found
 * through the device's PCI bus id (hipDeviceGetPCIBusId, from the HIP runtime
 * the library has loaded); read-only. ---- */
static void power_file(int device, char *out, size_t n) {
  out[0] = 0;
  void *hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_NOLOAD);
  if (!hip) hip = dlopen("libamdhip64.so", RTLD_NOW);
  if (!hip) return;
  int (*bus_id)(char *, int, int) = (int (*)(char *, int, int))dlsym(hip, "hipDeviceGetPCIBusId");
  char bus[64];
  if (!bus_id || bus_id(bus, (int)sizeof(bus), device) != 0) return;
  for (char *c = bus; *c; c++)
    if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
  char dir[256];
  snprintf(dir, sizeof(dir), "/sys/bus/pci/devices/%s/hwmon", bus);
  DIR *d = opendir(dir);
  if (!d) return;
  struct dirent *e;
  while ((e = readdir(d))) {
    if (strncmp(e->d_name, "hwmon", 5)) continue;
    static const char *names[2] = {"power1_input", "power1_average"};
    for (int k = 0; k < 2 && !out[0]; k++) {
      char f[512];
      snprintf(f, sizeof(f), "%.256s/%.64s/%.32s", dir, e->d_name, names[k]);
      FILE *fp = fopen(f, "r");
      if (!fp) continue;
      long long uw;
      if (fscanf(fp, "%lld", &uw) == 1) snprintf(out, n, "%s", f);
      fclose(fp);
    }
    if (out[0]) break;
  }
  closedir(d);
}

typedef struct {
  const char *path;
  volatile int stop;
  double sum_w;
  int n;
} sampler_t;

static void *sampler_main(void *arg) {
  sampler_t *sp = (sampler_t *)arg;
  const struct timespec period = {0, 10 * 1000 * 1000};
  while (!sp->stop) {
    FILE *fp = fopen(sp->path, "r");
    if (fp) {
      long long uw;
      if (fscanf(fp, "%lld", &uw) == 1) { sp->sum_w += uw * 1e-6; sp->n++; }
      fclose(fp);
    }
    nanosleep(&period, NULL);
  }
  return NULL;
}

/* S seconds of back-to-back launches (plain dispatches, timed 20 at a time) with
 * the board power sampled: mean W and the time per launch, for the ENERGY line */
static int energy_window(shard_t *s, cloudsc_gpu_state_t *st) {
  power_file(s->device, s->power_path, sizeof(s->power_path));
  if (!s->power_path[0]) return CLOUDSC_OK;
  sampler_t sp = {s->power_path, 0, 0.0, 0};
  pthread_t th;
  if (pthread_create(&th, NULL, sampler_main, &sp)) return CLOUDSC_OK;
  const double t0 = now();
  double span_ms = 0.0;
  int steps = 0, rc = CLOUDSC_OK;
  while (!rc && now() - t0 < s->energy_s) {
    float ms = 0.f;
    rc = cloudsc_state_run_span(st, s->variant | s->libm_bit, 20, &ms);
    span_ms += ms;
    steps += 20;
  }
  sp.stop = 1;
  pthread_join(th, NULL);
  s->power_samples = sp.n;
  s->board_w = sp.n ? sp.sum_w / sp.n : 0.0;
  s->energy_steps = steps;
  s->energy_ms_per_step = steps ? span_ms / steps : 0.0;
  return rc;
}

/* ---- --fields caller: the reference CUDA driver's shape (cloudsc_driver.cu:276-447) on caller-owned
 * device fields: allocate, expand the template on the device, launch, check, validate on the device.
 * The KSEG / SCC workspace is the caller's too: hipMalloc from the HIP runtime the library has loaded. ---- */
static void *hip_sym(const char *name) {
  void *hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_NOLOAD);
  if (!hip) hip = dlopen("libamdhip64.so", RTLD_NOW);
  return hip ? dlsym(hip, name) : NULL;
}

/* one step of a --fields caller | tendbuf shard on the field set f (tendbuf: its tendencies in the buffers) */
static int caller_step(const shard_t *s, int variant, int klev, const cloudsc_fields_t *f, void *ws,
                       const cloudsc_tend_cml_t *cml, const cloudsc_spp_t *spp) {
  if (s->advance) {                                      /* --advance N: in place */
    const cloudsc_advance_t adv = {(void *)f->pt, (void *)f->pq, (void *)f->pa, (void *)f->pclv};
    return cloudsc_gpu_run_advance(s->device, NULL, s->precision, variant, s->outputs, s->ngptot, s->nproma, klev, f, &adv,
                                   ws);
  }
  if (s->spp)                                            /* --spp unit */
    return cloudsc_gpu_run_spp(s->device, NULL, s->precision, variant, s->outputs, s->ngptot, s->nproma, klev, f, spp,
                               ws);
  if (s->cml)                                            /* --fields tendbuf-cml */
    return cloudsc_gpu_run_tendbuf_cml(s->device, NULL, s->precision, variant, s->outputs, s->ngptot, s->nproma, klev,
                                       s->tend_planes, f, cml, ws);
  if (s->outputs != CLOUDSC_OUTPUTS_ALL || s->inplace)   /* --outputs prognostic, --fields tendbuf-inplace */
    return s->tend_planes
               ? cloudsc_gpu_run_tendbuf_outputs(s->device, NULL, s->precision, variant, s->outputs, s->ngptot,
                                                 s->nproma, klev, s->tend_planes, f, ws)
               : cloudsc_gpu_run_outputs(s->device, NULL, s->precision, variant, s->outputs, s->ngptot, s->nproma,
                                         klev, f, ws);
  if (s->tend_planes)
    return cloudsc_gpu_run_tendbuf(s->device, NULL, s->precision, variant, s->ngptot, s->nproma, klev, s->tend_planes, f,
                                   ws);
  return cloudsc_gpu_run(s->device, NULL, s->precision, variant, s->ngptot, s->nproma, klev, f, ws);
}

/* the members of f the step reads (want_out 0: inputs and plude) or writes (1: outputs and plude) */
#define FIELD_DIR(n, N, k, d, i) CLOUDSC_FD_##d,
static const int k_field_dir[CLOUDSC_NFIELDS] = {CLOUDSC_FIELDS(FIELD_DIR)};
static void fields_part(const cloudsc_fields_t *f, int want_out, cloudsc_fields_t *part) {
  memset(part, 0, sizeof(*part));
  for (int m = 0; m < CLOUDSC_NFIELDS; m++)
    if (k_field_dir[m] == CLOUDSC_FD_INOUT || (k_field_dir[m] == CLOUDSC_FD_OUT) == (want_out != 0))
      ((const void **)part)[m] = ((const void *const *)f)[m];
}

/* --fields levels: `part` (0 inputs, 1 outputs) of src -> dst, a LEVELS side's NPROMA given as 0 */
static int levels_convert(const shard_t *s, int klev, int part, const cloudsc_fields_t *src, int src_nproma,
                          const cloudsc_fields_t *dst, int dst_nproma) {
  cloudsc_fields_t a, b;
  fields_part(src, part, &a);
  fields_part(dst, part, &b);
  return cloudsc_fields_convert_layout(s->device, NULL, s->ngptot, klev, s->outputs, s->precision,
                                       src_nproma ? CLOUDSC_LAYOUT_BLOCKED : CLOUDSC_LAYOUT_LEVELS, src_nproma, &a,
                                       s->precision, dst_nproma ? CLOUDSC_LAYOUT_BLOCKED : CLOUDSC_LAYOUT_LEVELS,
                                       dst_nproma, &b);
}

static void shard_caller(shard_t *s) {
  int (*set_device)(int) = (int (*)(int))hip_sym("hipSetDevice");
  int (*dmalloc)(void **, size_t) = (int (*)(void **, size_t))hip_sym("hipMalloc");
  int (*dmemset)(void *, int, size_t) = (int (*)(void *, int, size_t))hip_sym("hipMemset");
  int (*dfree)(void *) = (int (*)(void *))hip_sym("hipFree");
  const int klev = s->tmpl->klev, variant = s->variant | s->libm_bit;
  cloudsc_fields_t f, plude;
  memset(&f, 0, sizeof(f));
  memset(&plude, 0, sizeof(plude));
  void *ws = NULL;
  /* --fields tendbuf: g is f with the eight tendency members bound to the two buffers; tmp_* / loc_* hold
   * the tendency_tmp_* / tendency_loc_* members alone, of the separate arrays (sep) and of the buffers (buf) */
  const int tp = s->tend_planes, inplace = s->inplace, alloc_flags =
      (s->place_on ? 0 : CLOUDSC_PLACE_NONE) | (s->aerosols ? CLOUDSC_ALLOC_AEROSOLS : 0);
  void *buf_tmp = NULL, *buf_loc = NULL, *buf_cml = NULL;
  size_t buf_bytes = 0;
  cloudsc_tend_cml_t cml;
  memset(&cml, 0, sizeof(cml));
  cloudsc_fields_t g, tmp_sep, tmp_buf, loc_sep, loc_buf;
  memset(&tmp_sep, 0, sizeof(tmp_sep)); memset(&tmp_buf, 0, sizeof(tmp_buf));
  memset(&loc_sep, 0, sizeof(loc_sep)); memset(&loc_buf, 0, sizeof(loc_buf));
  s->rc = set_device && dmalloc && dmemset && dfree ? CLOUDSC_OK : CLOUDSC_EHIP;
  if (!s->rc && s->outputs != CLOUDSC_OUTPUTS_ALL)
    s->rc = cloudsc_fields_alloc_outputs(s->device, s->precision, s->ngptot, s->nproma, klev, alloc_flags, s->outputs,
                                         &f, &s->place);
  else if (!s->rc)
    s->rc = cloudsc_fields_alloc(s->device, s->precision, s->ngptot, s->nproma, klev, alloc_flags, &f, &s->place);
  /* --fields levels: `lev` is the caller's data, [ngptot][rows] (the elements of one block of ngptot columns);
   * `stage` the blocked set the template is expanded into and the outputs are validated in */
  cloudsc_fields_t stage, lev;
  memset(&stage, 0, sizeof(stage));
  memset(&lev, 0, sizeof(lev));
  if (!s->rc && s->levels) {
    const int flags = alloc_flags | CLOUDSC_PLACE_NONE;
    cloudsc_placement_t none;
    s->rc = cloudsc_fields_alloc_outputs(s->device, s->precision, s->ngptot, s->nproma, klev, flags, s->outputs, &stage, &none);
    if (!s->rc)
      s->rc = cloudsc_fields_alloc_outputs(s->device, s->precision, s->ngptot, s->ngptot, klev, flags, s->outputs, &lev, &none);
    if (!s->rc) s->rc = cloudsc_fields_expand(s->device, NULL, s->precision, s->ngptot, s->nproma, s->col_offset, s->tmpl, &stage);
    if (!s->rc) s->rc = levels_convert(s, klev, 0, &stage, s->nproma, &lev, 0);
    if (!s->rc) s->rc = levels_convert(s, klev, 0, &lev, 0, &f, s->nproma);
  }
  /* (tendbuf-inplace fills g below, once the tendency members are bound to the buffers) */
  if (!s->rc && !inplace && !s->levels) s->rc = cloudsc_fields_expand(s->device, NULL, s->precision, s->ngptot, s->nproma, s->col_offset, s->tmpl, &f);
  const long long wsb = cloudsc_gpu_scratch_bytes(s->precision, s->variant, s->ngptot, s->nproma, klev);
  if (!s->rc && wsb < 0) s->rc = CLOUDSC_EINVAL;
  if (!s->rc && wsb > 0 && (set_device(s->device) || dmalloc(&ws, (size_t)wsb) || dmemset(ws, 0, 256))) s->rc = CLOUDSC_ENOMEM;
  g = f;
  if (!s->rc && tp) {
    const size_t es = s->precision == CLOUDSC_FP64 ? 8 : 4;
    const size_t nb = (size_t)(s->ngptot / s->nproma + (s->ngptot % s->nproma ? 1 : 0));
    const size_t bytes = nb * (size_t)tp * (size_t)klev * (size_t)s->nproma * es;
    buf_bytes = bytes;
    /* tendbuf-cml: BUFFER_CML in the place of BUFFER_LOC, which the caller does not have */
    if (set_device(s->device) || dmalloc(&buf_tmp, bytes) || dmalloc(s->cml ? &buf_cml : &buf_loc, bytes)) s->rc = CLOUDSC_ENOMEM;
    if (!s->rc) s->rc = cloudsc_tendbuf_bind(&g, s->precision, s->nproma, klev, buf_tmp, s->cml ? buf_cml : buf_loc);
    if (!s->rc && s->cml) {
      s->rc = cloudsc_tendbuf_bind_cml(&cml, s->precision, s->nproma, klev, buf_cml);
      g.tendency_loc_t = g.tendency_loc_a = g.tendency_loc_q = g.tendency_loc_cld = NULL;   /* never touched */
    }
    tmp_sep.tendency_tmp_t = f.tendency_tmp_t; tmp_sep.tendency_tmp_a = f.tendency_tmp_a;
    tmp_sep.tendency_tmp_q = f.tendency_tmp_q; tmp_sep.tendency_tmp_cld = f.tendency_tmp_cld;
    tmp_buf.tendency_tmp_t = g.tendency_tmp_t; tmp_buf.tendency_tmp_a = g.tendency_tmp_a;
    tmp_buf.tendency_tmp_q = g.tendency_tmp_q; tmp_buf.tendency_tmp_cld = g.tendency_tmp_cld;
    loc_sep.tendency_loc_t = f.tendency_loc_t; loc_sep.tendency_loc_a = f.tendency_loc_a;
    loc_sep.tendency_loc_q = f.tendency_loc_q; loc_sep.tendency_loc_cld = f.tendency_loc_cld;
    loc_buf.tendency_loc_t = g.tendency_loc_t; loc_buf.tendency_loc_a = g.tendency_loc_a;
    loc_buf.tendency_loc_q = g.tendency_loc_q; loc_buf.tendency_loc_cld = g.tendency_loc_cld;
    /* tendbuf-inplace: every input from the template, tendency_tmp_* straight into their planes of BUFFER_TMP */
    if (!s->rc && inplace)
      s->rc = cloudsc_fields_expand_tendbuf(s->device, NULL, s->precision, s->ngptot, s->nproma, tp, s->col_offset,
                                            s->tmpl, &g);
    /* pack the expanded tendency_tmp_* into BUFFER_TMP (stream order: before the first step) */
    if (!s->rc && !inplace)
      s->rc = cloudsc_fields_convert_tendbuf(s->device, NULL, s->ngptot, klev, s->precision, s->nproma, 0, &tmp_sep,
                                             s->precision, s->nproma, tp, &tmp_buf);
  }
  /* --spp unit: one surface field of ones ([nblocks][nproma], the storage type) behind all five members */
  void *spp_ones = NULL;
  cloudsc_spp_t spp;
  memset(&spp, 0, sizeof(spp));
  if (!s->rc && s->spp) {
    int (*h2d)(void *, const void *, size_t, int) = (int (*)(void *, const void *, size_t, int))hip_sym("hipMemcpy");
    const size_t es = s->precision == CLOUDSC_FP64 ? 8 : 4;
    const size_t n = (size_t)(s->ngptot / s->nproma + (s->ngptot % s->nproma ? 1 : 0)) * (size_t)s->nproma;
    void *host = malloc(n * es);
    for (size_t i = 0; host && i < n; i++) {
      if (es == 8) ((double *)host)[i] = 1.0;
      else ((float *)host)[i] = 1.0f;
    }
    if (!host || !h2d || set_device(s->device) || dmalloc(&spp_ones, n * es) || h2d(spp_ones, host, n * es, 1))
      s->rc = CLOUDSC_ENOMEM;
    free(host);
    spp.ramid = spp.rcldiff = spp.rclcrit = spp.rlcritsnow = spp.rpecons = spp_ones;
  }
  plude.plude = f.plude;
  /* plude is INOUT: expanded again before every step, outside the timing */
  for (int r = 0; r < s->warmup && !s->rc; r++) {
    if (r) s->rc = cloudsc_fields_expand(s->device, NULL, s->precision, s->ngptot, s->nproma, s->col_offset, s->tmpl, &plude);
    /* a launch adds once: BUFFER_CML is zeroed again before every step, outside the timing */
    if (!s->rc && s->cml && dmemset(buf_cml, 0, buf_bytes)) s->rc = CLOUDSC_EHIP;
    if (!s->rc) s->rc = caller_step(s, variant, klev, &g, ws, &cml, &spp);
    if (!s->rc) s->rc = cloudsc_gpu_check(s->device, NULL, s->variant, ws);
  }
  pthread_barrier_wait(s->barrier);
  s->t_start = now();
  double timed = 0.0;
  for (int r = 0; r < s->reps && !s->rc; r++) {
    if (r || s->warmup)
      s->rc = cloudsc_fields_expand(s->device, NULL, s->precision, s->ngptot, s->nproma, s->col_offset, s->tmpl, &plude);
    if (!s->rc && s->cml && dmemset(buf_cml, 0, buf_bytes)) s->rc = CLOUDSC_EHIP;
    if (!s->rc) s->rc = cloudsc_gpu_check(s->device, NULL, CLOUDSC_VARIANT_KCACHE, NULL);   /* the expansion is done */
    const double k0 = now();
    if (!s->rc) s->rc = caller_step(s, variant, klev, &g, ws, &cml, &spp);
    if (!s->rc) s->rc = cloudsc_gpu_check(s->device, NULL, s->variant, ws);
    s->kernel_ms[r] = (float)(1e3 * (now() - k0));   /* launch to the check's return, on the host clock */
    timed += now() - k0;
  }
  s->t_end = s->t_start + timed;
  pthread_barrier_wait(s->barrier);
  if (!s->rc && tp && !inplace)   /* unpack BUFFER_LOC into the separate tendency_loc_* arrays the validation reads */
    s->rc = cloudsc_fields_convert_tendbuf(s->device, NULL, s->ngptot, klev, s->precision, s->nproma, tp, &loc_buf,
                                           s->precision, s->nproma, 0, &loc_sep);
  if (!s->rc && s->levels) s->rc = levels_convert(s, klev, 1, &f, s->nproma, &lev, 0);
  if (!s->rc && s->levels) s->rc = levels_convert(s, klev, 1, &lev, 0, &stage, s->nproma);
  const cloudsc_fields_t *vf = s->levels ? &stage : &f;   /* the separate arrays the validation reads */
  int member[CLOUDSC_NVALID];
#define VALID_MEMBER(n, N, k, d, i) CLOUDSC_IF_VALIDATED_##d(member[CLOUDSC_F_##N] = CLOUDSC_M_##n;)
  CLOUDSC_FIELDS(VALID_MEMBER)
#undef VALID_MEMBER
  if (s->advance > 1) {   /* --advance N > 1: nothing has a reference after more than one step */
    for (int id = 0; id < CLOUDSC_NVALID; id++) s->skipped[id] = 1;
  } else if (!s->rc && s->ref && (inplace || s->outputs != CLOUDSC_OUTPUTS_ALL)) {
    /* in place: BUFFER_LOC itself.  A prognostic set: the fields cloudsc_fields_alloc_outputs allocated -- the
     * library's selection, read off the set: a validated member it left NULL has no reference array either */
    cloudsc_reference_t ref = *s->ref;
    if (s->cml) {   /* 0 + loc: the cumulative planes validate as tendency_loc_* (the untouched vapour plane as zeros) */
      g.tendency_loc_t = cml.t; g.tendency_loc_a = cml.a; g.tendency_loc_q = cml.q; g.tendency_loc_cld = cml.cld;
    }
    for (int id = 0; id < CLOUDSC_NVALID; id++)
      if (!((const void *const *)vf)[member[id]]) { ref.field[id] = NULL; s->skipped[id] = 1; }
    s->rc = cloudsc_fields_validate_tendbuf(s->device, NULL, s->precision, s->ngptot, s->nproma, klev, inplace ? tp : 0,
                                            s->outputs, s->col_offset, inplace ? &g : vf, &ref, s->stats);
  } else if (!s->rc && s->ref)
    s->rc = cloudsc_fields_validate(s->device, NULL, s->precision, s->ngptot, s->nproma, klev, s->col_offset, vf, s->ref,
                                    s->stats);
  /* --advance: the local tendencies are not stored (their arrays hold what the allocation left): no row, not gated */
  for (int id = 0; s->advance && id < CLOUDSC_NVALID; id++)
    if (member[id] >= CLOUDSC_M_tendency_loc_t && member[id] <= CLOUDSC_M_tendency_loc_cld) s->skipped[id] = 1;
  if (s->rc) snprintf(s->err, sizeof(s->err), "%s", cloudsc_last_hip_error());
  if (ws) dfree(ws);
  if (buf_tmp) dfree(buf_tmp);
  if (buf_loc) dfree(buf_loc);
  if (buf_cml) dfree(buf_cml);
  if (spp_ones) dfree(spp_ones);
  cloudsc_fields_free(s->device, &f);
  cloudsc_fields_free(s->device, &stage);
  cloudsc_fields_free(s->device, &lev);
}

/* ---- --fields caller --batch N: N caller-owned sets of ngptot / N columns each, set i expanded from the template's
 * columns at col_offset + i * (ngptot / N), all of them stepped by one cloudsc_gpu_run_batch per rep under the
 * device's parameter set, each validated on the device and the statistics combined (double-double sums): the
 * table of one set of ngptot columns. ---- */
static void shard_batch(shard_t *s) {
  const int klev = s->tmpl->klev, n = s->batch, per = s->ngptot / n;
  const int alloc_flags = (s->place_on ? 0 : CLOUDSC_PLACE_NONE) | (s->aerosols ? CLOUDSC_ALLOC_AEROSOLS : 0);
  cloudsc_fields_t *f = (cloudsc_fields_t *)calloc((size_t)n, sizeof(*f));
  cloudsc_batch_t *batch = NULL;
  int nalloc = 0;
  s->rc = f ? CLOUDSC_OK : CLOUDSC_ENOMEM;
  for (int i = 0; i < n && !s->rc; i++) {
    s->rc = cloudsc_fields_alloc_outputs(s->device, s->precision, per, s->nproma, klev, alloc_flags, s->outputs, &f[i],
                                         &s->place);
    if (!s->rc) nalloc = i + 1;
    if (!s->rc)
      s->rc = cloudsc_fields_expand(s->device, NULL, s->precision, per, s->nproma, s->col_offset + (long long)i * per,
                                    s->tmpl, &f[i]);
  }
  if (!s->rc)
    s->rc = cloudsc_batch_create(&batch, s->device, s->precision, s->outputs, n, per, s->nproma, klev, f, NULL);
  /* plude is INOUT: expanded again before every step, outside the timing */
  for (int r = 0; r < s->warmup + s->reps; r++) {
    const int timed = r >= s->warmup;
    if (r == s->warmup) { pthread_barrier_wait(s->barrier); s->t_start = s->t_end = now(); }
    for (int i = 0; i < n && !s->rc && r; i++) {
      cloudsc_fields_t plude;
      memset(&plude, 0, sizeof(plude));
      plude.plude = f[i].plude;
      s->rc = cloudsc_fields_expand(s->device, NULL, s->precision, per, s->nproma, s->col_offset + (long long)i * per,
                                    s->tmpl, &plude);
    }
    if (!s->rc) s->rc = cloudsc_gpu_check(s->device, NULL, CLOUDSC_VARIANT_KCACHE, NULL);   /* the expansion is done */
    const double k0 = now();
    if (!s->rc) s->rc = cloudsc_gpu_run_batch(batch, NULL, s->variant);
    if (!s->rc) s->rc = cloudsc_gpu_check(s->device, NULL, CLOUDSC_VARIANT_KCACHE, NULL);
    if (timed) {
      s->kernel_ms[r - s->warmup] = (float)(1e3 * (now() - k0));   /* launch to the check's return, on the host clock */
      s->t_end += now() - k0;
    }
  }
  if (!s->reps) { pthread_barrier_wait(s->barrier); s->t_start = s->t_end = now(); }
  pthread_barrier_wait(s->barrier);
  int member[CLOUDSC_NVALID];
#define VALID_MEMBER(n, N, k, d, i) CLOUDSC_IF_VALIDATED_##d(member[CLOUDSC_F_##N] = CLOUDSC_M_##n;)
  CLOUDSC_FIELDS(VALID_MEMBER)
#undef VALID_MEMBER
  for (int i = 0; i < n && !s->rc && s->ref; i++) {
    /* a validated member the selection left NULL has no reference array either (as shard_caller) */
    cloudsc_reference_t ref = *s->ref;
    cloudsc_stats_t st[CLOUDSC_NVALID];
    memset(st, 0, sizeof(st));
    for (int id = 0; id < CLOUDSC_NVALID; id++)
      if (!((const void *const *)&f[i])[member[id]]) { ref.field[id] = NULL; s->skipped[id] = 1; }
    if (s->outputs != CLOUDSC_OUTPUTS_ALL)
      s->rc = cloudsc_fields_validate_tendbuf(s->device, NULL, s->precision, per, s->nproma, klev, 0, s->outputs,
                                              s->col_offset + (long long)i * per, &f[i], &ref, st);
    else
      s->rc = cloudsc_fields_validate(s->device, NULL, s->precision, per, s->nproma, klev,
                                      s->col_offset + (long long)i * per, &f[i], s->ref, st);
    for (int id = 0; id < CLOUDSC_NVALID && !s->rc; id++) {
      if (i == 0) s->stats[id] = st[id];
      else cloudsc_stats_combine(&s->stats[id], &st[id]);
    }
  }
  if (s->rc) snprintf(s->err, sizeof(s->err), "%s", cloudsc_last_hip_error());
  if (batch) cloudsc_batch_destroy(batch);
  for (int i = 0; i < nalloc; i++) cloudsc_fields_free(s->device, &f[i]);
  free(f);
}

static void *shard_main(void *arg) {
  shard_t *s = (shard_t *)arg;
  if (s->batch) { shard_batch(s); return NULL; }
  if (s->caller) { shard_caller(s); return NULL; }
  cloudsc_gpu_state_t *st = NULL;
  s->rc = cloudsc_state_create(&st, s->device, s->precision, s->ngptot, s->nproma, s->col_offset, s->tmpl,
                               s->params);
  if (!s->rc) s->rc = cloudsc_state_placement_report(st, &s->place);
  if (!s->rc && s->warmup > 0) {
    float *w = (float *)malloc(sizeof(float) * s->warmup);
    s->rc = w ? cloudsc_state_run(st, s->variant | s->libm_bit, s->warmup, w) : CLOUDSC_ENOMEM;
    free(w);
  }
  if (!s->rc) s->rc = cloudsc_state_sync(st);
  /* every shard reaches the barrier, also after an error, so nobody waits forever */
  pthread_barrier_wait(s->barrier);
  s->t_start = now();
  if (!s->rc) s->rc = cloudsc_state_run(st, s->variant | s->libm_bit, s->reps, s->kernel_ms);
  if (!s->rc) s->rc = cloudsc_state_sync(st);
  s->t_end = now();
  pthread_barrier_wait(s->barrier);
  /* untimed; every launch is the same step (plude is taken out of place), so
   * the validation below still checks the timed step's results */
  if (!s->rc && s->energy_s > 0.0) s->rc = energy_window(s, st);
  if (!s->rc && s->ref) s->rc = cloudsc_state_validate(st, s->ref, s->stats);
  if (s->rc) snprintf(s->err, sizeof(s->err), "%s", cloudsc_last_hip_error());
  if (st) cloudsc_state_destroy(st);
  return NULL;
}

/* ERROR_PRINT (validate_mod.F90:263-296 / cloudsc_validate.c:20-44) */
static double print_error(const char *name, int ndim, const cloudsc_stats_t *s, int ngptot) {
  const double eps = DBL_EPSILON;
  double rel;
  int iopt;
  if (s->errsum < eps) { rel = 0.0; iopt = 1; }
  else if (s->refsum < eps) { rel = s->errsum / (1.0 + s->refsum); iopt = 2; }
  else { rel = s->errsum / s->refsum; iopt = 3; }
  printf(" %20s %dD%d %20.13le %20.13le %20.13le %20.13le %20.13le %s\n", name, ndim, iopt, s->minval, s->maxval,
         s->maxerr, s->errsum / (double)ngptot, 100.0 * rel, rel > 10.0 * eps ? " !!!!" : "     ");
  return rel;
}

/* a precision code's name and the bytes of its real field elements in memory */
static const char *precision_name(int precision) {
  return precision == CLOUDSC_FP64 ? "fp64" : precision == CLOUDSC_MIXED ? "mixed" : "fp32";
}
static int precision_bytes(int precision) { return precision == CLOUDSC_FP64 ? 8 : 4; }

/* ---- host-memory paths: --transfer (GPU, H2D/D2H per chunk) and --variant cpu ---- */
/* from the inventory (cloudsc_fields.def): cloudsc_io input index and validated field id ->
 * cloudsc_fields_t member index; the kind of every output member (-1 for the others) */
#define INPUT_FIELD(n, N, k, d, i) CLOUDSC_IF_TEMPLATE_##d([CLOUDSC_T_##n] = CLOUDSC_M_##n, )
#define VALID_FIELD(n, N, k, d, i) CLOUDSC_IF_VALIDATED_##d([CLOUDSC_F_##N] = CLOUDSC_M_##n, )
#define OUT_KIND(n, N, k, d, i) CLOUDSC_FD_##d == CLOUDSC_FD_OUT ? CLOUDSC_FK_##k : -1,
static const int k_input_field[CLOUDSC_IO_NIN] = {CLOUDSC_FIELDS(INPUT_FIELD)};
static const int k_valid_field[CLOUDSC_NVALID] = {CLOUDSC_FIELDS(VALID_FIELD)};
static const int k_out_kind[CLOUDSC_NFIELDS] = {CLOUDSC_FIELDS(OUT_KIND)};

static int run_host(const options_t *o, const cloudsc_dataset_t *ds) {
  const int cpu = o->variant == VARIANT_CPU;
  const int es = precision_bytes(o->precision);
  /* the zinfo record: cloudsc_cpu_run_threads, fp64 (cloudsc_cpu_run_outputs, --outputs surface, keeps none) */
  const int per_thread = cpu && o->precision == CLOUDSC_FP64 && o->outputs != CLOUDSC_OUTPUTS_SURFACE && !o->spp &&
                         !o->advance;
  const int nb = o->ngptot / o->nproma + (o->ngptot % o->nproma ? 1 : 0);
  const int aer = ds->params.laericesed || ds->params.laericeauto;
  cloudsc_fields_t f;
  memset(&f, 0, sizeof(f));
  void **fp = (void **)&f;
  size_t host_bytes = 0;
  double *plude0 = NULL;
  int rc = CLOUDSC_OK;
  /* inputs: expanded on the host (load_state.c) */
  for (int i = 0; i < CLOUDSC_IO_NIN && !rc; i++) {
    const int kind = cloudsc_io_input_kind[i];
    const void *src = i == CLOUDSC_IO_KTYPE ? (const void *)ds->ktype : (const void *)ds->in[i];
    if (!src || (i >= CLOUDSC_IO_FIRST_AEROSOL && !aer)) continue;
    const int is_int = i == CLOUDSC_IO_KTYPE;
    const size_t n = (size_t)nb * (size_t)(cloudsc_io_elems(kind, ds->klev, o->nproma));
    const size_t bytes = n * (is_int ? sizeof(int) : (size_t)es);
    void *dst = aligned_alloc(4096, (bytes + 4095) & ~(size_t)4095);
    if (!dst) { rc = CLOUDSC_ENOMEM; break; }
    cloudsc_io_expand(src, kind, is_int, ds->klev, ds->klon, o->ngptot, o->nproma, 0, is_int ? 4 : es, dst);
    fp[k_input_field[i]] = dst;
    host_bytes += bytes;
    if (i == CLOUDSC_T_plude) {
      plude0 = (double *)malloc(bytes);
      if (!plude0) { rc = CLOUDSC_ENOMEM; break; }
      memcpy(plude0, dst, bytes);
    }
  }
  /* --outputs surface (--variant cpu): the ten diagnostic fluxes are not allocated, the four others are surface fields */
  const int surface = cpu && o->outputs == CLOUDSC_OUTPUTS_SURFACE;
  for (int m = 0; m < CLOUDSC_NFIELDS && !rc; m++) {
    if (k_out_kind[m] < 0) continue;
    if (surface && m >= CLOUDSC_M_pfsqlf && m <= CLOUDSC_M_pfsqitur) continue;
    const int okind = surface && m >= CLOUDSC_M_pfplsl && m <= CLOUDSC_M_pfhpsn ? CLOUDSC_FK_SURFACE : k_out_kind[m];
    const size_t bytes = (size_t)nb * (size_t)cloudsc_io_elems(okind, ds->klev, o->nproma) * es;
    void *dst = aligned_alloc(4096, (bytes + 4095) & ~(size_t)4095);
    if (!dst) { rc = CLOUDSC_ENOMEM; break; }
    memset(dst, 0xff, bytes);            /* NaN: the callee must write every element */
    fp[m] = dst;
    host_bytes += bytes;
  }
  const size_t plude_bytes = (size_t)nb * ds->klev * o->nproma * es;
  /* --spp unit (--variant cpu): one surface field of ones behind all five members */
  void *spp_ones = NULL;
  cloudsc_spp_t spp;
  memset(&spp, 0, sizeof(spp));
  if (!rc && cpu && o->spp) {
    const size_t n = (size_t)nb * (size_t)o->nproma;
    spp_ones = malloc(n * (size_t)es);
    if (!spp_ones) rc = CLOUDSC_ENOMEM;
    for (size_t i = 0; spp_ones && i < n; i++) {
      if (es == 8) ((double *)spp_ones)[i] = 1.0;
      else ((float *)spp_ones)[i] = 1.0f;
    }
    spp.ramid = spp.rcldiff = spp.rclcrit = spp.rlcritsnow = spp.rpecons = spp_ones;
  }
  cloudsc_host_pipeline_t *pipe = NULL;
  if (!rc && !cpu) rc = cloudsc_gpu_init(0, &ds->params);
  if (!rc && !cpu) rc = cloudsc_host_pipeline_create(&pipe, 0, o->precision, o->ngptot, o->nproma, ds->klev,
                                                     o->chunk_blocks, o->nstreams, &f);
  double total_ms = 0.0;
  /* --variant cpu: the per-thread record of the C dwarf (zinfo), summed over the timed steps */
  const int nth = o->numomp;
  double *th_s = cpu ? (double *)calloc((size_t)nth, sizeof(double)) : NULL;
  double *th_step = cpu ? (double *)calloc((size_t)nth, sizeof(double)) : NULL;
  int *th_blk = cpu ? (int *)calloc((size_t)nth, sizeof(int)) : NULL;
  int *th_col = cpu ? (int *)calloc((size_t)nth, sizeof(int)) : NULL;
  int *th_blk_step = cpu ? (int *)calloc((size_t)nth, sizeof(int)) : NULL;
  int *th_col_step = cpu ? (int *)calloc((size_t)nth, sizeof(int)) : NULL;
  if (cpu && (!th_s || !th_step || !th_blk || !th_col || !th_blk_step || !th_col_step)) rc = CLOUDSC_ENOMEM;
  for (int r = 0; r < o->warmup + o->reps && !rc; r++) {
    memcpy(f.plude, plude0, plude_bytes);                 /* INOUT restored, outside the timing */
    double ms = 0.0;
    if (cpu) {
      double secs = 0.0;
      if (o->advance) {   /* --advance N: in place */
        const cloudsc_advance_t adv = {(void *)f.pt, (void *)f.pq, (void *)f.pa, (void *)f.pclv};
        const double t0 = now();
        rc = cloudsc_cpu_run_advance(nth, o->precision, o->outputs, o->ngptot, o->nproma, ds->klev, &ds->params, &f, &adv);
        secs = now() - t0;
      } else if (o->spp) {
        const double t0 = now();
        rc = cloudsc_cpu_run_spp(nth, o->precision, o->outputs, o->ngptot, o->nproma, ds->klev, &ds->params, &f, &spp);
        secs = now() - t0;
      } else if (surface)
        rc = cloudsc_cpu_run_outputs(nth, o->precision, o->outputs, o->ngptot, o->nproma, ds->klev, &ds->params, &f);
      else if (per_thread)
        rc = cloudsc_cpu_run_threads(nth, o->ngptot, o->nproma, ds->klev, &ds->params, &f, &secs, th_step,
                                     th_blk_step, th_col_step);
      else
        rc = cloudsc_cpu_run_precision(nth, o->precision, o->ngptot, o->nproma, ds->klev, &ds->params, &f, &secs);
      ms = 1e3 * secs;
      if (r >= o->warmup)
        for (int t = 0; t < nth; t++) { th_s[t] += th_step[t]; th_blk[t] += th_blk_step[t]; th_col[t] += th_col_step[t]; }
    } else {
      rc = cloudsc_host_pipeline_run(pipe, o->variant | (o->exact_libm ? CLOUDSC_FP32_EXACT_LIBM : 0), &ms);
    }
    if (r >= o->warmup) total_ms += ms;
  }
  if (pipe) cloudsc_host_pipeline_destroy(pipe);
  int bad = 0;
  if (!rc) {
    const double t = 1e-3 * total_ms;
    const double cols = (double)o->ngptot * o->reps;
    printf("     NUMOMP=%d, NGPTOT=%d, NPROMA=%d, NGPBLKS=%d\n", o->numomp, o->ngptot, o->nproma, nb);
    printf(" Reference MFLOP count for 100 columns : %12.8f\n", 1.0e-06 * ZHPM);
    printf(" %10s%10s%10s%10s%10s %4s : %10s%10s%10s\n", "NUMOMP", "NGPTOT", "#GP-cols", "#BLKS", "NPROMA",
           "tid#", "Time(msec)", "MFlops/s", "col/s");
    /* per-thread rows (cloudsc_driver.c:238-253): columns and blocks of the last
     * step; time, MFlops/s and col/s over all timed steps like the TOTAL row */
    for (int t = 0; per_thread && t < nth; t++) {
      const double tl = th_s[t], zfrac = (double)th_col[t] / cols;
      printf(" %10d%10d%10d%10d%10d %4d : %10d%10d%10d @ core#\n", o->numomp, o->ngptot, th_col_step[t],
             th_blk_step[t], o->nproma, t, (int)(tl * 1000.),
             tl > 0 ? (int)(1.0e-06 * zfrac * ZHPM * (cols / 100.) / tl) : 0, tl > 0 ? (int)(cols / tl) : 0);
    }
    printf(" %10d%10d%10d%10d%10d %4d : %10d%10d%10d TOTAL\n", o->numomp, o->ngptot, o->ngptot, nb, o->nproma, -1,
           (int)(t * 1000.), (int)(1.0e-06 * ZHPM * (cols / 100.) / t), (int)(cols / t));
    if (cpu)
      printf(" TIMING: steps=%d cpu_ms_per_step=%.4f columns_per_s=%.1f host_bytes=%zu threads=%d "
             "(cloudsc_cpu_run, host cores)\n",
             o->reps, total_ms / o->reps, cols / t, host_bytes, o->numomp);
    else
      printf(" TIMING: steps=%d transfer_ms_per_step=%.4f columns_per_s=%.1f host_bytes=%zu chunk_blocks=%d "
             "streams=%d (H2D + kernel + D2H, pinned host memory)\n",
             o->reps, total_ms / o->reps, cols / t, host_bytes, o->chunk_blocks, o->nstreams);
    if (ds->has_reference) {
      printf(" %20s %s %20s %20s %20s %20s %20s\n", "Variable", "Dim", "MinValue", "MaxValue", "AbsMaxErr",
             "AvgAbsErr/GP", "MaxRelErr-%");
      const int gate = o->precision == CLOUDSC_FP64 || o->tol_given;
      double worst = 0.0;
      for (int v = 0; v < CLOUDSC_NVALID; v++) {
        cloudsc_stats_t st;
        int kind = cloudsc_io_ref_kind[v];
        const double *refv = ds->ref[v];
        if (!fp[k_valid_field[v]]) continue;   /* --outputs surface: not allocated, not computed: no row */
        /* --advance: the tendencies are not stored; after more than one step nothing has a reference */
        if (o->advance > 1 || (o->advance && k_valid_field[v] >= CLOUDSC_M_tendency_loc_t &&
                               k_valid_field[v] <= CLOUDSC_M_tendency_loc_cld))
          continue;
        if (surface && k_valid_field[v] >= CLOUDSC_M_pfplsl && k_valid_field[v] <= CLOUDSC_M_pfhpsn) {
          refv += (size_t)ds->klev * ds->klon;   /* the surface row of the reference profile */
          kind = CLOUDSC_FK_SURFACE;
        }
        cloudsc_io_field_stats(refv, kind, ds->klev, ds->klon, fp[k_valid_field[v]], es, o->ngptot,
                               o->nproma, 0, &st);
        const double rel = print_error(cloudsc_io_print_names[v], kind == 3 ? 1 : kind == 2 ? 3 : 2, &st,
                                       o->ngptot);
        if (rel > worst) worst = rel;
        if (gate && !(rel <= o->tol)) bad++;
      }
      if (gate)
        printf(" VALIDATION: %s (worst relative L1 error %.3e, gate %.1e, %d field(s) over)\n",
               bad ? "FAILED" : "PASSED", worst, o->tol, bad);
      else
        printf(" VALIDATION: reported only (%s vs the fp64 reference; worst relative L1 error %.3e)\n",
               precision_name(o->precision), worst);
    }
    if (o->advance)
      printf(" ADVANCE: steps=%d ms_per_step=%.4f in place (cloudsc_cpu_run_advance: pt, pq, pa, pclv rewritten)%s\n",
             o->advance, total_ms / o->reps, o->advance > 1 ? "; nothing validated after more than one step" : "");
  } else {
    fprintf(stderr, "dwarf-cloudsc-amd %s: %s (%s)\n", cpu ? "--variant cpu" : "--transfer", cloudsc_strerror(rc),
            cloudsc_last_hip_error());
  }
  for (int i = 0; i < CLOUDSC_NFIELDS; i++) free(fp[i]);
  free(plude0);
  free(spp_ones);
  free(th_s); free(th_step); free(th_blk); free(th_col); free(th_blk_step); free(th_col_step);
  return rc ? EXIT_FAILURE : (bad ? EXIT_FAILURE : EXIT_SUCCESS);
}

int main(int argc, char **argv) {
  options_t o;
  if (parse(argc, argv, &o)) { usage(argv[0]); return EXIT_FAILURE; }

  /* ---- load the KLON-column state (HDF5 read-only, else raw) ---- */
  cloudsc_dataset_t ds;
  int rc;
  const char *in_h5 = o.input_h5 ? o.input_h5 : (exists("input.h5") ? "input.h5" : NULL);
  if (in_h5) {
    const char *ref_h5 = o.reference_h5 ? o.reference_h5 : (exists("reference.h5") ? "reference.h5" : NULL);
    rc = cloudsc_io_load_hdf5(in_h5, ref_h5, &ds);
  } else {
    char dir[PATH_MAX];
    if (o.data_dir) snprintf(dir, sizeof(dir), "%s", o.data_dir);
    else default_data_dir(dir, sizeof(dir));
    rc = cloudsc_io_load_dir(dir, 1, &ds);
    if (!rc && o.reference_h5) {
      rc = cloudsc_io_load_hdf5_reference(o.reference_h5, &ds);     /* raw inputs, HDF5 reference */
      if (!rc) {
        size_t n = strlen(ds.source);
        snprintf(ds.source + n, sizeof(ds.source) - n, " + HDF5 %s (read-only)", o.reference_h5);
      }
    }
  }
  if (rc) {
    fprintf(stderr, "dwarf-cloudsc-amd: cannot load the input state: %s (%s)\n", cloudsc_strerror(rc),
            cloudsc_io_last_error());
    return EXIT_FAILURE;
  }
  if (o.write_h5_dir) {
    char a[PATH_MAX], b[PATH_MAX];
    snprintf(a, sizeof(a), "%s/input.h5", o.write_h5_dir);
    snprintf(b, sizeof(b), "%s/reference.h5", o.write_h5_dir);
    rc = cloudsc_io_write_hdf5(&ds, a, ds.has_reference ? b : NULL);
    if (rc) fprintf(stderr, "write failed: %s\n", cloudsc_io_last_error());
    else printf(" wrote %s%s%s\n", a, ds.has_reference ? " and " : "", ds.has_reference ? b : "");
    cloudsc_io_free(&ds);
    return rc ? EXIT_FAILURE : EXIT_SUCCESS;
  }

  if (o.tend_planes && o.fields_caller != 2 && o.fields_caller != 3 && o.fields_caller != 4) {
    fprintf(stderr, "dwarf-cloudsc-amd: --tend-planes goes with --fields tendbuf\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  /* (--outputs surface alone with --variant cpu: the host step, run_host) */
  const int cpu_surface = o.outputs_given && o.outputs == CLOUDSC_OUTPUTS_SURFACE && o.variant == VARIANT_CPU &&
                          !o.fields_caller && !o.transfer && !o.exact_libm;
  if (o.outputs_given && !cpu_surface &&
      (!o.fields_caller || o.transfer || o.exact_libm ||
       (o.variant != CLOUDSC_VARIANT_KSEG && o.variant != CLOUDSC_VARIANT_KCACHE))) {
    fprintf(stderr, "dwarf-cloudsc-amd: --outputs goes with --fields caller|tendbuf|tendbuf-inplace and --variant "
                    "kseg|kcache (no --transfer, no --fp32-exact-libm)\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.fields_caller == 4 && (!o.outputs_given || o.outputs == CLOUDSC_OUTPUTS_ALL)) {
    fprintf(stderr, "dwarf-cloudsc-amd: --fields tendbuf-cml needs --outputs prognostic|surface\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.fields_caller == 4 && o.exact_libm) {
    fprintf(stderr, "dwarf-cloudsc-amd: --fields tendbuf-cml has no --fp32-exact-libm form\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.fields_caller == 3 && o.exact_libm) {
    fprintf(stderr, "dwarf-cloudsc-amd: --fields tendbuf-inplace has no --fp32-exact-libm form\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.fields_caller >= 2 && (o.transfer || (o.variant != CLOUDSC_VARIANT_KSEG && o.variant != CLOUDSC_VARIANT_KCACHE))) {
    fprintf(stderr, "dwarf-cloudsc-amd: --fields tendbuf runs --variant kseg|kcache on device fields (no --transfer, "
                    "no cpu, scc or scc-private)\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.fields_levels && (o.transfer || (o.variant != CLOUDSC_VARIANT_KSEG && o.variant != CLOUDSC_VARIANT_KCACHE))) {
    fprintf(stderr, "dwarf-cloudsc-amd: --fields levels runs --variant kseg|kcache on device fields (no --transfer, "
                    "no cpu, scc or scc-private)\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  /* --spp: the per-column multiplier form exists for --fields caller|levels on kseg|kcache and for --variant cpu,
   * with --outputs all|prognostic: everything else is a usage error, never another step in its place */
  if (o.spp) {
    const int cpu = o.variant == VARIANT_CPU;
    const int gpu_ok = o.fields_caller == 1 && (o.variant == CLOUDSC_VARIANT_KSEG || o.variant == CLOUDSC_VARIANT_KCACHE);
    if (o.transfer || o.exact_libm || o.outputs == CLOUDSC_OUTPUTS_SURFACE || (cpu ? o.fields_caller != 0 : !gpu_ok)) {
      fprintf(stderr, "dwarf-cloudsc-amd: --spp goes with --fields caller|levels and --variant kseg|kcache, or with "
                      "--variant cpu (no --transfer, no --fp32-exact-libm, no --outputs surface, no tendency buffers)\n");
      cloudsc_io_free(&ds);
      return EXIT_FAILURE;
    }
  }
  /* --advance: the advancing form exists for --fields caller on kseg|kcache and for --variant cpu, with the
   * outputs all|surface: everything else is a usage error, never another step in its place.  Its N steps are the
   * timed steps: no warm-up step moves the state first */
  if (o.advance) {
    const int cpu = o.variant == VARIANT_CPU;
    const int gpu_ok = o.fields_caller == 1 && !o.fields_levels &&
                       (o.variant == CLOUDSC_VARIANT_KSEG || o.variant == CLOUDSC_VARIANT_KCACHE);
    if (o.transfer || o.exact_libm || o.spp || o.outputs == CLOUDSC_OUTPUTS_PROGNOSTIC || o.energy_s > 0.0 ||
        (cpu ? o.fields_caller != 0 : !gpu_ok)) {
      fprintf(stderr, "dwarf-cloudsc-amd: --advance goes with --fields caller and --variant kseg|kcache, or with "
                      "--variant cpu (--outputs all|surface; no --transfer, --fp32-exact-libm, --spp, --energy, no "
                      "tendency buffers)\n");
      cloudsc_io_free(&ds);
      return EXIT_FAILURE;
    }
    o.reps = o.advance;
    o.warmup = 0;
  }
  /* --batch: N plain caller-owned sets in one KCACHE launch on one device; everything else is a usage error, never
   * another step in its place */
  if (o.batch && (o.fields_caller != 1 || o.fields_levels || o.variant != CLOUDSC_VARIANT_KCACHE || o.transfer ||
                  o.exact_libm || o.spp || o.advance || o.ngpus != 1 || o.energy_s > 0.0 ||
                  (long long)o.batch * o.ngptot > INT_MAX)) {
    fprintf(stderr, "dwarf-cloudsc-amd: --batch goes with --fields caller and --variant kcache (one device; no --spp, "
                    "--advance, --transfer, --fp32-exact-libm or --energy)\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.fields_caller >= 2 && !o.tend_planes) o.tend_planes = CLOUDSC_TENDBUF_PLANES_MIN;
  if (o.fields_caller && (o.transfer || o.variant == VARIANT_CPU)) {
    fprintf(stderr, "dwarf-cloudsc-amd: --fields caller runs the GPU variants on device fields (no --transfer, no "
                    "--variant cpu)\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.variant == VARIANT_CPU) {
    if (o.precision == CLOUDSC_FP32 || o.ngpus != 1 || o.transfer) {
      fprintf(stderr, "dwarf-cloudsc-amd: --variant cpu runs fp64 or mixed on the host (no --gpus/--transfer/fp32)\n");
      cloudsc_io_free(&ds);
      return EXIT_FAILURE;
    }
    printf(" CLOUDSC-AMD: %s, variant cpu (cloudsc_cpu_run, %d host thread(s)); state: %s\n",
           precision_name(o.precision), o.numomp, ds.source);
    if (o.energy_s > 0.0) printf(" ENERGY: n/a (host variant: no GPU board power)\n");
    rc = run_host(&o, &ds);
    cloudsc_io_free(&ds);
    return rc;
  }

  int ndev = 0;
  if ((rc = cloudsc_gpu_device_count(&ndev)) || ndev <= 0) {
    fprintf(stderr, "dwarf-cloudsc-amd: no HIP device (%s)\n", rc ? cloudsc_strerror(rc) : "0 devices");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.ngpus > ndev)
    printf(" CLOUDSC-AMD: %d shards on %d visible device(s): shard d runs on device d %% %d\n", o.ngpus, ndev, ndev);

  cloudsc_debug_set_narrow_pack(o.narrow_pack);
  if (o.precision == CLOUDSC_MIXED &&
      (o.transfer || (o.variant != CLOUDSC_VARIANT_KSEG && o.variant != CLOUDSC_VARIANT_KCACHE))) {
    fprintf(stderr, "dwarf-cloudsc-amd: --precision mixed runs --variant kseg|kcache|cpu (no --transfer)\n");
    cloudsc_io_free(&ds);
    return EXIT_FAILURE;
  }
  if (o.transfer) {
    printf(" CLOUDSC-AMD: %s, variant %s, host-buffer path (--transfer), 1 device; state: %s\n",
           precision_name(o.precision),
           variant_name(o.variant),
           ds.source);
    if (o.energy_s > 0.0) printf(" ENERGY: n/a (the host-buffer path is bound by PCIe; run without --transfer)\n");
    rc = run_host(&o, &ds);
    cloudsc_io_free(&ds);
    return rc;
  }

  cloudsc_template_t tmpl;
  cloudsc_reference_t ref;
  cloudsc_io_template(&ds, &tmpl);
  cloudsc_io_reference(&ds, &ref);
  /* --batch N: from here on NGPTOT is the columns of the N sets together, NGPBLKS their blocks */
  const int set_cols = o.ngptot;
  if (o.batch) o.ngptot *= o.batch;
  const int nblocks = (o.batch ? o.batch : 1) * (set_cols / o.nproma + (set_cols % o.nproma ? 1 : 0));
  /* NPROMA blocks per wave of the launches (1 = unpacked; narrow blocks: --narrow-pack) */
  cloudsc_launch_geometry_t geo;
  if (cloudsc_gpu_launch_geometry(o.precision, o.variant, set_cols, o.nproma, ds.klev,
                                  ds.params.laericesed || ds.params.laericeauto, &geo) != CLOUDSC_OK)
    geo.pack = 1;
  printf(" CLOUDSC-AMD: %s, variant %s, %d device(s); state: %s (KLON=%d, KLEV=%d); pack=%d\n",
         o.precision == CLOUDSC_FP32 && o.exact_libm ? "fp32 (glibc expf/powf)" : precision_name(o.precision),
         variant_name(o.variant),
         o.ngpus, ds.source, ds.klon, ds.klev, geo.pack);

  /* the placement search costs ~0.5 s of kernel launches per state and saves
   * up to ~15 % per step: worth it for repeated steps, not for one (the
   * reference times a single launch, cloudsc_driver.cu:389-422) */
  const int place = o.place >= 0 ? o.place : o.reps > 1;
  cloudsc_set_placement_search(place ? -1 : 0);

  /* ---- shard: block-aligned contiguous ranges of the global column index ---- */
  shard_t *sh = (shard_t *)calloc((size_t)o.ngpus, sizeof(shard_t));
  pthread_t *th = (pthread_t *)calloc((size_t)o.ngpus, sizeof(pthread_t));
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, NULL, (unsigned)o.ngpus);
  const int blocks_per = nblocks / o.ngpus, extra = nblocks % o.ngpus;
  long long col = 0;
  int nused = 0;
  for (int d = 0; d < o.ngpus; d++) {
    const int nb = blocks_per + (d < extra ? 1 : 0);
    long long cols = (long long)nb * o.nproma;
    if (col + cols > o.ngptot) cols = o.ngptot - col;
    if (cols <= 0) break;
    shard_t *s = &sh[nused++];
    s->device = d % ndev; s->ngptot = (int)cols; s->col_offset = col; s->nproma = o.nproma;
    s->precision = o.precision; s->variant = o.variant; s->reps = o.reps; s->warmup = o.warmup;
    s->libm_bit = o.exact_libm ? CLOUDSC_FP32_EXACT_LIBM : 0;
    s->energy_s = o.energy_s;
    s->caller = o.fields_caller; s->place_on = place; s->levels = o.fields_levels;
    s->tend_planes = o.fields_caller >= 2 ? o.tend_planes : 0;
    s->inplace = o.fields_caller == 3 || o.fields_caller == 4;
    s->cml = o.fields_caller == 4;
    s->outputs = o.outputs;
    s->spp = o.spp;
    s->advance = o.advance;
    s->batch = o.batch;
    s->aerosols = ds.params.laericesed || ds.params.laericeauto;
    s->tmpl = &tmpl; s->params = &ds.params; s->ref = ds.has_reference ? &ref : NULL; s->barrier = &bar;
    s->kernel_ms = (float *)calloc((size_t)o.reps, sizeof(float));
    col += cols;
  }
  if (nused != o.ngpus) {
    pthread_barrier_destroy(&bar);
    pthread_barrier_init(&bar, NULL, (unsigned)nused);
  }
  /* --fields caller launches with the devices' default parameter sets (cloudsc_gpu_run) */
  for (int d = 0; d < nused && d < ndev && o.fields_caller; d++)
    if ((rc = cloudsc_gpu_init(sh[d].device, &ds.params))) {
      fprintf(stderr, "dwarf-cloudsc-amd: cloudsc_gpu_init: %s (%s)\n", cloudsc_strerror(rc), cloudsc_last_hip_error());
      cloudsc_io_free(&ds);
      return EXIT_FAILURE;
    }
  for (int d = 0; d < nused; d++) pthread_create(&th[d], NULL, shard_main, &sh[d]);
  for (int d = 0; d < nused; d++) pthread_join(th[d], NULL);
  pthread_barrier_destroy(&bar);

  int failed = 0;
  for (int d = 0; d < nused; d++)
    if (sh[d].rc) {
      fprintf(stderr, "dwarf-cloudsc-amd: shard %d (device %d): %s (%s)\n", d, sh[d].device,
              cloudsc_strerror(sh[d].rc), sh[d].err);
      failed = 1;
    }
  if (failed) { cloudsc_io_free(&ds); return EXIT_FAILURE; }

  /* ---- timing table (cloudsc_driver.c:233-262) ---- */
  double t0 = sh[0].t_start, t1 = sh[0].t_end;
  for (int d = 1; d < nused; d++) {
    if (sh[d].t_start < t0) t0 = sh[d].t_start;
    if (sh[d].t_end > t1) t1 = sh[d].t_end;
  }
  const double tdiff = t1 - t0;
  const double cols_done = (double)o.ngptot * o.reps;
  printf("     NUMOMP=%d, NGPTOT=%d, NPROMA=%d, NGPBLKS=%d\n", o.numomp, o.ngptot, o.nproma, nblocks);
  printf(" Reference MFLOP count for 100 columns : %12.8f\n", 1.0e-06 * ZHPM);
  printf(" %10s%10s%10s%10s%10s %4s : %10s%10s%10s\n", "NUMOMP", "NGPTOT", "#GP-cols", "#BLKS", "NPROMA", "tid#",
         "Time(msec)", "MFlops/s", "col/s");
  /* one row per shard, as the reference GPU driver prints one per host thread
   * (cloudsc_driver.cu:462-477): tid# = the shard (its host thread), and the row
   * ends in "@ core#" exactly as there, so JUBE's thr_time/thr_mflops patterns
   * (benchmark/include/include_patternset.yml:161-162) match it */
  for (int d = 0; d < nused; d++) {
    const double tl = sh[d].t_end - sh[d].t_start;
    const int nbd = sh[d].ngptot / o.nproma + (sh[d].ngptot % o.nproma ? 1 : 0);
    const double c = (double)sh[d].ngptot * o.reps;
    printf(" %10d%10d%10d%10d%10d %4d : %10d%10d%10d @ core#\n", o.numomp, o.ngptot, sh[d].ngptot, nbd, o.nproma,
           d, (int)(tl * 1000.), tl > 0 ? (int)(1.0e-06 * ZHPM * (c / 100.) / tl) : 0,
           tl > 0 ? (int)(c / tl) : 0);
  }
  printf(" %10d%10d%10d%10d%10d %4d : %10d%10d%10d TOTAL\n", o.numomp, o.ngptot, o.ngptot, nblocks, o.nproma, -1,
         (int)(tdiff * 1000.), tdiff > 0 ? (int)(1.0e-06 * ZHPM * (cols_done / 100.) / tdiff) : 0,
         tdiff > 0 ? (int)(cols_done / tdiff) : 0);
  /* precise figures for scripts (the table above keeps the reference's integer format) */
  double kmax = 0.0;
  for (int d = 0; d < nused; d++) {
    double k = 0.0;
    for (int r = 0; r < o.reps; r++) k += sh[d].kernel_ms[r];
    k /= o.reps;
    if (k > kmax) kmax = k;
  }
  printf(" TIMING: steps=%d wall_ms_per_step=%.4f kernel_ms_per_step=%.4f columns_per_s=%.1f devices=%d\n", o.reps,
         1e3 * tdiff / o.reps, kmax, cols_done / tdiff, nused);
  /* the placement search of each shard's state (cloudsc_state_placement_report) */
  for (int d = 0; d < nused; d++) {
    const cloudsc_placement_t *pl = &sh[d].place;
    if (pl->method == CLOUDSC_PLACE_METHOD_NONE) {
      printf(" PLACEMENT: shard=%d search=off\n", d);
      continue;
    }
    printf(" PLACEMENT: shard=%d search=%s first_ms=%.4f kept_ms=%.4f tries=%d moves=%d launches=%d "
           "search_ms=%.1f peak_transient_MB=%.1f\n", d,
           pl->method == CLOUDSC_PLACE_METHOD_KERNEL ? "kernel" : "rw-probe", pl->probe_first_ms, pl->probe_final_ms, pl->tries,
           pl->moves, pl->launches, pl->search_ms, pl->peak_transient_bytes / 1048576.0);
  }
  /* board power over the energy window (--energy): uJ per column = W x ms per launch / columns */
  if (o.energy_s > 0.0 && o.fields_caller) printf(" ENERGY: n/a (--fields caller has no energy window)\n");
  for (int d = 0; d < nused && o.energy_s > 0.0 && !o.fields_caller; d++) {
    if (!sh[d].power_path[0] || !sh[d].power_samples) {
      printf(" ENERGY: shard=%d device=%d n/a (no hwmon power file for this device)\n", d, sh[d].device);
      continue;
    }
    /* shards sharing a device (--gpus above the device count) read the same
     * board over overlapping windows: the board's power is not theirs alone
     * (ADVICE r05), so no per-column figure is claimed */
    int sharing = 0;
    for (int e = 0; e < nused; e++) sharing += sh[e].device == sh[d].device;
    if (sharing > 1) {
      printf(" ENERGY: shard=%d device=%d board_w=%.1f samples=%d uj_per_column=n/a (the device runs %d shards "
             "at once; its board power is theirs together)\n", d, sh[d].device, sh[d].board_w,
             sh[d].power_samples, sharing);
      continue;
    }
    printf(" ENERGY: shard=%d device=%d board_w=%.1f samples=%d steps=%d ms_per_step=%.4f uj_per_column=%.3f "
           "source=%s\n", d, sh[d].device, sh[d].board_w, sh[d].power_samples, sh[d].energy_steps,
           sh[d].energy_ms_per_step, sh[d].board_w * sh[d].energy_ms_per_step * 1e3 / sh[d].ngptot,
           sh[d].power_path);
  }

  /* ---- validation (cloudsc_validate.c:193-216, combined over devices) ---- */
  int bad = 0;
  if (ds.has_reference) {
    printf(" %20s %s %20s %20s %20s %20s %20s\n", "Variable", "Dim", "MinValue", "MaxValue", "AbsMaxErr",
           "AvgAbsErr/GP", "MaxRelErr-%");
    const int gate = o.precision == CLOUDSC_FP64 || o.tol_given;
    double worst = 0.0;
    for (int f = 0; f < CLOUDSC_NVALID; f++) {
      if (sh[0].skipped[f]) continue;   /* --outputs prognostic: not allocated, not computed: no row */
      cloudsc_stats_t s = sh[0].stats[f];
      for (int d = 1; d < nused; d++) cloudsc_stats_combine(&s, &sh[d].stats[f]);   /* double-double sums */
      int kind = cloudsc_io_ref_kind[f];
      /* --outputs surface: the four rows are the surface row's statistics */
      if (o.outputs == CLOUDSC_OUTPUTS_SURFACE && f >= CLOUDSC_F_PFPLSL && f <= CLOUDSC_F_PFHPSN) kind = CLOUDSC_FK_SURFACE;
      const double rel = print_error(cloudsc_io_print_names[f], kind == 3 ? 1 : kind == 2 ? 3 : 2, &s, o.ngptot);
      if (rel > worst) worst = rel;
      if (gate && !(rel <= o.tol)) bad++;
    }
    if (gate)
      printf(" VALIDATION: %s (worst relative L1 error %.3e, gate %.1e, %d field(s) over)\n",
             bad ? "FAILED" : "PASSED", worst, o.tol, bad);
    else
      printf(" VALIDATION: reported only (%s vs the fp64 reference; worst relative L1 error %.3e)\n",
             precision_name(o.precision), worst);
  } else {
    printf(" VALIDATION: skipped (no reference outputs loaded)\n");
  }
  if (o.batch)
    printf(" BATCH: sets=%d columns_per_set=%d ms_per_launch=%.4f (one cloudsc_gpu_run_batch per step)\n", o.batch,
           set_cols, kmax);
  if (o.advance)
    printf(" ADVANCE: steps=%d ms_per_step=%.4f in place (cloudsc_gpu_run_advance: pt, pq, pa, pclv rewritten)%s\n",
           o.advance, kmax, o.advance > 1 ? "; nothing validated after more than one step" : "");
  for (int d = 0; d < nused; d++) free(sh[d].kernel_ms);
  free(sh);
  free(th);
  cloudsc_io_free(&ds);
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
