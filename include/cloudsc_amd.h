/*
 * cloudsc_amd.h -- C ABI of the MI355X-native CLOUDSC dwarf (libcloudsc_amd.so).
 *
 * Plain C: no C++ or torch types, plain pointers and sizes.  Every entry point
 * returns 0 on success or a negative CLOUDSC_E* code; the library never calls
 * exit().  Parameters live in per-parameter-set device blocks: each device has
 * a default set (cloudsc_gpu_init, used by cloudsc_gpu_run), and every state
 * and host pipeline owns a private copy, so states with different parameters
 * can be interleaved on one device.  One host thread per device -- or one
 * thread driving N devices -- is safe.  cloudsc_gpu_init rewrites the device's
 * default set in place: it must not race with cloudsc_gpu_run or
 * cloudsc_host_pipeline_create on the same device from another thread (states
 * and pipelines already created are unaffected).
 *
 * Which reference interface each declaration replaces (paths relative to the
 * lukasm91/dwarf-p-cloudsc checkout):
 *
 *   cloudsc_params_t   <- struct TECLDP (src/cloudsc_c/cloudsc/yoecldp_c.h:21-141)
 *                         + YOMCST globals (yomcst_c.h:14-72) + YOETHF globals
 *                         (yoethf_c.h:14-36) + PTSPHY, filled by load_state()
 *                         (src/cloudsc_c/cloudsc/load_state.c:538-690)
 *   cloudsc_fields_t   <- the 56 array arguments of cloudsc_c()
 *                         (src/cloudsc_c/cloudsc/cloudsc_c.h:18-29) and of the
 *                         CUDA kernel (src/cloudsc_cuda/cloudsc/cloudsc_c_k_caching.cu:13-40)
 *   cloudsc_gpu_init   <- cudaMemcpy of the TECLDP struct + the 28 by-value
 *                         constants (src/cloudsc_cuda/cloudsc/cloudsc_driver.cu:312,383,412-416)
 *   cloudsc_gpu_check  <- the cudaPeekAtLastError/cudaDeviceSynchronize check
 *                         after the launch (cloudsc_driver.cu:419-420)
 *   cloudsc_cpu_run    <- the CPU dwarf's OpenMP block loop calling cloudsc_c()
 *                         (src/cloudsc_c/cloudsc/cloudsc_driver.c:183-217, kernel
 *                         cloudsc_c.c:19-2587, declared cloudsc_c.h:18-29)
 *   cloudsc_gpu_run    <- cloudsc_c<<<grid,nproma>>>(...) (cloudsc_driver.cu:391-416)
 *   cloudsc_state_*    <- the driver plumbing around the kernel: load+expand
 *                         (load_state.c:69-184,279), timing (cloudsc_driver.c:181-262),
 *                         validation (src/common/module/validate_mod.F90:118-296)
 *
 * Field layout (identical to the reference C/CUDA drivers, cloudsc_driver.c:114-171):
 * NPROMA-blocked, nblocks = ceil(ngptot/nproma), column jl of block b is global
 * column b*nproma+jl.
 *   full-level field     [nblocks][klev][nproma]
 *   half-level field     [nblocks][klev+1][nproma]      (paph, the 14 flux fields)
 *   species field        [nblocks][NCLV][klev][nproma]  (pclv, tendency_*_cld)
 *   surface field        [nblocks][nproma]              (plsm, ktype, prainfrac_toprfz)
 * Element type is double for CLOUDSC_FP64 and float for CLOUDSC_FP32 and
 * CLOUDSC_MIXED (ktype is always int32).  Lanes jl >= bsize of the last block are never read or written.
 *
 * Output contract (stronger than the reference C kernel, matches the CUDA one):
 * the callee writes EVERY output element of every active column -- including
 * tendency_loc_cld[vapour] (zero) and pcovptot at levels < NCLDTOP (zero) --
 * so the caller need not pre-zero (cf. cloudsc_driver.c:199-200).  plude is
 * read-modify-write exactly as in the reference (cloudsc_c.c:970,980).
 */
#ifndef CLOUDSC_AMD_H
#define CLOUDSC_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define CLOUDSC_NCLV 5          /* ql, qi, qr, qs, qv (yoecldp_c.h:13-18)            */

/* precision selector */
#define CLOUDSC_FP64 8
#define CLOUDSC_FP32 4
/* Mixed precision: every real field is float in memory (ktype int32, as
 * always), the arithmetic is double with the fp64 kernels' own exp/pow and
 * IEEE divisions.  A load widens (exact); a store narrows with one conversion,
 * round to nearest even with gradual underflow (no flush to zero).  The kernels
 * never read back an output they stored, and the state carried between levels
 * and KSEG segments stays double, so the contract is an identity, bit for bit
 * over every output field and plude:
 *
 *   out = (float) fp64_kernel( (double) in )
 *
 * with `in` the float fields as stored (a caller holding doubles rounds them
 * to float first: cloudsc_fields_convert does it on the device, with this same
 * conversion) and fp64_kernel the CLOUDSC_FP64 computation -- the
 * reference kernel's.  Half the bytes of fp64 per column and per resident
 * state, the accuracy of fp64 arithmetic on float-rounded data (DESIGN.md
 * §3.17).  Parameters, the KSEG workspace and cloudsc_gpu_scratch_bytes are
 * fp64's; CLOUDSC_FP32_EXACT_LIBM is ignored, as for fp64.
 * Where it runs: cloudsc_gpu_run / cloudsc_gpu_check with KCACHE and KSEG,
 * cloudsc_fields_alloc, the state API, cloudsc_cpu_run_precision and the
 * memory probes.  Where it does not (CLOUDSC_EINVAL): CLOUDSC_VARIANT_SCC and
 * CLOUDSC_VARIANT_SCC_PRIVATE, cloudsc_host_pipeline_create and
 * cloudsc_host_run; the drop-in cloudsc_c() is double by its signature. */
#define CLOUDSC_MIXED 12

/* kernel variant selector */
#define CLOUDSC_VARIANT_SCC    1   /* SCC baseline: level phases as separate sweeps, temporaries in HBM scratch */
#define CLOUDSC_VARIANT_KCACHE 2   /* SCC-k-caching: one fused level loop, carried state in registers       */
#define CLOUDSC_VARIANT_KSEG   3   /* SCC-k-caching, persistent work queue over (level segment, block)      */
                                   /* items; carried state handed between segments through HBM scratch   */
#define CLOUDSC_VARIANT_SCC_PRIVATE 4  /* SCC with per-thread private-array temporaries (scratch memory):   */
                                   /* the reference CUDA SCC form, cloudsc_c.cu:60-317; klev <= 137 as    */
                                   /* there (:53); no caller workspace                                     */

/* Option bit, OR-ed into a `variant` argument (cloudsc_gpu_run, cloudsc_state_run,
 * cloudsc_host_pipeline_run).  fp32 evaluates exp/pow in single precision with
 * the device's float forms by default (hardware exp2/log2 with an exact
 * argument reduction: <= 2 ulp, every operation float) and divides with the
 * hardware reciprocal and one residual correction (within 1 ulp); with this
 * bit it uses the reference CPU build's glibc expf/powf algorithms (computed in
 * double) and correctly rounded divisions instead: bit-identical to the
 * single-precision restatement, slower.  fp64 always uses the reference CPU
 * build's exp/pow and IEEE divisions and ignores the bit. */
#define CLOUDSC_FP32_EXACT_LIBM 0x100

/* error codes */
#define CLOUDSC_OK            0
#define CLOUDSC_EINVAL      (-1)   /* bad argument (sizes, NULL pointer, precision, variant) */
#define CLOUDSC_ENODEV      (-2)   /* no such HIP device                                      */
#define CLOUDSC_EHIP        (-3)   /* a HIP runtime call failed (see cloudsc_last_hip_error) */
#define CLOUDSC_ENOINIT     (-4)   /* cloudsc_gpu_init not called for this device           */
#define CLOUDSC_ENOMEM      (-5)   /* device or host allocation failed                        */
#define CLOUDSC_EIO         (-6)   /* file could not be read / wrong format                   */
#define CLOUDSC_EHANDOFF    (-7)   /* a KSEG segment hand-off timed out: outputs invalid      */

/* ------------------------------------------------------------------------ */
/* Parameters: YOMCST + YOETHF + TECLDP (without rbeta/rbetap1) + PTSPHY     */
/* ------------------------------------------------------------------------ */
typedef struct cloudsc_params {
  double ptsphy;
  /* YOMCST (the 9 the kernel reads) */
  double rg, rd, rcpd, retv, rlvtt, rlstt, rlmlt, rtt, rv;
  /* YOETHF */
  double r2es, r3les, r3ies, r4les, r4ies, r5les, r5ies, r5alvcp, r5alscp;
  double ralvdcp, ralsdcp, ralfdcp, rtwat, rtice, rticecu, rtwat_rtice_r, rtwat_rticecu_r;
  double rkoop1, rkoop2;
  /* TECLDP doubles, in yoecldp_c.h order */
  double ramid, rcldiff, rcldiff_convi, rclcrit, rclcrit_sea, rclcrit_land, rkconv, rprc1, rprc2;
  double rcldmax, rpecons, rvrfactor, rprecrhmax, rtaumel, ramin, rlmin, rkooptau, rcldtopp;
  double rlcritsnow, rsnowlin1, rsnowlin2, ricehi1, ricehi2, riceinit, rvice, rvrain, rvsnow;
  double rthomo, rcovpmin, rccn, rnice, rccnom, rccnss, rccnsu, rcldtopcf, rdepliqrefrate;
  double rdepliqrefdepth, rcl_kkaac, rcl_kkbac, rcl_kkaau, rcl_kkbauq, rcl_kkbaun;
  double rcl_kk_cloud_num_sea, rcl_kk_cloud_num_land, rcl_ai, rcl_bi, rcl_ci, rcl_di;
  double rcl_x1i, rcl_x2i, rcl_x3i, rcl_x4i, rcl_const1i, rcl_const2i, rcl_const3i, rcl_const4i;
  double rcl_const5i, rcl_const6i, rcl_apb1, rcl_apb2, rcl_apb3, rcl_as, rcl_bs, rcl_cs, rcl_ds;
  double rcl_x1s, rcl_x2s, rcl_x3s, rcl_x4s, rcl_const1s, rcl_const2s, rcl_const3s, rcl_const4s;
  double rcl_const5s, rcl_const6s, rcl_const7s, rcl_const8s, rdenswat, rdensref, rcl_ar, rcl_br;
  double rcl_cr, rcl_dr, rcl_x1r, rcl_x2r, rcl_x4r, rcl_ka273, rcl_cdenom1, rcl_cdenom2, rcl_cdenom3;
  double rcl_schmidt, rcl_dynvisc, rcl_const1r, rcl_const2r, rcl_const3r, rcl_const4r, rcl_fac1;
  double rcl_fac2, rcl_const5r, rcl_const6r, rcl_fzrab, rcl_fzrbb, nshapep, nshapeq;
  /* TECLDP integers / logicals (logical: 0 = .FALSE., nonzero = .TRUE.) */
  int lcldextra, lcldbudget, nssopt, ncldtop;
  int naeclbc, naecldu, naeclom, naeclss, naeclsu, nclddiag, naercld;
  int laerliqautolsp, laerliqautocp, laerliqautocpb, laerliqcoll, laericesed, laericeauto;
  int nbeta;
} cloudsc_params_t;

/* ------------------------------------------------------------------------ */
/* Field pointers (device pointers for cloudsc_gpu_run)                      */
/* ------------------------------------------------------------------------ */
typedef struct cloudsc_fields {
  /* inputs */
  const void *pt, *pq;
  const void *tendency_tmp_t, *tendency_tmp_q, *tendency_tmp_a, *tendency_tmp_cld;
  const void *pvfl, *pvfi, *phrsw, *phrlw, *pvervel, *pap, *paph, *plsm;
  const int  *ktype;
  const void *plu, *psnde, *pmfu, *pmfd, *pa, *pclv, *psupsat;
  /* aerosol inputs: read only when the matching LAER* flag is set; may be NULL otherwise */
  const void *plcrit_aer, *picrit_aer, *pre_ice, *pccn, *pnice;
  /* in/out */
  void *plude;
  /* outputs */
  void *tendency_loc_t, *tendency_loc_q, *tendency_loc_a, *tendency_loc_cld;
  void *pcovptot, *prainfrac_toprfz;
  void *pfsqlf, *pfsqif, *pfcqnng, *pfcqlng, *pfsqrf, *pfsqsf, *pfcqrng, *pfcqsng;
  void *pfsqltur, *pfsqitur, *pfplsl, *pfplsn, *pfhpsl, *pfhpsn;
} cloudsc_fields_t;

/* ------------------------------------------------------------------------ */
/* Low-level boundary: run the kernel on caller-owned device buffers         */
/* ------------------------------------------------------------------------ */

/* Number of visible HIP devices. */
int cloudsc_gpu_device_count(int *count);

/* Set the device's default parameter set (fp64 and fp32 mirrors, folded on
 * the host) used by cloudsc_gpu_run.  Must be called once per device before
 * cloudsc_gpu_run.  Calling it again replaces the set in place: it first waits
 * for all work on the device (hipDeviceSynchronize), so launches already
 * queued keep the parameters they were launched with.  States and host
 * pipelines are not affected (they hold their own copy).  Not to be called
 * concurrently with launches on the same device (see the top of this file). */
int cloudsc_gpu_init(int device, const cloudsc_params_t *params);

/* Enqueue one CLOUDSC step over ngptot columns on `stream` (a hipStream_t, or
 * NULL for the default stream) of `device`.  Asynchronous; errors in the launch
 * configuration are returned, asynchronous faults surface at the caller's sync.
 * SCC and KSEG need a workspace: pass scratch of cloudsc_gpu_scratch_bytes()
 * (KCACHE and SCC_PRIVATE need none: the latter's temporaries are the
 * kernel's private segment, sized by the HIP runtime at launch)
 * bytes (NULL is fine for KCACHE).  The KSEG workspace holds a dequeue counter
 * and per-block flags that are re-zeroed on `stream` before every launch, so one
 * workspace must not be shared by launches in flight on different streams.
 * nproma: 1..256 for KCACHE and SCC (one workgroup of nproma threads per
 * block), 1..2^24 for KSEG (64-column sub-blocks; all index arithmetic is
 * 64-bit); otherwise CLOUDSC_EINVAL.
 * Narrow blocks: KCACHE and KSEG can run blocks of nproma <= 32 packed,
 * 64 / nproma consecutive blocks per wave, instead of one block per partly
 * idle wave.  The memory layout, the workspace and the output bits are the
 * same either way; cloudsc_gpu_launch_geometry reports what a launch would
 * do, cloudsc_debug_set_narrow_pack overrides the measured default (DESIGN.md
 * §3.18).
 * A caller-owned KSEG workspace carries a sticky error word (below): zero it,
 * or pass it through cloudsc_gpu_check, before reusing the memory for a new
 * series of launches, or a stale count may surface as CLOUDSC_EHANDOFF. */
int cloudsc_gpu_run(int device, void *stream, int precision, int variant,
                    int ngptot, int nproma, int klev,
                    const cloudsc_fields_t *device_fields, void *scratch);

/* ------------------------------------------------------------------------ */
/* Caller-owned device fields, placed (round 5)                              */
/* ------------------------------------------------------------------------ */
/* How fast the kernel writes its 21 output fields depends on where they land
 * in HBM: field sets of one configuration ran the fp64 KSEG kernel at
 * 1.63-1.94 ms, and the slow ones stall on DRAM write credits (DESIGN.md
 * §3.12).  A placement search allocates candidate buffers, times a probe over
 * them and keeps a candidate when the probe is > 1 % faster.  Its cost and
 * result: */
typedef struct cloudsc_placement {
  float probe_first_ms, probe_final_ms;   /* probe time of the first / the kept placement            */
  int tries, moves;                       /* candidate buffers allocated / kept                      */
  int launches;                           /* probe launches run (untimed warm-ups included)          */
  int method;                             /* CLOUDSC_PLACE_METHOD_*                                  */
  double search_ms;                       /* wall time of the search                                 */
  long long peak_transient_bytes;         /* most device bytes held at once beyond the fields' own   */
  long long transient_budget_bytes;       /* the bound the free-memory check was made for (round 6):  */
                                          /* peak_transient_bytes never exceeds it; 0 = no search    */
} cloudsc_placement_t;
#define CLOUDSC_PLACE_METHOD_NONE        0   /* no search                                             */
#define CLOUDSC_PLACE_METHOD_KERNEL      1   /* the KSEG kernel on the state's own inputs (state API)  */
#define CLOUDSC_PLACE_METHOD_WRITE_PROBE 2   /* the kernel's output write pattern, no physics (round 5) */
#define CLOUDSC_PLACE_METHOD_RW_PROBE    3   /* the kernel's read + write pattern, no physics (round 6) */

/* cloudsc_fields_alloc flags */
#define CLOUDSC_PLACE_NONE     1   /* one allocation per field, no search (a caller that runs one step) */
#define CLOUDSC_ALLOC_AEROSOLS 2   /* also allocate the five aerosol inputs (LAERICESED/LAERICEAUTO)     */

/* Allocate the device buffers of every field of an (ngptot, nproma, klev,
 * precision) problem on `device` -- one allocation per field, block layout, as
 * the reference GPU driver's cudaMalloc calls do (cloudsc_driver.cu:276-328) --
 * for the caller to fill and to run with cloudsc_gpu_run.  Unless flags has
 * CLOUDSC_PLACE_NONE, the output buffers (plude included) are then placed by a
 * search timed with the kernel's memory pattern over the set -- every input
 * read and every output written as the KSEG kernel does, no physics, so no
 * field contents are needed: the caller fills the inputs afterwards (round 6:
 * reads and write-through stores, ranking 10 placements at Spearman 0.99
 * against the kernel, profiles/r06/place_corr_sc1_fp64.jsonl) -- 8 whole fresh
 * output sets, then up to two passes of one field at a time
 * (csrc/cloudsc_place.hip).  The search overwrites nothing the caller owns.
 * Input buffers are never moved (their placement does not change the kernel
 * time).  `report` (may be NULL) receives the search's cost and result.  On an
 * error nothing stays allocated. */
int cloudsc_fields_alloc(int device, int precision, int ngptot, int nproma, int klev, int flags,
                         cloudsc_fields_t *fields, cloudsc_placement_t *report);

/* Free the buffers cloudsc_fields_alloc made and set their pointers to NULL.
 * Non-NULL pointers it did not make (on this device) are left alone and make
 * the call return CLOUDSC_EINVAL. */
int cloudsc_fields_free(int device, cloudsc_fields_t *fields);

/* Copy a field set on `device` into another NPROMA blocking and / or storage
 * type, asynchronously on `stream` (a hipStream_t, NULL = the default stream),
 * in one kernel launch.  For every member that is non-NULL in both src and dst,
 * every row of its kind -- klev (full-level), klev + 1 (half-level),
 * CLOUDSC_NCLV * klev (species) or 1 (surface) -- and every global column
 * g < ngptot:
 *
 *   dst[g / dst_nproma][row][g % dst_nproma] = (dst type) src[g / src_nproma][row][g % src_nproma]
 *
 * The element type follows the precision code as everywhere else: double for
 * CLOUDSC_FP64, float for CLOUDSC_FP32 and CLOUDSC_MIXED; ktype is always an
 * int32 copy.  Widening is exact.  Narrowing is one conversion, round to
 * nearest even with gradual underflow, overflow to infinity, NaN stays NaN: the
 * conversion of the mixed kernels' stores and of the state's expansion.  Equal
 * types copy bits.  Lanes jl past the last column of dst's last block are never
 * written.  dst's input members are `const void *` in the struct and ARE
 * written here.  A member that is NULL in both sets is skipped, so any subset
 * converts: the inputs only, the outputs only, one field.
 * CLOUDSC_EINVAL: a member that is NULL in exactly one of the two sets, no
 * member to convert, the same pointer for a member in src and dst, an unknown
 * precision code, ngptot, klev or an NPROMA < 1, an NPROMA > 2^24, a NULL
 * struct.  Every argument is checked before the first HIP call: a bad argument
 * is CLOUDSC_EINVAL on a machine without a GPU too.  The buffers of src and dst
 * must not overlap: only pointer equality is checked.
 * Never synchronises; returns launch-configuration errors only, asynchronous
 * faults surface at the caller's sync.  Needs no cloudsc_gpu_init.  Moves about
 * as many bytes as a physics step (DESIGN.md §3.19 has the measured rates). */
int cloudsc_fields_convert(int device, void *stream, int ngptot, int klev,
                           int src_precision, int src_nproma, const cloudsc_fields_t *src,
                           int dst_precision, int dst_nproma, const cloudsc_fields_t *dst);

/* cloudsc_fields_convert for two sets of one output selection (below, "Output
 * selection").  With CLOUDSC_OUTPUTS_SURFACE the members pfplsl, pfplsn, pfhpsl,
 * pfhpsn of both sets are surface fields ([nblocks][nproma]) and are re-blocked
 * and re-typed as such; every other member as in cloudsc_fields_convert, which
 * this IS for CLOUDSC_OUTPUTS_ALL and CLOUDSC_OUTPUTS_PROGNOSTIC.  CLOUDSC_EINVAL:
 * an unknown `outputs` value and every argument error of cloudsc_fields_convert,
 * before the first HIP call. */
int cloudsc_fields_convert_outputs(int device, void *stream, int ngptot, int klev, int outputs,
                                   int src_precision, int src_nproma, const cloudsc_fields_t *src,
                                   int dst_precision, int dst_nproma, const cloudsc_fields_t *dst);

/* The same on HOST arrays, on `nthreads` host threads (<= 0: all hardware
 * threads) taking destination blocks from a shared counter: the same
 * semantics, conversion and errors.  Needs no GPU. */
int cloudsc_cpu_fields_convert(int nthreads, int ngptot, int klev,
                               int src_precision, int src_nproma, const cloudsc_fields_t *src,
                               int dst_precision, int dst_nproma, const cloudsc_fields_t *dst);

/* Field set layouts.  Every other entry point takes CLOUDSC_LAYOUT_BLOCKED.  In
 * CLOUDSC_LAYOUT_LEVELS the rows of one column are contiguous and there is no
 * padding: a member is [ngptot][rows] with the rows of its kind in the block
 * layout -- klev, klev + 1, CLOUDSC_NCLV * klev (row m * klev + k of species m:
 * [ngptot][CLOUDSC_NCLV][klev]) or 1 (surface members and ktype: [ngptot]).  It
 * is what MPAS (nVertLevels, nCells), (ncol, nlev) views and [sample][level]
 * NumPy arrays look like. */
#define CLOUDSC_LAYOUT_BLOCKED 0   /* [nblocks][rows][nproma], what every other entry point takes */
#define CLOUDSC_LAYOUT_LEVELS  1   /* [ngptot][rows]: the rows of one column contiguous, no padding */

/* cloudsc_fields_convert_outputs between field sets of either layout on
 * `device`, asynchronously on `stream`.  For every member that is non-NULL in
 * both sets, every row r of its kind under `outputs` and every global column
 * g < ngptot, the element [g / nproma][r][g % nproma] of a BLOCKED side and
 * [g][r] of a LEVELS side:  dst = (dst type) src, the conversion of
 * cloudsc_fields_convert (equal types copy bits, ktype is an int32 copy).
 * A LEVELS side has no NPROMA: its *_nproma must be 0.  The padding lanes of a
 * BLOCKED destination's last block are never written; a LEVELS destination is
 * written in exactly ngptot * rows elements.
 * BLOCKED -> BLOCKED is cloudsc_fields_convert_outputs; LEVELS -> LEVELS is that
 * copy over one block of ngptot columns (so ngptot <= 2^24 there).  Between the
 * two layouts the members of one row take the same copy, and the others one
 * transposing kernel through LDS tiles (at most two launches; DESIGN.md §3.27
 * has the access pattern and the rates).
 * CLOUDSC_EINVAL, before the first HIP call and so on a machine without a GPU
 * too: an unknown layout or `outputs`, a non-zero NPROMA on a LEVELS side, and
 * every argument error of cloudsc_fields_convert.  Never synchronises; needs no
 * cloudsc_gpu_init.  The step entry points take BLOCKED sets only: convert the
 * inputs once, and the outputs after a step.  Packed tendency buffers are not a
 * side of this call (unpack with cloudsc_fields_convert_tendbuf first). */
int cloudsc_fields_convert_layout(int device, void *stream, int ngptot, int klev, int outputs,
                                  int src_precision, int src_layout, int src_nproma, const cloudsc_fields_t *src,
                                  int dst_precision, int dst_layout, int dst_nproma, const cloudsc_fields_t *dst);

/* The same on HOST arrays, on `nthreads` host threads (<= 0: all hardware
 * threads) taking destination blocks (BLOCKED) or ranges of 256 columns
 * (LEVELS) from a shared counter.  Needs no GPU. */
int cloudsc_cpu_fields_convert_layout(int nthreads, int ngptot, int klev, int outputs,
                                      int src_precision, int src_layout, int src_nproma, const cloudsc_fields_t *src,
                                      int dst_precision, int dst_layout, int dst_nproma, const cloudsc_fields_t *dst);

/* What the loaded code object says about kernel `which` (0..7: the storage pairs
 * 8->8, 8->4, 4->8, 4->4 towards LEVELS, then the same towards BLOCKED) of the
 * layout conversion on `device`: scratch bytes per lane and LDS bytes per
 * workgroup.  For the tests; asks the runtime, launches nothing.  A library built
 * with -DCLOUDSC_LAYOUT_NAIVE (make variant) has no such kernels and does not
 * export this symbol. */
int cloudsc_debug_layout_kernel_resources(int device, int which, int *scratch_bytes, int *lds_bytes);

/* ------------------------------------------------------------------------ */
/* Packed tendency buffers (the reference's Fortran drivers)                 */
/* ------------------------------------------------------------------------ */
/* The reference's Fortran GPU, Loki and Python-interface drivers keep the
 * tendencies in two packed buffers (cloudsc_driver_gpu_scc_mod.F90:50-52,146-147),
 *
 *   BUFFER_TMP(NPROMA, NLEV, 3+NCLV, NGPBLKS), BUFFER_LOC(NPROMA, NLEV, 3+NCLV, NGPBLKS)
 *
 * whose planes 1..8 are T, A, Q, CLD(1..5): in C order [nblocks][planes][klev]
 * [nproma].  Inside a block a plane is an ordinary [klev][nproma] level field
 * and the five CLD planes an ordinary [5][klev][nproma] species field; only the
 * block stride differs: tend_planes * klev * nproma elements instead of klev *
 * nproma (5 * klev * nproma).  The "tendbuf" entry points take field sets whose
 * eight tendency members -- tendency_tmp_t/q/a/cld, tendency_loc_t/q/a/cld --
 * have that stride: each member points at the start of its plane in block 0, so
 * which plane a member is, and in which buffer, is the caller's choice.  Every
 * other member is a plain array as everywhere else.  tend_planes is the
 * number of planes per block, 8..64 (IFS builds carry more than 3 + NCLV). */
#define CLOUDSC_TENDBUF_PLANES_MIN 8        /* 3 + CLOUDSC_NCLV                */
#define CLOUDSC_TENDBUF_PLANES_MAX 64
#define CLOUDSC_TENDBUF_T 0                 /* reference plane order, 0-based  */
#define CLOUDSC_TENDBUF_A 1
#define CLOUDSC_TENDBUF_Q 2
#define CLOUDSC_TENDBUF_CLD 3

/* Set the eight tendency members of *fields to the plane starts of the two
 * buffers in the reference's plane order (CLOUDSC_TENDBUF_*): tendency_tmp_x =
 * buffer_tmp + plane * klev * nproma elements of the precision's storage type,
 * tendency_loc_x likewise in buffer_loc.  Pointer arithmetic only: host or
 * device buffers, any tend_planes.  The other members are left as they are.
 * CLOUDSC_EINVAL: a NULL argument, an unknown precision, nproma or klev < 1. */
int cloudsc_tendbuf_bind(cloudsc_fields_t *fields, int precision, int nproma, int klev,
                         const void *buffer_tmp, void *buffer_loc);

/* cloudsc_gpu_run on a field set whose eight tendency members have the block
 * stride tend_planes * klev * nproma (above); everything else -- arguments,
 * asynchrony, workspace, narrow-block packing, outputs, cloudsc_gpu_check,
 * cloudsc_gpu_scratch_bytes, cloudsc_gpu_launch_geometry -- is cloudsc_gpu_run's,
 * and the output bits are those of cloudsc_gpu_run on the same values in
 * separate arrays.  Only the elements of the planes the members point at are
 * touched, and of those only the lanes of real columns: other planes of a
 * buffer and padding lanes keep their contents.  A packed launch whose lane
 * offsets in a buffer would not fit 32 bits -- pack * tend_planes * klev *
 * nproma * 8 >= 2^32, i.e. KLEV >= 131072 at 64 planes -- runs unpacked;
 * cloudsc_gpu_launch_geometry does not take tend_planes and reports the
 * packed geometry for such a shape, the one case where it differs.
 * KCACHE and KSEG only: CLOUDSC_VARIANT_SCC and CLOUDSC_VARIANT_SCC_PRIVATE
 * have no tendency buffer form and return CLOUDSC_EINVAL.  So does the option
 * bit CLOUDSC_FP32_EXACT_LIBM: fp32 runs its default exp/pow here.  Also
 * CLOUDSC_EINVAL: tend_planes outside 8..64 and every argument error of
 * cloudsc_gpu_run; all of these are checked before the first HIP call. */
int cloudsc_gpu_run_tendbuf(int device, void *stream, int precision, int variant, int ngptot, int nproma,
                            int klev, int tend_planes, const cloudsc_fields_t *device_fields, void *scratch);

/* cloudsc_cpu_run_precision (below) on such a field set in HOST memory: the
 * same phase functions with the same block stride, the same bits as
 * cloudsc_cpu_run_precision on separate arrays.  Needs no GPU. */
int cloudsc_cpu_run_tendbuf(int nthreads, int precision, int ngptot, int nproma, int klev, int tend_planes,
                            const cloudsc_params_t *params, const cloudsc_fields_t *host_fields);

/* cloudsc_fields_convert with the tendency members of either side in packed
 * buffers: where src_tend_planes (dst_tend_planes) is non-zero, the eight
 * tendency members of src (dst) have the block stride *_tend_planes * klev *
 * *_nproma elements; 0 means separate arrays.  One launch packs (0 -> n),
 * unpacks (n -> 0) or re-packs (n -> m), combined if wanted with re-blocking
 * and re-typing; with 0 and 0 it is cloudsc_fields_convert.  Planes no member
 * points at and padding lanes are never written.  CLOUDSC_EINVAL as
 * cloudsc_fields_convert, and for a non-zero *_tend_planes outside 8..64.
 * (Comparison, validation and expansion read and write the buffers in place:
 * cloudsc_fields_compare_tendbuf, cloudsc_fields_validate_tendbuf and
 * cloudsc_fields_expand_tendbuf, below.) */
int cloudsc_fields_convert_tendbuf(int device, void *stream, int ngptot, int klev,
                                   int src_precision, int src_nproma, int src_tend_planes,
                                   const cloudsc_fields_t *src,
                                   int dst_precision, int dst_nproma, int dst_tend_planes,
                                   const cloudsc_fields_t *dst);

/* The same on HOST arrays, as cloudsc_cpu_fields_convert.  Needs no GPU. */
int cloudsc_cpu_fields_convert_tendbuf(int nthreads, int ngptot, int klev,
                                       int src_precision, int src_nproma, int src_tend_planes,
                                       const cloudsc_fields_t *src,
                                       int dst_precision, int dst_nproma, int dst_tend_planes,
                                       const cloudsc_fields_t *dst);

/* ------------------------------------------------------------------------ */
/* Output selection: a step that writes only the prognostic outputs          */
/* ------------------------------------------------------------------------ */
/* Ten of the 21 outputs are diagnostic fluxes that nothing in the step reads
 * back -- pfsqlf, pfsqif, pfcqnng, pfcqlng, pfsqrf, pfsqsf, pfcqrng, pfcqsng,
 * pfsqltur, pfsqitur: the running sums of section 8, which a host model uses
 * for budget diagnostics only.  They are 10 * (klev + 1) of the 24 * klev + 15
 * values a column writes (42 % of the stores, 19.7 % of a step's bytes,
 * DESIGN.md §3.5).  A caller that only advances its state needs the other
 * eleven: plude, tendency_loc_t/q/a/cld, pcovptot, prainfrac_toprfz, pfplsl,
 * pfplsn, pfhpsl, pfhpsn. */
#define CLOUDSC_OUTPUTS_ALL        0   /* all 21 outputs, as cloudsc_gpu_run                        */
#define CLOUDSC_OUTPUTS_PROGNOSTIC 1   /* the ten diagnostic fluxes neither computed nor written   */
/* A selection is a bit set.  Bit 0 (value 1, CLOUDSC_OUTPUTS_PROGNOSTIC): no
 * diagnostic flux profiles.  Bit 2 (value 4): the four precipitation / enthalpy
 * fluxes pfplsl, pfplsn, pfhpsl, pfhpsn at the surface only; valid only together
 * with bit 0.  The value 4 alone, the value 2 and every other value are unknown
 * (CLOUDSC_EINVAL) everywhere a selection is taken.
 *
 * CLOUDSC_OUTPUTS_SURFACE: what a host model couples to its surface scheme is
 * the surface precipitation and its enthalpy flux -- the last half-level row,
 * row klev (0-based) of the klev + 1 rows of the four profiles; the other rows
 * are budget diagnostics (at KLEV 137 in fp64 4,416 of the 56,036 B a column
 * writes).  With this selection
 *   - everything CLOUDSC_OUTPUTS_PROGNOSTIC says about the ten diagnostic
 *     members holds: not computed, read or written, may be NULL, a non-NULL one
 *     keeps every byte;
 *   - pfplsl, pfplsn, pfhpsl, pfhpsn are SURFACE FIELDS with the layout of
 *     prainfrac_toprfz, [nblocks][nproma] in the storage type; element [b][l]
 *     holds, bit for bit, what the full step stores at [b][klev][l] of the
 *     [nblocks][klev+1][nproma] profile, and nothing else of these profiles is
 *     stored anywhere.  The four members are required (non-NULL); padding lanes
 *     of a partial last block are not written;
 *   - plude, tendency_loc_t/q/a/cld, pcovptot and prainfrac_toprfz have the bits
 *     of the full step.
 * Support: cloudsc_gpu_run_outputs, cloudsc_cpu_run_outputs,
 * cloudsc_gpu_run_tendbuf_outputs, cloudsc_cpu_run_tendbuf_outputs,
 * cloudsc_fields_alloc_outputs, cloudsc_fields_validate_tendbuf,
 * cloudsc_fields_compare_outputs and cloudsc_fields_convert_outputs take it.
 *   GPU: KCACHE and KSEG x fp64, fp32, mixed x aerosols on / off x unpacked /
 *        packed narrow blocks x separate arrays / packed tendency buffers.
 *        SCC, SCC_PRIVATE and CLOUDSC_FP32_EXACT_LIBM: CLOUDSC_EINVAL before any
 *        HIP call.  One KSEG workspace serves ALL, PROGNOSTIC and SURFACE
 *        launches in any order.
 *   CPU: fp64 and mixed.
 * Not covered: the device-resident state (cloudsc_state_*), the host pipelines
 * and the drop-in always run CLOUDSC_OUTPUTS_ALL.  cloudsc_fields_compare,
 * cloudsc_fields_convert, cloudsc_fields_expand and their _tendbuf forms walk
 * members by the inventory's kind and know nothing of selections: a SURFACE set
 * must pass them with these four members NULL (fields_subset in Python), or go
 * through the _outputs forms below. */
#define CLOUDSC_OUTPUTS_SURFACE_BIT 4
#define CLOUDSC_OUTPUTS_SURFACE    5   /* PROGNOSTIC, and pfplsl/pfplsn/pfhpsl/pfhpsn as [nblocks][nproma] */

/* cloudsc_gpu_run with an output selection.  With CLOUDSC_OUTPUTS_ALL it IS
 * cloudsc_gpu_run: the same kernels, the same argument rules.  With
 * CLOUDSC_OUTPUTS_PROGNOSTIC the ten members above are neither read nor
 * written: they may be NULL, and a non-NULL one keeps every byte.  Every other
 * output has the bits cloudsc_gpu_run gives on the same inputs.  Everything
 * else -- asynchrony, the workspace and cloudsc_gpu_scratch_bytes, narrow-block
 * packing and cloudsc_gpu_launch_geometry, cloudsc_gpu_check -- is
 * cloudsc_gpu_run's.  The KSEG workspace keeps its layout: one workspace serves
 * launches of either selection in any order (the prognostic form does not
 * store or reload the six flux planes of the hand-off).
 * PROGNOSTIC exists for KCACHE and KSEG, in every precision, with and without
 * aerosols, packed and unpacked.  CLOUDSC_VARIANT_SCC, CLOUDSC_VARIANT_SCC_PRIVATE
 * and the option bit CLOUDSC_FP32_EXACT_LIBM have no such form: CLOUDSC_EINVAL,
 * like an unknown `outputs` value and every argument error of cloudsc_gpu_run
 * -- with PROGNOSTIC all of these are checked before the first HIP call.
 * The combined form with the tendency buffers is cloudsc_gpu_run_tendbuf_outputs.
 * cloudsc_fields_validate needs all 21 members: a prognostic set is validated
 * with cloudsc_fields_validate_tendbuf (tend_planes 0 for separate arrays), or
 * compared with cloudsc_fields_compare, which skips members that are NULL in
 * both sets. */
int cloudsc_gpu_run_outputs(int device, void *stream, int precision, int variant, int outputs,
                            int ngptot, int nproma, int klev,
                            const cloudsc_fields_t *device_fields, void *scratch);

/* cloudsc_cpu_run_precision (below) with an output selection, on HOST arrays
 * through the same phase functions: the same contract -- with PROGNOSTIC the
 * ten members may be NULL, a non-NULL one keeps every byte, the other outputs
 * have cloudsc_cpu_run_precision's bits.  CLOUDSC_EINVAL: an unknown `outputs`
 * value and every argument error of cloudsc_cpu_run_precision.  Needs no GPU. */
int cloudsc_cpu_run_outputs(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                            const cloudsc_params_t *params, const cloudsc_fields_t *host_fields);

/* cloudsc_gpu_run_tendbuf with an output selection: the prognostic step on the
 * packed tendency buffers, for a host model that only advances its state and
 * keeps its tendencies in BUFFER_TMP / BUFFER_LOC.  With CLOUDSC_OUTPUTS_ALL it
 * IS cloudsc_gpu_run_tendbuf: the same kernels, the same rules.  With
 * CLOUDSC_OUTPUTS_PROGNOSTIC the contract of cloudsc_gpu_run_outputs applies --
 * the ten diagnostic members may be NULL, a non-NULL one keeps every byte, the
 * eleven kept outputs have the bits of cloudsc_gpu_run on the same values in
 * separate arrays -- together with the touch rule of the buffers: only the
 * planes the members point at, only the lanes of real columns.  All eight
 * tendency planes are still read and written: the tendencies are prognostic.
 * KCACHE and KSEG, every precision, with and without aerosols, packed and
 * unpacked; one KSEG workspace serves every form in any order.
 * CLOUDSC_EINVAL: an unknown `outputs` value, tend_planes outside 8..64,
 * CLOUDSC_VARIANT_SCC, CLOUDSC_VARIANT_SCC_PRIVATE, the option bit
 * CLOUDSC_FP32_EXACT_LIBM, a NULL kept member and every argument error of
 * cloudsc_gpu_run; all checked before the first HIP call. */
int cloudsc_gpu_run_tendbuf_outputs(int device, void *stream, int precision, int variant, int outputs,
                                    int ngptot, int nproma, int klev, int tend_planes,
                                    const cloudsc_fields_t *device_fields, void *scratch);

/* The host twin, on HOST memory through the same phase functions: the bits of
 * cloudsc_cpu_run_precision on separate arrays for the eleven kept outputs.
 * CLOUDSC_EINVAL: an unknown `outputs` value, tend_planes outside 8..64 and
 * every argument error of cloudsc_cpu_run_precision.  Needs no GPU. */
int cloudsc_cpu_run_tendbuf_outputs(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                    int tend_planes, const cloudsc_params_t *params,
                                    const cloudsc_fields_t *host_fields);

/* ------------------------------------------------------------------------ */
/* The cumulative tendency buffer (BUFFER_CML)                               */
/* ------------------------------------------------------------------------ */
/* The reference's Fortran GPU, Loki and Python-interface drivers carry a third
 * buffer of the shape of BUFFER_TMP and BUFFER_LOC, BUFFER_CML(NPROMA, NLEV,
 * 3+NCLV, NGPBLKS), the "cumulative tendency used for final output"
 * (cloudsc_driver_gpu_scc_mod.F90:27,50).  The dwarf's kernel never reads it; a
 * host model adds every physics process's local tendency to it.  The entry
 * points below do that for this step: fused into the step
 * (cloudsc_gpu_run_tendbuf_cml: the caller needs no BUFFER_LOC at all, 8 * klev
 * elements per column of device memory less), or as a separate streaming pass
 * over a BUFFER_LOC that a step has filled (cloudsc_fields_accumulate_tendbuf).
 *
 * The four members are plane starts in block 0 of a buffer [nblocks]
 * [tend_planes][klev][nproma] of the precision's storage type -- t, q, a one
 * plane each, cld the first of five consecutive planes (ql, qi, qr, qs, vapour)
 * -- with the block stride tend_planes * klev * nproma elements, tend_planes
 * being the one the call is given.  Which planes they are is the caller's
 * choice; cloudsc_tendbuf_bind_cml sets the reference's order. */
typedef struct cloudsc_tend_cml { void *t, *q, *a, *cld; } cloudsc_tend_cml_t;

/* Set the four members of *cml to the plane starts of buffer_cml in the
 * reference's plane order (CLOUDSC_TENDBUF_T/A/Q/CLD), as cloudsc_tendbuf_bind
 * does for the other two buffers.  Pointer arithmetic only: a host or a device
 * buffer, any tend_planes.  CLOUDSC_EINVAL: a NULL argument, an unknown
 * precision, nproma or klev < 1. */
int cloudsc_tendbuf_bind_cml(cloudsc_tend_cml_t *cml, int precision, int nproma, int klev, void *buffer_cml);

/* cloudsc_gpu_run_tendbuf_outputs with the step's local tendencies ADDED to the
 * cumulative planes instead of stored to tendency_loc_*: one launch, the same
 * kernels' physics, 7 * klev more element loads per column and seven planes
 * stored instead of eight.
 *
 * What is accumulated.  For each of the seven planes T, Q, A, CLD(ql, qi, qr,
 * qs), every level and every real column, with `loc` what the step holds for
 * tendency_loc_* at that element:
 *   CLOUDSC_FP64   cml = cml + loc, one IEEE double add; loc is, bit for bit,
 *                  what cloudsc_gpu_run stores to tendency_loc_*;
 *   CLOUDSC_FP32   the same with one float add on the fp32 step's float;
 *   CLOUDSC_MIXED  cml = (float)((double)cml + loc64), loc64 the double the
 *                  kernel holds BEFORE its narrowing store: the mixed identity
 *                  out = (float) fp64_form((double) in) extends to CML, bit for
 *                  bit.  (cloudsc_fields_accumulate_tendbuf, below, adds the
 *                  already narrowed float in float arithmetic: in mixed the
 *                  fused form and step + pass differ in the last bit of some
 *                  elements; in fp64 and fp32 they are equal bit for bit.)
 * The add is its own rounding: it never merges into the multiply that produces
 * the tendency (-ffp-contract=off).
 * A launch adds once; repeated launches accumulate repeatedly (the caller
 * zeroes or carries BUFFER_CML as its time step requires).
 *
 * What is left alone.  The vapour plane (the fifth behind cml->cld) is neither
 * read nor written: the step's local vapour tendency is identically zero.
 * tendency_loc_t/q/a/cld of device_fields are neither read nor written: they
 * may be NULL, and a non-NULL one keeps every byte.  In BUFFER_CML only the
 * seven planes' elements in lanes of real columns are touched: other planes,
 * the vapour plane and the padding lanes of a partial last block keep every
 * byte.  Every other kept output (plude, pcovptot, prainfrac_toprfz, the four
 * precipitation fluxes as profiles or surface fields) has the full step's bits.
 *
 * `outputs` is CLOUDSC_OUTPUTS_PROGNOSTIC or CLOUDSC_OUTPUTS_SURFACE.
 * CLOUDSC_OUTPUTS_ALL is refused (CLOUDSC_EINVAL): a caller that wants the
 * flux diagnostics runs its step and then cloudsc_fields_accumulate_tendbuf.
 * KCACHE and KSEG, every precision, with and without aerosols, packed and
 * unpacked narrow blocks; one KSEG workspace serves this form and all others in
 * any order.  The device-resident state, the host pipelines and the drop-in do
 * not have the form.
 * CLOUDSC_EINVAL, all checked before the first HIP call: CLOUDSC_VARIANT_SCC,
 * CLOUDSC_VARIANT_SCC_PRIVATE, the option bit CLOUDSC_FP32_EXACT_LIBM, an
 * unknown option bit, tend_planes outside 8..64, a NULL cml or a NULL member of
 * it, a cml member equal to a tendency_tmp_* or tendency_loc_* member (pointer
 * equality only: overlapping planes are the caller's to avoid), and every
 * argument error of cloudsc_gpu_run_tendbuf_outputs (tendency_loc_* excepted).
 *
 * Rate (one MI355X, 163,840 columns, KSEG, four alternated runs of 3 x 20
 * steps each per precision, profiles/tendbuf_cml/rate.jsonl):
 * against the parent commit's cloudsc_gpu_run_tendbuf_outputs(PROGNOSTIC) the
 * fused step takes 1.081 (fp64), 1.017 (mixed), 1.072 (fp32) of the time; against
 * the same step followed by cloudsc_fields_accumulate_tendbuf 0.723, 0.788,
 * 0.733: fused is below step + pass in every precision. */
int cloudsc_gpu_run_tendbuf_cml(int device, void *stream, int precision, int variant, int outputs,
                                int ngptot, int nproma, int klev, int tend_planes,
                                const cloudsc_fields_t *device_fields, const cloudsc_tend_cml_t *cml,
                                void *scratch);

/* The host twin, on HOST memory through the same phase functions, fp64 and
 * mixed as the other host forms (CLOUDSC_FP32: CLOUDSC_EINVAL): the same
 * contract, the mixed rule included.  CLOUDSC_EINVAL: CLOUDSC_OUTPUTS_ALL or an
 * unknown `outputs` value, tend_planes outside 8..64, the cml rules above and
 * every argument error of cloudsc_cpu_run_tendbuf_outputs (tendency_loc_*
 * excepted).  Needs no GPU. */
int cloudsc_cpu_run_tendbuf_cml(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                int tend_planes, const cloudsc_params_t *params,
                                const cloudsc_fields_t *host_fields, const cloudsc_tend_cml_t *cml);

/* The separate pass: cml += tendency_loc_* over the same seven planes, for
 * callers outside the fused form (the SCC variants, CLOUDSC_OUTPUTS_ALL,
 * separate tendency arrays).  For every level and every real column
 *   cml = cml + loc   in the storage type's arithmetic: double for
 *                     CLOUDSC_FP64, float for CLOUDSC_FP32 AND CLOUDSC_MIXED
 *                     (the stored, already narrowed float is added: not the
 *                     fused form's mixed contract, above).
 * loc_tend_planes (cml_tend_planes) is 0 where tendency_loc_* of loc_fields
 * (the members of cml) are separate arrays -- [nblocks][klev][nproma] and
 * [nblocks][5][klev][nproma] -- or 8..64 where they are planes of a packed
 * buffer, independently on each side.  Only tendency_loc_t/q/a/cld of
 * loc_fields are looked at.  The vapour planes of both sides, other planes and
 * padding lanes are neither read nor written.  One streaming launch through
 * the field set item walker, like convert, compare and expand: asynchronous in
 * `stream`, no cloudsc_gpu_init needed, no workspace.  A launch adds once.
 * CLOUDSC_EINVAL (before the first HIP call): an unknown precision, ngptot,
 * nproma or klev < 1, nproma > 2^24, a *_tend_planes that is neither 0 nor
 * 8..64, a NULL argument, a NULL tendency_loc_* or cml member, a cml member
 * equal to a tendency_loc_* member.  CLOUDSC_ENODEV: no such device. */
int cloudsc_fields_accumulate_tendbuf(int device, void *stream, int precision, int ngptot, int nproma, int klev,
                                      int loc_tend_planes, const cloudsc_fields_t *loc_fields,
                                      int cml_tend_planes, const cloudsc_tend_cml_t *cml);

/* The same on HOST arrays, bit for bit.  Needs no GPU. */
int cloudsc_cpu_fields_accumulate_tendbuf(int nthreads, int precision, int ngptot, int nproma, int klev,
                                          int loc_tend_planes, const cloudsc_fields_t *loc_fields,
                                          int cml_tend_planes, const cloudsc_tend_cml_t *cml);

/* ------------------------------------------------------------------------ */
/* Per-column perturbed parameters (SPP)                                     */
/* ------------------------------------------------------------------------ */
/* An ensemble member under the IFS's stochastically perturbed parametrisations
 * multiplies a handful of cloud-scheme parameters by a random pattern that
 * differs from column to column (the PGP2DSPP(KLON, ...) arrays of the later
 * cloudsc.F90 cycles).  The entry points below take such multipliers as five
 * surface fields beside the launch's (device-wide) parameter set.
 *
 * Each member is a field [nblocks][nproma] in the precision's storage type,
 * with the layout of plsm: element [b][l] is the multiplier of column
 * b * nproma + l.  A NULL member means that parameter is not perturbed.  Padding
 * lanes of a partial last block are never read.  The fields are only read. */
typedef struct cloudsc_spp {
  const void *ramid;        /* RAMID: the critical relative humidity of new clouds (zrhc, both places)  */
  const void *rcldiff;      /* RCLDIFF: erosion of clouds by turbulent mixing (zldifdt)                  */
  const void *rclcrit;      /* RCLCRIT_SEA and RCLCRIT_LAND, whichever the column's PLSM selects          */
  const void *rlcritsnow;   /* RLCRITSNOW: snow autoconversion (zlcrit; not read under LAERICEAUTO)      */
  const void *rpecons;      /* RPECONS: evaporation of snow (zbeta)                                      */
} cloudsc_spp_t;

/* cloudsc_gpu_run_outputs with per-column multipliers.  The arithmetic is part
 * of the contract, so that a host can reproduce it with one multiply: with x
 * the column's multiplier as stored, `real` the compute type and p the
 * parameter of the launch's set converted to `real` as the ordinary step does,
 *   ramid'        = p.ramid * x                       (used at both places of zrhc)
 *   r             = p.rcldiff * x
 *   zldifdt0'     = r * ptsphy
 *   zldifdt_conv' = p.rcldiff_convi * zldifdt0'
 *   kk_lcrit'     = (land ? p.rclcrit_land : p.rclcrit_sea) * x
 *   rlcritsnow'   = p.rlcritsnow * x     (under LAERICEAUTO the aerosol value replaces it as in
 *                                         the ordinary step, and the member is not read)
 *   rg_rpecons'   = p.rg * (p.rpecons * x)
 * each a single IEEE operation of its own (no multiply-add is formed across
 * these products and their consumers).  CLOUDSC_FP64: x is a double, every
 * operation a double.  CLOUDSC_FP32: x is a float, every operation a float.
 * CLOUDSC_MIXED: x is stored as float and widened exactly, every operation a
 * double; the mixed identity extends to out = (float) fp64_spp_step((double)
 * in, (double) x).  A NULL member takes x = 1 for every column.
 * Hence, bit for bit on every output: with every multiplier exactly 1.0 the
 * step is cloudsc_gpu_run_outputs on the same inputs; with one tuple for all
 * columns it is the ordinary step under the cloudsc_params_t scaled on the host
 * (p.n * x in double for fp64; (double)((float)p.n * (float)x) for fp32); with
 * tuples that vary by column, each column is the ordinary step's under its own.
 * There is no clamping and no range check of x: a non-finite or non-positive
 * product is the caller's error, as a bad cloudsc_params_t value is.
 *
 * `outputs` is CLOUDSC_OUTPUTS_ALL or CLOUDSC_OUTPUTS_PROGNOSTIC.  KCACHE and
 * KSEG, fp64, fp32 (default exp/pow) and mixed, with and without aerosols,
 * packed and unpacked narrow blocks; everything else -- asynchrony, the
 * workspace, cloudsc_gpu_check -- is cloudsc_gpu_run_outputs's, and one KSEG
 * workspace serves SPP and other launches in any order (a later segment of a
 * column reads the column's multipliers again; the hand-off record is as it was).
 * CLOUDSC_EINVAL, all checked before the first HIP call: a NULL spp, an spp
 * with no member set (such a caller uses cloudsc_gpu_run_outputs), a member
 * equal to a member of device_fields (pointer equality only),
 * CLOUDSC_OUTPUTS_SURFACE, CLOUDSC_VARIANT_SCC, CLOUDSC_VARIANT_SCC_PRIVATE,
 * the option bit CLOUDSC_FP32_EXACT_LIBM and every argument error of
 * cloudsc_gpu_run_outputs.
 * The tendency-buffer and cumulative-tendency forms have no SPP twin (each
 * further form bit doubles the kernel instantiations); the device-resident
 * state (cloudsc_state_*), the host pipelines and the drop-in do not have the
 * form either. */
int cloudsc_gpu_run_spp(int device, void *stream, int precision, int variant, int outputs,
                        int ngptot, int nproma, int klev,
                        const cloudsc_fields_t *device_fields, const cloudsc_spp_t *spp, void *scratch);

/* The host twin, on HOST memory through the same phase functions, fp64 and
 * mixed as the other host forms (CLOUDSC_FP32: CLOUDSC_EINVAL): the same
 * contract.  CLOUDSC_EINVAL: the spp rules above, CLOUDSC_OUTPUTS_SURFACE or an
 * unknown `outputs` value and every argument error of cloudsc_cpu_run_outputs.
 * Needs no GPU. */
int cloudsc_cpu_run_spp(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                        const cloudsc_params_t *params, const cloudsc_fields_t *host_fields,
                        const cloudsc_spp_t *spp);

/* ------------------------------------------------------------------------ */
/* The advancing step: state in, state out                                   */
/* ------------------------------------------------------------------------ */
/* Hosts whose microphysics interface is "state in, state out, plus surface
 * precipitation" (level-contiguous (ncol, nlev) drivers that come in through
 * cloudsc_fields_convert_layout) have no use for the seven local tendencies:
 * they want the updated prognostics.  The entry points below store those
 * instead -- fused into the step (cloudsc_gpu_run_advance: seven state stores
 * per level replace the eight tendency stores, the vapour tendency's zeros
 * among them; no input is read twice), or as a streaming
 * pass over a set whose tendency_loc_* a step has filled
 * (cloudsc_fields_advance).  An advancing step can be called on its own output:
 * N calls integrate N time steps, with nothing in between but whatever the host
 * does to tendency_tmp_*.
 *
 * The definition.  For the seven advanced quantities X in {t, q, a, cld[0..3]},
 * with X the state member (pt, pq, pa, pclv[m]), tmp the incoming tendency
 * (tendency_tmp_*) and loc what the ordinary step of the same precision stores
 * in tendency_loc_* at that element:
 *   X0    = fl( X  + fl(ptsphy * tmp) )     the step's own starting value
 *   X_new = fl( X0 + fl(ptsphy * loc) )     one multiply, one add, each rounded
 *                                           on its own (no multiply-add)
 * in the working type: double for CLOUDSC_FP64 and CLOUDSC_MIXED, float for
 * CLOUDSC_FP32.  In CLOUDSC_MIXED the fused form takes loc as the double the
 * kernel holds BEFORE its narrowing store, so that the mixed identity out =
 * (float) fp64_form((double) in) extends to the new state bit for bit; the
 * separate pass can only take the stored, narrowed float (widened exactly), so
 * in mixed the two differ in the last bit of some elements.  In fp64 and fp32
 * they are equal bit for bit.
 * Every level is advanced, the levels above NCLDTOP included (there loc is what
 * the step stores there, X + ptsphy * tmp is still applied, and a -0 state
 * becomes +0).  Nothing is clipped and no conservation fix-up is made: a
 * slightly negative q is the caller's concern, as it is with the tendencies.
 * The fifth (vapour) plane behind adv->clv is never written (its tendency is
 * identically zero and the step never reads pclv's), nor are the padding lanes
 * of a partial last block.
 *
 * The four members are arrays in block layout and the set's storage type: t, q
 * and a [nblocks][klev][nproma], clv [nblocks][5][klev][nproma].  Each may be
 * the set's own pt / pq / pa / pclv (in place) or another array, independently
 * of the other three.  It may be no other member of the set and none of the
 * other three (pointer equality only: overlapping arrays are the caller's to
 * avoid). */
typedef struct cloudsc_advance { void *t, *q, *a, *clv; } cloudsc_advance_t;   /* block layout, storage type of the set */

/* cloudsc_gpu_run_outputs with the updated prognostics stored in place of the
 * local tendencies.  tendency_loc_t/q/a/cld of device_fields are neither read
 * nor written: they may be NULL, and a non-NULL one keeps every byte.  Every
 * other selected output (plude, pcovptot, prainfrac_toprfz, the fluxes of the
 * selection) has the ordinary step's bits.
 * In place is safe because every state element is loaded by the one lane that
 * later stores it, at its own level, before that store: pt, pq, pa and pclv are
 * read at row k only, and what level k needs of its neighbours travels in the
 * carried state (store_level_adv, cloudsc_kcache.h, has the argument for the
 * prefetch schedules, the KSEG hand-off and the packed form).
 * `outputs` is CLOUDSC_OUTPUTS_ALL or CLOUDSC_OUTPUTS_SURFACE (new state plus
 * surface precipitation); CLOUDSC_OUTPUTS_PROGNOSTIC alone is refused.  KCACHE
 * and KSEG, fp64, fp32 (default exp/pow) and mixed, with and without aerosols,
 * packed and unpacked narrow blocks; one KSEG workspace serves this form and
 * all others in any order.  The tendency-buffer, cumulative-tendency and
 * per-column multiplier forms have no advancing twin; the device-resident
 * state, the host pipelines and the drop-in do not have the form.
 * CLOUDSC_EINVAL, all checked before the first HIP call: a NULL adv or a NULL
 * member of it, a member that breaks the aliasing rule above,
 * CLOUDSC_OUTPUTS_PROGNOSTIC or an unknown `outputs` value, CLOUDSC_VARIANT_SCC,
 * CLOUDSC_VARIANT_SCC_PRIVATE, the option bit CLOUDSC_FP32_EXACT_LIBM and every
 * argument error of cloudsc_gpu_run_outputs (tendency_loc_* excepted). */
int cloudsc_gpu_run_advance(int device, void *stream, int precision, int variant, int outputs,
                            int ngptot, int nproma, int klev,
                            const cloudsc_fields_t *device_fields, const cloudsc_advance_t *adv, void *scratch);

/* The host twin, on HOST memory through the same phase functions, fp64 and
 * mixed as the other host forms (CLOUDSC_FP32: CLOUDSC_EINVAL): the same
 * contract.  Needs no GPU. */
int cloudsc_cpu_run_advance(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                            const cloudsc_params_t *params, const cloudsc_fields_t *host_fields,
                            const cloudsc_advance_t *adv);

/* The separate pass, for callers that want tendencies AND state: the two lines
 * of the definition over a set whose tendency_loc_* a step has filled, with loc
 * the stored element.  Arithmetic in double for CLOUDSC_FP64 and CLOUDSC_MIXED
 * (float elements are widened exactly, the result narrowed by one conversion),
 * in float for CLOUDSC_FP32.  ptsphy is the one of the device's parameter set
 * (cloudsc_gpu_init).  Only pt, pq, pa, pclv, tendency_tmp_* and tendency_loc_*
 * of device_fields are looked at; the aliasing rule is the one above; vapour
 * planes and padding lanes are neither read nor written.  One streaming launch
 * through the field set item walker, asynchronous in `stream`, no workspace.
 * CLOUDSC_EINVAL (before the first HIP call): an unknown precision, ngptot,
 * nproma or klev < 1, nproma > 2^24, a NULL argument, one of the twelve members
 * or an adv member NULL, the aliasing rule.  CLOUDSC_ENODEV: no such device.
 * CLOUDSC_ENOINIT: cloudsc_gpu_init not called for the device. */
int cloudsc_fields_advance(int device, void *stream, int precision, int ngptot, int nproma, int klev,
                           const cloudsc_fields_t *device_fields, const cloudsc_advance_t *adv);

/* The same on HOST arrays with ptsphy from `params`, bit for bit, in all three
 * precisions.  Needs no GPU. */
int cloudsc_cpu_fields_advance(int nthreads, int precision, int ngptot, int nproma, int klev,
                               const cloudsc_params_t *params, const cloudsc_fields_t *host_fields,
                               const cloudsc_advance_t *adv);

/* cloudsc_fields_alloc for an output selection.  With CLOUDSC_OUTPUTS_ALL it is
 * cloudsc_fields_alloc.  With CLOUDSC_OUTPUTS_PROGNOSTIC the ten diagnostic
 * members are not allocated and stay NULL (10 * (klev + 1) elements per column
 * of device memory less), and the placement search and its probe run over the
 * eleven allocated outputs only.  cloudsc_fields_free frees such a set.
 * With CLOUDSC_OUTPUTS_SURFACE the ten stay NULL as well, and pfplsl, pfplsn,
 * pfhpsl, pfhpsn are allocated as surface fields, nblocks * nproma elements
 * each (4 * klev elements per column less again); the search and its probe run
 * over the seven full-size outputs and these four small ones, the probe
 * writing the four once per column after the last level, as the kernel does.
 * CLOUDSC_EINVAL: an unknown `outputs` value (before the first HIP call) and
 * every argument error of cloudsc_fields_alloc. */
int cloudsc_fields_alloc_outputs(int device, int precision, int ngptot, int nproma, int klev, int flags,
                                 int outputs, cloudsc_fields_t *fields, cloudsc_placement_t *report);

/* Bytes of device scratch a variant needs for (ngptot, nproma, klev, precision); 0 for KCACHE. */
long long cloudsc_gpu_scratch_bytes(int precision, int variant, int ngptot, int nproma, int klev);

/* Wait for `stream` and report failures the kernels count on the device.
 * For KSEG: a segment whose predecessor did not hand over its carried state
 * within the spin bound gives up and counts itself in the workspace; its
 * columns are then wrong.  The count accumulates over the KSEG launches on
 * `scratch` until this call reads it (and clears it): CLOUDSC_EHANDOFF if it is
 * non-zero.  Callers of cloudsc_gpu_run with KSEG should call it after their
 * launches (the state and pipeline APIs do).  Other variants: only the sync. */
int cloudsc_gpu_check(int device, void *stream, int variant, void *scratch);

/* ---- batched step: many caller-owned field sets in one launch ----
 * An ensemble host has several members of 8-32 k columns each, every member in
 * its own device allocations and usually under its own parameter set.  One
 * KCACHE launch per member leaves most of the card idle (a step fills it at
 * about 131 k columns) and the launches of one stream serialise.  A batch runs
 * `nsets` field sets of one shape in ONE launch, each set under its own
 * parameter set.
 *
 * cloudsc_batch_create builds the kernel arguments of every set exactly as
 * cloudsc_gpu_run_outputs(KCACHE) would and uploads them, once and
 * synchronously, as one device table; the caller may free `sets` and `params`
 * (host arrays of nsets elements) when it returns.  params == NULL: every set
 * runs under the device's set (cloudsc_gpu_init is required, CLOUDSC_ENOINIT)
 * as it is at the time of each run; otherwise set i runs under params[i],
 * converted as cloudsc_gpu_init converts them, and no cloudsc_gpu_init is needed.
 * cloudsc_gpu_run_batch is one launch, asynchronous in `stream`, with no upload
 * and no allocation; cloudsc_gpu_check(device, stream, KCACHE, NULL) waits for it.
 *
 * Contract: every selected output of set i has, bit for bit, what
 * cloudsc_gpu_run_outputs(KCACHE, same precision and outputs) gives for that
 * set alone after cloudsc_gpu_init(device, &params[i]) -- fp64, fp32 (default
 * exp/pow) and mixed; CLOUDSC_OUTPUTS_ALL, PROGNOSTIC and SURFACE; packed and
 * unpacked narrow blocks (cloudsc_debug_set_narrow_pack, read at each run);
 * with aerosols (LAERICESED || LAERICEAUTO, then of every set's parameters, and
 * picrit_aer, pre_ice, pnice required in every set) or without.  plude is
 * updated in place, so two runs of one batch differ as two cloudsc_gpu_run do.
 *
 * Aliasing (pointer equality only): sets may share any input member -- "one
 * state, N parameter sets".  The members the step writes (the selected outputs
 * and plude) are exclusive: none may equal any other non-NULL member of its
 * own set or any non-NULL member of another set.
 *
 * CLOUDSC_VARIANT_KCACHE only: KSEG's workspace and hand-off records are per
 * set.  The tendency-buffer, cumulative, per-column multiplier and advancing
 * forms, cloudsc_state_*, the host pipelines and the drop-in have no batch.
 *
 * CLOUDSC_EINVAL, all before the first HIP call: batch or sets NULL; nsets < 1
 * or > CLOUDSC_BATCH_MAX_SETS; ngptot or nproma < 1, nproma > 256 (KCACHE; so
 * also > 2^24), klev < 2; an unknown precision or `outputs`; a required member
 * NULL in any set; one of picrit_aer, pre_ice, pnice set in some sets and not in
 * others; with params: an invalid set, sets that disagree on LAERICESED ||
 * LAERICEAUTO, aerosol parameters without the three aerosol members; the
 * aliasing rule.  cloudsc_gpu_run_batch: batch NULL, or a variant other than
 * CLOUDSC_VARIANT_KCACHE (KSEG, SCC, SCC_PRIVATE, unknown, or with
 * CLOUDSC_FP32_EXACT_LIBM) -- checked before the batch is looked at.
 * CLOUDSC_ENODEV, CLOUDSC_ENOINIT, CLOUDSC_ENOMEM, CLOUDSC_EHIP as elsewhere. */
/* the member index is the launch's second grid dimension, which holds at most 65535 */
#define CLOUDSC_BATCH_MAX_SETS 65535
typedef struct cloudsc_batch cloudsc_batch_t;
int cloudsc_batch_create(cloudsc_batch_t **batch, int device, int precision, int outputs,
                         int nsets, int ngptot, int nproma, int klev,
                         const cloudsc_fields_t *sets,      /* host array[nsets] of device pointers */
                         const cloudsc_params_t *params);   /* NULL: the device's set; else array[nsets] */
int cloudsc_gpu_run_batch(cloudsc_batch_t *batch, void *stream, int variant);
int cloudsc_batch_nsets(const cloudsc_batch_t *batch);      /* CLOUDSC_EINVAL for NULL */
int cloudsc_batch_destroy(cloudsc_batch_t *batch);          /* waits for the device; NULL is CLOUDSC_OK */

/* Diagnostic: the number of polls a KSEG consumer makes before it gives up
 * (default 2^24, restored by a negative value).  0 makes every hand-off fail
 * without polling -- used by the tests of the error path. */
int cloudsc_debug_set_kseg_spin_limit(long long limit);

/* Diagnostic: override the KSEG schedule for this process -- nseg level
 * segments per column (1..16) and a grid of `grid` workgroups -- 0 restores
 * the measured default (2 guided segments, one workgroup per resident slot).
 * The result bits do not depend on either; the tests use it to exercise the
 * hand-offs with few workgroups and many segments. */
int cloudsc_debug_set_kseg_schedule(int nseg, int grid);

/* The launch geometry of the physics kernels.  A one-wave work unit is what one
 * wave computes for one level segment: a 64-column sub-block of a block, or,
 * packed, `pack` whole blocks of nproma <= 32 columns. */
typedef struct cloudsc_launch_geometry {
  int pack;           /* NPROMA blocks per wave (1 = unpacked)              */
  int lanes;          /* active lanes of a full wave: pack * min(nproma,64) */
  int units;          /* one-wave work units per level segment              */
  int workgroups;     /* grid the launch would use                          */
  int wg_threads;     /* threads per workgroup                              */
} cloudsc_launch_geometry_t;

/* What cloudsc_gpu_run would launch for these arguments; host arithmetic only, needs no GPU.
 * laer != 0: the aerosol kernels.  CLOUDSC_EINVAL as cloudsc_gpu_run would return it.
 * KSEG sizes its grid by the device it runs on: `workgroups` is the grid on an
 * MI355X (256 compute units, two resident waves per SIMD), or the grid of
 * cloudsc_debug_set_kseg_schedule, never more than segments x units. */
int cloudsc_gpu_launch_geometry(int precision, int variant, int ngptot, int nproma, int klev,
                                int laer, cloudsc_launch_geometry_t *out);
/* The same for the launch of a batch (cloudsc_gpu_run_batch, KCACHE): the geometry of one
 * set, with `units` and `workgroups` times nsets -- the grid is (workgroups of a set) x nsets.
 * CLOUDSC_EINVAL: nsets out of range, and what cloudsc_gpu_launch_geometry returns it for. */
int cloudsc_batch_launch_geometry(int precision, int nsets, int ngptot, int nproma, int klev, int laer,
                                  cloudsc_launch_geometry_t *out);

/* Process-wide: 1 pack blocks of nproma <= 32, 0 never, negative = the default
 * (per width, as measured: DESIGN.md §3.18).  Packing needs every lane offset
 * to fit 32 bits: a launch with 64 / nproma * 5 * (klev + 1) * nproma * 8 >=
 * 2^32 runs unpacked whatever the mode.  SCC and SCC_PRIVATE never pack. */
int cloudsc_debug_set_narrow_pack(int mode);

/* Diagnostic: field placement of the states created after this call.  < 0 (the
 * default): one device allocation per field.  >= 0: all fields of a state in
 * one allocation, field i starting at a 2 MiB boundary plus (i * stagger) mod
 * 2 MiB -- for measuring how the HBM placement of the ~47 concurrently
 * streamed fields affects the kernel time (tools/ab_layout.py).  stagger must
 * be a multiple of 256 bytes (CLOUDSC_EINVAL otherwise) and is taken modulo
 * 2 MiB.  alloc_flags must be 0 (CLOUDSC_EINVAL otherwise): states created
 * after destroyed states whose fields were hipDeviceMallocContiguous
 * allocations computed wrong values -- in part the round-3 parameter-upload
 * race (fixed), in part a cause not found (profiles/r04/contiguous_alloc_hazard.txt);
 * the diagnostic build (-DCLOUDSC_DEBUG_KNOBS) admits the flags to reproduce it. */
int cloudsc_debug_set_state_layout(long long stagger, unsigned alloc_flags);

/* Diagnostic: the kernels' single-precision exp/pow on the device, element-wise
 * over n host values: which = 0 the float-internal expf (CLOUDSC_FP32 default),
 * 1 its powf(x, y), 2 the glibc-algorithm expf (CLOUDSC_FP32_EXACT_LIBM),
 * 3 its powf, 4 the fast kernels' division x / y (v_rcp_f32 + one correction),
 * 5 the exact kernels' division.  y is read for 1, 3, 4 and 5 only. */
int cloudsc_debug_fp32_libm(int device, int which, const float *x, const float *y, float *out, long long n);

/* Diagnostic: the kernels' double-precision device primitives, element-wise
 * over n host values, one thread per element in workgroups of block_threads
 * (64, 128 or 256, CLOUDSC_EINVAL otherwise; every thread copies the exp/pow
 * tables to LDS first, with that stride).  which =
 *   0 exp(x) (hot body from the LDS tables, range check after it)
 *   1 pow(x, y) (the split form)
 *   2, 3 the first / second result of the paired exp of (x, y)
 *   4 x / y (hardware reciprocal, two Newton steps, one correction)
 *   5 x / y with the shared-reciprocal form (cl_recip)
 *   6 x / y with the known-divisor form, the reciprocal RN(1 / y)
 *   7 sqrt(x) as the exact kernels call it
 *   8, 9 the complete out-of-line exp(x), pow(x, y) (constant-memory tables)
 *        on every argument, in range or not.
 * y is read for every code except 0, 7 and 8. */
int cloudsc_debug_fp64_libm(int device, int which, int block_threads, const double *x, const double *y, double *out,
                            long long n);

/* Human-readable message for an error code; last HIP error string of this thread. */
const char *cloudsc_strerror(int code);
const char *cloudsc_last_hip_error(void);

/* Measurement: the achievable HBM bandwidth of this device, a STREAM copy
 * between two buffers of bytes / 2 (>= 1 MiB each; 2 x bytes / 2 moved per
 * launch) in 16-byte-per-lane tiles, over three such buffer pairs allocated
 * together (their placement moves the rate by ~5 %), `reps` launches of each
 * tile shape per pair after one warm-up; the best launch, in GB/s (10^9 B/s).
 * bench.py reports it as roofline.achievable_peak beside the 8 TB/s spec. */
int cloudsc_hbm_copy_gbps(int device, long long bytes, int reps, double *gbps);

/* Measurement: the host<->device copy ceiling of this device, the bound of the
 * host-buffer pipeline: `bytes` (>= 1 MiB) of pinned host memory each way, one
 * stream per direction, 64 MiB copies; *h2d and *d2h one direction alone,
 * *both the total of the two directions copied at once; GB/s, best of `reps`.
 * bench.py reports pcie_inclusive against it. */
int cloudsc_pcie_gbps(int device, long long bytes, int reps, double *h2d, double *d2h, double *both);

/* Measurement: stream `bytes` (>= 1 MiB, a multiple of 16) through one device
 * buffer with `width` (4, 8 or 16) bytes per lane per access, non-temporal,
 * consecutive lanes on consecutive elements -- the CLOUDSC kernels' access
 * shape at width 8 (fp64) and 4 (fp32) -- as a read (mode 0) or a write
 * (mode 1); *ms = the fastest of `reps` launches.  A rocprofv3 PMC pass over it
 * calibrates FETCH_SIZE / WRITE_SIZE for those widths (tools/calib_counters.py). */
int cloudsc_debug_stream_probe(int device, int mode, int width, long long bytes, int reps, double *ms);

/* ABI introspection for bindings: sizeof of the public structs
 * (0 params, 1 fields, 2 template, 3 reference, 4 stats), -1 otherwise.
 * Later structs report their own size: cloudsc_fields_diff_sizeof. */
long long cloudsc_abi_sizeof(int which);

/* ------------------------------------------------------------------------ */
/* CPU variant (BASELINE.json config 1): explicitly selected, never a fallback */
/* ------------------------------------------------------------------------ */

/* One CLOUDSC step over ngptot columns in HOST memory (block layout, fp64),
 * on `nthreads` host threads (<= 0: all hardware threads) taking NPROMA blocks
 * from a shared counter -- the C dwarf's OpenMP block loop
 * (src/cloudsc_c/cloudsc/cloudsc_driver.c:183-217) around the kernel
 * cloudsc_c() (cloudsc_c.c:19-2587).  The per-level physics is the same source
 * the GPU kernels are built from, compiled for the host; the output is the
 * reference kernel's bit for bit.  Same output contract as cloudsc_gpu_run
 * (every output element written, plude read-modify-write).  *seconds (may be
 * NULL) = wall time of the block loop.  Needs no GPU. */
int cloudsc_cpu_run(int nthreads, int ngptot, int nproma, int klev, const cloudsc_params_t *params,
                    const cloudsc_fields_t *host_fields, double *seconds);

/* cloudsc_cpu_run for a precision code: CLOUDSC_FP64 (cloudsc_cpu_run itself)
 * or CLOUDSC_MIXED -- host_fields then holds float arrays, the same phase
 * functions run in double between a widening load and a narrowing store, and
 * the output is the CLOUDSC_MIXED contract above, bit for bit, on a machine
 * without a GPU.  Any other code: CLOUDSC_EINVAL (the fp32 arithmetic has no
 * host form). */
int cloudsc_cpu_run_precision(int nthreads, int precision, int ngptot, int nproma, int klev,
                              const cloudsc_params_t *params, const cloudsc_fields_t *host_fields,
                              double *seconds);

/* cloudsc_cpu_run with the C dwarf's per-thread record (zinfo,
 * cloudsc_driver.c:185-228, printed as the "@ core#" rows at :238-253): for
 * thread t < nthreads, thread_seconds[t] = its wall time, thread_blocks[t] =
 * NPROMA blocks it took (icalls), thread_columns[t] = columns it computed
 * (igpc).  Each array (may be NULL) holds nthreads entries; nthreads must be
 * > 0 here.  Threads beyond the block count report zeros. */
int cloudsc_cpu_run_threads(int nthreads, int ngptot, int nproma, int klev, const cloudsc_params_t *params,
                            const cloudsc_fields_t *host_fields, double *seconds, double *thread_seconds,
                            int *thread_blocks, int *thread_columns);

/* ------------------------------------------------------------------------ */
/* Dwarf plumbing on the device: expand a KLON-column template to NGPTOT      */
/* columns (global column g -> template column g % klon, load_state.c:69-184, */
/* expand_mod.F90:173-200), run, time, and validate against a KLON-column     */
/* reference with the Fortran ERROR_PRINT statistics (validate_mod.F90:263). */
/* ------------------------------------------------------------------------ */

/* Template / reference arrays in the HDF5 / Serialbox order: [lev][klon],
 * species [nclv][lev][klon], surface [klon].  Always double (fp32 runs convert
 * at expansion, as file_io_mod.F90:96-112 does). */
typedef struct cloudsc_template {
  int klon, klev;
  const double *pt, *pq, *tendency_tmp_t, *tendency_tmp_q, *tendency_tmp_a, *tendency_tmp_cld;
  const double *pvfl, *pvfi, *phrsw, *phrlw, *pvervel, *pap, *paph, *plsm;
  const int    *ktype;
  const double *plu, *plude, *psnde, *pmfu, *pmfd, *pa, *pclv, *psupsat;
  const double *plcrit_aer, *picrit_aer, *pre_ice, *pccn, *pnice;   /* may be NULL */
} cloudsc_template_t;

/* The 21 validated fields, in the dwarf's print order (cloudsc_validate.c:193-216). */
#define CLOUDSC_NVALID 21
enum cloudsc_field_id {
  CLOUDSC_F_PLUDE = 0, CLOUDSC_F_PCOVPTOT, CLOUDSC_F_PRAINFRAC_TOPRFZ,
  CLOUDSC_F_PFSQLF, CLOUDSC_F_PFSQIF, CLOUDSC_F_PFCQLNG, CLOUDSC_F_PFCQNNG,
  CLOUDSC_F_PFSQRF, CLOUDSC_F_PFSQSF, CLOUDSC_F_PFCQRNG, CLOUDSC_F_PFCQSNG,
  CLOUDSC_F_PFSQLTUR, CLOUDSC_F_PFSQITUR, CLOUDSC_F_PFPLSL, CLOUDSC_F_PFPLSN,
  CLOUDSC_F_PFHPSL, CLOUDSC_F_PFHPSN, CLOUDSC_F_TENDENCY_LOC_A,
  CLOUDSC_F_TENDENCY_LOC_Q, CLOUDSC_F_TENDENCY_LOC_T, CLOUDSC_F_TENDENCY_LOC_CLD
};

/* Reference outputs for the KLON template columns, same order as the enum;
 * each array in template order ([lev][klon], [nclv][lev][klon] or [klon]). */
typedef struct cloudsc_reference {
  int klon, klev;
  const double *field[CLOUDSC_NVALID];
} cloudsc_reference_t;

/* Per-field statistics, the inputs of ERROR_PRINT (validate_mod.F90:263-296).
 * The two sums are carried as double-doubles: errsum / refsum are the sums
 * rounded to double, errsum_lo / refsum_lo what that rounding left over (all
 * terms are non-negative, so hi + lo holds the sum to ~100 bits).  Sums of
 * partial statistics -- NPROMA blocks on the device, shards on the host, the
 * MPI_Reduce of validate_mod.F90:53-55 -- therefore depend on how the columns
 * were partitioned only within the double-double error (~2^-100 relative): in
 * practice a sharded run prints the unsharded run's table to the last digit; a
 * total within that distance of a rounding midpoint could round 1 ulp apart.
 * Combine partials with cloudsc_stats_combine. */
typedef struct cloudsc_stats {
  double minval, maxval, maxerr, errsum, refsum;
  double errsum_lo, refsum_lo;
} cloudsc_stats_t;

/* acc <- acc (+) part: min of mins, max of maxes and of max|d|, double-double
 * sums.  Start from {DBL_MAX, -DBL_MAX, 0, 0, 0, 0, 0}. */
void cloudsc_stats_combine(cloudsc_stats_t *acc, const cloudsc_stats_t *part);

typedef struct cloudsc_gpu_state cloudsc_gpu_state_t;

/* Allocate device buffers for columns [col_offset, col_offset+ngptot) of the
 * global problem and expand the template into them on the device (g % klon
 * with g the GLOBAL column index, so a sharded run is bit-identical to an
 * unsharded one).  Keeps a pristine copy of plude for repeated runs. */
int cloudsc_state_create(cloudsc_gpu_state_t **state, int device, int precision,
                         int ngptot, int nproma, long long col_offset,
                         const cloudsc_template_t *tmpl, const cloudsc_params_t *params);

/* Device pointers of the state's buffers (block layout) -- for callers that
 * want to drive cloudsc_gpu_run themselves (cloudsc_gpu_run uses the device's
 * default parameter set, not the state's). */
int cloudsc_state_fields(const cloudsc_gpu_state_t *state, cloudsc_fields_t *out);

/* How the state's output fields were placed (round 4).  The rate at which
 * the kernel writes its 21 output fields depends on where they land in HBM
 * (fp64 KSEG 1.63-1.94 ms for states of one configuration: fields written
 * together whose physical pages collide stall on DRAM write credits).  At
 * creation the state times the KSEG kernel on its own inputs over candidate
 * placements of its outputs -- eight whole fresh output sets (the last seven
 * shuffled with spacers), then one field at a time -- then of its inputs
 * (four whole fresh input sets, the last three shuffled with spacers,
 * contents copied), and keeps a candidate when the time drops by more than
 * 1 %.  Each rejected input set is freed as soon as it loses.
 * If the search's launches time out in a segment hand-off, the first
 * placement is kept and probe_final_ms is negative (the state is created).
 * probe_first_ms / probe_final_ms: the kernel time of the first / the kept
 * placement, tries / moves: buffers (outputs and inputs) allocated as
 * candidates / kept.  Cost (wall time, launches, transient bytes):
 * cloudsc_state_placement_report.
 * All zero when the search was off.  Any pointer may be NULL. */
int cloudsc_state_placement(const cloudsc_gpu_state_t *state, float *probe_first_ms, float *probe_final_ms,
                            int *tries, int *moves);

/* The placement search of the state (cloudsc_state_placement) with its cost:
 * all of it, outputs and inputs, method CLOUDSC_PLACE_METHOD_KERNEL, or
 * CLOUDSC_PLACE_METHOD_NONE with zeros when the search was off. */
int cloudsc_state_placement_report(const cloudsc_gpu_state_t *state, cloudsc_placement_t *report);

/* Passes of the output placement search of the states created after this
 * call, process-wide (0 = off: the first allocation is kept; negative = the
 * default, 2; at most 8).  The results do not depend on it; the search costs
 * ~0.5 s of kernel launches per fp64 state at NGPTOT=163840 and pays off only
 * over many steps (the CLI turns it off for one step). */
int cloudsc_set_placement_search(int passes);
/* The same (the name of rounds 3-4). */
int cloudsc_debug_set_placement_search(int passes);

/* Measurement: the memory-pattern probe (csrc/cloudsc_place.hip) over the
 * device fields f: one wave per 64-column sub-block streams the level planes
 * the way the KSEG kernel does, with no physics.  mode 0 writes every non-NULL
 * output field; mode 1 also reads every input field.  *ms = best of `reps`
 * timed launches after one untimed.  Outputs (plude included) are
 * overwritten with junk; input contents do not matter.  It ranks placements
 * of a field set without its contents (tools/place_corr.py). */
int cloudsc_debug_memory_probe(int device, int precision, int ngptot, int nproma, int klev,
                               const cloudsc_fields_t *f, int mode, int reps, float *ms);

/* Diagnostic (round 6 layout study, tools/layout_corr.py): the same probe over
 * fields in another HBM layout.  strides[6] = the element strides between
 * blocks, between rows (levels) and between species planes of the inputs, then
 * of the outputs; 0 keeps the reference block layout's.  Each field pointer
 * addresses row 0 of block 0 (species 0) of its field; every element the
 * strides address must lie inside that field's allocation. */
int cloudsc_debug_memory_probe_layout(int device, int precision, int ngptot, int nproma, int klev,
                                      const cloudsc_fields_t *f, int mode, int reps, const long long *strides,
                                      float *ms);

/* Diagnostic, diagnostic build only (-DCLOUDSC_DEBUG_CANARY; otherwise
 * CLOUDSC_EINVAL): every device buffer of the states and placement searches
 * carries a 64 KiB guard band of a known byte on each side.  *live = guarded
 * buffers alive, *bad_allocs = those with a changed guard byte, *bad_bytes =
 * changed guard bytes in them plus those found when buffers were freed since
 * the last call.  For the round-5 record of the contiguous-allocation failure
 * (tools/contig_diag_r05.py). */
int cloudsc_debug_canary_check(int *live, int *bad_allocs, long long *bad_bytes);

/* Diagnostic: copy `bytes` (a multiple of 4) from device memory src to dst
 * with a kernel (4-byte vector loads and stores through the caches, a grid
 * over all XCDs), then wait -- to compare what the shader cores read with what
 * a copy engine (hipMemcpy) reads from the same memory. */
int cloudsc_debug_kernel_copy(void *dst, const void *src, long long bytes);

/* Diagnostic: move field `member` (its position in cloudsc_fields_t) of a state
 * to a new device allocation, contents copied; the old allocation is kept until
 * the state is destroyed, so the field lands on other physical pages.  For
 * finding which fields' placement decides the kernel time
 * (tools/placement_fields.py).  CLOUDSC_EINVAL for a member the state does not
 * hold (aerosol fields it was created without). */
int cloudsc_debug_state_relocate_field(cloudsc_gpu_state_t *s, int member);

/* Diagnostic: the same for a state buffer that is not a field: which = 0 the
 * pristine plude copy, 1 the KSEG workspace (zeroed again before the next
 * launch), 2 the SCC temporaries.  CLOUDSC_EINVAL when the state does not hold
 * it yet (workspaces are allocated on first use). */
int cloudsc_debug_state_relocate_aux(cloudsc_gpu_state_t *s, int which);

/* Restore plude from the pristine copy -- for callers that run in place
 * through cloudsc_gpu_run on the state's buffers. */
int cloudsc_state_reset(cloudsc_gpu_state_t *state);

/* Launch `reps` back-to-back steps of `variant` on the state's stream and
 * time each with HIP events recorded on that stream, with the state's own
 * parameter set.  The INOUT field plude
 * is taken out of place: every step reads the pristine input copy and writes
 * its result to the state's plude buffer, so repeated steps compute the same
 * step without a restore copy.  ms_per_step[reps] receives the per-step
 * kernel time, recorded by each launch's own dispatch (may be NULL: then no
 * events are recorded).  KSEG: CLOUDSC_EHANDOFF if a segment hand-off
 * timed out (cloudsc_gpu_check). */
int cloudsc_state_run(cloudsc_gpu_state_t *state, int variant, int reps, float *ms_per_step);

/* As cloudsc_state_run, timed as a whole: `reps` plain dispatches back to
 * back between two events on the state's stream; *span_ms = the time from the
 * first launch's start to the last one's end.  A dispatch that records its own
 * events (cloudsc_state_run with ms_per_step) leaves ~5 us more between
 * kernels than a plain one; span_ms / reps is the sustained time per step. */
int cloudsc_state_run_span(cloudsc_gpu_state_t *state, int variant, int reps, float *span_ms);

/* Wait for all work of the state's stream. */
int cloudsc_state_sync(cloudsc_gpu_state_t *state);

/* Measurement: the effective shader clock of the state's KSEG launches since
 * the last reset, in GHz -- every workgroup adds the shader-clock cycles
 * (s_memtime) and the 100 MHz real-time ticks (s_memrealtime) it spent in the
 * kernel to two counters in the KSEG workspace; *ghz = cycles / ticks x the
 * real-time rate (0 before any KSEG launch).  Waits for the state's stream;
 * reset != 0 zeroes the counters afterwards.  bench.py reports it beside the
 * kernel time (the fp64 kernel follows the board's clock). */
int cloudsc_state_kseg_clock(cloudsc_gpu_state_t *state, int reset, double *ghz);

/* Field-wise statistics vs a KLON-column reference, computed on the device
 * (modulo indexing; no expanded reference in host or device memory):
 * cloudsc_fields_validate on the state's own fields, stream and column offset.
 * Waits for the state's stream.  It uses the device's compare / validate /
 * expand workspace (below) behind its mutex, so concurrent validations on one
 * device serialise, and cloudsc_fields_compare_release frees what it grew.
 * CLOUDSC_EINVAL: a NULL argument, a NULL array in ref->field[] (CLOUDSC_EHIP
 * before the state validated through the field-set kernel), ref->klon < 1,
 * ref->klev != the state's. */
int cloudsc_state_validate(cloudsc_gpu_state_t *state, const cloudsc_reference_t *ref,
                           cloudsc_stats_t stats[CLOUDSC_NVALID]);

/* Copy one validated output field to host memory in BLOCK layout as doubles
 * (fp32 and mixed states are widened, exactly).  `host` must hold the field's
 * blocked size. */
int cloudsc_state_download(cloudsc_gpu_state_t *state, int field_id, double *host);

/* Element count of a validated field in block layout for this state. */
long long cloudsc_state_field_elems(const cloudsc_gpu_state_t *state, int field_id);

int cloudsc_state_destroy(cloudsc_gpu_state_t *state);

/* ------------------------------------------------------------------------ */
/* Caller-owned field sets on the device: fill, validate, compare            */
/* ------------------------------------------------------------------------ */
/* The reference CUDA driver's shape (cloudsc_driver.cu:276-447) without a host
 * copy of any field: cloudsc_fields_alloc, cloudsc_fields_expand,
 * cloudsc_gpu_run, cloudsc_gpu_check, cloudsc_fields_validate -- and
 * cloudsc_fields_compare to hold two such sets against each other.
 * compare, validate and expand share one workspace per device (the partial
 * results, the uploaded reference or template), allocated on first use, grown
 * on demand, guarded by a mutex: calls on one device serialise.  Only the
 * first call on a device and a call that grows the workspace synchronise the
 * whole device; cloudsc_fields_compare_release frees it.  None of them needs
 * cloudsc_gpu_init. */

/* What cloudsc_fields_compare reports for one cloudsc_fields_t member. */
typedef struct cloudsc_field_diff {
  cloudsc_stats_t stats;              /* a against b as the reference                         */
  long long compared;                 /* elements compared: rows x ngptot; 0 = member skipped */
  long long mismatches;               /* elements that differ as bits                         */
  long long first_column, first_row;  /* the first mismatch, -1 / -1 if none                  */
} cloudsc_field_diff_t;

/* Number of cloudsc_fields_t members (the length of diff[] below) and
 * sizeof(cloudsc_field_diff_t), for bindings. */
int cloudsc_fields_members(void);
long long cloudsc_fields_diff_sizeof(void);

/* Compare two field sets on `device`, in any two NPROMA blockings and storage
 * types, in one streaming pass that reads every element once and writes none.
 * For every member that is non-NULL in both sets, every row of its kind and
 * every global column g < ngptot, with v the element of a and r the element of
 * b, both widened to double (exact; ktype is compared as int32):
 *   stats    min v, max v (fmin / fmax), max |v - r|, sum |v - r|, sum |r| --
 *            the ERROR_PRINT inputs with b as the reference, the sums as
 *            double-doubles (cloudsc_stats_t)
 *   mismatches  elements that differ AS BITS: the raw words when both sets have
 *            the same storage type, otherwise the 64-bit words after widening
 *            the float.  +0 against -0 counts (with |v - r| = 0); NaN against
 *            the same NaN word does not.  A NaN in an active lane makes the
 *            sums NaN; min, max and max |v - r| skip it.
 *   first_column / first_row  the mismatch with the smallest global column
 *            and, in that column, the smallest row.
 * diff[] has one record per cloudsc_fields_t member, in member order
 * (cloudsc_fields_members()).  A member that is NULL in both sets is skipped:
 * compared = 0, -1 / -1, stats = {DBL_MAX, -DBL_MAX, 0, ...}.  min, max,
 * max |v - r|, the counts and the first mismatch do not depend on the launch
 * grid or on either NPROMA; the sums depend on the grouping only within the
 * double-double bound stated at cloudsc_stats_t.  Padding lanes of a last
 * partial block are never read.
 * CLOUDSC_EINVAL: a member that is NULL in exactly one set, no member in both,
 * an unknown precision code, ngptot, klev or an NPROMA < 1, an NPROMA > 2^24,
 * a NULL struct or diff.  The same pointer on both sides is allowed (nothing
 * is written).  Every argument is checked before the first HIP call: a bad
 * argument is CLOUDSC_EINVAL on a machine without a GPU too.
 * Enqueues on `stream` (a hipStream_t, NULL = the default stream), waits for
 * THAT STREAM ONLY and then writes diff[]. */
int cloudsc_fields_compare(int device, void *stream, int ngptot, int klev,
                           int a_precision, int a_nproma, const cloudsc_fields_t *a,
                           int b_precision, int b_nproma, const cloudsc_fields_t *b,
                           cloudsc_field_diff_t *diff);

/* cloudsc_fields_compare for two sets of one output selection.  With
 * CLOUDSC_OUTPUTS_SURFACE the members pfplsl, pfplsn, pfhpsl, pfhpsn of both
 * sets are surface fields ([nblocks][nproma], one row: compared = ngptot,
 * first_row 0); every other member is walked by its kind.  With
 * CLOUDSC_OUTPUTS_ALL and CLOUDSC_OUTPUTS_PROGNOSTIC it IS cloudsc_fields_compare.
 * CLOUDSC_EINVAL: an unknown `outputs` value and every argument error of
 * cloudsc_fields_compare, before the first HIP call. */
int cloudsc_fields_compare_outputs(int device, void *stream, int ngptot, int klev, int outputs,
                                   int a_precision, int a_nproma, const cloudsc_fields_t *a,
                                   int b_precision, int b_nproma, const cloudsc_fields_t *b,
                                   cloudsc_field_diff_t *diff);

/* The same on HOST arrays, on `nthreads` host threads (<= 0: all hardware
 * threads) taking blocks of a from a shared counter, the threads' records
 * combined in thread order: the same semantics and errors.  Needs no GPU. */
int cloudsc_cpu_fields_compare(int nthreads, int ngptot, int klev,
                               int a_precision, int a_nproma, const cloudsc_fields_t *a,
                               int b_precision, int b_nproma, const cloudsc_fields_t *b,
                               cloudsc_field_diff_t *diff);

/* cloudsc_fields_compare with the eight tendency members of either side in a
 * packed tendency buffer (above, "Packed tendency buffers"): where
 * a_tend_planes (b_tend_planes) is non-zero, the tendency members of a (b) have
 * the block stride *_tend_planes * klev * *_nproma elements; 0 means separate
 * arrays, and 0 and 0 is cloudsc_fields_compare.  Nothing is written; padding
 * lanes and planes no member points at are never read.  diff[] is as there:
 * compared, first_column and first_row count in the member's own rows, and
 * min, max, the counts and the first mismatch do not depend on the grid or on
 * either blocking.  CLOUDSC_EINVAL as cloudsc_fields_compare, and for a
 * non-zero *_tend_planes outside 8..64; checked before the first HIP call. */
int cloudsc_fields_compare_tendbuf(int device, void *stream, int ngptot, int klev,
                                   int a_precision, int a_nproma, int a_tend_planes, const cloudsc_fields_t *a,
                                   int b_precision, int b_nproma, int b_tend_planes, const cloudsc_fields_t *b,
                                   cloudsc_field_diff_t *diff);

/* The same on HOST arrays, as cloudsc_cpu_fields_compare.  Needs no GPU. */
int cloudsc_cpu_fields_compare_tendbuf(int nthreads, int ngptot, int klev,
                                       int a_precision, int a_nproma, int a_tend_planes, const cloudsc_fields_t *a,
                                       int b_precision, int b_nproma, int b_tend_planes, const cloudsc_fields_t *b,
                                       cloudsc_field_diff_t *diff);

/* cloudsc_state_validate for a caller-owned set: the 21 validated members of
 * `fields` (all must be set: a set of CLOUDSC_OUTPUTS_PROGNOSTIC, whose ten
 * diagnostic fluxes are NULL, is validated with cloudsc_fields_validate_tendbuf
 * below) against the KLON-column reference, read as
 * ref[row][(col_offset + g) % klon] -- the comparison kernel with the
 * reference as its second operand.  The reference arrays are uploaded on
 * `stream`, ordered before the one launch; the call waits for that stream only
 * and writes stats[CLOUDSC_NVALID] in cloudsc_field_id order.  CLOUDSC_EINVAL:
 * a NULL argument, validated member or reference array, an unknown precision,
 * a size < 1, nproma > 2^24, col_offset < 0, ref->klev != klev, ref->klon < 1
 * (checked before the first HIP call). */
int cloudsc_fields_validate(int device, void *stream, int precision, int ngptot, int nproma, int klev,
                            long long col_offset, const cloudsc_fields_t *fields,
                            const cloudsc_reference_t *ref, cloudsc_stats_t *stats);

/* cloudsc_fields_validate reading the eight tendency members in place from
 * packed tendency buffers (tend_planes planes per block, 8..64; 0: separate
 * arrays), with an output selection.  With CLOUDSC_OUTPUTS_PROGNOSTIC each of
 * the ten diagnostic members may be NULL together with its reference array;
 * its stats[] record is then the "skipped" record of cloudsc_fields_compare,
 * {DBL_MAX, -DBL_MAX, 0, ...}.  A diagnostic member that is non-NULL while its
 * reference array is NULL, or the reverse, is CLOUDSC_EINVAL; one present on
 * both sides is validated.  With CLOUDSC_OUTPUTS_SURFACE the same holds for the
 * ten, and the four surface fields pfplsl, pfplsn, pfhpsl, pfhpsn are compared
 * with row klev of their reference profiles ([klev+1][klon], required): their
 * stats[] records, under the usual ids, are the statistics of that row alone.
 * tend_planes 0 with CLOUDSC_OUTPUTS_ALL is
 * cloudsc_fields_validate.  Nothing is written to the fields; padding lanes and
 * planes no member points at are never read.  CLOUDSC_EINVAL also: an unknown
 * `outputs` value, a non-zero tend_planes outside 8..64 and every argument
 * error of cloudsc_fields_validate (checked before the first HIP call). */
int cloudsc_fields_validate_tendbuf(int device, void *stream, int precision, int ngptot, int nproma, int klev,
                                    int tend_planes, int outputs, long long col_offset,
                                    const cloudsc_fields_t *fields, const cloudsc_reference_t *ref,
                                    cloudsc_stats_t *stats);

/* cloudsc_state_create's expansion for a caller-owned set: fills every
 * non-NULL INPUT member of `fields` (aerosol inputs and plude included; the
 * outputs are left alone) from the host template,
 *   dst[b][row][i] = (storage type) tmpl[row][(col_offset + b * nproma + i) % klon]
 * for the columns b * nproma + i < ngptot: padding lanes of a last partial
 * block are never written.  klev is the template's.  A member to fill whose
 * template array is NULL, no member to fill, col_offset < 0, an unknown
 * precision or a bad size: CLOUDSC_EINVAL before the first HIP call.
 * Asynchronous on `stream`: the template arrays are copied into the library's
 * pinned staging buffer before the call returns, so the caller may change or
 * free them at once; the fields are filled in stream order (synchronise
 * `stream`, or enqueue the consumer on it).  The call itself never waits for
 * `stream`; the next compare / validate / expand call on this device first
 * waits for this expansion's kernel, which still reads the staged template. */
int cloudsc_fields_expand(int device, void *stream, int precision, int ngptot, int nproma,
                          long long col_offset, const cloudsc_template_t *tmpl, const cloudsc_fields_t *fields);

/* cloudsc_fields_expand writing the tendency members (tendency_tmp_*; the
 * tendency_loc_* are outputs and left alone) straight into their planes of a
 * packed tendency buffer with tend_planes planes per block (8..64): only the
 * planes the members point at and the lanes of real columns are written.  The
 * same asynchrony and staging rules.  CLOUDSC_EINVAL: tend_planes outside 8..64
 * and every argument error of cloudsc_fields_expand, before the first HIP call. */
int cloudsc_fields_expand_tendbuf(int device, void *stream, int precision, int ngptot, int nproma,
                                  int tend_planes, long long col_offset, const cloudsc_template_t *tmpl,
                                  const cloudsc_fields_t *fields);

/* Free the device's compare / validate / expand workspace (after waiting for a
 * pending expansion); the next such call allocates it again. */
int cloudsc_fields_compare_release(int device);

/* Diagnostic: the grid of the comparison kernel (cloudsc_fields_compare and
 * cloudsc_fields_validate), process-wide: `workgroups` 256-thread workgroups,
 * 0 = the default, eight per compute unit (never more than there are work
 * items).  Negative or > 65536: CLOUDSC_EINVAL.  Only the low parts of the sums
 * may depend on it; the tests run the same comparison on 1 and 3 workgroups. */
int cloudsc_debug_set_compare_grid(int workgroups);

/* ------------------------------------------------------------------------ */
/* Host-buffer pipeline: the reference GPU drivers' H2D -> kernel -> D2H      */
/* (cloudsc_driver.cu:344-456), chunked and overlapped across streams         */
/* ------------------------------------------------------------------------ */
typedef struct cloudsc_host_pipeline cloudsc_host_pipeline_t;

/* `host` holds HOST pointers in block layout (full NPROMA blocks, the
 * precision's element type, ktype int).  The arrays are pinned in place
 * (hipHostRegister) until destroy; device buffers for `nstreams` chunk slots of
 * `chunk_blocks` blocks each are allocated here (1..16; chunk c uses slot
 * c % nstreams).  CLOUDSC_FP64 and CLOUDSC_FP32 only: CLOUDSC_MIXED returns
 * CLOUDSC_EINVAL.  cloudsc_gpu_init must have been called for the device; the
 * pipeline keeps a copy of the device's default parameter set as it is at
 * creation. */
int cloudsc_host_pipeline_create(cloudsc_host_pipeline_t **pipe, int device, int precision, int ngptot,
                                 int nproma, int klev, int chunk_blocks, int nstreams,
                                 const cloudsc_fields_t *host);

/* One step over all columns, pipelined over three streams: every H2D copy
 * (inputs, plude) on one, every kernel on a second, every D2H copy (outputs,
 * plude) on a third, ordered per chunk slot by events, so chunk c's inputs
 * move in while chunk c-1 computes and chunk c-2's outputs move out.  *ms =
 * elapsed time of the whole pipeline (transfers included), HIP events on the
 * null stream.  KSEG: CLOUDSC_EHANDOFF if a segment hand-off timed out in any
 * chunk. */
int cloudsc_host_pipeline_run(cloudsc_host_pipeline_t *pipe, int variant, double *ms);

int cloudsc_host_pipeline_destroy(cloudsc_host_pipeline_t *pipe);

/* Diagnostic: how the pipeline's host arrays are mapped for the device.
 * *n_arrays = the number of non-NULL host arrays; *n_not_one_mapping = how many
 * of them are NOT covered by a single pinned mapping from their first to their
 * last byte (hipPointerGetAttributes at both ends, device addresses exactly
 * bytes-1 apart).  0 is the invariant create establishes (merged page ranges,
 * each registered once). */
int cloudsc_debug_host_pipeline_mapping(const cloudsc_host_pipeline_t *pipe, int *n_arrays,
                                        int *n_not_one_mapping);

/* Diagnostic: 1 if [ptr, ptr+bytes) is currently pinned host memory reachable
 * by the device as one mapping, 0 if not (e.g. after the pipeline that pinned
 * it was destroyed). */
int cloudsc_debug_host_pinned(const void *ptr, long long bytes);

/* Diagnostic: how host pipeline steps run after this call move their data.
 * 1 (the default; negative restores it): every copy issued by the pipeline on
 * a copy engine of its own per direction (hsa_amd_memory_async_copy_on_engine,
 * engines chosen at creation), ordered with the kernels from the host -- the
 * runtime's own engine choice for hipMemcpyAsync lets both directions land on
 * one engine now and then, which serialises them (~1.7-3.3x slower steps,
 * profiles/r04/pipeline_engines.txt).  0: three HIP streams (one per
 * direction, one for the kernels) with the runtime's engine choice.  2: as 0,
 * with the outputs written back by a copy kernel through the pinned memory's
 * device address.  A pipeline whose engines could not be set up at creation
 * runs as 0.  CLOUDSC_EINVAL for other modes. */
int cloudsc_debug_set_pipeline_copy(int mode);

/* Diagnostic: the copy path a pipeline was set up with: *mode 1 with the
 * engine masks (hsa_amd_sdma_engine_id_t bits) it copies on per direction, or
 * 0 (HIP streams) with both masks 0.  Any output pointer may be NULL. */
int cloudsc_debug_host_pipeline_copy(const cloudsc_host_pipeline_t *pipe, int *mode, int *h2d_engine,
                                     int *d2h_engine);

/* Measurement: the time of one step's copies WITHOUT the kernels, on the same
 * copy engines, host arrays and device slots (every input H2D, every output
 * D2H, each direction back to back on its engine): the bound a step of this
 * pipeline is held against (bench.py's pcie_inclusive.bound_ms).  The host
 * OUTPUT arrays and plude receive the device slots' contents, not results:
 * run a step (with plude restored) before reading outputs again.
 * CLOUDSC_EINVAL when the pipeline has no copy engines (HIP-stream mode). */
int cloudsc_host_pipeline_copy_bound(cloudsc_host_pipeline_t *pipe, double *ms);

/* Diagnostic: the engine pair check a pipeline ran at creation (copy mode 1):
 * *overlap = time of 256 MiB each way at once / the slower direction alone
 * (1.0 = the directions fully concurrent, 2.0 = serialised) for the pair it
 * kept, *pairs_tried = engine pairs measured (the first pair under 1.3 is
 * kept, else the best of at most 6).  Both 0 in HIP-stream mode. */
int cloudsc_debug_host_pipeline_engine_check(const cloudsc_host_pipeline_t *pipe, double *overlap,
                                             int *pairs_tried);

/* ------------------------------------------------------------------------ */
/* One synchronous step on host arrays, callable from any host thread        */
/* ------------------------------------------------------------------------ */
/* The per-block call of the reference C dwarf's OpenMP loop
 * (src/cloudsc_c/cloudsc/cloudsc_driver.c:183-217 calls cloudsc_c() on one
 * NPROMA block from every thread) moved to the device: copy the inputs and
 * plude in (pageable memory is fine), run `variant`, copy the outputs and plude
 * back, wait.  `host` holds HOST pointers in block layout, like
 * cloudsc_cpu_run.  No cloudsc_gpu_init is needed: each calling thread keeps,
 * per device, its own stream, device buffers (grown to the largest call), KSEG
 * workspace and parameter set (uploaded again only when *params changes), so
 * concurrent callers share nothing.  Same output contract as cloudsc_gpu_run.
 * CLOUDSC_FP64 and CLOUDSC_FP32 only: CLOUDSC_MIXED returns CLOUDSC_EINVAL.
 * The drop-in cloudsc_c() of libcloudsc_c_amd_gpu.so (csrc/cloudsc_c_dropin.c)
 * is built on it. */
int cloudsc_host_run(int device, int precision, int variant, int ngptot, int nproma, int klev,
                     const cloudsc_params_t *params, const cloudsc_fields_t *host);

/* Free the calling thread's cloudsc_host_run contexts (device buffers, stream,
 * parameter sets) on every device; the next cloudsc_host_run creates them again. */
int cloudsc_host_run_release(void);

/* Where a cloudsc_host_run call's time goes (round 6, VERDICT r05 weak 6: the
 * GPU drop-in's per-call cost).  Sums over the calls of every thread since
 * profiling was enabled, in ms, each thread's FIRST call on a device left out
 * of them (it creates the thread's context and, in a fresh process, starts the
 * HIP runtime: first_calls / first_calls_ms count those apart): host side measured with a steady clock, the
 * device side with HIP events on the call's stream between its three
 * operations.  alloc: the calling thread's context, device selection, parameter
 * upload and buffer growth (the first calls: the HIP runtime's own start-up
 * lands here); setup: argument checks and the image layout; enqueue: issuing
 * the copies and the launch; pack / unpack: the active lanes between the caller's
 * arrays and the pinned staging buffer; h2d / kernel / d2h: the input copy, the
 * CLOUDSC launch (the KSEG prepare kernel included) and the output copy on the
 * device; wait: from the last enqueue to the stream sync's return (the device
 * work the host waits for); total: whole calls = alloc + setup + pack +
 * enqueue + wait + unpack. */
typedef struct cloudsc_host_run_profile {
  long long calls;
  double setup_ms, pack_ms, h2d_ms, kernel_ms, d2h_ms, wait_ms, unpack_ms, total_ms;
  double alloc_ms;     /* part of total_ms, not of setup_ms */
  double enqueue_ms;
  double max_call_ms;  /* the slowest single call counted */
  long long first_calls;
  double first_calls_ms;
} cloudsc_host_run_profile_t;
/* mode 1: zero the sums and start profiling (each call then records 4 events);
 * mode 0: copy the sums into *out (may be NULL) and keep profiling;
 * mode -1: copy the sums into *out (may be NULL) and stop. */
int cloudsc_host_run_profile(int mode, cloudsc_host_run_profile_t *out);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDSC_AMD_H */
