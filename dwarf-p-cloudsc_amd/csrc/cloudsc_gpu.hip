// cloudsc_gpu.hip -- libcloudsc_amd.so: the C ABI of include/cloudsc_amd.h on
// top of the hand-written CDNA4 kernels.
//
//   * parameters -> a device-memory block per parameter set (fp64 + fp32
//     mirrors, host-folded), passed to every launch by pointer and read with
//     scalar loads through the constant address space.  Each device has a
//     default set (cloudsc_gpu_init); every state and host pipeline owns its
//     own, so two states with different parameters never see each other's.
//     This replaces the TECLDP device struct passed by pointer + the 28
//     by-value scalars of src/cloudsc_cuda/cloudsc/cloudsc_driver.cu:312,383,411-416.
//   * cloudsc_gpu_run: one launch, NPROMA block -> workgroup, column -> lane
//     (KCACHE, SCC) or a persistent work queue of (level segment, 64-column
//     sub-block) items (KSEG).
//
// No CPU fallback: every GPU entry point fails with a CLOUDSC_E* code if HIP or
// the device is unavailable.  (cloudsc_cpu_run, cloudsc_cpu.cpp, is a separate,
// explicitly selected host variant, never substituted for a GPU run.)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "cloudsc_amd.h"
#include "cloudsc_dev.h"
#include "cloudsc_internal.h"
#include "cloudsc_kcache.h"
#include "cloudsc_params.h"
#include "cloudsc_scc.h"

using namespace cloudsc;
using namespace cloudsc_impl;

// ---------------------------------------------------------------------------
// error text (per calling thread)
// ---------------------------------------------------------------------------
namespace cloudsc_impl {
thread_local char g_hip_err[256] = "";
int hip_fail(hipError_t e, const char* what) {
  snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
  return CLOUDSC_EHIP;
}
void set_error_text(const char* text) { snprintf(g_hip_err, sizeof(g_hip_err), "%s", text); }
}  // namespace cloudsc_impl

// ---------------------------------------------------------------------------
// parameter sets
// ---------------------------------------------------------------------------
namespace {

// device layout of one parameter set: the fp64 mirror, then the fp32 one
constexpr size_t kSpOffset = (sizeof(DevParamsSpp<double>) + 255) & ~(size_t)255;
constexpr size_t kParamBlockBytes = kSpOffset + sizeof(DevParamsSpp<float>);

// the per-device default parameter sets (cloudsc_gpu_init)
std::mutex g_default_mu;
ParamSet g_default[kMaxDevices];

}  // namespace

namespace cloudsc_impl {

int check_params(const cloudsc_params_t* p) {
  if (!p) return CLOUDSC_EINVAL;
  if (p->ncldtop < 2) return CLOUDSC_EINVAL;        // the physics reads level jk-1 (za, ztp1)
  if (p->nssopt < 0 || p->nssopt > 3) return CLOUDSC_EINVAL;
  if (!(p->ptsphy > 0.0)) return CLOUDSC_EINVAL;
  return CLOUDSC_OK;
}

size_t param_block_bytes() { return kParamBlockBytes; }
void param_block_fill(char* blk, const cloudsc_params_t& p) {
  const DevParamsSpp<double> dp = fold_params<double>(p);
  const DevParamsSpp<float> sp = fold_params<float>(p);
  std::memcpy(blk, &dp, sizeof(dp));
  std::memcpy(blk + kSpOffset, &sp, sizeof(sp));
}

int param_set_upload(ParamSet* ps, int device, const cloudsc_params_t* p) {
  int rc = check_params(p);
  if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  if (!ps->dev) {
    hipError_t e = hipMalloc(&ps->dev, kParamBlockBytes);
    if (e != hipSuccess) { ps->dev = nullptr; hip_fail(e, "hipMalloc(params)"); return CLOUDSC_ENOMEM; }
  }
  std::vector<char> blk(kParamBlockBytes, 0);
  param_block_fill(blk.data(), *p);
  // hipMemcpy from pageable memory may return before the bytes have reached the
  // device, and the launches that read them run on non-blocking streams, which
  // do not wait for the null stream: a state created right after another one's
  // destruction read part of a stale parameter block in its first launch.
  // Copy on the null stream and wait for it.
#ifdef CLOUDSC_DEBUG_UNORDERED_PARAM_UPLOAD
  // diagnostic build only: the round-3 upload, unordered with the launches
  // (profiles/r04/contiguous_alloc_hazard.txt re-introduces it on purpose)
  HIPCHK(hipMemcpy(ps->dev, blk.data(), kParamBlockBytes, hipMemcpyHostToDevice));
#else
  HIPCHK(hipMemcpyAsync(ps->dev, blk.data(), kParamBlockBytes, hipMemcpyHostToDevice, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
#endif
  ps->device = device;
  ps->aer = p->laericesed || p->laericeauto;
  ps->ncldtop = p->ncldtop;
  ps->ptsphy = p->ptsphy;
  return CLOUDSC_OK;
}

int param_set_copy(ParamSet* dst, const ParamSet* src) {
  if (!src || !src->dev) return CLOUDSC_ENOINIT;
  HIPCHK(hipSetDevice(src->device));
  if (!dst->dev) {
    hipError_t e = hipMalloc(&dst->dev, kParamBlockBytes);
    if (e != hipSuccess) { dst->dev = nullptr; hip_fail(e, "hipMalloc(params)"); return CLOUDSC_ENOMEM; }
  }
  HIPCHK(hipMemcpyAsync(dst->dev, src->dev, kParamBlockBytes, hipMemcpyDeviceToDevice, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));   // D2D hipMemcpy does not wait either (param_set_upload)
  dst->device = src->device;
  dst->aer = src->aer;
  dst->ncldtop = src->ncldtop;
  dst->ptsphy = src->ptsphy;
  return CLOUDSC_OK;
}

void param_set_free(ParamSet* ps) {
  if (ps && ps->dev) {
    (void)hipSetDevice(ps->device);
    (void)hipFree(ps->dev);
    ps->dev = nullptr;
  }
}

const ParamSet* device_default_params(int device) {
  if (device < 0 || device >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lk(g_default_mu);
  return g_default[device].dev ? &g_default[device] : nullptr;
}

bool fields_complete(const cloudsc_fields_t* f, const StepForm& form) {
  const void* const* p = (const void* const*)f;
  for (int m = 0; m < kNumFields; m++)
    if (!p[m] && kFieldTable[m].dir != CLOUDSC_FD_AEROSOL && output_selected(m, form.outputs) &&
        !((form.cml || form.adv) && is_tendency_loc(m)))
      return false;
  return true;
}

int check_step_form(const StepForm& form, unsigned need, const cloudsc_fields_t* f) {
  const unsigned bits = form_bits(form);
  if (!outputs_known(form.outputs) || (bits & need) != need || !form_bits_consistent(bits)) return CLOUDSC_EINVAL;
  if (form.tend_planes && (form.tend_planes < CLOUDSC_TENDBUF_PLANES_MIN || form.tend_planes > CLOUDSC_TENDBUF_PLANES_MAX))
    return CLOUDSC_EINVAL;
  if (const cloudsc_tend_cml_t* cml = form.cml) {
    if (!f || !cml->t || !cml->q || !cml->a || !cml->cld) return CLOUDSC_EINVAL;
    const void* const mine[4] = {cml->t, cml->q, cml->a, cml->cld};
    const void* const theirs[8] = {f->tendency_tmp_t,   f->tendency_tmp_q, f->tendency_tmp_a, f->tendency_tmp_cld,
                                   f->tendency_loc_t,   f->tendency_loc_q, f->tendency_loc_a, f->tendency_loc_cld};
    for (const void* a : mine)
      for (const void* b : theirs)
        if (a == b) return CLOUDSC_EINVAL;
  }
  if (const cloudsc_spp_t* spp = form.spp) {
    const void* const mine[5] = {spp->ramid, spp->rcldiff, spp->rclcrit, spp->rlcritsnow, spp->rpecons};
    const void* const* theirs = (const void* const*)f;
    bool any = false;
    for (const void* a : mine) {
      if (!a) continue;
      any = true;
      for (int m = 0; f && m < kNumFields; m++)
        if (a == theirs[m]) return CLOUDSC_EINVAL;
    }
    if (!f || !any) return CLOUDSC_EINVAL;
  }
  if (form.adv && !advance_members_ok(f, form.adv)) return CLOUDSC_EINVAL;
  return CLOUDSC_OK;
}

}  // namespace cloudsc_impl

namespace {

// the launch's parameter block, as a constant-address-space pointer (scalar
// loads), typed with the kernel's choice of single-precision exp/pow forms
template <typename real, bool FAST, typename S>
__device__ __forceinline__ cptr<DevParamsT<real, FAST>> params_of(cptr<KArgs<real, S>> ka) {
  return (cptr<DevParamsT<real, FAST>>)((const KArgs<real, S>*)ka)->par;
}
template <typename F>
__device__ __forceinline__ cptr<typename F::params> params_of(cptr<typename F::fields> ka) {
  return (cptr<typename F::params>)((const typename F::fields*)ka)->par;
}

}  // namespace

// Kernel entry points.  The kernel-argument struct is the first explicit kernel
// argument, i.e. it sits at offset 0 of the kernarg segment; the bodies read it
// (and the parameter block it points at) through constant-address-space
// pointers.
//
// The k-caching kernels are two templates over the form descriptor F (KForm,
// cloudsc_kcache.h): kcache_entry<F>, one shot, and kseg_entry<F>, persistent
// and level-segmented.  F names the compute and storage types (float fields
// under double arithmetic are CLOUDSC_MIXED), the configuration and the form:
//   F::fast  fp32 exp/pow in their float-internal device forms (the
//            CLOUDSC_FP32 default); false: the reference CPU build's
//            algorithms (always for fp64);
//   F::tb    the tendency buffer form (cloudsc_gpu_run_tendbuf): the first
//            argument is a KArgsTB, tend_planes directly behind the KArgs;
//   F::prog  the prognostic-outputs form (CLOUDSC_OUTPUTS_PROGNOSTIC): the
//            plain KArgs, whose ten diagnostic flux members are never read;
//   F::surf  the surface-fluxes form (CLOUDSC_OUTPUTS_SURFACE): F::prog, and the
//            members pfplsl, pfplsn, pfhpsl, pfhpsn point at [nblocks][nproma]
//            surface fields, written once after the last level;
//   F::cml   the cumulative tendency form (cloudsc_gpu_run_tendbuf_cml): F::tb and
//            F::prog, the first argument a KArgsCML, the four BUFFER_CML plane starts
//            behind tend_planes; the tendency_loc_* members are never read;
//   F::spp   the per-column multiplier form (cloudsc_gpu_run_spp): alone or with
//            F::prog, the first argument a KArgsSPP, the five multiplier fields
//            behind the KArgs;
//   F::adv   the advancing form (cloudsc_gpu_run_advance): alone or with F::surf,
//            the first argument a KArgsADV, the four arrays of the updated
//            prognostics behind the KArgs; the tendency_loc_* members are never read;
//   F::pack  narrow blocks (NPROMA <= 32) packed into full waves: a workgroup
//            is one wave that walks PackArgs::pack consecutive blocks.
// A kernel has exactly the arguments its form needs: Pack is PackArgs for
// F::pack and empty otherwise, so an unpacked kernel's kernarg segment holds
// no PackArgs.
template <typename F, typename... Pack>
__global__ void __launch_bounds__(256, F::waves) kcache_entry(const typename F::kargs a, const Pack... g) {
  static_assert(sizeof...(Pack) == (F::pack ? 1 : 0), "PackArgs exactly when the form is packed");
  (void)a;
  libm_tables_to_lds<typename F::real>();
  const cptr<typename F::fields> ka = (cptr<typename F::fields>)__builtin_amdgcn_kernarg_segment_ptr();
  cloudsc_kcache_body<F>(ka, params_of<F>(ka), g...);
}
// The batched one-shot kernel (cloudsc_gpu_run_batch): kcache_entry over a device table of
// kernel-argument structs, one per member (field set), kBatchEntryStride<F> bytes apart.  The member index is
// blockIdx.y, the grid dimension the one-shot launch leaves free -- a workgroup id, so it arrives in a scalar
// register and is wave-uniform by construction -- and blockIdx.x is the block (F::pack: the group) within the
// member, exactly as in kcache_entry.  `ka` points at the member's entry instead of at the kernarg segment; the
// body reads it, and the parameter block its `par` points at, through the same constant-address-space pointer,
// with scalar loads, so each member runs under its own parameter set.  Packed: the wave of workgroup (g, m)
// walks blocks g * pack .. g * pack + pack - 1 of member m and pack_lane switches off the lanes whose block is
// past that member's nblocks, so a wave never runs into the next member.  Plain forms only: F::kargs is F::fields.
constexpr size_t kBatchEntryStride = (sizeof(KArgs<double>) + 63) & ~(size_t)63;   // whole scalar-cache lines
static_assert(sizeof(KArgs<float>) == sizeof(KArgs<double>) && sizeof(KArgs<double, float>) == sizeof(KArgs<double>),
              "one entry size for every precision: pointers and three ints");
template <typename F, typename... Pack>
__global__ void __launch_bounds__(256, F::waves) kcache_batch_entry(const char* table, const Pack... g) {
  static_assert(sizeof...(Pack) == (F::pack ? 1 : 0), "PackArgs exactly when the form is packed");
  static_assert(std::is_same<typename F::kargs, typename F::fields>::value, "the batch runs the plain forms");
  libm_tables_to_lds<typename F::real>();
  const cptr<typename F::fields> ka =
      (cptr<typename F::fields>)(const typename F::fields*)(table + (size_t)blockIdx.y * kBatchEntryStride);
  cloudsc_kcache_body<F>(ka, params_of<F>(ka), g...);
}
template <typename F, typename... Pack>
__global__ void __launch_bounds__(256, F::waves) kseg_entry(const typename F::kargs a,
                                                            const PersistArgs<typename F::real> pa, const Pack... g) {
  static_assert(sizeof...(Pack) == (F::pack ? 1 : 0), "PackArgs exactly when the form is packed");
  (void)a;
  libm_tables_to_lds<typename F::real>();
  const cptr<typename F::fields> ka = (cptr<typename F::fields>)__builtin_amdgcn_kernarg_segment_ptr();
  cloudsc_kcache_persistent_body<F>(ka, params_of<F>(ka), pa, g...);
}
template <typename real, bool AER, bool FAST = false>
__global__ void __launch_bounds__(256) scc_entry(const KArgs<real> a, const SccScratch<real> s) {
  (void)a;
  libm_tables_to_lds<real>();
  const cptr<KArgs<real>> ka = (cptr<KArgs<real>>)__builtin_amdgcn_kernarg_segment_ptr();
  cloudsc_scc_body<real, AER>(ka, s, params_of<real, FAST>(ka));
}
template <typename real, bool AER, bool FAST = false>
__global__ void __launch_bounds__(256) scc_private_entry(const KArgs<real> a) {
  (void)a;
  libm_tables_to_lds<real>();
  const cptr<KArgs<real>> ka = (cptr<KArgs<real>>)__builtin_amdgcn_kernarg_segment_ptr();
  cloudsc_scc_private_body<real, AER>(ka, params_of<real, FAST>(ka));
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
namespace {

// Kernel configuration: occupancy target (waves per SIMD, via __launch_bounds__)
// x load schedule (PF) x where the carried state lives (LDSC).  The product
// library instantiates only the measured defaults:
//   fp64: 2 waves/SIMD, carried state and neighbour planes in registers, the
//         next level's first-consumed inputs issued in the middle of the level
//         (cfg 23, PF 3; round 3: 0.8 % faster than cfg 20 on two boxes,
//         profiles/r03/sweep_pf3_fp64.jsonl; cfg 20 was 1.8 % faster than the
//         LDS-carry cfg 122, profiles/r01/sweep_kseg_cfgs_nt.jsonl);
//   fp32: 2 waves/SIMD with the register prefetch of level k+1 (cfg 21) -- 1.8-3.5 %
//         faster than round 1's 3-wave cfg 31 on the same box (profiles/r02/fp32_cfg_sweep.jsonl;
//         cfg 31 was 2-3 % faster than the 4-wave LDS-carry cfg 140, sweep_fp32_cfgs_libm.jsonl).
// The diagnostic build (-DCLOUDSC_DEBUG_KNOBS, `make variant`) instantiates the
// whole table and reads CLOUDSC_KCACHE_CFG / CLOUDSC_KSEG_* from the environment
// (tools/sweep.py); the product library never reads the environment.
template <typename real> struct DefaultCfg;
template <> struct DefaultCfg<double> { static constexpr int code = 23, waves = 2, pf = 3; };
#ifndef CLOUDSC_FP32_PF   // experiment builds: the fp32 load schedule (make variant VFLAGS=-DCLOUDSC_FP32_PF=3)
#define CLOUDSC_FP32_PF 1
#endif
template <> struct DefaultCfg<float> {
  static constexpr int code = 20 + CLOUDSC_FP32_PF, waves = 2, pf = CLOUDSC_FP32_PF;
};

#ifdef CLOUDSC_DEBUG_KNOBS
// code: [1]<waves><pf> -- leading 1 = carried state in LDS
#define CLOUDSC_FOR_EACH_CFG(X) \
  X(10, 1, 0, false) X(11, 1, 1, false) X(20, 2, 0, false) X(21, 2, 1, false) X(30, 3, 0, false) \
  X(31, 3, 1, false) X(40, 4, 0, false) X(41, 4, 1, false) X(120, 2, 0, true) X(121, 2, 1, true) X(23, 2, 3, false) X(24, 2, 4, false) X(33, 3, 3, false) \
  X(122, 2, 2, true) X(130, 3, 0, true) X(132, 3, 2, true) X(22, 2, 2, false) X(131, 3, 1, true) X(140, 4, 0, true) \
  X(123, 2, 3, true) X(133, 3, 3, true)
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
#endif

// One physics-kernel launch.  With `ev`, the dispatch packet itself records the
// start and stop timestamps (hipExtLaunchKernelGGL), so timing a step adds no
// event packets between consecutive kernels.
template <typename... Args>
void launch_physics(void (*kern)(Args...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const LaunchEvents* ev,
                    Args... args) {
  if (ev) hipExtLaunchKernelGGL(kern, grid, block, (std::uint32_t)lds, st, ev->start, ev->stop, 0u, args...);
  else hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
}

// the precision code of a (compute, storage) pair
template <typename real, typename S>
constexpr int kPrecisionOf = !std::is_same<real, S>::value ? CLOUDSC_MIXED : sizeof(real) == 8 ? CLOUDSC_FP64 : CLOUDSC_FP32;

// Whether this build instantiates the kernels of (variant kind, compute, storage, exact-libm, AER,
// form bits): those that exist.  Experiment builds (make variant VFLAGS=-DCLOUDSC_ONLY_KSEG=8 ...) keep only
// the plain KSEG kernels of one element size without aerosols -- for the per-phase ablation builds of
// tools/ablation.sh; every other combination returns CLOUDSC_EINVAL.
template <typename real, typename S, bool FAST>
constexpr bool kernel_kept(int kind, bool aer, unsigned form = 0u) {
#ifdef CLOUDSC_ONLY_KSEG
  if (kind != CLOUDSC_VARIANT_KSEG || aer || (form & (kFormTb | kFormProg | kFormSurf | kFormCml | kFormSpp | kFormAdv)) || sizeof(real) != CLOUDSC_ONLY_KSEG ||
      sizeof(S) != CLOUDSC_ONLY_KSEG)
    return false;
#endif
  (void)aer;
  return form_exists(kind, kPrecisionOf<real, S>, std::is_same<real, float>::value && !FAST, form);
}

// The descriptors of one launch, one per configuration (WAVES, PF, LDSC).  The product library
// instantiates `product` alone.  with_cfg calls f(F{}) for the descriptor F to launch: in a
// CLOUDSC_DEBUG_KNOBS build the configuration that CLOUDSC_KCACHE_CFG names, for the kernels the
// table applies to (TABLE: the plain unpacked KCACHE kernels and the plain KSEG kernels, packed or
// not); packed KCACHE and the tendency buffer and prognostic-outputs forms stay in the product
// configuration in every build.
template <typename real, typename S, bool AER, bool FAST, unsigned FORM>
struct LaunchForm {
  template <int WAVES, int PF, bool LDSC>
  using cfg = KForm<real, S, WAVES, PF, AER, LDSC, FAST, FORM>;
  using product = cfg<DefaultCfg<real>::waves, DefaultCfg<real>::pf, false>;
};
constexpr bool cfg_table_applies(int kind, unsigned form) {
  return !(form & (kFormTb | kFormProg | kFormSurf | kFormCml | kFormSpp | kFormAdv)) &&
         (kind == CLOUDSC_VARIANT_KSEG || !(form & kFormPack));
}
template <typename LF, bool TABLE, typename Fn>
int with_cfg(Fn&& f) {
#ifdef CLOUDSC_DEBUG_KNOBS
  if constexpr (TABLE) {
    switch (env_int("CLOUDSC_KCACHE_CFG", DefaultCfg<typename LF::product::real>::code)) {
#define X(code, w, pf, ldsc) \
  case code: return f(typename LF::template cfg<w, pf, ldsc>{});
      CLOUDSC_FOR_EACH_CFG(X)
#undef X
      default: return CLOUDSC_EINVAL;
    }
  }
#endif
  return f(typename LF::product{});
}

// the kernel arguments of a launch: a's, with tend_planes behind them in the tendency buffer form and the
// BUFFER_CML plane starts behind that in the cumulative tendency form, or the five multiplier fields behind them
// in the per-column multiplier form, or the four arrays of the updated prognostics in the advancing form
template <typename F>
typename F::kargs kernel_args(const typename F::fields& a, const StepForm& form) {
  if constexpr (F::adv) {
    using S = typename F::store;
    typename F::kargs t;
    static_cast<typename F::fields&>(t) = a;
    const cloudsc_advance_t* adv = form.adv;
    t.adv_t = (S*)adv->t; t.adv_q = (S*)adv->q; t.adv_a = (S*)adv->a; t.adv_clv = (S*)adv->clv;
    return t;
  } else if constexpr (F::spp) {
    using S = typename F::store;
    typename F::kargs t;
    static_cast<typename F::fields&>(t) = a;
    const cloudsc_spp_t* spp = form.spp;
    t.mult[SPP_RAMID] = (const S*)spp->ramid; t.mult[SPP_RCLDIFF] = (const S*)spp->rcldiff;
    t.mult[SPP_RCLCRIT] = (const S*)spp->rclcrit; t.mult[SPP_RLCRITSNOW] = (const S*)spp->rlcritsnow;
    t.mult[SPP_RPECONS] = (const S*)spp->rpecons;
    return t;
  } else if constexpr (F::tb) {
    typename F::kargs t;
    static_cast<typename F::fields&>(t) = a;
    t.tend_planes = form.tend_planes;
    if constexpr (F::cml) {
      using S = typename F::store;
      const cloudsc_tend_cml_t* cml = form.cml;
      t.cml_t = (S*)cml->t; t.cml_q = (S*)cml->q; t.cml_a = (S*)cml->a; t.cml_cld = (S*)cml->cld;
    }
    return t;
  } else {
    (void)form;
    return a;
  }
}

// The KCACHE launch: a workgroup of nproma threads per block, or (F::pack) one wave per group of pk.pack blocks
template <typename F>
int launch_kcache(hipStream_t st, const typename F::kargs& a, int nblocks, int nproma, const PackArgs& pk,
                  const LaunchEvents* ev) {
  const int wg = F::pack ? 64 : nproma;
  const size_t lds = F::ldsc ? carry_lds_bytes<typename F::real>(wg) : 0;
  if constexpr (F::pack) launch_physics(kcache_entry<F, PackArgs>, dim3(pk.ngroups), dim3(wg), lds, st, ev, a, pk);
  else launch_physics(kcache_entry<F>, dim3(nblocks), dim3(wg), lds, st, ev, a);
  return CLOUDSC_OK;
}

// ---- narrow blocks packed into full waves ----
// pack = 64 / nproma blocks per wave for nproma <= 32, on request
// (cloudsc_debug_set_narrow_pack) or by the measured default; 1 = unpacked.
// The packed kernels keep their lane offsets in 32 bits: the farthest one is
// below pack * 5 * (klev + 1) * nproma elements of 8 bytes.
std::atomic<int> g_narrow_pack{-1};
// The default of a width class (negative mode), by the rule of DESIGN.md 3.18:
// packed only where it measured faster than unpacked, by more than the spread
// of the repeats, in all three precisions (profiles/narrow_pack/kseg_pack_ab.jsonl).
// NPROMA 8 and 16 (pack 8 and 4) are 1.4-3.9 times faster packed; NPROMA 32
// (pack 2) gains 2.5 % in fp64 and 4.6 % in mixed but loses 41 % in fp32, so
// the widths above 16 (32 measured, 17-31 not measured) stay unpacked.
bool narrow_pack_default(int nproma) { return nproma <= 16; }
// Configurations whose packed kernel would not fit the register file without
// spilling stay unpacked (profiles/narrow_pack/kernel_resources.txt): none does.
bool narrow_pack_fits(int precision, int variant, bool aer) {
  (void)precision; (void)variant; (void)aer;
  return true;
}
int narrow_pack_factor(int precision, int variant, int nproma, int klev, bool aer) {
  if (variant != CLOUDSC_VARIANT_KCACHE && variant != CLOUDSC_VARIANT_KSEG) return 1;
  if (nproma > 32) return 1;
  const int mode = g_narrow_pack.load(std::memory_order_relaxed);
  if (mode == 0 || (mode < 0 && !narrow_pack_default(nproma))) return 1;
  if (!narrow_pack_fits(precision, variant, aer)) return 1;
  const int p = 64 / nproma;
  if ((unsigned long long)p * 5ull * (unsigned long long)(klev + 1) * (unsigned long long)nproma * 8ull >= (1ull << 32))
    return 1;
  return p;
}
// ---- persistent segmented variant ----
// Every item is one wave: a block of NPROMA > 64 columns is run as
// ceil(NPROMA/64) 64-column sub-blocks (the block layout is unchanged: sub-block
// h is columns h*64.. of each plane of the block), so every NPROMA runs with the
// one-wave schedule that measures fastest (profiles/r01/nproma_sweep_*).
int kseg_nsub(int nproma) { return (nproma + 63) / 64; }
int kseg_wg(int nproma) { return nproma < 64 ? nproma : 64; }
// workspace: [err, tag, clock sums..][stripe counters, one per 128 B][flags: nblocks*nsub][carry state]
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr size_t kKsegCtrOffset = 256;                                   // bytes
constexpr size_t kKsegFlagOffset = kKsegCtrOffset + kKsegStripes * kKsegCtrStride * sizeof(unsigned);
static_assert(kKsegFlagOffset == 1280, "KSEG control layout");
static_assert(sizeof(KsegEpoch::base) / sizeof(unsigned) == kKsegStripes, "one epoch base per stripe");
size_t kseg_ctl_bytes(int nblocks, int nproma) {
  return align256(kKsegFlagOffset + (size_t)nblocks * kseg_nsub(nproma) * sizeof(unsigned));
}
template <typename real>
size_t kseg_scratch_bytes(int nblocks, int nproma) {
  return kseg_ctl_bytes(nblocks, nproma) + (size_t)nblocks * kCarryN * nproma * sizeof(real);
}

// Segmentation, measured (profiles/r01/kseg_nseg_sweep*.jsonl,
// kseg_bounds_sweep_*.jsonl), for one-wave items (2048 slots): 2 segments, the
// second one smaller ("guided": the items dequeued last are short, so the tail
// is short; lower levels also cost more per level) -- the split at NCLDTOP +
// a share of the physics levels: 60 % in rounds 1-2 (1.768 ms against 1.788 at
// 62 %, profiles/r01/kseg_bounds_sweep_nt.jsonl); re-tuned in round 3 for the
// current kernels, interleaved on three boxes (profiles/r03/kseg_split_sweep.txt):
// fp32 50 % (-2.5 / -2.6 / -1.0 % against 60), fp64 55 % (-1.9 / -0.8 / +0.8 /
// -1.6 % on four boxes); 3 or 4 guided segments are 2.6-12 % slower.  Each hand-off
// costs 19 values out and in plus an L1 invalidate, so fewer segments win once
// the tail is short.
constexpr int kKsegNseg = 2;
#ifdef CLOUDSC_KSEG_SPLIT_PCT   // experiment builds override both (make variant VFLAGS=-DCLOUDSC_KSEG_SPLIT_PCT=..)
template <typename real> constexpr int kKsegSplitPct = CLOUDSC_KSEG_SPLIT_PCT;
#else
template <typename real> constexpr int kKsegSplitPct = sizeof(real) == 8 ? 55 : 50;
#endif

void kseg_bounds(int nseg, int klev, int ncldtop, int split_pct, int* lev) {
  const int top = ncldtop - 1 < klev ? (ncldtop - 1 > 0 ? ncldtop - 1 : 0) : klev;
  const int phys = klev - top;
  lev[0] = 0;
  if (nseg == 2) {
    lev[1] = top + (int)(((long long)split_pct * phys + 50) / 100);
    if (lev[1] <= 0) lev[1] = 1;
    if (lev[1] >= klev) lev[1] = klev - 1;
  } else {
    for (int sgm = 1; sgm < nseg; sgm++) lev[sgm] = top + (int)(((long long)phys * sgm + nseg / 2) / nseg);
  }
  lev[nseg] = klev;
}

// dequeue stripes of a grid (cloudsc_kcache.h): one per XCD, never more than workgroups
int kseg_nstripes(int grid) { return grid < kKsegStripes ? (grid > 0 ? grid : 1) : kKsegStripes; }

// consumer spin bound of a KSEG hand-off (cloudsc_debug_set_kseg_spin_limit)
std::atomic<unsigned> g_kseg_spin_limit{1u << 24};
// schedule overrides for the tests of the hand-off (cloudsc_debug_set_kseg_schedule); 0 = default
std::atomic<int> g_kseg_nseg{0}, g_kseg_grid{0};

}  // namespace

// KSEG workspace words: [1] timed-out hand-offs (sticky: accumulated over
// launches until cloudsc_gpu_check reads and clears it), [2] a tag marking [1]
// as initialised, [32..35] two 64-bit clock sums (PersistArgs::clk, accumulated
// like [1]), [64 + 32 s] the dequeue counter of stripe s, [320..] per-sub-block
// flags.  This
// kernel zeroes the counter and the flags before every launch of the low-level
// entry points, and before the first launch on a state's workspace (later
// launches of the state continue the counter and the flag stamps, KsegEpoch);
// the first launch on a workspace (tag absent) also zeroes the error word.
constexpr unsigned kKsegTag = 0xC105D5C1u;
constexpr size_t kKsegClkOffset = 128;   // bytes: words [32..35]
__global__ void __launch_bounds__(256) kseg_prepare_kernel(unsigned* ws, int nflags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && ws[2] != kKsegTag) { ws[1] = 0u; ws[2] = kKsegTag; ws[32] = ws[33] = ws[34] = ws[35] = 0u; }
  if (i < kKsegStripes) ws[kKsegCtrOffset / 4 + i * kKsegCtrStride] = 0u;
  for (int j = i; j < nflags; j += gridDim.x * blockDim.x) ws[kKsegFlagOffset / 4 + j] = 0u;
}

namespace {

constexpr int kSimdsPerCu = 4;                       // CDNA4 compute unit
// the KSEG grid for per_cu resident workgroups on each of ncu compute units
int kseg_grid_size(int per_cu, int ncu, int nitems, int nseg) {
  const int simds = kSimdsPerCu * ncu;
  const int units = nitems / (nseg > 0 ? nseg : 1);   // one-wave work units
  const int per_simd = per_cu / kSimdsPerCu > 0 ? per_cu / kSimdsPerCu : 1;
  int w = units / simds;
  if (w < 1) w = 1;
  if (w > per_simd) w = per_simd;
  int grid = per_cu < kSimdsPerCu ? per_cu * ncu : w * simds;
  if (const int g = g_kseg_grid.load(std::memory_order_relaxed)) grid = g;
#ifdef CLOUDSC_DEBUG_KNOBS
  grid = env_int("CLOUDSC_KSEG_GRID", 0) > 0 ? env_int("CLOUDSC_KSEG_GRID", 0) : grid;
#endif
  if (grid > nitems) grid = nitems;
  return grid;
}

// Resident workgroups per compute unit of kseg_entry<F>, by workgroup size (0: not asked yet): one
// table per kernel.  Threads driving different devices may race here, hence atomics.
template <typename F>
std::atomic<int> g_kseg_per_cu[65];

// The KSEG launch.  F::pack: one 64-lane workgroup per group of pk.pack blocks.
template <typename F>
int launch_kseg_cfg(hipStream_t st, const typename F::kargs& a, const PersistArgs<typename F::real>& pa, int nproma,
                    int nitems, int* grid_out, const LaunchEvents* ev, const PackArgs& pk) {
  using real = typename F::real;
  const int nseg = pa.nseg;
  const auto kern = [] {
    if constexpr (F::pack) return &kseg_entry<F, PackArgs>;
    else return &kseg_entry<F>;
  }();
  const int wg = F::pack ? 64 : kseg_wg(nproma);
  const size_t lds = F::ldsc ? carry_lds_bytes<real>(wg) : 0;
  // Waves per SIMD: as many as fit, but no more than whole rounds of the work
  // units (one column's 64-column sub-block) per SIMD: 2560 units on 1024 SIMDs
  // take 2 waves each; a third resident wave (fp32 fits 3) would only find a
  // next-segment item and spin until its predecessor finishes (fp32 KSEG 1.12 ms
  // at 2 waves/SIMD against 1.23 ms at 3, profiles/r02/kseg_grid_sweep.jsonl).
  // An over-estimate of residency only delays the extra workgroups: progress
  // never depends on it, items are dequeued in order.
  std::atomic<int>& cached = g_kseg_per_cu<F>[wg];
  int per_cu = cached.load(std::memory_order_relaxed);
  if (!per_cu) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, wg, lds);
    if (e != hipSuccess || n <= 0) n = 1;
    per_cu = n;
    cached.store(n, std::memory_order_relaxed);
  }
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0)
    ncu = 256;
  const int grid = kseg_grid_size(per_cu, ncu, nitems, nseg);
  PersistArgs<real> pg = pa;
  pg.nstripes = kseg_nstripes(grid);
  if constexpr (F::pack) launch_physics(kern, dim3(grid), dim3(wg), lds, st, ev, a, pg, pk);
  else launch_physics(kern, dim3(grid), dim3(wg), lds, st, ev, a, pg);
  *grid_out = grid;
  return CLOUDSC_OK;
}

// One launch, as gpu_run_impl asks for it: everything launch_v needs, by name
struct LaunchRequest {
  hipStream_t st;
  int kind;          // CLOUDSC_VARIANT_*, without option bits
  bool exact_libm;   // CLOUDSC_FP32_EXACT_LIBM
  const cloudsc_fields_t* f;
  int ngptot, nproma, klev;
  void* scratch;
  const void* plude_in;   // NULL: in place
  const ParamSet& ps;
  KsegEpoch* ep;
  const LaunchEvents* ev;
  StepForm form;
};

// The KSEG launch of a request: the schedule and the workspace's epoch, then with_form's kernel (launch_v)
template <typename real, typename ST, typename WithForm>
int launch_kseg(const LaunchRequest& rq, const KArgs<real, ST>& a, const PackArgs& pk, const WithForm& with_form) {
  const hipStream_t st = rq.st;
  void* const scratch = rq.scratch;
  KsegEpoch* const ep = rq.ep;
  const int nproma = rq.nproma, klev = rq.klev, nblocks = pk.nblocks, pack = pk.pack;
  if (!scratch) return CLOUDSC_EINVAL;
  PersistArgs<real> pa;
  pa.ctr = (unsigned*)((char*)scratch + kKsegCtrOffset);
  pa.err = (unsigned*)scratch + 1;
  pa.clk = (unsigned long long*)((char*)scratch + kKsegClkOffset);
  pa.flags = (unsigned*)((char*)scratch + kKsegFlagOffset);
  pa.state = (real*)((char*)scratch + kseg_ctl_bytes(nblocks, nproma));
  pa.nsub = pack > 1 ? 1 : kseg_nsub(nproma);
  // the schedule's units: blocks, or groups of `pack` blocks (one flag each:
  // the first pk.ngroups words of the flag area)
  const int nunits = pack > 1 ? pk.ngroups : nblocks;
  pa.spin_limit = g_kseg_spin_limit.load(std::memory_order_relaxed);
  // item order (segment, block, sub-block); (segment, sub-block, block) measured
  // the same within noise at NPROMA 128, 2 % slower at 256 (profiles/r01/kseg_subblock_order.jsonl)
  pa.sb_major = 0;
  pa.nseg = kKsegNseg;
  if (const int n = g_kseg_nseg.load(std::memory_order_relaxed)) pa.nseg = n > kMaxSeg ? kMaxSeg : n;
#ifdef CLOUDSC_DEBUG_KNOBS
  pa.sb_major = env_int("CLOUDSC_KSEG_SBMAJOR", 0) != 0;
  pa.nseg = env_int("CLOUDSC_KSEG_NSEG", kKsegNseg);
  pa.nseg = pa.nseg < 1 ? 1 : (pa.nseg > kMaxSeg ? kMaxSeg : pa.nseg);
#endif
  if (pa.nseg > klev) pa.nseg = klev;
  pa.nblocks = nblocks;
  for (int q = 0; q <= kMaxSeg; q++) pa.lev[q] = klev;
  kseg_bounds(pa.nseg, klev, rq.ps.ncldtop, kKsegSplitPct<real>, pa.lev);
#ifdef CLOUDSC_DEBUG_KNOBS
  if (const char* e = getenv("CLOUDSC_KSEG_BOUNDS")) {   // explicit interior boundaries
    int n = 1, v = 0;
    const char* q = e;
    while (*q && n < kMaxSeg) {
      v = (int)strtol(q, (char**)&q, 10);
      if (v <= pa.lev[n - 1] || v >= klev) break;
      pa.lev[n++] = v;
      if (*q == ',') q++;
    }
    pa.nseg = n;
    pa.lev[n] = klev;
  }
#endif
  pa.nitems = pa.nseg * nunits * pa.nsub;
  const bool zero_ws = !(ep && ep->ready);
  if (zero_ws) {
    const int nflags = nblocks * kseg_nsub(nproma);
    const int g = (nflags + 255) / 256 < 64 ? (nflags + 255) / 256 : 64;
    hipLaunchKernelGGL(kseg_prepare_kernel, dim3(g > 0 ? g : 1), dim3(256), 0, st, (unsigned*)scratch, nflags);
    if (ep) ep->ready = false;
  }
  for (int q = 0; q < kKsegStripes; q++) pa.base[q] = zero_ws ? 0u : ep->base[q];
  pa.stamp = zero_ws ? 0u : ep->stamp;
  int grid = 0;
  const int rc = with_form(std::integral_constant<int, CLOUDSC_VARIANT_KSEG>{}, [&](auto form) {
    using F = decltype(form);
    return launch_kseg_cfg<F>(st, kernel_args<F>(a, rq.form), pa, nproma, pa.nitems, &grid, rq.ev, pk);
  });
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  if (ep) {   // the next launch on this workspace continues where this one ends
    // stripe q took its items plus one past-the-end ticket per workgroup of it
    const int S = kseg_nstripes(grid);
    for (int q = 0; q < kKsegStripes; q++) {
      const unsigned nbs = q < S ? (unsigned)((nunits - q + S - 1) / S) : 0u;
      const unsigned wgs = q < S ? (unsigned)((grid - q + S - 1) / S) : 0u;
      ep->base[q] = pa.base[q] + (unsigned)pa.nseg * nbs * (unsigned)pa.nsub + wgs;
    }
    ep->stamp = pa.stamp + (unsigned)(kMaxSeg + 1);
    ep->ready = true;
  }
  return CLOUDSC_OK;
}

// real: the compute type; ST: the fields' element type (float under a double
// `real` is CLOUDSC_MIXED: the k-caching kernels only)
template <typename real, bool FAST, typename ST = real>
int launch_v(const LaunchRequest& rq) {
  const cloudsc_fields_t* f = rq.f;
  const int kind = rq.kind, nproma = rq.nproma, klev = rq.klev;
  const bool aer = rq.ps.aer;
  const unsigned bits = form_bits(rq.form);
  if (!kernel_kept<real, ST, FAST>(kind, aer, bits)) return CLOUDSC_EINVAL;
  KArgs<real, ST> a = make_kargs<real, ST>(
      f, rq.ngptot, nproma, klev, (const DevParams<real>*)((const char*)rq.ps.dev + (sizeof(real) == 8 ? 0 : kSpOffset)));
  if (rq.plude_in) a.plude_in = (const ST*)rq.plude_in;
  const int nblocks = rq.ngptot / nproma + (rq.ngptot % nproma ? 1 : 0);
  if (aer && (!f->pre_ice || !f->picrit_aer || !f->pnice)) return CLOUDSC_EINVAL;
  int rc = CLOUDSC_OK;
  // blocks per wave (1 = unpacked) and the packed launches' extra kernel argument
  int pack = narrow_pack_factor(kPrecisionOf<real, ST>, kind, nproma, klev, aer);
  // (a packed lane's offset in a tendency buffer: below pack * tend_planes * klev * nproma elements)
  if ((unsigned long long)pack * (unsigned)rq.form.tend_planes * (unsigned long long)klev * (unsigned)nproma * 8ull >=
      (1ull << 32))
    pack = 1;
  const PackArgs pk{pack, nblocks, (nblocks + pack - 1) / pack};
  // The k-caching launch of this call: go(F{}) with the descriptor F of its kernel -- the runtime
  // conditions become F's members here, and only kernels that exist are instantiated
  const auto with_form = [&](auto kind_c, auto&& go) {
    return dispatch_bools(
        [&](auto AER, auto PACK, auto TB, auto PROG, auto SURF, auto CML, auto SPP, auto ADV) {
          constexpr unsigned form = form_bits(TB, PROG, SURF, CML, SPP, ADV) | (PACK ? kFormPack : 0u);
          if constexpr (kernel_kept<real, ST, FAST>(kind_c, AER, form))
            return with_cfg<LaunchForm<real, ST, AER, FAST, form>, cfg_table_applies(kind_c, form)>(go);
          else
            return (int)CLOUDSC_EINVAL;
        },
        aer, pack > 1, (bits & kFormTb) != 0, (bits & kFormProg) != 0, (bits & kFormSurf) != 0, (bits & kFormCml) != 0,
        (bits & kFormSpp) != 0, (bits & kFormAdv) != 0);
  };
  if (kind == CLOUDSC_VARIANT_KCACHE) {
    rc = with_form(std::integral_constant<int, CLOUDSC_VARIANT_KCACHE>{}, [&](auto form) {
      using F = decltype(form);
      return launch_kcache<F>(rq.st, kernel_args<F>(a, rq.form), nblocks, nproma, pk, rq.ev);
    });
  } else if (kind == CLOUDSC_VARIANT_KSEG) {
    return launch_kseg(rq, a, pk, with_form);
  } else if (kind == CLOUDSC_VARIANT_SCC_PRIVATE) {
    if (klev > kPrivKlev) return CLOUDSC_EINVAL;    // the private arrays are sized at compile time
    rc = dispatch_bools(
        [&](auto AER) {
          if constexpr (kernel_kept<real, ST, FAST>(CLOUDSC_VARIANT_SCC_PRIVATE, AER))
            launch_physics(scc_private_entry<real, AER, FAST>, dim3(nblocks), dim3(nproma), 0, rq.st, rq.ev, a);
          return (int)CLOUDSC_OK;
        },
        aer);
  } else {
    if (!rq.scratch) return CLOUDSC_EINVAL;
    rc = dispatch_bools(
        [&](auto AER) {
          if constexpr (kernel_kept<real, ST, FAST>(CLOUDSC_VARIANT_SCC, AER))
            launch_physics(scc_entry<real, AER, FAST>, dim3(nblocks), dim3(nproma), 0, rq.st, rq.ev, a,
                           scc_scratch_carve<real>((char*)rq.scratch, nblocks, nproma, klev));
          return (int)CLOUDSC_OK;
        },
        aer);
  }
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

// The launch of a precision code: its (real, ST, FAST).  CLOUDSC_MIXED is the fp64 launch (exp/pow, parameter
// mirror, configuration, workspace) over float fields; fp32 runs the float-internal exp/pow unless the caller
// asks for the reference CPU build's forms (CLOUDSC_FP32_EXACT_LIBM), which are the only ones fp64 has
int launch(int precision, const LaunchRequest& rq) {
  switch (precision) {
    case CLOUDSC_FP64: return launch_v<double, false>(rq);
    case CLOUDSC_FP32: return dispatch_bools([&](auto FAST) { return launch_v<float, FAST>(rq); }, !rq.exact_libm);
    case CLOUDSC_MIXED: return launch_v<double, false, float>(rq);
    default: return CLOUDSC_EINVAL;
  }
}

// The batched KCACHE launch (kcache_batch_entry): the grid of launch_kcache in x, the members in y.  The packing
// decision is the one-shot launch's, taken here, at each run; the kernels are the product configuration's.
template <typename real, bool FAST, typename ST = real>
int launch_batch_v(hipStream_t st, const BatchLaunch& b) {
  const bool aer = b.aer;
  const unsigned bits = form_bits(false, outputs_prognostic(b.outputs), outputs_surface(b.outputs), false);
  if (!kernel_kept<real, ST, FAST>(CLOUDSC_VARIANT_KCACHE, aer, bits)) return CLOUDSC_EINVAL;
  const int nblocks = b.ngptot / b.nproma + (b.ngptot % b.nproma ? 1 : 0);
  const int pack = narrow_pack_factor(kPrecisionOf<real, ST>, CLOUDSC_VARIANT_KCACHE, b.nproma, b.klev, aer);
  const PackArgs pk{pack, nblocks, (nblocks + pack - 1) / pack};
  const int rc = dispatch_bools(
      [&](auto AER, auto PACK, auto PROG, auto SURF) {
        constexpr unsigned form = form_bits(false, PROG, SURF, false) | (PACK ? kFormPack : 0u);
        if constexpr (kernel_kept<real, ST, FAST>(CLOUDSC_VARIANT_KCACHE, AER, form)) {
          using F = typename LaunchForm<real, ST, AER, FAST, form>::product;
          static_assert(!F::ldsc, "the product configuration carries its state in registers");
          const char* table = (const char*)b.table;
          if constexpr (F::pack)
            hipLaunchKernelGGL((kcache_batch_entry<F, PackArgs>), dim3(pk.ngroups, b.nsets), dim3(64), 0, st, table, pk);
          else
            hipLaunchKernelGGL((kcache_batch_entry<F>), dim3(nblocks, b.nsets), dim3(b.nproma), 0, st, table);
          return (int)CLOUDSC_OK;
        } else {
          return (int)CLOUDSC_EINVAL;
        }
      },
      aer, pack > 1, (bits & kFormProg) != 0, (bits & kFormSurf) != 0);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

template <typename real, typename ST>
void batch_entry_fill(void* entry, const cloudsc_fields_t* f, int ngptot, int nproma, int klev, const void* block) {
  const KArgs<real, ST> a = make_kargs<real, ST>(
      f, ngptot, nproma, klev, (const DevParams<real>*)((const char*)block + (sizeof(real) == 8 ? 0 : kSpOffset)));
  static_assert(sizeof(a) <= kBatchEntryStride, "an entry holds the kernel arguments");
  std::memcpy(entry, &a, sizeof(a));
}

}  // namespace

namespace cloudsc_impl {
size_t batch_entry_stride() { return kBatchEntryStride; }
void batch_make_entry(int precision, void* entry, const cloudsc_fields_t* f, int ngptot, int nproma, int klev,
                      const void* param_block) {
  switch (precision) {
    case CLOUDSC_FP64: return batch_entry_fill<double, double>(entry, f, ngptot, nproma, klev, param_block);
    case CLOUDSC_FP32: return batch_entry_fill<float, float>(entry, f, ngptot, nproma, klev, param_block);
    default: return batch_entry_fill<double, float>(entry, f, ngptot, nproma, klev, param_block);
  }
}
int launch_kcache_batch(void* stream, const BatchLaunch& b) {
  switch (b.precision) {
    case CLOUDSC_FP64: return launch_batch_v<double, false>((hipStream_t)stream, b);
    case CLOUDSC_FP32: return launch_batch_v<float, true>((hipStream_t)stream, b);
    case CLOUDSC_MIXED: return launch_batch_v<double, false, float>((hipStream_t)stream, b);
    default: return CLOUDSC_EINVAL;
  }
}
}  // namespace cloudsc_impl

// ---------------------------------------------------------------------------
// C ABI: low level
// ---------------------------------------------------------------------------
extern "C" {

int cloudsc_gpu_device_count(int* count) {
  if (!count) return CLOUDSC_EINVAL;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
  *count = n;
  return CLOUDSC_OK;
}

int cloudsc_gpu_init(int device, const cloudsc_params_t* params) {
  int rc = check_params(params);
  if (rc) return rc;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || device >= kMaxDevices)
    return CLOUDSC_ENODEV;
  HIPCHK(hipSetDevice(device));
  // The default set is overwritten in place: wait for every launch on the
  // device that may still read it (states and pipelines have their own sets).
  HIPCHK(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(g_default_mu);
  return param_set_upload(&g_default[device], device, params);
}

long long cloudsc_gpu_scratch_bytes(int precision, int variant, int ngptot, int nproma, int klev) {
  if (ngptot <= 0 || nproma <= 0 || klev < 2) return -1;
  variant = variant_kind(variant);
  if (variant == CLOUDSC_VARIANT_KCACHE || variant == CLOUDSC_VARIANT_SCC_PRIVATE) return 0;
  if (!precision_storage_bytes(precision)) return -1;
  const int nblocks = ngptot / nproma + (ngptot % nproma ? 1 : 0);
  // workspaces hold values of the compute type (the KSEG carried state, the SCC temporaries)
  const bool dbl = precision_computes_double(precision);
  if (variant == CLOUDSC_VARIANT_KSEG)
    return dbl ? kseg_scratch_bytes<double>(nblocks, nproma) : kseg_scratch_bytes<float>(nblocks, nproma);
  if (variant != CLOUDSC_VARIANT_SCC || precision == CLOUDSC_MIXED) return -1;
  return dbl ? scc_scratch_bytes<double>(nblocks, nproma, klev) : scc_scratch_bytes<float>(nblocks, nproma, klev);
}

}  // extern "C"

namespace cloudsc_impl {
// the checks of validate_run_args that need no device
int validate_shape_args(int precision, int variant, int ngptot, int nproma, int klev) {
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (variant != CLOUDSC_VARIANT_KCACHE && variant != CLOUDSC_VARIANT_SCC && variant != CLOUDSC_VARIANT_KSEG &&
      variant != CLOUDSC_VARIANT_SCC_PRIVATE)
    return CLOUDSC_EINVAL;
  // mixed precision exists for the k-caching kernels only
  if (precision == CLOUDSC_MIXED && variant != CLOUDSC_VARIANT_KCACHE && variant != CLOUDSC_VARIANT_KSEG)
    return CLOUDSC_EINVAL;
  // KCACHE and SCC run one workgroup of nproma threads per block; KSEG runs
  // 64-column sub-blocks of any block width
  const int max_nproma = variant == CLOUDSC_VARIANT_KSEG ? (1 << 24) : 256;
  if (ngptot <= 0 || nproma <= 0 || nproma > max_nproma || klev < 2) return CLOUDSC_EINVAL;
  return CLOUDSC_OK;
}
int validate_run_args(int device, int precision, int variant, int ngptot, int nproma, int klev) {
  if (variant & ~(0xff | CLOUDSC_FP32_EXACT_LIBM)) return CLOUDSC_EINVAL;
  variant = variant_kind(variant);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CLOUDSC_ENODEV;
  if (device < 0 || device >= n || device >= kMaxDevices) return CLOUDSC_ENODEV;
  return validate_shape_args(precision, variant, ngptot, nproma, klev);
}

int gpu_run_impl(int device, void* stream, const StepShape& sh, const cloudsc_fields_t* f, void* scratch,
                 const StepForm& form, const RunContext& ctx) {
  // unknown option bits are an argument error here, before they are stripped (validate_run_args below sees
  // the variant's kind only): such a call must never launch
  if (sh.variant & ~(0xff | CLOUDSC_FP32_EXACT_LIBM)) return CLOUDSC_EINVAL;
  const int kind = variant_kind(sh.variant);
  int rc = validate_run_args(device, sh.precision, kind, sh.ngptot, sh.nproma, sh.klev);
  if (rc) return rc;
  const ParamSet* ps = ctx.ps ? ctx.ps : device_default_params(device);
  if (!ps || !ps->dev) return CLOUDSC_ENOINIT;
  if (ps->device != device) return CLOUDSC_EINVAL;
  if (!f || !fields_complete(f, form)) return CLOUDSC_EINVAL;
  HIPCHK(hipSetDevice(device));
  return launch(sh.precision, LaunchRequest{(hipStream_t)stream, kind, (sh.variant & CLOUDSC_FP32_EXACT_LIBM) != 0, f,
                                            sh.ngptot, sh.nproma, sh.klev, scratch, ctx.plude_in, *ps, ctx.ep, ctx.lev,
                                            form});
}

// A form entry: every argument rule first -- the form's own (check_step_form, with the bits `need` of the entry), no
// option bits (so no fp32 exact-libm), the shape, the support matrix, the fields the form touches, KSEG's workspace --
// so that an argument error is CLOUDSC_EINVAL before any HIP call; then the run, the device's checks first
static int gpu_run_form(int device, void* stream, const StepShape& sh, const cloudsc_fields_t* f, void* scratch,
                        const StepForm& form, unsigned need) {
  int rc = check_step_form(form, need, f);
  if (rc) return rc;
  if (sh.variant & ~0xff) return CLOUDSC_EINVAL;
  if ((rc = validate_shape_args(sh.precision, sh.variant, sh.ngptot, sh.nproma, sh.klev))) return rc;
  if (!form_exists(sh.variant, sh.precision, /*exact_libm=*/false, form_bits(form))) return CLOUDSC_EINVAL;   // no SCC form
  if (!f || !fields_complete(f, form) || (sh.variant == CLOUDSC_VARIANT_KSEG && !scratch)) return CLOUDSC_EINVAL;
  return gpu_run_impl(device, stream, sh, f, scratch, form, {});
}

int kseg_clock(int device, void* stream, void* scratch, bool reset, double* ghz, double* seconds) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long w[2] = {0, 0};
  HIPCHK(hipMemcpy(w, (char*)scratch + kKsegClkOffset, sizeof(w), hipMemcpyDeviceToHost));
  int khz = 0;
  HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device));
  if (ghz) *ghz = w[1] && khz > 0 ? (double)w[0] / (double)w[1] * (double)khz * 1e-6 : 0.0;
  if (seconds) *seconds = khz > 0 ? (double)w[1] / ((double)khz * 1e3) : 0.0;
  if (reset) {
    HIPCHK(hipMemsetAsync((char*)scratch + kKsegClkOffset, 0, sizeof(w), (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  }
  return CLOUDSC_OK;
}

int kseg_check(int device, void* stream, void* scratch) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned w[3] = {0, 0, 0};
  HIPCHK(hipMemcpy(w, scratch, sizeof(w), hipMemcpyDeviceToHost));
  const unsigned err = w[2] == kKsegTag ? w[1] : 0u;   // no tag: no KSEG launch on this workspace yet
  if (err) {
    // on the launches' stream, and waited for: the next launch must not race it
    HIPCHK(hipMemsetAsync((unsigned*)scratch + 1, 0, sizeof(unsigned), (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    char msg[96];
    std::snprintf(msg, sizeof(msg), "KSEG: %u segment hand-offs timed out", err);
    set_error_text(msg);
    return CLOUDSC_EHANDOFF;
  }
  return CLOUDSC_OK;
}
}  // namespace cloudsc_impl

extern "C" {

int cloudsc_gpu_run(int device, void* stream, int precision, int variant, int ngptot, int nproma,
                    int klev, const cloudsc_fields_t* f, void* scratch) {
  return gpu_run_impl(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch, {}, {});
}

int cloudsc_tendbuf_bind(cloudsc_fields_t* f, int precision, int nproma, int klev, const void* buffer_tmp,
                         void* buffer_loc) {
  const size_t eb = precision_storage_bytes(precision);
  if (!f || !eb || nproma < 1 || klev < 1 || !buffer_tmp || !buffer_loc) return CLOUDSC_EINVAL;
  const size_t plane = (size_t)klev * (size_t)nproma * eb;
  const char* tmp = (const char*)buffer_tmp;
  char* loc = (char*)buffer_loc;
  f->tendency_tmp_t = tmp + CLOUDSC_TENDBUF_T * plane;
  f->tendency_tmp_a = tmp + CLOUDSC_TENDBUF_A * plane;
  f->tendency_tmp_q = tmp + CLOUDSC_TENDBUF_Q * plane;
  f->tendency_tmp_cld = tmp + CLOUDSC_TENDBUF_CLD * plane;
  f->tendency_loc_t = loc + CLOUDSC_TENDBUF_T * plane;
  f->tendency_loc_a = loc + CLOUDSC_TENDBUF_A * plane;
  f->tendency_loc_q = loc + CLOUDSC_TENDBUF_Q * plane;
  f->tendency_loc_cld = loc + CLOUDSC_TENDBUF_CLD * plane;
  return CLOUDSC_OK;
}

int cloudsc_gpu_run_tendbuf(int device, void* stream, int precision, int variant, int ngptot, int nproma, int klev,
                            int tend_planes, const cloudsc_fields_t* f, void* scratch) {
  return gpu_run_form(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch, {tend_planes}, kFormTb);
}

int cloudsc_gpu_run_outputs(int device, void* stream, int precision, int variant, int outputs, int ngptot, int nproma,
                            int klev, const cloudsc_fields_t* f, void* scratch) {
  if (outputs == CLOUDSC_OUTPUTS_ALL)   // cloudsc_gpu_run itself: the device's checks first
    return cloudsc_gpu_run(device, stream, precision, variant, ngptot, nproma, klev, f, scratch);
  return gpu_run_form(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch, {0, outputs}, kFormProg);
}

// (with CLOUDSC_OUTPUTS_ALL the form, and so every rule, is cloudsc_gpu_run_tendbuf's)
int cloudsc_gpu_run_tendbuf_outputs(int device, void* stream, int precision, int variant, int outputs, int ngptot,
                                    int nproma, int klev, int tend_planes, const cloudsc_fields_t* f, void* scratch) {
  return gpu_run_form(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch, {tend_planes, outputs},
                      kFormTb);
}

int cloudsc_tendbuf_bind_cml(cloudsc_tend_cml_t* cml, int precision, int nproma, int klev, void* buffer_cml) {
  const size_t eb = precision_storage_bytes(precision);
  if (!cml || !eb || nproma < 1 || klev < 1 || !buffer_cml) return CLOUDSC_EINVAL;
  const size_t plane = (size_t)klev * (size_t)nproma * eb;
  char* b = (char*)buffer_cml;
  cml->t = b + CLOUDSC_TENDBUF_T * plane;
  cml->a = b + CLOUDSC_TENDBUF_A * plane;
  cml->q = b + CLOUDSC_TENDBUF_Q * plane;
  cml->cld = b + CLOUDSC_TENDBUF_CLD * plane;
  return CLOUDSC_OK;
}

// (kFormProg: CLOUDSC_OUTPUTS_ALL is refused)
int cloudsc_gpu_run_tendbuf_cml(int device, void* stream, int precision, int variant, int outputs, int ngptot,
                                int nproma, int klev, int tend_planes, const cloudsc_fields_t* f,
                                const cloudsc_tend_cml_t* cml, void* scratch) {
  return gpu_run_form(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch,
                      {tend_planes, outputs, cml}, kFormCml | kFormTb | kFormProg);
}

// (every rule before the first HIP call, CLOUDSC_OUTPUTS_ALL included: the form has no cloudsc_gpu_run behind it)
int cloudsc_gpu_run_spp(int device, void* stream, int precision, int variant, int outputs, int ngptot, int nproma,
                        int klev, const cloudsc_fields_t* f, const cloudsc_spp_t* spp, void* scratch) {
  return gpu_run_form(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch, {0, outputs, nullptr, spp},
                      kFormSpp);
}

// (every rule before the first HIP call; CLOUDSC_OUTPUTS_PROGNOSTIC alone is no form: form_bits_consistent)
int cloudsc_gpu_run_advance(int device, void* stream, int precision, int variant, int outputs, int ngptot, int nproma,
                            int klev, const cloudsc_fields_t* f, const cloudsc_advance_t* adv, void* scratch) {
  StepForm form;
  form.outputs = outputs;
  form.adv = adv;
  return gpu_run_form(device, stream, {precision, variant, ngptot, nproma, klev}, f, scratch, form, kFormAdv);
}

int cloudsc_gpu_check(int device, void* stream, int variant, void* scratch) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return CLOUDSC_ENODEV;
  if (variant_kind(variant) != CLOUDSC_VARIANT_KSEG) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return CLOUDSC_OK;
  }
  if (!scratch) return CLOUDSC_EINVAL;
  return kseg_check(device, stream, scratch);
}

int cloudsc_debug_set_kseg_schedule(int nseg, int grid) {
  if (nseg < 0 || grid < 0) return CLOUDSC_EINVAL;
  g_kseg_nseg.store(nseg, std::memory_order_relaxed);
  g_kseg_grid.store(grid, std::memory_order_relaxed);
  return CLOUDSC_OK;
}

int cloudsc_debug_set_narrow_pack(int mode) {
  g_narrow_pack.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed);
  return CLOUDSC_OK;
}

int cloudsc_gpu_launch_geometry(int precision, int variant, int ngptot, int nproma, int klev, int laer,
                                cloudsc_launch_geometry_t* out) {
  if (!out) return CLOUDSC_EINVAL;
  if (variant & ~(0xff | CLOUDSC_FP32_EXACT_LIBM)) return CLOUDSC_EINVAL;
  variant = variant_kind(variant);
  const int rc = validate_shape_args(precision, variant, ngptot, nproma, klev);
  if (rc) return rc;
  const int nblocks = ngptot / nproma + (ngptot % nproma ? 1 : 0);
  const int pack = narrow_pack_factor(precision, variant, nproma, klev, laer != 0);
  const int nsub = kseg_nsub(nproma);
  out->pack = pack;
  out->lanes = pack * (nproma < 64 ? nproma : 64);
  out->units = (nblocks + pack - 1) / pack * nsub;
  if (variant == CLOUDSC_VARIANT_KSEG) {
    int nseg = kKsegNseg;
    if (const int n = g_kseg_nseg.load(std::memory_order_relaxed)) nseg = n > kMaxSeg ? kMaxSeg : n;
    if (nseg > klev) nseg = klev;
    // an MI355X: 256 compute units, 2 resident waves per SIMD (one-wave workgroups)
    out->workgroups = kseg_grid_size(2 * kSimdsPerCu, 256, nseg * out->units, nseg);
    out->wg_threads = pack > 1 ? 64 : kseg_wg(nproma);
  } else {
    out->workgroups = pack > 1 ? out->units : nblocks;
    out->wg_threads = pack > 1 ? 64 : nproma;
  }
  return CLOUDSC_OK;
}

int cloudsc_debug_set_kseg_spin_limit(long long limit) {
  if (limit < 0) limit = 1LL << 24;
  g_kseg_spin_limit.store(limit > 0xffffffffLL ? 0xffffffffu : (unsigned)limit, std::memory_order_relaxed);
  return CLOUDSC_OK;
}

const char* cloudsc_strerror(int code) {
  switch (code) {
    case CLOUDSC_OK: return "success";
    case CLOUDSC_EINVAL: return "invalid argument";
    case CLOUDSC_ENODEV: return "no such HIP device";
    case CLOUDSC_EHIP: return "HIP runtime error";
    case CLOUDSC_ENOINIT: return "cloudsc_gpu_init not called for this device";
    case CLOUDSC_ENOMEM: return "out of memory";
    case CLOUDSC_EIO: return "I/O error";
    case CLOUDSC_EHANDOFF: return "KSEG segment hand-off timed out (outputs invalid)";
    default: return "unknown error";
  }
}

const char* cloudsc_last_hip_error(void) { return g_hip_err; }

#ifdef CLOUDSC_KSEG_TRACE
// diagnostic build only (tools/kseg_trace.py): per item {start, end, workgroup, xcc<<16|hw_id}
int cloudsc_kseg_trace(unsigned long long* host, int nitems) {
  if (nitems > kTraceMax) nitems = kTraceMax;
  HIPCHK(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_kseg_trace), sizeof(unsigned long long) * 4 * nitems));
  return CLOUDSC_OK;
}
#endif

// Diagnostic: the single-precision exp/pow forms of the kernels on the device,
// element-wise (tests/test_gpu_parity.py measures their ulp distance).
__global__ void __launch_bounds__(256) fp32_libm_kernel(int which, const float* x, const float* y, float* out,
                                                        long long n) {
  libm_tables_to_lds<float>();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r;
  switch (which) {
    case 0: r = cl_expf_fast(x[i]); break;
    case 1: r = cl_powf_fast(x[i], y[i]); break;
    case 2: r = cl_exp_impl(x[i]); break;
    case 3: r = cl_powr(x[i], y[i]); break;
    case 4: r = cl_divf_fast(x[i], y[i]); break;     // the fast kernels' x / y
    default: r = cl_div(x[i], y[i]); break;          // the exact kernels' x / y
  }
  out[i] = r;
}

int cloudsc_debug_fp32_libm(int device, int which, const float* x, const float* y, float* out, long long n) {
  if (which < 0 || which > 5 || !x || !out || n <= 0 || ((which & 1 || which >= 4) && !y)) return CLOUDSC_EINVAL;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return CLOUDSC_ENODEV;
  HIPCHK(hipSetDevice(device));
  float *dx = nullptr, *dy = nullptr, *dout = nullptr;
  const size_t bytes = (size_t)n * sizeof(float);
  hipError_t e = hipMalloc(&dx, bytes);
  if (e == hipSuccess) e = hipMalloc(&dy, bytes);
  if (e == hipSuccess) e = hipMalloc(&dout, bytes);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dy, y ? y : x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fp32_libm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, which, dx, dy,
                       dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dout);
  if (e != hipSuccess) return hip_fail(e, "fp32 libm diagnostic");
  return CLOUDSC_OK;
}

// Diagnostic: the double-precision device primitives of the kernels, element-wise
// (tests/test_device_math_gpu.py compares them bit for bit with the host C
// library's exp/pow and IEEE division / sqrt).  Every case calls the kernels'
// own function.  Every thread copies the tables before the bounds check (the
// copy ends in a barrier), with the stride of the launch's block size.
__global__ void __launch_bounds__(256) fp64_libm_kernel(int which, const double* x, const double* y, double* out,
                                                        long long n) {
  libm_tables_to_lds<double>();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = x[i], b = y[i];
  double r;
  switch (which) {
    case 0: r = cl_exp_impl(a); break;
    case 1: r = cl_powr(a, b); break;
    case 2:
    case 3: {
      double r0, r1;
      cloudsc_libm::exp_pair_split(a, b, &r0, &r1, LdsLibmTabs{}, DevLibmCold{});
      r = which == 2 ? r0 : r1;
      break;
    }
    case 4: r = cl_div(a, b); break;
    case 5: r = cl_div(a, cl_recip(b)); break;
    case 6: r = cl_div(a, Recip<double>{b, 1.0 / b}); break;   // cl_div_known / cl_div_lit: r = RN(1/d)
    case 7: r = cl_sqrt_p<double>(DevParamsT<double, false>{}, a); break;
    case 8: r = cl_exp_cold(a); break;
    default: r = cl_pow_cold(a, b); break;
  }
  out[i] = r;
}

int cloudsc_debug_fp64_libm(int device, int which, int block_threads, const double* x, const double* y, double* out,
                            long long n) {
  const bool reads_y = which != 0 && which != 7 && which != 8;
  if (which < 0 || which > 9 || !x || !out || n <= 0 || (reads_y && !y)) return CLOUDSC_EINVAL;
  if (block_threads != 64 && block_threads != 128 && block_threads != 256) return CLOUDSC_EINVAL;
  if ((n + block_threads - 1) / block_threads > 0x7fffffffLL) return CLOUDSC_EINVAL;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return CLOUDSC_ENODEV;
  HIPCHK(hipSetDevice(device));
  double *dx = nullptr, *dy = nullptr, *dout = nullptr;
  const size_t bytes = (size_t)n * sizeof(double);
  hipError_t e = hipMalloc(&dx, bytes);
  if (e == hipSuccess) e = hipMalloc(&dy, bytes);
  if (e == hipSuccess) e = hipMalloc(&dout, bytes);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dy, reads_y ? y : x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fp64_libm_kernel, dim3((unsigned)((n + block_threads - 1) / block_threads)),
                       dim3(block_threads), 0, nullptr, which, dx, dy, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dout);
  if (e != hipSuccess) return hip_fail(e, "fp64 libm diagnostic");
  return CLOUDSC_OK;
}

long long cloudsc_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(cloudsc_params_t);
    case 1: return sizeof(cloudsc_fields_t);
    case 2: return sizeof(cloudsc_template_t);
    case 3: return sizeof(cloudsc_reference_t);
    case 4: return sizeof(cloudsc_stats_t);
    default: return -1;
  }
}

}  // extern "C"
