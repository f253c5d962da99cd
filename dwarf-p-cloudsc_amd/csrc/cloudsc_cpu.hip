// cloudsc_cpu.hip -- cloudsc_cpu_run: the CPU variant of the dwarf (BASELINE.json
// config 1, `dwarf-cloudsc-c 1 16384 32`), explicitly selected by the caller.
// It is never substituted for a GPU run: the GPU entry points have no fallback.
//
// Reference: the C dwarf's OpenMP block loop (src/cloudsc_c/cloudsc/cloudsc_driver.c:
// 183-217, schedule(runtime)) calling the kernel cloudsc_c() (cloudsc_c.c:19-2587)
// on one NPROMA block at a time.  Here the per-level phase functions are the
// ones the GPU kernels are built from (cloudsc_kcache.h: init_level,
// physics_level, flux_level, ... compiled for the host), run level-outer and
// column-inner over a block -- the same order of operations per column, so the
// output is the reference kernel's bit for bit (tests/test_cpu.py pins it
// against oracle/_ref, the reference kernel compiled from its sources).
// Host threads take blocks from a shared counter (dynamic schedule).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "cloudsc_amd.h"
#include "cloudsc_internal.h"
#include "cloudsc_kcache.h"
#include "cloudsc_params.h"

using namespace cloudsc;

namespace {

// The state of one column that crosses levels, as in kcache_levels
// (cloudsc_kcache.h), without the GPU's software pipelining of the loads.
template <typename real>
struct HostColumn {
  CarryState<real> cs;
  Neighbors<real> nb;
  ColConst<real> cc;
};

// real: the compute type, S: the fields' element type (float under double = CLOUDSC_MIXED);
// TB: the tendency members are planes of packed buffers and A is a KArgsTB (cloudsc_kcache.h);
// PROG: the prognostic-outputs form, the ten diagnostic flux members of A never touched (flux_level);
// SURF: the surface-fluxes form, the other four flux members surface fields written after the last level;
// CML: the cumulative tendency form, A a KArgsCML and the local tendencies added to its planes (load_cml, store_level_cml);
// SPP: the per-column multiplier form, A a KArgsSPP (SppCol: the multipliers read from the host fields where they are used);
// ADV: the advancing form, A a KArgsADV and the updated prognostics stored to its arrays (store_level_adv)
template <typename real, bool AER, bool TB, bool PROG, bool SURF, bool CML, bool SPP, bool ADV, typename S>
void run_block(const DevParamsSpp<real>& c, const KArgs<real, S>& A, int b, std::vector<HostColumn<real>>& col) {
  const int nproma = A.nproma, klev = A.klev;
  const int bsize = std::min(nproma, A.ngptot - b * nproma);
  const size_t u1 = (size_t)b * nproma;
  const size_t u2 = (size_t)b * klev * nproma;
  const size_t uh = (size_t)b * (klev + 1) * nproma;
  const size_t u3 = (size_t)b * 5 * klev * nproma;
  const int ncldtop0 = c.ncldtop - 1;
  const int l1 = 1 < klev ? 1 : klev - 1;
  using Spp = typename std::conditional<SPP, SppCol<real, S, const KArgs<real, S>*, unsigned>, NoSpp>::type;
  const auto spp_of = [&](unsigned lo) {   // the column's own parameters (nothing of them is kept: formed where asked for)
    Spp spp;
    if constexpr (SPP) { spp.ka = &A; spp.u1 = u1; spp.lane = lo; }
    return spp;
  };
  for (int jl = 0; jl < bsize; jl++) {
    const unsigned lo = (unsigned)jl * (unsigned)sizeof(S);
    HostColumn<real>& h = col[jl];
    init_carry<real, PROG>(h.cs);
    flux_top<PROG, SURF>(c, A, uh, lo);
    h.cc = column_constants(c, A, u1, uh, lo);
    if constexpr (SPP) h.cc.kk_lcrit = h.cc.kk_lcrit * spp_of(lo).mult(SPP_RCLCRIT);
    h.nb.paph_k = ldg(A.paph, uh, lo);
    h.nb.paph_n = ldg(A.paph, uh + (size_t)nproma, lo);
    h.nb.pmfu_k = ldg(A.pmfu, u2, lo);
    h.nb.pmfd_k = ldg(A.pmfd, u2, lo);
    h.nb.pmfu_n = ldg(A.pmfu, u2 + (size_t)l1 * nproma, lo);
    h.nb.pmfd_n = ldg(A.pmfd, u2 + (size_t)l1 * nproma, lo);
    h.nb.plu_n = ldg(A.plu, u2 + (size_t)l1 * nproma, lo);
  }
  for (int k = 0; k < klev; k++) {
    const bool physics = k >= ncldtop0;
    const int k2 = k + 2 < klev ? k + 2 : klev - 1;
    const int kh2 = k + 2 < klev + 1 ? k + 2 : klev;
    for (int jl = 0; jl < bsize; jl++) {
      const unsigned lo = (unsigned)jl * (unsigned)sizeof(S);
      HostColumn<real>& h = col[jl];
      LevelIn<real> cur;
      load_level<real, AER, TB>(cur, A, u2, u3, k, klev, nproma, lo);
      LevelState<real> ls;
      PhysOut<real> po;
      init_level(c, cur, ls);
      for (int m = 0; m < 4; m++) { po.zqxn[m] = R(0.0); po.ctend[m] = R(0.0); }
      po.plude_k = cur.plude;
      po.atend = R(0.0);
      po.zcovptot_out = R(0.0);
      if constexpr (SPP) {
        if (physics) physics_level_spp(c, k, klev, ncldtop0, cur, h.nb, h.cc, ls, h.cs, po, NoMidHook{}, spp_of(lo));
      } else {
        if (physics) physics_level(c, k, klev, ncldtop0, cur, h.nb, h.cc, ls, h.cs, po);
      }
      if constexpr (CML) {
        CmlIn<real> cm;
        load_cml(cm, A, u2, k, klev, nproma, lo);
        store_level_cml(A, u2, k, klev, nproma, lo, ls, po, cm);
      } else if constexpr (ADV) {
        store_level_adv(c, A, u2, u3, k, klev, nproma, lo, ls, po);
      } else {
        store_level<TB>(A, u2, u3, k, klev, nproma, lo, physics, ls, po);
      }
      flux_level<PROG, SURF>(c, A, uh + (size_t)(k + 1) * nproma, lo, cur, ls, po, h.nb.paph_k, h.nb.paph_n, h.cs);
      h.cs.t_prev = ls.ztp1;
      h.cs.a_prev = ls.za;
      h.cs.pap_prev = cur.pap;
      h.nb.paph_k = h.nb.paph_n;
      h.nb.paph_n = ldg(A.paph, uh + (size_t)kh2 * nproma, lo);
      h.nb.pmfu_k = h.nb.pmfu_n;
      h.nb.pmfd_k = h.nb.pmfd_n;
      h.nb.pmfu_n = ldg(A.pmfu, u2 + (size_t)k2 * nproma, lo);
      h.nb.pmfd_n = ldg(A.pmfd, u2 + (size_t)k2 * nproma, lo);
      h.nb.plu_n = ldg(A.plu, u2 + (size_t)k2 * nproma, lo);
    }
  }
  for (int jl = 0; jl < bsize; jl++) stg(A.prainfrac, u1, (unsigned)jl * (unsigned)sizeof(S), col[jl].cs.rainfrac);
  if constexpr (SURF)
    for (int jl = 0; jl < bsize; jl++) flux_surface(c, A, u1, (unsigned)jl * (unsigned)sizeof(S), col[jl].cs);
}

// The host threads of a run (<= 0: one per hardware thread), and where its wall time and the per-thread records go
// (each may be NULL; nthreads entries): a thread's own wall time, the NPROMA blocks it took, the columns it computed
struct CpuThreads {
  int nthreads;
  double* seconds = nullptr;
  double* thread_seconds = nullptr;
  int* thread_blocks = nullptr;
  int* thread_columns = nullptr;
};

// the block loop over fields of element type S, computed in double
template <typename S>
int cpu_run(int ngptot, int nproma, int klev, const cloudsc_params_t* params, const cloudsc_fields_t* f,
            const cloudsc_impl::StepForm& form, const CpuThreads& th) {
  using namespace cloudsc_impl;
  int nthreads = th.nthreads;
  int rc = check_params(params);
  if (rc) return rc;
  if (!f || !fields_complete(f, form) || ngptot <= 0 || nproma <= 0 || klev < 2) return CLOUDSC_EINVAL;
  const bool aer = params->laericesed || params->laericeauto;
  if (aer && (!f->pre_ice || !f->picrit_aer || !f->pnice)) return CLOUDSC_EINVAL;
  if (nthreads <= 0 && (th.thread_seconds || th.thread_blocks || th.thread_columns)) return CLOUDSC_EINVAL;
  const DevParamsSpp<double> c = fold_params<double>(*params);
  KArgsCML<double, S> A;
  static_cast<KArgs<double, S>&>(A) = make_kargs<double, S>(f, ngptot, nproma, klev, nullptr);
  A.tend_planes = form.tend_planes;   // 0: separate arrays
  A.cml_t = A.cml_q = A.cml_a = A.cml_cld = nullptr;
  if (const cloudsc_tend_cml_t* cml = form.cml) {
    A.cml_t = (S*)cml->t; A.cml_q = (S*)cml->q; A.cml_a = (S*)cml->a; A.cml_cld = (S*)cml->cld;
  }
  // the per-column multiplier form has its own argument block (never together with the tendency buffer forms)
  KArgsSPP<double, S> M;
  static_cast<KArgs<double, S>&>(M) = A;
  for (const S*& m : M.mult) m = nullptr;
  if (const cloudsc_spp_t* spp = form.spp) {
    M.mult[SPP_RAMID] = (const S*)spp->ramid; M.mult[SPP_RCLDIFF] = (const S*)spp->rcldiff;
    M.mult[SPP_RCLCRIT] = (const S*)spp->rclcrit; M.mult[SPP_RLCRITSNOW] = (const S*)spp->rlcritsnow;
    M.mult[SPP_RPECONS] = (const S*)spp->rpecons;
  }
  // and so has the advancing form
  KArgsADV<double, S> V;
  static_cast<KArgs<double, S>&>(V) = A;
  V.adv_t = V.adv_q = V.adv_a = V.adv_clv = nullptr;
  if (const cloudsc_advance_t* adv = form.adv) {
    V.adv_t = (S*)adv->t; V.adv_q = (S*)adv->q; V.adv_a = (S*)adv->a; V.adv_clv = (S*)adv->clv;
  }
  const int nblocks = ngptot / nproma + (ngptot % nproma ? 1 : 0);
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  const int nreq = nthreads;                 // the caller's per-thread arrays have nreq entries
  nthreads = std::min(nthreads, nblocks);
  for (int t = 0; t < nreq; t++) {           // threads beyond the block count do nothing
    if (th.thread_seconds) th.thread_seconds[t] = 0.0;
    if (th.thread_blocks) th.thread_blocks[t] = 0;
    if (th.thread_columns) th.thread_columns[t] = 0;
  }
  std::atomic<int> next{0};
  const unsigned bits = form_bits(form);
  // per thread, as the C dwarf's zinfo (cloudsc_driver.c:185-228): its own
  // wall time, NPROMA blocks taken (icalls) and columns computed (igpc)
  auto worker = [&](int tid) {
    const auto s0 = std::chrono::steady_clock::now();
    std::vector<HostColumn<double>> col((size_t)nproma);
    int icalls = 0, igpc = 0;
    for (int b = next.fetch_add(1); b < nblocks; b = next.fetch_add(1)) {
      // the run_block of the form: those whose bits go together (form_bits_consistent), as on the GPU
      dispatch_bools(
          [&](auto AER, auto TB, auto PROG, auto SURF, auto CML, auto SPP, auto ADV) {
            if constexpr (form_bits_consistent(form_bits(TB, PROG, SURF, CML, SPP, ADV))) {
              if constexpr (ADV) run_block<double, AER, TB, PROG, SURF, CML, SPP, ADV>(c, V, b, col);
              else if constexpr (SPP) run_block<double, AER, TB, PROG, SURF, CML, SPP, ADV>(c, M, b, col);
              else run_block<double, AER, TB, PROG, SURF, CML, SPP, ADV>(c, A, b, col);
            }
            return 0;
          },
          aer, (bits & kFormTb) != 0, (bits & kFormProg) != 0, (bits & kFormSurf) != 0, (bits & kFormCml) != 0,
          (bits & kFormSpp) != 0, (bits & kFormAdv) != 0);
      icalls++;
      igpc += std::min(nproma, ngptot - b * nproma);
    }
    const auto s1 = std::chrono::steady_clock::now();
    if (th.thread_seconds) th.thread_seconds[tid] = std::chrono::duration<double>(s1 - s0).count();
    if (th.thread_blocks) th.thread_blocks[tid] = icalls;
    if (th.thread_columns) th.thread_columns[tid] = igpc;
  };
  const auto t0 = std::chrono::steady_clock::now();
  if (nthreads == 1) {
    worker(0);
  } else {
    std::vector<std::thread> pool;
    pool.reserve((size_t)nthreads);
    try {
      for (int t = 0; t < nthreads; t++) pool.emplace_back(worker, t);
    } catch (...) {
      rc = CLOUDSC_ENOMEM;          // the threads already started finish the blocks
    }
    for (auto& t : pool) t.join();
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (th.seconds) *th.seconds = std::chrono::duration<double>(t1 - t0).count();
  return rc;
}

// A run entry: the form's rules (check_step_form, with the bits `need` of the entry), then the block loop of the
// precision's storage type.  The host form computes in double: CLOUDSC_FP64 and CLOUDSC_MIXED.
int cpu_run_form(int precision, int ngptot, int nproma, int klev, const cloudsc_params_t* params,
                 const cloudsc_fields_t* f, const cloudsc_impl::StepForm& form, unsigned need, const CpuThreads& th) {
  if (cloudsc_impl::check_step_form(form, need, f) || !cloudsc_impl::precision_computes_double(precision))
    return CLOUDSC_EINVAL;
  switch (cloudsc_impl::precision_storage_bytes(precision)) {
    case sizeof(double): return cpu_run<double>(ngptot, nproma, klev, params, f, form, th);
    case sizeof(float): return cpu_run<float>(ngptot, nproma, klev, params, f, form, th);
    default: return CLOUDSC_EINVAL;
  }
}

}  // namespace

extern "C" int cloudsc_cpu_run_threads(int nthreads, int ngptot, int nproma, int klev,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f, double* seconds,
                                       double* thread_seconds, int* thread_blocks, int* thread_columns) {
  return cpu_run_form(CLOUDSC_FP64, ngptot, nproma, klev, params, f, {}, 0u,
                      {nthreads, seconds, thread_seconds, thread_blocks, thread_columns});
}

extern "C" int cloudsc_cpu_run_precision(int nthreads, int precision, int ngptot, int nproma, int klev,
                                         const cloudsc_params_t* params, const cloudsc_fields_t* f,
                                         double* seconds) {
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, {}, 0u, {nthreads, seconds});
}

extern "C" int cloudsc_cpu_run(int nthreads, int ngptot, int nproma, int klev, const cloudsc_params_t* params,
                               const cloudsc_fields_t* f, double* seconds) {
  return cloudsc_cpu_run_precision(nthreads, CLOUDSC_FP64, ngptot, nproma, klev, params, f, seconds);
}

extern "C" int cloudsc_cpu_run_tendbuf(int nthreads, int precision, int ngptot, int nproma, int klev, int tend_planes,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f) {
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, {tend_planes}, kFormTb, {nthreads});
}

extern "C" int cloudsc_cpu_run_outputs(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f) {
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, {0, outputs}, 0u, {nthreads});
}

extern "C" int cloudsc_cpu_run_tendbuf_outputs(int nthreads, int precision, int outputs, int ngptot, int nproma,
                                               int klev, int tend_planes, const cloudsc_params_t* params,
                                               const cloudsc_fields_t* f) {
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, {tend_planes, outputs}, kFormTb, {nthreads});
}

// (kFormProg: CLOUDSC_OUTPUTS_ALL is refused)
extern "C" int cloudsc_cpu_run_tendbuf_cml(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                           int tend_planes, const cloudsc_params_t* params, const cloudsc_fields_t* f,
                                           const cloudsc_tend_cml_t* cml) {
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, {tend_planes, outputs, cml},
                      kFormCml | kFormTb | kFormProg, {nthreads});
}

extern "C" int cloudsc_cpu_run_spp(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                   const cloudsc_params_t* params, const cloudsc_fields_t* f,
                                   const cloudsc_spp_t* spp) {
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, {0, outputs, nullptr, spp}, kFormSpp, {nthreads});
}

// (CLOUDSC_OUTPUTS_PROGNOSTIC alone is no form: form_bits_consistent)
extern "C" int cloudsc_cpu_run_advance(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f,
                                       const cloudsc_advance_t* adv) {
  cloudsc_impl::StepForm form;
  form.outputs = outputs;
  form.adv = adv;
  return cpu_run_form(precision, ngptot, nproma, klev, params, f, form, kFormAdv, {nthreads});
}
