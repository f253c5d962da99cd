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
// CML: the cumulative tendency form, A a KArgsCML and the local tendencies added to its planes (load_cml, store_level_cml)
template <typename real, bool AER, bool TB, bool PROG = false, bool SURF = false, bool CML = false, typename S>
void run_block(const DevParams<real>& c, const KArgs<real, S>& A, int b, std::vector<HostColumn<real>>& col) {
  const int nproma = A.nproma, klev = A.klev;
  const int bsize = std::min(nproma, A.ngptot - b * nproma);
  const size_t u1 = (size_t)b * nproma;
  const size_t u2 = (size_t)b * klev * nproma;
  const size_t uh = (size_t)b * (klev + 1) * nproma;
  const size_t u3 = (size_t)b * 5 * klev * nproma;
  const int ncldtop0 = c.ncldtop - 1;
  const int l1 = 1 < klev ? 1 : klev - 1;
  for (int jl = 0; jl < bsize; jl++) {
    const unsigned lo = (unsigned)jl * (unsigned)sizeof(S);
    HostColumn<real>& h = col[jl];
    init_carry<real, PROG>(h.cs);
    flux_top<PROG, SURF>(c, A, uh, lo);
    h.cc = column_constants(c, A, u1, uh, lo);
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
      if (physics) physics_level(c, k, klev, ncldtop0, cur, h.nb, h.cc, ls, h.cs, po);
      if constexpr (CML) {
        CmlIn<real> cm;
        load_cml(cm, A, u2, k, klev, nproma, lo);
        store_level_cml(A, u2, k, klev, nproma, lo, ls, po, cm);
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

// the block loop over fields of element type S, computed in double
template <typename S>
int cpu_run(int nthreads, int ngptot, int nproma, int klev, const cloudsc_params_t* params,
            const cloudsc_fields_t* f, double* seconds, double* thread_seconds, int* thread_blocks,
            int* thread_columns, int tend_planes = 0, int outputs = CLOUDSC_OUTPUTS_ALL,
            const cloudsc_tend_cml_t* cml = nullptr) {
  int rc = cloudsc_impl::check_params(params);
  if (rc) return rc;
  if (!f || !cloudsc_impl::fields_complete(f, outputs, cml != nullptr) || ngptot <= 0 || nproma <= 0 || klev < 2)
    return CLOUDSC_EINVAL;
  const bool aer = params->laericesed || params->laericeauto;
  if (aer && (!f->pre_ice || !f->picrit_aer || !f->pnice)) return CLOUDSC_EINVAL;
  if (nthreads <= 0 && (thread_seconds || thread_blocks || thread_columns)) return CLOUDSC_EINVAL;
  const DevParams<double> c = fold_params<double>(*params);
  KArgsCML<double, S> A;
  static_cast<KArgs<double, S>&>(A) = make_kargs<double, S>(f, ngptot, nproma, klev, nullptr);
  A.tend_planes = tend_planes;   // 0: separate arrays
  A.cml_t = A.cml_q = A.cml_a = A.cml_cld = nullptr;
  if (cml) { A.cml_t = (S*)cml->t; A.cml_q = (S*)cml->q; A.cml_a = (S*)cml->a; A.cml_cld = (S*)cml->cld; }
  const int nblocks = ngptot / nproma + (ngptot % nproma ? 1 : 0);
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  const int nreq = nthreads;                 // the caller's per-thread arrays have nreq entries
  nthreads = std::min(nthreads, nblocks);
  for (int t = 0; t < nreq; t++) {           // threads beyond the block count do nothing
    if (thread_seconds) thread_seconds[t] = 0.0;
    if (thread_blocks) thread_blocks[t] = 0;
    if (thread_columns) thread_columns[t] = 0;
  }
  std::atomic<int> next{0};
  // per thread, as the C dwarf's zinfo (cloudsc_driver.c:185-228): its own
  // wall time, NPROMA blocks taken (icalls) and columns computed (igpc)
  auto worker = [&](int tid) {
    const auto s0 = std::chrono::steady_clock::now();
    std::vector<HostColumn<double>> col((size_t)nproma);
    int icalls = 0, igpc = 0;
    for (int b = next.fetch_add(1); b < nblocks; b = next.fetch_add(1)) {
      if (cml && outputs == CLOUDSC_OUTPUTS_SURFACE) {
        if (aer) run_block<double, true, true, true, true, true>(c, A, b, col);
        else run_block<double, false, true, true, true, true>(c, A, b, col);
      } else if (cml) {
        if (aer) run_block<double, true, true, true, false, true>(c, A, b, col);
        else run_block<double, false, true, true, false, true>(c, A, b, col);
      } else if (outputs == CLOUDSC_OUTPUTS_SURFACE && tend_planes) {
        if (aer) run_block<double, true, true, true, true>(c, A, b, col);
        else run_block<double, false, true, true, true>(c, A, b, col);
      } else if (outputs == CLOUDSC_OUTPUTS_SURFACE) {
        if (aer) run_block<double, true, false, true, true>(c, A, b, col);
        else run_block<double, false, false, true, true>(c, A, b, col);
      } else if (outputs == CLOUDSC_OUTPUTS_PROGNOSTIC && tend_planes) {
        if (aer) run_block<double, true, true, true>(c, A, b, col);
        else run_block<double, false, true, true>(c, A, b, col);
      } else if (outputs == CLOUDSC_OUTPUTS_PROGNOSTIC) {
        if (aer) run_block<double, true, false, true>(c, A, b, col);
        else run_block<double, false, false, true>(c, A, b, col);
      } else if (tend_planes) {
        if (aer) run_block<double, true, true>(c, A, b, col);
        else run_block<double, false, true>(c, A, b, col);
      } else if (aer) {
        run_block<double, true, false>(c, A, b, col);
      } else {
        run_block<double, false, false>(c, A, b, col);
      }
      icalls++;
      igpc += std::min(nproma, ngptot - b * nproma);
    }
    const auto s1 = std::chrono::steady_clock::now();
    if (thread_seconds) thread_seconds[tid] = std::chrono::duration<double>(s1 - s0).count();
    if (thread_blocks) thread_blocks[tid] = icalls;
    if (thread_columns) thread_columns[tid] = igpc;
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
  if (seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
  return rc;
}

}  // namespace

extern "C" int cloudsc_cpu_run_threads(int nthreads, int ngptot, int nproma, int klev,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f, double* seconds,
                                       double* thread_seconds, int* thread_blocks, int* thread_columns) {
  return cpu_run<double>(nthreads, ngptot, nproma, klev, params, f, seconds, thread_seconds, thread_blocks,
                         thread_columns);
}

extern "C" int cloudsc_cpu_run_precision(int nthreads, int precision, int ngptot, int nproma, int klev,
                                         const cloudsc_params_t* params, const cloudsc_fields_t* f,
                                         double* seconds) {
  if (!cloudsc_impl::precision_computes_double(precision)) return CLOUDSC_EINVAL;   // the host form computes in double
  switch (cloudsc_impl::precision_storage_bytes(precision)) {
    case sizeof(double):
      return cpu_run<double>(nthreads, ngptot, nproma, klev, params, f, seconds, nullptr, nullptr, nullptr);
    case sizeof(float):
      return cpu_run<float>(nthreads, ngptot, nproma, klev, params, f, seconds, nullptr, nullptr, nullptr);
    default: return CLOUDSC_EINVAL;
  }
}

extern "C" int cloudsc_cpu_run(int nthreads, int ngptot, int nproma, int klev, const cloudsc_params_t* params,
                               const cloudsc_fields_t* f, double* seconds) {
  return cloudsc_cpu_run_precision(nthreads, CLOUDSC_FP64, ngptot, nproma, klev, params, f, seconds);
}

extern "C" int cloudsc_cpu_run_tendbuf(int nthreads, int precision, int ngptot, int nproma, int klev, int tend_planes,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f) {
  if (tend_planes < CLOUDSC_TENDBUF_PLANES_MIN || tend_planes > CLOUDSC_TENDBUF_PLANES_MAX) return CLOUDSC_EINVAL;
  if (!cloudsc_impl::precision_computes_double(precision)) return CLOUDSC_EINVAL;   // as cloudsc_cpu_run_precision
  switch (cloudsc_impl::precision_storage_bytes(precision)) {
    case sizeof(double):
      return cpu_run<double>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, tend_planes);
    case sizeof(float):
      return cpu_run<float>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, tend_planes);
    default: return CLOUDSC_EINVAL;
  }
}

extern "C" int cloudsc_cpu_run_outputs(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                       const cloudsc_params_t* params, const cloudsc_fields_t* f) {
  if (!cloudsc_impl::outputs_known(outputs)) return CLOUDSC_EINVAL;
  if (!cloudsc_impl::precision_computes_double(precision)) return CLOUDSC_EINVAL;   // as cloudsc_cpu_run_precision
  switch (cloudsc_impl::precision_storage_bytes(precision)) {
    case sizeof(double):
      return cpu_run<double>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, 0, outputs);
    case sizeof(float):
      return cpu_run<float>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, 0, outputs);
    default: return CLOUDSC_EINVAL;
  }
}

extern "C" int cloudsc_cpu_run_tendbuf_outputs(int nthreads, int precision, int outputs, int ngptot, int nproma,
                                               int klev, int tend_planes, const cloudsc_params_t* params,
                                               const cloudsc_fields_t* f) {
  if (!cloudsc_impl::outputs_known(outputs)) return CLOUDSC_EINVAL;
  if (tend_planes < CLOUDSC_TENDBUF_PLANES_MIN || tend_planes > CLOUDSC_TENDBUF_PLANES_MAX) return CLOUDSC_EINVAL;
  if (!cloudsc_impl::precision_computes_double(precision)) return CLOUDSC_EINVAL;   // as cloudsc_cpu_run_precision
  switch (cloudsc_impl::precision_storage_bytes(precision)) {
    case sizeof(double):
      return cpu_run<double>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, tend_planes,
                             outputs);
    case sizeof(float):
      return cpu_run<float>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, tend_planes,
                            outputs);
    default: return CLOUDSC_EINVAL;
  }
}

extern "C" int cloudsc_cpu_run_tendbuf_cml(int nthreads, int precision, int outputs, int ngptot, int nproma, int klev,
                                           int tend_planes, const cloudsc_params_t* params, const cloudsc_fields_t* f,
                                           const cloudsc_tend_cml_t* cml) {
  if (outputs != CLOUDSC_OUTPUTS_PROGNOSTIC && outputs != CLOUDSC_OUTPUTS_SURFACE) return CLOUDSC_EINVAL;   // not ALL
  if (tend_planes < CLOUDSC_TENDBUF_PLANES_MIN || tend_planes > CLOUDSC_TENDBUF_PLANES_MAX) return CLOUDSC_EINVAL;
  if (!cloudsc_impl::precision_computes_double(precision)) return CLOUDSC_EINVAL;   // as cloudsc_cpu_run_precision
  if (cloudsc_impl::check_tend_cml(f, cml)) return CLOUDSC_EINVAL;
  switch (cloudsc_impl::precision_storage_bytes(precision)) {
    case sizeof(double):
      return cpu_run<double>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, tend_planes,
                             outputs, cml);
    case sizeof(float):
      return cpu_run<float>(nthreads, ngptot, nproma, klev, params, f, nullptr, nullptr, nullptr, nullptr, tend_planes,
                            outputs, cml);
    default: return CLOUDSC_EINVAL;
  }
}
