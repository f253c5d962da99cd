// cloudsc_advance.hip -- advance the prognostic state by a step's local
// tendencies as a pass of its own: cloudsc_fields_advance on the device (one
// streaming kernel, stream-ordered), cloudsc_cpu_fields_advance on the host.
//
// For each of the seven quantities T, Q, A, CLD(ql, qi, qr, qs), every level k
// and every global column g < ngptot, with x the state member (pt, pq, pa,
// pclv), tmp = tendency_tmp_* and loc = tendency_loc_* at that element:
//
//   x0  = x  + ptsphy * tmp
//   adv = x0 + ptsphy * loc
//
// four operations, each rounded on its own (-ffp-contract=off), in double for
// CLOUDSC_FP64 and CLOUDSC_MIXED (float elements widen exactly, the result is
// narrowed by one conversion) and in float for CLOUDSC_FP32.  The vapour planes
// are neither read nor written.  This is the unfused path: the fused form is
// the kernels' own (cloudsc_gpu_run_advance, store_level_adv in
// cloudsc_kcache.h), which in mixed precision takes loc before its narrowing.
//
// The kernel.  The item scheme of cloudsc_fieldset.h with four entries {a, b} =
// {state member, adv member}, the CLD entry 4 * klev rows long in arrays whose
// blocks are 5 * klev rows apart; tmp and loc of an entry have its shape and
// travel beside the table.  adv may be the state member itself: a lane loads
// its rows of the three operands before it stores them, and no other lane
// touches its column.  Every byte is touched once: non-temporal loads and
// stores.  Lanes past ngptot do nothing.
#include <hip/hip_runtime.h>

#include "cloudsc_fieldset.h"

using namespace cloudsc_impl;

namespace {

constexpr int kAdvSpecies = CLOUDSC_NCLV - 1;   // ql, qi, qr, qs: the vapour plane is left alone

struct AdvTable : FsTable<void> {
  const void* tmp[4];
  const void* loc[4];
  long long brows[4];   // rows between consecutive blocks of entry i, in all four operands
  double ptsphy;        // PTSPHY; the fp32 pass computes with (float)ptsphy, as the fp32 step does
};

// one element: R the working type
template <typename R>
__host__ __device__ __forceinline__ R adv_value(R x, R tmp, R loc, R dt) {
  const R a = dt * tmp;
  const R x0 = x + a;
  const R b = dt * loc;
  return x0 + b;
}

// nrows rows of one column at element offset `off` of the four operands, the row stride the NPROMA
template <typename T, typename R>
__device__ __forceinline__ void adv_rows(const void* x, const void* tmp, const void* loc, void* dst, size_t off,
                                         size_t np, int nrows, R dt) {
  const T* xs = (const T*)x + off;
  const T* ts = (const T*)tmp + off;
  const T* ls = (const T*)loc + off;
  T* d = (T*)dst + off;
  for (int r = 0; r < nrows; r += kFsBatch) {
    T u[kFsBatch], v[kFsBatch], w[kFsBatch];
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) {
        u[q] = __builtin_nontemporal_load(xs + (size_t)(r + q) * np);
        v[q] = __builtin_nontemporal_load(ts + (size_t)(r + q) * np);
        w[q] = __builtin_nontemporal_load(ls + (size_t)(r + q) * np);
      }
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows)
        __builtin_nontemporal_store((T)adv_value<R>((R)u[q], (R)v[q], (R)w[q], dt), d + (size_t)(r + q) * np);
  }
}

// the per-item part of fs_kernel
template <typename T, typename R>
struct AdvItem {
  using Args = AdvTable;
  __device__ AdvItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned np = (unsigned)a.anp;
    const FsPos p = fs_pos(g, np);
    const FsRows r = fs_rows(a, m, chunk);
    adv_rows<T, R>(a.e[m].a, a.tmp[m], a.loc[m], a.e[m].b, fs_offset_strided(p, np, r, (size_t)a.brows[m]), np,
                   r.nrows, (R)a.ptsphy);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};

// the same index arithmetic in plain loops: block b of every entry
template <typename T, typename R>
void adv_block(const AdvTable& a, long long b) {
  const long long np = a.anp;
  const long long bsize = std::min<long long>(np, a.ngptot - b * np);
  const R dt = (R)a.ptsphy;
  for (int m = 0; m < a.n; m++) {
    for (long long row = 0; row < a.e[m].rows; row++) {
      const size_t off = (size_t)(b * a.brows[m] + row) * (size_t)np;
      const T* x = (const T*)a.e[m].a + off;
      const T* tmp = (const T*)a.tmp[m] + off;
      const T* loc = (const T*)a.loc[m] + off;
      T* d = (T*)a.e[m].b + off;
      for (long long j = 0; j < bsize; j++) d[j] = (T)adv_value<R>((R)x[j], (R)tmp[j], (R)loc[j], dt);
    }
  }
}

// the argument rules and the table: four entries, rows klev, klev, klev, 4 * klev
int adv_build(int precision, int ngptot, int nproma, int klev, const cloudsc_fields_t* f, const cloudsc_advance_t* adv,
              AdvTable* a) {
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || nproma < 1 || nproma > kFsMaxNproma) return CLOUDSC_EINVAL;
  if (!advance_members_ok(f, adv)) return CLOUDSC_EINVAL;
  const void* const x[4] = {f->pt, f->pq, f->pa, f->pclv};
  const void* const tmp[4] = {f->tendency_tmp_t, f->tendency_tmp_q, f->tendency_tmp_a, f->tendency_tmp_cld};
  const void* const loc[4] = {f->tendency_loc_t, f->tendency_loc_q, f->tendency_loc_a, f->tendency_loc_cld};
  void* const dst[4] = {adv->t, adv->q, adv->a, adv->clv};
  for (int i = 0; i < 4; i++)
    if (!x[i] || !tmp[i] || !loc[i]) return CLOUDSC_EINVAL;
  for (int i = 0; i < 4; i++) {
    a->e[i] = {x[i], dst[i], i == 3 ? (long long)kAdvSpecies * klev : (long long)klev};
    a->tmp[i] = tmp[i];
    a->loc[i] = loc[i];
    a->brows[i] = i == 3 ? (long long)CLOUDSC_NCLV * klev : (long long)klev;
  }
  a->n = 4;
  fs_shape(a, ngptot, nproma, nproma);
  return CLOUDSC_OK;
}

}  // namespace

extern "C" int cloudsc_fields_advance(int device, void* stream, int precision, int ngptot, int nproma, int klev,
                                      const cloudsc_fields_t* device_fields, const cloudsc_advance_t* adv) {
  AdvTable a = {};
  int ncu = 0;
  int rc = adv_build(precision, ngptot, nproma, klev, device_fields, adv, &a);
  if (rc || (rc = fs_device(device, &ncu))) return rc;
  const ParamSet* ps = device_default_params(device);
  if (!ps || !ps->dev) return CLOUDSC_ENOINIT;
  a.ptsphy = ps->ptsphy;
  HIPCHK(hipSetDevice(device));
  const dim3 grid(fs_grid(a, ncu)), wg(kFsThreads);
  hipStream_t st = (hipStream_t)stream;
  switch (precision) {
    case CLOUDSC_FP64: hipLaunchKernelGGL((fs_kernel<AdvItem<double, double>>), grid, wg, 0, st, a); break;
    case CLOUDSC_MIXED: hipLaunchKernelGGL((fs_kernel<AdvItem<float, double>>), grid, wg, 0, st, a); break;
    default: hipLaunchKernelGGL((fs_kernel<AdvItem<float, float>>), grid, wg, 0, st, a); break;
  }
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_advance(int nthreads, int precision, int ngptot, int nproma, int klev,
                                          const cloudsc_params_t* params, const cloudsc_fields_t* host_fields,
                                          const cloudsc_advance_t* adv) {
  AdvTable a = {};
  const int rc = adv_build(precision, ngptot, nproma, klev, host_fields, adv, &a);
  if (rc) return rc;
  if (!params || !(params->ptsphy > 0.0)) return CLOUDSC_EINVAL;
  a.ptsphy = params->ptsphy;
  void (*block)(const AdvTable&, long long) = precision == CLOUDSC_FP64    ? adv_block<double, double>
                                              : precision == CLOUDSC_MIXED ? adv_block<float, double>
                                                                           : adv_block<float, float>;
  const long long nblocks = ((long long)ngptot + nproma - 1) / nproma;
  fs_run_blocks(nthreads, nblocks, [&](int, long long b) { block(a, b); });
  return CLOUDSC_OK;
}
