// cloudsc_accumulate.hip -- add a step's local tendencies to the cumulative
// tendency planes (the Fortran drivers' BUFFER_CML) as a pass of its own:
// cloudsc_fields_accumulate_tendbuf on the device (one streaming kernel,
// stream-ordered), cloudsc_cpu_fields_accumulate_tendbuf on the host.
//
// For each of the seven planes T, Q, A, CLD(ql, qi, qr, qs), every level k and
// every global column g < ngptot:
//
//   cml[g / np][k][g % np] = cml[g / np][k][g % np] + loc[g / np][k][g % np]
//
// one add in the storage type (double for CLOUDSC_FP64, float for CLOUDSC_FP32
// and CLOUDSC_MIXED).  The vapour plane behind the four CLD planes is neither
// read nor written on either side.  This is the unfused path: the fused form is
// the kernels' own (cloudsc_gpu_run_tendbuf_cml, store_level in cloudsc_kcache.h).
//
// The kernel.  The item scheme of cloudsc_fieldset.h with four entries {a, b} =
// {tendency_loc_x, cml->x}, the CLD entry 4 * klev rows long; either side may
// be a plane of a packed buffer, so both block strides come from the table
// (FsTendTable).  Per item a lane walks its rows with eight loads per operand in
// flight before their eight stores.  Every byte is touched once: non-temporal
// loads and stores.  Lanes past ngptot do nothing.
#include <hip/hip_runtime.h>

#include "cloudsc_fieldset.h"

using namespace cloudsc_impl;

namespace {

constexpr int kAccSpecies = CLOUDSC_NCLV - 1;   // ql, qi, qr, qs: the vapour plane is left alone

// nrows rows of one column: loc + lo, cml + co address the first row, the row stride is the NPROMA
template <typename T>
__device__ __forceinline__ void acc_rows(const void* loc, void* cml, size_t lo, size_t co, size_t np, int nrows) {
  const T* l = (const T*)loc + lo;
  T* c = (T*)cml + co;
  for (int r = 0; r < nrows; r += kFsBatch) {
    T v[kFsBatch], w[kFsBatch];
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) {
        v[q] = __builtin_nontemporal_load(l + (size_t)(r + q) * np);
        w[q] = __builtin_nontemporal_load(c + (size_t)(r + q) * np);
      }
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) __builtin_nontemporal_store(w[q] + v[q], c + (size_t)(r + q) * np);
  }
}

// the per-item part of fs_kernel
template <typename T>
struct AccItem {
  using Args = FsTendTable;
  __device__ AccItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned np = (unsigned)a.anp;
    const FsPos p = fs_pos(g, np);
    const FsRows r = fs_rows(a, m, chunk);
    acc_rows<T>(a.e[m].a, a.e[m].b, fs_offset_strided(p, np, r, (size_t)a.abrows[m]),
                fs_offset_strided(p, np, r, (size_t)a.bbrows[m]), np, r.nrows);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};

// the same index arithmetic in plain loops: block b of every entry
template <typename T>
void acc_block(const FsTendTable& a, long long b) {
  const long long np = a.anp;
  const long long bsize = std::min<long long>(np, a.ngptot - b * np);
  for (int m = 0; m < a.n; m++) {
    const T* l = (const T*)a.e[m].a;
    T* c = (T*)a.e[m].b;
    for (long long row = 0; row < a.e[m].rows; row++) {
      const T* lrow = l + (size_t)(b * a.abrows[m] + row) * (size_t)np;
      T* crow = c + (size_t)(b * a.bbrows[m] + row) * (size_t)np;
      for (long long j = 0; j < bsize; j++) crow[j] = crow[j] + lrow[j];
    }
  }
}

// the argument rules and the table: four entries, rows klev, klev, klev, 4 * klev; a side's block stride in
// rows is planes * klev in a packed buffer, or the separate array's own (klev, 5 * klev)
int acc_build(int precision, int ngptot, int nproma, int klev, int loc_planes, const cloudsc_fields_t* f,
              int cml_planes, const cloudsc_tend_cml_t* cml, FsTendTable* a) {
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || nproma < 1 || nproma > kFsMaxNproma) return CLOUDSC_EINVAL;
  if (!fs_tend_planes_ok(loc_planes) || !fs_tend_planes_ok(cml_planes)) return CLOUDSC_EINVAL;
  if (!f || !f->tendency_loc_t || !f->tendency_loc_q || !f->tendency_loc_a || !f->tendency_loc_cld) return CLOUDSC_EINVAL;
  if (!cml || !cml->t || !cml->q || !cml->a || !cml->cld) return CLOUDSC_EINVAL;
  const void* const loc[4] = {f->tendency_loc_t, f->tendency_loc_q, f->tendency_loc_a, f->tendency_loc_cld};
  void* const dst[4] = {cml->t, cml->q, cml->a, cml->cld};
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      if (dst[i] == loc[j]) return CLOUDSC_EINVAL;
  for (int i = 0; i < 4; i++) {
    const long long own = i == 3 ? (long long)CLOUDSC_NCLV * klev : klev;
    a->e[i] = {loc[i], dst[i], i == 3 ? (long long)kAccSpecies * klev : (long long)klev};
    a->abrows[i] = loc_planes ? (long long)loc_planes * klev : own;
    a->bbrows[i] = cml_planes ? (long long)cml_planes * klev : own;
  }
  a->n = 4;
  fs_shape(a, ngptot, nproma, nproma);
  return CLOUDSC_OK;
}

}  // namespace

extern "C" int cloudsc_fields_accumulate_tendbuf(int device, void* stream, int precision, int ngptot, int nproma,
                                                 int klev, int loc_tend_planes, const cloudsc_fields_t* loc_fields,
                                                 int cml_tend_planes, const cloudsc_tend_cml_t* cml) {
  FsTendTable a = {};
  int ncu = 0;
  int rc = acc_build(precision, ngptot, nproma, klev, loc_tend_planes, loc_fields, cml_tend_planes, cml, &a);
  if (rc || (rc = fs_device(device, &ncu))) return rc;
  HIPCHK(hipSetDevice(device));
  const dim3 grid(fs_grid(a, ncu)), wg(kFsThreads);
  hipStream_t st = (hipStream_t)stream;
  if (precision_storage_bytes(precision) == 8) hipLaunchKernelGGL((fs_kernel<AccItem<double>>), grid, wg, 0, st, a);
  else hipLaunchKernelGGL((fs_kernel<AccItem<float>>), grid, wg, 0, st, a);
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_accumulate_tendbuf(int nthreads, int precision, int ngptot, int nproma, int klev,
                                                     int loc_tend_planes, const cloudsc_fields_t* loc_fields,
                                                     int cml_tend_planes, const cloudsc_tend_cml_t* cml) {
  FsTendTable a = {};
  const int rc = acc_build(precision, ngptot, nproma, klev, loc_tend_planes, loc_fields, cml_tend_planes, cml, &a);
  if (rc) return rc;
  void (*block)(const FsTendTable&, long long) =
      precision_storage_bytes(precision) == 8 ? acc_block<double> : acc_block<float>;
  const long long nblocks = ((long long)ngptot + nproma - 1) / nproma;
  fs_run_blocks(nthreads, nblocks, [&](int, long long b) { block(a, b); });
  return CLOUDSC_OK;
}
