// cloudsc_convert.hip -- copy a field set into another NPROMA blocking and / or
// storage type: cloudsc_fields_convert on the device (one streaming kernel,
// stream-ordered), cloudsc_cpu_fields_convert on the host.
//
// For every member set in both field sets, every row r of its kind and every
// global column g < ngptot:
//
//   dst[g / dnp][r][g % dnp] = (dst type) src[g / snp][r][g % snp]
//
// The kernel.  The item scheme of cloudsc_fieldset.h, entry {a, b} = {src, dst}:
// per item a lane walks its rows with eight loads in flight before their eight
// stores.  Loads and stores are plain non-temporal vector accesses: each byte is
// touched once.  Lanes past ngptot do nothing, so the padding lanes of the
// destination's last block keep their contents.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cloudsc_fieldset.h"

using namespace cloudsc_impl;

namespace {

using ConvTable = FsTable<void>;   // entry {a, b} = {src, dst}

// the per-item part of fs_kernel
template <int SB, int DB>
struct ConvItem {
  using Args = ConvTable;
  using S = typename ConvPair<SB, DB>::S;
  using D = typename ConvPair<SB, DB>::D;
  __device__ ConvItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned snp = (unsigned)a.anp, dnp = (unsigned)a.bnp;
    const FsPos sp = fs_pos(g, snp), dp = fs_pos(g, dnp);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t so = fs_offset(sp, snp, r), doff = fs_offset(dp, dnp, r);
    if (a.int_mask >> m & 1) conv_rows<int, int>(a.e[m].a, a.e[m].b, so, doff, snp, dnp, r.nrows);
    else conv_rows<S, D>(a.e[m].a, a.e[m].b, so, doff, snp, dnp, r.nrows);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};

// The same with the tendency members of either side in packed buffers (cloudsc_fields_convert_tendbuf): the
// block strides come from the table, everything else is ConvItem's.
template <int SB, int DB>
struct ConvTendItem {
  using Args = FsTendTable;
  using S = typename ConvPair<SB, DB>::S;
  using D = typename ConvPair<SB, DB>::D;
  __device__ ConvTendItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned snp = (unsigned)a.anp, dnp = (unsigned)a.bnp;
    const FsPos sp = fs_pos(g, snp), dp = fs_pos(g, dnp);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t so = fs_offset_strided(sp, snp, r, (size_t)a.abrows[m]);
    const size_t doff = fs_offset_strided(dp, dnp, r, (size_t)a.bbrows[m]);
    if (a.int_mask >> m & 1) conv_rows<int, int>(a.e[m].a, a.e[m].b, so, doff, snp, dnp, r.nrows);
    else conv_rows<S, D>(a.e[m].a, a.e[m].b, so, doff, snp, dnp, r.nrows);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};

// the columns of destination block db of one entry, on the host: the kernel's index arithmetic in plain loops
template <typename S, typename D>
void conv_block_entry(const FsEntry<void>& e, const ConvTable& a, long long db, long long sbrows, long long dbrows) {
  const long long snp = a.anp, dnp = a.bnp, g0 = db * dnp;
  const long long bsize = std::min<long long>(dnp, a.ngptot - g0);
  const S* s = (const S*)e.a;
  D* d = (D*)e.b;
  for (long long row = 0; row < e.rows; row++) {
    D* drow = d + (size_t)(db * dbrows + row) * (size_t)dnp;
    fs_runs(g0, bsize, snp, [&](long long jl, long long sb, long long sj, long long run) {
      const S* srow = s + (size_t)(sb * sbrows + row) * (size_t)snp + sj;
      for (long long i = 0; i < run; i++) drow[jl + i] = (D)srow[i];
    });
  }
}

// sbrows / dbrows: the rows between consecutive blocks of every entry in src / dst (NULL: the entry's own rows)
template <int SB, int DB>
void conv_block(const ConvTable& a, long long db, const long long* sbrows, const long long* dbrows) {
  for (int m = 0; m < a.n; m++) {
    const long long sr = sbrows ? sbrows[m] : a.e[m].rows, dr = dbrows ? dbrows[m] : a.e[m].rows;
    if (a.int_mask >> m & 1) conv_block_entry<int, int>(a.e[m], a, db, sr, dr);
    else conv_block_entry<typename ConvPair<SB, DB>::S, typename ConvPair<SB, DB>::D>(a.e[m], a, db, sr, dr);
  }
}

}  // namespace

// outputs: the selection both sets were allocated for (the shape of the four surface flux members)
static int convert_impl(int device, void* stream, int ngptot, int klev, int src_precision, int src_nproma,
                        const cloudsc_fields_t* src, int dst_precision, int dst_nproma, const cloudsc_fields_t* dst,
                        int outputs) {
  ConvTable a = {};
  int ncu = 0;
  int rc = fs_build(ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, &a, nullptr, outputs);
  if (rc || (rc = fs_device(device, &ncu))) return rc;
  HIPCHK(hipSetDevice(device));
  const dim3 grid(fs_grid(a, ncu)), wg(kFsThreads);
  hipStream_t st = (hipStream_t)stream;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  if (s8 && d8) hipLaunchKernelGGL((fs_kernel<ConvItem<8, 8>>), grid, wg, 0, st, a);
  else if (s8) hipLaunchKernelGGL((fs_kernel<ConvItem<8, 4>>), grid, wg, 0, st, a);
  else if (d8) hipLaunchKernelGGL((fs_kernel<ConvItem<4, 8>>), grid, wg, 0, st, a);
  else hipLaunchKernelGGL((fs_kernel<ConvItem<4, 4>>), grid, wg, 0, st, a);
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_convert(int device, void* stream, int ngptot, int klev, int src_precision,
                                      int src_nproma, const cloudsc_fields_t* src, int dst_precision,
                                      int dst_nproma, const cloudsc_fields_t* dst) {
  return convert_impl(device, stream, ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst,
                      CLOUDSC_OUTPUTS_ALL);
}

extern "C" int cloudsc_fields_convert_outputs(int device, void* stream, int ngptot, int klev, int outputs,
                                              int src_precision, int src_nproma, const cloudsc_fields_t* src,
                                              int dst_precision, int dst_nproma, const cloudsc_fields_t* dst) {
  if (!outputs_known(outputs)) return CLOUDSC_EINVAL;
  if (!outputs_surface(outputs))   // cloudsc_fields_convert itself
    return cloudsc_fields_convert(device, stream, ngptot, klev, src_precision, src_nproma, src, dst_precision,
                                  dst_nproma, dst);
  return convert_impl(device, stream, ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst,
                      outputs);
}

int cloudsc_impl::cpu_convert(int nthreads, int ngptot, int klev, int src_precision, int src_nproma,
                              const cloudsc_fields_t* src, int dst_precision, int dst_nproma,
                              const cloudsc_fields_t* dst, int outputs) {
  ConvTable a = {};
  int rc = fs_build(ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, &a, nullptr, outputs);
  if (rc) return rc;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  void (*block)(const ConvTable&, long long, const long long*, const long long*) =
      s8 && d8 ? conv_block<8, 8> : s8 ? conv_block<8, 4> : d8 ? conv_block<4, 8> : conv_block<4, 4>;
  const long long nblocks = ((long long)ngptot + dst_nproma - 1) / dst_nproma;
  fs_run_blocks(nthreads, nblocks, [&](int, long long b) { block(a, b, nullptr, nullptr); });
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_convert(int nthreads, int ngptot, int klev, int src_precision, int src_nproma,
                                          const cloudsc_fields_t* src, int dst_precision, int dst_nproma,
                                          const cloudsc_fields_t* dst) {
  return cpu_convert(nthreads, ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst,
                     CLOUDSC_OUTPUTS_ALL);
}

extern "C" int cloudsc_fields_convert_tendbuf(int device, void* stream, int ngptot, int klev, int src_precision,
                                              int src_nproma, int src_tend_planes, const cloudsc_fields_t* src,
                                              int dst_precision, int dst_nproma, int dst_tend_planes,
                                              const cloudsc_fields_t* dst) {
  FsTendTable a = {};
  int ncu = 0;
  int rc = fs_build_tend(ngptot, klev, src_precision, src_nproma, src_tend_planes, src, dst_precision, dst_nproma,
                         dst_tend_planes, dst, &a);
  if (rc || (rc = fs_device(device, &ncu))) return rc;
  HIPCHK(hipSetDevice(device));
  const dim3 grid(fs_grid(a, ncu)), wg(kFsThreads);
  hipStream_t st = (hipStream_t)stream;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  if (s8 && d8) hipLaunchKernelGGL((fs_kernel<ConvTendItem<8, 8>>), grid, wg, 0, st, a);
  else if (s8) hipLaunchKernelGGL((fs_kernel<ConvTendItem<8, 4>>), grid, wg, 0, st, a);
  else if (d8) hipLaunchKernelGGL((fs_kernel<ConvTendItem<4, 8>>), grid, wg, 0, st, a);
  else hipLaunchKernelGGL((fs_kernel<ConvTendItem<4, 4>>), grid, wg, 0, st, a);
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_convert_tendbuf(int nthreads, int ngptot, int klev, int src_precision,
                                                  int src_nproma, int src_tend_planes, const cloudsc_fields_t* src,
                                                  int dst_precision, int dst_nproma, int dst_tend_planes,
                                                  const cloudsc_fields_t* dst) {
  FsTendTable a = {};
  int rc = fs_build_tend(ngptot, klev, src_precision, src_nproma, src_tend_planes, src, dst_precision, dst_nproma,
                         dst_tend_planes, dst, &a);
  if (rc) return rc;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  void (*block)(const ConvTable&, long long, const long long*, const long long*) =
      s8 && d8 ? conv_block<8, 8> : s8 ? conv_block<8, 4> : d8 ? conv_block<4, 8> : conv_block<4, 4>;
  const long long nblocks = ((long long)ngptot + dst_nproma - 1) / dst_nproma;
  fs_run_blocks(nthreads, nblocks, [&](int, long long b) { block(a, b, a.abrows, a.bbrows); });
  return CLOUDSC_OK;
}
