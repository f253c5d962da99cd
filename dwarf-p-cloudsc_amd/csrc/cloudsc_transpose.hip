// cloudsc_transpose.hip -- copy a field set between the block layout and the
// level-contiguous column layout: cloudsc_fields_convert_layout on the device
// (stream-ordered), cloudsc_cpu_fields_convert_layout on the host.
//
// For every member set in both field sets, every row r of its kind and every
// global column g < ngptot, the element is
//
//   CLOUDSC_LAYOUT_BLOCKED  [g / np][r][g % np]
//   CLOUDSC_LAYOUT_LEVELS   [g][r]                 (rows of a column contiguous)
//
// and dst = (dst type) src as in cloudsc_fields_convert.  Two sets of one layout
// and the members of one row (surface fields, ktype: the same array in both
// layouts) go to cloudsc_fields_convert_outputs; what is left is a transpose.
//
// The kernel.  The items of cloudsc_fieldset.h -- (member, tile of 256 columns,
// chunk of 16 rows), strided by the workgroups in the walker's order -- with the
// kernel's own loop: a wave takes 64 columns of the tile through a wave-private
// LDS tile of 16 rows x 64 columns, so there is no workgroup barrier, and lanes
// past ngptot still serve the LEVELS side of the columns before them.
//
//   BLOCKED side  lane l holds column l and walks the 16 rows: a wave's access
//                 to a row is runs of min(NPROMA, 64) elements, as in the copy.
//   LEVELS side   lane l holds row l % 16 of column 4 q + l / 16 in access q of
//                 16: a wave's access is four runs of 16 rows (128 bytes of
//                 doubles, 64 of floats), one per column.
//
// The tile holds the narrower of the two storage types (the one conversion
// happens before a narrowing copy's LDS store and after a widening copy's LDS
// load): 8 KiB per wave of doubles, 32 KiB per workgroup.  Element (row r,
// column c) lies at r * 64 + (c ^ r ^ (c & 1) << 4); DESIGN.md section 3.27
// counts the bank conflicts.  Loads and stores of global memory are
// non-temporal: each byte is touched once.
#include <hip/hip_runtime.h>

#include "cloudsc_fieldset.h"

using namespace cloudsc_impl;

namespace {

using ConvTable = FsTable<void>;   // entry {a, b} = {src, dst}; the NPROMA of a LEVELS side is not looked at

constexpr int kTrWave = 64;                     // columns of a wave's tile = lanes
constexpr int kTrWaves = kFsThreads / kTrWave;  // wave tiles of a workgroup
constexpr int kTrCols = kTrWave / kFsRows;      // columns of one LEVELS access of a wave
static_assert(kFsRows == 16 && kTrWave == 64, "the swizzle takes 16 rows of 64 columns");

// the tile's element index of (row, column): a row's 64 columns permuted by the row, and the odd columns
// moved to the other half of a 32-bank row
__device__ __forceinline__ unsigned tr_at(unsigned r, unsigned c) { return r * kTrWave + (c ^ r ^ ((c & 1u) << 4)); }

// orders a wave's LDS writes before its LDS reads of other lanes' elements (and the reverse): the wave's LDS
// accesses execute in order, so nothing is waited for
__device__ __forceinline__ void tr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// TO_LEVELS: a BLOCKED (NPROMA a.anp), b LEVELS; otherwise a LEVELS, b BLOCKED (NPROMA a.bnp)
template <int SB, int DB, bool TO_LEVELS>
__global__ void __launch_bounds__(kFsThreads) tr_kernel(const ConvTable a) {
  using S = typename ConvPair<SB, DB>::S;
  using D = typename ConvPair<SB, DB>::D;
  using T = typename std::conditional<(SB <= DB), S, D>::type;   // what the tile holds
  __shared__ T lds[kTrWaves][kFsRows * kTrWave];
  const unsigned lane = threadIdx.x % kTrWave, wave = threadIdx.x / kTrWave;
  T* __restrict__ t = lds[wave];
  const unsigned lr = lane % kFsRows, lc = lane / kFsRows;   // the LEVELS side: this lane's row and column of four
  const unsigned np = (unsigned)(TO_LEVELS ? a.anp : a.bnp);
  int m = 0;
  unsigned long long first = 0;   // the first item of entry m
  unsigned long long nchunk = fs_chunks(a.e[0].rows);
  unsigned long long count = nchunk * a.ntiles;
  for (unsigned long long it = blockIdx.x;; it += gridDim.x) {
    while (it >= first + count) {
      first += count;
      if (++m >= a.n) return;
      nchunk = fs_chunks(a.e[m].rows);
      count = nchunk * a.ntiles;
    }
    const unsigned long long local = it - first, tile = local / nchunk, chunk = local - tile * nchunk;
    const unsigned long long col0 = tile * kFsThreads + wave * kTrWave;   // the wave's first column
    if (col0 >= (unsigned long long)a.ngptot) continue;                   // the whole wave: its tile is not used
    const unsigned ncols = (unsigned)std::min<unsigned long long>(kTrWave, (unsigned long long)a.ngptot - col0);
    const FsRows r = fs_rows(a, m, chunk);
    const S* __restrict__ s = (const S*)a.e[m].a;
    D* __restrict__ d = (D*)a.e[m].b;
    // the LEVELS side's element of row lr of the wave's column lc: columns are r.rows apart
    const size_t lev = ((size_t)col0 + lc) * r.rows + r.row0 + lr;
    const size_t lev_step = (size_t)kTrCols * r.rows;
    // the BLOCKED side's element of row r.row0 of column col0 + lane: rows are np apart
    size_t blk = 0;
    if (lane < ncols) blk = fs_offset(fs_pos((unsigned)col0 + lane, np), np, r);
    if (TO_LEVELS) {
      if (lane < ncols) {
        for (int q0 = 0; q0 < kFsRows; q0 += kFsBatch) {
          S v[kFsBatch];
#pragma unroll
          for (int q = 0; q < kFsBatch; q++)
            if (q0 + q < r.nrows) v[q] = __builtin_nontemporal_load(s + blk + (size_t)(q0 + q) * np);
#pragma unroll
          for (int q = 0; q < kFsBatch; q++)
            if (q0 + q < r.nrows) t[tr_at(q0 + q, lane)] = (T)v[q];
        }
      }
      tr_wave_sync();
      if ((int)lr < r.nrows) {
#pragma unroll
        for (int q = 0; q < kFsRows; q++) {
          const unsigned c = q * kTrCols + lc;
          if (c < ncols) __builtin_nontemporal_store((D)t[tr_at(lr, c)], d + lev + q * lev_step);
        }
      }
    } else {
      if ((int)lr < r.nrows) {
        for (int q0 = 0; q0 < kFsRows; q0 += kFsBatch) {
          S v[kFsBatch];
#pragma unroll
          for (int q = 0; q < kFsBatch; q++)
            if ((q0 + q) * kTrCols + lc < ncols) v[q] = __builtin_nontemporal_load(s + lev + (q0 + q) * lev_step);
#pragma unroll
          for (int q = 0; q < kFsBatch; q++)
            if ((q0 + q) * kTrCols + lc < ncols) t[tr_at(lr, (q0 + q) * kTrCols + lc)] = (T)v[q];
        }
      }
      tr_wave_sync();
      if (lane < ncols) {
#pragma unroll
        for (int q = 0; q < kFsRows; q++)
          if (q < r.nrows) __builtin_nontemporal_store((D)t[tr_at(q, lane)], d + blk + (size_t)q * np);
      }
    }
    tr_wave_sync();   // the tile is read before the next item writes it
  }
}

#ifdef CLOUDSC_LAYOUT_NAIVE
// The form without a tile (make variant VFLAGS=-DCLOUDSC_LAYOUT_NAIVE), the one the tile is measured against:
// the copy's lane-per-column walk with the LEVELS side's offset g * rows + row, a lane striding by `rows`.
template <int SB, int DB, bool TO_LEVELS>
struct NaiveItem {
  using Args = ConvTable;
  using S = typename ConvPair<SB, DB>::S;
  using D = typename ConvPair<SB, DB>::D;
  __device__ NaiveItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned np = (unsigned)(TO_LEVELS ? a.anp : a.bnp);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t blk = fs_offset(fs_pos(g, np), np, r), lev = (size_t)g * r.rows + r.row0;
    if (TO_LEVELS) conv_rows<S, D>(a.e[m].a, a.e[m].b, blk, lev, np, 1, r.nrows);
    else conv_rows<S, D>(a.e[m].a, a.e[m].b, lev, blk, 1, np, r.nrows);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};
#endif

template <int SB, int DB, bool TO_LEVELS>
void tr_launch(const ConvTable& a, dim3 grid, hipStream_t st) {
#ifdef CLOUDSC_LAYOUT_NAIVE
  hipLaunchKernelGGL((fs_kernel<NaiveItem<SB, DB, TO_LEVELS>>), grid, dim3(kFsThreads), 0, st, a);
#else
  hipLaunchKernelGGL((tr_kernel<SB, DB, TO_LEVELS>), grid, dim3(kFsThreads), 0, st, a);
#endif
}

// the element offset of (global column g, row) in a member of `rows` rows: np = 0 is the LEVELS layout
inline size_t tr_host_offset(long long g, long long row, long long rows, long long np) {
  if (!np) return (size_t)g * (size_t)rows + (size_t)row;
  const long long b = g / np;
  return (size_t)(b * rows + row) * (size_t)np + (size_t)(g - b * np);
}

// the columns [g0, g1) of one entry on the host; snp / dnp: the NPROMA of a BLOCKED side, 0 for a LEVELS side.
// The destination's inner index runs innermost.
template <typename S, typename D>
void tr_host_entry(const FsEntry<void>& e, long long g0, long long g1, long long snp, long long dnp) {
  const S* s = (const S*)e.a;
  D* d = (D*)e.b;
  if (dnp) {
    for (long long row = 0; row < e.rows; row++)
      for (long long g = g0; g < g1; g++)
        d[tr_host_offset(g, row, e.rows, dnp)] = (D)s[tr_host_offset(g, row, e.rows, snp)];
  } else {
    for (long long g = g0; g < g1; g++)
      for (long long row = 0; row < e.rows; row++)
        d[tr_host_offset(g, row, e.rows, dnp)] = (D)s[tr_host_offset(g, row, e.rows, snp)];
  }
}

template <int SB, int DB>
void tr_host_range(const ConvTable& a, long long g0, long long g1, long long snp, long long dnp) {
  for (int m = 0; m < a.n; m++) {
    if (a.int_mask >> m & 1) tr_host_entry<int, int>(a.e[m], g0, g1, snp, dnp);
    else tr_host_entry<typename ConvPair<SB, DB>::S, typename ConvPair<SB, DB>::D>(a.e[m], g0, g1, snp, dnp);
  }
}

constexpr bool layout_known(int layout) { return layout == CLOUDSC_LAYOUT_BLOCKED || layout == CLOUDSC_LAYOUT_LEVELS; }

// The argument rules of both entry points, and the NPROMA a LEVELS side has where it is walked as a blocked
// one.  Two LEVELS sets: both one block of ngptot columns, the same element positions on both sides.  One
// LEVELS set: the other side's NPROMA -- looked at for the members of one row only, which are [ngptot] in
// any blocking.
int layout_args(int ngptot, int outputs, int src_layout, int* src_nproma, int dst_layout, int* dst_nproma) {
  if (!outputs_known(outputs) || !layout_known(src_layout) || !layout_known(dst_layout)) return CLOUDSC_EINVAL;
  const bool sl = src_layout == CLOUDSC_LAYOUT_LEVELS, dl = dst_layout == CLOUDSC_LAYOUT_LEVELS;
  if ((sl && *src_nproma != 0) || (dl && *dst_nproma != 0)) return CLOUDSC_EINVAL;
  if (sl) *src_nproma = dl ? ngptot : *dst_nproma;
  if (dl) *dst_nproma = sl ? ngptot : *src_nproma;
  return CLOUDSC_OK;
}

}  // namespace

extern "C" int cloudsc_fields_convert_layout(int device, void* stream, int ngptot, int klev, int outputs,
                                             int src_precision, int src_layout, int src_nproma,
                                             const cloudsc_fields_t* src, int dst_precision, int dst_layout,
                                             int dst_nproma, const cloudsc_fields_t* dst) {
  int rc = layout_args(ngptot, outputs, src_layout, &src_nproma, dst_layout, &dst_nproma);
  if (rc) return rc;
  if (src_layout == dst_layout)   // the same element positions as two blocked sets
    return cloudsc_fields_convert_outputs(device, stream, ngptot, klev, outputs, src_precision, src_nproma, src,
                                          dst_precision, dst_nproma, dst);
  ConvTable all = {}, a = {};
  int member[kFsMaxEntries], ncu = 0;
  rc = fs_build(ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, &all, member, outputs);
  if (rc) return rc;
  // the members of one row are the same array in both layouts: the copy takes them; the others are transposed
  cloudsc_fields_t src1 = {}, dst1 = {};
  int n1 = 0;
  for (int i = 0; i < all.n; i++) {
    if (all.e[i].rows == 1) {
      ((const void**)&src1)[member[i]] = all.e[i].a;
      ((void**)&dst1)[member[i]] = all.e[i].b;
      n1++;
    } else {
      a.e[a.n++] = all.e[i];
    }
  }
  fs_shape(&a, ngptot, src_nproma, dst_nproma);
  if ((rc = fs_device(device, &ncu))) return rc;
  if (n1 && (rc = cloudsc_fields_convert_outputs(device, stream, ngptot, klev, outputs, src_precision, src_nproma,
                                                 &src1, dst_precision, dst_nproma, &dst1)))
    return rc;
  if (!a.n) return CLOUDSC_OK;
  HIPCHK(hipSetDevice(device));
  const dim3 grid(fs_grid(a, ncu));
  hipStream_t st = (hipStream_t)stream;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  if (dst_layout == CLOUDSC_LAYOUT_LEVELS) {
    if (s8 && d8) tr_launch<8, 8, true>(a, grid, st);
    else if (s8) tr_launch<8, 4, true>(a, grid, st);
    else if (d8) tr_launch<4, 8, true>(a, grid, st);
    else tr_launch<4, 4, true>(a, grid, st);
  } else {
    if (s8 && d8) tr_launch<8, 8, false>(a, grid, st);
    else if (s8) tr_launch<8, 4, false>(a, grid, st);
    else if (d8) tr_launch<4, 8, false>(a, grid, st);
    else tr_launch<4, 4, false>(a, grid, st);
  }
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

#ifndef CLOUDSC_LAYOUT_NAIVE
extern "C" int cloudsc_debug_layout_kernel_resources(int device, int which, int* scratch_bytes, int* lds_bytes) {
  static const void* const kernels[8] = {
      (const void*)tr_kernel<8, 8, true>,  (const void*)tr_kernel<8, 4, true>,  (const void*)tr_kernel<4, 8, true>,
      (const void*)tr_kernel<4, 4, true>,  (const void*)tr_kernel<8, 8, false>, (const void*)tr_kernel<8, 4, false>,
      (const void*)tr_kernel<4, 8, false>, (const void*)tr_kernel<4, 4, false>};
  int ncu = 0;
  if (which < 0 || which >= 8 || !scratch_bytes || !lds_bytes) return CLOUDSC_EINVAL;
  const int rc = fs_device(device, &ncu);
  if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  hipFuncAttributes at;
  HIPCHK(hipFuncGetAttributes(&at, kernels[which]));
  *scratch_bytes = (int)at.localSizeBytes;
  *lds_bytes = (int)at.sharedSizeBytes;
  return CLOUDSC_OK;
}
#endif

extern "C" int cloudsc_cpu_fields_convert_layout(int nthreads, int ngptot, int klev, int outputs, int src_precision,
                                                 int src_layout, int src_nproma, const cloudsc_fields_t* src,
                                                 int dst_precision, int dst_layout, int dst_nproma,
                                                 const cloudsc_fields_t* dst) {
  int rc = layout_args(ngptot, outputs, src_layout, &src_nproma, dst_layout, &dst_nproma);
  if (rc) return rc;
  if (src_layout == dst_layout)
    return cpu_convert(nthreads, ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, outputs);
  ConvTable a = {};
  rc = fs_build(ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, &a, nullptr, outputs);
  if (rc) return rc;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  void (*range)(const ConvTable&, long long, long long, long long, long long) =
      s8 && d8 ? tr_host_range<8, 8> : s8 ? tr_host_range<8, 4> : d8 ? tr_host_range<4, 8> : tr_host_range<4, 4>;
  // destination blocks (BLOCKED), or ranges of a tile's columns (LEVELS)
  const bool to_levels = dst_layout == CLOUDSC_LAYOUT_LEVELS;
  const long long per = to_levels ? kFsThreads : dst_nproma;
  const long long snp = to_levels ? src_nproma : 0, dnp = to_levels ? 0 : dst_nproma;
  fs_run_blocks(nthreads, ((long long)ngptot + per - 1) / per, [&](int, long long b) {
    range(a, b * per, std::min<long long>((b + 1) * per, ngptot), snp, dnp);
  });
  return CLOUDSC_OK;
}
