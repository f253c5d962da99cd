// cloudsc_convert.hip -- copy a field set into another NPROMA blocking and / or
// storage type: cloudsc_fields_convert on the device (one streaming kernel,
// stream-ordered), cloudsc_cpu_fields_convert on the host.
//
// For every member set in both field sets, every row r of its kind and every
// global column g < ngptot:
//
//   dst[g / dnp][r][g % dnp] = (dst type) src[g / snp][r][g % snp]
//
// The kernel.  One launch per call: the members travel as a table of {src, dst,
// rows} entries in the kernel arguments, generated from cloudsc_fields.def
// through kFieldTable.  A work item is (member, tile of 256 consecutive global
// columns, chunk of 16 rows); a grid of at most eight workgroups per compute
// unit strides the items, a member's items in (tile, chunk) order with the
// chunk running fastest, so the workgroups in flight together sweep
// neighbouring rows of the same blocks.  Lane t of a workgroup owns column
// tile * 256 + t: it divides once per item to find its source and destination
// block and lane (32-bit divisions: g < 2^31), then walks the rows by adding
// the two NPROMAs, eight loads in flight before their eight stores.  Consecutive
// lanes hold consecutive columns, so a wave's 64 stores to a destination row
// are one run of 64 elements when dst NPROMA is a multiple of 64 and runs of
// min(dst NPROMA, 64) otherwise, and its loads are runs of min(src NPROMA, 64).
// Every element offset is 64-bit (one fp64 species field at 163840 columns is
// 0.9 GB).  Loads and stores are plain non-temporal vector accesses: each byte
// is touched once.  Lanes past ngptot do nothing, so the padding lanes of the
// destination's last block keep their contents.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "cloudsc_internal.h"

using namespace cloudsc_impl;

namespace {

constexpr int kConvMaxEntries = 48;   // the table's capacity (about 1 KiB of kernel arguments)
static_assert(kNumFields <= kConvMaxEntries, "the conversion table holds every cloudsc_fields_t member");
static_assert(kNumFields <= 64, "ConvArgs::int_mask has one bit per member");
constexpr int kConvThreads = 256;     // columns per tile = threads per workgroup
constexpr int kConvRows = 16;         // rows per item
constexpr int kConvBatch = 8;         // loads a lane has in flight
constexpr int kConvMaxNproma = 1 << 24;

struct ConvEntry {
  const void* src;
  void* dst;
  long long rows;   // klev | klev + 1 | NCLV * klev | 1
};
struct ConvArgs {
  ConvEntry e[kConvMaxEntries];
  unsigned long long int_mask;   // bit i: entry i is int32 (ktype), copied as it is
  int n, ngptot, snp, dnp;
  unsigned ntiles;               // ceil(ngptot / kConvThreads)
};

// the element type of a storage size; a copy between equal sizes moves bits
template <int BYTES> struct ConvReal { using type = double; using bits = unsigned long long; };
template <> struct ConvReal<4> { using type = float; using bits = unsigned; };

// nrows rows of one column: src + so, dst + doff address the first row, the row strides are the NPROMAs
template <typename S, typename D>
__device__ __forceinline__ void conv_rows(const void* src, void* dst, size_t so, size_t doff, size_t snp, size_t dnp,
                                          int nrows) {
  const S* __restrict__ s = (const S*)src + so;
  D* __restrict__ d = (D*)dst + doff;
  for (int r = 0; r < nrows; r += kConvBatch) {
    S v[kConvBatch];
#pragma unroll
    for (int q = 0; q < kConvBatch; q++)
      if (r + q < nrows) v[q] = __builtin_nontemporal_load(s + (size_t)(r + q) * snp);
#pragma unroll
    for (int q = 0; q < kConvBatch; q++)
      if (r + q < nrows) __builtin_nontemporal_store((D)v[q], d + (size_t)(r + q) * dnp);
  }
}

template <int SB, int DB>
__global__ void __launch_bounds__(kConvThreads) fields_convert_kernel(const ConvArgs a) {
  using S = typename std::conditional<SB == DB, typename ConvReal<SB>::bits, typename ConvReal<SB>::type>::type;
  using D = typename std::conditional<SB == DB, typename ConvReal<DB>::bits, typename ConvReal<DB>::type>::type;
  int m = 0;
  unsigned long long first = 0;   // the first item of member m
  unsigned long long nchunk = (unsigned long long)(a.e[0].rows + kConvRows - 1) / kConvRows;
  unsigned long long count = nchunk * a.ntiles;
  for (unsigned long long it = blockIdx.x;; it += gridDim.x) {
    while (it >= first + count) {
      first += count;
      if (++m >= a.n) return;
      nchunk = (unsigned long long)(a.e[m].rows + kConvRows - 1) / kConvRows;
      count = nchunk * a.ntiles;
    }
    const unsigned long long local = it - first, tile = local / nchunk, chunk = local - tile * nchunk;
    const unsigned long long g64 = tile * kConvThreads + threadIdx.x;
    if (g64 >= (unsigned long long)a.ngptot) continue;
    const unsigned g = (unsigned)g64, snp = (unsigned)a.snp, dnp = (unsigned)a.dnp;
    const unsigned sb = g / snp, sj = g - sb * snp, db = g / dnp, dj = g - db * dnp;
    const size_t rows = (size_t)a.e[m].rows, row0 = (size_t)chunk * kConvRows;
    const int nrows = (int)std::min<size_t>(kConvRows, rows - row0);
    const size_t so = ((size_t)sb * rows + row0) * snp + sj, doff = ((size_t)db * rows + row0) * dnp + dj;
    if (a.int_mask >> m & 1) conv_rows<int, int>(a.e[m].src, a.e[m].dst, so, doff, snp, dnp, nrows);
    else conv_rows<S, D>(a.e[m].src, a.e[m].dst, so, doff, snp, dnp, nrows);
  }
}

// the argument rules of both entry points, and the table; no HIP call
int conv_build(int ngptot, int klev, int src_precision, int src_nproma, const cloudsc_fields_t* src,
               int dst_precision, int dst_nproma, const cloudsc_fields_t* dst, ConvArgs* a) {
  if (!src || !dst) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(src_precision) || !precision_storage_bytes(dst_precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || src_nproma < 1 || dst_nproma < 1) return CLOUDSC_EINVAL;
  if (src_nproma > kConvMaxNproma || dst_nproma > kConvMaxNproma) return CLOUDSC_EINVAL;
  std::memset(a, 0, sizeof(*a));
  for (int m = 0; m < kNumFields; m++) {
    const void* s = ((const void* const*)src)[m];
    void* d = ((void* const*)dst)[m];   // dst's input members are const void * in the struct and written here
    if (!s && !d) continue;
    if (!s || !d || s == d) return CLOUDSC_EINVAL;
    ConvEntry& e = a->e[a->n];
    e.src = s;
    e.dst = d;
    e.rows = (long long)(per_block_elems(kFieldTable[m].kind, 1, klev));
    if (kFieldTable[m].is_int) a->int_mask |= 1ull << a->n;
    a->n++;
  }
  if (!a->n) return CLOUDSC_EINVAL;
  a->ngptot = ngptot;
  a->snp = src_nproma;
  a->dnp = dst_nproma;
  a->ntiles = (unsigned)(((long long)ngptot + kConvThreads - 1) / kConvThreads);
  return CLOUDSC_OK;
}

// the columns of destination block db, on the host: the kernel's index arithmetic in plain loops, a run
// of columns that stays inside one source block at a time
template <typename S, typename D>
void conv_block_entry(const ConvEntry& e, const ConvArgs& a, long long db) {
  const long long snp = a.snp, dnp = a.dnp, g0 = db * dnp;
  const long long bsize = std::min<long long>(dnp, a.ngptot - g0);
  const S* s = (const S*)e.src;
  D* d = (D*)e.dst;
  for (long long row = 0; row < e.rows; row++) {
    D* drow = d + (size_t)(db * e.rows + row) * (size_t)dnp;
    for (long long jl = 0; jl < bsize;) {
      const long long g = g0 + jl, sb = g / snp, sj = g - sb * snp;
      const long long run = std::min(bsize - jl, snp - sj);
      const S* srow = s + (size_t)(sb * e.rows + row) * (size_t)snp + sj;
      for (long long i = 0; i < run; i++) drow[jl + i] = (D)srow[i];
      jl += run;
    }
  }
}

template <int SB, int DB>
void conv_block(const ConvArgs& a, long long db) {
  using S = typename std::conditional<SB == DB, typename ConvReal<SB>::bits, typename ConvReal<SB>::type>::type;
  using D = typename std::conditional<SB == DB, typename ConvReal<DB>::bits, typename ConvReal<DB>::type>::type;
  for (int m = 0; m < a.n; m++) {
    if (a.int_mask >> m & 1) conv_block_entry<int, int>(a.e[m], a, db);
    else conv_block_entry<S, D>(a.e[m], a, db);
  }
}

std::atomic<int> g_conv_ncu[kMaxDevices];   // compute units per device, 0 = not asked yet

}  // namespace

extern "C" int cloudsc_fields_convert(int device, void* stream, int ngptot, int klev, int src_precision,
                                      int src_nproma, const cloudsc_fields_t* src, int dst_precision,
                                      int dst_nproma, const cloudsc_fields_t* dst) {
  ConvArgs a;
  int rc = conv_build(ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, &a);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CLOUDSC_ENODEV; }
  if (device < 0 || device >= ndev || device >= kMaxDevices) return CLOUDSC_ENODEV;
  HIPCHK(hipSetDevice(device));
  int ncu = g_conv_ncu[device].load(std::memory_order_relaxed);
  if (!ncu) {
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) {
      (void)hipGetLastError();
      ncu = 256;
    }
    g_conv_ncu[device].store(ncu, std::memory_order_relaxed);
  }
  unsigned long long items = 0;
  for (int m = 0; m < a.n; m++) items += (unsigned long long)((a.e[m].rows + kConvRows - 1) / kConvRows) * a.ntiles;
  // eight workgroups of four waves per compute unit: every wave slot of the device
  const dim3 grid((unsigned)std::min<unsigned long long>(items, (unsigned long long)ncu * 8)), wg(kConvThreads);
  hipStream_t st = (hipStream_t)stream;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  if (s8 && d8) hipLaunchKernelGGL((fields_convert_kernel<8, 8>), grid, wg, 0, st, a);
  else if (s8) hipLaunchKernelGGL((fields_convert_kernel<8, 4>), grid, wg, 0, st, a);
  else if (d8) hipLaunchKernelGGL((fields_convert_kernel<4, 8>), grid, wg, 0, st, a);
  else hipLaunchKernelGGL((fields_convert_kernel<4, 4>), grid, wg, 0, st, a);
  HIPCHK(hipGetLastError());
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_convert(int nthreads, int ngptot, int klev, int src_precision, int src_nproma,
                                          const cloudsc_fields_t* src, int dst_precision, int dst_nproma,
                                          const cloudsc_fields_t* dst) {
  ConvArgs a;
  int rc = conv_build(ngptot, klev, src_precision, src_nproma, src, dst_precision, dst_nproma, dst, &a);
  if (rc) return rc;
  const bool s8 = precision_storage_bytes(src_precision) == 8, d8 = precision_storage_bytes(dst_precision) == 8;
  void (*block)(const ConvArgs&, long long) =
      s8 && d8 ? conv_block<8, 8> : s8 ? conv_block<8, 4> : d8 ? conv_block<4, 8> : conv_block<4, 4>;
  const long long nblocks = ((long long)ngptot + dst_nproma - 1) / dst_nproma;
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  nthreads = (int)std::min<long long>(nthreads, nblocks);
  std::atomic<long long> next{0};
  auto worker = [&]() {
    for (long long b = next.fetch_add(1); b < nblocks; b = next.fetch_add(1)) block(a, b);
  };
  if (nthreads == 1) {
    worker();
  } else {
    std::vector<std::thread> pool;
    pool.reserve((size_t)nthreads);
    try {
      for (int t = 1; t < nthreads; t++) pool.emplace_back(worker);
    } catch (...) {
      // fewer threads than asked for: every block is still taken, by them and by the caller
    }
    worker();
    for (auto& t : pool) t.join();
  }
  return CLOUDSC_OK;
}
