// cloudsc_compare.hip -- judge and fill caller-owned field sets on the device:
// cloudsc_fields_compare (two field sets in any two NPROMA blockings and storage
// types), cloudsc_fields_validate (a set against a KLON-column reference),
// cloudsc_fields_expand (a set filled from the KLON-column template) and the host
// twin cloudsc_cpu_fields_compare.
//
// For every member set in both field sets, every row r of its kind and every
// global column g < ngptot, with v = a[g / anp][r][g % anp] and
// r = b[g / bnp][r][g % bnp] widened to double (exact):
//
//   d = |v - r|;  min v, max v, max d;  sum d and sum |r| as double-doubles;
//   the number of elements whose bits differ and the smallest g * rows + r of them
//
// The kernel.  The item scheme of cloudsc_convert.hip: the members travel as a
// table of {a, b, rows} entries in the kernel arguments (kFieldTable), a work item
// is (member, tile of 256 consecutive global columns, chunk of 16 rows), a grid of
// at most eight workgroups per compute unit strides the items.  Lane t owns column
// tile * 256 + t, divides once per item for its block and lane in each set's own
// NPROMA and walks the rows with eight non-temporal loads per operand in flight;
// there is no store in the streaming part.  Each lane keeps one record (nine
// 64-bit accumulators); when a workgroup's item sequence leaves a member the
// record is reduced over the workgroup (cross-lane shuffles, then four records
// through LDS) and written as that workgroup's partial of the member, a neutral
// one if it had no item there.  A second kernel, one wave per member, combines
// the partials of a member in workgroup order.  No atomics.  min, max, max d, the
// count and the first key are exact whatever the grid and the blockings; the two
// sums depend on the grouping within the double-double bound of cloudsc_stats_t.
// Every element offset and every key is 64-bit.  Lanes past ngptot contribute
// nothing, so padding lanes are never read.
//
// cloudsc_fields_validate is the same kernel with the b operand a double array
// [rows][klon] read at column (col_offset + g) % klon through the caches (the
// reference is small and every tile reads all of it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "cloudsc_internal.h"

using namespace cloudsc_impl;

namespace {

constexpr int kCmpMaxEntries = 48;    // the table's capacity (about 1 KiB of kernel arguments)
static_assert(kNumFields <= kCmpMaxEntries, "the comparison table holds every cloudsc_fields_t member");
static_assert(kNumFields <= 64, "CmpArgs::int_mask has one bit per member");
constexpr int kCmpThreads = 256;      // columns per tile = threads per workgroup
constexpr int kCmpRows = 16;          // rows per item
constexpr int kCmpBatch = 8;          // loads per operand a lane has in flight
constexpr int kCmpMaxNproma = 1 << 24;
constexpr int kCmpMaxGrid = 1 << 16;  // cloudsc_debug_set_compare_grid
constexpr unsigned long long kNoKey = ~0ull;

// One record: a lane's accumulators, a workgroup's partial of a member, a member's result
struct CmpRec {
  double mn, mx, me;                  // min v, max v, max d
  double es_hi, es_lo, rs_hi, rs_lo;  // sum d, sum |r|
  long long mism;                     // elements that differ as bits
  unsigned long long first;           // smallest g * rows + row among them, kNoKey if none
};
__host__ __device__ __forceinline__ CmpRec cmp_neutral() {
  return {__DBL_MAX__, -__DBL_MAX__, 0.0, 0.0, 0.0, 0.0, 0.0, 0, kNoKey};
}
__host__ __device__ __forceinline__ void cmp_combine(CmpRec& c, const CmpRec& p) {
  c.mn = fmin(c.mn, p.mn);
  c.mx = fmax(c.mx, p.mx);
  c.me = fmax(c.me, p.me);
  const DD e = dd_add(DD{c.es_hi, c.es_lo}, DD{p.es_hi, p.es_lo});
  const DD r = dd_add(DD{c.rs_hi, c.rs_lo}, DD{p.rs_hi, p.rs_lo});
  c.es_hi = e.hi; c.es_lo = e.lo; c.rs_hi = r.hi; c.rs_lo = r.lo;
  c.mism += p.mism;
  c.first = p.first < c.first ? p.first : c.first;
}

// How an element is held: the word that is loaded and compared, and its value as a double.
// nt: read once (non-temporal); the reference of a validation is read through the caches.
struct W8 {
  using word = unsigned long long;
  static constexpr bool nt = true;
  static __host__ __device__ __forceinline__ double val(word w) { return __builtin_bit_cast(double, w); }
};
struct W8Ref : W8 { static constexpr bool nt = false; };
struct W4 {
  using word = unsigned;
  static constexpr bool nt = true;
  static __host__ __device__ __forceinline__ double val(word w) { return (double)__builtin_bit_cast(float, w); }
};
struct WInt {   // ktype
  using word = unsigned;
  static constexpr bool nt = true;
  static __host__ __device__ __forceinline__ double val(word w) { return (double)(int)w; }
};
template <int BYTES> struct CmpReal { using type = W8; };
template <> struct CmpReal<4> { using type = W4; };

template <typename A, typename B>
__host__ __device__ __forceinline__ void cmp_elem(typename A::word wa, typename B::word wb, unsigned long long key,
                                                  CmpRec& c) {
  const double v = A::val(wa), r = B::val(wb), d = fabs(v - r);
  c.mn = fmin(c.mn, v);
  c.mx = fmax(c.mx, v);
  c.me = fmax(c.me, d);
  const DD e = dd_add(DD{c.es_hi, c.es_lo}, DD{d, 0.0});
  const DD s = dd_add(DD{c.rs_hi, c.rs_lo}, DD{fabs(r), 0.0});
  c.es_hi = e.hi; c.es_lo = e.lo; c.rs_hi = s.hi; c.rs_lo = s.lo;
  bool differ;
  if constexpr (sizeof(typename A::word) == sizeof(typename B::word)) differ = wa != wb;   // the raw words
  else differ = __builtin_bit_cast(unsigned long long, v) != __builtin_bit_cast(unsigned long long, r);
  if (differ) {
    c.mism++;
    c.first = key < c.first ? key : c.first;
  }
}

struct CmpEntry {
  const void* a;
  const void* b;    // the second set's member, or (validate) the member's reference [rows][klon] on the device
  long long rows;   // klev | klev + 1 | NCLV * klev | 1
};
struct CmpArgs {
  CmpEntry e[kCmpMaxEntries];
  unsigned long long int_mask;   // bit i: entry i is int32 (ktype)
  int n, ngptot, anp, bnp;
  unsigned ntiles;               // ceil(ngptot / kCmpThreads)
  int klon;                      // validate: columns of the reference
  long long col_offset;          // validate: the global column of column 0
  CmpRec* part;                  // [workgroups][n]
};

// nrows rows of one column: x + ao, y + bo address the first row, as / bs are the row strides
template <typename A, typename B>
__device__ __forceinline__ void cmp_rows(const void* pa, const void* pb, size_t ao, size_t bo, size_t as, size_t bs,
                                         int nrows, unsigned long long key0, CmpRec& acc) {
  const typename A::word* __restrict__ x = (const typename A::word*)pa + ao;
  const typename B::word* __restrict__ y = (const typename B::word*)pb + bo;
  for (int r = 0; r < nrows; r += kCmpBatch) {
    typename A::word wa[kCmpBatch];
    typename B::word wb[kCmpBatch];
#pragma unroll
    for (int q = 0; q < kCmpBatch; q++)
      if (r + q < nrows) {
        wa[q] = __builtin_nontemporal_load(x + (size_t)(r + q) * as);
        if constexpr (B::nt) wb[q] = __builtin_nontemporal_load(y + (size_t)(r + q) * bs);
        else wb[q] = y[(size_t)(r + q) * bs];
      }
#pragma unroll
    for (int q = 0; q < kCmpBatch; q++)
      if (r + q < nrows) cmp_elem<A, B>(wa[q], wb[q], key0 + (unsigned long long)(r + q), acc);
  }
}

// the workgroup's record of one member: shuffles within a wave, the waves' records through LDS;
// every thread of the workgroup calls it (touched is uniform), acc comes back neutral
__device__ __forceinline__ void cmp_flush(CmpRec* out, CmpRec& acc, bool touched) {
  if (!touched) {   // no item of this member: acc is still neutral
    if (threadIdx.x == 0) *out = cmp_neutral();
    return;
  }
  for (int off = warpSize / 2; off > 0; off >>= 1) {
    CmpRec p;
    p.mn = __shfl_down(acc.mn, off);
    p.mx = __shfl_down(acc.mx, off);
    p.me = __shfl_down(acc.me, off);
    p.es_hi = __shfl_down(acc.es_hi, off);
    p.es_lo = __shfl_down(acc.es_lo, off);
    p.rs_hi = __shfl_down(acc.rs_hi, off);
    p.rs_lo = __shfl_down(acc.rs_lo, off);
    p.mism = __shfl_down(acc.mism, off);
    p.first = __shfl_down(acc.first, off);
    cmp_combine(acc, p);   // lanes whose partner is past the wave combine with themselves: only lane 0 is used
  }
  __shared__ CmpRec s[kCmpThreads / 64];
  const int wave = threadIdx.x / warpSize;
  if (threadIdx.x % warpSize == 0) s[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    CmpRec t = s[0];
    for (int w = 1; w < kCmpThreads / warpSize; w++) cmp_combine(t, s[w]);
    *out = t;
  }
  __syncthreads();   // s is written again at the next member
  acc = cmp_neutral();
}

// AB, BB: bytes of a real element of a and b; REF: b is the reference of a validation (double, [rows][klon])
template <int AB, int BB, bool REF>
__global__ void __launch_bounds__(kCmpThreads) fields_compare_kernel(const CmpArgs a) {
  using A = typename CmpReal<AB>::type;
  using B = typename std::conditional<REF, W8Ref, typename CmpReal<BB>::type>::type;
  CmpRec acc = cmp_neutral();
  bool touched = false;
  int m = 0;
  unsigned long long first = 0;   // the first item of member m
  unsigned long long nchunk = (unsigned long long)(a.e[0].rows + kCmpRows - 1) / kCmpRows;
  unsigned long long count = nchunk * a.ntiles;
  CmpRec* part = a.part + (size_t)blockIdx.x * a.n;
  for (unsigned long long it = blockIdx.x;; it += gridDim.x) {   // `it` is the same in every thread of the workgroup
    while (it >= first + count) {
      cmp_flush(part + m, acc, touched);
      touched = false;
      first += count;
      if (++m >= a.n) return;
      nchunk = (unsigned long long)(a.e[m].rows + kCmpRows - 1) / kCmpRows;
      count = nchunk * a.ntiles;
    }
    touched = true;
    const unsigned long long local = it - first, tile = local / nchunk, chunk = local - tile * nchunk;
    const unsigned long long g64 = tile * kCmpThreads + threadIdx.x;
    if (g64 < (unsigned long long)a.ngptot) {
      const unsigned g = (unsigned)g64, anp = (unsigned)a.anp;
      const unsigned ab = g / anp, aj = g - ab * anp;
      const size_t rows = (size_t)a.e[m].rows, row0 = (size_t)chunk * kCmpRows;
      const int nrows = (int)std::min<size_t>(kCmpRows, rows - row0);
      const size_t ao = ((size_t)ab * rows + row0) * anp + aj;
      size_t bo, bs;
      if constexpr (REF) {
        bs = (size_t)a.klon;
        bo = row0 * bs + (size_t)((a.col_offset + (long long)g) % a.klon);
      } else {
        const unsigned bnp = (unsigned)a.bnp, bb = g / bnp, bj = g - bb * bnp;
        bs = bnp;
        bo = ((size_t)bb * rows + row0) * bnp + bj;
      }
      const unsigned long long key0 = (unsigned long long)g * rows + row0;
      if (!REF && (a.int_mask >> m & 1)) cmp_rows<WInt, WInt>(a.e[m].a, a.e[m].b, ao, bo, anp, bs, nrows, key0, acc);
      else cmp_rows<A, B>(a.e[m].a, a.e[m].b, ao, bo, anp, bs, nrows, key0, acc);
    }
  }
}

// one wave per member: the partials of the member in workgroup order (lane l takes workgroups l, l + 64, ...,
// then the lanes combine in a fixed tree)
__global__ void __launch_bounds__(64) fields_compare_combine_kernel(const CmpRec* __restrict__ part, int nwg, int n,
                                                                    CmpRec* __restrict__ res) {
  const int m = blockIdx.x;
  CmpRec acc = cmp_neutral();
  for (int w = threadIdx.x; w < nwg; w += 64) cmp_combine(acc, part[(size_t)w * n + m]);
  for (int off = 32; off > 0; off >>= 1) {
    CmpRec p;
    p.mn = __shfl_down(acc.mn, off);
    p.mx = __shfl_down(acc.mx, off);
    p.me = __shfl_down(acc.me, off);
    p.es_hi = __shfl_down(acc.es_hi, off);
    p.es_lo = __shfl_down(acc.es_lo, off);
    p.rs_hi = __shfl_down(acc.rs_hi, off);
    p.rs_lo = __shfl_down(acc.rs_lo, off);
    p.mism = __shfl_down(acc.mism, off);
    p.first = __shfl_down(acc.first, off);
    cmp_combine(acc, p);
  }
  if (threadIdx.x == 0) res[m] = acc;
}

// Template expansion into a caller-owned set, the same item scheme: dst[g / np][row][g % np] =
// (T) src[row][(col_offset + g) % klon] for g < ngptot (padding lanes are not written); src is the staged
// template on the device (double, ktype int)
struct ExpEntry {
  const void* src;
  void* dst;
  long long rows;
};
struct ExpArgs {
  ExpEntry e[kCmpMaxEntries];
  unsigned long long int_mask;
  int n, ngptot, np, klon;
  unsigned ntiles;
  long long col_offset;
};
template <typename S, typename D>
__device__ __forceinline__ void exp_rows(const void* src, void* dst, size_t so, size_t doff, size_t klon, size_t np,
                                         int nrows) {
  const S* __restrict__ s = (const S*)src + so;
  D* __restrict__ d = (D*)dst + doff;
  for (int r = 0; r < nrows; r++) __builtin_nontemporal_store((D)s[(size_t)r * klon], d + (size_t)r * np);
}
template <typename D>
__global__ void __launch_bounds__(kCmpThreads) fields_expand_kernel(const ExpArgs a) {
  int m = 0;
  unsigned long long first = 0;
  unsigned long long nchunk = (unsigned long long)(a.e[0].rows + kCmpRows - 1) / kCmpRows;
  unsigned long long count = nchunk * a.ntiles;
  for (unsigned long long it = blockIdx.x;; it += gridDim.x) {
    while (it >= first + count) {
      first += count;
      if (++m >= a.n) return;
      nchunk = (unsigned long long)(a.e[m].rows + kCmpRows - 1) / kCmpRows;
      count = nchunk * a.ntiles;
    }
    const unsigned long long local = it - first, tile = local / nchunk, chunk = local - tile * nchunk;
    const unsigned long long g64 = tile * kCmpThreads + threadIdx.x;
    if (g64 >= (unsigned long long)a.ngptot) continue;
    const unsigned g = (unsigned)g64, np = (unsigned)a.np, b = g / np, j = g - b * np;
    const size_t rows = (size_t)a.e[m].rows, row0 = (size_t)chunk * kCmpRows;
    const int nrows = (int)std::min<size_t>(kCmpRows, rows - row0);
    const size_t so = row0 * (size_t)a.klon + (size_t)((a.col_offset + (long long)g) % a.klon);
    const size_t doff = ((size_t)b * rows + row0) * np + j;
    if (a.int_mask >> m & 1) exp_rows<int, int>(a.e[m].src, a.e[m].dst, so, doff, (size_t)a.klon, np, nrows);
    else exp_rows<double, D>(a.e[m].src, a.e[m].dst, so, doff, (size_t)a.klon, np, nrows);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
long long member_rows(int m, int klev) { return (long long)per_block_elems(kFieldTable[m].kind, 1, klev); }

void diff_skipped(cloudsc_field_diff_t* d) {
  d->stats = {__DBL_MAX__, -__DBL_MAX__, 0.0, 0.0, 0.0, 0.0, 0.0};
  d->compared = 0;
  d->mismatches = 0;
  d->first_column = d->first_row = -1;
}
cloudsc_stats_t rec_stats(const CmpRec& r) { return {r.mn, r.mx, r.me, r.es_hi, r.rs_hi, r.es_lo, r.rs_lo}; }
void diff_from(cloudsc_field_diff_t* d, const CmpRec& r, long long rows, int ngptot) {
  d->stats = rec_stats(r);
  d->compared = rows * ngptot;
  d->mismatches = r.mism;
  d->first_column = r.first == kNoKey ? -1 : (long long)(r.first / (unsigned long long)rows);
  d->first_row = r.first == kNoKey ? -1 : (long long)(r.first % (unsigned long long)rows);
}

// the argument rules of both comparisons and the table; member[i] = the cloudsc_fields_t position of entry i;
// no HIP call
int cmp_build(int ngptot, int klev, int a_precision, int a_nproma, const cloudsc_fields_t* fa, int b_precision,
              int b_nproma, const cloudsc_fields_t* fb, const cloudsc_field_diff_t* diff, CmpArgs* a, int* member) {
  if (!fa || !fb || !diff) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(a_precision) || !precision_storage_bytes(b_precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || a_nproma < 1 || b_nproma < 1) return CLOUDSC_EINVAL;
  if (a_nproma > kCmpMaxNproma || b_nproma > kCmpMaxNproma) return CLOUDSC_EINVAL;
  std::memset(a, 0, sizeof(*a));
  for (int m = 0; m < kNumFields; m++) {
    const void* pa = ((const void* const*)fa)[m];
    const void* pb = ((const void* const*)fb)[m];
    if (!pa && !pb) continue;
    if (!pa || !pb) return CLOUDSC_EINVAL;
    CmpEntry& e = a->e[a->n];
    e.a = pa;
    e.b = pb;
    e.rows = member_rows(m, klev);
    if (kFieldTable[m].is_int) a->int_mask |= 1ull << a->n;
    member[a->n++] = m;
  }
  if (!a->n) return CLOUDSC_EINVAL;
  a->ngptot = ngptot;
  a->anp = a_nproma;
  a->bnp = b_nproma;
  a->ntiles = (unsigned)(((long long)ngptot + kCmpThreads - 1) / kCmpThreads);
  return CLOUDSC_OK;
}

// the columns of block ab of set a, on the host: the kernel's index arithmetic in plain loops, a run of
// columns that stays inside one block of b at a time
template <typename A, typename B>
void cmp_block_entry(const CmpEntry& e, const CmpArgs& a, long long ab, CmpRec& acc) {
  const long long anp = a.anp, bnp = a.bnp, g0 = ab * anp;
  const long long bsize = std::min<long long>(anp, a.ngptot - g0);
  const typename A::word* x = (const typename A::word*)e.a;
  const typename B::word* y = (const typename B::word*)e.b;
  for (long long row = 0; row < e.rows; row++) {
    const typename A::word* xrow = x + (size_t)(ab * e.rows + row) * (size_t)anp;
    for (long long jl = 0; jl < bsize;) {
      const long long g = g0 + jl, bb = g / bnp, bj = g - bb * bnp;
      const long long run = std::min(bsize - jl, bnp - bj);
      const typename B::word* yrow = y + (size_t)(bb * e.rows + row) * (size_t)bnp + bj;
      for (long long i = 0; i < run; i++)
        cmp_elem<A, B>(xrow[jl + i], yrow[i], (unsigned long long)(g + i) * (unsigned long long)e.rows + row, acc);
      jl += run;
    }
  }
}
template <int AB, int BB>
void cmp_block(const CmpArgs& a, long long ab, CmpRec* acc) {
  using A = typename CmpReal<AB>::type;
  using B = typename CmpReal<BB>::type;
  for (int m = 0; m < a.n; m++) {
    if (a.int_mask >> m & 1) cmp_block_entry<WInt, WInt>(a.e[m], a, ab, acc[m]);
    else cmp_block_entry<A, B>(a.e[m], a, ab, acc[m]);
  }
}

// Per-device workspace of the device entry points: the workgroups' partials, the members' results (device and
// pinned host), the uploaded reference or template, and the event of the last expansion still using them.
// Grows on demand (a growth frees and allocates: the only device-wide synchronisation after the first call).
struct CmpWorkspace {
  std::mutex mu;
  int ncu = 0;
  CmpRec* part = nullptr;
  size_t part_cap = 0;          // records
  CmpRec* res = nullptr;        // [kCmpMaxEntries], device
  CmpRec* hres = nullptr;       // [kCmpMaxEntries], pinned host
  char* stage = nullptr;        // device: the reference (validate) or the template (expand)
  char* hstage = nullptr;       // pinned host: the template of an expansion, copied from the caller's arrays
  size_t stage_cap = 0, hstage_cap = 0;
  hipEvent_t busy = nullptr;    // recorded after an expansion's last kernel
  bool pending = false;
};
CmpWorkspace g_ws[kMaxDevices];
std::atomic<int> g_cmp_grid{0};   // cloudsc_debug_set_compare_grid

int ws_device(int device, CmpWorkspace** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CLOUDSC_ENODEV; }
  if (device < 0 || device >= ndev || device >= kMaxDevices) return CLOUDSC_ENODEV;
  *out = &g_ws[device];
  return CLOUDSC_OK;
}

// with ws.mu held and the device current: the fixed buffers, and no earlier expansion still reading the stage
int ws_ready(CmpWorkspace& ws, int device) {
  if (!ws.ncu) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) {
      (void)hipGetLastError();
      ncu = 256;
    }
    ws.ncu = ncu;
  }
  if (!ws.res) HIPCHK(hipMalloc((void**)&ws.res, kCmpMaxEntries * sizeof(CmpRec)));
  if (!ws.hres) HIPCHK(hipHostMalloc((void**)&ws.hres, kCmpMaxEntries * sizeof(CmpRec), hipHostMallocDefault));
  if (!ws.busy) HIPCHK(hipEventCreateWithFlags(&ws.busy, hipEventDisableTiming));
  if (ws.pending) {
    HIPCHK(hipEventSynchronize(ws.busy));
    ws.pending = false;
  }
  return CLOUDSC_OK;
}
int ws_grow_part(CmpWorkspace& ws, size_t records) {
  if (records <= ws.part_cap) return CLOUDSC_OK;
  if (ws.part) { (void)hipFree(ws.part); ws.part = nullptr; ws.part_cap = 0; }
  HIPCHK(hipMalloc((void**)&ws.part, records * sizeof(CmpRec)));
  ws.part_cap = records;
  return CLOUDSC_OK;
}
int ws_grow_stage(CmpWorkspace& ws, size_t bytes, bool host_too) {
  if (bytes > ws.stage_cap) {
    if (ws.stage) { (void)hipFree(ws.stage); ws.stage = nullptr; ws.stage_cap = 0; }
    HIPCHK(hipMalloc((void**)&ws.stage, bytes));
    ws.stage_cap = bytes;
  }
  if (host_too && bytes > ws.hstage_cap) {
    if (ws.hstage) { (void)hipHostFree(ws.hstage); ws.hstage = nullptr; ws.hstage_cap = 0; }
    HIPCHK(hipHostMalloc((void**)&ws.hstage, bytes, hipHostMallocDefault));
    ws.hstage_cap = bytes;
  }
  return CLOUDSC_OK;
}

unsigned long long cmp_items(const CmpEntry* e, int n, unsigned ntiles) {
  unsigned long long items = 0;
  for (int m = 0; m < n; m++) items += (unsigned long long)((e[m].rows + kCmpRows - 1) / kCmpRows) * ntiles;
  return items;
}
unsigned cmp_grid(const CmpWorkspace& ws, unsigned long long items) {
  const int knob = g_cmp_grid.load(std::memory_order_relaxed);
  // eight workgroups of four waves per compute unit: every wave slot of the device
  const unsigned long long want = knob > 0 ? (unsigned long long)knob : (unsigned long long)ws.ncu * 8;
  return (unsigned)std::min<unsigned long long>(items, want);
}

// with ws.mu held: launch both kernels over the table, wait for `st`, leave the n records in ws.hres
template <bool REF>
int cmp_launch(CmpWorkspace& ws, hipStream_t st, CmpArgs& a, bool a8, bool b8) {
  const unsigned grid = cmp_grid(ws, cmp_items(a.e, a.n, a.ntiles));
  int rc = ws_grow_part(ws, (size_t)grid * a.n);
  if (rc) return rc;
  a.part = ws.part;
  const dim3 g(grid), wg(kCmpThreads);
  if (REF) {
    if (a8) hipLaunchKernelGGL((fields_compare_kernel<8, 8, true>), g, wg, 0, st, a);
    else hipLaunchKernelGGL((fields_compare_kernel<4, 8, true>), g, wg, 0, st, a);
  } else {
    if (a8 && b8) hipLaunchKernelGGL((fields_compare_kernel<8, 8, false>), g, wg, 0, st, a);
    else if (a8) hipLaunchKernelGGL((fields_compare_kernel<8, 4, false>), g, wg, 0, st, a);
    else if (b8) hipLaunchKernelGGL((fields_compare_kernel<4, 8, false>), g, wg, 0, st, a);
    else hipLaunchKernelGGL((fields_compare_kernel<4, 4, false>), g, wg, 0, st, a);
  }
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(fields_compare_combine_kernel, dim3(a.n), dim3(64), 0, st, (const CmpRec*)ws.part, (int)grid, a.n,
                     ws.res);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ws.hres, ws.res, (size_t)a.n * sizeof(CmpRec), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return CLOUDSC_OK;
}

// the cloudsc_fields_t position of every validated field (cloudsc_field_id order), from the inventory
void valid_members(int* member) {
#define VALID_MEMBER(n, N, k, d, i) CLOUDSC_IF_VALIDATED_##d(member[CLOUDSC_F_##N] = CLOUDSC_M_##n;)
  CLOUDSC_FIELDS(VALID_MEMBER)
#undef VALID_MEMBER
}

}  // namespace

extern "C" int cloudsc_fields_members(void) { return kNumFields; }
extern "C" long long cloudsc_fields_diff_sizeof(void) { return (long long)sizeof(cloudsc_field_diff_t); }

extern "C" int cloudsc_debug_set_compare_grid(int workgroups) {
  if (workgroups < 0 || workgroups > kCmpMaxGrid) return CLOUDSC_EINVAL;
  g_cmp_grid.store(workgroups, std::memory_order_relaxed);
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_compare(int device, void* stream, int ngptot, int klev, int a_precision, int a_nproma,
                                      const cloudsc_fields_t* fa, int b_precision, int b_nproma,
                                      const cloudsc_fields_t* fb, cloudsc_field_diff_t* diff) {
  CmpArgs a;
  int member[kCmpMaxEntries];
  int rc = cmp_build(ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb, diff, &a, member);
  if (rc) return rc;
  CmpWorkspace* ws = nullptr;
  if ((rc = ws_device(device, &ws))) return rc;
  std::lock_guard<std::mutex> lock(ws->mu);
  HIPCHK(hipSetDevice(device));
  if ((rc = ws_ready(*ws, device))) return rc;
  rc = cmp_launch<false>(*ws, (hipStream_t)stream, a, precision_storage_bytes(a_precision) == 8,
                         precision_storage_bytes(b_precision) == 8);
  if (rc) return rc;
  for (int m = 0; m < kNumFields; m++) diff_skipped(&diff[m]);
  for (int i = 0; i < a.n; i++) diff_from(&diff[member[i]], ws->hres[i], a.e[i].rows, ngptot);
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_compare(int nthreads, int ngptot, int klev, int a_precision, int a_nproma,
                                          const cloudsc_fields_t* fa, int b_precision, int b_nproma,
                                          const cloudsc_fields_t* fb, cloudsc_field_diff_t* diff) {
  CmpArgs a;
  int member[kCmpMaxEntries];
  int rc = cmp_build(ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb, diff, &a, member);
  if (rc) return rc;
  const bool a8 = precision_storage_bytes(a_precision) == 8, b8 = precision_storage_bytes(b_precision) == 8;
  void (*block)(const CmpArgs&, long long, CmpRec*) =
      a8 && b8 ? cmp_block<8, 8> : a8 ? cmp_block<8, 4> : b8 ? cmp_block<4, 8> : cmp_block<4, 4>;
  const long long nblocks = ((long long)ngptot + a_nproma - 1) / a_nproma;
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  nthreads = (int)std::min<long long>(nthreads, nblocks);
  std::vector<CmpRec> acc((size_t)nthreads * a.n, cmp_neutral());   // one record per (thread, member)
  std::atomic<long long> next{0};
  auto worker = [&](int t) {
    for (long long b = next.fetch_add(1); b < nblocks; b = next.fetch_add(1)) block(a, b, &acc[(size_t)t * a.n]);
  };
  if (nthreads == 1) {
    worker(0);
  } else {
    std::vector<std::thread> pool;
    pool.reserve((size_t)nthreads);
    try {
      for (int t = 1; t < nthreads; t++) pool.emplace_back(worker, t);
    } catch (...) {
      // fewer threads than asked for: every block is still taken, by them and by the caller
    }
    worker(0);
    for (auto& t : pool) t.join();
  }
  for (int m = 0; m < kNumFields; m++) diff_skipped(&diff[m]);
  for (int i = 0; i < a.n; i++) {
    CmpRec r = cmp_neutral();
    for (int t = 0; t < nthreads; t++) cmp_combine(r, acc[(size_t)t * a.n + i]);   // in thread order
    diff_from(&diff[member[i]], r, a.e[i].rows, ngptot);
  }
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_validate(int device, void* stream, int precision, int ngptot, int nproma, int klev,
                                       long long col_offset, const cloudsc_fields_t* fields,
                                       const cloudsc_reference_t* ref, cloudsc_stats_t* stats) {
  if (!fields || !ref || !stats || col_offset < 0) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || nproma < 1 || nproma > kCmpMaxNproma) return CLOUDSC_EINVAL;
  if (ref->klon <= 0 || ref->klev != klev) return CLOUDSC_EINVAL;
  int member[CLOUDSC_NVALID];
  valid_members(member);
  CmpArgs a;
  std::memset(&a, 0, sizeof(a));
  size_t off[CLOUDSC_NVALID], total = 0;   // bytes of each reference array in the stage
  for (int id = 0; id < CLOUDSC_NVALID; id++) {
    const void* p = ((const void* const*)fields)[member[id]];
    if (!p || !ref->field[id]) return CLOUDSC_EINVAL;
    a.e[id].a = p;
    a.e[id].rows = member_rows(member[id], klev);
    off[id] = total;
    total += (size_t)a.e[id].rows * ref->klon * sizeof(double);
  }
  a.n = CLOUDSC_NVALID;
  a.ngptot = ngptot;
  a.anp = nproma;
  a.bnp = 1;
  a.ntiles = (unsigned)(((long long)ngptot + kCmpThreads - 1) / kCmpThreads);
  a.klon = ref->klon;
  a.col_offset = col_offset % ref->klon;
  CmpWorkspace* ws = nullptr;
  int rc = ws_device(device, &ws);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(ws->mu);
  HIPCHK(hipSetDevice(device));
  if ((rc = ws_ready(*ws, device))) return rc;
  if ((rc = ws_grow_stage(*ws, total, false))) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int id = 0; id < CLOUDSC_NVALID; id++) {
    // on `stream`, ordered before the kernel that reads it
    HIPCHK(hipMemcpyAsync(ws->stage + off[id], ref->field[id], (size_t)a.e[id].rows * ref->klon * sizeof(double),
                          hipMemcpyHostToDevice, st));
    a.e[id].b = ws->stage + off[id];
  }
  rc = cmp_launch<true>(*ws, st, a, precision_storage_bytes(precision) == 8, true);
  if (rc) return rc;
  for (int id = 0; id < CLOUDSC_NVALID; id++) stats[id] = rec_stats(ws->hres[id]);
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_expand(int device, void* stream, int precision, int ngptot, int nproma,
                                     long long col_offset, const cloudsc_template_t* t,
                                     const cloudsc_fields_t* fields) {
  if (!t || !fields || col_offset < 0) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || nproma < 1 || nproma > kCmpMaxNproma || t->klon <= 0 || t->klev < 1) return CLOUDSC_EINVAL;
  const void* tmpl[kNumFields] = {};   // the template array of each cloudsc_fields_t member (NULL: none, or absent)
#define TEMPLATE_OF(n) tmpl[CLOUDSC_M_##n] = t->n;
  CLOUDSC_TEMPLATE_ORDER(TEMPLATE_OF)
#undef TEMPLATE_OF
  ExpArgs a;
  std::memset(&a, 0, sizeof(a));
  const void* host[kCmpMaxEntries];
  size_t off[kCmpMaxEntries], bytes[kCmpMaxEntries], total = 0;
  for (int m = 0; m < kNumFields; m++) {
    if (kFieldTable[m].dir == CLOUDSC_FD_OUT) continue;
    void* d = ((void* const*)fields)[m];   // input members are const void * in the struct and written here
    if (!d) continue;
    if (!tmpl[m]) return CLOUDSC_EINVAL;   // a member to fill that the template does not hold
    ExpEntry& e = a.e[a.n];
    e.dst = d;
    e.rows = member_rows(m, t->klev);
    if (kFieldTable[m].is_int) a.int_mask |= 1ull << a.n;
    host[a.n] = tmpl[m];
    off[a.n] = total;
    bytes[a.n] = (size_t)e.rows * t->klon * (kFieldTable[m].is_int ? sizeof(int) : sizeof(double));
    total += (bytes[a.n] + 15) / 16 * 16;
    a.n++;
  }
  if (!a.n) return CLOUDSC_EINVAL;
  a.ngptot = ngptot;
  a.np = nproma;
  a.klon = t->klon;
  a.ntiles = (unsigned)(((long long)ngptot + kCmpThreads - 1) / kCmpThreads);
  a.col_offset = col_offset % t->klon;
  CmpWorkspace* ws = nullptr;
  int rc = ws_device(device, &ws);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(ws->mu);
  HIPCHK(hipSetDevice(device));
  if ((rc = ws_ready(*ws, device))) return rc;
  if ((rc = ws_grow_stage(*ws, total, true))) return rc;
  // the caller's arrays are copied here, so they are the caller's again when this returns
  for (int i = 0; i < a.n; i++) {
    std::memcpy(ws->hstage + off[i], host[i], bytes[i]);
    a.e[i].src = ws->stage + off[i];
  }
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(ws->stage, ws->hstage, total, hipMemcpyHostToDevice, st));
  unsigned long long items = 0;
  for (int i = 0; i < a.n; i++) items += (unsigned long long)((a.e[i].rows + kCmpRows - 1) / kCmpRows) * a.ntiles;
  const dim3 grid((unsigned)std::min<unsigned long long>(items, (unsigned long long)ws->ncu * 8)), wg(kCmpThreads);
  if (precision_storage_bytes(precision) == 8) hipLaunchKernelGGL(fields_expand_kernel<double>, grid, wg, 0, st, a);
  else hipLaunchKernelGGL(fields_expand_kernel<float>, grid, wg, 0, st, a);
  HIPCHK(hipGetLastError());
  // the staged template is read until the kernel ends: the next call on this device waits for this event
  HIPCHK(hipEventRecord(ws->busy, st));
  ws->pending = true;
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_compare_release(int device) {
  if (device < 0 || device >= kMaxDevices) return CLOUDSC_EINVAL;
  CmpWorkspace& ws = g_ws[device];
  std::lock_guard<std::mutex> lock(ws.mu);
  if (!ws.res && !ws.part && !ws.stage && !ws.hres && !ws.hstage && !ws.busy) return CLOUDSC_OK;   // never used
  HIPCHK(hipSetDevice(device));
  if (ws.pending) { (void)hipEventSynchronize(ws.busy); ws.pending = false; }
  if (ws.part) (void)hipFree(ws.part);
  if (ws.res) (void)hipFree(ws.res);
  if (ws.stage) (void)hipFree(ws.stage);
  if (ws.hres) (void)hipHostFree(ws.hres);
  if (ws.hstage) (void)hipHostFree(ws.hstage);
  if (ws.busy) (void)hipEventDestroy(ws.busy);
  ws.part = ws.res = ws.hres = nullptr;
  ws.stage = ws.hstage = nullptr;
  ws.busy = nullptr;
  ws.part_cap = ws.stage_cap = ws.hstage_cap = 0;
  return CLOUDSC_OK;
}
