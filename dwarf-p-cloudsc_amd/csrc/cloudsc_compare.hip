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
// The kernel.  The item scheme of cloudsc_fieldset.h: per item a lane walks its
// rows with eight non-temporal loads per operand in flight; there is no store in
// the streaming part.  Each lane keeps one record (nine 64-bit accumulators); when
// a workgroup's item sequence leaves a member the record is reduced over the
// workgroup (cross-lane shuffles, then four records through LDS) and written as
// that workgroup's partial of the member, a neutral one if it had no item there.
// A second kernel, one wave per member, combines the partials of a member in
// workgroup order.  No atomics.  min, max, max d, the count and the first key are
// exact whatever the grid and the blockings; the two sums depend on the grouping
// within the double-double bound of cloudsc_stats_t.  Every key is 64-bit.  Lanes
// past ngptot contribute nothing, so padding lanes are never read.
//
// cloudsc_fields_validate is the same kernel with the b operand a double array
// [rows][klon] read at column (col_offset + g) % klon through the caches (the
// reference is small and every tile reads all of it).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <mutex>
#include <type_traits>

#include "cloudsc_fieldset.h"

using namespace cloudsc_impl;

namespace {

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

// nrows rows of one column: x + ao, y + bo address the first row, as / bs are the row strides
template <typename A, typename B>
__device__ __forceinline__ void cmp_rows(const void* pa, const void* pb, size_t ao, size_t bo, size_t as, size_t bs,
                                         int nrows, unsigned long long key0, CmpRec& acc) {
  const typename A::word* __restrict__ x = (const typename A::word*)pa + ao;
  const typename B::word* __restrict__ y = (const typename B::word*)pb + bo;
  for (int r = 0; r < nrows; r += kFsBatch) {
    typename A::word wa[kFsBatch];
    typename B::word wb[kFsBatch];
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) {
        wa[q] = __builtin_nontemporal_load(x + (size_t)(r + q) * as);
        if constexpr (B::nt) wb[q] = __builtin_nontemporal_load(y + (size_t)(r + q) * bs);
        else wb[q] = y[(size_t)(r + q) * bs];
      }
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) cmp_elem<A, B>(wa[q], wb[q], key0 + (unsigned long long)(r + q), acc);
  }
}

// the lanes' records combined into lane 0 of each wave: cross-lane shuffles, a fixed tree from offset `half`
__device__ __forceinline__ void cmp_wave_reduce(CmpRec& acc, int half) {
  for (int off = half; off > 0; off >>= 1) {
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
}

// the workgroup's record of one member: shuffles within a wave, the waves' records through LDS;
// every thread of the workgroup calls it (touched is uniform), acc comes back neutral
__device__ __forceinline__ void cmp_flush(CmpRec* out, CmpRec& acc, bool touched) {
  if (!touched) {   // no item of this member: acc is still neutral
    if (threadIdx.x == 0) *out = cmp_neutral();
    return;
  }
  cmp_wave_reduce(acc, warpSize / 2);
  __shared__ CmpRec s[kFsThreads / 64];
  const int wave = threadIdx.x / warpSize;
  if (threadIdx.x % warpSize == 0) s[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    CmpRec t = s[0];
    for (int w = 1; w < kFsThreads / warpSize; w++) cmp_combine(t, s[w]);
    *out = t;
  }
  __syncthreads();   // s is written again at the next member
  acc = cmp_neutral();
}

struct CmpArgs : FsTable<const void> {
  int klon;               // validate: columns of the reference
  long long col_offset;   // validate: the global column of its column 0
  CmpRec* part;           // [workgroups][n]
};
// The comparison's part of fs_kernel.  AB, BB: bytes of a real element of a and b; REF: b is the reference
// of a validation (double, [rows][klon])
template <int AB, int BB, bool REF>
struct CmpItem {
  using Args = CmpArgs;
  using A = typename CmpReal<AB>::type;
  using B = typename std::conditional<REF, W8Ref, typename CmpReal<BB>::type>::type;
  CmpRec acc = cmp_neutral();
  CmpRec* part;   // this workgroup's
  __device__ CmpItem(const Args& a) : part(a.part + (size_t)blockIdx.x * a.n) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned anp = (unsigned)a.anp;
    const FsPos ap = fs_pos(g, anp);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t ao = fs_offset(ap, anp, r);
    size_t bo, bs;
    if constexpr (REF) {
      bs = (size_t)a.klon;
      bo = fs_wrapped(g, a.col_offset, a.klon, r);
    } else {
      const unsigned bnp = (unsigned)a.bnp;
      bs = bnp;
      bo = fs_offset(fs_pos(g, bnp), bnp, r);
    }
    const unsigned long long key0 = (unsigned long long)g * r.rows + r.row0;
    if (!REF && (a.int_mask >> m & 1)) cmp_rows<WInt, WInt>(a.e[m].a, a.e[m].b, ao, bo, anp, bs, r.nrows, key0, acc);
    else cmp_rows<A, B>(a.e[m].a, a.e[m].b, ao, bo, anp, bs, r.nrows, key0, acc);
  }
  // by every thread of the workgroup: the flush holds barriers
  __device__ __forceinline__ void left(const Args&, int m, bool touched) { cmp_flush(part + m, acc, touched); }
};

// The same with the tendency members of either side in packed buffers (cloudsc_fields_compare_tendbuf,
// cloudsc_fields_validate_tendbuf): the block strides come from the table, everything else is CmpItem's --
// the key and the rows stay the member's own.
struct CmpTendArgs : CmpArgs {
  long long abrows[kFsMaxEntries], bbrows[kFsMaxEntries];   // rows between consecutive blocks of a and b
};
template <int AB, int BB, bool REF>
struct CmpTendItem {
  using Args = CmpTendArgs;
  using A = typename CmpReal<AB>::type;
  using B = typename std::conditional<REF, W8Ref, typename CmpReal<BB>::type>::type;
  CmpRec acc = cmp_neutral();
  CmpRec* part;   // this workgroup's
  __device__ CmpTendItem(const Args& a) : part(a.part + (size_t)blockIdx.x * a.n) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned anp = (unsigned)a.anp;
    const FsPos ap = fs_pos(g, anp);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t ao = fs_offset_strided(ap, anp, r, (size_t)a.abrows[m]);
    size_t bo, bs;
    if constexpr (REF) {
      bs = (size_t)a.klon;
      bo = fs_wrapped(g, a.col_offset, a.klon, r);
    } else {
      const unsigned bnp = (unsigned)a.bnp;
      bs = bnp;
      bo = fs_offset_strided(fs_pos(g, bnp), bnp, r, (size_t)a.bbrows[m]);
    }
    const unsigned long long key0 = (unsigned long long)g * r.rows + r.row0;
    if (!REF && (a.int_mask >> m & 1)) cmp_rows<WInt, WInt>(a.e[m].a, a.e[m].b, ao, bo, anp, bs, r.nrows, key0, acc);
    else cmp_rows<A, B>(a.e[m].a, a.e[m].b, ao, bo, anp, bs, r.nrows, key0, acc);
  }
  __device__ __forceinline__ void left(const Args&, int m, bool touched) { cmp_flush(part + m, acc, touched); }
};

// one wave per member: the partials of the member in workgroup order (lane l takes workgroups l, l + 64, ...,
// then the lanes combine in a fixed tree)
__global__ void __launch_bounds__(64) fields_compare_combine_kernel(const CmpRec* __restrict__ part, int nwg, int n,
                                                                    CmpRec* __restrict__ res) {
  const int m = blockIdx.x;
  CmpRec acc = cmp_neutral();
  for (int w = threadIdx.x; w < nwg; w += 64) cmp_combine(acc, part[(size_t)w * n + m]);
  cmp_wave_reduce(acc, 32);
  if (threadIdx.x == 0) res[m] = acc;
}

// Template expansion into a caller-owned set, the same item scheme: dst[g / np][row][g % np] =
// (T) src[row][(col_offset + g) % klon] for g < ngptot (padding lanes are not written); entry {a, b} =
// {src, dst}, src the staged template on the device (double, ktype int), np = bnp
template <typename S, typename D>
__device__ __forceinline__ void exp_rows(const void* src, void* dst, size_t so, size_t doff, size_t klon, size_t np,
                                         int nrows) {
  const S* __restrict__ s = (const S*)src + so;
  D* __restrict__ d = (D*)dst + doff;
  for (int r = 0; r < nrows; r++) __builtin_nontemporal_store((D)s[(size_t)r * klon], d + (size_t)r * np);
}
struct ExpArgs : FsTable<void> {
  int klon;               // columns of the template
  long long col_offset;   // the global column of its column 0
};
template <typename D>
struct ExpItem {
  using Args = ExpArgs;
  __device__ ExpItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned np = (unsigned)a.bnp;
    const FsPos p = fs_pos(g, np);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t so = fs_wrapped(g, a.col_offset, a.klon, r), doff = fs_offset(p, np, r);
    if (a.int_mask >> m & 1) exp_rows<int, int>(a.e[m].a, a.e[m].b, so, doff, (size_t)a.klon, np, r.nrows);
    else exp_rows<double, D>(a.e[m].a, a.e[m].b, so, doff, (size_t)a.klon, np, r.nrows);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};

// The same writing the tendency members straight into their planes of a packed buffer
// (cloudsc_fields_expand_tendbuf): the destination's block strides come from the table.
struct ExpTendArgs : ExpArgs {
  long long bbrows[kFsMaxEntries];   // rows between consecutive blocks of the destination
};
template <typename D>
struct ExpTendItem {
  using Args = ExpTendArgs;
  __device__ ExpTendItem(const Args&) {}
  __device__ __forceinline__ void item(const Args& a, int m, unsigned g, unsigned long long chunk) {
    const unsigned np = (unsigned)a.bnp;
    const FsPos p = fs_pos(g, np);
    const FsRows r = fs_rows(a, m, chunk);
    const size_t so = fs_wrapped(g, a.col_offset, a.klon, r), doff = fs_offset_strided(p, np, r, (size_t)a.bbrows[m]);
    if (a.int_mask >> m & 1) exp_rows<int, int>(a.e[m].a, a.e[m].b, so, doff, (size_t)a.klon, np, r.nrows);
    else exp_rows<double, D>(a.e[m].a, a.e[m].b, so, doff, (size_t)a.klon, np, r.nrows);
  }
  __device__ __forceinline__ void left(const Args&, int, bool) {}
};

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
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

// the columns of block ab of set a of one entry, on the host: the kernel's index arithmetic in plain loops
// abrows / bbrows: the rows between consecutive blocks of the entry in a / b (its own rows, or a packed buffer's)
template <typename A, typename B>
void cmp_block_entry(const FsEntry<const void>& e, const CmpArgs& a, long long ab, long long abrows, long long bbrows,
                     CmpRec& acc) {
  const long long anp = a.anp, bnp = a.bnp, g0 = ab * anp;
  const long long bsize = std::min<long long>(anp, a.ngptot - g0);
  const typename A::word* x = (const typename A::word*)e.a;
  const typename B::word* y = (const typename B::word*)e.b;
  for (long long row = 0; row < e.rows; row++) {
    const typename A::word* xrow = x + (size_t)(ab * abrows + row) * (size_t)anp;
    fs_runs(g0, bsize, bnp, [&](long long jl, long long bb, long long bj, long long run) {
      const typename B::word* yrow = y + (size_t)(bb * bbrows + row) * (size_t)bnp + bj;
      const unsigned long long g = (unsigned long long)(g0 + jl), rows = (unsigned long long)e.rows;
      for (long long i = 0; i < run; i++) cmp_elem<A, B>(xrow[jl + i], yrow[i], (g + i) * rows + row, acc);
    });
  }
}
// abrows / bbrows: per entry (NULL: every entry's own rows)
template <int AB, int BB>
void cmp_block(const CmpArgs& a, long long ab, const long long* abrows, const long long* bbrows, CmpRec* acc) {
  using A = typename CmpReal<AB>::type;
  using B = typename CmpReal<BB>::type;
  for (int m = 0; m < a.n; m++) {
    const long long ar = abrows ? abrows[m] : a.e[m].rows, br = bbrows ? bbrows[m] : a.e[m].rows;
    if (a.int_mask >> m & 1) cmp_block_entry<WInt, WInt>(a.e[m], a, ab, ar, br, acc[m]);
    else cmp_block_entry<A, B>(a.e[m], a, ab, ar, br, acc[m]);
  }
}

// Per-device workspace of the device entry points: the workgroups' partials, the members' results (device and
// pinned host), the uploaded reference or template, and the event of the last expansion still using them.
// Grows on demand (a growth frees and allocates: the only device-wide synchronisation after the first call).
struct CmpWorkspace {
  std::mutex mu;
  CmpRec* part = nullptr;
  size_t part_cap = 0;          // records
  CmpRec* res = nullptr;        // [kFsMaxEntries], device
  CmpRec* hres = nullptr;       // [kFsMaxEntries], pinned host
  char* stage = nullptr;        // device: the reference (validate) or the template (expand)
  char* hstage = nullptr;       // pinned host: the template of an expansion, copied from the caller's arrays
  size_t stage_cap = 0, hstage_cap = 0;
  hipEvent_t busy = nullptr;    // recorded after an expansion's last kernel
  bool pending = false;
};
CmpWorkspace g_ws[kMaxDevices];
std::atomic<int> g_cmp_grid{0};   // cloudsc_debug_set_compare_grid

// the workspace of `device` (*ncu: its compute units), locked, with the device current, the fixed buffers
// there and no earlier expansion still reading the stage
int ws_open(int device, std::unique_lock<std::mutex>& lock, CmpWorkspace** out, int* ncu) {
  int rc = fs_device(device, ncu);
  if (rc) return rc;
  CmpWorkspace& ws = g_ws[device];
  *out = &ws;
  lock = std::unique_lock<std::mutex>(ws.mu);
  HIPCHK(hipSetDevice(device));
  if (!ws.res) HIPCHK(hipMalloc((void**)&ws.res, kFsMaxEntries * sizeof(CmpRec)));
  if (!ws.hres) HIPCHK(hipHostMalloc((void**)&ws.hres, kFsMaxEntries * sizeof(CmpRec), hipHostMallocDefault));
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

// with ws.mu held: launch both kernels over the table, wait for `st`, leave the n records in ws.hres
// Item: CmpItem over a CmpArgs, CmpTendItem over a CmpTendArgs
template <bool REF, template <int, int, bool> class Item = CmpItem, typename Args = CmpArgs>
int cmp_launch(CmpWorkspace& ws, int ncu, hipStream_t st, Args& a, bool a8, bool b8) {
  const unsigned grid = fs_grid(a, ncu, g_cmp_grid.load(std::memory_order_relaxed));
  int rc = ws_grow_part(ws, (size_t)grid * a.n);
  if (rc) return rc;
  a.part = ws.part;
  const dim3 g(grid), wg(kFsThreads);
  if (REF) {
    if (a8) hipLaunchKernelGGL((fs_kernel<Item<8, 8, true>>), g, wg, 0, st, a);
    else hipLaunchKernelGGL((fs_kernel<Item<4, 8, true>>), g, wg, 0, st, a);
  } else {
    if (a8 && b8) hipLaunchKernelGGL((fs_kernel<Item<8, 8, false>>), g, wg, 0, st, a);
    else if (a8) hipLaunchKernelGGL((fs_kernel<Item<8, 4, false>>), g, wg, 0, st, a);
    else if (b8) hipLaunchKernelGGL((fs_kernel<Item<4, 8, false>>), g, wg, 0, st, a);
    else hipLaunchKernelGGL((fs_kernel<Item<4, 4, false>>), g, wg, 0, st, a);
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

// outputs: the selection both sets were allocated for (the shape of the four surface flux members)
static int compare_impl(int device, void* stream, int ngptot, int klev, int a_precision, int a_nproma,
                        const cloudsc_fields_t* fa, int b_precision, int b_nproma, const cloudsc_fields_t* fb,
                        int outputs, cloudsc_field_diff_t* diff) {
  CmpArgs a = {};
  int member[kFsMaxEntries], ncu = 0;
  if (!diff) return CLOUDSC_EINVAL;
  int rc = fs_build(ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb, &a, member, outputs);
  if (rc) return rc;
  CmpWorkspace* ws = nullptr;
  std::unique_lock<std::mutex> lock;
  if ((rc = ws_open(device, lock, &ws, &ncu))) return rc;
  rc = cmp_launch<false>(*ws, ncu, (hipStream_t)stream, a, precision_storage_bytes(a_precision) == 8,
                         precision_storage_bytes(b_precision) == 8);
  if (rc) return rc;
  for (int m = 0; m < kNumFields; m++) diff_skipped(&diff[m]);
  for (int i = 0; i < a.n; i++) diff_from(&diff[member[i]], ws->hres[i], a.e[i].rows, ngptot);
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_compare(int device, void* stream, int ngptot, int klev, int a_precision, int a_nproma,
                                      const cloudsc_fields_t* fa, int b_precision, int b_nproma,
                                      const cloudsc_fields_t* fb, cloudsc_field_diff_t* diff) {
  return compare_impl(device, stream, ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb,
                      CLOUDSC_OUTPUTS_ALL, diff);
}

extern "C" int cloudsc_fields_compare_outputs(int device, void* stream, int ngptot, int klev, int outputs,
                                              int a_precision, int a_nproma, const cloudsc_fields_t* fa,
                                              int b_precision, int b_nproma, const cloudsc_fields_t* fb,
                                              cloudsc_field_diff_t* diff) {
  if (!outputs_known(outputs)) return CLOUDSC_EINVAL;
  if (!outputs_surface(outputs))   // cloudsc_fields_compare itself
    return cloudsc_fields_compare(device, stream, ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb,
                                  diff);
  return compare_impl(device, stream, ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb, outputs,
                      diff);
}

// the host comparison; a_planes / b_planes: the tendency members of that side are planes of a packed buffer
// with so many planes per block (0: separate arrays)
static int cpu_compare(int nthreads, int ngptot, int klev, int a_precision, int a_nproma, int a_planes,
                       const cloudsc_fields_t* fa, int b_precision, int b_nproma, int b_planes,
                       const cloudsc_fields_t* fb, cloudsc_field_diff_t* diff) {
  CmpArgs a = {};
  int member[kFsMaxEntries];
  if (!diff || !fs_tend_planes_ok(a_planes) || !fs_tend_planes_ok(b_planes)) return CLOUDSC_EINVAL;
  int rc = fs_build(ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb, &a, member);
  if (rc) return rc;
  long long abrows[kFsMaxEntries], bbrows[kFsMaxEntries];
  for (int i = 0; i < a.n; i++) {
    abrows[i] = fs_tend_brows(a, i, member[i], klev, a_planes);
    bbrows[i] = fs_tend_brows(a, i, member[i], klev, b_planes);
  }
  const bool a8 = precision_storage_bytes(a_precision) == 8, b8 = precision_storage_bytes(b_precision) == 8;
  void (*block)(const CmpArgs&, long long, const long long*, const long long*, CmpRec*) =
      a8 && b8 ? cmp_block<8, 8> : a8 ? cmp_block<8, 4> : b8 ? cmp_block<4, 8> : cmp_block<4, 4>;
  const long long nblocks = ((long long)ngptot + a_nproma - 1) / a_nproma;
  nthreads = fs_threads(nthreads, nblocks);
  std::vector<CmpRec> acc((size_t)nthreads * a.n, cmp_neutral());   // one record per (thread, member)
  fs_run_blocks(nthreads, nblocks, [&](int t, long long b) { block(a, b, abrows, bbrows, &acc[(size_t)t * a.n]); });
  for (int m = 0; m < kNumFields; m++) diff_skipped(&diff[m]);
  for (int i = 0; i < a.n; i++) {
    CmpRec r = cmp_neutral();
    for (int t = 0; t < nthreads; t++) cmp_combine(r, acc[(size_t)t * a.n + i]);   // in thread order
    diff_from(&diff[member[i]], r, a.e[i].rows, ngptot);
  }
  return CLOUDSC_OK;
}

extern "C" int cloudsc_cpu_fields_compare(int nthreads, int ngptot, int klev, int a_precision, int a_nproma,
                                          const cloudsc_fields_t* fa, int b_precision, int b_nproma,
                                          const cloudsc_fields_t* fb, cloudsc_field_diff_t* diff) {
  return cpu_compare(nthreads, ngptot, klev, a_precision, a_nproma, 0, fa, b_precision, b_nproma, 0, fb, diff);
}

extern "C" int cloudsc_cpu_fields_compare_tendbuf(int nthreads, int ngptot, int klev, int a_precision, int a_nproma,
                                                  int a_tend_planes, const cloudsc_fields_t* fa, int b_precision,
                                                  int b_nproma, int b_tend_planes, const cloudsc_fields_t* fb,
                                                  cloudsc_field_diff_t* diff) {
  return cpu_compare(nthreads, ngptot, klev, a_precision, a_nproma, a_tend_planes, fa, b_precision, b_nproma,
                     b_tend_planes, fb, diff);
}

extern "C" int cloudsc_fields_compare_tendbuf(int device, void* stream, int ngptot, int klev, int a_precision,
                                              int a_nproma, int a_tend_planes, const cloudsc_fields_t* fa,
                                              int b_precision, int b_nproma, int b_tend_planes,
                                              const cloudsc_fields_t* fb, cloudsc_field_diff_t* diff) {
  if (!fs_tend_planes_ok(a_tend_planes) || !fs_tend_planes_ok(b_tend_planes)) return CLOUDSC_EINVAL;
  if (!a_tend_planes && !b_tend_planes)   // cloudsc_fields_compare itself
    return cloudsc_fields_compare(device, stream, ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb,
                                  diff);
  CmpTendArgs a = {};
  int member[kFsMaxEntries], ncu = 0;
  if (!diff) return CLOUDSC_EINVAL;
  int rc = fs_build(ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb,
                    static_cast<FsTable<const void>*>(&a), member);
  if (rc) return rc;
  for (int i = 0; i < a.n; i++) {
    a.abrows[i] = fs_tend_brows(a, i, member[i], klev, a_tend_planes);
    a.bbrows[i] = fs_tend_brows(a, i, member[i], klev, b_tend_planes);
  }
  CmpWorkspace* ws = nullptr;
  std::unique_lock<std::mutex> lock;
  if ((rc = ws_open(device, lock, &ws, &ncu))) return rc;
  rc = cmp_launch<false, CmpTendItem>(*ws, ncu, (hipStream_t)stream, a, precision_storage_bytes(a_precision) == 8,
                                      precision_storage_bytes(b_precision) == 8);
  if (rc) return rc;
  for (int m = 0; m < kNumFields; m++) diff_skipped(&diff[m]);
  for (int i = 0; i < a.n; i++) diff_from(&diff[member[i]], ws->hres[i], a.e[i].rows, ngptot);
  return CLOUDSC_OK;
}

// the validation; tend_planes: the tendency members of `fields` are planes of a packed buffer with so many
// planes per block (0: separate arrays); outputs: the selection the set was allocated for
static int validate_impl(int device, void* stream, int precision, int ngptot, int nproma, int klev, int tend_planes,
                         int outputs, long long col_offset, const cloudsc_fields_t* fields,
                         const cloudsc_reference_t* ref, cloudsc_stats_t* stats) {
  if (!fields || !ref || !stats || col_offset < 0) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || nproma < 1 || nproma > kFsMaxNproma) return CLOUDSC_EINVAL;
  if (ref->klon <= 0 || ref->klev != klev) return CLOUDSC_EINVAL;
  int member[CLOUDSC_NVALID];
  valid_members(member);
  CmpTendArgs a = {};
  int id_of[CLOUDSC_NVALID];               // the validated field of each entry
  size_t off[CLOUDSC_NVALID], total = 0;   // bytes of each entry's reference array in the stage
  size_t ref_row0[CLOUDSC_NVALID];         // the first reference row of each entry
  for (int id = 0; id < CLOUDSC_NVALID; id++) {
    const void* p = ((const void* const*)fields)[member[id]];
    const bool optional = !output_selected(member[id], outputs);
    if (optional && !p && !ref->field[id]) continue;   // skipped: absent on both sides
    if (!p || !ref->field[id]) return CLOUDSC_EINVAL;
    const int i = a.n;
    fs_add<const void>(&a, member[id], klev, p, nullptr, outputs);   // b: the staged reference, below
    a.abrows[i] = a.bbrows[i] = fs_tend_brows(a, i, member[id], klev, tend_planes);
    // CLOUDSC_OUTPUTS_SURFACE: a surface flux member is one row, held against row klev of its reference profile
    ref_row0[i] = outputs_surface(outputs) && is_surface_flux(member[id]) ? (size_t)klev : 0;
    id_of[i] = id;
    off[i] = total;
    total += (size_t)a.e[i].rows * ref->klon * sizeof(double);
  }
  fs_shape(&a, ngptot, nproma, 1);
  a.klon = ref->klon;
  a.col_offset = col_offset % ref->klon;
  CmpWorkspace* ws = nullptr;
  std::unique_lock<std::mutex> lock;
  int ncu = 0, rc = ws_open(device, lock, &ws, &ncu);
  if (rc || (rc = ws_grow_stage(*ws, total, false))) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < a.n; i++) {
    // on `stream`, ordered before the kernel that reads it
    HIPCHK(hipMemcpyAsync(ws->stage + off[i], ref->field[id_of[i]] + ref_row0[i] * (size_t)ref->klon,
                          (size_t)a.e[i].rows * ref->klon * sizeof(double), hipMemcpyHostToDevice, st));
    a.e[i].b = ws->stage + off[i];
  }
  const bool a8 = precision_storage_bytes(precision) == 8;
  if (!tend_planes && outputs == CLOUDSC_OUTPUTS_ALL) {   // every member's own rows: the kernel without the strides
    CmpArgs& plain = a;
    rc = cmp_launch<true>(*ws, ncu, st, plain, a8, true);
  } else {
    rc = cmp_launch<true, CmpTendItem>(*ws, ncu, st, a, a8, true);
  }
  if (rc) return rc;
  for (int id = 0; id < CLOUDSC_NVALID; id++) stats[id] = {__DBL_MAX__, -__DBL_MAX__, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < a.n; i++) stats[id_of[i]] = rec_stats(ws->hres[i]);
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_validate_tendbuf(int device, void* stream, int precision, int ngptot, int nproma,
                                               int klev, int tend_planes, int outputs, long long col_offset,
                                               const cloudsc_fields_t* fields, const cloudsc_reference_t* ref,
                                               cloudsc_stats_t* stats) {
  if (!fs_tend_planes_ok(tend_planes)) return CLOUDSC_EINVAL;
  if (!outputs_known(outputs)) return CLOUDSC_EINVAL;
  return validate_impl(device, stream, precision, ngptot, nproma, klev, tend_planes, outputs, col_offset, fields, ref,
                       stats);
}

extern "C" int cloudsc_fields_validate(int device, void* stream, int precision, int ngptot, int nproma, int klev,
                                       long long col_offset, const cloudsc_fields_t* fields,
                                       const cloudsc_reference_t* ref, cloudsc_stats_t* stats) {
  return validate_impl(device, stream, precision, ngptot, nproma, klev, 0, CLOUDSC_OUTPUTS_ALL, col_offset, fields,
                       ref, stats);
}

// the expansion; tend_planes: the tendency members of `fields` are planes of a packed buffer with so many
// planes per block (0: separate arrays)
static int expand_impl(int device, void* stream, int precision, int ngptot, int nproma, int tend_planes,
                       long long col_offset, const cloudsc_template_t* t, const cloudsc_fields_t* fields) {
  if (!t || !fields || col_offset < 0) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || nproma < 1 || nproma > kFsMaxNproma || t->klon <= 0 || t->klev < 1) return CLOUDSC_EINVAL;
  const void* tmpl[kNumFields] = {};   // the template array of each cloudsc_fields_t member (NULL: none, or absent)
#define TEMPLATE_OF(n) tmpl[CLOUDSC_M_##n] = t->n;
  CLOUDSC_TEMPLATE_ORDER(TEMPLATE_OF)
#undef TEMPLATE_OF
  ExpTendArgs a = {};
  const void* host[kFsMaxEntries];
  size_t off[kFsMaxEntries], bytes[kFsMaxEntries], total = 0;
  for (int m = 0; m < kNumFields; m++) {
    if (kFieldTable[m].dir == CLOUDSC_FD_OUT) continue;
    void* d = ((void* const*)fields)[m];   // input members are const void * in the struct and written here
    if (!d) continue;
    if (!tmpl[m]) return CLOUDSC_EINVAL;   // a member to fill that the template does not hold
    const int i = a.n;
    fs_add<void>(&a, m, t->klev, nullptr, d);   // a: the staged template, below
    a.bbrows[i] = fs_tend_brows(a, i, m, t->klev, tend_planes);
    host[i] = tmpl[m];
    off[i] = total;
    bytes[i] = (size_t)a.e[i].rows * t->klon * (kFieldTable[m].is_int ? sizeof(int) : sizeof(double));
    total += (bytes[i] + 15) / 16 * 16;
  }
  if (!a.n) return CLOUDSC_EINVAL;
  fs_shape(&a, ngptot, 1, nproma);
  a.klon = t->klon;
  a.col_offset = col_offset % t->klon;
  CmpWorkspace* ws = nullptr;
  std::unique_lock<std::mutex> lock;
  int ncu = 0, rc = ws_open(device, lock, &ws, &ncu);
  if (rc || (rc = ws_grow_stage(*ws, total, true))) return rc;
  // the caller's arrays are copied here, so they are the caller's again when this returns
  for (int i = 0; i < a.n; i++) {
    std::memcpy(ws->hstage + off[i], host[i], bytes[i]);
    a.e[i].a = ws->stage + off[i];
  }
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(ws->stage, ws->hstage, total, hipMemcpyHostToDevice, st));
  const dim3 grid(fs_grid(a, ncu)), wg(kFsThreads);   // cloudsc_debug_set_compare_grid does not apply
  const bool d8 = precision_storage_bytes(precision) == 8;
  if (tend_planes) {
    if (d8) hipLaunchKernelGGL(fs_kernel<ExpTendItem<double>>, grid, wg, 0, st, a);
    else hipLaunchKernelGGL(fs_kernel<ExpTendItem<float>>, grid, wg, 0, st, a);
  } else {
    const ExpArgs& plain = a;
    if (d8) hipLaunchKernelGGL(fs_kernel<ExpItem<double>>, grid, wg, 0, st, plain);
    else hipLaunchKernelGGL(fs_kernel<ExpItem<float>>, grid, wg, 0, st, plain);
  }
  HIPCHK(hipGetLastError());
  // the staged template is read until the kernel ends: the next call on this device waits for this event
  HIPCHK(hipEventRecord(ws->busy, st));
  ws->pending = true;
  return CLOUDSC_OK;
}

extern "C" int cloudsc_fields_expand(int device, void* stream, int precision, int ngptot, int nproma,
                                     long long col_offset, const cloudsc_template_t* t,
                                     const cloudsc_fields_t* fields) {
  return expand_impl(device, stream, precision, ngptot, nproma, 0, col_offset, t, fields);
}

extern "C" int cloudsc_fields_expand_tendbuf(int device, void* stream, int precision, int ngptot, int nproma,
                                             int tend_planes, long long col_offset, const cloudsc_template_t* t,
                                             const cloudsc_fields_t* fields) {
  if (tend_planes < CLOUDSC_TENDBUF_PLANES_MIN || tend_planes > CLOUDSC_TENDBUF_PLANES_MAX) return CLOUDSC_EINVAL;
  return expand_impl(device, stream, precision, ngptot, nproma, tend_planes, col_offset, t, fields);
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
