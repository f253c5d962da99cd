// cloudsc_fieldset.h -- the item scheme of the streaming kernels over caller-owned
// field sets (cloudsc_convert.hip, cloudsc_compare.hip), once: the table, the
// device walker, the index helpers and the host plumbing.  Not part of the ABI.
//
// The table.  One launch covers every member: the members travel as a table of
// {a, b, rows} entries by value in the kernel arguments, generated from
// cloudsc_fields.def through kFieldTable.
//
// The items.  A work item is (member, tile of 256 consecutive global columns,
// chunk of 16 rows); a grid of at most eight workgroups per compute unit strides
// the items of all members as one sequence, a member's items in (tile, chunk)
// order with the chunk running fastest, so the workgroups in flight together
// sweep neighbouring rows of the same blocks.  Lane t of a workgroup owns column
// g = tile * 256 + t: it divides once per item and set for its block and lane
// (32-bit divisions: g < 2^31) and then walks the rows of the chunk by adding the
// NPROMA, eight loads in flight.  Consecutive lanes hold consecutive columns, so
// a wave's 64 accesses to a row are one run of 64 elements when the NPROMA is a
// multiple of 64 and runs of min(NPROMA, 64) otherwise.  Every element offset is
// 64-bit (one fp64 species field at 163840 columns is 0.9 GB).  Lanes past ngptot
// do nothing, so padding lanes are neither read nor written.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "cloudsc_internal.h"

namespace cloudsc_impl {

constexpr int kFsMaxEntries = 48;   // the table's capacity (about 1 KiB of kernel arguments)
static_assert(kNumFields <= kFsMaxEntries, "the table holds every cloudsc_fields_t member");
static_assert(kNumFields <= 64, "FsTable::int_mask has one bit per member");
constexpr int kFsThreads = 256;     // columns per tile = threads per workgroup
constexpr int kFsRows = 16;         // rows per item
constexpr int kFsBatch = 8;         // loads per operand a lane has in flight
constexpr int kFsMaxNproma = 1 << 24;

// B: `void` where the second member is written (convert, expand), `const void` where both are read
template <typename B>
struct FsEntry {
  const void* a;    // the first set's member; convert, expand: the source
  B* b;             // the second set's member; convert, expand: the destination; validate: the reference
  long long rows;   // klev | klev + 1 | NCLV * klev | 1
};
// the part of the kernel arguments that every kernel has; a kernel's own arguments derive from it
template <typename B>
struct FsTable {
  FsEntry<B> e[kFsMaxEntries];
  unsigned long long int_mask;   // bit i: entry i is int32 (ktype)
  int n, ngptot, anp, bnp;       // entries, columns, the NPROMA of a and of b
  unsigned ntiles;               // ceil(ngptot / kFsThreads)
};

__host__ __device__ __forceinline__ unsigned long long fs_chunks(long long rows) {
  return (unsigned long long)(rows + kFsRows - 1) / kFsRows;
}

// The walker: the kernel of every field set entry point, workgroup blockIdx.x walking its items.  K gives
// the kernel's own part: K::Args, the kernel arguments (an FsTable or derived from one); K(a), a thread's
// state; k.item(a, m, g, chunk), called for lane g < ngptot of an item of entry m, which takes the rows
// fs_rows(a, m, chunk); k.left(a, m, touched), called when the workgroup's sequence has left entry m,
// `touched` if it had an item there.  Every thread of the workgroup calls left (m, first, count and `it`
// depend on blockIdx.x and the table only), so it may hold a barrier.  It is the kernel itself and not a
// device function inlined into three kernels, so that its loop compiles the same whatever K is.
template <typename K>
__global__ void __launch_bounds__(kFsThreads) fs_kernel(const typename K::Args a) {
  bool touched = false;
  int m = 0;
  unsigned long long first = 0;   // the first item of entry m
  unsigned long long nchunk = fs_chunks(a.e[0].rows);
  unsigned long long count = nchunk * a.ntiles;
  K k(a);
  for (unsigned long long it = blockIdx.x;; it += gridDim.x) {
    while (it >= first + count) {
      k.left(a, m, touched);
      touched = false;
      first += count;
      if (++m >= a.n) return;
      nchunk = fs_chunks(a.e[m].rows);
      count = nchunk * a.ntiles;
    }
    touched = true;
    const unsigned long long local = it - first, tile = local / nchunk, chunk = local - tile * nchunk;
    const unsigned long long g64 = tile * kFsThreads + threadIdx.x;
    if (g64 < (unsigned long long)a.ngptot) k.item(a, m, (unsigned)g64, chunk);
  }
}

// the rows of chunk `chunk` of entry m: [row0, row0 + nrows) of the entry's `rows`
struct FsRows {
  size_t rows, row0;
  int nrows;
};
template <typename B>
__device__ __forceinline__ FsRows fs_rows(const FsTable<B>& a, int m, unsigned long long chunk) {
  const size_t rows = (size_t)a.e[m].rows, row0 = (size_t)chunk * kFsRows;
  return {rows, row0, (int)std::min<size_t>(kFsRows, rows - row0)};
}
// column g in blocks of np columns: block g / np, lane g % np (one 32-bit division), and the element offset
// of its first row in a member: [block][row0][lane]
struct FsPos {
  unsigned block, lane;
};
__device__ __forceinline__ FsPos fs_pos(unsigned g, unsigned np) {
  const unsigned b = g / np;
  return {b, g - b * np};
}
__device__ __forceinline__ size_t fs_offset(FsPos p, unsigned np, FsRows r) {
  return ((size_t)p.block * r.rows + r.row0) * np + p.lane;
}
// the same in a member whose blocks are `brows` rows apart (a plane of a packed tendency buffer: brows > r.rows)
__device__ __forceinline__ size_t fs_offset_strided(FsPos p, unsigned np, FsRows r, size_t brows) {
  return ((size_t)p.block * brows + r.row0) * np + p.lane;
}
// the same in a [rows][klon] operand whose column 0 is global column col_offset: [row0][(col_offset + g) % klon]
__device__ __forceinline__ size_t fs_wrapped(unsigned g, long long col_offset, int klon, FsRows r) {
  return r.row0 * (size_t)klon + (size_t)((col_offset + (long long)g) % klon);
}

// The copies (cloudsc_convert.hip, cloudsc_transpose.hip).  The element type of a storage size; a copy between equal sizes moves bits
template <int BYTES> struct ConvReal { using type = double; using bits = unsigned long long; };
template <> struct ConvReal<4> { using type = float; using bits = unsigned; };
template <int SB, int DB> struct ConvPair {
  using S = typename std::conditional<SB == DB, typename ConvReal<SB>::bits, typename ConvReal<SB>::type>::type;
  using D = typename std::conditional<SB == DB, typename ConvReal<DB>::bits, typename ConvReal<DB>::type>::type;
};

// nrows rows of one column: src + so, dst + doff address the first row, the row strides are the NPROMAs
template <typename S, typename D>
__device__ __forceinline__ void conv_rows(const void* src, void* dst, size_t so, size_t doff, size_t snp, size_t dnp,
                                          int nrows) {
  const S* __restrict__ s = (const S*)src + so;
  D* __restrict__ d = (D*)dst + doff;
  for (int r = 0; r < nrows; r += kFsBatch) {
    S v[kFsBatch];
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) v[q] = __builtin_nontemporal_load(s + (size_t)(r + q) * snp);
#pragma unroll
    for (int q = 0; q < kFsBatch; q++)
      if (r + q < nrows) __builtin_nontemporal_store((D)v[q], d + (size_t)(r + q) * dnp);
  }
}

// ---------------------------------------------------------------------------
// host side; no HIP call up to fs_device
// ---------------------------------------------------------------------------
// entry a->n++ for cloudsc_fields_t member m; outputs: the selection of the sets, which overrides the
// inventory's kind for the four surface flux members (field_kind_of) -- here in the walker's table, not in
// the inventory
template <typename B>
inline void fs_add(FsTable<B>* a, int m, int klev, const void* pa, B* pb, int outputs = CLOUDSC_OUTPUTS_ALL) {
  a->e[a->n] = {pa, pb, (long long)per_block_elems(field_kind_of(m, outputs), 1, klev)};
  if (kFieldTable[m].is_int) a->int_mask |= 1ull << a->n;
  a->n++;
}
template <typename B>
inline void fs_shape(FsTable<B>* a, int ngptot, int anp, int bnp) {
  a->ngptot = ngptot;
  a->anp = anp;
  a->bnp = bnp;
  a->ntiles = (unsigned)(((long long)ngptot + kFsThreads - 1) / kFsThreads);
}
// the argument rules of a pair of field sets and its table (*a zeroed by the caller): every member set in
// both; member[i] (if asked for) = the cloudsc_fields_t position of entry i; a table whose second set is
// written (convert) refuses a member that is the same array in both
template <typename B>
inline int fs_build(int ngptot, int klev, int a_precision, int a_nproma, const cloudsc_fields_t* fa, int b_precision,
                    int b_nproma, const cloudsc_fields_t* fb, FsTable<B>* a, int* member = nullptr,
                    int outputs = CLOUDSC_OUTPUTS_ALL) {
  if (!fa || !fb) return CLOUDSC_EINVAL;
  if (!precision_storage_bytes(a_precision) || !precision_storage_bytes(b_precision)) return CLOUDSC_EINVAL;
  if (ngptot < 1 || klev < 1 || a_nproma < 1 || b_nproma < 1) return CLOUDSC_EINVAL;
  if (a_nproma > kFsMaxNproma || b_nproma > kFsMaxNproma) return CLOUDSC_EINVAL;
  for (int m = 0; m < kNumFields; m++) {
    const void* pa = ((const void* const*)fa)[m];
    B* pb = ((B* const*)fb)[m];   // input members are const void * in the struct; convert writes them
    if (!pa && !pb) continue;
    if (!pa || !pb || (!std::is_const<B>::value && pa == pb)) return CLOUDSC_EINVAL;
    if (member) member[a->n] = m;
    fs_add(a, m, klev, pa, pb, outputs);
  }
  if (!a->n) return CLOUDSC_EINVAL;
  fs_shape(a, ngptot, a_nproma, b_nproma);
  return CLOUDSC_OK;
}

// Packed tendency buffers (cloudsc_fields_convert_tendbuf): a table with the rows between consecutive blocks
// of every entry, on both sides.  A plain member's is its `rows`; the eight tendency members of a side whose
// tend_planes is non-zero are planes of a buffer [nblocks][tend_planes][klev][np]: tend_planes * klev.
struct FsTendTable : FsTable<void> {
  long long abrows[kFsMaxEntries], bbrows[kFsMaxEntries];
};
inline bool fs_is_tendency(int m) { return std::strncmp(kFieldTable[m].name, "tendency_", 9) == 0; }
inline bool fs_tend_planes_ok(int planes) {
  return planes == 0 || (planes >= CLOUDSC_TENDBUF_PLANES_MIN && planes <= CLOUDSC_TENDBUF_PLANES_MAX);
}
// the rows between consecutive blocks of entry i of a table, for a side with `planes` planes (0: separate
// arrays), member = the entry's cloudsc_fields_t position
template <typename B>
inline long long fs_tend_brows(const FsTable<B>& a, int i, int member, int klev, int planes) {
  return planes && fs_is_tendency(member) ? (long long)planes * klev : a.e[i].rows;
}
// fs_build, then the block strides of the two sides; member: scratch of kFsMaxEntries ints
inline int fs_build_tend(int ngptot, int klev, int a_precision, int a_nproma, int a_planes, const cloudsc_fields_t* fa,
                         int b_precision, int b_nproma, int b_planes, const cloudsc_fields_t* fb, FsTendTable* a) {
  if (!fs_tend_planes_ok(a_planes) || !fs_tend_planes_ok(b_planes)) return CLOUDSC_EINVAL;
  int member[kFsMaxEntries];
  const int rc = fs_build<void>(ngptot, klev, a_precision, a_nproma, fa, b_precision, b_nproma, fb, a, member);
  if (rc) return rc;
  for (int i = 0; i < a->n; i++) {
    a->abrows[i] = fs_tend_brows(*a, i, member[i], klev, a_planes);
    a->bbrows[i] = fs_tend_brows(*a, i, member[i], klev, b_planes);
  }
  return CLOUDSC_OK;
}

template <typename B>
inline unsigned long long fs_items(const FsTable<B>& a) {
  unsigned long long items = 0;
  for (int m = 0; m < a.n; m++) items += fs_chunks(a.e[m].rows) * a.ntiles;
  return items;
}
// workgroups of a launch: eight of four waves per compute unit (every wave slot of the device), or `knob`
template <typename B>
inline unsigned fs_grid(const FsTable<B>& a, int ncu, int knob = 0) {
  const unsigned long long want = knob > 0 ? (unsigned long long)knob : (unsigned long long)ncu * 8;
  return (unsigned)std::min<unsigned long long>(fs_items(a), want);
}

inline std::atomic<int> g_fs_ncu[kMaxDevices];   // compute units per device, 0 = not asked yet
// CLOUDSC_ENODEV unless `device` is one of this process's; its compute units
inline int fs_device(int device, int* ncu) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CLOUDSC_ENODEV; }
  if (device < 0 || device >= ndev || device >= kMaxDevices) return CLOUDSC_ENODEV;
  *ncu = g_fs_ncu[device].load(std::memory_order_relaxed);
  if (!*ncu) {
    if (hipDeviceGetAttribute(ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || *ncu <= 0) {
      (void)hipGetLastError();
      *ncu = 256;
    }
    g_fs_ncu[device].store(*ncu, std::memory_order_relaxed);
  }
  return CLOUDSC_OK;
}

// cloudsc_cpu_fields_convert for two sets of one output selection (cloudsc_convert.hip)
int cpu_convert(int nthreads, int ngptot, int klev, int src_precision, int src_nproma, const cloudsc_fields_t* src,
                int dst_precision, int dst_nproma, const cloudsc_fields_t* dst, int outputs);

// The host twins walk a block of one set and meet the other set in runs: fn(jl, b, j, run) for the columns
// [g0 + jl, g0 + jl + run) of [g0, g0 + n), which are columns [j, j + run) of block b in blocks of np
template <typename Fn>
inline void fs_runs(long long g0, long long n, long long np, Fn&& fn) {
  for (long long jl = 0; jl < n;) {
    const long long g = g0 + jl, b = g / np, j = g - b * np;
    const long long run = std::min(n - jl, np - j);
    fn(jl, b, j, run);
    jl += run;
  }
}

// the threads of fs_run_blocks: nthreads (<= 0: the hardware's), at most one per block
inline int fs_threads(int nthreads, long long nblocks) {
  if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
  return (int)std::min<long long>(nthreads, nblocks);
}
// fn(thread, block) for every block in [0, nblocks), the blocks taken from a shared counter by
// fs_threads(nthreads, nblocks) threads, the caller among them as thread 0.  One thread runs inline; threads
// that fail to start are done without.
template <typename Fn>
inline void fs_run_blocks(int nthreads, long long nblocks, Fn&& fn) {
  nthreads = fs_threads(nthreads, nblocks);
  std::atomic<long long> next{0};
  auto worker = [&](int t) {
    for (long long b = next.fetch_add(1); b < nblocks; b = next.fetch_add(1)) fn(t, b);
  };
  if (nthreads == 1) {
    worker(0);
    return;
  }
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

}  // namespace cloudsc_impl
