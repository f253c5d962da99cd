// cloudsc_state.hip -- the device-resident dwarf state of include/cloudsc_amd.h
// (cloudsc_state_*): on-device expansion of the KLON-column template (g % klon
// of the GLOBAL column index), timed runs on the state's stream, and validation
// against the KLON-column reference through cloudsc_fields_validate.
#include <algorithm>
#include <atomic>
#include <hip/hip_runtime.h>

#include <chrono>

#include <cstdio>
#include <cstring>
#include <vector>

#include "cloudsc_amd.h"
#include "cloudsc_internal.h"

using namespace cloudsc_impl;

// ---------------------------------------------------------------------------
// plumbing kernel: expansion
// ---------------------------------------------------------------------------
// dst[b][L][i] = src[L][(col_offset + b*nproma + i) % klon], L < nlev.
// A 1-D grid strides over all nblocks*nlev*nproma elements with 64-bit
// indices: no grid dimension carries the block count (HIP's y/z limit is
// 65536 -- the CUDA driver's gridDim.z quirk, SURVEY.md Appendix B item 7,
// cloudsc_driver.cu:391-397), and nlev*nproma may exceed 2^31 (685 species
// levels x NPROMA > 3.1 M).
template <typename T, typename S>
__global__ void expand_kernel(T* __restrict__ dst, const S* __restrict__ src, int nlev, int klon,
                              int nproma, long long col_offset, long long nblocks) {
  const long long per = (long long)nlev * nproma, total = per * nblocks;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long b = e / per, r = e - b * per;
    const long long L = r / nproma, i = r - L * nproma;
    const long long g = col_offset + b * nproma + i;
    dst[e] = (T)src[L * klon + g % klon];
  }
}

// ---------------------------------------------------------------------------
// C ABI: device-resident dwarf state
// ---------------------------------------------------------------------------
struct cloudsc_gpu_state {
  int device, precision, ngptot, nproma, klev, klon, nblocks;
  long long col_offset;
  size_t es;                      // bytes of a real field element in memory (precision_storage_bytes)
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  cloudsc_fields_t f;             // device pointers
  void* plude_pristine;
  void* scratch;                  // SCC temporaries
  void* kseg_ws;                  // KSEG counter, flags and carried state
  cloudsc_impl::KsegEpoch kseg_epoch;   // where the last launch on kseg_ws left its counter and flag stamps
  ParamSet params;                // the state's own parameter set (never shared)
  std::vector<void*> allocs;
  size_t fbytes[kNumFields];      // bytes of each field, cloudsc_fields_t order
  float place_first_ms = 0.f, place_final_ms = 0.f;           // output write probe before / after the search
  int place_tries = 0, place_moves = 0;
  cloudsc_impl::PlaceCost pcost;                              // the search's cost (both phases)
};

namespace {

size_t field_elems(const cloudsc_gpu_state* s, int kind) {
  return (size_t)s->nblocks * per_block_elems(kind, s->nproma, s->klev);
}

// the cloudsc_fields_t position of a validated field (cloudsc_field_id), from the inventory
int valid_member(int id) {
  int member[CLOUDSC_NVALID];
#define VALID_MEMBER(n, N, k, d, i) CLOUDSC_IF_VALIDATED_##d(member[CLOUDSC_F_##N] = CLOUDSC_M_##n;)
  CLOUDSC_FIELDS(VALID_MEMBER)
  return member[id];
}

#ifdef CLOUDSC_DEBUG_KNOBS
// diagnostic build only: allocation flags of the state's fields
// (cloudsc_debug_set_state_layout, hipExtMallocWithFlags); 0 = hipMalloc
std::atomic<unsigned> g_alloc_flags{0};
#endif

int dalloc(cloudsc_gpu_state* s, void** p, size_t bytes) {
#ifdef CLOUDSC_DEBUG_KNOBS
  const unsigned fl = g_alloc_flags.load();
  hipError_t e = dev_malloc(p, bytes, fl);
#else
  hipError_t e = dev_malloc(p, bytes);
#endif
  if (e != hipSuccess) { hip_fail(e, "hipMalloc"); return CLOUDSC_ENOMEM; }
  s->allocs.push_back(*p);
  return CLOUDSC_OK;
}

// Diagnostic field placement (cloudsc_debug_set_state_layout): < 0 = one
// hipMalloc per field (the default); >= 0 = all fields of a state carved out of
// one arena, field i starting at a 2 MiB boundary plus (i * stagger) mod 2 MiB.
std::atomic<long long> g_layout_stagger{-1};
constexpr size_t kArenaAlign = (size_t)2 << 20;
struct Arena {
  char* base = nullptr;
  size_t off = 0;
  long long stagger = -1;
  int n = 0;
};
size_t arena_span(size_t bytes) { return (bytes + kArenaAlign - 1) / kArenaAlign * kArenaAlign + kArenaAlign; }
int field_alloc(cloudsc_gpu_state* s, Arena& ar, void** p, size_t bytes) {
  if (!ar.base) return dalloc(s, p, bytes);
  // stagger < 2 MiB (cloudsc_debug_set_state_layout) and n < 64: no overflow
  *p = ar.base + ar.off + (size_t)(((long long)ar.n * ar.stagger) % (long long)kArenaAlign);
  ar.off += arena_span(bytes);
  ar.n++;
  return CLOUDSC_OK;
}

// ---------------------------------------------------------------------------
// Output placement search.  How fast the kernel writes its 21 output fields
// depends on where they land in HBM: states of one configuration ran 1.63-1.94
// ms (fp64 KSEG), the whole difference carried by the OUTPUT fields -- moving
// them to fresh allocations one at a time recovered it, moving inputs did
// nothing (profiles/r04/placement/placement_fields_fp64.jsonl) -- and the slow
// states stall 5-10x longer on DRAM write credits (TCC_EA0_WRREQ_DRAM_CREDIT_STALL,
// profiles/r04/placement/placement_pmc.txt).  Each field alone writes at the
// same rate wherever it lies; the loss comes from fields written together
// whose physical pages collide (tools/place_probe.hip reproduces a 26 % spread
// with no CLOUDSC code; staggering the fields' virtual offsets does not remove
// it, profiles/r04/placement/ab_layout_staggers_fp64.txt).  So at creation the
// state times the physics kernel itself (KSEG, on the state's inputs) over
// candidate placements of its outputs: whole fresh output sets first, then one
// field at a time, keeping a candidate only if the kernel time drops by more
// than 1 % (search_outputs, cloudsc_place.hip: a rejected set is freed at once
// behind spacers that keep the next set off its pages, rejected single fields
// are held until their pass ends); an allocation failure ends the search with
// the best placement so far.  Outputs are written before the search's launches
// only by those launches and are reset afterwards: the results do not depend
// on it (cloudsc_debug_set_placement_search turns it off).
std::atomic<int> g_place_passes{2};   // cloudsc_debug_set_placement_search
#ifndef CLOUDSC_PLACE_SETS   // experiment builds: make variant VFLAGS=-DCLOUDSC_PLACE_SETS=n
#define CLOUDSC_PLACE_SETS 8
#endif
constexpr int kPlaceSets = CLOUDSC_PLACE_SETS;   // whole fresh output sets tried before the field-by-field passes
constexpr int kPlaceInputSets = 4;               // input sets (place_inputs): the first in field order, the others
                                                 // shuffled with spacers

// the KSEG kernel's time on the state's inputs with the output pointers of f:
// best of 2 timed launches after one untimed, in ms; < 0 on an error
float probe_kernel(cloudsc_gpu_state* s, const cloudsc_fields_t& f, const void* plude_in = nullptr) {
  float best = -1.f;
  const LaunchEvents lev{s->ev0, s->ev1};
  const RunContext ctx{plude_in ? plude_in : s->plude_pristine, &s->params, &s->kseg_epoch, &lev};
  for (int r = 0; r < 3; r++) {
    if (gpu_run_impl(s->device, s->stream, {s->precision, CLOUDSC_VARIANT_KSEG, s->ngptot, s->nproma, s->klev}, &f,
                     s->kseg_ws, {}, ctx) != CLOUDSC_OK ||
        hipEventSynchronize(s->ev1) != hipSuccess)
      return -1.f;
    float t = 0.f;
    if (hipEventElapsedTime(&t, s->ev0, s->ev1) != hipSuccess) return -1.f;
    if (r > 0 && (best < 0.f || t < best)) best = t;
  }
  return best;
}

void dfree(cloudsc_gpu_state* s, void* p) {
  for (auto& q : s->allocs)
    if (q == p) { q = s->allocs.back(); s->allocs.pop_back(); break; }
  dev_free(p);
}

// members/bytes: the output fields (positions in cloudsc_fields_t); moves
// s->f's pointers.  The search itself is search_outputs (cloudsc_place.hip)
// with the KSEG kernel on the state's own inputs as the probe.
int place_outputs(cloudsc_gpu_state* s, const int* members, const size_t* bytes, int n) {
  const int passes = g_place_passes.load();
  if (passes <= 0) return CLOUDSC_OK;
  PlaceCost& cost = s->pcost;
  const auto t0 = std::chrono::steady_clock::now();
  auto probe = [&](const cloudsc_fields_t& f) {
    cost.launches += 3;
    return probe_kernel(s, f);
  };
  // the shader clock leaves its idle level over the first ~10-15 launches
  // (bench.py prewarm): warm it before the first time is taken
  for (int w = 0; w < 4; w++)
    if (probe(s->f) < 0.f) return CLOUDSC_EHIP;
  cloudsc_fields_t f = s->f;
  int rc = search_outputs(f, members, bytes, n, kPlaceSets, passes, 0x9e3779b9u ^ (uint32_t)(uintptr_t)s, probe,
                          cost);
  void** bf = (void**)&f;
  void** sf = (void**)&s->f;
  // probes whose segment hand-offs timed out (the diagnostic spin limit, or a
  // real fault of the schedule) timed nothing meaningful: keep the first
  // placement, clear the workspace's error and record the search as abandoned
  // (probe_final_ms < 0); a KSEG run of the state reports such a fault itself
  bool revert = rc != CLOUDSC_OK;
  if (rc == CLOUDSC_OK) {
    const int hc = kseg_check(s->device, s->stream, s->kseg_ws);
    if (hc == CLOUDSC_EHANDOFF) {
      revert = true;
      cost.moves = 0;
      cost.final_ms = -1.f;
    } else {
      rc = hc;
      revert = rc != CLOUDSC_OK;
    }
  }
  // the chosen buffers become the state's and the originals they replace go
  // (or, reverting, the other way round)
  for (int q = 0; q < n; q++) {
    const int m = members[q];
    if (bf[m] == sf[m]) continue;
    if (revert) {
      dev_free(bf[m]);
      continue;
    }
    dfree(s, sf[m]);
    s->allocs.push_back(bf[m]);
    sf[m] = bf[m];
  }
  s->place_first_ms = cost.first_ms;
  s->place_final_ms = cost.final_ms;
  s->place_tries = cost.tries;
  s->place_moves = cost.moves;
  cost.search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// Whole fresh INPUT sets, contents copied, after the output search: one state in
// six kept its slow time through every output candidate
// (profiles/r04/placement/placement_search_ab_fp64.jsonl), so the pages its
// inputs landed on are tried too.  Same rule: a set is kept when the kernel is
// more than 1 % faster.  members/bytes: the input fields (positions in
// cloudsc_fields_t); member -1 is the pristine plude copy.  A rejected set is
// freed as soon as it loses; the spacers, held to the end, keep the next
// candidate off its pages.
int place_inputs(cloudsc_gpu_state* s, const int* members, const size_t* bytes, int n) {
  float best = s->place_final_ms;
  if (!(best > 0.f) || g_place_passes.load() <= 0) return CLOUDSC_OK;
  void** sf = (void**)&s->f;
  auto slot = [&](void** set, void*& pl, int m) -> void*& { return m < 0 ? pl : set[m]; };
  cloudsc_fields_t best_f = s->f;
  void* best_pl = s->plude_pristine;
  std::vector<void*> mine;               // every candidate buffer allocated here
  std::vector<void*> spacers;
  uint32_t rng = 0x85ebca6bu ^ (uint32_t)(uintptr_t)s;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
  int rc = CLOUDSC_OK;
  PlaceCost& cost = s->pcost;
  const auto t0 = std::chrono::steady_clock::now();
  size_t live = 0;                        // candidate and spacer bytes held now
  auto note = [&]() { cost.peak_bytes = std::max(cost.peak_bytes, (long long)live); };
  std::vector<size_t> mine_bytes;
  for (int k = 0; k < kPlaceInputSets && rc == CLOUDSC_OK; k++) {
    cloudsc_fields_t cand = s->f;
    void* cand_pl = s->plude_pristine;
    void** cf = (void**)&cand;
    int order[64];
    for (int q = 0; q < n; q++) order[q] = q;
    if (k > 0)
      for (int q = n - 1; q > 0; q--) std::swap(order[q], order[next() % (q + 1)]);
    int got = 0;
    for (int i = 0; i < n; i++) {
      const int q = order[i];
      if (k > 0) {
        void* sp = nullptr;
        const size_t sb = ((size_t)1 + next() % 16) << 21;
        if (dev_malloc(&sp, sb) != hipSuccess) { (void)hipGetLastError(); break; }
        spacers.push_back(sp);
        live += sb;
        note();
      }
      void* p = nullptr;
      if (dev_malloc(&p, bytes[q]) != hipSuccess) { (void)hipGetLastError(); break; }
      mine.push_back(p);
      mine_bytes.push_back(bytes[q]);
      live += bytes[q];
      note();
      void*& src = slot(sf, s->plude_pristine, members[q]);
      if (hipMemcpyAsync(p, src, bytes[q], hipMemcpyDeviceToDevice, s->stream) != hipSuccess) {
        rc = CLOUDSC_EHIP;
        break;
      }
      slot(cf, cand_pl, members[q]) = p;
      got++;
    }
    if (rc != CLOUDSC_OK || got < n) break;
    const float t = probe_kernel(s, cand, cand_pl);
    cost.launches += 3;
    s->place_tries += n;
    if (t < 0.f) { rc = CLOUDSC_EHIP; break; }
    // the set that loses -- this candidate, or the one it beats -- is freed
    // at once (the transient footprint); the spacers, held to the
    // end, keep the next candidate off its pages
    cloudsc_fields_t lose_f = cand;
    void* lose_pl = cand_pl;
    if (t < best * 0.99f) {
      lose_f = best_f; lose_pl = best_pl;
      best = t; best_f = cand; best_pl = cand_pl; s->place_moves += n;
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess) { rc = CLOUDSC_EHIP; break; }
    void** lf = (void**)&lose_f;
    for (int q = 0; q < n; q++) {
      void* p = slot(lf, lose_pl, members[q]);
      for (size_t j = 0; j < mine.size(); j++)
        if (mine[j] == p) {       // a candidate of this search (not one of the state's own buffers)
          dev_free(p);
          live -= mine_bytes[j];
          mine[j] = mine.back(); mine.pop_back();
          mine_bytes[j] = mine_bytes.back(); mine_bytes.pop_back();
          break;
        }
    }
  }
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == CLOUDSC_OK) rc = CLOUDSC_EHIP;
  for (void* p : spacers) dev_free(p);
  // as for the outputs: hand-off timeouts in the probes keep the first placement
  if (rc == CLOUDSC_OK) {
    const int hc = kseg_check(s->device, s->stream, s->kseg_ws);
    if (hc == CLOUDSC_EHANDOFF) { best_f = s->f; best_pl = s->plude_pristine; best = s->place_final_ms; }
    else rc = hc;
  }
  if (rc != CLOUDSC_OK) { best_f = s->f; best_pl = s->plude_pristine; }
  void** bf = (void**)&best_f;
  for (int q = 0; q < n; q++) {          // adopt the chosen set, free the originals it replaces
    void*& cur = slot(sf, s->plude_pristine, members[q]);
    void* chosen = slot(bf, best_pl, members[q]);
    if (chosen == cur) continue;
    dfree(s, cur);
    s->allocs.push_back(chosen);
    cur = chosen;
  }
  for (void* p : mine) {
    bool kept = false;
    for (void* q : s->allocs) kept = kept || q == p;
    if (!kept) dev_free(p);
  }
  if (rc == CLOUDSC_OK) s->place_final_ms = best;
  cost.search_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// upload one template array and expand it into the block-layout device field
int expand_into(cloudsc_gpu_state* s, void* dst, const void* host_src, int nlev, bool is_int) {
  const size_t src_bytes = (size_t)nlev * s->klon * (is_int ? sizeof(int) : sizeof(double));
  void* d_src = nullptr;
  HIPCHK(dev_malloc(&d_src, src_bytes));
  hipError_t e = hipMemcpyAsync(d_src, host_src, src_bytes, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) {
    // 1-D grid, enough workgroups to fill the chip, the kernel strides the rest
    const long long total = (long long)nlev * s->nproma * s->nblocks;
    const long long want = (total + 255) / 256;
    dim3 grid((unsigned)(want < 16384 ? want : 16384));
    if (is_int)
      hipLaunchKernelGGL((expand_kernel<int, int>), grid, dim3(256), 0, s->stream, (int*)dst, (const int*)d_src,
                         nlev, s->klon, s->nproma, s->col_offset, (long long)s->nblocks);
    else if (s->es == sizeof(double))
      hipLaunchKernelGGL((expand_kernel<double, double>), grid, dim3(256), 0, s->stream, (double*)dst,
                         (const double*)d_src, nlev, s->klon, s->nproma, s->col_offset, (long long)s->nblocks);
    else
      hipLaunchKernelGGL((expand_kernel<float, double>), grid, dim3(256), 0, s->stream, (float*)dst,
                         (const double*)d_src, nlev, s->klon, s->nproma, s->col_offset, (long long)s->nblocks);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  }
  dev_free(d_src);
  if (e != hipSuccess) return hip_fail(e, "expand");
  return CLOUDSC_OK;
}

}  // namespace

extern "C" {

int cloudsc_state_create(cloudsc_gpu_state_t** out, int device, int precision, int ngptot, int nproma,
                         long long col_offset, const cloudsc_template_t* t, const cloudsc_params_t* params) {
  if (!out || !t || !params || col_offset < 0) return CLOUDSC_EINVAL;
  *out = nullptr;
  int rc = check_params(params);
  if (rc) return rc;
  rc = validate_run_args(device, precision, CLOUDSC_VARIANT_KSEG, ngptot, nproma, t->klev);
  if (rc) return rc;
  if (t->klon <= 0) return CLOUDSC_EINVAL;
  const void* tmpl[kNumFields] = {};   // the template array of each cloudsc_fields_t member (NULL: none, or absent)
#define TEMPLATE_OF(n) tmpl[CLOUDSC_M_##n] = t->n;
  CLOUDSC_TEMPLATE_ORDER(TEMPLATE_OF)
  for (int m = 0; m < kNumFields; m++) {
    const int dir = kFieldTable[m].dir;
    if (dir != CLOUDSC_FD_OUT && dir != CLOUDSC_FD_AEROSOL && !tmpl[m]) return CLOUDSC_EINVAL;
  }
  if (params->laericesed && !t->pre_ice) return CLOUDSC_EINVAL;
  if (params->laericeauto && (!t->picrit_aer || !t->pnice)) return CLOUDSC_EINVAL;

  cloudsc_gpu_state* s = new cloudsc_gpu_state();
  s->device = device; s->precision = precision; s->ngptot = ngptot; s->nproma = nproma;
  s->klev = t->klev; s->klon = t->klon; s->col_offset = col_offset;
  s->nblocks = ngptot / nproma + (ngptot % nproma ? 1 : 0);
  s->es = precision_storage_bytes(precision);
  std::memset(&s->f, 0, sizeof(s->f));
  auto fail = [&](int r) { cloudsc_state_destroy(s); return r; };
  if (hipSetDevice(device) != hipSuccess) return fail(CLOUDSC_ENODEV);
  if ((rc = param_set_upload(&s->params, device, params))) return fail(rc);
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) return fail(CLOUDSC_EHIP);
  if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) return fail(CLOUDSC_EHIP);

  const int kl = s->klev;
  void** fp = (void**)&s->f;
  for (int m = 0; m < kNumFields; m++)
    s->fbytes[m] = field_elems(s, kFieldTable[m].kind) * (kFieldTable[m].is_int ? sizeof(int) : s->es);
  // The order of the device allocations is behaviour, and the placement searches get it too: the
  // template's inputs in member order, the pristine plude copy (member -1) last among them, plude and the outputs
  int imem[kNumFields + 1], irow[kNumFields + 1], outs[kNumFields], nin = 0, no = 0;
  size_t ibytes[kNumFields + 1], obytes[kNumFields], in_set = 0, out_set = 0;
  auto add_input = [&](int member, int row) {   // row: the table row of its shape and template array
    imem[nin] = member;
    irow[nin] = row;
    in_set += ibytes[nin++] = s->fbytes[row];
  };
  for (int m = 0; m < kNumFields; m++) {
    const int dir = kFieldTable[m].dir;
    if ((dir == CLOUDSC_FD_IN || dir == CLOUDSC_FD_AEROSOL) && tmpl[m]) add_input(m, m);
    if (dir == CLOUDSC_FD_INOUT || dir == CLOUDSC_FD_OUT) {
      outs[no] = m;
      out_set += obytes[no++] = s->fbytes[m];
    }
  }
  add_input(-1, CLOUDSC_M_plude);
  Arena ar;
  ar.stagger = g_layout_stagger.load();
  if (ar.stagger >= 0) {
    size_t total = 0;
    for (int q = 0; q < nin; q++) total += arena_span(ibytes[q]);
    for (int q = 0; q < no; q++) total += arena_span(obytes[q]);
    void* base = nullptr;
    if ((rc = dalloc(s, &base, total))) return fail(rc);
    ar.base = (char*)base;
  }
  for (int q = 0; q < nin; q++) {
    const FieldDesc& d = kFieldTable[irow[q]];
    void* p = nullptr;
    if ((rc = field_alloc(s, ar, &p, ibytes[q]))) return fail(rc);
    if ((rc = expand_into(s, p, tmpl[irow[q]], (int)per_block_elems(d.kind, 1, kl), d.is_int))) return fail(rc);
    (imem[q] < 0 ? s->plude_pristine : fp[imem[q]]) = p;
  }
  for (int q = 0; q < no; q++)
    if ((rc = field_alloc(s, ar, &fp[outs[q]], obytes[q]))) return fail(rc);
  if (!ar.base && g_place_passes.load() > 0) {   // one allocation per field: search for a fast placement
    // the KSEG workspace the search's launches use (and later KSEG runs)
    const long long wsb = cloudsc_gpu_scratch_bytes(s->precision, CLOUDSC_VARIANT_KSEG, ngptot, nproma, kl);
    if (wsb <= 0) return fail(CLOUDSC_EINVAL);
    if ((rc = dalloc(s, &s->kseg_ws, (size_t)wsb))) return fail(rc);
    if (hipMemsetAsync(s->kseg_ws, 0, 256, s->stream) != hipSuccess) return fail(CLOUDSC_EHIP);
    // no room for two candidate sets and their spacers next to the state: no
    // search (cloudsc_state_placement_report then says NONE)
    const size_t budget = std::max(search_transient_bytes(out_set, no, kPlaceSets),
                                   search_transient_bytes(in_set, nin, kPlaceInputSets));
    const bool room = search_fits(budget);
    if (room) s->pcost.budget_bytes = (long long)budget;
    if (room && (rc = place_outputs(s, outs, obytes, no))) return fail(rc);
    // then the inputs (contents copied) and the pristine plude copy
    if (room && (rc = place_inputs(s, imem, ibytes, nin))) return fail(rc);
  }
  for (int q = 0; q < no; q++)   // NaN
    if (hipMemsetAsync(fp[outs[q]], 0xff, obytes[q], s->stream) != hipSuccess) return fail(CLOUDSC_EHIP);
  if (hipMemcpyAsync(s->f.plude, s->plude_pristine, s->fbytes[CLOUDSC_M_plude], hipMemcpyDeviceToDevice, s->stream) !=
      hipSuccess)
    return fail(CLOUDSC_EHIP);
  if (hipStreamSynchronize(s->stream) != hipSuccess) return fail(CLOUDSC_EHIP);
  *out = s;
  return CLOUDSC_OK;
}

int cloudsc_debug_set_state_layout(long long stagger, unsigned alloc_flags) {
  // Allocation flags are refused by the product library (the diagnostic build,
  // -DCLOUDSC_DEBUG_KNOBS, admits them to reproduce the following).  After
  // states whose fields were hipDeviceMallocContiguous allocations had been
  // destroyed, later states computed wrong values.  Two causes were found
  // (profiles/r04/contiguous_alloc_hazard.txt): the round-3 parameter upload
  // (a null-stream hipMemcpy from pageable memory, unordered with the launches;
  // fixed in param_set_upload -- re-introducing it makes the failure reappear),
  // and a second one that remains with the fix in one order of states: the
  // input fields of a new state (plain hipMalloc) hold wrong words right after
  // its expansion, with no live allocations overlapping, also with every kernel
  // and copy serialized (AMD_SERIALIZE_KERNEL/COPY=3), KCACHE as KSEG; a
  // standalone HIP program with the same allocation pattern does not reproduce
  // it.  Unexplained; the library never allocates with flags.
  // A stagger must keep every field aligned for the widest element (a multiple
  // of 256 bytes) and is taken modulo the 2 MiB arena alignment.
  if (stagger >= 0 && stagger % 256 != 0) return CLOUDSC_EINVAL;
#ifdef CLOUDSC_DEBUG_KNOBS
  g_alloc_flags.store(alloc_flags);
#else
  if (alloc_flags != 0) return CLOUDSC_EINVAL;
#endif
  g_layout_stagger.store(stagger < 0 ? -1 : stagger % (long long)kArenaAlign);
  return CLOUDSC_OK;
}

int cloudsc_state_placement(const cloudsc_gpu_state_t* s, float* probe_first_ms, float* probe_final_ms,
                            int* tries, int* moves) {
  if (!s) return CLOUDSC_EINVAL;
  if (probe_first_ms) *probe_first_ms = s->place_first_ms;
  if (probe_final_ms) *probe_final_ms = s->place_final_ms;
  if (tries) *tries = s->place_tries;
  if (moves) *moves = s->place_moves;
  return CLOUDSC_OK;
}

int cloudsc_state_placement_report(const cloudsc_gpu_state_t* s, cloudsc_placement_t* r) {
  if (!s || !r) return CLOUDSC_EINVAL;
  std::memset(r, 0, sizeof(*r));
  r->probe_first_ms = s->place_first_ms;
  r->probe_final_ms = s->place_final_ms;
  r->tries = s->place_tries;
  r->moves = s->place_moves;
  r->launches = s->pcost.launches;
  r->search_ms = s->pcost.search_ms;
  r->peak_transient_bytes = s->pcost.peak_bytes;
  r->transient_budget_bytes = s->pcost.budget_bytes;
  r->method = s->pcost.launches ? CLOUDSC_PLACE_METHOD_KERNEL : CLOUDSC_PLACE_METHOD_NONE;
  return CLOUDSC_OK;
}

int cloudsc_set_placement_search(int passes) {
  if (passes > 8) return CLOUDSC_EINVAL;
  g_place_passes.store(passes < 0 ? 2 : passes);
  return CLOUDSC_OK;
}

int cloudsc_debug_set_placement_search(int passes) { return cloudsc_set_placement_search(passes); }

int cloudsc_debug_state_relocate_field(cloudsc_gpu_state_t* s, int member) {
  const int nmem = (int)(sizeof(s->fbytes) / sizeof(s->fbytes[0]));
  if (!s || member < 0 || member >= nmem) return CLOUDSC_EINVAL;
  void** slot = (void**)&s->f + member;
  const size_t bytes = s->fbytes[member];
  if (!*slot || !bytes) return CLOUDSC_EINVAL;
  HIPCHK(hipSetDevice(s->device));
  // the old allocation stays with the state until it is destroyed, so the copy
  // lands on other physical pages
  void* q = nullptr;
  int rc = dalloc(s, &q, bytes);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(q, *slot, bytes, hipMemcpyDeviceToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *slot = q;
  return CLOUDSC_OK;
}

// Diagnostic: move one of the state's buffers that are not fields to fresh
// memory (the old one stays with the state until it is destroyed): which = 0
// the pristine plude copy, 1 the KSEG workspace (zeroed again before the next
// launch), 2 the SCC temporaries.
int cloudsc_debug_state_relocate_aux(cloudsc_gpu_state_t* s, int which) {
  if (!s || which < 0 || which > 2) return CLOUDSC_EINVAL;
  void** slot = which == 0 ? &s->plude_pristine : which == 1 ? &s->kseg_ws : &s->scratch;
  if (!*slot) return CLOUDSC_EINVAL;
  const size_t bytes =
      which == 0 ? s->fbytes[CLOUDSC_M_plude]
                 : (size_t)cloudsc_gpu_scratch_bytes(s->precision, which == 1 ? CLOUDSC_VARIANT_KSEG : CLOUDSC_VARIANT_SCC,
                                                     s->ngptot, s->nproma, s->klev);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  void* q = nullptr;
  int rc = dalloc(s, &q, bytes);
  if (rc) return rc;
  if (which == 0) HIPCHK(hipMemcpyAsync(q, *slot, bytes, hipMemcpyDeviceToDevice, s->stream));
  if (which == 1) {
    HIPCHK(hipMemsetAsync(q, 0, 256, s->stream));
    s->kseg_epoch.ready = false;
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  *slot = q;
  return CLOUDSC_OK;
}

int cloudsc_state_fields(const cloudsc_gpu_state_t* s, cloudsc_fields_t* out) {
  if (!s || !out) return CLOUDSC_EINVAL;
  *out = s->f;
  return CLOUDSC_OK;
}

int cloudsc_state_reset(cloudsc_gpu_state_t* s) {
  if (!s) return CLOUDSC_EINVAL;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpyAsync(s->f.plude, s->plude_pristine, s->fbytes[CLOUDSC_M_plude], hipMemcpyDeviceToDevice,
                        s->stream));
  return CLOUDSC_OK;
}

#if defined(CLOUDSC_DEBUG_KNOBS) || defined(CLOUDSC_DEBUG_LAUNCH_FORMS)
// Diagnostic (debug builds only): the time between consecutive physics launches.
// `reps` launches back to back, timed as a whole by two stream events; mode 0 =
// the product form (each dispatch records its own event pair), 1 = plain
// dispatches, 2 = one hipGraph holding the workspace reset and the `reps`
// launches (KSEG's epoch arguments are baked into the graph, so the graph
// starts from a zeroed workspace), replayed once for warm-up and once timed.
int cloudsc_debug_launch_forms(cloudsc_gpu_state_t* s, int variant, int reps, int mode, double* ms) {
  if (!s || reps <= 0 || mode < 0 || mode > 2 || !ms) return CLOUDSC_EINVAL;
  int rc = cloudsc_state_run(s, variant, 1, nullptr);   // workspace allocated and warm
  if (rc) return rc;
  void* scratch = variant_kind(variant) == CLOUDSC_VARIANT_SCC ? s->scratch
                  : variant_kind(variant) == CLOUDSC_VARIANT_KSEG ? s->kseg_ws : nullptr;
  hipEvent_t t0, t1;
  HIPCHK(hipEventCreate(&t0));
  HIPCHK(hipEventCreate(&t1));
  std::vector<hipEvent_t> ev(2 * (size_t)reps);
  for (auto& e : ev) HIPCHK(hipEventCreate(&e));
  auto issue = [&](bool events) {
    int r0 = CLOUDSC_OK;
    for (int r = 0; r < reps && r0 == CLOUDSC_OK; r++) {
      const LaunchEvents lev{ev[2 * r], ev[2 * r + 1]};
      r0 = gpu_run_impl(s->device, s->stream, {s->precision, variant, s->ngptot, s->nproma, s->klev}, &s->f, scratch, {},
                        {s->plude_pristine, &s->params, &s->kseg_epoch, events ? &lev : nullptr});
    }
    return r0;
  };
  float t = 0.f;
  if (mode < 2) {
    HIPCHK(hipEventRecord(t0, s->stream));
    rc = issue(mode == 0);
    HIPCHK(hipEventRecord(t1, s->stream));
  } else {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    s->kseg_epoch.ready = false;   // the graph's first launch zeroes the workspace
    HIPCHK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    rc = issue(false);
    HIPCHK(hipStreamEndCapture(s->stream, &g));
    if (rc == CLOUDSC_OK) HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    if (rc == CLOUDSC_OK) HIPCHK(hipGraphLaunch(ge, s->stream));
    HIPCHK(hipEventRecord(t0, s->stream));
    if (rc == CLOUDSC_OK) HIPCHK(hipGraphLaunch(ge, s->stream));
    HIPCHK(hipEventRecord(t1, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    s->kseg_epoch.ready = false;   // the device counters no longer match the host's epoch
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  HIPCHK(hipEventElapsedTime(&t, t0, t1));
  *ms = t / reps;
  for (auto& e : ev) (void)hipEventDestroy(e);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  if (rc == CLOUDSC_OK && variant_kind(variant) == CLOUDSC_VARIANT_KSEG)
    rc = kseg_check(s->device, s->stream, scratch);
  return rc;
}
#endif

// The launches of cloudsc_state_run (per_launch: each dispatch records its own
// event pair, ms[r]; ms may be NULL, then plain dispatches) and of
// cloudsc_state_run_span (plain dispatches bracketed by two stream events,
// *span_ms).  A dispatch that records events costs ~5 us more between kernels
// than a plain one (fp64 6.2 against 1.3 us above the kernel's duration,
// fp32 5.3 against 0.7 us; profiles/r05/launch_forms.txt).
static int state_launches(cloudsc_gpu_state_t* s, int variant, int reps, float* ms, float* span_ms) {
  if (!s || reps <= 0) return CLOUDSC_EINVAL;
  HIPCHK(hipSetDevice(s->device));
  void* scratch = nullptr;
  const int vk = variant_kind(variant);   // without the option bits
  if (vk == CLOUDSC_VARIANT_SCC || vk == CLOUDSC_VARIANT_KSEG) {   // workspaces, allocated on first use
    void*& ws = vk == CLOUDSC_VARIANT_SCC ? s->scratch : s->kseg_ws;
    if (!ws) {
      const long long nb = cloudsc_gpu_scratch_bytes(s->precision, vk, s->ngptot, s->nproma, s->klev);
      if (nb <= 0) return CLOUDSC_EINVAL;
      int rc0 = dalloc(s, &ws, (size_t)nb);
      if (rc0) return rc0;
      HIPCHK(hipMemsetAsync(ws, 0, 256, s->stream));   // control words (the first launch zeroes the rest)
    }
    scratch = ws;
  }
  // per-launch pairs, or the two bracketing events of a span
  std::vector<hipEvent_t> ev(ms ? 2 * (size_t)reps : span_ms ? 2 : 0);
  int rc = CLOUDSC_OK;
  for (auto& e : ev) {
    hipError_t ce = hipEventCreate(&e);
    if (ce != hipSuccess) { e = nullptr; rc = hip_fail(ce, "hipEventCreate"); }
  }
  if (rc == CLOUDSC_OK && span_ms) {
    hipError_t re = hipEventRecord(ev[0], s->stream);
    if (re != hipSuccess) rc = hip_fail(re, "hipEventRecord");
  }
  for (int r = 0; r < reps && rc == CLOUDSC_OK; r++) {
    // out of place: every step reads the pristine plude and writes the INOUT
    // result to f.plude, so repeated steps see the same input with no restore copy
    const LaunchEvents lev{ms ? ev[2 * r] : nullptr, ms ? ev[2 * r + 1] : nullptr};
    rc = gpu_run_impl(s->device, s->stream, {s->precision, variant, s->ngptot, s->nproma, s->klev}, &s->f, scratch, {},
                      {s->plude_pristine, &s->params, &s->kseg_epoch, ms ? &lev : nullptr});
  }
  if (rc == CLOUDSC_OK && span_ms) {
    hipError_t re = hipEventRecord(ev[1], s->stream);
    if (re != hipSuccess) rc = hip_fail(re, "hipEventRecord");
  }
  hipError_t e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess && rc == CLOUDSC_OK) rc = hip_fail(e, "hipStreamSynchronize");
  for (int r = 0; ms && r < reps && rc == CLOUDSC_OK; r++) {
    e = hipEventElapsedTime(&ms[r], ev[2 * r], ev[2 * r + 1]);
    if (e != hipSuccess) rc = hip_fail(e, "hipEventElapsedTime");
  }
  if (span_ms && rc == CLOUDSC_OK) {
    e = hipEventElapsedTime(span_ms, ev[0], ev[1]);
    if (e != hipSuccess) rc = hip_fail(e, "hipEventElapsedTime");
  }
  for (auto& x : ev)
    if (x) (void)hipEventDestroy(x);
  if (rc == CLOUDSC_OK && vk == CLOUDSC_VARIANT_KSEG) {
    // a segment whose predecessor never arrived gives up after a bounded spin
    // and counts itself in the workspace's error word: its results are
    // invalid.  The count accumulates over the reps of this call (the word is
    // sticky across launches); kseg_check reads and clears it, and any failure
    // resets kseg_epoch (below), so the next call zeroes the workspace again.
    rc = kseg_check(s->device, s->stream, scratch);
  }
  if (rc != CLOUDSC_OK) s->kseg_epoch.ready = false;   // zero the workspace again before the next launch
  return rc;
}

int cloudsc_state_run(cloudsc_gpu_state_t* s, int variant, int reps, float* ms) {
  return state_launches(s, variant, reps, ms, nullptr);
}

int cloudsc_state_run_span(cloudsc_gpu_state_t* s, int variant, int reps, float* span_ms) {
  if (!span_ms) return CLOUDSC_EINVAL;
  return state_launches(s, variant, reps, nullptr, span_ms);
}

int cloudsc_state_kseg_clock(cloudsc_gpu_state_t* s, int reset, double* ghz) {
  if (!s || !ghz) return CLOUDSC_EINVAL;
  *ghz = 0.0;
  if (!s->kseg_ws) {   // no KSEG launch yet: nothing measured; a reset is a no-op
    return CLOUDSC_OK;
  }
  return kseg_clock(s->device, s->stream, s->kseg_ws, reset != 0, ghz, nullptr);
}

int cloudsc_state_sync(cloudsc_gpu_state_t* s) {
  if (!s) return CLOUDSC_EINVAL;
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  return CLOUDSC_OK;
}

long long cloudsc_state_field_elems(const cloudsc_gpu_state_t* s, int id) {
  if (!s || id < 0 || id >= CLOUDSC_NVALID) return -1;
  return (long long)field_elems(s, kFieldTable[valid_member(id)].kind);
}

int cloudsc_state_download(cloudsc_gpu_state_t* s, int id, double* host) {
  if (!s || !host || id < 0 || id >= CLOUDSC_NVALID) return CLOUDSC_EINVAL;
  HIPCHK(hipSetDevice(s->device));
  const int m = valid_member(id);
  const void* src = ((void* const*)&s->f)[m];
  const size_t n = field_elems(s, kFieldTable[m].kind);
  HIPCHK(hipStreamSynchronize(s->stream));
  if (s->es == sizeof(double)) {
    HIPCHK(hipMemcpy(host, src, n * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    std::vector<float> tmp(n);
    HIPCHK(hipMemcpy(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) host[i] = tmp[i];
  }
  return CLOUDSC_OK;
}

int cloudsc_state_validate(cloudsc_gpu_state_t* s, const cloudsc_reference_t* ref, cloudsc_stats_t* stats) {
  if (!s || !ref || !stats || ref->klon <= 0 || ref->klev != s->klev) return CLOUDSC_EINVAL;
  return cloudsc_fields_validate(s->device, s->stream, s->precision, s->ngptot, s->nproma, s->klev, s->col_offset,
                                 &s->f, ref, stats);
}

void cloudsc_stats_combine(cloudsc_stats_t* acc, const cloudsc_stats_t* p) {
  if (!acc || !p) return;
  acc->minval = fmin(acc->minval, p->minval);
  acc->maxval = fmax(acc->maxval, p->maxval);
  acc->maxerr = fmax(acc->maxerr, p->maxerr);
  const DD e = dd_add(DD{acc->errsum, acc->errsum_lo}, DD{p->errsum, p->errsum_lo});
  const DD r = dd_add(DD{acc->refsum, acc->refsum_lo}, DD{p->refsum, p->refsum_lo});
  acc->errsum = e.hi; acc->errsum_lo = e.lo;
  acc->refsum = r.hi; acc->refsum_lo = r.lo;
}

int cloudsc_state_destroy(cloudsc_gpu_state_t* s) {
  if (!s) return CLOUDSC_OK;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : s->allocs) dev_free(p);
  param_set_free(&s->params);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
  return CLOUDSC_OK;
}

}  // extern "C"

