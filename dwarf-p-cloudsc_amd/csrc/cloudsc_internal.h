// cloudsc_internal.h -- host-side internals shared by the translation units of
// libcloudsc_amd.so (kernels + low-level ABI, device-resident state, host
// pipeline).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <type_traits>

#include "cloudsc_amd.h"
#include "cloudsc_fields.def"

namespace cloudsc {
// the bits of a k-caching kernel's form (KForm, cloudsc_kcache.h)
enum : unsigned { kFormPack = 1u, kFormTb = 2u, kFormProg = 4u, kFormSurf = 8u, kFormCml = 16u, kFormSpp = 32u, kFormAdv = 64u };
}  // namespace cloudsc

namespace cloudsc_impl {

constexpr int kMaxDevices = 64;

// The fields of cloudsc_fields_t in member order, generated from the one inventory (cloudsc_fields.def,
// which also holds CLOUDSC_FK_* / CLOUDSC_FD_* and binds its lists to include/cloudsc_amd.h)
struct FieldDesc { const char* name; int kind, dir, is_int; };
#define CLOUDSC_FIELD_DESC(n, N, k, d, i) {#n, CLOUDSC_FK_##k, CLOUDSC_FD_##d, i},
inline constexpr FieldDesc kFieldTable[] = {CLOUDSC_FIELDS(CLOUDSC_FIELD_DESC)};
inline constexpr int kNumFields = CLOUDSC_NFIELDS;

// fields of `kind` whose direction is in the bit set dirs (1 << FD_*)
constexpr int count_fields(int kind, int dirs) {
  int n = 0;
  for (const FieldDesc& d : kFieldTable) n += d.kind == kind && (dirs >> d.dir & 1);
  return n;
}

// What a precision code means, in one place: the bytes of a real field element
// in memory (0: not a precision code) and the type the physics computes in.
// CLOUDSC_MIXED stores float and computes double.
inline size_t precision_storage_bytes(int precision) {
  switch (precision) {
    case CLOUDSC_FP64: return sizeof(double);
    case CLOUDSC_FP32:
    case CLOUDSC_MIXED: return sizeof(float);
    default: return 0;
  }
}
inline bool precision_computes_double(int precision) { return precision != CLOUDSC_FP32; }

inline size_t per_block_elems(int kind, int nproma, int klev) {
  switch (kind) {
    case CLOUDSC_FK_LEVEL: return (size_t)klev * nproma;
    case CLOUDSC_FK_HALF: return (size_t)(klev + 1) * nproma;
    case CLOUDSC_FK_SPECIES: return (size_t)CLOUDSC_NCLV * klev * nproma;
    default: return (size_t)nproma;
  }
}

// One parameter set on one device: the host-folded fp64 and fp32 DevParams
// blocks in device memory (read by the kernels through a KArgs pointer), plus
// the host-side values the launch itself needs.
struct ParamSet {
  void* dev = nullptr;     // device block (fp64 mirror at 0, fp32 mirror after it)
  int device = -1;
  bool aer = false;        // LAERICESED || LAERICEAUTO: aerosol inputs are read
  int ncldtop = 0;         // NCLDTOP (KSEG segment bounds)
  double ptsphy = 0.0;     // PTSPHY (cloudsc_fields_advance)
};
int check_params(const cloudsc_params_t* p);
// (re)upload `p` into ps (allocated on first use) on `device`; synchronous
int param_set_upload(ParamSet* ps, int device, const cloudsc_params_t* p);
// copy of another set on the same device (device-to-device)
int param_set_copy(ParamSet* dst, const ParamSet* src);
void param_set_free(ParamSet* ps);
// the device's default set (cloudsc_gpu_init), NULL if never initialised
const ParamSet* device_default_params(int device);

// records "what: hip error string" for cloudsc_last_hip_error(); returns CLOUDSC_EHIP
int hip_fail(hipError_t e, const char* what);
// sets the cloudsc_last_hip_error() text for a failure that is not a HIP error
void set_error_text(const char* text);
// device / precision / variant / size checks shared by every entry point
int validate_run_args(int device, int precision, int variant, int ngptot, int nproma, int klev);
// the checks of validate_run_args that need no device (`variant`: a kind, without option bits)
int validate_shape_args(int precision, int variant, int ngptot, int nproma, int klev);

// ---- the batched KCACHE launch (cloudsc_batch.hip owns the table, cloudsc_gpu.hip the kernels) ----
// a parameter set's device block: its size, and its host image (the fp64 mirror, then the fp32 one)
size_t param_block_bytes();
void param_block_fill(char* block, const cloudsc_params_t& p);
// One entry of a batch's device table: the kernel arguments cloudsc_gpu_run_outputs would pass for f, with `par`
// pointing into the device parameter block `param_block`; entries are batch_entry_stride() bytes apart
size_t batch_entry_stride();
void batch_make_entry(int precision, void* entry, const cloudsc_fields_t* f, int ngptot, int nproma, int klev,
                      const void* param_block);
struct BatchLaunch {
  int precision, outputs, nsets, ngptot, nproma, klev;
  bool aer;            // LAERICESED || LAERICEAUTO of every member's parameters
  const void* table;   // device: nsets entries
};
// one launch on `stream`, no upload, no allocation; the caller has set the device
int launch_kcache_batch(void* stream, const BatchLaunch& b);

// The ten diagnostic flux members pfsqlf ... pfsqitur (consecutive in cloudsc_fields_t): running sums of
// section 8 that nothing in the step reads back; CLOUDSC_OUTPUTS_PROGNOSTIC leaves them out
constexpr bool is_flux_diagnostic(int member) { return member >= CLOUDSC_M_pfsqlf && member <= CLOUDSC_M_pfsqitur; }
static_assert(CLOUDSC_M_pfsqitur - CLOUDSC_M_pfsqlf + 1 == 10 && CLOUDSC_M_pfplsl == CLOUDSC_M_pfsqitur + 1,
              "the diagnostic flux members");
// The output selections are bit sets (cloudsc_amd.h): the three known values, and their two bits
constexpr bool outputs_known(int outputs) {
  return outputs == CLOUDSC_OUTPUTS_ALL || outputs == CLOUDSC_OUTPUTS_PROGNOSTIC || outputs == CLOUDSC_OUTPUTS_SURFACE;
}
constexpr bool outputs_prognostic(int outputs) { return (outputs & CLOUDSC_OUTPUTS_PROGNOSTIC) != 0; }
constexpr bool outputs_surface(int outputs) { return (outputs & CLOUDSC_OUTPUTS_SURFACE_BIT) != 0; }
static_assert(CLOUDSC_OUTPUTS_SURFACE == (CLOUDSC_OUTPUTS_PROGNOSTIC | CLOUDSC_OUTPUTS_SURFACE_BIT), "the selection bits");
// The four precipitation / enthalpy flux members (consecutive): half-level profiles, or, with
// CLOUDSC_OUTPUTS_SURFACE, surface fields that hold the profiles' last row
constexpr bool is_surface_flux(int member) { return member >= CLOUDSC_M_pfplsl && member <= CLOUDSC_M_pfhpsn; }
static_assert(CLOUDSC_M_pfhpsn - CLOUDSC_M_pfplsl + 1 == 4, "the surface flux members");
// the shape kind of member m under a selection: the inventory's, overridden for the four members above
constexpr int field_kind_of(int member, int outputs) {
  return outputs_surface(outputs) && is_surface_flux(member) ? (int)CLOUDSC_FK_SURFACE : kFieldTable[member].kind;
}
// whether an output selection (CLOUDSC_OUTPUTS_*) touches member m
constexpr bool output_selected(int member, int outputs) {
  return !outputs_prognostic(outputs) || !is_flux_diagnostic(member);
}
// The four local tendency members (consecutive): the cumulative tendency form never touches them
constexpr bool is_tendency_loc(int member) { return member >= CLOUDSC_M_tendency_loc_t && member <= CLOUDSC_M_tendency_loc_cld; }

// The form of one step, on the GPU and on the CPU: what every run entry says beyond the shape.  The default is
// cloudsc_gpu_run's: separate tendency arrays, every output, the local tendencies stored.
struct StepForm {
  int tend_planes = 0;                      // != 0: tendency members are planes of packed buffers
  int outputs = CLOUDSC_OUTPUTS_ALL;        // CLOUDSC_OUTPUTS_*
  const cloudsc_tend_cml_t* cml = nullptr;  // the cumulative tendency planes
  const cloudsc_spp_t* spp = nullptr;       // the per-column parameter multipliers
  const cloudsc_advance_t* adv = nullptr;   // the advancing form: where the updated prognostics go
};
// a form's kForm* bits (kFormPack is the launch's own, not a form's)
constexpr unsigned form_bits(bool tb, bool prog, bool surf, bool cml, bool spp = false, bool adv = false) {
  using namespace cloudsc;
  return (tb ? kFormTb : 0u) | (prog ? kFormProg : 0u) | (surf ? kFormSurf : 0u) | (cml ? kFormCml : 0u) |
         (spp ? kFormSpp : 0u) | (adv ? kFormAdv : 0u);
}
constexpr unsigned form_bits(const StepForm& s) {
  return form_bits(s.tend_planes != 0, outputs_prognostic(s.outputs), outputs_surface(s.outputs), s.cml != nullptr,
                   s.spp != nullptr, s.adv != nullptr);
}
// The support matrix, the part the bits alone decide: the surface-fluxes form is a prognostic-outputs form, the
// cumulative tendency form a tendency buffer, prognostic-outputs form, the per-column multiplier form stands alone or
// with the prognostic-outputs form only, the advancing form stands alone or with the surface-fluxes form only
// (KForm's static_asserts)
constexpr bool form_bits_consistent(unsigned form) {
  using namespace cloudsc;
  return (!(form & kFormSurf) || (form & kFormProg)) && (!(form & kFormCml) || ((form & kFormTb) && (form & kFormProg))) &&
         (!(form & kFormSpp) || !(form & (kFormTb | kFormSurf | kFormCml))) &&
         (!(form & kFormAdv) || (!(form & (kFormTb | kFormCml | kFormSpp)) && (!(form & kFormProg) || (form & kFormSurf))));
}
// The support matrix: whether (variant kind, precision, fp32 exact-libm, form bits) has a GPU kernel.  MIXED runs on the
// k-caching variants only; so do the forms, alone or combined, which fp32 has with its default exp/pow only; the SCC
// variants are plain.  (The exact-libm bit means nothing outside fp32; every k-caching kernel has its packed twin, so
// kFormPack is not asked about.)  The CPU variant has every consistent form (cloudsc_cpu.hip).
constexpr bool form_exists(int kind, int precision, bool exact_libm, unsigned form) {
  const bool kcaching = kind == CLOUDSC_VARIANT_KCACHE || kind == CLOUDSC_VARIANT_KSEG;
  if (!kcaching && kind != CLOUDSC_VARIANT_SCC && kind != CLOUDSC_VARIANT_SCC_PRIVATE) return false;
  if (precision != CLOUDSC_FP64 && precision != CLOUDSC_FP32 && precision != CLOUDSC_MIXED) return false;
  if (precision == CLOUDSC_MIXED && !kcaching) return false;
  if (!form_bits_consistent(form)) return false;
  if (form & ~cloudsc::kFormPack) return kcaching && !(precision == CLOUDSC_FP32 && exact_libm);
  return true;
}
// runtime conditions as compile-time constants, in one place:
// dispatch_bools(f, c0, c1, ...) calls f(std::bool_constant<c0>{}, std::bool_constant<c1>{}, ...)
template <bool... Bs, typename Fn>
int dispatch_bools(Fn&& f) {
  return f(std::integral_constant<bool, Bs>{}...);
}
template <bool... Bs, typename Fn, typename... Rest>
int dispatch_bools(Fn&& f, bool c, Rest... rest) {
  return c ? dispatch_bools<Bs..., true>(f, rest...) : dispatch_bools<Bs..., false>(f, rest...);
}

// every pointer the step reads or writes (aerosol inputs, with CLOUDSC_OUTPUTS_PROGNOSTIC the ten diagnostic
// fluxes and, in the cumulative tendency and the advancing form, tendency_loc_t/q/a/cld excepted) is set
bool fields_complete(const cloudsc_fields_t* f, const StepForm& form = {});
// The rules of a form that need neither a shape nor a device, the same for the GPU and the CPU entries: a known
// selection, the bits `need` that the entry stands for, bits that go together, a plane count in range, and the
// pointer rules of the cumulative planes -- cml's four members set, none of them a tendency_tmp_* or
// tendency_loc_* member of f (pointer equality only) -- and of the multipliers -- at least one member of spp set,
// none of them a member of f -- and of the advancing form -- adv's four members set, each its
// own state member of f (pt, pq, pa, pclv: in place) or no member of f at all, no two of them equal.  A form the entry does not stand for (bits outside `need`: a cml or an spp the
// entry never passes) cannot occur.  CLOUDSC_EINVAL or CLOUDSC_OK.
int check_step_form(const StepForm& form, unsigned need, const cloudsc_fields_t* f);
// The pointer rules of cloudsc_advance_t, for the step's entries and for the separate pass (cloudsc_advance.hip): the
// four members set, no two of them equal, each its own state member of f (pt, pq, pa, pclv: in place) or no member
// of f at all.  Pointer equality only.
inline bool advance_members_ok(const cloudsc_fields_t* f, const cloudsc_advance_t* adv) {
  if (!f || !adv || !adv->t || !adv->q || !adv->a || !adv->clv) return false;
  const void* const mine[4] = {adv->t, adv->q, adv->a, adv->clv};
  const int own[4] = {CLOUDSC_M_pt, CLOUDSC_M_pq, CLOUDSC_M_pa, CLOUDSC_M_pclv};
  const void* const* theirs = (const void* const*)f;
  for (int i = 0; i < 4; i++) {
    for (int j = 0; j < i; j++)
      if (mine[i] == mine[j]) return false;
    for (int m = 0; m < kNumFields; m++)
      if (m != own[i] && mine[i] == theirs[m]) return false;
  }
  return true;
}
// Host record of one KSEG workspace owned by a caller that launches on it in
// stream order (a state): after the first launch zeroes it, later launches
// continue its ticket counter and flag stamps instead of zeroing it again.
struct KsegEpoch {
  bool ready = false;       // false: zero the workspace before the next launch
  unsigned base[8] = {};    // per dequeue stripe (kKsegStripes, cloudsc_kcache.h)
  unsigned stamp = 0;
};
// Start/stop events of one launch, recorded by the kernel's own dispatch
// (hipExtLaunchKernelGGL) instead of separate event packets around it.
struct LaunchEvents {
  hipEvent_t start, stop;
};
// The shape arguments of a run entry; `variant` may carry option bits (CLOUDSC_FP32_EXACT_LIBM)
struct StepShape {
  int precision, variant, ngptot, nproma, klev;
};
// What the library's own callers add to a run: a separate source of plude (NULL = in place, the reference INOUT
// semantics; otherwise plude is read from there and the result written to f->plude), an explicit parameter set
// (NULL = the device's default set), a KSEG workspace record (NULL = zero the workspace before every KSEG launch)
// and events timing the physics kernel (NULL = none)
struct RunContext {
  const void* plude_in = nullptr;
  const ParamSet* ps = nullptr;
  KsegEpoch* ep = nullptr;
  const LaunchEvents* lev = nullptr;
};
// cloudsc_gpu_run in the form `form`: the device checks, the argument rules, the launch
int gpu_run_impl(int device, void* stream, const StepShape& shape, const cloudsc_fields_t* f, void* scratch,
                 const StepForm& form, const RunContext& ctx);
// the kernel variant of a `variant` argument without its option bits (CLOUDSC_FP32_EXACT_LIBM)
inline int variant_kind(int variant) { return variant & 0xff; }
// waits for `stream` and returns CLOUDSC_EHANDOFF if the last KSEG launch on
// `scratch` counted a timed-out segment hand-off
int kseg_check(int device, void* stream, void* scratch);
// waits for `stream`; the effective shader clock of the KSEG launches on
// `scratch` since the last reset (sum of shader-clock cycles over sum of
// real-time ticks of the workgroups, times the real-time rate) and the summed
// workgroup-seconds behind it; reset zeroes the sums
int kseg_clock(int device, void* stream, void* scratch, bool reset, double* ghz, double* seconds);

// the memory-pattern probe of cloudsc_place.hip over f on `stream`: best of
// `reps` timed launches after one untimed, ms; mode 0 outputs written only, 1
// inputs read too (every non-NULL output of f is overwritten); strides (6, may
// be NULL): the inputs' and outputs' block / row / species element strides of
// another layout (cloudsc_debug_memory_probe_layout); outputs: CLOUDSC_OUTPUTS_*,
// with PROGNOSTIC the ten diagnostic flux members of f are not looked at
int memory_probe(int device, hipStream_t stream, int precision, int ngptot, int nproma, int klev,
                 const cloudsc_fields_t* f, int mode, int reps, hipEvent_t e0, hipEvent_t e1, float* best_ms,
                 const long long* strides = nullptr, int outputs = CLOUDSC_OUTPUTS_ALL);

// What a placement search cost and found (cloudsc_place.hip)
struct PlaceCost {
  float first_ms = 0.f, final_ms = 0.f;   // probe time of the first / the kept placement
  int tries = 0, moves = 0;               // candidate buffers allocated / kept
  int launches = 0;                       // probe launches (untimed ones included)
  double search_ms = 0.0;                 // wall time of the search
  long long peak_bytes = 0;               // most candidate and spacer bytes held at once
  long long budget_bytes = 0;             // the bound search_fits was asked for (peak_bytes stays below it)
};
// the output placement search (see cloudsc_place.hip): moves f's output
// members (members/bytes: positions in cloudsc_fields_t and sizes) to the
// fastest candidate buffers under `probe` (ms, < 0 on an error); never frees
// the caller's original buffers
int search_outputs(cloudsc_fields_t& f, const int* members, const size_t* bytes, int n, int sets, int passes,
                   uint32_t seed, const std::function<float(const cloudsc_fields_t&)>& probe, PlaceCost& cost);

// Device allocations of the state and the placement searches.  Plain
// hipMalloc / hipExtMallocWithFlags + hipFree; in the diagnostic build
// -DCLOUDSC_DEBUG_CANARY every buffer gets a 64 KiB guard band of a known byte
// on each side, checked by cloudsc_debug_canary_check and at free (the
// round-5 record of the contiguous-allocation failure).
hipError_t dev_malloc(void** p, size_t bytes, unsigned flags = 0);
void dev_free(void* p);

// whether a placement search whose candidates peak at about `transient` bytes
// fits the device's free memory with room to spare (on a device
// shared by several ranks the search must not starve their allocations)
bool search_fits(size_t transient);
// the transient bytes a placement search holds at most over sets of set_bytes
// in n buffers with `sets` whole sets tried: two candidate sets and the spacers
size_t search_transient_bytes(size_t set_bytes, int n, int sets);

// copy ceiling on the pipelines' engine pair (cloudsc_pipeline.hip)
int pcie_engine_gbps(int device, size_t nb, int reps, double* h2d, double* d2h, double* both);

// ---------------------------------------------------------------------------
// plumbing shared by cloudsc_state.hip and cloudsc_compare.hip
// ---------------------------------------------------------------------------
// Double-double accumulation of non-negative terms (Knuth's TwoSum, then a
// renormalisation): hi + lo carries the sum to ~100 bits, so partial sums
// combined in any grouping -- NPROMA blocks here, shards or ranks on the host --
// round to the same double unless the exact sum lies within ~2^-100 of a
// rounding midpoint.  No FMA contraction applies (-ffp-contract=off),
// and nothing here is reassociated (no fast-math).
struct DD {
  double hi, lo;
};
__host__ __device__ __forceinline__ DD dd_add(DD a, DD b) {
  const double s = a.hi + b.hi;
  const double bb = s - a.hi;
  const double e = (a.hi - (s - bb)) + (b.hi - bb);   // TwoSum error of a.hi + b.hi
  const double t = e + (a.lo + b.lo);
  const double hi = s + t;
  return {hi, t - (hi - s)};                          // FastTwoSum renormalisation
}

}  // namespace cloudsc_impl

#define HIPCHK(call)                                                \
  do {                                                              \
    hipError_t e_ = (call);                                         \
    if (e_ != hipSuccess) return cloudsc_impl::hip_fail(e_, #call); \
  } while (0)
